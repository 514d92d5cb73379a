"""CPU checks of the observation-normalisation contract (include/sacmi.h): the
six functions are declared, exported and bridged; and the host model (tests/obs_norm_model.py)
of the chunked fp64 running moments, the derived fp32 vectors and the fp32 normalise expression
agrees with exact rational arithmetic on a fixture built to break a careless implementation
(a column at 4096 with a spread of 0.01, a constant, a tiny and a huge column).

Bounds (the model's own error, measured on this fixture, is about 100x below them): M2 within
1e-9 relative, the mean within 1e-12 of max|x_k|, both fp32 vectors within 1 ulp.  The
E[x^2] - mean^2 form in fp64 is kept as the control that must miss the M2 bound."""
import os
import re
import subprocess

import numpy as np
import pytest

from obs_norm_model import (CUTS, NaiveMoments, RunningMoments, exact_vectors, fixture_exact,
                            fixture_rows, moment_errors, normalize, ulp32, vectors)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sacmi.h")
LIB = os.path.join(ROOT, "humanoid-walking-with-sac_amd", "sacmi", "libsacmi.so")
FUNCS = ("sacmi_set_obs_norm", "sacmi_obs_norm", "sacmi_obs_norm_update",
         "sacmi_obs_norm_get_moments", "sacmi_obs_norm_set_moments", "sacmi_obs_norm_get_vectors")
M2_RTOL, MEAN_RTOL, EPS = 1e-9, 1e-12, 1e-8


def test_abi_declares_exports_and_bridges_the_six_functions():
    text = open(HEADER).read()
    declared = set(re.findall(r"^\s*int\s+(sacmi_\w+)\s*\(", text, re.M))
    assert not [f for f in FUNCS if f not in declared]
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (sacmi_\w+)", out))
    assert not [f for f in FUNCS if f not in exported]
    from sacmi import _lib as L
    assert not [f for f in FUNCS if f not in L.EXPORTS]


def run_model(form):
    x = fixture_rows()
    m = RunningMoments(x.shape[1], form)
    for lo, hi in zip(CUTS[:-1], CUTS[1:]):
        m.update(x[lo:hi])
    return m


@pytest.mark.parametrize("form", ["chan", "welford", "device"])
def test_chunked_moments_match_exact_arithmetic(form):
    x = fixture_rows()
    m = run_model(form)
    assert m.count == len(x)
    e_m2, e_mean = moment_errors(m.count, m.mean, m.m2, x, fixture_exact())
    print(f"{form}: M2 {e_m2:.2e} relative, mean {e_mean:.2e} of max|x|")
    assert e_m2 <= M2_RTOL and e_mean <= MEAN_RTOL
    assert m.m2[5] == 0.0 and m.mean[5] == -2.5          # the constant column, exactly
    nmean, nrstd = vectors(m.count, m.mean, m.m2, EPS)
    want_mean, want_rstd = exact_vectors(*fixture_exact(), EPS)
    u = max(ulp32(nmean, want_mean).max(), ulp32(nrstd, want_rstd).max())
    print(f"{form}: vectors {u:.1f} ulp")
    assert u <= 1.0
    assert nrstd[5] == np.float32(1e4)                    # var 0: 1 / sqrt(eps)


def test_sum_of_squares_form_misses_the_bound():
    """The control: fp64 sums of x and x^2 lose column 3 (4096 +- 0.01) to cancellation."""
    x = fixture_rows()
    m = NaiveMoments(x.shape[1])
    for lo, hi in zip(CUTS[:-1], CUTS[1:]):
        m.update(x[lo:hi])
    n, _, em2 = fixture_exact()
    rel3 = abs(m.m2[3] - float(em2[3])) / float(em2[3])
    print(f"naive: column 3 M2 off by {rel3:.2e} relative")
    assert rel3 > 1e3 * M2_RTOL
    _, want_rstd = exact_vectors(*fixture_exact(), EPS)
    assert ulp32(vectors(n, m.mean, m.m2, EPS)[1], want_rstd)[3] > 100


def test_count_zero_is_the_identity():
    m = RunningMoments(5)
    nmean, nrstd = vectors(m.count, m.mean, m.m2, EPS)
    assert np.array_equal(nmean, np.zeros(5, np.float32)) and np.array_equal(nrstd, np.ones(5, np.float32))
    x = np.array([[1.5, -2.0, 0.0, 3e30, -7.25]], np.float32)
    assert np.array_equal(normalize(x, nmean, nrstd, np.inf), x)
    m.update(np.zeros((0, 5), np.float32))                # an empty chunk changes nothing
    assert m.count == 0


def test_normalize_expression_clip_nan_inf():
    nmean = np.array([1.0, 0.0, -2.0, 0.5], np.float32)
    nrstd = np.array([2.0, 1.0, 0.5, 4.0], np.float32)
    x = np.array([[3.0, np.nan, 100.0, 0.5], [-9.0, 0.25, np.inf, -np.inf]], np.float32)
    y = normalize(x, nmean, nrstd, 1.5)
    want = np.array([[1.5, np.nan, 1.5, 0.0], [-1.5, 0.25, 1.5, -1.5]], np.float32)
    assert np.array_equal(y, want, equal_nan=True)
    assert np.isnan(y[0, 1])                              # a NaN is not clamped away
    y = normalize(x, nmean, nrstd, np.inf)                # clip = inf: none
    want = np.array([[4.0, np.nan, 51.0, 0.0], [-20.0, 0.25, np.inf, -np.inf]], np.float32)
    assert np.array_equal(y, want, equal_nan=True)
    # two fp32 roundings: the difference, then the product
    a, mu, rs = np.float32(1.0000001), np.float32(0.33333334), np.float32(3.0000002)
    assert normalize(a, mu, rs, np.inf) == np.float32(np.float32(a - mu) * rs)


def test_nan_row_poisons_its_column_only():
    x = fixture_rows()[:40].copy()
    x[7, 2] = np.nan
    m = RunningMoments(x.shape[1], "device").update(x)
    assert np.isnan(m.mean[2]) and np.isnan(m.m2[2])
    ok = np.arange(x.shape[1]) != 2
    assert np.all(np.isfinite(m.mean[ok])) and np.all(np.isfinite(m.m2[ok]))


def _resource_report(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass", line)
        if not m:
            continue
        f = re.match(r"Function Name: (\S+)", m.group(1))
        if f:
            cur = out.setdefault(f.group(1), [])
        elif cur is not None:
            cur.append(m.group(1))
    return out


def test_recorded_resource_reports_leave_every_existing_kernel_as_it_was():
    """profiles/obs_norm/: `make resources` of the parent commit and of this one.  Every kernel
    of the parent has the same registers, scratch, LDS and occupancy (the parent's k_gather is
    this commit's k_gather<false>), and the new kernels use no scratch."""
    d = os.path.join(ROOT, "profiles", "obs_norm")
    parent = _resource_report(os.path.join(d, "resources_parent.txt"))
    this = _resource_report(os.path.join(d, "resources_this.txt"))
    assert len(parent) > 100
    rename = {"_ZN5sacmi8k_gatherENS_10GatherArgsE": "_ZN5sacmi8k_gatherILb0EJEEEvNS_10GatherArgsEDpT0_"}
    for name, rows in parent.items():
        assert this[rename.get(name, name)] == rows, name
    new = sorted(set(this) - {rename.get(n, n) for n in parent})
    assert len(new) == 4 and all("obs" in n or "k_gatherILb1E" in n for n in new), new
    for n in new:
        assert "ScratchSize [bytes/lane]: 0" in this[n] and "VGPRs Spill: 0" in this[n], n
