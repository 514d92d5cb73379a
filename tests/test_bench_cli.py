"""bench.py argument contract (the driver runs `bench.py --gpus N --steps K --warmup W`,
N > 1 under torch.distributed.run): the batch is resolved before either path runs."""
import pytest

import bench


def test_default_is_config2_batch256():
    a = bench.parse_args([])
    assert (a.config, a.batch, a.gpus) == (2, 256, 1)


def test_driver_multi_gpu_args_resolve_batch():
    a = bench.parse_args(["--gpus", "8", "--steps", "50", "--warmup", "10"])
    assert a.batch == 256 and a.steps == 50 and a.warmup == 10


def test_config3_batch4096():
    assert bench.parse_args(["--config", "3"]).batch == 4096


def test_plain_run_times_steps_once_and_nothing_else():
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not a.full and a.windows == 1 and a.dump_outputs is None
    assert a.no_cpu_baseline and a.no_roofline and a.no_trainer_loop
    assert bench.parse_args(["--steps", "20", "--windows", "7"]).windows == 7


def test_full_run_keeps_the_windows_and_the_extra_measurements():
    a = bench.parse_args(["--full", "--steps", "20", "--warmup", "5"])
    assert a.full and a.windows == 100
    assert not (a.no_cpu_baseline or a.no_roofline or a.no_trainer_loop)
    assert bench.parse_args(["--full"]).windows == 10
    assert bench.parse_args(["--full", "--no-roofline"]).no_roofline


def test_dump_outputs_writes_float_arrays_within_the_limit(tmp_path):
    import numpy as np
    arrays = {"losses": np.arange(6, dtype=np.float32).reshape(2, 3),
              "w": np.arange(1000, dtype=np.float32), "n": np.array([3], np.int64),
              "log_alpha": np.array([0.5])}
    n = bench.dump_outputs(str(tmp_path / "a"), arrays)
    assert n == {"losses": 6, "w": 1000, "n": 1, "log_alpha": 1}
    for k, v in arrays.items():
        z = np.load(tmp_path / "a" / f"{k}.npy")
        assert z.dtype == (np.float32 if v.dtype == np.float32 else np.float64)
        assert z.shape == v.shape and np.array_equal(z, v)
    # over the limit: the small arrays whole (none written empty), the same fixed sample of
    # the large one on every run
    n = bench.dump_outputs(str(tmp_path / "b"), arrays, max_bytes=2048)
    bench.dump_outputs(str(tmp_path / "c"), arrays, max_bytes=2048)
    assert n == {"losses": 6, "w": 502, "n": 1, "log_alpha": 1}
    size = 0
    for k, v in arrays.items():
        z = np.load(tmp_path / "b" / f"{k}.npy")
        size += z.nbytes
        assert z.size == n[k] and np.all(np.isin(z, v.astype(np.float64)))
        assert np.array_equal(z, np.load(tmp_path / "c" / f"{k}.npy"))
        if k != "w":
            assert np.array_equal(z, v)
    assert size <= 2048
    w = np.load(tmp_path / "b" / "w.npy")
    assert np.all(np.diff(w) > 0)                      # sorted flat indices, no repeats


@pytest.mark.parametrize("steps,upl", [(1, 20), (20, 20), (23, 20), (4080, 20), (4096, 20),
                                       (4097, 20), (9000, 20), (100000, 20), (5000, 256),
                                       (8193, 1), (4103, 20)])
def test_any_number_of_steps_is_fetched_within_the_loss_ring(steps, upl):
    """The library keeps the last LOSS_RING updates' losses: a window of any length fetches
    them in chunks of whole launches no longer than that, and launches what one run of
    `steps` updates launches."""
    chunks = bench.fetch_chunks(steps, upl)
    assert sum(chunks) == steps and all(0 < c <= bench.LOSS_RING for c in chunks)
    assert all(c % upl == 0 for c in chunks[:-1])
    assert sum((bench.launches(c, upl) for c in chunks), []) == bench.launches(steps, upl)
    assert set(bench.launches(steps, upl)) == set(bench.graph_sizes(steps, upl))
    if steps <= bench.LOSS_RING // upl * upl:
        assert chunks == [steps]                       # one fetch, at the window's end


def test_untimed_launches_before_the_first_window():
    assert bench.untimed_launches(23, 2, 20) == [3, 20, 2] + bench.SETTLE_PASSES * [20, 3]
    assert bench.untimed_launches(20, 45, 20) == [20, 20, 20, 5] + bench.SETTLE_PASSES * [20]
    assert bench.untimed_launches(7, 0, 20) == [7] + bench.SETTLE_PASSES * [7]


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(tmp_path):
    """A plain run end to end at a small replay, with a window longer than the loss ring
    (4103 updates: two fetches, launches of 20 and 3): the line's headline fields, null
    where --full would measure, and the dump.  The dumped losses, parameters and log_alpha
    are bit for bit those of a context that this process sets up with the same seeds and
    steps through the same launches, read right after the last timed update — so they are
    the state after that update, and a run in another process with the same arguments
    computes the same files."""
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    from sacmi import Config, Context
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "dump"
    N, W, FILL = 4103, 2, 4096
    argv = ["--gpus", "1", "--steps", str(N), "--warmup", str(W), "--fill", str(FILL)]
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + argv +
                       ["--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == N and d["warmup"] == W and d["windows"] == 1 and d["full"] is False
    assert d["unit"] == "grad-steps/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 1) < 1e-2
    assert abs(d["window_ms_min_med_max"][1] / N - d["ms_per_step"]) < 1e-3
    for k in ("roofline", "cpu_baseline", "trainer_loop", "trainer_loop_faithful",
              "one_update_per_launch_steps_per_s", "api_faithful_steps_per_s"):
        assert d[k] is None, k
    files = sorted(os.listdir(out))
    assert "losses.npy" in files and "log_alpha.npy" in files and len(files) == 2 + 8 + 4 * 6
    total = 0
    for f in files:
        z = np.load(out / f)
        total += z.nbytes
        assert z.dtype in (np.float32, np.float64) and np.all(np.isfinite(z)), f
    assert total <= bench.DUMP_MAX_BYTES
    assert np.load(out / "losses.npy").shape == (N, 3)

    # the same inputs and launches in this process (bench.main's set-up)
    args = bench.parse_args(argv)
    wl = bench.workload(args)
    ctx = Context(Config(wl["S"], wl["A"], wl["H"], max_batch=args.batch, capacity=FILL, seed=1,
                         replay=wl["replay"], n_hidden=wl["n_hidden"],
                         compute_dtype=wl["dtype"]), 0)
    bench.init_agent(ctx, 0)
    ctx.push(*bench.synth(FILL, 1000, wl["S"], wl["A"]))
    upl = args.updates_per_launch
    for k in bench.untimed_launches(N, W, upl):
        ctx.step_many_async(args.batch, k)
    rows = []
    for c in bench.fetch_chunks(N, upl):
        for k in bench.launches(c, upl):
            ctx.step_many_async(args.batch, k)
        rows.append(ctx.fetch_losses(c))
    want = bench.final_outputs(ctx, np.concatenate(rows))
    ctx.close()
    assert sorted(k + ".npy" for k in want) == files
    for k, v in want.items():
        assert np.array_equal(np.load(out / f"{k}.npy"), v), k
    assert want["losses"].shape == (N, 3) and len({tuple(x) for x in want["losses"]}) > N // 2
    assert np.any(want["q1.fc1.bias"] != 0)                # zero at init (bench.init_agent)
    assert want["log_alpha"][0] != 0.0


def test_roofline_scales_out_the_instrumentation(monkeypatch):
    """The roofline's level durations come from the instrumented replay; they are scaled by
    the uninstrumented graph's time per update over the instrumented one (never up)."""
    info = dict(graph_us=2400.0, sum_us=2400.0, allreduce_us=0.0, n_updates=20, gemm_us=2000.0,
                gemm_flops=20 * 3.2e9, gemm_bytes=20 * 11 * 7.6e6, levels=220,
                kernel_launches={"k_gemm": 220}, achieved_tflops=20 * 3.2e9 / 2000e-6 / 1e12,
                sites_us={})
    monkeypatch.setattr(bench, "timeline_roofline", lambda *a, **k: dict(info))
    monkeypatch.setattr(bench, "pmc_counters", lambda *a, **k: None)
    args = bench.parse_args([])
    wl = {"dtype": "fp32"}
    r = bench.roofline_object(None, args, wl, 157.3, step_us_real=114.0)
    assert abs(r["instrumentation_scale"] - 114.0 / 120.0) < 1e-4
    assert abs(r["gemm_us_per_step"] - 100.0 * 114.0 / 120.0) < 0.01
    assert abs(r["achieved"] - 3.2e9 / (95e-6) / 1e12) < 0.01
    assert abs(r["achieved_timeline_raw"] - 32.0) < 1e-3
    r = bench.roofline_object(None, args, wl, 157.3, step_us_real=130.0)   # slower: no scaling up
    assert r["instrumentation_scale"] == 1.0 and abs(r["achieved"] - 32.0) < 1e-3


def test_pmc_figures_only_for_the_sources_they_were_measured_on(tmp_path, monkeypatch):
    import json
    import os
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import pmc_summary  # noqa: F401  (the real tools module, before ROOT moves)
    (tmp_path / "profiles").mkdir()
    z = {"csrc_digest": "0" * 16, "per_level": {"traffic_bytes": 1.0, "mfma_busy": 0.5}}
    (tmp_path / "profiles" / "pmc_c2.json").write_text(json.dumps(z))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench.pmc_counters(2) is None                 # stale digest: no counters
    z["csrc_digest"] = pmc_summary.csrc_digest(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    (tmp_path / "profiles" / "pmc_c2.json").write_text(json.dumps(z))
    monkeypatch.setattr(pmc_summary, "csrc_digest", lambda root=None: z["csrc_digest"])
    assert bench.pmc_counters(2)["per_level"]["mfma_busy"] == 0.5
