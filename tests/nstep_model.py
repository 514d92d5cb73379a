"""Host model of the n-step gather (sacmi_set_nstep; csrc/nstep.hip, include/sacmi.h): numpy
fp32 with exactly the device's roundings, a brute-force fp64 return to hold it against, the ring
fixture of the GPU tests and the rows of a one-step ring that collapse to the same minibatch.
"""
import numpy as np

NMAX = 32


def g_table(gamma):
    """g[j] = float32(gamma ** j) from fp64, rounded once; g[0] = 1."""
    return np.array([np.float64(gamma) ** j for j in range(NMAX)], np.float64).astype(np.float32)


def nstep_rows(rew, done, ep_end, head, length, capacity, n, gamma, idx, by_slot=False):
    """The gather's (m, R, d', slot of s2) for sampled rows `idx` (deque positions, or ring slots
    with by_slot).  rew, done: float32 [capacity] as stored (done raw: != 0 is terminal), ep_end:
    [capacity] flags.  R, d' float32 with the device's roundings: every product and every sum
    rounded on its own, in the order j = 1..m."""
    assert 1 <= n <= NMAX and 1 <= length <= capacity
    rew = np.asarray(rew, np.float32)
    done = np.asarray(done, np.float32)
    g = g_table(gamma)
    idx = np.asarray(idx, np.int64).reshape(-1)
    ms, Rs, ds, slots = [], [], [], []
    for ix in idx:
        p0 = int(ix) if by_slot else (head + int(ix)) % capacity
        i = (p0 - head + capacity) % capacity if by_slot else int(ix)
        assert 0 <= i < length
        jmax = min(n - 1, length - 1 - i)
        m = jmax
        for j in range(jmax + 1):
            p = (p0 + j) % capacity
            if done[p] != 0 or ep_end[p]:
                m = j
                break
        R = np.float32(rew[p0])
        for j in range(1, m + 1):
            R = np.float32(R + np.float32(g[j] * rew[(p0 + j) % capacity]))
        pm = (p0 + m) % capacity
        if done[pm] != 0:
            d = np.float32(1)
        elif m == 0:
            d = np.float32(0)
        else:
            d = np.float32(np.float32(1) - g[m])
        ms.append(m); Rs.append(R); ds.append(d); slots.append(pm)
    return (np.array(ms, np.int64), np.array(Rs, np.float32), np.array(ds, np.float32),
            np.array(slots, np.int64))


def coefficient(d, gamma):
    """What the unchanged row algebra makes of d': fl(fl(1 - d') * (float)gamma), float32."""
    d = np.asarray(d, np.float32)
    return ((np.float32(1) - d).astype(np.float32) * np.float32(gamma)).astype(np.float32)


def brute_force(rew, done, ep_end, head, length, capacity, n, gamma, i):
    """fp64, by the definition, for deque position i: (m, R64, sum |g_j r_j|, gamma^(m+1) or 0
    behind a terminal)."""
    p0 = (head + i) % capacity
    R, A, m = 0.0, 0.0, 0
    for j in range(n):
        p = (p0 + j) % capacity
        R += float(gamma) ** j * float(rew[p])
        A += abs(float(gamma) ** j * float(rew[p]))
        m = j
        if done[p] != 0 or ep_end[p] or i + j == length - 1:
            break
    term = done[(p0 + m) % capacity] != 0
    return m, R, A, 0.0 if term else float(gamma) ** (m + 1)


class Ring:
    """A host mirror of the replay ring's reward / done / flag arrays under deque(maxlen) pushes
    (flags written for every stored row, as the device does while n-step is on)."""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.rew = np.zeros(capacity, np.float32)
        self.done = np.zeros(capacity, np.float32)
        self.ep_end = np.zeros(capacity, np.uint8)
        self.row = np.full(capacity, -1, np.int64)      # which pushed row a slot holds
        self.wpos = 0
        self.length = 0
        self.pushed = 0

    @property
    def head(self):
        return 0 if self.length < self.capacity else self.wpos

    def push(self, r, d, end=None):
        r = np.asarray(r, np.float32).reshape(-1)
        d = np.asarray(d).reshape(-1)
        end = np.zeros(len(r), np.uint8) if end is None else np.asarray(end).reshape(-1)
        for k in range(len(r)):
            self.rew[self.wpos] = r[k]
            self.done[self.wpos] = 1.0 if d[k] else 0.0
            self.ep_end[self.wpos] = 1 if end[k] else 0
            self.row[self.wpos] = self.pushed
            self.pushed += 1
            self.wpos = (self.wpos + 1) % self.capacity
            self.length = min(self.capacity, self.length + 1)
        return self

    def mark_episode_end(self):
        self.ep_end[(self.wpos - 1) % self.capacity] = 1

    def rows(self, n, gamma, idx, by_slot=False):
        return nstep_rows(self.rew, self.done, self.ep_end, self.head, self.length, self.capacity,
                          n, gamma, idx, by_slot)


LONG, TAIL = 33, 5      # a stretch without any mark, longer than the largest n, and what follows
# (length, how the episode's last row is marked): a terminal, a flag-only end (done 0), both at
# once, or nothing at all (the chain runs on into the next episode's rows)
EPISODES = ((2, "T"), (3, "F"), (1, "B"), (4, "."), (5, "T"), (6, "F"), (7, "B"), (8, "."), (9, "T"))


def fixture_marks(n_rows):
    """(done, episode_end) of the GPU tests' fixture, laid out from the newest row backwards so
    that every ring capacity sees the same window: TAIL unmarked rows, a stretch of LONG rows
    without marks (a window of 32 fits), then episodes of lengths 1..9 (EPISODES, repeating)."""
    done = np.zeros(n_rows, np.uint8)
    end = np.zeros(n_rows, np.uint8)
    last, k = n_rows - TAIL - LONG - 1, 0         # the last row of the episode being laid
    while last >= 0:
        length, kind = EPISODES[k % len(EPISODES)]
        done[last] = kind in "TB"
        end[last] = kind in "FB"
        last -= length
        k += 1
    return done, end


CATEGORIES = ("full n", "terminal inside", "flag inside", "newest", "wraps", "m == 0")


def categories(ring, n, gamma, idx, by_slot=False):
    """name -> how many of the sampled rows fall in each category (not exclusive)."""
    m, R, d, sl = ring.rows(n, gamma, idx, by_slot)
    idx = np.asarray(idx, np.int64)
    p0 = idx if by_slot else (ring.head + idx) % ring.capacity
    i = (p0 - ring.head + ring.capacity) % ring.capacity
    marked_t = ring.done[sl] != 0
    marked_f = (ring.ep_end[sl] != 0) & ~marked_t
    plain = ~marked_t & ~marked_f
    return {"full n": int(np.sum((m == n - 1) & plain)),
            "terminal inside": int(np.sum(marked_t & (m > 0))),
            "flag inside": int(np.sum(marked_f & (m > 0))),
            "newest": int(np.sum((m == ring.length - 1 - i) & plain & (m < n - 1))),
            "wraps": int(np.sum((p0 + m >= ring.capacity) & (m > 0))),
            "m == 0": int(np.sum(m == 0))}


def collapsed_rows(ring, n, gamma, s, a, s2):
    """The one-step ring that gathers to the same minibatch: for every stored deque position i
    (oldest first) the row (s_i, a_i, R_i, s2 of p_m, done = d' != 0) and the raw d'_i.  s, a, s2
    are indexed by pushed row number."""
    idx = np.arange(ring.length)
    m, R, d, sl = ring.rows(n, gamma, idx)
    first = ring.row[(ring.head + idx) % ring.capacity]
    last = ring.row[sl]
    return (s[first], a[first], R, s2[last], (d != 0).astype(np.uint8)), d
