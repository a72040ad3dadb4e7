"""TEST INFRASTRUCTURE: the fixed reduction order of csrc/reduce.hpp as a numpy transcription,
shared by tests/test_gpu_reduce_order.py (which pins the kernels to it) and tests/lsqr_model.py.

  1. thread t of workgroup b of a grid of G workgroups of NT threads adds the entries
     b*NT + t + m*G*NT, m ascending, to an accumulator that starts at +0.0;
  2. the 64-lane xor butterfly, offsets 32 .. 1, by lane index;
  3. the NT/64 wave totals added left to right;
  4. one workgroup sums the G partials: thread t takes the partials t, t + NT, .. in that order
     (strided_sum), then 2 and 3 again.
"""
import numpy as np

LANE = np.arange(64)


def thread_sums(vals, G, NT):
    """Step 1 (and strided_sum, with G = 1): the (G, NT) per-thread sums of `vals`."""
    n, W = len(vals), G * NT
    M = max(1, -(-n // W))
    pad = np.zeros(M * W)
    pad[:n] = vals
    live = np.arange(M * W) < n
    s = np.zeros(W)  # +0.0
    for m in range(M):
        sl = slice(m * W, (m + 1) * W)
        s = np.where(live[sl], s + pad[sl], s)
    return s.reshape(G, NT)


def wave_totals(s):
    """Step 2 on (G, NT) thread sums: (G, NT / 64) wave totals."""
    v = s.reshape(s.shape[0], -1, 64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., LANE ^ off]
    assert np.array_equal(v, np.broadcast_to(v[..., :1], v.shape))  # every lane holds the total
    return v[..., 0]


def block_totals(s):
    """Steps 2 and 3: one total per workgroup."""
    w = wave_totals(s)
    t = w[:, 0].copy()
    for i in range(1, w.shape[1]):
        t = t + w[:, i]
    return t


def partials_total(p, NT):
    """Step 4."""
    return block_totals(thread_sums(p, 1, NT))[0]


def grid(n, cap):
    return min(cap, max(1, -(-n // 256)))


def sumsq_ref(x):
    """mlamg_norm2's sum of squares: grid capped at 1024, finished by 1024 threads."""
    return partials_total(block_totals(thread_sums(x * x, grid(len(x), 1024), 256)), 1024)


def sum_ref(x):
    """mlamg_remove_mean's sum: the fixed 512-workgroup grid, finished by 256 threads."""
    return partials_total(block_totals(thread_sums(x, 512, 256)), 256)


def remove_mean_ref(x):
    return x - sum_ref(x) / float(len(x))


def ill_scaled(n, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal(n) * 10.0 ** rs.uniform(-3, 3, n)
