"""The windows the prompt-statistics tests share (tests/test_timellm_prompt_ref.py on the CPU, tests/test_gpu_timellm_prompt.py on the
GPU), generated from fixed seeds, with their float64 statistics (tests/timellm_prompt_ref.py) computed once.

Shapes (B, L, C, top_k): (1, 1, 1, 3) L = 1: empty diff, lags padded past L; (3, 2, 1, 5); (4, 16, 3, 3) the golden's shape;
(5, 32, 8, 5) cfg5; (2, 33, 5, 5) odd L, no unpaired middle lag; (2, 257, 2, 7) one past a 256-thread workgroup's row per thread;
(1, 64, 64, 5) widest C; (1, 2048, 8, 5) the L limit with the tile at its 64 KB limit.

B counts the ORDINARY windows: an AR(1) series (phi 0.8, so the autocorrelation decays by lag and the largest lags are far apart) plus a
ramp whose sign alternates by window (both trends occur).  Every case carries three SPECIAL windows behind them:
  constant     every element 0.75: every comparison a tie, trend exactly 0, lags [0, 1, 2, ...]
  signed zero  data * mask with negative data and channel 0 fully masked (all -0.0); with C >= 2 channel 1 is masked too and its first
               data element positive, so the channel is +0.0 followed by -0.0: the lowest-index rule decides min, max and median
  nan          an ordinary window with one NaN in its last channel

Asserted HERE, at import, on the CPU -- the conditions that make the GPU comparisons meaningful:
  * every ordinary window with L > 1 has |trend64| >= 1e-2 max|x| (at L == 1 the trend is the empty sum, 0, on every path), so the
    fp32 sequential sum (error <= L^2 2^-23 max|x| only when that is far smaller; the sign test is made where it is) has its sign;
  * the distinct corr64[tau], tau <= L // 2, around the selection boundary -- the classes {tau, L - tau} the list takes and the first it
    leaves out -- are at least 1e-3 corr64[0] apart.  The fp32 direct sum is off by at most about L 2^-24 C corr[0] (1.2e-4 at L 2048),
    so the reference alone decides the order."""
import numpy as np
import torch

import timellm_prompt_ref as R

PHI = 0.8
SHAPES = [(1, 1, 1, 3), (3, 2, 1, 5), (4, 16, 3, 3), (5, 32, 8, 5), (2, 33, 5, 5), (2, 257, 2, 7), (1, 64, 64, 5), (1, 2048, 8, 5)]
SEEDS = {(1, 1, 1, 3): 1, (3, 2, 1, 5): 1, (4, 16, 3, 3): 1, (5, 32, 8, 5): 1, (2, 33, 5, 5): 1, (2, 257, 2, 7): 1, (1, 64, 64, 5): 1,
         (1, 2048, 8, 5): 1}
ORDINARY, CONSTANT, SIGNED_ZERO, NAN = "ordinary", "constant", "signed_zero", "nan"
TREND_MARGIN, CORR_GAP = 1e-2, 1e-3


def ordinary_windows(n, L, C, seed):
    """(n, L, C) float32: AR(1) at its stationary variance plus a ramp of alternating sign"""
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(n, L, C, generator=g, dtype=torch.float64).numpy()
    x = np.empty_like(e)
    x[:, 0] = e[:, 0] / np.sqrt(1.0 - PHI * PHI)
    for t in range(1, L):
        x[:, t] = PHI * x[:, t - 1] + e[:, t]
    ramp = np.linspace(-1.0, 1.0, L) if L > 1 else np.zeros(1)
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    return (x + sign[:, None, None] * ramp[None, :, None]).astype(np.float32)


def build(shape, seed):
    """x (B + 3, L, C) float32 and the kind of every window"""
    B, L, C, _ = shape
    o = ordinary_windows(B + 2, L, C, seed)
    const = np.full((1, L, C), 0.75, np.float32)
    data, mask = -np.abs(o[B:B + 1]) - 0.5, np.ones((1, L, C), np.float32)
    mask[0, :, 0] = 0.0
    if C >= 2:
        mask[0, :, 1] = 0.0
        data[0, 0, 1] = 0.5
    nan = o[B + 1:B + 2].copy()
    nan[0, L // 3, C - 1] = np.nan
    x = np.concatenate([o[:B], const, data * mask, nan], axis=0)
    return np.ascontiguousarray(x), [ORDINARY] * B + [CONSTANT, SIGNED_ZERO, NAN]


def boundary_gap(x, top_k):
    """the smallest gap, relative to corr64[0], between consecutive distinct half-correlations from the largest down to the first class
    the selection leaves out (inf when every class is taken)"""
    L = x.shape[0]
    h = R.half_corr64(x)
    order = np.argsort(-h, kind="stable")
    taken, n_cls = 0, 0
    while taken < min(top_k, L) and n_cls < len(order):
        tau = int(order[n_cls])
        taken += 1 if tau == 0 or 2 * tau == L else 2
        n_cls += 1
    v = h[order[:n_cls + 1]]
    return float(np.min(-np.diff(v)) / h[0]) if len(v) > 1 else float("inf")


def trend_margin(x):
    return abs(float(np.diff(x.astype(np.float64), axis=0).sum(axis=0).mean())) / float(np.abs(x).max())


def meaningful(shape, x, kinds):
    """the two import-time conditions over a case's ordinary windows"""
    _, L, _, top_k = shape
    for b, kind in enumerate(kinds):
        if kind != ORDINARY:
            continue
        if L > 1 and trend_margin(x[b]) < TREND_MARGIN:
            return False
        if boundary_gap(x[b], top_k) < CORR_GAP:
            return False
    return True


class Case:
    def __init__(self, shape):
        self.shape = shape
        self.B, self.L, self.C, self.top_k = shape
        self.x, self.kinds = build(shape, SEEDS[shape])
        assert meaningful(shape, self.x, self.kinds), f"case {shape}: seed {SEEDS[shape]} leaves a trend or a lag gap inside fp32 rounding"
        self.stats64, self.lags64 = R.batch_stats64(self.x, self.top_k)      # computed once, read-only
        self.stats64.setflags(write=False)
        self.lags64.setflags(write=False)
        self.x.setflags(write=False)
        self.ordinary = [b for b, k in enumerate(self.kinds) if k == ORDINARY]

    def window(self, kind):
        return self.kinds.index(kind)


CASES = [Case(s) for s in SHAPES]
IDS = ["B{}_L{}_C{}_k{}".format(*s) for s in SHAPES]
