"""Float64 restatement, in plain torch on the CPU, of TimesNet's period selection as immtsf.ops.timesnet_spectrum computes it
(csrc/timesnet_spectrum.hip), written from models/TimesNet.py (FFT_for_Period / fft_for_period_device, the softmax and the padded
transpose of TimesBlock.forward) and the formulas of include/immtsf.h -- not from the kernels: an explicit direct DFT, the means, the zeroed
constant term, the top-k with equal values to the lower index, the weights, their softmax, the position-major image, and the analytic
gradient.  tests/test_timesnet_spectrum_ref.py pins it to torch.fft.rfft + autograd in float64; tests/test_gpu_timesnet_spectrum.py holds
the kernels to it.  Also the case table of the GPU tests."""
import functools
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timesnet_periods_ref as P  # noqa: E402


def dft(x):
    """x (B, T, N) float64 -> (Re, Im, cos, sin): Re[b, f, n] = sum_t x cos th_ft, Im = -sum_t x sin th_ft for f = 0..T // 2, th_ft = 2 pi
    ((f t) mod T) / T; cos / sin (F, T) are the tables"""
    assert x.dtype == torch.float64 and x.dim() == 3
    T = x.shape[1]
    f = torch.arange(T // 2 + 1).view(-1, 1)
    t = torch.arange(T).view(1, -1)
    th = 2.0 * math.pi * ((f * t) % T).double() / T
    c, s = torch.cos(th), torch.sin(th)
    return torch.einsum("ft,btn->bfn", c, x), -torch.einsum("ft,btn->bfn", s, x), c, s


def topk_low_index(freq, k):
    """the k largest of a 1-D tensor, descending, equal values to the lower index"""
    v = freq.tolist()
    return sorted(range(len(v)), key=lambda i: (-v[i], i))[:k]


def spectrum_ref(x, k):
    """x (B, T, N) -> dict of float64 / integer results: amp (B, F, N), amp_mean (B, F), freq (F, freq[0] = 0), top (k, list), period / rows
    (k, int32 arrays: period = T // f, T where f == 0; rows = B (T rounded up to a multiple of the period)), weight (B, k), w (B, k),
    xl (2T B, N: row t B + b = x[b, t], zero for t >= T)"""
    x = x.double()
    B, T, N = x.shape
    re, im, _, _ = dft(x)
    amp = torch.sqrt(re * re + im * im)
    amp_mean = amp.mean(-1)
    freq = amp_mean.mean(0)
    freq[0] = 0
    top = topk_low_index(freq, k)
    period = [T // f if f > 0 else T for f in top]
    rows = [B * (-(-T // p) * p) for p in period]
    weight = amp_mean[:, top]
    w = torch.softmax(weight, dim=1)
    xl = torch.cat([x.transpose(0, 1), torch.zeros(T, B, N, dtype=torch.float64)]).reshape(2 * T * B, N)
    return dict(amp=amp, amp_mean=amp_mean, freq=freq, top=top, period=np.asarray(period, dtype=np.int32), rows=np.asarray(rows, dtype=np.int32),
                weight=weight, w=w, xl=xl)


def spectrum_grad_ref(x, k, g_w=None, g_xl=None):
    """the analytic gradient of sum(w g_w) + sum(xl g_xl) in x: dx[b, t, n] = g_xl[t B + b, n] + (1 / N) sum_j gs[b, j] (Re_j cos th_jt -
    Im_j sin th_jt) / amp_j over the k selected frequencies, gs = w (g_w - sum_j g_w w); a term with amp_j == 0 is 0"""
    x = x.double()
    B, T, N = x.shape
    r = spectrum_ref(x, k)
    dx = torch.zeros_like(x)
    if g_xl is not None:
        dx += g_xl.double().reshape(2 * T, B, N)[:T].transpose(0, 1)
    if g_w is not None:
        g_w, w = g_w.double(), r["w"]
        gs = w * (g_w - (g_w * w).sum(1, keepdim=True))                                # (B, k)
        re, im, c, s = dft(x)
        top = r["top"]
        re, im, amp, c, s = re[:, top], im[:, top], r["amp"][:, top], c[top], s[top]   # (B, k, N) x 3, (k, T) x 2
        ure = torch.where(amp > 0, re / amp.clamp(min=1e-300), torch.zeros_like(re))
        uim = torch.where(amp > 0, im / amp.clamp(min=1e-300), torch.zeros_like(im))
        dx += (torch.einsum("bj,bjn,jt->btn", gs, ure, c) - torch.einsum("bj,bjn,jt->btn", gs, uim, s)) / N
    return dx


# ---- the case table of the GPU tests: name -> (B, T, N, k, freqs, amps, seed); inputs are timesnet_periods_ref.spectral_batch with k planted
# lines (a Nyquist line wherever T is even).  "a" and "c" are BLOCK_BATCHES' entries
_A, _C = P.BLOCK_BATCHES["a"], P.BLOCK_BATCHES["c"]
CASES = {
    "a": (_A[0], _A[1], _A[2], len(_A[3]), _A[3], _A[4], _A[5]),                      # (3, 30, 8, 5)
    "c": (_C[0], _C[1], _C[2], len(_C[3]), _C[3], _C[4], _C[5]),                      # (2, 66, 8, 4)
    "one": (1, 7, 1, 1, (2,), (1.0,), 13),                                            # one window, one channel, odd T, F = 4
    "odd": (5, 33, 3, 2, (3, 16), (1.0, 0.6), 14),                                    # odd T, N not a multiple of 4
    "cfg4": (2, 64, 16, 5, (1, 4, 9, 16, 32), (1.0, 0.7, 0.5, 0.35, 0.2), 15),        # cfg4's tile
    "wide": (2, 192, 64, 5, (2, 5, 24, 61, 96), (1.0, 0.7, 0.5, 0.35, 0.2), 16),      # the largest shape the route is required to take
}
# just past the route's limit T N <= 16384 (130 x 128 = 16640): must take the torch path
PAST = ("past", (1, 130, 128, 2, (3, 65), (1.0, 0.5), 17))


@functools.lru_cache(maxsize=None)
def case_input(name):
    """the case's x (B, T, N) float32, on the CPU; shared by the tests, never modified"""
    B, T, N, k, freqs, amps, seed = PAST[1] if name == PAST[0] else CASES[name]
    assert len(freqs) == k
    return P.spectral_batch(B, T, N, freqs, amps, seed)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    k = (PAST[1] if name == PAST[0] else CASES[name])[3]
    return spectrum_ref(case_input(name), k)
