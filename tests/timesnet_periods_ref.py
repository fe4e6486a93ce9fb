"""Float64 restatement, in plain torch on the CPU, of TimesNet's period-on-the-device operators (csrc/conv.hip: period_rows, conv2d_periods,
period_aggregate), written from models/TimesNet.py:76-91 and the layout comments of csrc/conv.hip -- not from the kernels.  Images are
"position-major": row l * B + b of a (Lmax * B, C) matrix is position l of window b, so an image of any length is a prefix of one buffer.
tests/test_timesnet_periods_ref.py pins it to layers.Conv_Blocks.Inception_Block_V1 and to TimesBlock(cfg).double() on the CPU;
tests/test_gpu_timesnet_periods.py holds the kernels to it."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def period_rows_ref(top, total, B):
    """top: k frequency indices -> (period int32 (k), rows int32 (k)): period = total // f (f == 0 -> total, the kernel's documented guard),
    rows = B * (total rounded up to a multiple of the period)   (models/TimesNet.py:76-81)"""
    period, rows = [], []
    for f in np.asarray(top).reshape(-1).tolist():
        p = total // f if f > 0 else total
        length = total if total % p == 0 else (total // p + 1) * p
        period.append(p)
        rows.append(length * B)
    return np.asarray(period, dtype=np.int32), np.asarray(rows, dtype=np.int32)


def merged_kernel(weights, biases):
    """the mean of n same-padded convolutions with kernel sizes 1, 3, .., 2n-1 as ONE kernel: the mean of the kernels zero-padded to the
    largest size, in the operators' layout W_eff (Cout, KS*KS*Cin), tap-major and channel-minor; b_eff the mean bias.  -> (W_eff, b_eff, KS)"""
    n = len(weights)
    KS = 2 * n - 1
    padded = [F.pad(w, (n - 1 - i,) * 4) for i, w in enumerate(weights)]        # (Cout, Cin, KS, KS) each
    W = torch.stack(padded).mean(0)
    return W.permute(0, 2, 3, 1).reshape(W.shape[0], -1), torch.stack(list(biases)).mean(0), KS


def conv_periods_ref(x, periods, Weff, beff, KS, B, Lmax, act, rows=None):
    """x: (Lmax*B, Cin) shared by every image or (k, Lmax*B, Cin), float64, position-major.  Image j is the first rows[j] = length_j * B rows
    seen as (B, Cin, length_j / p_j, p_j); rows defaults to period_rows' for a series of Lmax // 2 steps (TimesBlock: Lmax = 2 total).
    -> (y (k, Lmax*B, Cout) with zeros beyond each image, valid (k, Lmax*B) bool).  act: None or "gelu" (exact erf)."""
    periods = [int(p) for p in np.asarray(periods).reshape(-1)]
    k, R = len(periods), Lmax * B
    if rows is None:
        total = Lmax // 2
        rows = [-(-total // p) * p * B for p in periods]
    rows = [int(r) for r in np.asarray(rows).reshape(-1)]
    Cout, Cin = Weff.shape[0], x.shape[-1]
    assert x.dtype == torch.float64 and Weff.shape[1] == KS * KS * Cin and x.shape[-2] == R
    W = Weff.reshape(Cout, KS, KS, Cin).permute(0, 3, 1, 2)
    ys = []
    valid = torch.zeros(k, R, dtype=torch.bool)
    for j, (p, r) in enumerate(zip(periods, rows)):
        length = r // B
        assert r == length * B and length % p == 0 and r <= R
        xj = x if x.dim() == 2 else x[j]
        img = xj[:r].reshape(length, B, Cin).permute(1, 2, 0).reshape(B, Cin, length // p, p)
        o = F.conv2d(img, W, beff, padding=KS // 2)
        if act == "gelu":
            o = 0.5 * o * (1.0 + torch.erf(o / math.sqrt(2.0)))
        else:
            assert act is None
        o = o.reshape(B, Cout, length).permute(2, 0, 1).reshape(r, Cout)
        ys.append(F.pad(o, (0, 0, 0, R - r)))
        valid[j, :r] = True
    return torch.stack(ys), valid


def period_aggregate_ref(Y, w, x, B, total, Lmax):
    """out[b, t, :] = x[b, t, :] + sum_j w[b, j] Y[j, t B + b, :],  t < total   (Y (k, Lmax*B, N), w (B, k), x (B, total, N))"""
    k, _, N = Y.shape
    Yc = Y.reshape(k, Lmax, B, N)[:, :total].permute(2, 1, 3, 0)               # (B, total, N, k)
    return x + (Yc * w.reshape(B, 1, 1, k)).sum(-1)


def spectral_batch(B, total, N, freqs, amps, seed):
    """(B, total, N) float32 whose spectrum has len(freqs) clean lines: integer cycle counts over `total`, strictly decreasing amplitudes,
    a random phase per (line, window, channel) on a cosine (a Nyquist line keeps |cos phase| of its amplitude), 1 % noise"""
    assert len(freqs) == len(amps) and all(a > b for a, b in zip(amps[:-1], amps[1:]))
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(total, dtype=torch.float64).view(1, total, 1)
    x = torch.zeros(B, total, N, dtype=torch.float64)
    for f, a in zip(freqs, amps):
        phase = 2 * math.pi * torch.rand(B, 1, N, generator=g, dtype=torch.float64)
        x = x + a * torch.cos(2 * math.pi * f * t / total + phase)
    x = x + 0.01 * torch.randn(B, total, N, generator=g, dtype=torch.float64)
    return x.float()


def spectrum_topk(x, k):
    """the float64 period selection of models/TimesNet.py FFT_for_Period: (top (k) frequency indices by mean amplitude, the mean-amplitude
    spectrum with its constant term zeroed, the per-window weights (B, k))"""
    amp = torch.fft.rfft(x.double(), dim=1).abs()
    freq = amp.mean(0).mean(-1)
    freq[0] = 0
    top = torch.topk(freq, k).indices
    return top, freq, amp.mean(-1)[:, top]


# the spectral batches of the GPU tests' whole-block configurations: name -> (B, total, N, freqs, amps, seed)
BLOCK_BATCHES = {
    "a": (3, 30, 8, (1, 2, 4, 7, 15), (1.0, 0.7, 0.5, 0.35, 0.2), 11),
    "b": (3, 30, 8, (1, 2, 4, 7, 15), (1.0, 0.7, 0.5, 0.35, 0.2), 11),
    "c": (2, 66, 8, (1, 3, 11, 33), (1.0, 0.7, 0.5, 0.3), 12),
}


def timesblock_ref(x, top, weight, blocks, B, total):
    """a TimesBlock composed from the three operators above: x (B, total, N) float64, top / weight from spectrum_topk, blocks = the two
    Inception blocks' ((weights), (biases)) -> (B, total, N)"""
    Lmax = 2 * total
    N = x.shape[-1]
    period, rows = period_rows_ref(top, total, B)
    xl = F.pad(x.transpose(0, 1), (0, 0, 0, 0, 0, Lmax - total)).reshape(Lmax * B, N)
    W1, b1, K1 = merged_kernel(*blocks[0])
    W2, b2, K2 = merged_kernel(*blocks[1])
    img, _ = conv_periods_ref(xl, period, W1, b1, K1, B, Lmax, "gelu", rows=rows)
    out, _ = conv_periods_ref(img, period, W2, b2, K2, B, Lmax, None, rows=rows)
    return period_aggregate_ref(out, F.softmax(weight, dim=1), x, B, total, Lmax)
