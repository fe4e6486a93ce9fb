"""Float64 restatement of DLinear.forecasting() and of its parameter gradients (numpy; no torch, no GPU): the yardstick of
tests/test_gpu_dlinear.py, itself pinned against the real reference's goldens in tests/test_dlinear_ref.py.

S = input_len, P = pred_len, k = moving_avg.  data, mask (B, L, C) and tp (B, L) are zero-padded from L to S.  Per window b, channel c:

    cnt = max(sum m, 1); mean = sum d m / cnt; xc = d m - mean (EVERY l < S); std = sqrt(sum (xc m)^2 / cnt + 1e-5); xn = xc / std
    trend[l] = (1/k) sum_{|j| <= (k-1)//2} xn[clamp(l + j, 0, S-1)]; seas = xn - trend
    out[p] = Ws[p] . seas + Wt[p] . trend + Wtau[p] . tp[b] + bs[p] + bt[p] + btau[p];  y[b, p, c] = out[p] std + mean  (p < Lp)

Weights are (G, P, S) and biases (G, P) with G = C (one set per channel: individual mode) or G = 1 (shared)."""
import numpy as np


def stage(data, mask, tp, S, k):
    """-> seas, trend (B, C, S), times (B, S), mean, std (B, C), all float64"""
    data, mask, tp = (np.asarray(a, dtype=np.float64) for a in (data, mask, tp))
    B, L, C = data.shape
    assert L <= S and k % 2 == 1
    d, m, t = np.zeros((B, S, C)), np.zeros((B, S, C)), np.zeros((B, S))
    d[:, :L], m[:, :L], t[:, :L] = data, mask, tp
    cnt = np.maximum(m.sum(1), 1.0)
    mean = (d * m).sum(1) / cnt
    xc = d * m - mean[:, None, :]
    std = np.sqrt(((xc * m) ** 2).sum(1) / cnt + 1e-5)
    xn = xc / std[:, None, :]
    half = (k - 1) // 2
    idx = np.clip(np.arange(S)[:, None] + np.arange(-half, half + 1)[None, :], 0, S - 1)      # (S, k)
    trend = xn[:, idx, :].sum(2) / k
    seas = xn - trend
    return seas.transpose(0, 2, 1), trend.transpose(0, 2, 1), t, mean, std


def _w(a, C):
    a = np.asarray(a, dtype=np.float64)
    return np.broadcast_to(a, (C,) + a.shape[1:])


def forward(data, mask, tp, Lp, k, Ws, Wt, Wu, bs, bt, bu):
    """-> y (B, Lp, C) float64"""
    P, S = np.asarray(Ws).shape[1:]
    C = np.asarray(data).shape[2]
    seas, trend, t, mean, std = stage(data, mask, tp, S, k)
    out = (np.einsum("cpl,bcl->bcp", _w(Ws, C), seas) + np.einsum("cpl,bcl->bcp", _w(Wt, C), trend) +
           np.einsum("cpl,bl->bcp", _w(Wu, C), t) + (_w(bs, C) + _w(bt, C) + _w(bu, C))[None])
    y = out * std[:, :, None] + mean[:, :, None]
    return y.transpose(0, 2, 1)[:, :Lp]


def backward(data, mask, tp, k, S, P, dY, individual):
    """dY (B, Lp, C) -> dWs, dWt, dWtau (G, P, S), db (G, P) -- the three bias gradients are one array"""
    dY = np.asarray(dY, dtype=np.float64)
    B, Lp, C = dY.shape
    seas, trend, t, _, std = stage(data, mask, tp, S, k)
    dO = np.zeros((B, C, P))
    dO[:, :, :Lp] = dY.transpose(0, 2, 1) * std[:, :, None]      # rows p >= Lp were sliced off: no gradient
    dWs, dWt = np.einsum("bcp,bcl->cpl", dO, seas), np.einsum("bcp,bcl->cpl", dO, trend)
    dWu, db = np.einsum("bcp,bl->cpl", dO, t), dO.sum(0)
    if not individual:
        dWs, dWt, dWu, db = (a.sum(0, keepdims=True) for a in (dWs, dWt, dWu, db))
    return dWs, dWt, dWu, db


def golden_params(z, individual, C):
    """the six stacked parameter arrays (and, with prefix "g.", gradients) of a model_dlinear*.npz fixture"""
    def take(prefix, mod, leaf):
        if individual:
            return np.stack([z[f"{prefix}{mod}.{i}.{leaf}"] for i in range(C)])
        return z[f"{prefix}{mod}.{leaf}"][None]
    mods = ("Linear_Seasonal", "Linear_Trend", "Linear_Time")
    return {prefix: [take(prefix, m, "weight") for m in mods] + [take(prefix, m, "bias") for m in mods] for prefix in ("p.", "g.")}
