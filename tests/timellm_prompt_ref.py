"""float64 restatement of the five statistics TimeLLM's prompt spells (models/TimeLLM.py _get_prompt), in the form
immtsf.ops.timellm_prompt_stats documents: selections with ties to the lower time index, the lower median, the circular
autocorrelation summed DIRECTLY (no FFT) for tau <= L // 2 and mirrored, the largest lags with ties to the lower lag.  numpy only.
tests/test_timellm_prompt_ref.py pins it against the torch expressions of _get_prompt evaluated in float64."""
import numpy as np


def half_corr64(x):
    """corr[tau] = mean_c sum_t x[t, c] x[(t + tau) mod L, c] for tau = 0 .. L // 2; x (L, C)"""
    x = np.asarray(x, np.float64)
    L = x.shape[0]
    return np.array([(x * np.roll(x, -tau, axis=0)).sum(axis=0).mean() for tau in range(L // 2 + 1)])


def full_corr64(x):
    """all L lags: corr[L - tau] is corr[tau], bit for bit"""
    h = half_corr64(x)
    L = np.asarray(x).shape[0]
    full = np.empty(L)
    for tau in range(L):
        full[tau] = h[min(tau, L - tau)]
    return full


def window_stats64(x, top_k):
    """x (L, C) -> mins, maxs, meds (C,) float64 (each an element of x, or NaN), trend (float), lags (top_k,) int"""
    x = np.asarray(x, np.float64)
    L, C = x.shape
    nan_c = np.isnan(x).any(axis=0)
    mins, maxs, meds = np.empty(C), np.empty(C), np.empty(C)
    for c in range(C):
        col = x[:, c]
        if nan_c[c]:
            mins[c] = maxs[c] = meds[c] = np.nan
            continue
        mins[c] = col[int(np.argmin(col))]                      # argmin / argmax return the FIRST of equal elements (-0.0 == 0.0)
        maxs[c] = col[int(np.argmax(col))]
        meds[c] = col[np.argsort(col, kind="stable")[(L - 1) // 2]]      # stable: ties to the lower time index
    trend = float(np.diff(x, axis=0).sum(axis=0).mean())       # an empty sum at L == 1: 0
    corr = full_corr64(x)
    corr = np.where(np.isnan(corr), -np.inf, corr)
    kk = min(top_k, L)
    lags = list(np.argsort(-corr, kind="stable")[:kk])        # descending, ties to the lower lag
    lags += [lags[-1]] * (top_k - kk)
    return mins, maxs, meds, trend, np.array(lags, dtype=np.int64)


def batch_stats64(x, top_k):
    """x (B, L, C) -> stats (B, 3 C + 1) float64 = min | max | median | trend, lags (B, top_k) int64"""
    x = np.asarray(x, np.float64)
    B, L, C = x.shape
    stats, lags = np.empty((B, 3 * C + 1)), np.empty((B, top_k), dtype=np.int64)
    for b in range(B):
        mn, mx, md, tr, lg = window_stats64(x[b], top_k)
        stats[b] = np.concatenate([mn, mx, md, [tr]])
        lags[b] = lg
    return stats, lags
