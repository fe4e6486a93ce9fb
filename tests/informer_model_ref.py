"""The two non-layer stages of models/Informer.py restated in float64 from their formulas (DESIGN 4j addendum): functions of tensors,
differentiated by autograd.  The yardsticks of csrc/informer.hip; pinned to tests/informer_ref.py and the goldens in
tests/test_informer_model_ref.py."""
import torch


def front(data, mask, tp, tpp, input_len, pred_len, W_enc, W_dec, pe_enc, pe_dec, scale_enc=None, scale_dec=None):
    """data, mask (B, L, C), tp (B, L), tpp (B, Lp), W_* (D, 2C + 1, 3), pe_* (>= length, D) -> (enc (B, input_len, D), dec (B, pred_len,
    D), means, stdev (B, 1, C)).  scale_enc / scale_dec: the dropout factors keep / (1 - p) in the outputs' shapes (None: no dropout)."""
    B, L, C = data.shape
    Lp = tpp.shape[1]
    S, P = input_len, pred_len
    d = torch.zeros(B, S, C, dtype=data.dtype)
    m = torch.zeros(B, S, C, dtype=data.dtype)
    t = torch.zeros(B, S, dtype=data.dtype)
    tq = torch.zeros(B, P, dtype=data.dtype)
    d[:, :L], m[:, :L], t[:, :L], tq[:, :Lp] = data, mask, tp, tpp
    cnt = m.sum(1, keepdim=True).clamp(min=1)
    means = (d * m).sum(1, keepdim=True) / cnt
    x = d * m - means
    stdev = torch.sqrt(((x * m) ** 2).sum(1, keepdim=True) / cnt + 1e-5)
    inp = torch.cat([x / stdev, m, t.unsqueeze(-1)], -1)                                   # (B, S, 2C + 1)
    l, q = torch.arange(S), torch.arange(P)
    enc = pe_enc[:S].unsqueeze(0) + sum(torch.einsum("blc,dc->bld", inp[:, (l + k - 1) % S, :], W_enc[:, :, k]) for k in range(3))
    dec = pe_dec[:P].unsqueeze(0) + sum(tq[:, (q + k - 1) % P].unsqueeze(-1) * W_dec[:, 2 * C, k] for k in range(3))
    if scale_enc is not None:
        enc = enc * scale_enc
    if scale_dec is not None:
        dec = dec * scale_dec
    return enc, dec, means, stdev


def tail(x, gamma, beta, W, b, means, stdev, Lp, eps=1e-5):
    """x (B, pred_len, D) -> LayerNorm -> W (C, D), b (C) -> * stdev + means (B, 1, C), rows t < Lp -> (B, Lp, C)"""
    x = x[:, :Lp]
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    n = (x - mu) / torch.sqrt(var + eps) * gamma + beta
    return (n @ W.t() + b) * stdev + means
