"""The two stages of models/TimesNet.py around its TimesBlock loop restated in float64 from the reference's forecasting()
(models/TimesNet.py:104-131 and :137-148) and layers/Embed.py (TokenEmbedding: circular 3-tap Conv1d without bias; PositionalEmbedding;
DataEmbedding's dropout): functions of tensors, with the parameter gradients written out.  The yardsticks of csrc/timesnet_model.hip and of
the row-offset tail of csrc/informer.hip; pinned to torch.nn.functional + autograd and to the golden in tests/test_timesnet_model_ref.py."""
import torch


def front(data, mask, tp, tpp, input_len, pred_len, W_token, pe, W_predict, b_predict, scale=None):
    """data, mask (B, L, C), tp (B, L), tpp (B, Lp), W_token (D, 2C + 1, 3), pe (>= input_len, D), W_predict (T, T), b_predict (T) ->
    (enc (B, T, D), means, stdev (B, 1, C), E (B, T, D), inp (B, input_len, 2C + 1)).  scale: the dropout factors keep / (1 - p),
    (B, input_len, D) (None: no dropout)."""
    B, L, C = data.shape
    Lp = tpp.shape[1]
    S, P = input_len, pred_len
    d = torch.zeros(B, S, C, dtype=data.dtype)
    m = torch.zeros(B, S, C, dtype=data.dtype)
    t = torch.zeros(B, S, dtype=data.dtype)
    tq = torch.zeros(B, P, dtype=data.dtype)
    d[:, :L], m[:, :L], t[:, :L], tq[:, :Lp] = data, mask, tp, tpp
    means = d.mean(1, keepdim=True)                                                        # over all S rows, the padding included
    x = d - means
    stdev = torch.sqrt((x ** 2).mean(1, keepdim=True) + 1e-5)
    inp = torch.cat([x / stdev, m, t.unsqueeze(-1)], -1)                                   # (B, S, 2C + 1)
    s = torch.arange(S)
    emb = pe[:S].unsqueeze(0) + sum(torch.einsum("bsc,dc->bsd", inp[:, (s + k - 1) % S, :], W_token[:, :, k]) for k in range(3))
    if scale is not None:
        emb = emb * scale
    E = torch.cat([emb, tq.unsqueeze(-1).expand(B, P, emb.shape[-1])], 1)                  # (B, T, D)
    enc = torch.einsum("ts,bsd->btd", W_predict, E) + b_predict.view(1, -1, 1)
    return enc, means, stdev, E, inp


def front_grads(d_enc, E, inp, W_predict, input_len, scale=None):
    """the parameter gradients of `front` from the upstream d_enc (B, T, D): -> dict(W_predict (T, T), b_predict (T), W_token (D, 2C + 1, 3))"""
    S = input_len
    dWp = torch.einsum("btd,bsd->ts", d_enc, E)
    dbp = d_enc.sum((0, 2))
    dE = torch.einsum("ts,btd->bsd", W_predict, d_enc)[:, :S]
    if scale is not None:
        dE = dE * scale
    s = torch.arange(S)
    dWc = torch.stack([torch.einsum("bsd,bsc->dc", dE, inp[:, (s + k - 1) % S, :]) for k in range(3)], -1)
    return dict(W_predict=dWp, b_predict=dbp, W_token=dWc)


def tail(x, gamma, beta, W, b, means, stdev, input_len, Lp, eps=1e-5):
    """x (B, T, D) -> LayerNorm -> W (C, D), b (C) -> * stdev + means (B, 1, C), rows input_len .. input_len + Lp - 1 -> (B, Lp, C)"""
    x = x[:, input_len:input_len + Lp]
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    n = (x - mu) / torch.sqrt(var + eps) * gamma + beta
    return (n @ W.t() + b) * stdev + means


def tail_grads(dy, x, gamma, beta, W, stdev, input_len, Lp, eps=1e-5):
    """the gradients of `tail` from the upstream dy (B, Lp, C): -> dict(x (B, T, D; zeros outside the horizon rows), gamma, beta, W, b)"""
    D = x.shape[-1]
    xs = x[:, input_len:input_len + Lp]
    mu = xs.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xs - mu) ** 2).mean(-1, keepdim=True) + eps)
    xh = (xs - mu) * rstd
    n = xh * gamma + beta
    dz = dy * stdev                                                                        # (B, Lp, C)
    dn = dz @ W                                                                            # (B, Lp, D)
    g = dn * gamma
    dxs = rstd * (g - g.sum(-1, keepdim=True) / D - xh * (g * xh).sum(-1, keepdim=True) / D)
    dx = torch.zeros_like(x)
    dx[:, input_len:input_len + Lp] = dxs
    return dict(x=dx, gamma=(dn * xh).sum((0, 1)), beta=dn.sum((0, 1)), W=torch.einsum("blc,bld->cd", dz, n), b=dz.sum((0, 1)))
