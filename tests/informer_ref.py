"""Informer's layers restated in float64 from the reference's mathematics (layers/SelfAttention_Family.py ProbAttention,
layers/Transformer_EncDec.py ConvLayer / DecoderLayer / Decoder, models/Informer.py): functions of tensors and of a state dict, not
modules, differentiated by autograd.  The yardsticks of csrc/prob_attn.hip and csrc/conv_distil.hip.

Two definitions the reference leaves open are fixed as the product fixes them: ties in the sparsity measure go to the lower query index
(the selected set is ascending), and the measure is the un-squeezed one."""
import math

import torch
import torch.nn.functional as F


def measure(q, k, sample):
    """q (B, L_Q, H, D), k (B, L_K, H, D), sample (L_Q, U) -> M (B, H, L_Q) = max_j q_i.k_s(i,j) - sum_j q_i.k_s(i,j) / L_K"""
    Q, K = q.transpose(1, 2), k.transpose(1, 2)
    QK = torch.einsum("bhld,bhlud->bhlu", Q, K[:, :, sample.long(), :])
    return QK.max(-1).values - QK.sum(-1) / k.shape[1]


def select(M, u):
    """the u largest per (b, h), ties to the lower index, ascending -> (B, H, u) int64"""
    top = torch.sort(M, dim=-1, descending=True, stable=True).indices[..., :u]
    return torch.sort(top, dim=-1).values


def min_gap(M, u):
    """smallest gap between the u-th and (u+1)-th largest M over (b, h), relative to max|M| (inf when every query is selected)"""
    if u >= M.shape[-1]:
        return float("inf")
    top = torch.sort(M, dim=-1, descending=True).values
    return float(((top[..., u - 1] - top[..., u]) / M.abs().amax(-1)).min())


def prob_attention(q, k, v, sample, u, scale, causal, sel=None):
    """-> (out (B, H, L_Q, D), sel (B, H, u)).  No gradient through the measure."""
    B, LQ, H, D = q.shape
    LK = k.shape[1]
    Q, K, V = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    if sel is None:
        with torch.no_grad():
            sel = select(measure(q, k, sample), u)
    rows = []
    for b in range(B):
        for h in range(H):
            if causal:
                assert LQ == LK
                ctx = torch.cumsum(V[b, h], 0)
            else:
                ctx = V[b, h].mean(0, keepdim=True).expand(LQ, D)
            ctx = [ctx[i] for i in range(LQ)]
            for i in sel[b, h].tolist():
                s = (Q[b, h, i] @ K[b, h].t()) * scale
                if causal:
                    s = s.masked_fill(torch.arange(LK) > i, float("-inf"))
                ctx[i] = torch.softmax(s, -1) @ V[b, h]
            rows.append(torch.stack(ctx))
    return torch.stack(rows).reshape(B, H, LQ, D), sel


def n_sample(factor, L):
    return min(factor * math.ceil(math.log(L)), L)


def conv_layer(x, p, pre, training, eps=1e-5, momentum=0.1):
    """ConvLayer on x (B, L, d) with p[pre + 'downConv.weight'] ...: -> (out (B, (L + 1) // 2 + 1, d), buffers after the call)"""
    W, b = p[pre + "downConv.weight"], p[pre + "downConv.bias"]
    gamma, beta = p[pre + "norm.weight"], p[pre + "norm.bias"]
    rm, rv, nb = p[pre + "norm.running_mean"], p[pre + "norm.running_var"], p[pre + "norm.num_batches_tracked"]
    B, L, d = x.shape
    T = L + 2
    t = torch.arange(T)
    y = b + sum(x[:, (t - 2 + kk) % L, :] @ W[:, :, kk].t() for kk in range(3))      # (B, T, d)
    if training:
        R = B * T
        mean = y.mean((0, 1))
        var = ((y - mean) ** 2).mean((0, 1))
        after = {"running_mean": (1 - momentum) * rm + momentum * mean.detach(),
                 "running_var": (1 - momentum) * rv + momentum * var.detach() * R / (R - 1), "num_batches_tracked": nb + 1}
    else:
        mean, var = rm, rv
        after = {"running_mean": rm, "running_var": rv, "num_batches_tracked": nb}
    a = F.elu((y - mean) / torch.sqrt(var + eps) * gamma + beta)
    Lo = (L + 1) // 2 + 1
    out = []
    for s in range(Lo):
        win = [tt for tt in (2 * s - 1, 2 * s, 2 * s + 1) if 0 <= tt < T]
        out.append(a[:, win, :].max(1).values)
    return torch.stack(out, 1), after


def _ln(x, p, pre, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), p[pre + "weight"], p[pre + "bias"], eps)


def _lin(x, p, pre):
    return x @ p[pre + "weight"].t() + p[pre + "bias"]


def attention_layer(xq, xkv, p, pre, H, factor, causal, sample, log):
    """AttentionLayer around ProbAttention: the (B, H, L, D) result is reshaped to (B, L, H D) WITHOUT a transpose, as the reference"""
    B, L, _ = xq.shape
    S = xkv.shape[1]
    q = _lin(xq, p, pre + "query_projection.").view(B, L, H, -1)
    k = _lin(xkv, p, pre + "key_projection.").view(B, S, H, -1)
    v = _lin(xkv, p, pre + "value_projection.").view(B, S, H, -1)
    u = n_sample(factor, L)
    assert tuple(sample.shape) == (L, n_sample(factor, S)), (sample.shape, L, S)
    with torch.no_grad():
        log.append(min_gap(measure(q, k, sample), u))
    out, _ = prob_attention(q, k, v, sample, u, 1.0 / math.sqrt(q.shape[-1]), causal)
    return _lin(out.reshape(B, L, -1), p, pre + "out_projection.")


def _ffn(x, p, pre, act):
    y = act(x @ p[pre + "conv1.weight"].squeeze(-1).t() + p[pre + "conv1.bias"])
    return y @ p[pre + "conv2.weight"].squeeze(-1).t() + p[pre + "conv2.bias"]


def _embed(x, p, pre):
    W = p[pre + "value_embedding.tokenConv.weight"]      # (d, c, 3), circular padding 1, no bias
    L = x.shape[1]
    t = torch.arange(L)
    y = sum(x[:, (t - 1 + kk) % L, :] @ W[:, :, kk].t() for kk in range(3))
    return y + p[pre + "position_embedding.pe"][:, :L]


def informer(p, opts, tpp, data, tp, mask, samples, training=True):
    """models/Informer.py forecasting() at dropout 0 from the state dict p (float64) -> (out (B, Lp, C), the conv layers' buffers after
    the call, the smallest measure gap per ProbAttention call).  samples: the (L_Q, U_part) draws in call order."""
    act = F.relu if opts["activation"] == "relu" else F.gelu
    H, factor = opts["n_heads"], opts["factor"]
    B, L, C = data.shape
    if L < opts["input_len"]:
        pad = opts["input_len"] - L
        z = data.new_zeros(B, pad, C)
        data, mask, tp = torch.cat([data, z], 1), torch.cat([mask, z], 1), torch.cat([tp, z[:, :, 0]], 1)
    Lp = tpp.shape[1]
    if Lp < opts["pred_len"]:
        tpp = torch.cat([tpp, tpp.new_zeros(B, opts["pred_len"] - Lp)], 1)
    cnt = mask.sum(1, keepdim=True).clamp(min=1)
    x = data * mask
    means = x.sum(1, keepdim=True) / cnt
    x = x - means
    stdev = torch.sqrt(((x * mask) ** 2).sum(1, keepdim=True) / cnt + 1e-5)
    x = x / stdev
    zp = data.new_zeros(B, opts["pred_len"], C)
    enc = _embed(torch.cat([x, mask, tp.unsqueeze(-1)], -1), p, "enc_embedding.")
    dec = _embed(torch.cat([zp, zp, tpp.unsqueeze(-1)], -1), p, "dec_embedding.")
    samples, log, after = list(samples), [], {}
    for i in range(opts["e_layers"]):
        pre = f"encoder.attn_layers.{i}."
        a = attention_layer(enc, enc, p, pre + "attention.", H, factor, False, samples.pop(0), log)
        enc = _ln(enc + a, p, pre + "norm1.")
        enc = _ln(enc + _ffn(enc, p, pre, act), p, pre + "norm2.")
        if opts["distil"] and i < opts["e_layers"] - 1:
            enc, bufs = conv_layer(enc, p, f"encoder.conv_layers.{i}.", training)
            after.update({f"encoder.conv_layers.{i}.norm.{k}": v for k, v in bufs.items()})
    enc = _ln(enc, p, "encoder.norm.")
    for i in range(opts["d_layers"]):
        pre = f"decoder.layers.{i}."
        dec = _ln(dec + attention_layer(dec, dec, p, pre + "self_attention.", H, factor, True, samples.pop(0), log), p, pre + "norm1.")
        dec = _ln(dec + attention_layer(dec, enc, p, pre + "cross_attention.", H, factor, False, samples.pop(0), log), p, pre + "norm2.")
        dec = _ln(dec + _ffn(dec, p, pre, act), p, pre + "norm3.")
    assert not samples
    dec = _lin(_ln(dec, p, "decoder.norm."), p, "decoder.projection.")
    return (dec * stdev + means)[:, :Lp], after, log
