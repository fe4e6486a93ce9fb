"""Float64 restatement of TimeMixer.forecasting() (reference models/TimeMixer.py:268-326) for the default option set -- moving-average
decomposition, channel independence, average pooling with window 2 -- in torch float64; gradients come from autograd.  The yardstick of
tests/test_gpu_timemixer.py, itself pinned against the real reference's goldens in tests/test_timemixer_ref.py.

Parameters are a dict under the reference's state-dict names.  `keep` is the dropout of the embedding (layers/Embed.py:109-126, the
model's only dropout, once per scale): a list of per-scale (B, T_i, d_model) multipliers, 0 or 1 / (1 - p); None applies no dropout.
`dtype` is torch.float64 except for the margin check, which runs this very arithmetic in float32."""
import math

import torch
import torch.nn.functional as F


def scale_lengths(input_len, down_sampling_layers, w=2):
    """T_0 .. T_n; n is the constructor's clipped count (models/TimeMixer.py:176-185)"""
    T, cur, n = [input_len], input_len, 0
    while n < down_sampling_layers and cur >= w:
        cur //= w
        n += 1
        T.append(cur)
    return T


def _movavg(x, k):
    """layers/Autoformer_EncDec.py:21-38 on (B, T, d): replicate-padded on both sides, window k (odd), stride 1"""
    half = (k - 1) // 2
    xp = torch.cat([x[:, :1].expand(-1, half, -1), x, x[:, -1:].expand(-1, half, -1)], dim=1)
    return F.avg_pool1d(xp.permute(0, 2, 1), k, 1).permute(0, 2, 1)


def _mlp(p, prefix, x):
    """nn.Sequential(Linear, GELU (exact erf form), Linear) on the last axis"""
    h = F.linear(x, p[prefix + ".0.weight"], p[prefix + ".0.bias"])
    h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
    return F.linear(h, p[prefix + ".2.weight"], p[prefix + ".2.bias"])


def forward(p, data, mask, tp, Lp, input_len, pred_len, e_layers, moving_avg, down_sampling_layers=3, keep=None,
            dtype=torch.float64):
    """data, mask (B, L <= input_len, C), tp (B, L) -> (B, Lp, C).  p: name -> tensor of `dtype` (leaves that may want a gradient)."""
    data, mask, tp = (torch.as_tensor(t).to(dtype) for t in (data, mask, tp))
    B, L, C = data.shape
    T = scale_lengths(input_len, down_sampling_layers)
    n = len(T) - 1
    if L < input_len:                                                     # models/TimeMixer.py:278-286
        z = torch.zeros(B, input_len - L, C, dtype=dtype)
        data, mask, tp = torch.cat([data, z], 1), torch.cat([mask, z], 1), torch.cat([tp, z[:, :, 0]], 1)
    x = data * mask                                                       # :297-303
    cnt = mask.sum(1, keepdim=True).clamp(min=1)
    means = x.sum(1, keepdim=True) / cnt
    x = x - means
    stdev = torch.sqrt(((x * mask) ** 2).sum(1, keepdim=True) / cnt + 1e-5)
    x = x / stdev
    enc = torch.cat([x, mask, tp.unsqueeze(-1)], dim=-1)                  # :306
    xs = [enc]                                                            # :249-266, AvgPool1d(2) drops an odd tail
    for i in range(n):
        cur = xs[-1]
        xs.append(0.5 * (cur[:, 0:2 * T[i + 1]:2] + cur[:, 1:2 * T[i + 1]:2]))
    W = p["enc_embedding.value_embedding.tokenConv.weight"]               # (d, 2C+1, 3); layers/Embed.py:29-42: circular, 3 taps
    pe = p["enc_embedding.position_embedding.pe"][0]
    out = []
    for i, xi in enumerate(xs):                                           # :312
        taps = torch.stack([torch.roll(xi, 1, 1), xi, torch.roll(xi, -1, 1)], dim=-1)      # (B, T, K, 3)
        e = torch.einsum("btkj,fkj->btf", taps, W) + pe[:T[i]]
        out.append(e if keep is None else e * torch.as_tensor(keep[i]).to(dtype))
    for j in range(e_layers):                                             # :134-161
        pre = f"pdm_blocks.{j}."
        trend = [_movavg(o, moving_avg) for o in out]
        season = [(o - t).permute(0, 2, 1) for o, t in zip(out, trend)]
        trend = [t.permute(0, 2, 1) for t in trend]
        os_ = [season[0]]                                                 # :50-63, bottom-up
        for i in range(n):
            os_.append(season[i + 1] + _mlp(p, pre + f"mix_season.down_sampling_layers.{i}", os_[-1]))
        if j < e_layers - 1:                                              # :84-97, top-down; layer m serves scale n-1-m
            ot = [None] * (n + 1)
            ot[n] = trend[n]
            for i in range(n - 1, -1, -1):
                ot[i] = trend[i] + _mlp(p, pre + f"mix_trend.up_sampling_layers.{n - 1 - i}", ot[i + 1])
            out = [o + _mlp(p, pre + "out_layer", (a + b).permute(0, 2, 1)) for o, a, b in zip(out, os_, ot)]
        else:       # :319 reads the coarsest scale alone: the last block's trend mixing and its finer out_layer results are dead
            out = out[:n] + [out[n] + _mlp(p, pre + "out_layer", (os_[n] + trend[n]).permute(0, 2, 1))]
    dec = F.linear(out[n].permute(0, 2, 1), p[f"predict_layers.{n}.weight"], p[f"predict_layers.{n}.bias"]).permute(0, 2, 1)   # :319-322
    dec = F.linear(dec, p["projection.weight"], p["projection.bias"])
    return (dec * stdev + means)[:, :Lp]                                  # :325-326


def dead_names(names, e_layers, n):
    """the parameters forecasting() never reaches (grad is None after backward())"""
    dead = set()
    for k in names:
        if k.startswith("normalize_layers.") or k.startswith("enc_embedding.temporal_embedding.") or \
                k.startswith(f"pdm_blocks.{e_layers - 1}.mix_trend."):
            dead.add(k)
        if k.startswith("predict_layers.") and int(k.split(".")[1]) < n:
            dead.add(k)
    return dead


def run(params, data, mask, tp, upstream, input_len, pred_len, e_layers, moving_avg, keep=None, dtype=torch.float64):
    """-> (out, {name: gradient or None}) for every floating-point entry of `params` (numpy arrays or tensors) but the pe buffer"""
    p = {k: torch.as_tensor(v).to(dtype).clone() for k, v in params.items()}
    for k, v in p.items():
        if not k.endswith(".pe"):
            v.requires_grad_(True)
    up = torch.as_tensor(upstream).to(dtype)
    out = forward(p, data, mask, tp, up.shape[1], input_len, pred_len, e_layers, moving_avg, keep=keep, dtype=dtype)
    (out * up).sum().backward()
    return out.detach(), {k: v.grad for k, v in p.items() if not k.endswith(".pe")}
