"""The TTM backbone restated in float64 from the reference's mathematics (models/TTM.py, layers/MLP.py): a function of the state
dict, not a module.  `run` differentiates it with autograd; `block` and `gate` are one mixer block and the feature mixer's gate +
residual on their own, the yardsticks of csrc/ttm.hip.  Optional dropout enters as keep multipliers (0 or 1 / (1 - p)).

keep of a narrow block: (k1, k2) in the kernel's element order -- k1 (G, D, 2F), k2 (G, D, F) with G = B M groups (patch) or B N groups
(channel, group = b N + n)."""
import torch
import torch.nn.functional as F

BLOCK_KEYS = ("norm.weight", "norm.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias",
              "gating_block.attn_layer.weight", "gating_block.attn_layer.bias")


def block(x, params, mode, keep=None, eps=1e-5):
    """x (B, M, N, D); params in BLOCK_KEYS order; mode patch / channel / feature"""
    gamma, beta, W1, b1, W2, b2, Wg, bg = params
    B, M, N, D = x.shape
    t = F.layer_norm(x, (D,), gamma, beta, eps)
    if mode == "patch":
        t = t.permute(0, 1, 3, 2)          # (B, M, D, N)
    elif mode == "channel":
        t = t.permute(0, 3, 2, 1)          # (B, D, N, M)
    h = F.gelu(t @ W1.t() + b1)
    if keep is not None:
        k1, k2 = keep
        if mode == "patch":
            k1, k2 = k1.reshape(B, M, D, -1), k2.reshape(B, M, D, -1)
        else:
            k1, k2 = k1.reshape(B, N, D, -1).permute(0, 2, 1, 3), k2.reshape(B, N, D, -1).permute(0, 2, 1, 3)
        h = h * k1.to(h.dtype)
    u = h @ W2.t() + b2
    if keep is not None:
        u = u * k2.to(u.dtype)
    y = u * torch.softmax(u @ Wg.t() + bg, -1)
    if mode == "patch":
        y = y.permute(0, 1, 3, 2)
    elif mode == "channel":
        y = y.permute(0, 3, 2, 1)
    return x + y


def gate(res, u, g):
    return res + u * torch.softmax(g, -1)


def _block(P, prefix, x, mode):
    return block(x, [P[prefix + k] for k in BLOCK_KEYS], mode)


def _layer(P, prefix, x, mix_channel):
    if mix_channel:
        x = _block(P, prefix + "channel_feature_mixer.", x, "channel")
    if x.shape[2] > 1:
        x = _block(P, prefix + "patch_mixer.", x, "patch")
    return _block(P, prefix + "feature_mixer.", x, "feature")


def num_patches(opts):
    return (max(opts["input_len"], opts["patch_size"]) - opts["patch_size"]) // opts["stride"] + 1


def forward(P, data, mask, tp, Lp, opts):
    """P: name -> tensor (the state dict); data, mask (B, L, C), tp (B, L) -> (B, Lp, C)"""
    B, L, C = data.shape
    S = opts["input_len"]
    if L < S:
        z = data.new_zeros(B, S - L, C)
        data, mask, tp = torch.cat([data, z], 1), torch.cat([mask, z], 1), torch.cat([tp, z[:, :, 0]], 1)
    vals = data * mask
    t = tp.unsqueeze(-1)
    x = torch.cat([vals, mask, t], -1)
    if opts["use_norm"]:
        cnt = mask.sum(1).clamp(min=1)
        mu = vals.sum(1) / cnt
        cen = vals - mu.unsqueeze(1)
        sd = torch.sqrt(((cen * mask) ** 2).sum(1) / cnt + 1e-5)
        x = torch.cat([cen / sd.unsqueeze(1), mask - 0.5, (t - t.mean(1, keepdim=True)) / (t.std(1, keepdim=True) + 1e-5)], -1)
        m2 = x.mean(1, keepdim=True).detach()
        s2 = torch.sqrt(x.var(1, keepdim=True, unbiased=False) + 1e-5)
        x = (x - m2) / s2
    mix = opts["mode"] == "mix_channel"
    x = x.permute(0, 2, 1).unfold(-1, opts["patch_size"], opts["stride"])
    x = x @ P["backbone.patcher.weight"].t() + P["backbone.patcher.bias"]
    AP = opts["AP_levels"]
    if AP > 0:
        for i, lvl in enumerate(reversed(range(AP))):
            k = 2 ** lvl
            Bx, M, N, D = x.shape
            x = x.reshape(Bx, M, N * k, D // k)
            for j in range(opts["e_layers"]):
                x = _layer(P, f"backbone.encoder.mixers.{i}.mixer_layers.{j}.", x, mix)
            x = x.reshape(Bx, M, N, D)
    else:
        for j in range(opts["e_layers"]):
            x = _layer(P, f"backbone.encoder.mixers.{j}.", x, mix)
    if opts["use_decoder"]:
        x = x @ P["decoder_adapter.weight"].t() + P["decoder_adapter.bias"]
        for j in range(opts["d_layers"]):
            x = _layer(P, f"decoder.mixers.{j}.", x, mix)
    y = x.flatten(-2) @ P["head.base_forecast_block.weight"].t() + P["head.base_forecast_block.bias"]
    y = y.transpose(-1, -2)
    if opts["use_norm"]:
        y = y * s2 + m2
    y = y[..., :C]
    if opts["use_norm"]:
        y = y * sd.unsqueeze(1) + mu.unsqueeze(1)
    return y[:, :Lp, :]


def run(params, data, mask, tp, upstream, opts, dtype=torch.float64):
    """-> (out, name -> gradient or None)"""
    P = {k: torch.as_tensor(v).detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    data, mask, tp, upstream = (torch.as_tensor(t).detach().to(dtype) for t in (data, mask, tp, upstream))
    out = forward(P, data, mask, tp, upstream.shape[1], opts)
    (out * upstream).sum().backward()
    return out.detach(), {k: (None if p.grad is None else p.grad.detach()) for k, p in P.items()}


def run_block(x, params, upstream, mode, keep=None, dtype=torch.float64):
    """one narrow block -> (out, dx, the eight parameter gradients)"""
    x = torch.as_tensor(x).detach().cpu().to(dtype).clone().requires_grad_(True)
    ps = [torch.as_tensor(p).detach().cpu().to(dtype).clone().requires_grad_(True) for p in params]
    if keep is not None:
        keep = tuple(k.detach().cpu().to(dtype) for k in keep)
    out = block(x, ps, mode, keep=keep)
    (out * torch.as_tensor(upstream).detach().cpu().to(dtype)).sum().backward()
    return out.detach(), x.grad, [p.grad for p in ps]
