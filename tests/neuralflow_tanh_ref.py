"""float64 restatement of NeuralFlow.forecasting() for the coupling flow with either time net, written from the algorithm and on its own
(nothing of tests/neuralflow_ref.py or of the product is imported): the yardstick of the fused TimeTanh kernels.

  time net      phi(t) = scale t  (TimeLinear)  |  tanh(scale t)  (TimeTanh), scale (1, 2 dim); (phi_s, phi_b) = its two halves
  layer i       m = ones on the first dim // 2 coordinates (even i) or on the others (odd i); no coordinate at dim == 1
                (s, b) = latent_net([x m, t]) -- Linears with Tanh between them;  x <- x where m, x exp(s phi_s) + b phi_b elsewhere
  encoder       h = c = 0; for i = L-1 .. 0: h <- flow_enc(h, t_i - prev) with prev = t_{L-1} + 0.01 first, then t_{i+1}; an LSTM cell on
                [data_i, mask_i], kept where any feature of point i is observed; (mu, sr) = transform_z0(h), sigma = softplus(sr)
  decode        z0 = mu + eps sigma;  out[b, j] = decoder(flow_gen(z0[b], tpp[b, j]))

run() returns the forecast and the gradient of sum(out * upstream) for every parameter (None where there is none), as float64 tensors,
and -- what the tests' input condition reads -- the largest phi^2 and |scale t| each of the two flows met.  `params` is the module's
state_dict.  Pinned to the module's own composed path in float64 in tests/test_neuralflow_tanh_ref.py."""
import torch

TIME_NETS = ("TimeLinear", "TimeTanh")
_ENC = "nf_model_core.encoder_z0."
_FLOWS = {"enc": _ENC + "z0_diffeq_solver.solver.flow.transforms.", "gen": "nf_model_core.diffeq_solver.solver.flow.transforms."}
_DEC = "nf_model_core.decoder.decoder.0."


def _numbered(p, prefix):
    """the sorted layer numbers N of the keys prefix + 'N.' ..."""
    return sorted({int(k[len(prefix):].split(".", 1)[0]) for k in p if k.startswith(prefix)})


def _mlp(p, prefix, x):
    idx = _numbered(p, prefix)
    for n in idx:
        x = x @ p[f"{prefix}{n}.weight"].T + p[f"{prefix}{n}.bias"]
        if n != idx[-1]:
            x = torch.tanh(x)
    return x


def _flow(p, which, x, t, time_net, stats):
    """x (..., D), t (..., 1) -> the state at t"""
    prefix = _FLOWS[which]
    D = x.shape[-1]
    for i in _numbered(p, prefix):
        keep = torch.zeros(D, dtype=torch.bool)
        if D > 1:
            keep[:D // 2] = True
            if i % 2:
                keep = ~keep
        sb = _mlp(p, f"{prefix}{i}.latent_net.net.", torch.cat([x * keep.to(x.dtype), t], -1))
        a = p[f"{prefix}{i}.time_net.scale"] * t
        phi = torch.tanh(a) if time_net == "TimeTanh" else a
        stats[which + "_phi2"] = max(stats.get(which + "_phi2", 0.0), float(phi.detach().square().max()))
        stats[which + "_arg"] = max(stats.get(which + "_arg", 0.0), float(a.detach().abs().max()))
        y = x * torch.exp(sb[..., :D] * phi[..., :D]) + sb[..., D:] * phi[..., D:]
        x = torch.where(keep, x, y)
    return x


def forecast(p, tpp, data, tp, mask, eps, time_net, stats=None):
    """p: name -> tensor of one float dtype (the inputs are cast to it); tpp (B, Lp), data, mask (B, L, C), tp (B, L), eps (B, latents)
    or (1, B, latents) -> (B, Lp, C)"""
    if time_net not in TIME_NETS:
        raise ValueError(time_net)
    stats = {} if stats is None else stats
    dt = p[_DEC + "weight"].dtype
    tpp, data, tp, mask, eps = (torch.as_tensor(v).to(dt) for v in (tpp, data, tp, mask, eps))
    B, L, _ = data.shape
    R = p[_ENC + "lstm.weight_hh"].shape[1]
    h = torch.zeros(B, R, dtype=dt)
    c = torch.zeros(B, R, dtype=dt)
    for i in range(L - 1, -1, -1):
        prev = tp[:, i + 1] if i + 1 < L else tp[:, L - 1] + 0.01
        h = _flow(p, "enc", h, (tp[:, i] - prev).unsqueeze(-1), time_net, stats)
        gates = torch.cat([data[:, i], mask[:, i]], -1) @ p[_ENC + "lstm.weight_ih"].T + p[_ENC + "lstm.bias_ih"] + \
            h @ p[_ENC + "lstm.weight_hh"].T + p[_ENC + "lstm.bias_hh"]
        gi, gf, gg, go = gates.split(R, -1)
        cn = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        hn = torch.sigmoid(go) * torch.tanh(cn)
        seen = mask[:, i].sum(-1, keepdim=True) > 0
        h, c = torch.where(seen, hn, h), torch.where(seen, cn, c)
    mu, sr = _mlp(p, _ENC + "transform_z0.", h).chunk(2, -1)
    z0 = mu + eps.reshape(mu.shape) * torch.nn.functional.softplus(sr)
    Lp = tpp.shape[1]
    z = _flow(p, "gen", z0.unsqueeze(1).expand(B, Lp, z0.shape[-1]), tpp.unsqueeze(-1), time_net, stats)
    return z @ p[_DEC + "weight"].T + p[_DEC + "bias"]


def run(params, tpp, data, tp, mask, eps, upstream, time_net, dtype=torch.float64):
    """-> (out, name -> gradient of sum(out * upstream) or None, stats), tensors as float64.  stats: enc_phi2, gen_phi2 (the largest
    phi^2 of each flow, so 1 - phi^2 gets as far from 1 as that) and enc_arg, gen_arg (the largest |scale t|)"""
    p = {k: torch.as_tensor(v).detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    stats = {}
    out = forecast(p, tpp, data, tp, mask, eps, time_net, stats)
    (out * torch.as_tensor(upstream).to(dtype)).sum().backward()
    return out.detach().double(), {k: (None if v.grad is None else v.grad.double()) for k, v in p.items()}, stats
