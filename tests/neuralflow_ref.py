"""float64 restatement of NeuralFlow.forecasting (reference models/NeuralFlow.py over lib/neural_flow_components at model = 'flow',
flow_model = 'coupling'), written from the algorithm: the encoder walks the observed points i = L-1 .. 0 with h = c = 0 -- a coupling
flow step on h over t_i - prev_t (prev_t = t[:, -1] + 0.01 at first, then the point before; every window has its own times), then an
LSTM cell on [data_i, mask_i] whose result is kept where any feature of the point is observed; transform_z0, softplus on the deviation
half, z0 = mu + eps sigma; the generative flow takes z0 to every forecast time on its own; the Linear decoder on every state.  A
coupling flow is a chain of layers, layer i with the mask m (ones on the first dim // 2 coordinates at even i, on the others at odd i,
none at dim == 1): (s, b) = MLP([x m, t]), phi = time_net(t) = scale t (TimeLinear) or tanh(scale t) (TimeTanh), and the coordinates
outside the mask become x exp(s phi_s) + b phi_b.  Any number of flow layers and of hidden layers.  Plain torch on the CPU; pinned to
the goldens of the reference's own code in tests/test_neuralflow_ref.py.  `params` is the module's state_dict (names as in the
reference)."""
import torch
import torch.nn.functional as F

CORE = "nf_model_core."
ENC = CORE + "encoder_z0."
ENC_FLOW = ENC + "z0_diffeq_solver.solver.flow.transforms."
GEN_FLOW = CORE + "diffeq_solver.solver.flow.transforms."
DEC = CORE + "decoder.decoder.0."


def mlp(p, prefix, x):
    """a Sequential of Linear layers at the even indices with Tanh between them"""
    idx = sorted(int(k[len(prefix):].split(".")[0]) for k in p if k.startswith(prefix) and k.endswith(".weight"))
    for i in idx:
        x = F.linear(x, p[f"{prefix}{i}.weight"], p[f"{prefix}{i}.bias"])
        if i != idx[-1]:
            x = torch.tanh(x)
    return x


def flow(p, prefix, x, t, time_net):
    """x (..., D), t (..., 1) -> the flow's state at t"""
    D = x.shape[-1]
    layers = sorted({int(k[len(prefix):].split(".")[0]) for k in p if k.startswith(prefix)})
    for i in layers:
        m = torch.zeros(D, dtype=x.dtype)
        if D > 1:
            if i % 2 == 0:
                m[:D // 2] = 1
            else:
                m[D // 2:] = 1
        s, b = mlp(p, f"{prefix}{i}.latent_net.net.", torch.cat([x * m, t], -1)).chunk(2, -1)
        phi = p[f"{prefix}{i}.time_net.scale"] * t
        if time_net == "TimeTanh":
            phi = torch.tanh(phi)
        phi_s, phi_b = phi.chunk(2, -1)
        x = torch.where(m.bool(), x, x * torch.exp(s * phi_s) + b * phi_b)
    return x


def lstm_cell(p, x, h, c):
    gates = F.linear(x, p[ENC + "lstm.weight_ih"], p[ENC + "lstm.bias_ih"]) + F.linear(h, p[ENC + "lstm.weight_hh"], p[ENC + "lstm.bias_hh"])
    i, f, g, o = gates.chunk(4, -1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


def encode(p, data, mask, tp, time_net):
    B, L, _ = data.shape
    R = p[ENC + "lstm.weight_hh"].shape[1]
    h, c = torch.zeros(B, R, dtype=data.dtype), torch.zeros(B, R, dtype=data.dtype)
    for i in reversed(range(L)):
        prev = tp[:, i + 1] if i + 1 < L else tp[:, -1] + 0.01
        h = flow(p, ENC_FLOW, h, (tp[:, i] - prev)[:, None], time_net)
        hn, cn = lstm_cell(p, torch.cat([data[:, i], mask[:, i]], -1), h, c)
        seen = mask[:, i].sum(-1, keepdim=True) > 0
        h, c = torch.where(seen, hn, h), torch.where(seen, cn, c)
    mu, sr = mlp(p, ENC + "transform_z0.", h).chunk(2, -1)
    return mu, F.softplus(sr)


def forecast(p, tpp, data, tp, mask, eps, time_net="TimeLinear"):
    """p: name -> tensor (any float dtype; the inputs are cast to it); tpp (B, Lp), tp (B, L), eps (B, latents) -> (B, Lp, C)"""
    dt = p[DEC + "weight"].dtype
    tpp, data, tp, mask, eps = (torch.as_tensor(v).to(dt) for v in (tpp, data, tp, mask, eps))
    mu, sigma = encode(p, data, mask, tp, time_net)
    z0 = mu + eps.reshape(mu.shape) * sigma
    z = flow(p, GEN_FLOW, z0[:, None, :].expand(-1, tpp.shape[1], -1), tpp[:, :, None], time_net)
    return F.linear(z, p[DEC + "weight"], p[DEC + "bias"])


def run(params, tpp, data, tp, mask, eps, upstream, dtype=torch.float64, time_net="TimeLinear"):
    """-> (out, name -> gradient of sum(out * upstream), None for the parameters without one), both as float64 tensors"""
    p = {k: torch.as_tensor(v).detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    out = forecast(p, tpp, data, tp, mask, eps, time_net)
    (out * torch.as_tensor(upstream).to(dtype)).sum().backward()
    return out.detach().double(), {k: (None if v.grad is None else v.grad.double()) for k, v in p.items()}
