"""float64 restatement of LatentODE.forecasting (reference models/LatentODE.py over lib/latent_ode_components), written from the
algorithm: the ODE-RNN encoder walks the observed points i = L-1 .. 0 -- from prev_t (t[-1] + 0.01 at first, then the point before) to
t_i by one Euler step where prev_t - t_i < minimum_step = (t[-1] - t[0]) / 50, else by max(2, int((prev_t - t_i) / minimum_step)) - 1
steps of the 3/8-rule RK4 on an even grid, then the GRU update (sigmoid gates, the reset applied to mean and deviation, abs on the new
deviation, the update kept only where any feature of the point is observed, abs again); L == 1 is a GRU update from zeros;
transform_z0, abs on the deviation half, z0 = mu + eps sigma; one RK4 step of the generative net per interval of tp_to_predict, z0 at
tp_to_predict[0]; the Linear decoder on every state.  With ode_z0_encoder = 'rnn': a GRU over [delta_t, data, mask] in reverse order
and hiddens_to_z0.  Any number of hidden layers in the two gradient nets; n_traj_samples > 1 (eps (n, B, latents)) averages the
forecasts.  Plain torch on the CPU; pinned to the real reference's goldens in tests/test_latent_ode_ref.py.  `params` is the module's
state_dict (names as in the reference)."""
import torch
import torch.nn.functional as F

CORE = "latent_ode_model_core."
ENC = CORE + "encoder_z0."
GRU = ENC + "GRU_update."
ENC_ODE = ENC + "z0_diffeq_solver.ode_func.gradient_net."
GEN_ODE = CORE + "diffeq_solver.ode_func.gradient_net."
DEC = CORE + "decoder.decoder.0."


def mlp(p, prefix, x):
    """a Sequential of Linear layers at the even indices with Tanh between them"""
    idx = sorted(int(k[len(prefix):].split(".")[0]) for k in p if k.startswith(prefix) and k.endswith(".weight"))
    for i in idx:
        x = F.linear(x, p[f"{prefix}{i}.weight"], p[f"{prefix}{i}.bias"])
        if i != idx[-1]:
            x = torch.tanh(x)
    return x


def rk4(f, y, h):
    k1 = f(y)
    k2 = f(y + h * k1 / 3)
    k3 = f(y + h * (k2 - k1 / 3))
    k4 = f(y + h * (k1 - k2 + k3))
    return y + (k1 + 3 * (k2 + k3) + k4) * h / 8


def plan(tp):
    """-> per observed point (euler, number of RK4 steps, t_i - prev_t), as python numbers"""
    L = len(tp)
    t = [float(v) for v in tp]
    minimum_step = (t[-1] - t[0]) / 50
    out = []
    for i in range(L):
        prev = t[i + 1] if i + 1 < L else t[-1] + 0.01
        gap = prev - t[i]
        out.append((gap < minimum_step, 0 if gap < minimum_step else max(2, int(gap / minimum_step)) - 1, t[i] - prev))
    return out


def gru_update(p, y, s, x):
    cat = torch.cat([y, s, x], -1)
    u = torch.sigmoid(mlp(p, GRU + "update_gate.", cat))
    r = torch.sigmoid(mlp(p, GRU + "reset_gate.", cat))
    new, new_std = mlp(p, GRU + "new_state_net.", torch.cat([y * r, s * r, x], -1)).chunk(2, -1)
    ny = (1 - u) * new + u * y
    ns = (1 - u) * new_std.abs() + u * s
    m = (x[..., x.shape[-1] // 2:].sum(-1, keepdim=True) > 0).to(y.dtype)
    return m * ny + (1 - m) * y, (m * ns + (1 - m) * s).abs()


def encode_odernn(p, x, tp):
    B, L, _ = x.shape
    R = p[GRU + "update_gate.2.weight"].shape[0]
    y, s = torch.zeros(B, R, dtype=x.dtype), torch.zeros(B, R, dtype=x.dtype)
    if L == 1:
        y, s = gru_update(p, y, s, x[:, 0])
    else:
        f = lambda v: mlp(p, ENC_ODE, v)      # noqa: E731
        steps = plan(tp)
        for i in reversed(range(L)):
            euler, n, gap = steps[i]
            if euler:
                y = y + f(y) * gap
            for _ in range(n):
                y = rk4(f, y, gap / n)
            y, s = gru_update(p, y, s, x[:, i])
    mu, sg = mlp(p, ENC + "transform_z0.", torch.cat([y, s], -1)).chunk(2, -1)
    return mu, sg.abs()


def encode_rnn(p, x, tp):
    B, L, _ = x.shape
    H = p[ENC + "gru_rnn.weight_hh_l0"].shape[1]
    dt = torch.cat([(tp[1:] - tp[:-1]).flip(0), torch.zeros(1, dtype=x.dtype)])
    seq = torch.cat([dt[:, None, None].expand(L, B, 1), x.permute(1, 0, 2).flip(0)], -1)
    h = torch.zeros(B, H, dtype=x.dtype)
    for k in range(L):
        gi = F.linear(seq[k], p[ENC + "gru_rnn.weight_ih_l0"], p[ENC + "gru_rnn.bias_ih_l0"])
        gh = F.linear(h, p[ENC + "gru_rnn.weight_hh_l0"], p[ENC + "gru_rnn.bias_hh_l0"])
        ir, iz, inn = gi.chunk(3, -1)
        hr, hz, hn = gh.chunk(3, -1)
        r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
        n = torch.tanh(inn + r * hn)
        h = (1 - z) * n + z * h
    mu, sg = mlp(p, ENC + "hiddens_to_z0.", h).chunk(2, -1)
    return mu, sg.abs()


def forecast(p, tpp, data, tp, mask, eps):
    """p: name -> tensor (any float dtype; the inputs are cast to it); eps (B, latents) or (n, B, latents) -> the forecast (B, Lp, C)"""
    dt = p[DEC + "weight"].dtype
    tpp, data, tp, mask, eps = (torch.as_tensor(v).to(dt) for v in (tpp, data, tp, mask, eps))
    x = torch.cat([data, mask], -1)
    mu, sg = (encode_rnn if ENC + "gru_rnn.weight_ih_l0" in p else encode_odernn)(p, x, tp)
    if eps.dim() == 2:
        eps = eps[None]
    z = mu[None] + eps * sg[None]
    g = lambda v: mlp(p, GEN_ODE, v)      # noqa: E731
    rows = [z]
    for j in range(1, len(tpp)):
        z = rk4(g, z, tpp[j] - tpp[j - 1])
        rows.append(z)
    out = F.linear(torch.stack(rows, 2), p[DEC + "weight"], p[DEC + "bias"])      # (n, B, Lp, C)
    return out.mean(0)


def run(params, tpp, data, tp, mask, eps, upstream, dtype=torch.float64):
    """-> (out, name -> gradient of sum(out * upstream), None for the parameters without one), both as float64 tensors"""
    p = {k: torch.as_tensor(v).detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    out = forecast(p, tpp, data, tp, mask, eps)
    (out * torch.as_tensor(upstream).to(dtype)).sum().backward()
    return out.detach().double(), {k: (None if v.grad is None else v.grad.double()) for k, v in p.items()}
