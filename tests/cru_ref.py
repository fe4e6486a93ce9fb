"""float64 restatement of CRU.forecasting (reference models/CRU.py:71-97 over lib/cru_components) for the continuous cell with the single
Linear + softmax coefficient net -- and, for the composed path's other branches, the discrete cell (cru_rkn) with hidden layers in the
coefficient net and the time-sensitive net -- written from the reference's formulation: the loop over all T = L + Lp time points, the masked
Kalman update, the basis mix scattered into banded blocks, torch.matrix_exp of A dt and of the 2 lsd x 2 lsd Van Loan block matrix
[[A, Q], [0, -A^T]] dt, the prior covariance (exp(A dt) Sigma + M2) exp(A dt)^T and its three block diagonals.  Plain torch on the CPU;
pinned to the real reference's goldens in tests/test_cru_ref.py.  `params` is the module's state_dict (names as in the reference)."""
import numpy as np
import torch
import torch.nn.functional as F

CORE = "cru_model_core."
CELL = CORE + "_cru_layer._cell."
ENC = CORE + "_enc._module."
DEC = CORE + "_dec._module."


def band_index(lod, bandwidth):
    band = np.triu(np.ones([lod, lod]), -bandwidth) * np.tril(np.ones([lod, lod]), bandwidth)
    idx = np.nonzero(band)      # row-major, as torch.where
    return torch.from_numpy(idx[0]), torch.from_numpy(idx[1])


def variance(x, kind, cell=False):
    if kind == "exp":
        return torch.exp(x)
    if kind == "relu":
        return torch.clamp(x, min=0)
    if kind == "square":
        return x * x
    if kind == "abs":
        return x.abs()
    if cell:
        return torch.log(torch.exp(x) + 1.0)
    assert kind == "elup1", kind
    return torch.where(x < 0, torch.exp(x), x + 1.0)


def dead_names(names):
    """the parameters forecasting() never reads: the decoder's variance head"""
    return {k for k in names if k.startswith(DEC + "_hidden_layers_var.") or k.startswith(DEC + "_out_layer_var.")}


def _stack(p, prefix, h):
    for i in (0, 3, 6):
        h = torch.relu(F.linear(h, p[f"{prefix}.{i}.weight"], p[f"{prefix}.{i}.bias"]))
        h = F.layer_norm(h, h.shape[-1:], p[f"{prefix}.{i + 2}.weight"], p[f"{prefix}.{i + 2}.bias"], 1e-5)
    return h


def coefficients(p, mean, delta, t_sensitive, hidden_act):
    """the coefficient net: Linear (+ activation) per hidden layer, Linear, softmax; a time-sensitive net also reads the step's dt"""
    x = torch.cat([mean, delta[:, None]], 1) if t_sensitive else mean
    idx = sorted(int(k[len(CELL + "_coefficient_net."):].split(".")[0]) for k in p if k.startswith(CELL + "_coefficient_net.") and
                 k.endswith(".weight"))
    for i in idx:
        x = F.linear(x, p[f"{CELL}_coefficient_net.{i}.weight"], p[f"{CELL}_coefficient_net.{i}.bias"])
        if i != idx[-1]:
            x = getattr(torch, hidden_act.lower())(x)
    return torch.softmax(x, -1)[:, :, None]


def forecast(p, tpp, data, tp, mask, bandwidth, enc_var="square", trans_var="elup1", norms=None, rkn=False, t_sensitive=False,
             hidden_act=None):
    """p: name -> tensor (any float dtype; the inputs are cast to it) -> the forecast (B, Lp, C).  norms: a list that receives, per
    predict, the (B,) 1-norms of A dt.  rkn: the discrete cell (RKNCell._predict, CRUCell.py:316-347): the transition matrix is I + the
    basis mix, applied as it stands, dt read by a time-sensitive coefficient net only"""
    dt = p[CORE + "_log_icu"].dtype
    tpp, data, tp = tpp.to(dt), data.to(dt), tp.to(dt)
    B, L, C = data.shape
    Lp = tpp.shape[1]
    lod = p[CORE + "_log_icu"].shape[1]
    lsd = 2 * lod
    t = torch.cat([tp, tpp], 1)
    obs = torch.cat([data, torch.zeros(B, Lp, C, dtype=dt)], 1)
    valid = torch.cat([mask.bool().any(-1), torch.zeros(B, Lp, dtype=torch.bool)], 1)
    h = _stack(p, ENC + "_hidden_layers", obs.reshape(B * (L + Lp), C))
    h = h / h.norm(dim=-1, keepdim=True).clamp(min=1e-8)
    y = F.linear(h, p[ENC + "_mean_layer.weight"], p[ENC + "_mean_layer.bias"]).view(B, L + Lp, lod)
    yv = variance(F.linear(h, p[ENC + "_log_var_layer.weight"], p[ENC + "_log_var_layer.bias"]), enc_var).view(B, L + Lp, lod)
    i0, i1 = band_index(lod, bandwidth)
    q = variance(p[CELL + "_log_transition_noise"], trans_var, cell=True)
    Q = torch.diag_embed(q.repeat(B, 1))
    mean = torch.zeros(1, lsd, dtype=dt).expand(B, lsd)
    cu = torch.log(torch.exp(p[CORE + "_log_icu"]) + 1.0).expand(B, lod)
    cl = torch.log(torch.exp(p[CORE + "_log_icl"]) + 1.0).expand(B, lod)
    cs = torch.zeros(B, lod, dtype=dt)
    T = L + Lp
    posts = []
    for i in range(T):
        den = cu + yv[:, i]
        qu, ql = cu / den, cs / den
        res = y[:, i] - mean[:, :lod]
        v = valid[:, i, None]
        mean = torch.where(v, mean + torch.cat([qu * res, ql * res], -1), mean)
        cu, cl, cs = torch.where(v, (1 - qu) * cu, cu), torch.where(v, cl - ql * cs, cl), torch.where(v, (1 - qu) * cs, cs)
        posts.append(mean)
        if i == T - 1:
            break
        d = (t[:, i + 1] - t[:, i])[:, None, None]
        c = coefficients(p, mean, d[:, 0, 0], t_sensitive, hidden_act)
        blocks = []
        for name in ("_tm_11_basis", "_tm_12_basis", "_tm_21_basis", "_tm_22_basis"):
            flat = (c * p[CELL + name]).sum(1)
            tm = torch.zeros(B, lod, lod, dtype=dt)
            tm[:, i0, i1] = flat
            if rkn and name in ("_tm_11_basis", "_tm_22_basis"):
                tm = tm + torch.eye(lod, dtype=dt)
            blocks.append(tm)
        if rkn:
            t11, t12, t21, t22 = blocks
            mv = lambda m, v: (m @ v[..., None])[..., 0]      # noqa: E731
            mu, ml = mean[:, :lod], mean[:, lod:]
            mean = torch.cat([mv(t11, mu) + mv(t12, ml), mv(t21, mu) + mv(t22, ml)], -1)
            ncu = mv(t11 * t11, cu) + 2.0 * mv(t11 * t12, cs) + mv(t12 * t12, cl) + q[..., :lod]
            ncl = mv(t21 * t21, cu) + 2.0 * mv(t21 * t22, cs) + mv(t22 * t22, cl) + q[..., lod:]
            cs = mv(t21 * t11, cu) + mv(t22 * t11, cs) + mv(t21 * t12, cs) + mv(t22 * t12, cl)
            cu, cl = ncu, ncl
            continue
        A = torch.cat([torch.cat(blocks[:2], -1), torch.cat(blocks[2:], -1)], -2)
        if norms is not None:
            norms.append((A * d).detach().abs().sum(-2).max(-1).values)
        eA = torch.matrix_exp(A * d)
        Sigma = torch.cat([torch.cat([torch.diag_embed(cu), torch.diag_embed(cs)], -1),
                           torch.cat([torch.diag_embed(cs), torch.diag_embed(cl)], -1)], -2)
        Bm = torch.cat([torch.cat([A, Q], -1), torch.cat([torch.zeros_like(Q), -A.transpose(-2, -1)], -1)], -2)
        M2 = torch.matrix_exp(Bm * d)[:, :lsd, lsd:]
        prior = (eA @ Sigma + M2) @ eA.transpose(-2, -1)
        mean = (eA @ mean[..., None])[..., 0]
        cu = torch.diagonal(prior[:, :lod, :lod], dim1=-1, dim2=-2)
        cl = torch.diagonal(prior[:, lod:, lod:], dim1=-1, dim2=-2)
        cs = torch.diagonal(prior[:, :lod, lod:], dim1=-1, dim2=-2)
    post = torch.stack(posts, 1)[:, L:]
    out = F.linear(_stack(p, DEC + "_hidden_layers_mean", post.reshape(B * Lp, lsd)), p[DEC + "_out_layer_mean.weight"],
                   p[DEC + "_out_layer_mean.bias"])
    return out.view(B, Lp, C)


def run(params, tpp, data, tp, mask, upstream, bandwidth, enc_var="square", trans_var="elup1", dtype=torch.float64, **cell):
    """-> (out, name -> gradient of sum(out * upstream), None for the parameters without one), both as float64 tensors"""
    p = {k: torch.as_tensor(v).detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    as_t = lambda x: torch.as_tensor(x)      # noqa: E731
    out = forecast(p, as_t(tpp), as_t(data), as_t(tp), as_t(mask), bandwidth, enc_var, trans_var, **cell)
    (out * as_t(upstream).to(dtype)).sum().backward()
    return out.detach().double(), {k: (None if v.grad is None else v.grad.double()) for k, v in p.items()}
