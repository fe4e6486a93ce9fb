"""Inputs, parameters, route predicates and the error measure shared by tests/test_recgr_ref.py (CPU) and tests/test_gpu_recgr.py (GPU):
TTF_RecAvg (csrc/recavg.hip) where the recency weights are NOT all ~1, and MMF_GR_Add (csrc/gru.hip, csrc/gr_train.hip) at hidden sizes of
more than one wave and with saturated gates.  Everything is built on the CPU from seeded generators; plain torch, imports nothing of immtsf.
The float64 reference is oracle.fusion_ref as it stands (pinned by test_recgr_ref.py)."""
import math

import torch

# ================================================================================================ TTF_RecAvg
# (name, T, d, sigma, bf16 route of the backward).  tau and t_hat both live in [0, 1]; sigma 0.05 / 0.3 spreads the weights of a window
# over many decades.  Clamped denominators need a note-to-step gap of several sigma, which [0, 1] only holds at sigma = 0.05: the stale,
# late-clamped and barely-clamped windows exist in the 0.05 cases only.
REC_CASES = [
    ("one_tile", 32, 64, 0.05, "mfma"),            # one 32-step tile, no padded rows
    ("padded_rows", 7, 32, 0.05, "mfma"),          # T < 32: zero-padded rows of dS
    ("d_not_32", 9, 20, 0.3, "fp32"),              # d % 32 != 0
    ("two_step_tiles", 40, 32, 0.05, "fp32"),      # T > 32: the forward's second 32-step pass
    ("wide_d", 5, 260, 0.3, "fp32"),               # d > 256: the forward's second blockIdx.y; d % 32 != 0
]
REC_N = 136            # note slots per window (>= 130 notes + interior masked slots)
REC_DM = 24            # d_m of the cases with input_proj (without: d_m = d)
CLAMP = 1e-6
STALE_GAP_SIGMAS = 12.0      # >= 10 sigma asked; 12: exp(-144) is 0 in float32 (expf underflows below exp(-103.98)), so a stale window's weights
#                              are exactly 0 on the device and its gradient contributions have to be exactly 0
BARELY = (4.57, 4.62)        # t_hat / sigma of the barely-clamped window's steps (its one note at tau = 0): denominator exp(-dl^2) in
#                              [5.3e-10, 8.6e-10]: clamped, below the 1e-9 edge of the forbidden band, and large enough for the clamp's zeroed
#                              dDn branch to matter (the branch is worth denominator / 1e-6 of d log_sigma: 5e-4 to 9e-4, above the fp32 bar)


def rec_bwd_route(precision, T, d, aligned16=True):
    """which backward kernel launch_recavg_bwd takes.  Source: csrc/recavg.hip:260
        if (precision == 1 && mfma_on && T <= 32 && (d % 32) == 0 && lm <= 150 * 1024 && (al & 15) == 0)
    with lm (:257) = 2 * 32 * (d + 8) * 2 + 32 * 40 * 2 + (3 * 32 + 16) * 4 bytes, mfma_on = true (:256)"""
    lm = 2 * 32 * (d + 8) * 2 + 32 * 40 * 2 + (3 * 32 + 16) * 4
    return "mfma" if precision == "bf16" and T <= 32 and d % 32 == 0 and lm <= 150 * 1024 and aligned16 else "fp32"


def rec_case(name):
    return next(c for c in REC_CASES if c[0] == name)


def _u(g, lo, hi, *shape):
    return lo + (hi - lo) * torch.rand(*shape, generator=g)


def _sorted_u(g, lo, hi, n):
    return torch.sort(_u(g, lo, hi, n)).values


def rec_windows(sigma):
    """the window kinds of a case, in batch order"""
    kinds = ["empty", "one", "n65", "n33", "n64", "n131_scattered", "future"]      # (the loud windows, b % 3 == 2: the two of more than two note blocks)
    if sigma <= 0.05:
        kinds += ["barely_clamped", "late_clamped", "stale"]          # (barely_clamped quiet: 1e6 / rstd-fold gradients, it would drown the batch)
    return kinds


# draws whose d log_recency_sigma terms cancelled (kappa > 4 in float64) were drawn again
_REC_RESEED = {("padded_rows", True): 1, ("wide_d", True): 3}


def rec_inputs(name, with_proj, only=None):
    """-> dict(notes (B, N, d_m), tau (B, N), t_hat (B, T), up (B, T, d), kinds).  only: keep that one window kind (a batch of one).
    Note i of a window is  c + a(tau_i) u + noise  (a falls with age), the upstream gradient  s[b, t] g0 + noise  with s > 0: a random
    gradient whose d log_recency_sigma terms do not cancel (test_recgr_ref.py holds kappa = sum |term| / |sum term| <= 4)."""
    _, T, d, sigma, _ = rec_case(name)
    d_m = REC_DM if with_proj else d
    g = torch.Generator().manual_seed(4100 + 97 * T + d + (1 if with_proj else 0) + 10000 * _REC_RESEED.get((name, with_proj), 0))
    kinds = rec_windows(sigma)
    B, N = len(kinds), REC_N
    c, u = torch.randn(d_m, generator=g), torch.randn(d_m, generator=g)
    notes, tau, t_hat = torch.zeros(B, N, d_m), _u(g, 0.0, 1.0, B, N), torch.zeros(B, T)
    lo_t = 0.3 if sigma <= 0.05 else 0.82        # steps late enough for the oldest note (tau = 0) to be >= 1e3 below the newest
    for b, kind in enumerate(kinds):
        live = torch.zeros(N, dtype=torch.bool)
        if kind == "empty":
            t_hat[b] = _sorted_u(g, 0.0, 1.0, T)
            continue
        if kind == "one":
            live[0] = True
            tau[b, 0] = 0.4
            t_hat[b] = _sorted_u(g, 0.3, 0.5, T)
        elif kind in ("n33", "n65"):
            n = int(kind[1:])
            live[:n] = True
            tau[b, :n] = _sorted_u(g, 0.0, 1.0, n)
            tau[b, 0], tau[b, n - 1] = 0.0, 1.0
            if n == 65:          # newest first: the old notes, which carry d log_recency_sigma, sit past the first 32-note block
                tau[b, :n] = tau[b, :n].flip(0)
            t_hat[b] = _sorted_u(g, lo_t, 1.0, T)
        elif kind == "n64":
            live[:64] = True
            hi = 0.6 if sigma <= 0.05 else 0.9
            tau[b, :64] = _sorted_u(g, 0.0, hi, 64)
            tau[b, 0], tau[b, 63] = 0.0, hi
            t_hat[b] = _sorted_u(g, lo_t, min(1.0, hi + 2.0 * sigma), T)
        elif kind == "n131_scattered":       # 131 notes in 136 slots: the masked slots (with a tau of their own) are not a suffix
            live[:] = True
            live[torch.tensor([0, 17, 40, 77, 100])] = False
            idx = torch.nonzero(live).reshape(-1)
            tau[b, idx] = _sorted_u(g, 0.0, 1.0, 131).flip(0)          # newest first, as in n65
            tau[b, idx[0]], tau[b, idx[-1]] = 1.0, 0.0
            t_hat[b] = _sorted_u(g, lo_t, 1.0, T)
        elif kind == "future":               # every note after every step: all weights exactly 1
            live[:12] = True
            tau[b, :12] = _sorted_u(g, 0.6, 1.0, 12)
            t_hat[b] = _sorted_u(g, 0.0, 0.55, T)
        elif kind == "stale":                # every note >= 12 sigma before every step: the clamp is active on every step
            live[:5] = True
            tau[b, :5] = _sorted_u(g, 0.0, 0.05, 5)
            t_hat[b] = _sorted_u(g, 0.05 + STALE_GAP_SIGMAS * sigma + 0.01, 1.0, T)
        elif kind == "late_clamped":         # the early steps sit among the notes, the late ones >= 12 sigma after the last
            live[:9] = True
            tau[b, :9] = _sorted_u(g, 0.1, 0.3, 9)
            tau[b, 8] = 0.3
            ne = (T + 1) // 2
            t_hat[b, :ne] = _sorted_u(g, 0.05, 0.4, ne)
            t_hat[b, ne:] = _sorted_u(g, 0.3 + STALE_GAP_SIGMAS * sigma + 0.01, 1.0, T - ne)
        elif kind == "barely_clamped":
            live[0] = True
            tau[b, 0] = 0.0
            t_hat[b] = _sorted_u(g, BARELY[0] * sigma, BARELY[1] * sigma, T)
        else:
            raise KeyError(kind)
        a = (2.0 * tau[b] - 1.0).unsqueeze(1)
        rows = c + a * u + 0.5 * torch.randn(N, d_m, generator=g)
        notes[b] = torch.where(live.unsqueeze(1), rows, torch.zeros_like(rows))
    g0 = torch.randn(d, generator=g)
    amp = torch.tensor([(1.0, 0.03, 8.0)[b % 3] for b in range(B)]).view(B, 1, 1)      # loud and quiet windows side by side
    up = amp * (_u(g, 0.5, 1.5, B, T, 1) * g0 + 0.25 * torch.randn(B, T, d, generator=g))
    out = dict(notes=notes, tau=tau, t_hat=t_hat, up=up, kinds=kinds)
    if only is not None:
        b = kinds.index(only)
        out = dict(notes=notes[b:b + 1].clone(), tau=tau[b:b + 1].clone(), t_hat=t_hat[b:b + 1].clone(), up=up[b:b + 1].clone(), kinds=[only])
    return out


def rec_params(name, with_proj):
    """state_dict of fusions.TTF_RecAvg for the case, float32: LayerNorm weight and bias are not 1 and 0"""
    _, T, d, sigma, _ = rec_case(name)
    g = torch.Generator().manual_seed(5200 + 31 * T + d + (1 if with_proj else 0))
    p = {"log_recency_sigma": torch.tensor(math.log(sigma), dtype=torch.float32)}
    if with_proj:
        k = REC_DM ** -0.5
        p["input_proj.weight"], p["input_proj.bias"] = _u(g, -k, k, d, REC_DM), _u(g, -k, k, d)
    k = d ** -0.5
    p["proj.weight"], p["proj.bias"] = _u(g, -k, k, d, d), _u(g, -k, k, d)
    p["layer_norm.weight"], p["layer_norm.bias"] = _u(g, 0.5, 1.5, d), _u(g, -0.3, 0.3, d)
    return p


def rec_analysis(p, inp):
    """float64 quantities the conditions are stated in: denom (B, T) un-clamped, live (B, T) = window has text and its step is not
    clamped, spread (B, T) = max / min weight over the window's notes, and the d log_recency_sigma terms (B, N, T)
        term[b, i, t] = dL/dw[b, i, t] * w[b, i, t] * 2 dl[b, i, t]^2          (csrc/recavg.hip:113)
    obtained by autograd on the weights themselves (sum(terms) is d log_recency_sigma: test_recgr_ref.py checks it)."""
    from oracle import fusion_ref as R
    p = {k: v.double() for k, v in p.items()}
    notes, tau, t_hat, up = (inp[k].double() for k in ("notes", "tau", "t_hat", "up"))
    mask = R.note_mask_of(notes)
    V = R.linear(notes, p["input_proj.weight"], p["input_proj.bias"]) if "input_proj.weight" in p else notes
    dl = (t_hat[:, None, :] - tau[:, :, None]).clamp_min(0) / p["log_recency_sigma"].exp()
    w = (torch.exp(-dl * dl) * mask.double()[:, :, None]).requires_grad_(True)
    denom = w.sum(dim=1)
    x = R.layer_norm(torch.einsum("bnt,bnd->btd", w, V) / denom.clamp_min(CLAMP).unsqueeze(-1), p["layer_norm.weight"], p["layer_norm.bias"])
    (R.linear(x, p["proj.weight"], p["proj.bias"]) * up).sum().backward()
    terms = (w.grad * w * 2.0 * dl * dl).detach()
    wd = w.detach()
    big = wd.masked_fill(~mask[:, :, None], 0.0).amax(dim=1)
    small = wd.masked_fill(~mask[:, :, None], float("inf")).amin(dim=1)
    live = mask.any(dim=1, keepdim=True) & (denom.detach() >= CLAMP)
    spread = torch.where(live, big / small.clamp_min(1e-300), torch.ones_like(big))
    return dict(denom=denom.detach(), live=live, spread=spread, terms=terms, mask=mask)


# ================================================================================================ MMF_GR_Add
# (form, (B, T, C, d, Hd)).  "split": the shape is inside gr_split_ok's limits and runs through project_kv / forward_loss;
# "written": runs through forward() (csrc/gru.hip: one thread per hidden unit, Hd rounded up to whole waves)
GR_CASES = [
    ("written", (3, 5, 3, 8, 1)),           # smallest hidden size
    ("written", (4, 33, 5, 16, 17)),        # just outside the split form's limits (Hd = 17)
    ("written", (3, 96, 5, 16, 70)),        # two waves, long T
    ("written", (2, 12, 16, 24, 130)),      # three waves, the last one partly filled
    ("split", (5, 64, 16, 16, 16)),         # the split form's limits on T, C and Hd together (95 KB of LDS: the opt-in above 64 KB)
    ("split", (3, 7, 3, 8, 1)),             # smallest hidden size
    ("split", (6, 33, 6, 64, 6)),           # odd T, C = Hd
]
GR_WEIGHTS = ("default", "saturating")
GR_SITE = 6            # csrc/common.hpp: SITE_GR_OUT, element (b T + t) C + c
GR_KEYS = ("gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0", "residual_head.weight", "residual_head.bias",
           "gate_net.weight", "gate_net.bias", "layer_norm.weight", "layer_norm.bias")


def gr_pw(C, Hd):
    """csrc/gr_train.hip: gr_pw"""
    return (3 * Hd + C + 7) & ~7


def gr_lds_floats(T, C, Hd, PW):
    """csrc/gr_train.hip: gr_lds_floats"""
    return (T * C + T * PW + 3 * Hd * C + C * C + 3 * Hd * Hd + 3 * Hd + C * Hd + 3 * C + 6 * T * Hd + 4 * T * C + T * Hd + 3 * T * Hd + Hd + 3 * Hd +
            2 * T * C + C + 64)


def gr_split_ok(B, T, C, d, Hd):
    """csrc/gr_train.hip: gr_split_ok"""
    return (B > 0 and 1 <= T <= 64 and 1 <= C <= 16 and 1 <= Hd <= 16 and d >= 8 and d % 8 == 0 and
            gr_lds_floats(T, C, Hd, gr_pw(C, Hd)) * 4 <= 150 * 1024)


def gr_id(case):
    return case[0] + "_" + "x".join(map(str, case[1]))


def gr_params(shape, weights):
    """state_dict of fusions.MMF_GR_Add(d, C, Hd), float32.  default: nn.GRU's U(+-1/sqrt(Hd)); saturating: W_ih and W_hh x 3 and biases
    of 1.5 N(0, 1), which puts a good part of r and z outside (0.05, 0.95)"""
    B, T, C, d, Hd = shape
    g = torch.Generator().manual_seed(6300 + 13 * T + 7 * C + d + 1000 * Hd)
    k, I = Hd ** -0.5, C + d
    p = {"gru.weight_ih_l0": _u(g, -k, k, 3 * Hd, I), "gru.weight_hh_l0": _u(g, -k, k, 3 * Hd, Hd),
         "gru.bias_ih_l0": _u(g, -k, k, 3 * Hd), "gru.bias_hh_l0": _u(g, -k, k, 3 * Hd),
         "residual_head.weight": _u(g, -k, k, C, Hd), "residual_head.bias": _u(g, -k, k, C),
         "gate_net.weight": _u(g, -I ** -0.5, I ** -0.5, C, I), "gate_net.bias": _u(g, -I ** -0.5, I ** -0.5, C),
         "layer_norm.weight": _u(g, 0.5, 1.5, C), "layer_norm.bias": _u(g, -0.3, 0.3, C)}
    if weights == "saturating":
        p["gru.weight_ih_l0"] = 3.0 * p["gru.weight_ih_l0"]
        p["gru.weight_hh_l0"] = 3.0 * p["gru.weight_hh_l0"]
        p["gru.bias_ih_l0"] = 1.5 * torch.randn(3 * Hd, generator=g)
        p["gru.bias_hh_l0"] = 1.5 * torch.randn(3 * Hd, generator=g)
    else:
        assert weights == "default"
    return p


# Draws that the bf16 floor condition of test_recgr_ref.py refuses (gr_bf16_floor: the float64 oracle with the operands of the GEMMs
# rounded to bf16 has to stay at or below half of each bf16 bar) were drawn again.  Both were first measured on the MI355X in bf16 mode:
#   written (3, 5, 3, 8, 1), saturating weights, first draw: dW_hh 4.0e-2, db_ih 4.4e-2, db_hh 4.8e-2 relative L2 against the bar of 4e-2
#       (fp32 mode on the same inputs: 7e-6); the emulation gives the same three figures on the CPU, so it is operand rounding into
#       saturated gates of a single hidden unit, not a kernel error
#   split (3, 7, 3, 8, 1), default weights, first draw: db_ih 5.6e-2 against 4e-2 (three numbers, each a sum of 21 signed terms that
#       cancels 12-fold in float64)
_GR_RESEED = {(3, 5, 3, 8, 1): 4, (3, 7, 3, 8, 1): 7}


def gr_inputs(shape, redraw=None):
    """redraw: a draw other than the committed one (0: the first).
    -> dict(Y (B, T, C), E (B, T, d), M (B, 1) bool with window 1 text-less, up (B, T, C), truth, mask (variable 0 unobserved where
    C > 2), cnt (C,))"""
    B, T, C, d, Hd = shape
    g = torch.Generator().manual_seed(7400 + 11 * B + 13 * T + 17 * C + d + 100 * Hd + 10000 * (_GR_RESEED.get(tuple(shape), 0) if redraw is None else redraw))
    amp = torch.tensor([(1.0, 0.03, 8.0)[(b + 1) % 3] for b in range(B)]).view(B, 1, 1)
    Y, E = torch.randn(B, T, C, generator=g), torch.randn(B, T, d, generator=g)
    M = torch.ones(B, 1, dtype=torch.bool)
    M[1] = False
    up = amp * torch.randn(B, T, C, generator=g)
    truth = Y + torch.randn(B, T, C, generator=g)
    mask = (torch.rand(B, T, C, generator=g) > 0.4).float()
    if C > 2:
        mask[..., 0] = 0.0
    mask[0, 0, C - 1] = 1.0
    return dict(Y=Y, E=E, M=M, up=up, truth=truth, mask=mask, cnt=mask.reshape(-1, C).sum(0))


def gr_gates(p, inp):
    """float64 r and z of every (b, t, unit): oracle.fusion_ref.gru_seq's recurrence with the gates kept"""
    from oracle import fusion_ref as R
    p = {k: v.double() for k, v in p.items()}
    x = torch.cat([inp["Y"], inp["E"]], dim=-1).double()
    Hd = p["gru.weight_hh_l0"].shape[1]
    gi = R.linear(x, p["gru.weight_ih_l0"], p["gru.bias_ih_l0"])
    h = x.new_zeros(x.shape[0], Hd)
    rs, zs = [], []
    for t in range(x.shape[1]):
        gh = R.linear(h, p["gru.weight_hh_l0"], p["gru.bias_hh_l0"])
        i_r, i_z, i_n = gi[:, t].chunk(3, dim=-1)
        h_r, h_z, h_n = gh.chunk(3, dim=-1)
        r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
        h = (1.0 - z) * torch.tanh(i_n + r * h_n) + z * h
        rs.append(r)
        zs.append(z)
    return torch.stack(rs, 1), torch.stack(zs, 1)


# ---- bf16 mode restated in float64: what rounding the GEMM operands to bf16 costs, with everything else exact
def _r16(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _GemmLinear(torch.autograd.Function):
    """x w^T with the operands of the products that bf16 mode runs as bf16 GEMMs rounded to bf16 (fp32 accumulation taken as exact):
    fwd: the forward product; dx: g w; dw: g^T x"""

    @staticmethod
    def forward(ctx, x, w, fwd, dx, dw):
        ctx.save_for_backward(x, w)
        ctx.flags = (dx, dw)
        return _r16(x) @ _r16(w).t() if fwd else x @ w.t()

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        dx, dw = ctx.flags
        g2, x2 = g.reshape(-1, g.shape[-1]), x.reshape(-1, x.shape[-1])
        gx = _r16(g) @ _r16(w) if dx else g @ w
        gw = _r16(g2).t() @ _r16(x2) if dw else g2.t() @ x2
        return gx, gw, None, None, None


class _BiasFromRounded(torch.autograd.Function):
    """x + b whose db is the column sum of the bf16 image of the gradient (csrc/gr_train.hip: d b_cat comes out of the GEMM that reads dP16)"""

    @staticmethod
    def forward(ctx, x, b):
        return x + b

    @staticmethod
    def backward(ctx, g):
        return g, _r16(g).reshape(-1, g.shape[-1]).sum(0)


def gr_forward(p, Y, E, M, mode=None, keep=None, p_drop=0.0):
    """oracle.fusion_ref.mmf_gr_add restated with its products pluggable (test_recgr_ref.py holds mode=None to the oracle at 1e-12).
    mode "written": csrc/fusion_blocks_rec_gr.hip in bf16 mode -- gi, gl forward and their dx, dW; dW_hh and dW_r (the recurrence and the
    tail themselves are fp32 kernels).  mode "split": csrc/gr_train.hip -- the text columns of the two maps (P, dE, dW_cat); the Y columns,
    the recurrence, the tail and their gradients are one fp32 kernel."""
    from oracle import fusion_ref as R
    B, T, C = Y.shape
    on = mode is not None
    lin = _GemmLinear.apply
    w_ih, w_g = p["gru.weight_ih_l0"], p["gate_net.weight"]
    if mode == "split":
        gi = _BiasFromRounded.apply(Y @ w_ih[:, :C].t() + lin(E, w_ih[:, C:], True, True, True), p["gru.bias_ih_l0"])
        gl = _BiasFromRounded.apply(Y @ w_g[:, :C].t() + lin(E, w_g[:, C:], True, True, True), p["gate_net.bias"])
    else:
        x = torch.cat([Y, E], dim=-1)
        gi = lin(x, w_ih, on, on, on) + p["gru.bias_ih_l0"]
        gl = lin(x, w_g, on, on, on) + p["gate_net.bias"]
    rec = mode == "written"
    h = Y.new_zeros(B, p["gru.weight_hh_l0"].shape[1])
    outs = []
    for t in range(T):
        gh = lin(h, p["gru.weight_hh_l0"], False, False, rec) + p["gru.bias_hh_l0"]
        i_r, i_z, i_n = gi[:, t].chunk(3, dim=-1)
        h_r, h_z, h_n = gh.chunk(3, dim=-1)
        r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
        h = (1.0 - z) * torch.tanh(i_n + r * h_n) + z * h
        outs.append(h)
    hs = torch.stack(outs, dim=1)
    dn = R.layer_norm(lin(hs, p["residual_head.weight"], False, False, rec) + p["residual_head.bias"], p["layer_norm.weight"], p["layer_norm.bias"])
    dn = R._drop(dn, keep, p_drop)
    g = torch.where(M.view(B, 1, 1), torch.sigmoid(gl), torch.ones_like(gl))
    return g * Y + (1 - g) * (Y + dn)


def gr_bf16_floor(form, shape, weights, redraw=None):
    """-> (outputs, gradients): worst relative L2 per tensor of gr_forward in the form's bf16 mode against float64, on the case's inputs
    (dropout 0) under the loss the GPU test uses for the form"""
    from oracle import fusion_ref as R
    p0, inp = gr_params(shape, weights), gr_inputs(shape, redraw)
    res = []
    for mode in (None, form):
        q = {k: v.double().clone().requires_grad_(True) for k, v in p0.items()}
        Y, E = inp["Y"].double().clone().requires_grad_(True), inp["E"].double().clone().requires_grad_(True)
        out = gr_forward(q, Y, E, inp["M"], mode)
        val = R.masked_mse(inp["truth"].double(), out, inp["mask"].double()) if form == "split" else (out * inp["up"].double()).sum()
        val.backward()
        res.append(({"Y_out": out.detach(), "loss": val.detach().reshape(1)}, dict({"dY": Y.grad, "dE": E.grad}, **{k: v.grad for k, v in q.items()})))
    (o64, g64), (o16, g16) = res
    outs = ("Y_out", "loss") if form == "split" else ("Y_out",)
    return max(l2_error(o16[k], o64[k]) for k in outs), max(l2_error(g16[k], g64[k]) for k in g64)


# ================================================================================================ references (any dtype) and the measure
def rec_reference(p, inp, dtype=torch.float64):
    """oracle.fusion_ref.ttf_recavg forward + backward under inp['up'] -> dict: E_txt, M_txt, g.<parameter>"""
    from oracle import fusion_ref as R
    q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    E, M = R.ttf_recavg(q, inp["notes"].to(dtype), inp["tau"].to(dtype), inp["t_hat"].to(dtype))
    (E * inp["up"].to(dtype)).sum().backward()
    out = {"E_txt": E.detach(), "M_txt": M}
    out.update({"g." + k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in q.items()})
    return out


def gr_reference(p, inp, dtype=torch.float64, keep=None, p_drop=0.0, loss=False):
    """oracle.fusion_ref.mmf_gr_add forward + backward -> dict: Y_out, dY, dE, g.<parameter>; loss=False: under inp['up'];
    loss=True: under oracle masked_mse against inp['truth'] / inp['mask'] (also 'loss')"""
    from oracle import fusion_ref as R
    q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    Y, E = inp["Y"].to(dtype).clone().requires_grad_(True), inp["E"].to(dtype).clone().requires_grad_(True)
    drop = None if keep is None else {"out": keep.to(dtype)}
    out = R.mmf_gr_add(q, Y, E, inp["M"], drop, p_drop)
    res = {"Y_out": out.detach()}
    if loss:
        val = R.masked_mse(inp["truth"].to(dtype), out, inp["mask"].to(dtype))
        val.backward()
        res["loss"] = val.detach().reshape(1)
    else:
        (out * inp["up"].to(dtype)).sum().backward()
    res["dY"], res["dE"] = Y.grad, E.grad
    res.update({"g." + k: v.grad for k, v in q.items()})
    return res


def gr_project_reference(p, inp, dtype=torch.float64):
    """the split form's P (B, T, pw) = E [W_ih[:, C:] ; W_g[:, C:]]^T + [b_ih ; b_g], zero in the padding columns"""
    p = {k: v.to(dtype) for k, v in p.items()}
    E = inp["E"].to(dtype)
    C = inp["Y"].shape[2]
    Hd = p["gru.weight_hh_l0"].shape[1]
    P = E.new_zeros(*E.shape[:2], gr_pw(C, Hd))
    P[..., :3 * Hd] = E @ p["gru.weight_ih_l0"][:, C:].t() + p["gru.bias_ih_l0"]
    P[..., 3 * Hd:3 * Hd + C] = E @ p["gate_net.weight"][:, C:].t() + p["gate_net.bias"]
    return P


def parts_of(name, shape, C=None):
    """the slices of a tensor the error is taken over: [(label, index)].  Per window for E_txt / Y_out / P / dY / dE; per gate block
    (r, z, n) for the GRU's four tensors, W_ih and gate_net.weight additionally split into their Y and text columns; else whole."""
    key = name[2:] if name.startswith("g.") else name
    if key in ("E_txt", "Y_out", "P", "dY", "dE"):
        return [(f"window {b}", (b,)) for b in range(shape[0])]
    if key.startswith("gru."):
        Hd = shape[0] // 3
        blocks = [(gname, slice(i * Hd, (i + 1) * Hd)) for i, gname in enumerate("rzn")]
        if key == "gru.weight_ih_l0":
            return [(f"{gn} {cn}", (rows, cols)) for gn, rows in blocks for cn, cols in (("Y", slice(0, C)), ("text", slice(C, None)))]
        return [(gn, (rows,)) for gn, rows in blocks]
    if key == "gate_net.weight":
        return [("Y", (slice(None), slice(0, C))), ("text", (slice(None), slice(C, None)))]
    return [("all", ())]


def part_error(got, want, parts):
    """worst over the parts of  max |got - want| / max(max |want| of the part, 1e-6 of the tensor's largest |want|)  -> (error, label).
    A part whose bound is 0 (an all-zero tensor) has to be matched exactly; a NaN is an infinite error."""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    floor = 1e-6 * float(want.abs().max()) if want.numel() else 0.0
    worst, where = 0.0, parts[0][0]
    for label, idx in parts:
        g, w = got[idx], want[idx]
        if w.numel() == 0:
            continue
        diff = float((g - w).abs().max())
        bound = max(float(w.abs().max()), floor)
        err = float("inf") if diff != diff else 0.0 if diff == 0.0 else diff / bound if bound > 0 else float("inf")
        if err > worst:
            worst, where = err, label
    return worst, where


def l2_error(got, want):
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    den, num = float(want.norm()), float((got - want).norm())
    return float("inf") if num != num else 0.0 if num == 0.0 else num / den if den > 0 else float("inf")
