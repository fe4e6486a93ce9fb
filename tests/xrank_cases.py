"""Cases, parameters, inputs, route predicates, the float64 references and the parts of the error measure shared by tests/test_xrank_ref.py
(CPU) and tests/test_gpu_xrank.py (GPU): MMF_XAttn_Add in its low-rank form (csrc/xrank.hip).  Everything is built on the CPU from seeded
generators; plain torch, imports nothing of immtsf.  The float64 reference is oracle.fusion_ref.mmf_xattn_add as it stands; the low-rank
algebra of xrank.hip's header is restated beside it (lowrank_forward) and pinned to it by test_xrank_ref.py.  part_error / l2_error / the
bf16 GEMM restatement are recgr_cases', not copies."""
import math

import torch

from recgr_cases import _GemmLinear, _r16, l2_error, part_error  # noqa: F401  (re-exported to the two test files)

# ================================================================================================ routes, restated from csrc/xrank.hip
XQ_LDS_MAX = 60 * 1024


def pw_of(C, H):
    """xr_dims: row pitch of P, H (2C+1) columns padded to a multiple of 8"""
    return (H * (2 * C + 1) + 7) & ~7


def mask_bytes(T):
    """xq_mask_bytes"""
    return (((T + 3) // 4) + 3) & ~3


def lds_floats(T, C, H):
    """xq_lds_floats: LDS floats of the Q kernels per window"""
    PW = pw_of(C, H)
    masks = H * T * (mask_bytes(T) // 4)
    packed = T * (PW + 2 * C + 2 * H) + masks
    CM, TP = (8 if C <= 8 else 16), (T + 3) & ~3
    padded = H * TP * (2 * CM + 4) + T * (2 * CM + 2 * H) + masks
    return max(packed, padded)


def supported(T, C, d, H):
    """xr_supported"""
    if C < 1 or C > 15 or H > 4 or d % H or (d // H) % 4 or d > 4096 or pw_of(C, H) > 128:
        return False
    return lds_floats(T, C, H) * 4 <= XQ_LDS_MAX


def wpb_of(B, T, C, H):
    """xq_wpb: windows per workgroup"""
    wpb = max(256 // T, 1)
    per = lds_floats(T, C, H) * 4
    while wpb > 1 and per * wpb > XQ_LDS_MAX:
        wpb -= 1
    while wpb > 1 and -(-B // wpb) < 256:
        wpb -= 1
    return wpb


def parts_lanes(B, T, C, H):
    """xq_dims: lanes per (window, row)"""
    wpb, parts, nch = wpb_of(B, T, C, H), 1, (T + 3) // 4
    while parts < 8 and wpb * T * parts * 2 <= 256 and parts * 2 <= nch:
        parts *= 2
    return parts


def rank_expand(rows, d, PW):
    """rank_expand_ok (the operands here are dense and aligned): 0, or the template width of rank_expand_kernel"""
    return PW if rows >= 4096 and PW in (8, 16, 24, 32) and d % 4 == 0 and d <= 1024 else 0


def hf(precision, d):
    """xr_hf: does bf16 mode run the P product on bf16 operands at this width"""
    return precision == "bf16" and d >= 16 and d % 16 == 0


def seam_p_fwd(rows, d, PW):
    """seam_p_fwd_shape_ok (csrc/seam_small.hip): the "_z" forward product's skinny kernel, bf16 mode only"""
    return 512 <= rows < 8192 and 1 <= PW <= 64 and 32 <= d <= 1024 and d % 32 == 0


def route(shape):
    B, T, C, d, H = shape
    PW = pw_of(C, H)
    wpb = wpb_of(B, T, C, H)
    return dict(parts=parts_lanes(B, T, C, H), CM=8 if C <= 8 else 16, PW=PW, wpb=wpb, last=B - (-(-B // wpb) - 1) * wpb, vec=C % 4 == 0,
                expand=rank_expand(B * T, d, PW))


# (name, (B, T, C, d, H), the route the case is for).  Lanes per row as xq_dims gives them: 1 for T <= 4 and T > 128, 2 for T in 5..12 and
# 65..128, 4 for T in 13..28 and 33..64, 8 for T in 29..32 (while windows do not share a workgroup).  Three rows moved off the shapes first
# proposed for them, whose T fell into another band: cm16_low 30 -> 26 (still T % 4 = 2), upper 37: 4 lanes, not 2 -> the 2-lane upper band
# is long_2 (T = 70), and the single lane of a long window is long_1 (T = 129); lanes_8 is the band nobody had listed.
CASES = [
    ("degenerate", (1, 1, 1, 4, 1), dict(parts=1, CM=8, PW=8, wpb=1, vec=False, expand=0)),          # one key, LayerNorm over one column
    ("scalar_row", (5, 3, 3, 16, 1), dict(parts=1, CM=8, PW=8, wpb=1, vec=False, expand=0)),         # T < 5, scalar load_row
    ("lanes_2", (4, 7, 4, 32, 2), dict(parts=2, CM=8, PW=24, wpb=1, vec=True, expand=0)),            # T % 4 = 3: unaligned drop4; 18 -> 24
    ("lanes_4", (3, 13, 8, 32, 4), dict(parts=4, CM=8, PW=72, wpb=1, vec=True, expand=0)),           # CM = 8 at its edge, H = 4, E = 8
    ("cm16_low", (3, 26, 9, 48, 1), dict(parts=4, CM=16, PW=24, wpb=1, vec=False, expand=0)),        # CM = 16 at its lower edge, T % 4 = 2
    ("lanes_8", (3, 30, 9, 48, 1), dict(parts=8, CM=16, PW=24, wpb=1, vec=False, expand=0)),         # T in 29..32: the row_half_mirror sums
    ("cm16_high", (2, 9, 15, 64, 4), dict(parts=2, CM=16, PW=128, wpb=1, vec=False, expand=0)),      # C's limit, 124 -> 128 = the PW limit
    ("upper", (2, 37, 5, 16, 2), dict(parts=4, CM=8, PW=24, wpb=1, vec=False, expand=0)),            # T in 33..64
    ("long_2", (2, 70, 4, 16, 1), dict(parts=2, CM=8, PW=16, wpb=1, vec=True, expand=0)),            # T in 65..128
    ("long_1", (2, 129, 4, 16, 1), dict(parts=1, CM=8, PW=16, wpb=1, vec=True, expand=0)),           # T > 128
    ("shared_3", (770, 5, 5, 16, 2), dict(parts=2, CM=8, PW=24, wpb=3, last=2, vec=False, expand=0)),    # 257 workgroups, 3850 rows
    ("shared_2", (520, 8, 3, 16, 1), dict(parts=2, CM=8, PW=8, wpb=2, last=2, vec=False, expand=8)),     # 4160 rows: rank_expand_kernel<8>
    ("expand_16", (180, 23, 5, 32, 1), dict(parts=4, CM=8, PW=16, wpb=1, vec=False, expand=16)),         # 4140 rows: rank_expand_kernel<16>
]
PEAK_GAIN = 4.0          # the peaked variants: Y and proj_k.weight times 2 each; test_xrank_ref.py: the scores then reach +-11 to +-38 (the +-15
#                          asked for); the float32 oracle is still 4x below the fp32 bars at 8 and 16, so it is not what sets the gain
PEAKED = [c[0] for c in CASES if c[1][0] <= 5 and c[0] != "degenerate"]
# peaked variants whose bf16 floor (operand rounding alone, test_xrank_ref.py) is above half a bf16 bar -- 1.26, 0.73 and 0.56 of a bar: they
# run in fp32 only; the plain variants of the same shapes and the six other peaked ones carry bf16
BF16_PEAKED_OFF = ("lanes_2", "long_2", "long_1")
VARIANTS = [(c[0], False) for c in CASES] + [(n, True) for n in PEAKED]
Z_CASES = ["lanes_2", "expand_16"]       # the "_z" hand-over: 28 rows (the GEMM) and 4140 rows (bf16: seam_p_fwd_kernel; dZ: rank_expand_kernel<16>)
KAPPAS = (0.25, 0.7, 2.0)
SITE_ATTN, SITE_OUT = 4, 5


def case(name):
    return next(c for c in CASES if c[0] == name)


def vid(v):
    return f"{v[0]}{'_peaked' if v[1] else ''}"


def kappa_of(name):
    return KAPPAS[[c[0] for c in CASES].index(name) % 3]


def _gen(name, salt):
    return torch.Generator().manual_seed(7300 + 131 * [c[0] for c in CASES].index(name) + salt)


def params(name, peaked=False):
    """state_dict of fusions.MMF_XAttn_Add, float32.  Weights N(0, 1 / fan_in); every bias N(0, 1) times the rms of its weight's entries times
    sqrt(fan_in), so that a bias term is about as large as the product it is added to; LayerNorm weight in [0.5, 1.5], bias in [-0.3, 0.3]."""
    _, (B, T, C, d, H), _ = case(name)
    g = _gen(name, 1)

    def w(o, i):
        return torch.randn(o, i, generator=g) / math.sqrt(i)

    def b(wt):
        return torch.randn(wt.shape[0], generator=g) * float(wt.pow(2).mean().sqrt()) * math.sqrt(wt.shape[1])

    p = {"proj_q.weight": w(d, C), "proj_k.weight": w(d, d), "proj_v.weight": w(d, d), "attn.in_proj_weight": w(3 * d, d)}
    p["attn.in_proj_bias"] = b(p["attn.in_proj_weight"])
    p["attn.out_proj.weight"] = w(d, d)
    p["attn.out_proj.bias"] = b(p["attn.out_proj.weight"])
    p["residual_head.weight"] = w(C, d)
    p["residual_head.bias"] = b(p["residual_head.weight"])
    p["layer_norm.weight"] = 0.5 + torch.rand(C, generator=g)
    p["layer_norm.bias"] = -0.3 + 0.6 * torch.rand(C, generator=g)
    if peaked:
        p["proj_k.weight"] = p["proj_k.weight"] * (PEAK_GAIN / 2)
    return p


def proj_out(name):
    """the producer's last linear map of the "_z" cases: (weight (d, d), bias (d))"""
    d = case(name)[1][3]
    g = _gen(name, 2)
    return torch.randn(d, d, generator=g) / math.sqrt(d), 0.5 * torch.randn(d, generator=g)


def inputs(name, peaked=False):
    """-> dict(Y (B, T, C), E (B, T, d) (the "_z" cases read it as Z), M (B, 1) bool, up (B, T, C), truth, mask (B, T, C) 0/1, cnt (C)).
    Window 1 (window 0 of a batch of one excepted: see test_xrank_ref.py) has no text; loud and quiet windows sit side by side in `up`;
    variable C - 1 of `mask` is fully masked where C > 1 (its count is 0: the loss averages over the others)."""
    _, (B, T, C, d, H), _ = case(name)
    g = _gen(name, 3)
    Y, E = torch.randn(B, T, C, generator=g), torch.randn(B, T, d, generator=g)
    if peaked:
        Y = Y * 2.0
    M = torch.ones(B, 1, dtype=torch.bool)
    if B > 1:
        M[1] = False
        if B > 5:                  # (large batches: the partial last workgroup ends in a text-less window)
            M[B - 1] = False
    amp = torch.tensor([(1.0, 0.05, 6.0)[b % 3] for b in range(B)]).view(B, 1, 1)
    up = amp * torch.randn(B, T, C, generator=g)
    truth = torch.randn(B, T, C, generator=g)
    truth[0, 0, 0] = 0.0                        # (the evaluation's t != 0 branch)
    mask = (torch.rand(B, T, C, generator=g) < 0.7).float()
    mask[0, 0, 0] = 1.0
    if C > 1:
        mask[..., C - 1] = 0.0
    return dict(Y=Y, E=E, M=M, up=up, truth=truth, mask=mask, cnt=mask.reshape(-1, C).sum(0))


# ================================================================================================ references (any dtype)
def _leaves(p, inp, dtype, po=None):
    q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    Y, E = inp["Y"].to(dtype).clone().requires_grad_(True), inp["E"].to(dtype).clone().requires_grad_(True)
    w = None if po is None else tuple(t.to(dtype).clone().requires_grad_(True) for t in po)
    return q, Y, E, w


def _finish(out, q, Y, E, w, inp, dtype, loss, extra=None):
    from oracle import fusion_ref as R
    res = {"Y_out": out.detach()}
    if loss:
        val = R.masked_mse(inp["truth"].to(dtype), out, inp["mask"].to(dtype))
        val.backward()
        res["loss"] = val.detach().reshape(1)
    else:
        (out * inp["up"].to(dtype)).sum().backward()

    def grad(t):
        return (t.grad if t.grad is not None else torch.zeros_like(t)).detach()
    res["dY"], res["dE"] = grad(Y), grad(E)
    res.update({"g." + k: grad(v) for k, v in q.items()})
    if w is not None:
        res["g.proj_out.weight"], res["g.proj_out.bias"] = grad(w[0]), grad(w[1])
    res.update(extra or {})
    return res


def _drop(keep, dtype):
    return None if keep is None else {"attn": keep[0].to(dtype), "out": keep[1].to(dtype)}


def reference(p, inp, H, kappa, dtype=torch.float64, keep=None, p_drop=0.0, loss=False, po=None, M=None):
    """oracle.fusion_ref.mmf_xattn_add forward + backward -> dict: Y_out, dY, dE (dZ with po), g.<parameter> (and loss).  loss=False: under
    inp['up']; loss=True: under oracle masked_mse.  keep: (attn (B, H, T, T), out (B, T, C)) keep masks.  po: (W_po, b_po), the text side is
    linear(E, W_po, b_po).  M: another M_txt than the case's."""
    from oracle import fusion_ref as R
    q, Y, E, w = _leaves(p, inp, dtype, po)
    Et = E if w is None else R.linear(E, w[0], w[1])
    out = R.mmf_xattn_add(q, Y, Et, inp["M"] if M is None else M, H, kappa, _drop(keep, dtype), p_drop)
    return _finish(out, q, Y, E, w, inp, dtype, loss)


def fold(p, H):
    """the fold of xrank.hip's header: -> (W_fold ((2C+1) H, d), b_fold ((2C+1) H), b_HO (C)); per head the rows of G_h (C + 1: the k
    weights of the C query columns, then the k bias row) and of U_h (C)"""
    d = p["proj_k.weight"].shape[0]
    Eh = d // H
    scale = math.sqrt(1.0 / Eh)
    in_w, in_b = p["attn.in_proj_weight"], p["attn.in_proj_bias"]
    WQf, WKf, WVf = in_w[:d] @ p["proj_q.weight"], in_w[d:2 * d] @ p["proj_k.weight"], in_w[2 * d:] @ p["proj_v.weight"]
    WHO = p["residual_head.weight"] @ p["attn.out_proj.weight"]
    bHO = p["residual_head.weight"] @ p["attn.out_proj.bias"] + p["residual_head.bias"]
    rows = []
    for h in range(H):
        sl = slice(h * Eh, (h + 1) * Eh)
        Aq = torch.cat([WQf[sl], in_b[:d][sl].unsqueeze(1)], 1)                 # (E, C + 1)
        Kk = torch.cat([WKf[sl], in_b[d:2 * d][sl].unsqueeze(1)], 1)            # (E, d + 1)
        Vv = torch.cat([WVf[sl], in_b[2 * d:][sl].unsqueeze(1)], 1)
        rows += [scale * Aq.t() @ Kk, WHO[:, sl] @ Vv]
    Wf = torch.cat(rows, 0)
    return Wf[:, :d], Wf[:, d], bHO


def lowrank_forward(p, Y, E, M, H, kappa, drop=None, p_drop=0.0, bf16=False, po=None):
    """Y_out by the low-rank algebra: P = [E | 1] W_fold^T, scores [Y | 1] . (k weights | k bias), softmax, dropout, the mix of the v
    weights, + b_HO, LayerNorm(C), dropout, the kappa blend; text-less windows return Y / (1 + kappa).  bf16: the operands of the P product
    and of its two gradient products rounded to bf16 (csrc/xrank.hip in bf16 mode), everything else in the tensors' dtype.  -> (Y_out, P)"""
    from oracle import fusion_ref as R
    B, T, C = Y.shape
    Wf, bf, bHO = fold(p, H)
    if po is not None:                  # the "_z" form: W_fold composed with the producer's map
        Wf, bf = Wf @ po[0], Wf @ po[1] + bf
    P = _GemmLinear.apply(E, Wf, bf16, bf16, bf16) + bf
    Ph = P.view(B, T, H, 2 * C + 1)
    kw, kb, vw = Ph[..., :C], Ph[..., C], Ph[..., C + 1:]
    s = torch.einsum("btc,bshc->bhts", Y, kw) + kb.permute(0, 2, 1).unsqueeze(2)
    a = torch.softmax(s, dim=-1)
    if drop is not None:
        a = R._drop(a, drop.get("attn"), p_drop)
    delta = torch.einsum("bhts,bshc->btc", a, vw) + bHO
    dn = R.layer_norm(delta, p["layer_norm.weight"], p["layer_norm.bias"])
    if drop is not None:
        dn = R._drop(dn, drop.get("out"), p_drop)
    dn = torch.where(M.view(B, 1, 1), dn, torch.zeros_like(dn))
    return (Y + kappa * dn) / (1.0 + kappa), P


def lowrank_reference(p, inp, H, kappa, dtype=torch.float64, keep=None, p_drop=0.0, loss=False, bf16=False, po=None):
    """lowrank_forward + backward, the dict of reference() plus P"""
    q, Y, E, w = _leaves(p, inp, dtype, po)
    out, P = lowrank_forward(q, Y, E, inp["M"], H, kappa, _drop(keep, dtype), p_drop, bf16, w)
    return _finish(out, q, Y, E, w, inp, dtype, loss, {"P": P.detach()})


def eval_sums(truth, pred, mask):
    """lib.evaluation's five per-variable sums in float64 -> (sums (5, C), sums of the terms' absolute values): squared error, absolute error,
    absolute percentage error over truth != 0, observations, observations with truth != 0"""
    C = pred.shape[-1]
    t, pr, m = (x.double().reshape(-1, C) for x in (truth, pred, mask))
    nz = t != 0
    dd = (t - pr).abs()
    ape = torch.where(nz, dd / torch.where(nz, t, torch.ones_like(t)), torch.zeros_like(t)) * m
    terms = torch.stack([(t - pr) ** 2 * m, dd * m, ape, m, nz.double() * m])
    return terms.sum(1), terms.abs().sum(1)


# ================================================================================================ the measure
OUTPUTS = ("Y_out", "P", "loss", "sums")
KEY_BIAS = "g.attn.in_proj_bias"


def parts_of(name, shape, C=None, H=1):
    """the slices of a tensor the error is taken over: [(label, index)].  Per window for Y_out / dY / dE / P; per head block of rows for the
    q / k / v thirds of in_proj_weight and in_proj_bias and for proj_q / proj_k / proj_v; per head block of columns for out_proj.weight;
    else the whole tensor.  The k third of in_proj_bias is NOT a part (zero in exact arithmetic: see key_bias_ok)."""
    key = name[2:] if name.startswith("g.") else name
    if key in ("Y_out", "dY", "dE", "P"):
        return [(f"window {b}", (b,)) for b in range(shape[0])]
    if key in ("attn.in_proj_weight", "attn.in_proj_bias"):
        d = shape[0] // 3
        Eh = d // H
        thirds = "qv" if key.endswith("bias") else "qkv"
        return [(f"{t} head {h}", (slice("qkv".index(t) * d + h * Eh, "qkv".index(t) * d + (h + 1) * Eh),)) for t in thirds for h in range(H)]
    if key in ("proj_q.weight", "proj_k.weight", "proj_v.weight"):
        Eh = shape[0] // H
        return [(f"head {h}", (slice(h * Eh, (h + 1) * Eh),)) for h in range(H)]
    if key == "attn.out_proj.weight":
        Eh = shape[1] // H
        return [(f"head {h}", (slice(None), slice(h * Eh, (h + 1) * Eh))) for h in range(H)]
    return [("all", ())]


def key_bias_error(got, want):
    """the k third of d in_proj_bias, zero in exact arithmetic (the softmax does not see a shift of a row's scores):
    max |got| / max |want over the whole in_proj_bias|, to be held to the gradient bar"""
    d = want.shape[0] // 3
    num, den = float(got.double()[d:2 * d].abs().max()), float(want.double().abs().max())
    return 0.0 if num == 0.0 else num / den if den > 0 else float("inf")
