"""GPU checks of MMF_XAttn_Add's low-rank form (csrc/xrank.hip: the fold, the P projection, the Q kernels -- forward, backward, fused loss +
backward, evaluation -- rank_expand_kernel and the chain rule through xjobs_kernel), run through fusions.MMF_XAttn_Add -- that is, through the
C ABI -- in train mode against oracle.fusion_ref.mmf_xattn_add (+ masked_mse) in float64.  tests/test_xrank_ref.py pins that reference to the
low-rank algebra on the CPU, asserts the route of every case of tests/xrank_cases.py from the predicates of xrank.hip, and holds the inputs to
the conditions they are built for.

Inputs: no parameter is trivial -- in_proj_bias (all three blocks) and out_proj.bias are as large as the products they are added to, so the
bias column of G_h (kw[C] in the score), the b_v column of U_h and the W_res b_out half of b_HO all count; kappa in {0.25, 0.7, 2.0}; every
batch of more than one window has a text-less one; the last variable of `mask` is fully masked; dropout 0 and 0.2 under the Philox masks the
kernels draw (ops.dropout_keep_mask, sites 4 and 5), config.next_seed pinned.  Peaked variants (Y and proj_k.weight times 2 each, gain 4):
scores span +-11 to +-38, softmax rows from flat to 0.99 on one key, none exactly one-hot in float32.
Shapes: xrank_cases.CASES, one per route -- lanes per row 1 / 2 / 4 / 8 on both sides of T = 64 and 128, CM = 8 and 16 at their edges,
scalar and vector load_row, T % 4 in {1, 2, 3} (unaligned drop4), P padded 18 -> 24 and 124 -> 128, 2 and 3 windows per workgroup with a
partial last workgroup (770 and 520 windows), dE by rank_expand_kernel<8> / <16> and by the GEMM, fp32 and bf16 wherever xr_hf holds.
The "_z" hand-over runs at 28 rows (GEMM) and 4140 rows (bf16: seam_p_fwd_kernel, which tests/test_gpu_seam_small.py also holds to float64
on its own at 512 to 2048 rows; dZ by rank_expand_kernel<16>).

Error measure: fp32 per part (xrank_cases.parts_of: per window for Y_out / P / dY / dE; per head block for the q / k / v thirds of in_proj,
proj_q / proj_k / proj_v (rows) and out_proj.weight (columns); else the tensor), max |got - want| / max |want| of the part, floor 1e-6 of the
tensor's largest element (test_xrank_ref.py: no part of any case is that small, so the floor never decides).  The k third of d in_proj_bias
is zero in exact arithmetic and is no part: max |got| <= gradient bar * max |want over in_proj_bias|.  bf16: relative L2 per tensor.
Bars, the project's own, not widened: fp32 1e-4 outputs / 2e-4 gradients, bf16 3e-2 / 4e-2.
Evaluation (forward_metrics, xrank_q_eval_kernel): the five per-variable sums against lib.evaluation's formulas in float64 on the float64
forecast.  The sums are functions of an output held to 1e-4 of its window's maximum, delta_w; so fp32: |d se| <= sum m (2 |t - p| delta_w +
delta_w^2), |d ae| <= sum m delta_w, |d ape| <= sum m delta_w / |t|, each + 1e-6 of the sum of the absolute terms for the float32 terms
themselves (test_gpu_eval.py's yardstick); counts exact.  bf16: relative L2 of each error statistic over the variables <= 3e-2.

The float32 yardstick (the oracle in float32 on the CPU against float64, same measure; test_xrank_ref.py asserts it >= 4x below the fp32
bars): outputs <= 8.4e-7, gradients <= 6.5e-6 (dE, shared_2), peaked 8.3e-7 / 1.2e-5 (d in_proj_bias, long_1).  It is not what limits the
peaked gain: at gain 8 and 16 it still reads at most 1.6e-5, under a third of the 5e-5 it may reach.  The gain is the power of two that
gives the +-15 asked for.  The bf16 floor (the restatement with the operands of the P
product and of its gradient products rounded to bf16; asserted <= half of the bf16 bars) holds on every plain case and on six of the nine
peaked ones; lanes_2, long_2 and long_1 peaked read 1.26, 0.73 and 0.56 of a bar from operand rounding alone and run in fp32 only.

Exact requirements: a text-less window has Y_out == Y * inv bit for bit, inv = 1.f / (1.f + kappa) in float32 -- the kernels' expression
(y + kappa * 0) * inv; dY == up * inv bit for bit on the two-halves route; dE (dZ) == 0; with no text in the batch every parameter gradient
is exactly 0.
Measured on the MI355X, the worst case of each bar class: see MEASURED below.  Mutations: see MUTATIONS."""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xrank_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu
FP32_BARS = (1e-4, 2e-4)         # outputs, gradients
BF16_L2_BARS = (3e-2, 4e-2)
SEED = 777
MEASURED = """worst figure of one run per bar class (fp32: per part; bf16: relative L2 per tensor)
                    fp32 outputs   fp32 gradients                             key bias third   bf16 outputs   bf16 gradients
two halves          1.2e-6         6.8e-6 (d in_proj_weight, lanes_2 peaked)  2.3e-6           2.8e-3         1.9e-2 (d in_proj_bias, long_1, p 0.2)
"_z" hand-over      5.6e-7         3.1e-6 (d in_proj_bias, lanes_2)           6.2e-7           4.4e-3         1.2e-2 (d residual_head.bias, expand_16)
forward_loss        1.9e-7         6.8e-6 (dE, shared_2)                      2.3e-6           3.9e-4         1.4e-2 (d proj_k.weight, cm16_low peaked)
bars                1e-4           2e-4                                       2e-4             3e-2           4e-2
forward_metrics     fp32: 1.5e-3 of the bound derived from the output bar (lanes_2); bf16: 3.0e-3 (long_2) against 3e-2
The fp32 figures are those of the float32 oracle on the CPU: nothing is lost to the fold.  232 cases, under 4 s."""
MUTATIONS = """each applied alone to a scratch copy of csrc/xrank.hip, rebuilt, this file run once (232 cases):
kw[C] dropped from the score in xrank_q_fwd_rows         116 fail: two halves 78 of 80 (all but `degenerate`, whose one key makes the score
                                                         irrelevant), "_z" 8 of 8, forward_metrics 30 of 40; forward_loss (its own kernel) passes
bh[c] (b_HO) left out of delta in xrank_q_fwd_rows       121 fail: two halves 78 of 80, "_z" 8 of 8, forward_metrics 35 of 40
LDS window offset lw * T * PW replaced by 0              11 fail: shared_3 and shared_2 only (the two cases whose workgroups hold more than one
                                                         window): two halves 8 of 8, forward_metrics 3 of 4
drop4's unaligned branch reusing the aligned word        82 fail: every dropout-0.2 run of two halves (39 of 40) and forward_loss (39 of 40) but
                                                         `degenerate` (T = 1, C = 1: every index is aligned), "_z" 4 of 4; no dropout-0 run
`s < T` loosened to `s < 4 * nch`                        NOT run: xrank_q_fwd_kernel is launched with wpb * T * PW floats of LDS, not with
                                                         xq_lds_floats, so the rows T .. 4 nch - 1 of a workgroup's last window lie past its
                                                         own allocation; the read cannot be confirmed in bounds"""
WORST = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _nothing_more_after_a_device_error():
    """a launch that failed on the device leaves the process unusable: end the session rather than launch the remaining cases on it"""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"device error, no further case is launched: {e}", returncode=3)


@pytest.fixture(autouse=True)
def _config_as_found():
    from immtsf import config
    was = (config.precision, config.xattn_rank, config.xattn_fused_loss, config.next_seed)
    config.xattn_rank, config.xattn_fused_loss = True, True
    config.next_seed = lambda: SEED
    try:
        yield
    finally:
        config.precision, config.xattn_rank, config.xattn_fused_loss, config.next_seed = was


def _precisions(variant):
    name, peaked = variant
    on = X.hf("bf16", X.case(name)[1][3]) and not (peaked and name in X.BF16_PEAKED_OFF)
    return ("fp32", "bf16") if on else ("fp32",)


RUNS = [(v, pd, pr) for v in X.VARIANTS for pd in (0.0, 0.2) for pr in _precisions(v)]


def _rid(r):
    return f"{X.vid(r[0])}-p{r[1]}-{r[2]}"


@functools.lru_cache(maxsize=None)
def _keep(name, pd):
    """the masks the kernels draw for SEED at the two sites, (attn (B, H, T, T), out (B, T, C)), or None; kept fractions within 5 sigma"""
    if pd <= 0.0:
        return None
    from immtsf import ops
    _, (B, T, C, d, H), _ = X.case(name)
    res = []
    for site, shape in ((X.SITE_ATTN, (B, H, T, T)), (X.SITE_OUT, (B, T, C))):
        n = math.prod(shape)
        keep = ops.dropout_keep_mask(SEED, site, n, pd, _dev()).cpu()
        assert abs(float(keep.double().mean()) - (1.0 - pd)) <= 5.0 * math.sqrt(pd * (1.0 - pd) / n) + 1e-12, (site, float(keep.double().mean()), n)
        res.append(keep.view(*shape))
    return tuple(res)


@functools.lru_cache(maxsize=None)
def _reference(name, peaked, pd, loss, z=False, no_text=False):
    _, (B, T, C, d, H), _ = X.case(name)
    fn = X.lowrank_reference if not no_text else X.reference          # (equal to 1e-10, test_xrank_ref.py; the restatement also yields P)
    kw = dict(M=torch.zeros(B, 1, dtype=torch.bool)) if no_text else {}
    return fn(X.params(name, peaked), X.inputs(name, peaked), H, X.kappa_of(name), torch.float64, _keep(name, pd), pd, loss,
              po=X.proj_out(name) if z else None, **kw)


def _module(name, peaked, pd, precision):
    from fusions.MMF_XAttn_Add import MMF_XAttn_Add
    from immtsf import ops
    _, (B, T, C, d, H), want = X.case(name)
    m = MMF_XAttn_Add(d, C, d, n_heads_fusion=H, dropout=pd, kappa=X.kappa_of(name))
    m.load_state_dict(X.params(name, peaked))
    m = m.to(_dev()).train()
    m.precision = precision
    assert m._rank(T) and ops.mmf_xrank_pw(T, C, d, H) == want["PW"]          # the low-rank form takes the case, at the row pitch of its route
    return m


def _note(cls, err, what):
    if err > WORST.get(cls, (0.0, ""))[0]:
        WORST[cls] = (err, what)


def _assert_close(label, got, want, precision, C, H, form):
    """every tensor of `want` against `got`: fp32 per part, bf16 relative L2 per tensor; every figure printed before anything is asserted"""
    bad = []
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k, w in want.items():
        g = got[k]
        out = k in X.OUTPUTS
        if precision == "fp32":
            bar = FP32_BARS[0 if out else 1]
            err, where = X.part_error(g, w, X.parts_of(k, w.shape, C, H))
            print(f"{label} {k}: worst part error {err:.2e} ({where}, bar {bar:.0e})")
            if k == X.KEY_BIAS:
                kerr = X.key_bias_error(g, w)
                print(f"{label} {k}: k third {kerr:.2e} of the tensor's largest (bar {bar:.0e})")
                if not kerr < bar:
                    bad.append(f"{k} k third {kerr:.2e}")
                _note(f"{form} fp32 key bias", kerr, label)
        else:
            bar = BF16_L2_BARS[0 if out else 1]
            err, where = X.l2_error(g, w), "L2"
            print(f"{label} {k}: relative L2 {err:.2e} (bar {bar:.0e})")
        _note(f"{form} {precision} {'outputs' if out else 'gradients'}", err, f"{k} {label}")
        if not (torch.isfinite(g).all() and err < bar):
            bad.append(f"{k} {err:.2e} at {where} (bar {bar:.0e})")
    print("WORST", WORST)
    assert not bad, f"{label}: " + "; ".join(bad)


def _grads(m, y, e, lin=None):
    got = {"dY": y.grad.cpu(), "dE": e.grad.cpu()}
    got.update({"g." + k: v.grad.cpu() for k, v in m.named_parameters()})
    if lin is not None:
        got["g.proj_out.weight"], got["g.proj_out.bias"] = lin.weight.grad.cpu(), lin.bias.grad.cpu()
    return got


def _inv(kappa):
    return torch.tensor(1.0) / (torch.tensor(1.0) + torch.tensor(kappa, dtype=torch.float32))


def _p_of(kv, C, H):
    """P without its padding columns, which have to be zero"""
    P, n = kv[0].detach().cpu(), H * (2 * C + 1)
    assert not P[..., n:].any(), "the padding columns of P are not zero"
    return P[..., :n]


def _two_halves(variant, pd, precision, z=False, no_text=False):
    name, peaked = variant
    dev = _dev()
    _, (B, T, C, d, H), _ = X.case(name)
    inp = X.inputs(name, peaked)
    m = _module(name, peaked, pd, precision)
    lin = None
    if z:
        lin = torch.nn.Linear(d, d)
        lin.load_state_dict(dict(zip(("weight", "bias"), X.proj_out(name))))
        lin = lin.to(dev)
    y, e = inp["Y"].to(dev).requires_grad_(True), inp["E"].to(dev).requires_grad_(True)
    M = torch.zeros(B, 1, dtype=torch.bool) if no_text else inp["M"]
    kv = m.project_kv(e, proj=lin)
    out = m(y, e, M.to(dev), kv=kv)
    assert type(out.grad_fn).__name__ == "MMFXRankQFnBackward" and m.last_seed == (SEED if pd > 0 else 0)
    out.backward(inp["up"].to(dev))
    torch.cuda.synchronize()
    got = dict(_grads(m, y, e, lin), Y_out=out.detach().cpu())
    if not no_text:
        got["P"] = _p_of(kv, C, H)
    return got, inp, M.view(B)


def _exact_textless(got, inp, M, kappa, dY=True):
    inv = _inv(kappa)
    for b in torch.nonzero(~M).reshape(-1).tolist()[:4]:
        if "Y_out" in got:
            assert torch.equal(got["Y_out"][b], inp["Y"][b] * inv), f"Y_out of text-less window {b} is not Y * (1.f / (1.f + kappa)) bit for bit"
        if dY:
            assert torch.equal(got["dY"][b], inp["up"][b] * inv), f"dY of text-less window {b} is not up * (1.f / (1.f + kappa)) bit for bit"
    assert not got["dE"][~M].any(), "dE of a text-less window is not exactly 0"


@pytest.mark.parametrize("run", RUNS, ids=_rid)
def test_two_halves_against_float64(run):
    """project_kv (fold, P projection) + forward (xrank_q_fwd_kernel), backward (xrank_q_bwd_kernel, dE by the GEMM or rank_expand_kernel, the
    chain rule through xjobs_kernel): P, Y_out, dY, dE and the eleven parameter gradients"""
    variant, pd, precision = run
    name, peaked = variant
    _, (B, T, C, d, H), _ = X.case(name)
    got, inp, M = _two_halves(variant, pd, precision)
    _exact_textless(got, inp, M, X.kappa_of(name))
    _assert_close(f"halves {_rid(run)}", got, _reference(name, peaked, pd, False), precision, C, H, "halves")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("pd", [0.0, 0.2])
@pytest.mark.parametrize("name", X.Z_CASES)
def test_z_handover_against_float64(name, pd, precision):
    """project_kv(Z, proj=proj_out) against the oracle applied to linear(Z, W_po, b_po): the composed fold, P, dZ, d proj_out.weight, d
    proj_out.bias and everything else"""
    _, (B, T, C, d, H), _ = X.case(name)
    got, inp, M = _two_halves((name, False), pd, precision, z=True)
    _exact_textless(got, inp, M, X.kappa_of(name))
    _assert_close(f"z {name}-p{pd}-{precision}", got, _reference(name, False, pd, False, z=True), precision, C, H, "z")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", [c[0] for c in X.CASES if c[1][0] > 1 and X.hf("bf16", c[1][3])])
def test_no_text_at_all_gives_exactly_zero_parameter_gradients(name, precision):
    _, (B, T, C, d, H), _ = X.case(name)
    got, inp, M = _two_halves((name, False), 0.2, precision, no_text=True)
    want = _reference(name, False, 0.2, False, no_text=True)
    assert all(not w.any() for k, w in want.items() if k.startswith("g.") or k == "dE")           # float64 has zeros there
    for k in want:
        if k.startswith("g."):
            assert not got[k].any(), f"{k} is not exactly 0 without text: {float(got[k].abs().max()):.3e}"
    _exact_textless(got, inp, M, X.kappa_of(name))


@pytest.mark.parametrize("run", RUNS, ids=_rid)
def test_forward_loss_against_float64(run):
    """forward_loss with config.xattn_fused_loss (xrank_q_train_kernel: forward, masked MSE and backward in one launch) against oracle +
    masked_mse: the loss, dY, dE and the eleven parameter gradients"""
    from immtsf.ops import backward_unit
    variant, pd, precision = run
    name, peaked = variant
    dev = _dev()
    _, (B, T, C, d, H), _ = X.case(name)
    inp = X.inputs(name, peaked)
    m = _module(name, peaked, pd, precision)
    y, e = inp["Y"].to(dev).requires_grad_(True), inp["E"].to(dev).requires_grad_(True)
    kv = m.project_kv(e)
    loss = m.forward_loss(y, e, inp["M"].to(dev), inp["truth"].to(dev), inp["mask"].to(dev), inp["cnt"].to(dev), kv=kv)
    assert type(loss.grad_fn).__name__ == "MMFXRankQLossFnBackward"
    backward_unit(loss)
    torch.cuda.synchronize()
    got = dict(_grads(m, y, e), loss=loss.detach().reshape(1).cpu())
    want = dict(_reference(name, peaked, pd, True))
    del want["Y_out"], want["P"]                 # (the training launch hands no Y_out back; P is held by the two-halves test)
    _exact_textless(got, inp, inp["M"].view(B), X.kappa_of(name), dY=False)
    _assert_close(f"loss {_rid(run)}", got, want, precision, C, H, "loss")


@pytest.mark.parametrize("run", [r for r in RUNS if r[1] == 0.0], ids=lambda r: f"{X.vid(r[0])}-{r[2]}")
def test_forward_metrics_against_float64(run):
    """forward_metrics in evaluation mode (xrank_q_eval_kernel): the five per-variable sums, added to the accumulator"""
    variant, _, precision = run
    name, peaked = variant
    dev = _dev()
    _, (B, T, C, d, H), _ = X.case(name)
    inp = X.inputs(name, peaked)
    m = _module(name, peaked, 0.2, precision).eval()
    acc = torch.full((5, C), 2.0, dtype=torch.float64, device=dev)
    m.forward_metrics(inp["Y"].to(dev), inp["E"].to(dev), inp["M"].to(dev), inp["truth"].to(dev), inp["mask"].to(dev), acc)
    torch.cuda.synchronize()
    got = acc.cpu() - 2.0
    pred = _reference(name, peaked, 0.0, False)["Y_out"]
    want, want_abs = X.eval_sums(inp["truth"], pred, inp["mask"])
    assert torch.equal(got[3:], want[3:]), "the observation counts are not exact"
    label = f"eval {X.vid(variant)} {precision}"
    if precision == "fp32":
        t, mk = inp["truth"].double(), inp["mask"].double()
        dw = FP32_BARS[0] * pred.abs().amax(dim=(1, 2), keepdim=True)
        nz = (t != 0).double()
        bound = torch.stack([(mk * (2 * (t - pred).abs() * dw + dw * dw)).reshape(-1, C).sum(0), (mk * dw).reshape(-1, C).sum(0),
                             (mk * nz * dw / torch.where(t != 0, t.abs(), torch.ones_like(t))).reshape(-1, C).sum(0)]) + 1e-6 * want_abs[:3]
        err = (got[:3] - want[:3]).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{label}: worst |got - want| / bound {worst:.2e}")
        _note("eval fp32 (of its bound)", worst, label)
        assert bool((err <= bound).all()), (label, err, bound)
    else:
        errs = [X.l2_error(got[k], want[k]) for k in range(3)]
        print(f"{label}: relative L2 of se / ae / ape sums {errs}")
        _note("eval bf16", max(errs), label)
        assert max(errs) < BF16_L2_BARS[0], (label, errs)
    print("WORST", WORST)
