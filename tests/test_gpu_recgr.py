"""GPU checks of TTF_RecAvg (csrc/recavg.hip) and MMF_GR_Add (csrc/gru.hip as written, csrc/gr_train.hip in split form), run through the
drop-in modules fusions.TTF_RecAvg / fusions.MMF_GR_Add -- that is, through the C ABI -- against oracle.fusion_ref in float64 (pinned on the
CPU by tests/test_recgr_ref.py, which also holds the inputs of tests/recgr_cases.py to the conditions they are built for).

RecAvg: tau and t_hat both in [0, 1] at sigma 0.05 / 0.3 (weights over many decades, d log_recency_sigma not a cancelling sum), windows of
0, 1, 33, 64, 65 and 131 notes (masked slots not a suffix), stale / late-clamped / barely-clamped / all-future windows, the five (T, d) of
both sides of the bf16 route predicate, with and without input_proj, fp32 and bf16: E_txt, M_txt (bit-exact) and every parameter gradient.
GR_Add: hidden sizes 1 to 130 (up to three waves), T up to 96, default and saturating weights, dropout 0 and 0.2 under the exported mask, a
text-less window; as written: Y_out, dY, dE, ten parameter gradients; split: project_kv, forward_loss + backward_unit against oracle
mmf_gr_add + masked MSE, and the no-grad output-only launch.

Error measure: per part (recgr_cases.parts_of: per window for E_txt / Y_out / P / dY / dE; per gate block r, z, n for W_ih, W_hh, b_ih,
b_hh, W_ih and gate_net.weight also split into Y and text columns; else the tensor), max |got - want| / max |want| of the part, floor 1e-6
of the tensor's largest element, the worst part reported.  Bars, the project's own, not widened for the finer measure: fp32 with
GEMMs in the path 1e-4 outputs / 2e-4 gradients; bf16 relative L2 per tensor 3e-2 / 4e-2, log_recency_sigma included (kappa <= 4 and three
bf16 roundings of 2^-9 per term bound it by about 2.3e-2).
The float32 yardstick (the same oracle in float32 on the CPU against float64, per part, on these inputs; test_recgr_ref.py asserts it >= 4x
below the fp32 bars): RecAvg outputs <= 2.5e-6, gradients <= 1.6e-6 (the windows run alone included); GR_Add outputs <= 3.3e-7, gradients
<= 8.7e-6 (the Hd = 1 cases, where a gate block is a single number); no case had to be changed for it.
The bf16 floor (MMF_GR_Add's bf16 mode restated in float64, GEMM operands rounded to bf16; test_recgr_ref.py asserts it at or below half
of the bf16 bars on every GR case): outputs <= 2.5e-3, gradients <= 1.7e-2.
Measured on the MI355X, the worst case of each bar class: see MEASURED below.
Of the issue's five mutations, "raw >= 1e-6 always true" is caught for recavg_bwd_kernel only (the barely-clamped window alone in fp32,
where it moves d log_recency_sigma by 5e-4 to 9e-4): in recavg_bwd_mfma_kernel the same branch is worth that much against a bf16 bar
of 4e-2, and on the stale and late-clamped windows E_raw is exactly 0, so both branches give 0.  With no denominator allowed in
[1e-9, 1e-3] no input can tell the two branches of the MFMA kernel apart under its bar.

Exact requirements: a text-less window has Y_out == Y_ts bit for bit, dE == 0 and (as written) dY == the upstream gradient; a stale window
(every note >= 12 sigma before every step: its float32 weights are exactly 0, its float64 gradient contributions below 1e-40) run alone
gives d log_recency_sigma == 0 and d input_proj == 0 exactly."""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recgr_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
FP32_BARS = (1e-4, 2e-4)         # outputs, gradients
BF16_L2_BARS = (3e-2, 4e-2)
OUTPUTS = ("E_txt", "Y_out", "P", "loss", "Y_out_nograd")
SEED = 777
MEASURED = """worst figure of one run per bar class (fp32: per part; bf16: relative L2 per tensor)
                     fp32 outputs   fp32 gradients                     bf16 outputs   bf16 gradients
RecAvg               3.3e-6         1.9e-6 (log_recency_sigma 1.5e-6)  3.5e-3         1.8e-2 (log_recency_sigma, (7, 32) without input_proj)
GR_Add as written    2.3e-7         8.3e-6 (dW_hh r block, Hd = 1)     1.4e-3         1.5e-2 (dW_hh, Hd = 1, saturating)
GR_Add split         3.2e-7         4.2e-5 (db_hh z block, Hd = 1,     2.5e-3         2.6e-2 (dW_hh, Hd = 1, saturating, dropout 0.2)
                                            saturating, dropout 0.2)
bars                 1e-4           2e-4                               3e-2           4e-2"""


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


def _assert_close(label, got, want, precision, Cc=None):
    """every tensor of `want` against `got`: fp32 per part, bf16 relative L2 per tensor; every figure printed before anything is asserted"""
    bad = []
    for k, w in want.items():
        if k == "M_txt":
            continue
        g = got[k]
        out = k in OUTPUTS
        if precision == "fp32":
            bar = FP32_BARS[0 if out else 1]
            err, where = C.part_error(g, w, C.parts_of(k.replace("_nograd", ""), w.shape, Cc))
            print(f"{label} {k}: worst part error {err:.2e} ({where}, bar {bar:.0e})")
        else:
            bar = BF16_L2_BARS[0 if out else 1]
            err, where = C.l2_error(g, w), "L2"
            print(f"{label} {k}: relative L2 {err:.2e} (bar {bar:.0e})")
        if not (torch.isfinite(g).all() and err < bar):
            bad.append(f"{k} {err:.2e} at {where} (bar {bar:.0e})")
    assert not bad, f"{label}: " + "; ".join(bad)


# ================================================================================================ TTF_RecAvg
def _recavg(name, with_proj, precision, only=None):
    from fusions.load_llm import register_d_model
    from fusions.TTF_RecAvg import TTF_RecAvg
    dev = _dev()
    _, T, d, sigma, _ = C.rec_case(name)
    inp = C.rec_inputs(name, with_proj, only)
    register_d_model("RECGR", inp["notes"].shape[2])
    m = TTF_RecAvg("RECGR", 6, recency_sigma=sigma, dropout=0.0, d_txt=d if with_proj else None)
    m.load_state_dict(C.rec_params(name, with_proj))
    m = m.to(dev).train()
    m.precision = precision
    E, M = m(inp["notes"].to(dev), inp["tau"].to(dev), inp["t_hat"].to(dev))
    E.backward(inp["up"].to(dev))
    torch.cuda.synchronize()
    got = {"E_txt": E.detach().cpu(), "M_txt": M.cpu()}
    got.update({"g." + k: v.grad.cpu() for k, v in m.named_parameters()})
    return got


@functools.lru_cache(maxsize=None)
def _rec_reference(name, with_proj, only=None):
    return C.rec_reference(C.rec_params(name, with_proj), C.rec_inputs(name, with_proj, only))


REC_IDS = [(c[0], wp) for c in C.REC_CASES for wp in (False, True)]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("case", REC_IDS, ids=lambda x: f"{x[0]}_{'proj' if x[1] else 'noproj'}")
def test_recavg_against_float64(case, precision):
    """the whole batch of window kinds of a case.  bf16: (32, 64) and (7, 32) take the MFMA backward, the other three the fp32 kernel
    (recgr_cases.rec_bwd_route, asserted on the CPU)"""
    name, with_proj = case
    got, want = _recavg(name, with_proj, precision), _rec_reference(name, with_proj)
    assert got["M_txt"].dtype == torch.bool and torch.equal(got["M_txt"], want["M_txt"])
    assert set(got) == set(want)
    _assert_close(f"recavg {name} proj={with_proj} {precision}", got, want, precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", [c[0] for c in C.REC_CASES if c[3] <= 0.05])
def test_recavg_stale_window_alone_contributes_exactly_nothing(name, precision):
    """every step clamped, every float32 weight exactly 0: d log_recency_sigma and d input_proj of the window are 0, not the residue of
    1e6-fold dS times a weight that should have been 0; E_txt is proj(LayerNorm(0)) = proj(bias)"""
    got, want = _recavg(name, True, precision, "stale"), _rec_reference(name, True, "stale")
    for k in ("g.log_recency_sigma", "g.input_proj.weight", "g.input_proj.bias"):
        assert float(want[k].abs().max()) < 1e-40         # float64: exp(-144) and below
        assert not got[k].any(), f"{k} of an all-clamped window is not exactly 0: {float(got[k].abs().max()):.3e}"
    _assert_close(f"recavg {name} stale alone {precision}", got, {k: want[k] for k in ("E_txt", "g.proj.weight", "g.proj.bias", "g.layer_norm.bias")},
                  precision)


@pytest.mark.parametrize("with_proj", [False, True], ids=["noproj", "proj"])
@pytest.mark.parametrize("name", [c[0] for c in C.REC_CASES if c[3] <= 0.05])
def test_recavg_barely_clamped_window_alone_fp32(name, with_proj):
    """one note, every denominator in (2.5e-10, 1e-9): clamped, and E_raw = w V / 1e-6 is not negligible next to V.  Taking the un-clamped
    branch of dDn here changes d log_recency_sigma by denominator / 1e-6 = 5e-4 to 9e-4 of itself (test_recgr_ref.py), above the bar"""
    got, want = _recavg(name, with_proj, "fp32", "barely_clamped"), _rec_reference(name, with_proj, "barely_clamped")
    _assert_close(f"recavg {name} proj={with_proj} barely clamped alone", got, want, "fp32")


# ================================================================================================ MMF_GR_Add
class _fixed_seed:
    """config.next_seed pinned, so that the float64 reference under the exported mask is shared by the fp32 and the bf16 run"""

    def __enter__(self):
        from immtsf import config
        self.was = config.next_seed
        config.next_seed = lambda: SEED

    def __exit__(self, *exc):
        from immtsf import config
        config.next_seed = self.was


def _keep(shape, pd):
    """the mask the kernels draw for (SEED, SITE_GR_OUT) over (B, T, C), or None; its kept fraction within a binomial 5 sigma of 1 - p"""
    if pd <= 0.0:
        return None
    from immtsf import ops
    B, T, Cc = shape[:3]
    n = B * T * Cc
    keep = ops.dropout_keep_mask(SEED, C.GR_SITE, n, pd, _dev()).cpu()
    assert abs(float(keep.double().mean()) - (1.0 - pd)) <= 5.0 * math.sqrt(pd * (1.0 - pd) / n), (float(keep.double().mean()), n)
    return keep.view(B, T, Cc)


def _module(shape, weights, pd, precision):
    from fusions.MMF_GR_Add import MMF_GR_Add
    B, T, Cc, d, Hd = shape
    m = MMF_GR_Add(d, Cc, Hd, dropout=pd)
    m.load_state_dict(C.gr_params(shape, weights))
    m = m.to(_dev()).train()
    m.precision = precision
    return m


def _grads(m, y, e):
    got = {"dY": y.grad.cpu(), "dE": e.grad.cpu()}
    got.update({"g." + k: v.grad.cpu() for k, v in m.named_parameters()})
    return got


@functools.lru_cache(maxsize=None)
def _gr_reference(shape, weights, pd, loss):
    return C.gr_reference(C.gr_params(shape, weights), C.gr_inputs(shape), keep=_keep(shape, pd), p_drop=pd, loss=loss)


# both weight sets in both precisions.  (In bf16 mode the saturated gates of a single hidden unit amplify the rounding of the GEMM operands:
# a first draw of (3, 5, 3, 8, 1) measured 4.0e-2 to 4.8e-2 on dW_hh, db_ih, db_hh here, one of the split (3, 7, 3, 8, 1) 5.6e-2 on db_ih,
# against 4e-2.  test_recgr_ref.py reproduces both figures on the CPU from operand rounding alone, and holds every case's draw to half
# the bf16 bars under that restatement: see recgr_cases._GR_RESEED.)
GR_VARIANTS = [(w, pd, pr) for w in C.GR_WEIGHTS for pd in (0.0, 0.2) for pr in ("fp32", "bf16")]


@pytest.mark.parametrize("weights,pd,precision", GR_VARIANTS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", [s for f, s in C.GR_CASES if f == "written"], ids=lambda s: "x".join(map(str, s)))
def test_gr_add_as_written_against_float64(shape, weights, pd, precision):
    """forward() with autograd on: concat, the two GEMMs, gru_fwd_kernel / gru_bwd_kernel with one thread per hidden unit (Hd = 70: two
    waves, 130: three) exchanging the hidden state and dgh through LDS, the tail; Y_out, dY, dE and the ten parameter gradients"""
    dev = _dev()
    B, T, Cc, d, Hd = shape
    inp = C.gr_inputs(shape)
    m = _module(shape, weights, pd, precision)
    y, e = inp["Y"].to(dev).requires_grad_(True), inp["E"].to(dev).requires_grad_(True)
    with _fixed_seed():
        out = m(y, e, inp["M"].to(dev))
    assert type(out.grad_fn).__name__ == "MMFGRAddFnBackward"
    out.backward(inp["up"].to(dev))
    torch.cuda.synchronize()
    got = dict(_grads(m, y, e), Y_out=out.detach().cpu())
    want = _gr_reference(shape, weights, pd, False)
    assert set(got) == set(want)
    # the text-less window: float64 has an identity and zeros there, and so must the kernels
    assert torch.equal(got["Y_out"][1], inp["Y"][1]), "Y_out of a text-less window is not Y_ts bit for bit"
    assert not got["dE"][1].any(), "dE of a text-less window is not exactly 0"
    assert torch.equal(got["dY"][1], inp["up"][1]), "dY of a text-less window is not the upstream gradient bit for bit"
    _assert_close(f"gr_add written {shape} {weights} p={pd} {precision}", got, want, precision, Cc)


@pytest.mark.parametrize("weights,pd,precision", GR_VARIANTS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", [s for f, s in C.GR_CASES if f == "split"], ids=lambda s: "x".join(map(str, s)))
def test_gr_add_split_form_against_float64(shape, weights, pd, precision):
    """project_kv (the P half), forward_loss + backward_unit (gr_train_kernel<true>: the Y half, the masked MSE and the backward of both in
    one launch) against oracle mmf_gr_add + oracle masked_mse in float64: P, the loss, dY, dE, the ten parameter gradients; and the
    output-only launch under no_grad (gr_train_kernel<false>)"""
    from immtsf import config
    from immtsf.ops import backward_unit
    dev = _dev()
    B, T, Cc, d, Hd = shape
    inp = C.gr_inputs(shape)
    p = C.gr_params(shape, weights)
    assert config.gr_split
    m = _module(shape, weights, pd, precision)
    y, e = inp["Y"].to(dev).requires_grad_(True), inp["E"].to(dev).requires_grad_(True)
    M = inp["M"].to(dev)
    kv = m.project_kv(e)
    assert kv[0] is not None and kv[0].shape == (B, T, C.gr_pw(Cc, Hd))
    with _fixed_seed():
        loss = m.forward_loss(y, e, M, inp["truth"].to(dev), inp["mask"].to(dev), inp["cnt"].to(dev), kv=kv)
    assert type(loss.grad_fn).__name__ == "MMFGRQLossFnBackward"
    backward_unit(loss)
    torch.cuda.synchronize()
    got = dict(_grads(m, y, e), P=kv[0].detach().cpu(), loss=loss.detach().reshape(1).cpu())
    m.eval()
    with torch.no_grad():
        got["Y_out_nograd"] = m(y.detach(), e.detach(), M, kv=m.project_kv(e.detach())).cpu()
    want = dict(_gr_reference(shape, weights, pd, True))
    del want["Y_out"]                                       # (under the mask; the training launch hands no Y_out back)
    want["P"] = C.gr_project_reference(p, inp)
    want["Y_out_nograd"] = _gr_reference(shape, weights, 0.0, True)["Y_out"]
    assert set(got) == set(want)
    assert torch.equal(got["Y_out_nograd"][1], inp["Y"][1]), "Y_out of a text-less window is not Y_ts bit for bit"
    assert not got["dE"][1].any(), "dE of a text-less window is not exactly 0"
    _assert_close(f"gr_add split {shape} {weights} p={pd} {precision}", got, want, precision, Cc)
