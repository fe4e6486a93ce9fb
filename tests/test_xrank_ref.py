"""CPU checks behind tests/test_gpu_xrank.py (MMF_XAttn_Add's low-rank form, csrc/xrank.hip).  (1) The float64 reference --
oracle.fusion_ref.mmf_xattn_add (+ masked_mse) run in float64 as it stands, under dropout keep masks -- equals the low-rank algebra of
xrank.hip's header restated in float64 (xrank_cases.lowrank_forward: G_h, U_h, W_fold, P = [E | 1] W_fold^T, scores from [Y | 1], b_HO) to
1e-10, outputs and every gradient by autograd, the "_z" composition included.  (2) Every case takes the route it is listed for, by the
predicates of xrank.hip restated in Python.  (3) The same oracle in float32 on the CPU, under the per-part measure, stays >= 4x below the
fp32 bars on every case and variant, and still at two and four times the peaked gain: the gain is set by the span asked for, not by
float32.  (4) The restatement with the
operands of the P product and of its gradient products rounded to bf16 stays at or below half of the bf16 bars on every variant that the GPU
test runs in bf16 (three peaked variants do not, and run in fp32 only: xrank_cases.BF16_PEAKED_OFF).  (5) The inputs have the
properties the GPU test relies on; these are requirements, a case edited out of them fails here."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xrank_cases as X  # noqa: E402

F64_BAR = 1e-10
FP32_BARS = (1e-4, 2e-4)         # outputs, gradients: the GPU test's
BF16_L2_BARS = (3e-2, 4e-2)
P_DROP = 0.2


def _keep(name, p_drop=P_DROP):
    """CPU keep masks of the two dropout sites (the GPU test uses the masks the kernels draw; here any Bernoulli mask serves)"""
    _, (B, T, C, d, H), _ = X.case(name)
    g = torch.Generator().manual_seed(B + 7 * T + 31 * C)
    return (torch.rand(B, H, T, T, generator=g) >= p_drop).double(), (torch.rand(B, T, C, generator=g) >= p_drop).double()


def _figures(got, want, C, H, bars=None):
    """-> {tensor: (error, where)} under the GPU test's fp32 measure; the key bias third by its own rule"""
    out = {}
    for k, w in want.items():
        out[k] = X.part_error(got[k], w, X.parts_of(k, w.shape, C, H))
        if k == X.KEY_BIAS:
            out[k + "[k]"] = (X.key_bias_error(got[k], w), "k third")
    return out


@functools.lru_cache(maxsize=None)
def _ref(name, peaked, loss, dropped, dtype=torch.float64, gain=None):
    _, (B, T, C, d, H), _ = X.case(name)
    p, inp = X.params(name, peaked), X.inputs(name, peaked)
    if gain is not None:             # a peaked variant at another gain than PEAK_GAIN
        p["proj_k.weight"] = p["proj_k.weight"] * (gain / X.PEAK_GAIN)
    return X.reference(p, inp, H, X.kappa_of(name), dtype, _keep(name) if dropped else None, P_DROP if dropped else 0.0, loss)


# ---- (1) the algebra
@pytest.mark.parametrize("loss,dropped", [(False, False), (False, True), (True, True)])
@pytest.mark.parametrize("variant", X.VARIANTS, ids=X.vid)
def test_lowrank_algebra_equals_the_oracle_in_float64(variant, loss, dropped):
    name, peaked = variant
    _, (B, T, C, d, H), _ = X.case(name)
    want = _ref(name, peaked, loss, dropped)
    got = X.lowrank_reference(X.params(name, peaked), X.inputs(name, peaked), H, X.kappa_of(name), torch.float64,
                              _keep(name) if dropped else None, P_DROP if dropped else 0.0, loss)
    assert want["Y_out"].dtype == torch.float64
    for k, w in want.items():
        err = float((got[k] - w).abs().max()) / max(float(w.abs().max()), 1e-300) if float(w.abs().max()) > 0 else float(got[k].abs().max())
        assert err <= F64_BAR, (k, err)


@pytest.mark.parametrize("name", X.Z_CASES)
def test_z_composition_equals_the_oracle_on_the_projected_text_in_float64(name):
    _, (B, T, C, d, H), _ = X.case(name)
    p, inp, po = X.params(name), X.inputs(name), X.proj_out(name)
    want = X.reference(p, inp, H, X.kappa_of(name), keep=_keep(name), p_drop=P_DROP, po=po)
    got = X.lowrank_reference(p, inp, H, X.kappa_of(name), keep=_keep(name), p_drop=P_DROP, po=po)
    assert "g.proj_out.weight" in want and float(want["g.proj_out.weight"].abs().max()) > 0
    for k, w in want.items():
        assert float((got[k] - w).abs().max()) <= F64_BAR * float(w.abs().max()), k


def test_eval_sums_are_lib_evaluation_s_formulas():
    """xrank_cases.eval_sums against the per-variable sums written out element by element (lib/evaluation.py: mse, mae, mape over truth != 0)"""
    inp = X.inputs("lanes_2")
    pred = _ref("lanes_2", False, False, False)["Y_out"]
    s, a = X.eval_sums(inp["truth"], pred, inp["mask"])
    t, m = inp["truth"].double(), inp["mask"].double()
    for c in range(pred.shape[-1]):
        tc, pc, mc = t[..., c].reshape(-1), pred[..., c].reshape(-1), m[..., c].reshape(-1)
        want = [sum(float((x - y) ** 2 * w) for x, y, w in zip(tc, pc, mc)), sum(float(abs(x - y) * w) for x, y, w in zip(tc, pc, mc)),
                sum(float(abs(x - y) / x * w) for x, y, w in zip(tc, pc, mc) if x != 0), float(mc.sum()), float(mc[tc != 0].sum())]
        assert torch.allclose(s[:, c], torch.tensor(want, dtype=torch.float64), rtol=1e-12, atol=1e-12)
    assert inp["truth"][0, 0, 0] == 0 and inp["mask"][0, 0, 0] == 1 and bool((a >= s.abs() - 1e-12).all())


# ---- (2) routes
def test_every_case_takes_the_route_it_is_listed_for():
    for name, shape, want in X.CASES:
        B, T, C, d, H = shape
        assert X.supported(T, C, d, H), name
        got = X.route(shape)
        for k, v in want.items():
            assert got[k] == v, (name, k, got[k], v)
    seen = {(r["parts"]) for _, _, r in X.CASES}
    assert seen == {1, 2, 4, 8}
    # the bands of lanes per row, both sides of each edge, while a workgroup holds one window
    for T, parts in ((4, 1), (5, 2), (12, 2), (13, 4), (28, 4), (29, 8), (32, 8), (33, 4), (64, 4), (65, 2), (128, 2), (129, 1)):
        assert X.parts_lanes(2, T, 4, 1) == parts, T
    assert {r["CM"] for _, _, r in X.CASES} == {8, 16} and {r["wpb"] for _, _, r in X.CASES} == {1, 2, 3}
    assert {r["expand"] for _, _, r in X.CASES} == {0, 8, 16} and {r["vec"] for _, _, r in X.CASES} == {True, False}
    assert X.case("cm16_high")[1][2] == 15 and not X.supported(9, 16, 64, 4)              # C's limit
    assert X.pw_of(15, 4) == 128 and not X.supported(9, 15, 65, 5)                        # the PW limit is not crossed (and H <= 4)
    assert X.pw_of(4, 2) == 24 and 2 * 9 == 18                                            # padding of H (2C+1) up to PW
    assert any(s[1] % 4 == 3 for _, s, _ in X.CASES) and any(s[1] % 4 == 2 for _, s, _ in X.CASES)      # unaligned drop4 (base = ... * T)
    # the partial last workgroup, and the row counts on both sides of rank_expand's 4096
    assert X.route(X.case("shared_3")[1])["last"] == 2 and 770 * 5 < 4096 <= 520 * 8 and 180 * 23 >= 4096
    # bf16: which cases round the P product's operands; the "_z" cases sit on both sides of the skinny forward product
    assert [X.hf("bf16", c[1][3]) for c in X.CASES] == [False] + [True] * 12
    zs = [X.seam_p_fwd(X.case(n)[1][0] * X.case(n)[1][1], X.case(n)[1][3], X.route(X.case(n)[1])["PW"]) for n in X.Z_CASES]
    assert zs == [False, True]


# ---- (3) the float32 yardstick
YARD = {}


@pytest.mark.parametrize("loss", [False, True], ids=["up", "loss"])
@pytest.mark.parametrize("variant", X.VARIANTS, ids=X.vid)
def test_float32_oracle_is_four_times_below_the_fp32_bars(variant, loss):
    name, peaked = variant
    _, (B, T, C, d, H), _ = X.case(name)
    want, got = _ref(name, peaked, loss, True), _ref(name, peaked, loss, True, torch.float32)
    bad = []
    for k, (err, where) in _figures(got, want, C, H).items():
        bar = FP32_BARS[0 if k in X.OUTPUTS else 1]
        cls = ("peaked " if peaked else "") + ("outputs" if k in X.OUTPUTS else "gradients")
        YARD[cls] = max(YARD.get(cls, (0.0, ""))[0], err), (k, name) if err >= YARD.get(cls, (0.0, ""))[0] else YARD[cls][1]
        if not err * 4 <= bar:
            bad.append((k, err, where))
    print(f"{X.vid(variant)} loss={loss}: worst so far {YARD}")
    assert not bad, bad


def test_peak_gain_gives_the_span_asked_for_and_float32_is_not_what_limits_it():
    """at PEAK_GAIN the peaked scores reach at least +-10 on every peaked case and +-40 on none (+-15 was asked for: the nearest power of
    two); the float32 oracle is still >= 4x below the fp32 bars at twice and four times that gain, so the yardstick sets no smaller gain"""
    spans, over = [], []
    for name in X.PEAKED:
        _, (B, T, C, d, H), _ = X.case(name)
        spans.append(_scores(name, True).abs().max().item())
        for gain in (2 * X.PEAK_GAIN, 4 * X.PEAK_GAIN):
            want, got = _ref(name, True, False, True, gain=gain), _ref(name, True, False, True, torch.float32, gain=gain)
            over.append(max(err / FP32_BARS[0 if k in X.OUTPUTS else 1] for k, (err, _) in _figures(got, want, C, H).items()))
    print("peaked |score| maxima", [f"{s:.1f}" for s in spans], "worst yardstick / bar at 2x and 4x the gain", [f"{o:.2f}" for o in over])
    assert min(spans) >= 10.0 and max(spans) <= 40.0
    assert max(over) <= 0.25


# ---- (4) the bf16 floor
@pytest.mark.parametrize("loss", [False, True], ids=["up", "loss"])
@pytest.mark.parametrize("variant", [v for v in X.VARIANTS if X.hf("bf16", X.case(v[0])[1][3]) and not (v[1] and v[0] in X.BF16_PEAKED_OFF)], ids=X.vid)
def test_bf16_operand_rounding_stays_below_half_the_bf16_bars(variant, loss):
    name, peaked = variant
    _, (B, T, C, d, H), _ = X.case(name)
    want = _ref(name, peaked, loss, True)
    got = X.lowrank_reference(X.params(name, peaked), X.inputs(name, peaked), H, X.kappa_of(name), torch.float64, _keep(name), P_DROP, loss, bf16=True)
    bad = []
    for k, w in want.items():
        err, bar = X.l2_error(got[k], w), BF16_L2_BARS[0 if k in X.OUTPUTS else 1]
        if not err <= bar / 2:
            bad.append((k, err))
    assert not bad, bad


# ---- (5) conditions on the inputs
def _scores(name, peaked, dtype=torch.float64):
    _, (B, T, C, d, H), _ = X.case(name)
    p, inp = {k: v.to(dtype) for k, v in X.params(name, peaked).items()}, X.inputs(name, peaked)
    Wf, bf, _ = X.fold(p, H)
    Ph = (inp["E"].to(dtype) @ Wf.t() + bf).view(B, T, H, 2 * C + 1)
    s = torch.einsum("btc,bshc->bhts", inp["Y"].to(dtype), Ph[..., :C]) + Ph[..., C].permute(0, 2, 1).unsqueeze(2)
    return s[inp["M"].view(B)]


@pytest.mark.parametrize("variant", X.VARIANTS, ids=X.vid)
def test_inputs_have_the_properties_the_gpu_test_relies_on(variant):
    name, peaked = variant
    _, (B, T, C, d, H), _ = X.case(name)
    p, inp = X.params(name, peaked), X.inputs(name, peaked)
    M = inp["M"].view(B)
    # a text-less window in every batch of more than one window (the batch of one is the degenerate case: its window is live, and the
    # GPU test runs every case once more with no text at all)
    assert bool(M[0]) and (B == 1 or not bool(M[1])) and (B <= 5 or not bool(M[B - 1]))
    assert all(float(v.abs().min()) > 0 for v in p.values()), "a parameter with a zero entry"
    b_in, w_in = p["attn.in_proj_bias"], p["attn.in_proj_weight"]
    for t in range(3):          # each bias block about as large as the products it is added to
        ratio = float(b_in[t * d:(t + 1) * d].pow(2).mean().sqrt()) / (float(w_in[t * d:(t + 1) * d].pow(2).mean().sqrt()) * d ** 0.5)
        assert 0.4 <= ratio <= 2.5, (t, ratio)
    assert 0.5 <= float(p["layer_norm.weight"].min()) and float(p["layer_norm.weight"].max()) <= 1.5 and float(p["layer_norm.bias"].abs().max()) <= 0.3
    assert X.kappa_of(name) in X.KAPPAS and {X.kappa_of(c[0]) for c in X.CASES} == set(X.KAPPAS)
    assert set(inp["mask"].unique().tolist()) <= {0.0, 1.0} and (C == 1 or float(inp["mask"][..., C - 1].sum()) == 0) and float(inp["cnt"][0]) > 0
    # no live row's softmax is exactly one-hot in float32: every probability is a positive float32
    a32 = torch.softmax(_scores(name, peaked, torch.float32), dim=-1)
    assert float(a32.min()) > 0.0
    if peaked:          # near one-hot rows and flat rows side by side
        top = torch.softmax(_scores(name, True), dim=-1).max(dim=-1).values
        assert float(top.max()) > 0.95 and float(top.min()) < 0.5, (float(top.min()), float(top.max()))
    if name == "degenerate":    # LayerNorm over one column: x - mean(x) is exactly 0, nothing in front of it has a gradient
        want = _ref(name, peaked, False, True)
        assert all(not want[k].any() for k in want if k.startswith("g.") and not k.startswith("g.layer_norm")) and not want["dE"].any()
        return
    # every part of every gradient is live: above 1e-6 of its tensor's largest entry, so the floor of the measure never decides.  Exempt: the
    # key bias third (not a part) and dE of the text-less windows (exactly 0 by the block's definition, required exactly of the kernels)
    for loss in (False, True):
        want = _ref(name, peaked, loss, True)
        for k, w in want.items():
            if k in ("Y_out", "loss"):
                continue
            top = float(w.abs().max())
            for label, idx in X.parts_of(k, w.shape, C, H):
                if k == "dE" and not bool(M[idx[0]]):
                    assert not w[idx].any()
                    continue
                assert float(w[idx].abs().max()) > 1e-6 * top, (k, label)
        kb = want[X.KEY_BIAS][d:2 * d]
        assert float(kb.abs().max()) <= 1e-12 * float(want[X.KEY_BIAS].abs().max())       # zero in exact arithmetic


def test_the_measure_sees_a_wrong_head_block_and_a_wrong_bias_column():
    """a head block 1000x smaller than the tensor's largest, wrong by 1 %: invisible to the max norm over the tensor, 1e-2 under parts_of; and
    the score's bias term kw[C] dropped from the restatement moves Y_out by far more than the output bar on these parameters"""
    w = torch.ones(3 * 8, 8, dtype=torch.float64)
    w[4:8] *= 1e-3
    g = w.clone()
    g[4:8] *= 1.01
    assert float((g - w).abs().max() / w.abs().max()) < 2e-5
    err, where = X.part_error(g, w, X.parts_of("g.attn.in_proj_weight", w.shape, 3, 2))
    assert err > 9e-3 and where == "q head 1"
    name = "lanes_2"
    _, (B, T, C, d, H), _ = X.case(name)
    p = {k: v.double() for k, v in X.params(name).items()}
    inp = X.inputs(name)
    good, _ = X.lowrank_forward(p, inp["Y"].double(), inp["E"].double(), inp["M"], H, X.kappa_of(name))
    p0 = dict(p)
    p0["attn.in_proj_bias"] = torch.cat([torch.zeros(d, dtype=torch.float64), p["attn.in_proj_bias"][d:]])      # b_q = 0: the bias row of G_h is 0
    bad, _ = X.lowrank_forward(p0, inp["Y"].double(), inp["E"].double(), inp["M"], H, X.kappa_of(name))
    assert X.part_error(bad, good, X.parts_of("Y_out", good.shape))[0] > 100 * FP32_BARS[0]
