"""CPU checks behind tests/test_gpu_recgr.py.  (1) The float64 reference -- oracle.fusion_ref.ttf_recavg, gru_seq and mmf_gr_add, run in float64
as they stand -- equals torch.nn.GRU(...).double() and a written-out restatement of the RecAvg formula to 1e-12.  (2) The inputs of
tests/recgr_cases.py have the properties the GPU test relies on; these are requirements, a case edited out of them fails here: no live
denominator within [1e-9, 1e-3] of the clamp, weights spread over >= 1e3 inside a window on >= 25 % of the live (window, step) pairs,
d log_recency_sigma not a cancelling sum (kappa <= 4), >= 20 % of r and z saturated in the saturating weight sets, every window length and
denominator regime present, the routes and the split predicate as listed.  (3) The same oracle in float32 on the CPU, under the per-part
error measure, stays >= 4x below every fp32 bar of the GPU test.  (4) The measure sees a wrong small part, and the float64 reference with
three mistakes of csrc/recavg.hip written into it misses the GPU test's bars on these inputs (a fourth, dgh's z and n blocks swapped, is
only shown to move dW_hh and db_hh by far more than the bars).  (5) MMF_GR_Add's bf16 mode restated in float64 -- GEMM operands rounded
to bf16 -- stays at or below half of the bf16 bars on every GR case, and reproduces the two device figures for which a first draw was
given up.
One test here needs the built library although it needs no GPU: the split predicate is checked against immtsf.ops.gr_split_pw itself."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recgr_cases as C  # noqa: E402
from oracle import fusion_ref as R  # noqa: E402

F64_BAR = 1e-12
FP32_BARS = (1e-4, 2e-4)         # outputs, gradients: the GPU test's
REC_IDS = [(c[0], wp) for c in C.REC_CASES for wp in (False, True)]
GR_IDS = [(case, w) for case in C.GR_CASES for w in C.GR_WEIGHTS]


def _rel(got, want):
    return float((got.detach() - want.detach()).abs().max() / want.detach().abs().max().clamp_min(1e-300))


def _rid(x):
    return f"{x[0]}_{'proj' if x[1] else 'noproj'}"


def _gid(x):
    return f"{C.gr_id(x[0])}_{x[1]}"


# ---- (1) the reference
@pytest.mark.parametrize("shape,weights", [((3, 9, 4, 6, 5), "default"), ((2, 40, 5, 16, 70), "saturating"), ((3, 5, 3, 8, 1), "saturating")])
def test_gru_seq_and_mmf_gr_add_equal_torch_gru_in_float64(shape, weights):
    B, T, Cc, d, Hd = shape
    p, inp = {k: v.double() for k, v in C.gr_params(shape, weights).items()}, C.gr_inputs(shape)
    gru = torch.nn.GRU(Cc + d, Hd, batch_first=True).double()
    gru.load_state_dict({k[4:]: v for k, v in p.items() if k.startswith("gru.")})
    x = torch.cat([inp["Y"], inp["E"]], -1).double().requires_grad_(True)
    want = gru(x)[0]
    x2 = x.detach().clone().requires_grad_(True)
    q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    got = R.gru_seq(x2, q["gru.weight_ih_l0"], q["gru.weight_hh_l0"], q["gru.bias_ih_l0"], q["gru.bias_hh_l0"])
    assert got.dtype == torch.float64 and _rel(got, want) <= F64_BAR
    up = torch.randn(B, T, Hd, generator=torch.Generator().manual_seed(1)).double()
    (want * up).sum().backward()
    (got * up).sum().backward()
    assert _rel(x2.grad, x.grad) <= F64_BAR
    for k, v in gru.named_parameters():
        assert _rel(q["gru." + k].grad, v.grad) <= F64_BAR, k
    # the block around it, from torch's own modules
    Y, E = inp["Y"].double(), inp["E"].double()
    h = gru(torch.cat([Y, E], -1))[0]
    dn = torch.nn.functional.layer_norm(torch.nn.functional.linear(h, p["residual_head.weight"], p["residual_head.bias"]), (Cc,),
                                        p["layer_norm.weight"], p["layer_norm.bias"], 1e-5)
    g = torch.sigmoid(torch.nn.functional.linear(torch.cat([Y, E], -1), p["gate_net.weight"], p["gate_net.bias"]))
    g = torch.where(inp["M"].view(B, 1, 1), g, torch.ones_like(g))
    out = R.mmf_gr_add(p, Y, E, inp["M"])
    assert out.dtype == torch.float64 and _rel(out, (Y + (1 - g) * dn).detach()) <= F64_BAR
    assert torch.equal(out[1], Y[1])          # the text-less window: an identity in float64


@pytest.mark.parametrize("case", REC_IDS, ids=_rid)
def test_ttf_recavg_equals_the_written_out_formula_in_float64(case):
    """w[b, i, t] = exp(-(max(t_hat - tau, 0) / sigma)^2) over the notes with sum |embedding| > 0; E_raw = sum_i w V / max(sum_i w, 1e-6);
    LayerNorm; proj -- one window at a time, and d log_recency_sigma as the sum of the terms of rec_analysis"""
    p, inp = C.rec_params(*case), C.rec_inputs(*case)
    ref = C.rec_reference(p, inp)
    assert ref["E_txt"].dtype == torch.float64
    q = {k: v.double() for k, v in p.items()}
    sigma = float(q["log_recency_sigma"].exp())
    for b in range(inp["notes"].shape[0]):
        notes, tau, t_hat = inp["notes"][b].double(), inp["tau"][b].double(), inp["t_hat"][b].double()
        idx = torch.nonzero(notes.abs().sum(1) > 0).reshape(-1)
        assert bool(ref["M_txt"][b]) == (idx.numel() > 0)
        V = notes[idx] @ q["input_proj.weight"].t() + q["input_proj.bias"] if case[1] else notes[idx]
        w = torch.exp(-((t_hat[None, :] - tau[idx, None]).clamp_min(0) / sigma) ** 2)              # (n, T)
        raw = torch.einsum("nt,nd->td", w, V) / w.sum(0).clamp_min(1e-6)[:, None]
        x = torch.nn.functional.layer_norm(raw, (raw.shape[1],), q["layer_norm.weight"], q["layer_norm.bias"], 1e-5)
        want = x @ q["proj.weight"].t() + q["proj.bias"]
        assert float((ref["E_txt"][b] - want).abs().max()) <= F64_BAR * float(ref["E_txt"].abs().max()), b
    a = C.rec_analysis(p, inp)
    assert abs(float(a["terms"].sum()) - float(ref["g.log_recency_sigma"])) <= 1e-10 * float(a["terms"].abs().sum())


# ---- (2) the cases
def test_recavg_cases_cover_the_window_lengths_and_routes():
    assert [c[1:3] for c in C.REC_CASES] == [(32, 64), (7, 32), (9, 20), (40, 32), (5, 260)]
    assert {c[3] for c in C.REC_CASES} == {0.05, 0.3}
    for name, T, d, sigma, route in C.REC_CASES:
        assert C.rec_bwd_route("bf16", T, d) == route and C.rec_bwd_route("fp32", T, d) == "fp32", name
        assert C.rec_bwd_route("bf16", T, d, aligned16=False) == "fp32"
    assert [c[0] for c in C.REC_CASES if c[4] == "mfma"] == ["one_tile", "padded_rows"]
    assert any(c[4] == "mfma" and c[3] == 0.05 for c in C.REC_CASES) and any(c[4] == "fp32" and c[3] == 0.05 for c in C.REC_CASES)   # clamps on both kernels
    assert any(T > 32 for _, T, *_ in C.REC_CASES) and any(d > 256 for _, _, d, *_ in C.REC_CASES)
    for case in REC_IDS:
        inp = C.rec_inputs(*case)
        mask = R.note_mask_of(inp["notes"])
        n = dict(zip(inp["kinds"], mask.sum(1).tolist()))
        assert n["empty"] == 0 and n["one"] == 1 and n["n33"] == 33 and n["n64"] == 64 and n["n65"] == 65 and n["n131_scattered"] >= 130
        row = mask[inp["kinds"].index("n131_scattered")]
        assert not row[0] and row[1] and not row[17:].all() and row[-1]        # masked slots in front of and between live ones
        assert float(inp["tau"].min()) >= 0 and float(inp["tau"].max()) <= 1 and float(inp["t_hat"].min()) >= 0 and float(inp["t_hat"].max()) <= 1
        assert float(inp["tau"][~mask].abs().max()) > 0        # a masked slot's tau is not 0: it must not be read as a note at time 0


@pytest.mark.parametrize("case", REC_IDS, ids=_rid)
def test_recavg_cases_hold_their_conditions(case):
    name, T, d, sigma, _ = C.rec_case(case[0])
    p, inp = C.rec_params(*case), C.rec_inputs(*case)
    a = C.rec_analysis(p, inp)
    text = a["mask"].any(1)
    den = a["denom"]
    assert not ((den[text] >= 1e-9) & (den[text] <= 1e-3)).any(), "a denominator near the clamp: float32 and float64 could take different sides"
    dl32 = (inp["t_hat"][:, None, :] - inp["tau"][:, :, None]).clamp_min(0) / p["log_recency_sigma"].exp()           # float32
    den32 = (torch.exp(-dl32 * dl32) * a["mask"].float()[:, :, None]).sum(1)
    assert den32.dtype == torch.float32 and torch.equal(den32[text] < 1e-6, den[text] < 1e-6)
    live = a["live"]
    assert float((a["spread"][live] >= 1e3).double().mean()) >= 0.25
    kappa = float(a["terms"].abs().sum() / a["terms"].sum().abs())
    assert kappa <= 4.0, kappa
    kind = {k: i for i, k in enumerate(inp["kinds"])}
    b = kind["future"]
    w_future = torch.exp(-((inp["t_hat"][b][None] - inp["tau"][b][a["mask"][b]][:, None]).clamp_min(0) / sigma) ** 2)
    assert torch.equal(w_future, torch.ones_like(w_future))          # weights exactly 1
    if sigma <= 0.05:
        b = kind["stale"]
        gap = inp["t_hat"][b].min() - inp["tau"][b][a["mask"][b]].max()
        assert float(gap) >= max(10.0, C.STALE_GAP_SIGMAS) * sigma and (den[b] < 1e-9).all()
        b = kind["late_clamped"]
        ne = (T + 1) // 2
        assert (den[b, :ne] > 1e-3).all() and (den[b, ne:] < 1e-9).all() and ne < T
        b = kind["barely_clamped"]
        assert (den[b] > 2.5e-10).all() and (den[b] < 1e-9).all()
    else:
        assert (den[text] > 1e-3).all()


@pytest.mark.parametrize("case", GR_IDS, ids=_gid)
def test_gr_cases_hold_their_conditions(case):
    (form, shape), weights = case
    B, T, Cc, d, Hd = shape
    assert form == "written" or C.gr_split_ok(*shape)          # (forward() with autograd on runs the block as written at any shape)
    p, inp = C.gr_params(shape, weights), C.gr_inputs(shape)
    assert not inp["M"].all() and inp["M"].any()
    r, z = C.gr_gates(p, inp)
    rz = torch.cat([r, z])
    sat = float(((rz < 0.05) | (rz > 0.95)).double().mean())
    if weights == "saturating":
        assert sat >= 0.20, sat
        assert torch.equal(p["gru.weight_hh_l0"], 3.0 * C.gr_params(shape, "default")["gru.weight_hh_l0"])
    ref = C.gr_reference(p, inp, loss=form == "split")
    assert all(torch.isfinite(v).all() for v in ref.values())
    assert torch.equal(ref["Y_out"][1], inp["Y"][1].double()) and not ref["dE"][1].any()
    if form == "written":
        assert torch.equal(ref["dY"][1], inp["up"][1].double())


def test_gr_cases_are_the_listed_ones_and_the_split_predicate_is_the_librarys():
    assert [s for f, s in C.GR_CASES if f == "written"] == [(3, 5, 3, 8, 1), (4, 33, 5, 16, 17), (3, 96, 5, 16, 70), (2, 12, 16, 24, 130)]
    assert [s for f, s in C.GR_CASES if f == "split"] == [(5, 64, 16, 16, 16), (3, 7, 3, 8, 1), (6, 33, 6, 64, 6)]
    assert C.gr_split_ok(4, 33, 5, 16, 16) and not C.gr_split_ok(4, 33, 5, 16, 17)            # (4, 33, 5, 16, 17): outside through Hd alone
    assert [(-(-Hd // 64), Hd % 64) for _, (_, _, _, _, Hd) in C.GR_CASES[2:4]] == [(2, 6), (3, 2)]      # waves, units in the last one
    from immtsf.ops import gr_split_pw
    for T in (1, 33, 64, 65):
        for Cc in (1, 16, 17):
            for d in (4, 8, 12, 16):
                for Hd in (1, 16, 17):
                    want = C.gr_pw(Cc, Hd) if C.gr_split_ok(1, T, Cc, d, Hd) else 0
                    assert gr_split_pw(T, Cc, d, Hd) == want, (T, Cc, d, Hd)


# ---- (3) the float32 yardstick
def _yardstick(r32, r64, Cc=None):
    outs, grads = {}, {}
    for k, w in r64.items():
        if k == "M_txt":
            assert torch.equal(r32[k], w)
            continue
        (outs if k in ("E_txt", "Y_out", "loss") else grads)[k] = C.part_error(r32[k], w, C.parts_of(k, w.shape, Cc))[0]
    return max(outs.values()), max(grads.values())


@pytest.mark.parametrize("case", REC_IDS, ids=_rid)
def test_float32_oracle_sits_4x_below_the_fp32_bars_recavg(case):
    p, inp = C.rec_params(*case), C.rec_inputs(*case)
    out, grad = _yardstick(C.rec_reference(p, inp, torch.float32), C.rec_reference(p, inp))
    print(f"recavg {_rid(case)}: float32 oracle against float64, worst part: output {out:.2e}, gradient {grad:.2e}")
    assert 4 * out <= FP32_BARS[0] and 4 * grad <= FP32_BARS[1]


@pytest.mark.parametrize("only", ["barely_clamped", "stale"])
@pytest.mark.parametrize("case", [c for c in REC_IDS if C.rec_case(c[0])[3] <= 0.05], ids=_rid)
def test_float32_oracle_sits_4x_below_the_fp32_bars_recavg_window_alone(case, only):
    """the two windows the GPU test also runs alone (the stale one: the tensors it compares there)"""
    p, inp = C.rec_params(*case), C.rec_inputs(*case, only=only)
    r32, r64 = C.rec_reference(p, inp, torch.float32), C.rec_reference(p, inp)
    if only == "stale":
        r32, r64 = ({k: r[k] for k in ("E_txt", "g.proj.weight", "g.proj.bias", "g.layer_norm.bias")} for r in (r32, r64))
    out, grad = _yardstick(r32, r64)
    print(f"recavg {_rid(case)} {only} alone: float32 oracle against float64, worst part: output {out:.2e}, gradient {grad:.2e}")
    assert 4 * out <= FP32_BARS[0] and 4 * grad <= FP32_BARS[1]


@pytest.mark.parametrize("case", GR_IDS, ids=_gid)
def test_float32_oracle_sits_4x_below_the_fp32_bars_gr_add(case):
    (form, shape), weights = case
    p, inp = C.gr_params(shape, weights), C.gr_inputs(shape)
    loss = form == "split"
    out, grad = _yardstick(C.gr_reference(p, inp, torch.float32, loss=loss), C.gr_reference(p, inp, loss=loss), shape[2])
    if loss:
        out = max(out, C.part_error(C.gr_project_reference(p, inp, torch.float32), C.gr_project_reference(p, inp), C.parts_of("P", (shape[0],)))[0])
    print(f"gr_add {_gid(case)}: float32 oracle against float64, worst part: output {out:.2e}, gradient {grad:.2e}")
    assert 4 * out <= FP32_BARS[0] and 4 * grad <= FP32_BARS[1]


# ---- (3b) the bf16 floor
BF16_L2_BARS = (3e-2, 4e-2)      # outputs, gradients: the GPU test's


@pytest.mark.parametrize("case", GR_IDS, ids=_gid)
def test_bf16_operand_rounding_alone_stays_at_half_the_bf16_bars_gr_add(case):
    """what bf16 mode costs by design -- the operands of its GEMMs rounded to bf16, everything else exact, in float64 (recgr_cases.gr_forward)
    -- has to leave half of each bf16 bar to the kernels.  A draw that does not is unfit for the bar and is drawn again, like a draw that
    fails the float32 yardstick."""
    (form, shape), weights = case
    p, inp = {k: v.double() for k, v in C.gr_params(shape, weights).items()}, C.gr_inputs(shape)
    Y, E = inp["Y"].double(), inp["E"].double()
    assert _rel(C.gr_forward(p, Y, E, inp["M"]), R.mmf_gr_add(p, Y, E, inp["M"])) <= F64_BAR        # the restatement is the oracle
    out, grad = C.gr_bf16_floor(form, shape, weights)
    print(f"gr_add {_gid(case)}: bf16 operands in float64 against float64, relative L2: output {out:.2e}, gradient {grad:.2e}")
    assert 2 * out <= BF16_L2_BARS[0] and 2 * grad <= BF16_L2_BARS[1]


def test_bf16_floor_reproduces_what_the_first_draws_measured_on_the_device():
    """the two first draws that were given up (recgr_cases._GR_RESEED): the emulation gives on the CPU what the MI355X gave in bf16 mode --
    written (3, 5, 3, 8, 1) saturating: db_hh 4.81e-2; split (3, 7, 3, 8, 1) default: db_ih 5.62e-2 -- so both were the format's floor
    above the bar of 4e-2, not a kernel's error"""
    assert abs(C.gr_bf16_floor("written", (3, 5, 3, 8, 1), "saturating", redraw=0)[1] - 4.81e-2) < 0.02e-2
    assert abs(C.gr_bf16_floor("split", (3, 7, 3, 8, 1), "default", redraw=0)[1] - 5.62e-2) < 0.02e-2


# ---- (4) the measure, and what it catches
def test_part_error_sees_a_wrong_small_part():
    Hd, I, Cc = 5, 9, 3
    want = torch.randn(3 * Hd, I, generator=torch.Generator().manual_seed(0)).double()
    want[2 * Hd:, :Cc] *= 1e-3                                   # the n gate's Y columns are quiet
    got = want.clone()
    got[2 * Hd, 0] += 1e-4 * float(want[2 * Hd:, :Cc].abs().max())
    parts = C.parts_of("g.gru.weight_ih_l0", want.shape, Cc)
    assert [p_[0] for p_ in parts] == ["r Y", "r text", "z Y", "z text", "n Y", "n text"]
    err, where = C.part_error(got, want, parts)
    assert float((got - want).abs().max() / want.abs().max()) < 1e-6 and 0.9e-4 < err < 1.1e-4 and where == "n Y"
    zero = torch.zeros(4, 3)
    assert C.part_error(zero, zero, C.parts_of("dE", zero.shape)) == (0.0, "window 0")
    assert C.part_error(zero + 1e-30, zero, C.parts_of("dE", zero.shape))[0] == float("inf")
    assert C.part_error(want * float("nan"), want, parts)[0] == float("inf")
    w2 = torch.ones(3, 4).double()
    w2[1] = 0                                                    # an all-zero window in a live tensor: the floor of 1e-6 of the largest element
    g2 = w2.clone()
    g2[1, 0] = 1e-7
    assert abs(C.part_error(g2, w2, C.parts_of("dE", w2.shape))[0] - 0.1) < 1e-9
    assert [p_[0] for p_ in C.parts_of("g.gru.bias_hh_l0", (3 * Hd,))] == ["r", "z", "n"] and len(C.parts_of("g.gate_net.weight", (Cc, I), Cc)) == 2
    assert C.parts_of("g.log_recency_sigma", ()) == [("all", ())]


def test_recavg_mistakes_written_into_float64_miss_the_bars():
    """what three mistakes in csrc/recavg.hip would give, computed in float64 from the terms of rec_analysis: the 2 of 2 dl^2 dropped; the
    un-clamped branch of dDn taken on a clamped step (the barely-clamped window alone); the notes past the first 32 of a window left out of
    d log_recency_sigma (the MFMA backward stopping after its first block)"""
    for case in REC_IDS:
        p, inp = C.rec_params(*case), C.rec_inputs(*case)
        a = C.rec_analysis(p, inp)
        want = float(a["terms"].sum())
        assert abs(0.5 * want - want) / abs(want) > 4e-2
        packed = torch.cumsum(a["mask"].long(), 1) - 1                       # a note's index among its window's live notes
        first = (a["terms"] * (packed < 32).double()[:, :, None]).sum()
        if C.rec_case(case[0])[4] == "mfma":
            assert abs(float(first) - want) / abs(want) > 4e-2, case
    for name in ("one_tile", "padded_rows", "two_step_tiles"):
        for wp in (False, True):
            p, inp = C.rec_params(name, wp), C.rec_inputs(name, wp, only="barely_clamped")
            a = C.rec_analysis(p, inp)
            # the wrong branch adds dDn[t] = -(dE_raw[t] . E_raw[t]) / 1e-6 to every dw[i, t]; with one note E_raw = w V / 1e-6, so the
            # term of (note, t) becomes term (1 - w / 1e-6)
            w = a["denom"][0]
            wrong = float((a["terms"][0].sum(0) * (1.0 - w / C.CLAMP)).sum())
            want = float(a["terms"].sum())
            assert abs(wrong - want) / abs(want) > 1.25 * FP32_BARS[1], (name, wp, abs(wrong - want) / abs(want))


@pytest.mark.parametrize("case", [c for c in GR_IDS if c[0][0] == "written"], ids=_gid)
def test_gru_z_and_n_blocks_of_dgh_swapped_misses_the_bars(case):
    """dgh feeds dW_hh and db_hh: with its z and n blocks swapped those two gradients have their blocks swapped (and the carried dh is
    wrong, which this does not even count)"""
    (form, shape), weights = case
    Hd = shape[4]
    ref = C.gr_reference(C.gr_params(shape, weights), C.gr_inputs(shape))
    for k in ("g.gru.weight_hh_l0", "g.gru.bias_hh_l0"):
        w = ref[k]
        swapped = torch.cat([w[:Hd], w[2 * Hd:], w[Hd:2 * Hd]])
        assert C.part_error(swapped, w, C.parts_of(k, w.shape))[0] > 100 * FP32_BARS[1]
        assert C.l2_error(swapped, w) > 4e-2
