"""CPU checks behind tests/test_gpu_tpatch_stages.py.  (1) The float64 reference of tests/tpatch_stage_cases.py -- oracle graph_stage and
decode on a module that holds only what they read -- equals the whole float32 oracle module (itself pinned to the reference's goldens by
test_oracle_golden.py) to 1e-5, and the written-out restatements that the kink condition and the bf16 reference are taken from equal it to
1e-12.  (2) The ReLU-kink condition: in float64 no pre-activation of any case -- the gates' tanh, the adjacency logits, the mixing layer's
Z, the decoder's two hidden layers, the latter also with bf16 operands -- lies within 1e-5 max |.| of zero; the rows of logits made
exactly 0 are exactly 0 in float32 too.  Nothing is excluded from any comparison.  (3) Every case takes the route it is built for, by
csrc/gcn.hip's and csrc/decoder.hip's launcher arithmetic restated in Python, which is checked against the library's own
immtsf_tpatchgnn_gcn_lds_bytes / _decoder_lds_bytes where the library is built (it loads without a GPU).  (4) The regimes: gate == 0
nodes, saturated gates, uniform and one-hot adjacency rows, uneven walks.  (5) The float32 yardstick: the same oracle in float32 on the
CPU, per part, stays >= 4x below the fp32 bars with ReLU masks identical to float64's.  (6) The bf16 floor: how far the decoder's bf16
mode sits from fp32 by design (printed; the GPU comparison of bf16 mode is made against the restatement, not against plain float64), and
what the one rounding the MFMA backward makes beyond the restatement (g2) costs: at most half the bf16 gradient bar.
One test needs the built library (build() first), though no GPU: the restated LDS arithmetic is checked against the library's own."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tpatch_stage_cases as C  # noqa: E402

F64_BAR = 1e-12
FP32_BARS = (1e-4, 2e-4)         # outputs, gradients: the GPU test's
GRAPH_IDS = [(c[0], s) for c in C.GRAPH_CASES for s in C.GRAPH_SETS]
DEC_IDS = [(c[0], ti) for c in C.DEC_CASES for ti in (False, True)]


def _gid(x):
    return f"{x[0]}_{x[1]}"


def _did(x):
    return f"{x[0]}_{'te_inside' if x[1] else 'te_tensor'}"


def _rel(got, want):
    return float((got.detach() - want.detach()).abs().max() / want.detach().abs().max().clamp_min(1e-300))


# ---- (1) the reference
def test_float64_twin_equals_the_float32_oracle_module():
    """the benchmark dimensions, default parameters: the whole TPatchGNNRef in float32 against the members-only module in float64"""
    from oracle.tpatchgnn_ref import TPatchGNNRef
    _, N, M, D, nd, order = C.graph_case("benchmark")[1]
    E = C.dec_case("benchmark")[1][4]
    args = types.SimpleNamespace(device="cpu", hid_dim=D, C=N, npatch=M, nlayer=1, te_dim=E, n_heads=1, tf_layer=1, node_dim=nd, hop=order,
                                 outlayer="Linear")
    torch.manual_seed(3)
    ref = TPatchGNNRef(args)
    sd = ref.state_dict()
    names = ["nodevec1", "nodevec2", "nodevec_gate1.0.0.weight", "nodevec_gate1.0.0.bias", "nodevec_gate2.0.0.weight", "nodevec_gate2.0.0.bias",
             "nodevec_linear1.0.weight", "nodevec_linear1.0.bias", "nodevec_linear2.0.weight", "nodevec_linear2.0.bias", "gconv.0.mlp.mlp.weight",
             "gconv.0.mlp.mlp.bias"]
    p = {k: sd[n].clone() for k, n in zip(C.GCN_KEYS, names)}
    x, up = C.graph_inputs("benchmark", "default")
    twin, q = C.graph_twin(p, order)
    x64, x32 = x.double().requires_grad_(True), x.clone().requires_grad_(True)
    o64, o32 = twin.graph_stage(0, x64), ref.graph_stage(0, x32)
    (o64 * up.double()).sum().backward()
    (o32 * up).sum().backward()
    assert o64.dtype == torch.float64 and _rel(o32.double(), o64) < 1e-5 and _rel(x32.grad.double(), x64.grad) < 1e-5
    rp = dict(ref.named_parameters())
    for k, n in zip(C.GCN_KEYS, names):
        assert _rel(rp[n].grad.double(), q[k].grad) < 1e-5, k
    # the decoder (hid_dim = 32 = H) and LearnableTE
    dnames = ["decoder.0.weight", "decoder.0.bias", "decoder.2.weight", "decoder.2.bias", "decoder.4.weight", "decoder.4.bias"]
    dp = {k: sd[n].clone() for k, n in zip(C.DEC_KEYS, dnames)}
    inp = C.dec_inputs("benchmark")
    dtwin, dq = C.dec_twin(dp)
    tq = {k: sd[k].double().clone().requires_grad_(True) for k in C.TE_KEYS}
    te32, te64 = ref.LearnableTE(inp["t"].unsqueeze(-1)), C.learnable_te(tq, inp["t"])
    assert te64.dtype == torch.float64 and _rel(te32.double(), te64) < 1e-5
    h64, h32 = inp["h"].double().requires_grad_(True), inp["h"].clone().requires_grad_(True)
    d64, d32 = dtwin.decode(h64, te64), ref.decode(h32, te32)
    (d64 * inp["up"].double()).sum().backward()
    (d32 * inp["up"]).sum().backward()
    assert _rel(d32.double(), d64) < 1e-5 and _rel(h32.grad.double(), h64.grad) < 1e-5
    for k, n in zip(C.DEC_KEYS + C.TE_KEYS, dnames + list(C.TE_KEYS)):
        assert _rel(rp[n].grad.double(), dict(dq, **tq)[k].grad) < 1e-5, k


@pytest.mark.parametrize("case", GRAPH_IDS, ids=_gid)
def test_graph_stage_written_out_equals_the_oracle_in_float64(case):
    name, pset = case
    order = C.graph_case(name)[1][5]
    p = {k: v.double() for k, v in C.graph_params(name, pset).items()}
    x = C.graph_inputs(name, pset)[0].double()
    want = C.graph_reference(name, pset)["out"]
    pre = C.graph_pre(p, x, order)
    assert want.dtype == torch.float64 and _rel(torch.relu(pre["Z"]), want) <= F64_BAR


@pytest.mark.parametrize("case", DEC_IDS, ids=_did)
def test_decoder_written_out_equals_the_oracle_in_float64(case):
    name, te_inside = case
    p, inp = C.dec_params(name), C.dec_inputs(name)
    q = {k: v.double() for k, v in p.items()}
    te = C.learnable_te(p, inp["t"]) if te_inside else inp["te"].double()
    want = C.dec_reference(name, te_inside)["out"]
    assert want.dtype == torch.float64 and _rel(C.dec_forward(q, inp["h"].double(), te), want) <= F64_BAR
    # |w t + b| <= 8, and what the form with te as a tensor is given is LearnableTE to float32 rounding
    arg = inp["t"].double().unsqueeze(-1) * q["te_periodic.weight"][:, 0] + q["te_periodic.bias"]
    assert arg.numel() == 0 or float(arg.abs().max()) <= 8.0
    assert float((inp["te"].double() - C.learnable_te(p, inp["t"])).abs().max()) <= 6e-8 * max(1.0, float(inp["te"].abs().max()))


# ---- (2) the kink condition
@pytest.mark.parametrize("case", GRAPH_IDS, ids=_gid)
def test_graph_cases_hold_the_kink_condition(case):
    name, pset = case
    B, N, M, D, _, order = C.graph_case(name)[1]
    assert B * N * M * D <= 50000
    k = C.graph_kinks(name, pset)
    print(f"graph {_gid(case)}: smallest |pre-activation| / max: " + ", ".join(f"{a} {b:.1e}" for a, b in k.items()))
    assert min(k.values()) >= C.KINK, k
    # the exact zeros among the logits are zeros in float32 as well, and nowhere else than in the rows made so
    p = C.graph_params(name, pset)
    x = C.graph_inputs(name, pset)[0]
    l64 = C.graph_pre({a: b.double() for a, b in p.items()}, x.double(), order)["logits"]
    l32 = C.graph_pre(p, x, order)["logits"]
    assert torch.equal(l64 == 0, l32 == 0)
    rows = [n for n, kind in enumerate(C.node_kinds(N)[0]) if kind == "zero_zero"] if pset == "gates" else []
    zero_rows = torch.nonzero((l64 == 0).any(-1).any(0).any(0)).reshape(-1).tolist()
    assert zero_rows == rows and all(bool((l64[:, :, r] == 0).all()) for r in rows)
    if (name, pset) in C._GRAPH_RESEED:          # a re-drawn case: its first draw did violate the condition
        assert min(C.graph_kinks(name, pset, redraw=0).values()) < C.KINK


@pytest.mark.parametrize("name", [c[0] for c in C.DEC_CASES])
def test_decoder_cases_hold_the_kink_condition(name):
    k = C.dec_kinks(name)
    print(f"decoder {name}: smallest |pre-activation| / max: " + ", ".join(f"{a} {b:.1e}" for a, b in k.items()))
    assert min(k.values()) >= C.KINK, k
    if name in C._DEC_RESEED and name != "e16_atomics":          # (e16_atomics: drawn again for its bf16 floor)
        assert min(C.dec_kinks(name, redraw=0).values()) < C.KINK


# ---- (3) the routes
def test_graph_cases_take_the_routes_they_are_built_for():
    assert [c[1] for c in C.GRAPH_CASES] == [(64, 8, 2, 32, 10, 1), (3, 5, 3, 13, 3, 2), (2, 1, 1, 8, 2, 3), (3, 41, 2, 32, 10, 1),
                                             (130, 3, 2, 64, 10, 1), (345, 3, 3, 8, 2, 1)]
    for name, shape, (lds, walk) in C.GRAPH_CASES:
        r = C.gcn_route(shape)
        assert r["supported"], name
        assert r["bwd_opt_in"] == (lds == "above"), (name, r)
        assert r["walk"] == (walk is not None) and (walk is None or r["per_cu"] == walk), (name, r)
        if walk is not None:         # uneven: a few workgroups do two cells, the rest one
            assert r["cap"] < r["cells"] < r["cap"] + 16 and r["grid"] == r["cap"] and 0 < r["two"] < 16, (name, r)
    r = C.gcn_route(C.graph_case("above_64k")[1])
    assert (r["bwd_bytes"], r["fwd_bytes"], r["fwd_opt_in"], r["per_cu"]) == (89924, 69164, True, 1)
    r = C.gcn_route(C.graph_case("walk_per_cu_1")[1])
    assert r["bwd_bytes"] > 80 * 1024 and (r["cap"], r["cells"]) == (256, 260)
    assert C.gcn_route(C.graph_case("walk_per_cu_4")[1])["cap"] == 1024
    # the shape test_fused_graph_stage_vs_eager used to carry never reached the kernel; the one that replaced it does, above 64 KB
    old = C.gcn_route((2, 41, 2, 64, 10, 1))
    assert old["bwd_bytes"] == 171204 and C.GCN_MAX_LDS == 163584 and not old["supported"]
    new = C.gcn_route((2, 41, 2, 32, 10, 1))
    assert new["supported"] and new["bwd_opt_in"] and new["fwd_opt_in"]
    # D and nd off the unroll-8 stride, N = 1, orders 2 and 3
    assert any(s[3] % 8 and s[4] % 8 and s[5] == 2 for _, s, _ in C.GRAPH_CASES) and any(s[1] == 1 and s[5] == 3 for _, s, _ in C.GRAPH_CASES)


def test_decoder_cases_take_the_routes_they_are_built_for():
    assert [c[1] for c in C.DEC_CASES[:6]] == [(64, 8, 32, 32, 10), (3, 33, 7, 32, 1), (2, 5, 1, 24, 4), (2, 3, 260, 32, 10), (4, 6, 12, 48, 16),
                                               (4, 6, 13, 48, 16)]
    route = {(c[0], pr): C.dec_route(c[1], pr) for c in C.DEC_CASES for pr in c[2]}
    assert all(r["supported"] for r in route.values())
    for (name, pr), r in route.items():
        assert r["kernel"] == ("mfma" if pr == "bf16" else "fp32")
        assert r["walk"] == name.startswith("walk"), (name, pr, r)
        if pr == "fp32":
            assert r["opt_in"] and r["per"] == 1 and r["cap"] == 256         # the two chunk images alone are 73 728 B
    r = route[("partial_chunk_e1", "fp32")]
    assert (r["lpc"], r["nc"], r["partial"]) == (8, 32, True) and C.dec_case("partial_chunk_e1")[1][1] == r["nc"] + 1
    assert route[("one_step", "fp32")]["nc"] == 256 and C.lpc_of(1) == 1
    assert route[("two_chunks_per_variable", "fp32")]["chunks"] == 2 and C.lpc_of(260) == 256
    assert not route[("e16_atomics", "bf16")]["slabs"] and route[("e16_slabs", "bf16")]["slabs"]
    assert C.dec_case("e16_atomics")[1][2] == 12 and C.dec_case("e16_slabs")[1][2] == 13 and C.dec_case("e16_slabs")[1][4] == 16
    assert not route[("two_chunks_per_variable", "bf16")]["slabs"]           # (Lp = 260: the slabs do not fit, LDS atomics)
    for key in (("walk_fp32", "fp32"), ("walk_mfma", "bf16")):
        r = route[key]
        assert r["grid"] == r["cap"] and 0 < r["two"] < 16, (key, r)
    assert route[("walk_fp32", "fp32")]["cap"] == 256 and route[("walk_mfma", "bf16")]["cap"] == 512
    # a W2 that is not 16-byte aligned: bf16 mode runs the fp32 kernels
    assert C.dec_route(C.dec_case("partial_chunk_e1")[1], "bf16", w2_aligned=False)["kernel"] == "fp32"
    for name, shape, _ in C.DEC_CASES:
        assert shape[0] * shape[1] * shape[2] * C.H <= 50000 or name == "benchmark"
    assert C.DISTINCT_WINDOWS * 8 * 32 * C.H <= 50000


def test_restated_lds_arithmetic_is_the_librarys():
    """needs the built library, not a GPU"""
    from immtsf import _lib
    lib = _lib.load()
    for N in (1, 3, 5, 8, 41, 60, 300):
        for D in (8, 13, 32, 64):
            for nd in (2, 3, 10):
                for order in (1, 2, 3):
                    r = C.gcn_route((1, N, 1, D, nd, order))
                    assert lib.immtsf_tpatchgnn_gcn_lds_bytes(N, D, nd, order) == (r["bwd_bytes"] if r["supported"] else 0), (N, D, nd, order)
                    if r["supported"]:
                        assert lib.immtsf_tpatchgnn_gcn_saved_floats(2, N, 3, D, nd, order) == 6 * C.gcn_lds(N, D, nd, order)[2]
    for N in (1, 5, 33, 41, 300):
        for Lp in (1, 7, 12, 13, 260, 600):
            for D in (16, 24, 48, 200):
                for E in (1, 4, 16):
                    assert lib.immtsf_tpatchgnn_decoder_lds_bytes(N, Lp, D, E, C.H) == C.dec_lds_bytes(N, Lp, D, E), (N, Lp, D, E)
    for _, shape, _ in C.GRAPH_CASES:
        assert lib.immtsf_tpatchgnn_gcn_lds_bytes(*shape[1:]) > 0
    for _, shape, _ in C.DEC_CASES:
        assert lib.immtsf_tpatchgnn_decoder_lds_bytes(*shape[1:], C.H) > 0


# ---- (4) the regimes
@pytest.mark.parametrize("name", [c[0] for c in C.GRAPH_CASES])
def test_gates_set_has_dead_and_saturated_gates_and_uniform_rows(name):
    N, order = C.graph_case(name)[1][1], C.graph_case(name)[1][5]
    p = C.graph_params(name, "gates")
    x = C.graph_inputs(name, "gates")[0]
    one, two = C.node_kinds(N)
    for dtype in (torch.float64, torch.float32):
        pre = C.graph_pre({k: v.to(dtype) for k, v in p.items()}, x.to(dtype), order)
        g1, g2 = torch.relu(pre["tanh1"]), torch.relu(pre["tanh2"])
        for n in range(N):
            if one[n].startswith("zero"):          # the whole node, in every cell: gate exactly 0, and far from the kink
                assert not g1[:, :, n].any() and float(pre["tanh1"][:, :, n].max()) < -0.5
                assert float(pre["logits"][:, :, n].max()) <= 0
                assert torch.equal(pre["A"][:, :, n], torch.full_like(pre["A"][:, :, n], 1.0 / N))          # uniform
            if one[n] == "zero_neg":
                assert float(pre["logits"][:, :, n].max()) < -1.0
            if one[n] == "sat":
                assert float(pre["tanh1"][:, :, n].min()) > 1 - 1e-6
            if two[n] == "sat":
                assert float(pre["tanh2"][:, :, n].min()) > 1 - 1e-6
            if two[n] == "zero":
                assert not g2[:, :, n].any() and float(pre["tanh2"][:, :, n].max()) < -0.5
        if dtype == torch.float32 and N > 1:           # saturated in float32: tanh is exactly 1, its derivative exactly 0
            assert (pre["tanh1"][:, :, one.index("sat")] == 1).all()
    assert any(k.startswith("zero") for k in one) and (N == 1 or ("sat" in one and "live" in one and "zero" in two))
    assert float(p["gate1.bias"]) <= -3 and float(p["gate2.bias"]) >= 3


@pytest.mark.parametrize("name", C.DEAD_GATE_CASES)
def test_dead_gate_variant_has_gate_1_at_zero_everywhere(name):
    D, order = C.graph_case(name)[1][3], C.graph_case(name)[1][5]
    p = C.graph_params_dead_gate1(name)
    x = C.graph_inputs(name, "gates")[0]
    assert min(C.graph_kinks(name, "gates", params=p).values()) >= C.KINK
    for dtype in (torch.float64, torch.float32):
        pre = C.graph_pre({k: v.to(dtype) for k, v in p.items()}, x.to(dtype), order)
        assert float(pre["tanh1"].max()) < -0.5 and float(torch.relu(pre["tanh2"]).max()) > 0.5
    r64, r32 = C.graph_reference(name, "gates", params=p), C.graph_reference(name, "gates", torch.float32, params=p)
    for k in ("lin1.weight", "lin1.bias", "gate1.weight", "gate1.bias"):
        assert not r64["g." + k].any()
    assert float(r64["g.nodevec1"].abs().max()) > 0 and float(r64["g.lin2.weight"].abs().max()) > 0
    err = {k: C.part_error(r32[k], w, C.parts_of(k, w.shape, D))[0] for k, w in r64.items()}
    assert 4 * err["out"] <= FP32_BARS[0] and 4 * max(v for k, v in err.items() if k != "out") <= FP32_BARS[1], err


@pytest.mark.parametrize("name", [c[0] for c in C.GRAPH_CASES])
def test_peaky_set_has_one_hot_rows_and_logits_of_30_to_100(name):
    B, N, M, _, _, order = C.graph_case(name)[1]
    p = {k: v.double() for k, v in C.graph_params(name, "peaky").items()}
    pre = C.graph_pre(p, C.graph_inputs(name, "peaky")[0].double(), order)
    top = float(pre["logits"].max())
    print(f"graph {name} peaky: largest logit {top:.1f}, rows with a weight > 0.999: {int((pre['A'].amax(-1) > 0.999).sum())} of {B * M * N}")
    assert 30.0 <= top <= 100.0
    assert (pre["A"].amax(-1) > 0.999).any()


# ---- (5) the float32 yardstick
def _split(err):
    outs = max(v for k, v in err.items() if k == "out")
    grads = max(v for k, v in err.items() if k != "out")
    return outs, grads


@pytest.mark.parametrize("case", GRAPH_IDS, ids=_gid)
def test_float32_oracle_sits_4x_below_the_fp32_bars_graph_stage(case):
    name, pset = case
    _, N, _, D, _, order = C.graph_case(name)[1]
    r64, r32 = C.graph_reference(name, pset), C.graph_reference(name, pset, torch.float32)
    err = {k: C.part_error(r32[k], w, C.parts_of(k, w.shape, D))[0] for k, w in r64.items()}
    out, grad = _split(err)
    print(f"graph {_gid(case)}: float32 oracle against float64, worst part: output {out:.2e}, gradient {grad:.2e} ({max(err, key=err.get)})")
    assert 4 * out <= FP32_BARS[0] and 4 * grad <= FP32_BARS[1], err
    p, x = C.graph_params(name, pset), C.graph_inputs(name, pset)[0]
    p64 = C.graph_pre({k: v.double() for k, v in p.items()}, x.double(), order)
    p32 = C.graph_pre(p, x, order)
    for k in ("tanh1", "tanh2", "logits", "Z"):
        assert torch.equal(p32[k] > 0, p64[k] > 0), k
    if N == 1:         # one node: the adjacency is 1, and everything in front of the softmax has a gradient of exactly 0
        for k in C.GCN_KEYS[:10]:
            assert not r64["g." + k].any() and not r32["g." + k].any(), k


@pytest.mark.parametrize("case", DEC_IDS, ids=_did)
def test_float32_oracle_sits_4x_below_the_fp32_bars_decoder(case):
    name, te_inside = case
    D = C.dec_case(name)[1][3]
    k64, k32 = {}, {}
    r64, r32 = C.dec_reference(name, te_inside, keep=k64), C.dec_reference(name, te_inside, dtype=torch.float32, keep=k32)
    err = {k: C.part_error(r32[k], w, C.parts_of(k, w.shape, D))[0] for k, w in r64.items()}
    out, grad = _split(err)
    print(f"decoder {_did(case)}: float32 oracle against float64, worst part: output {out:.2e}, gradient {grad:.2e} ({max(err, key=err.get)})")
    assert 4 * out <= FP32_BARS[0] and 4 * grad <= FP32_BARS[1], err
    for k in ("z1", "z2"):
        assert torch.equal(k32[k] > 0, k64[k] > 0), k


def test_benchmark_decoder_forward_with_64_distinct_windows_float32_yardstick():
    """the forward is continuous in its pre-activations: no kink condition, every element compared"""
    inp = C.dec_inputs("benchmark", distinct=True)
    assert len({tuple(w.reshape(-1).tolist()) for w in inp["h"]}) == 64 and len({tuple(w.tolist()) for w in inp["t"]}) == 64
    for te_inside in (False, True):
        want = C.dec_forward_reference("benchmark", te_inside)
        err = C.part_error(C.dec_forward_reference("benchmark", te_inside, dtype=torch.float32), want, C.parts_of("out", want.shape))[0]
        assert 4 * err <= FP32_BARS[0], err


# ---- (6) the bf16 floor
@pytest.mark.parametrize("case", [c for c in DEC_IDS if "bf16" in C.dec_case(c[0])[2]], ids=_did)
def test_bf16_floor_of_the_decoder(case):
    """printed, not held to a bar: the GPU test compares bf16 mode with the restatement, whose distance from plain float64 this is"""
    name, te_inside = case
    r64, r16 = C.dec_reference(name, te_inside), C.dec_reference(name, te_inside, bf16=True)
    err = {k: C.l2_error(r16[k], w) for k, w in r64.items() if w.numel()}
    out, grad = _split(err)
    print(f"decoder {_did(case)}: bf16 operands in float64 against float64, relative L2: output {out:.2e}, gradient {grad:.2e} ({max(err, key=err.get)})")
    assert all(torch.isfinite(v).all() for v in r16.values()) and 0 < out < 0.1


@pytest.mark.parametrize("case", [c for c in DEC_IDS if "bf16" in C.dec_case(c[0])[2]], ids=_did)
def test_rounding_g2_alone_stays_at_half_the_bf16_gradient_bar(case):
    """the MFMA backward rounds a third operand, g2, which the reference of the GPU test does not: in float64 that rounding alone has to
    leave half of the gradient bar to the kernel.  A draw that does not is unfit for the bar and is drawn again, like one that fails the
    float32 yardstick."""
    name, te_inside = case
    f = C.dec_bf16_g_floor(name, te_inside)
    print(f"decoder {_did(case)}: g2 rounded to bf16 as well, against the restatement, relative L2: {max(f.values()):.2e} ({max(f, key=f.get)})")
    assert 2 * max(f.values()) <= 1.5e-2, f


def test_g2_rounding_reproduces_what_the_first_draw_measured_on_the_device():
    """e16_atomics, first draw, LearnableTE inside: d te_scale.weight 1.64e-2 on the MI355X in bf16 mode, and the same from g2's rounding on
    the CPU"""
    assert C._DEC_RESEED["e16_atomics"] == 1
    assert abs(C.dec_bf16_g_floor("e16_atomics", True, redraw=0)["g.te_scale.weight"] - 1.64e-2) < 0.02e-2


# ---- the measure
def test_parts_and_the_measure():
    D, order = 5, 2
    assert [p[0] for p in C.parts_of("g.mlp.weight", (D, (order + 1) * D, 1, 1), D)] == ["hop 0", "hop 1", "hop 2"]
    assert [p[0] for p in C.parts_of("g.W1", (C.H, D + 3), D)] == ["h", "te"]
    assert len(C.parts_of("out", (3, 4, 2, D))) == 6 and len(C.parts_of("out", (3, 7, 4))) == 3 and len(C.parts_of("dte", (3, 7, 2))) == 3
    for k in C.GCN_KEYS[:10] + C.TE_KEYS + C.DEC_KEYS[1:]:
        assert C.parts_of("g." + k, (3, 3)) == [("all", ())]
    want = torch.randn(D, (order + 1) * D, 1, 1, generator=torch.Generator().manual_seed(0)).double()
    want[:, 2 * D:] *= 1e-3                                      # the last hop's slab is quiet
    got = want.clone()
    got[0, 2 * D] += 1e-4 * float(want[:, 2 * D:].abs().max())
    err, where = C.part_error(got, want, C.parts_of("g.mlp.weight", want.shape, D))
    assert float((got - want).abs().max() / want.abs().max()) < 1e-6 and 0.9e-4 < err < 1.1e-4 and where == "hop 2"
    zero = torch.zeros(4, 3)
    assert C.part_error(zero, zero, [("all", ())]) == (0.0, "all") and C.part_error(zero + 1e-30, zero, [("all", ())])[0] == float("inf")
    assert C.part_error(want * float("nan"), want, [("all", ())])[0] == float("inf")
    w2 = torch.ones(3, 4, 2).double()
    w2[1] = 0                                                    # an all-zero window in a live tensor: the floor of 1e-6 of the largest element
    g2 = w2.clone()
    g2[1, 0, 0] = 1e-7
    assert abs(C.part_error(g2, w2, C.parts_of("dh", w2.shape))[0] - 0.1) < 1e-9
