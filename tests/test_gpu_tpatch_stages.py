"""GPU checks of tPatchGNN's adaptive-graph stage (csrc/gcn.hip) and forecast decoder (csrc/decoder.hip) through immtsf.ops -- that is,
through the C ABI -- against oracle.tpatchgnn_ref's graph_stage / decode in float64 (pinned on the CPU by tests/test_tpatch_stages_ref.py,
which also holds the inputs of tests/tpatch_stage_cases.py to the conditions they are built for and every case to its route).

Graph stage, (B, N, M, D, nd, order), each under three parameter sets (default; gates: whole nodes with a gate of exactly 0 or a saturated
tanh, adjacency rows whose logits are all < 0 or all exactly 0; peaky: one-hot rows, logits up to 36):
  benchmark            (64, 8, 2, 32, 10, 1)    32 504 B of LDS, 128 cells on 128 workgroups
  odd_two_hops         (3, 5, 3, 13, 3, 2)      D and nd off the unroll-8 stride
  one_node_three_hops  (2, 1, 1, 8, 2, 3)       N = 1: the adjacency is 1
  above_64k            (3, 41, 2, 32, 10, 1)    89 924 B (forward 69 164 B): both launchers take the hipFuncSetAttribute route
  walk_per_cu_1        (130, 3, 2, 64, 10, 1)   83 044 B: one workgroup per CU, 260 cells on 256 workgroups (4 do two cells)
  walk_per_cu_4        (345, 3, 3, 8, 2, 1)     2 500 B: four per CU, 1035 cells on 1024 workgroups (11 do two)
ops.gcn_adaptive under autograd (forward_saved + backward_saved): out, dx, twelve parameter gradients; on benchmark, above_64k and
walk_per_cu_1 also the recomputing pair immtsf_tpatchgnn_gcn_forward / _backward.
Decoder, (B, N, Lp, D, E), H = 32, each as tpatch_decoder (te a tensor: out, dh, dte, six gradients) and tpatch_decoder_te (LearnableTE
inside: out, dh, six + four gradients), fp32 and bf16 (route fp32 | bf16):
  benchmark                (64, 8, 32, 32, 10)   8 variables per 256-row chunk | slabs
  partial_chunk_e1         (3, 33, 7, 32, 1)     32 variables per chunk + 1, no periodic part (its pointers are null) | LDS atomics
  one_step                 (2, 5, 1, 24, 4)      Lp = 1 | LDS atomics
  two_chunks_per_variable  (2, 3, 260, 32, 10)   two 256-step chunks per variable | LDS atomics (the slabs do not fit)
  e16_atomics              (4, 6, 12, 48, 16)    E = 16 | Lp = 12: LDS atomics
  e16_slabs                (4, 6, 13, 48, 16)    E = 16 | Lp = 13: slabs
  walk_fp32                (260, 2, 3, 16, 4)    fp32 only: 260 windows on 256 workgroups
  walk_mfma                (516, 1, 3, 16, 4)    bf16 only: 516 windows on 512 workgroups
and bf16 mode with a W2 at a 4-byte storage offset (ops passes the pointer through unchanged: dec_mfma_ok is false and the fp32 kernels run,
which the fp32 bars against plain float64 show), and gradient buffers that start from a non-zero fill.  The benchmark case repeats
four (h, t) under 64 upstream gradients (tpatch_stage_cases.dec_inputs: the kink condition); its forward, which needs no such condition, is
also run with 64 different windows.

Error measure: fp32 per part (tpatch_stage_cases.parts_of: per cell / window for outputs and data gradients; every parameter gradient on its
own, mlp.weight per hop slab, W1 split into its h and te columns), max |got - want| / max |want| of the part, floor 1e-6 of the tensor's
largest element, the worst part reported; bars 1e-4 outputs / 2e-4 gradients.  bf16 decoder: relative L2 per tensor against
the float64 restatement with the second layer's two operands rounded to bf16, bars 2e-3 / 1.5e-2 (those of
test_fused_decoder_bf16_mfma_vs_eager for the same arithmetic).  No element is left out of any comparison: the cases hold the ReLU-kink
condition (no float64 pre-activation within 1e-5 max |.| of zero).
The float32 yardstick (the same oracle in float32 on the CPU against float64, per part, on these inputs; test_tpatch_stages_ref.py asserts
it >= 4x below the fp32 bars with identical ReLU masks): graph stage outputs <= 9.3e-7, gradients <= 2.3e-5 (d gate1.bias, above_64k
gates: a scalar, the sum over every cell and node); decoder outputs <= 1.3e-5 (walk_mfma: windows of three numbers), gradients <= 2.7e-6.
(The peaky set scales ONE node vector: with all of them scaled the float32 oracle itself misses the bars, see tpatch_stage_cases.graph_params.)
The bf16 floor (the restatement against plain float64, relative L2): outputs <= 3.6e-3, gradients <= 5.7e-2 with te a tensor and up to
2.7e-1 on the scalar d te_scale.bias.  The MFMA backward rounds a third operand, g2, which the restatement does not.  The restatement is
kept at the two operands all the same: they are the reference the bars of test_fused_decoder_bf16_mfma_vs_eager were set against, and a
reference that followed every rounding of the kernel would stop seeing a rounding that should not be there.  What g2's rounding costs is
instead bounded on the CPU, in float64, on every case's inputs: <= 6.2e-3, held to half the gradient bar (tpatch_stage_cases.dec_bf16_g_floor).
Measured on the MI355X, the worst case of each bar class: see MEASURED below.

Exact requirements, each checked against what float64 gives first: with N = 1 the gradients of the node vectors, gates and lin* are
exactly 0; with every node's gate 1 exactly 0 the gradients of lin1 and gate1 are exactly 0.

The seven mutations of the issue, each run once against this file: see MUTATIONS below."""
import functools
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tpatch_stage_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
FP32_BARS = (1e-4, 2e-4)         # outputs, gradients: per part
BF16_L2_BARS = (2e-3, 1.5e-2)    # the decoder's bf16 mode against its restatement: relative L2 per tensor
MEASURED = """worst figure of one MI355X run per bar class (fp32: per part; bf16: relative L2 per tensor against the restatement); 65 cases, none failed
                              fp32 outputs                  fp32 gradients                                 bf16 outputs   bf16 gradients
graph stage (autograd)        1.7e-6 (walk_per_cu_1 gates)  3.8e-5 (d gate2.bias, odd_two_hops default)    -              -
graph stage (recomputing)     1.7e-6 (walk_per_cu_1 gates)  3.0e-5 (d gate1.bias, above_64k gates)         -              -
decoder, te a tensor          8.6e-7 (walk_fp32)            1.0e-6 (dW1, two_chunks_per_variable)          8.8e-6         2.6e-3 (db1, e16_slabs)
decoder, LearnableTE inside   8.6e-7                        2.4e-6 (d te_scale.bias, two_chunks_...)       8.8e-6         6.1e-3 (d te_scale.bias, two_chunks_...)
forward, 64 distinct windows  3.6e-7                        -                                              6.8e-6         -
decoder, buffers at 0.125     -                             below the rows above                           -              2.9e-3
bf16 mode, W2 4 bytes off     below 1e-6 (fp32 bars, against plain float64: the fp32 kernels ran)
bars                          1e-4                          2e-4                                           2e-3           1.5e-2
CPU float32 yardstick         9.3e-7 / 1.3e-5 (decoder)     2.3e-5 / 2.7e-6 (decoder)"""
MUTATIONS = """each applied to a scratch copy of the kernel (arithmetic only), the library rebuilt, this file run once on an MI355X; the tests that fail
1 gcn_bwd_kernel: g_mw assigned per cell, not added     9: the six walk_per_cu_1 / walk_per_cu_4 cases and walk_per_cu_1's three recomputing
                                                           ones -- the walk cases and no other
2 softmax backward without the row term sum A dA        28: every graph case but one_node_three_hops gates (gate 0: nothing reaches the softmax);
                                                           the one-node cases fail their exact zeros
3 relu' of the logits as >= 0                           26: every graph case with N > 1 (S = relu(.) >= 0 always: the mask is gone)
4 gate derivative without the relu mask on tanh         26: every graph case with N > 1, the dead-gate test on d gate1 == 0
5 second hop's backward with A for A^T                  4: odd_two_hops under its three sets and in the dead-gate test -- the only order >= 2
                                                           case with N > 1
6 dec_bwd_kernel: dv without the last variable of a     13: every fp32 case whose last chunk is partial (partial_chunk_e1, one_step, e16_atomics,
  partial chunk                                            e16_slabs, walk_fp32, both forms), the misaligned-W2 pair, the fp32 buffers test
7 dec_te_grad: sin for cos                              7: every fp32 LearnableTE-inside case with E > 1, the fp32 buffers test (the MFMA backward
                                                           has its own cos and does not call dec_te_grad)
All seven are caught."""


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


def _assert_close(label, got, want, precision, D=None):
    """every tensor of `want` against `got`: fp32 per part, bf16 relative L2 per tensor; every figure printed before anything is asserted"""
    assert set(got) == set(want), (sorted(got), sorted(want))
    bad = []
    for k, w in want.items():
        g = got[k]
        out = k == "out"
        if not w.numel():
            assert g.shape == w.shape
            continue
        if precision == "fp32":
            bar = FP32_BARS[0 if out else 1]
            err, where = C.part_error(g, w, C.parts_of(k, w.shape, D))
            print(f"{label} {k}: worst part error {err:.2e} ({where}, bar {bar:.0e})")
        else:
            bar = BF16_L2_BARS[0 if out else 1]
            err, where = C.l2_error(g, w), "L2"
            print(f"{label} {k}: relative L2 {err:.2e} (bar {bar:.1e})")
        if not (torch.isfinite(g).all() and err < bar):
            bad.append(f"{k} {err:.2e} at {where} (bar {bar:.1e})")
    assert not bad, f"{label}: " + "; ".join(bad)


# ================================================================================================ the adaptive-graph stage
def _graph_through_ops(name, pset, params=None):
    """ops.gcn_adaptive under autograd: immtsf_tpatchgnn_gcn_forward_saved + _backward_saved"""
    from immtsf import ops
    dev = _dev()
    _, N, _, D, nd, order = C.graph_case(name)[1]
    assert ops.gcn_adaptive_supported(N, D, nd, order), "the case would take the stock-torch branch of tPatchGNN._graph_stage"
    p = C.graph_params(name, pset) if params is None else params
    q = {k: v.to(dev).requires_grad_(True) for k, v in p.items()}
    mod = lambda s: types.SimpleNamespace(weight=q[s + ".weight"], bias=q[s + ".bias"])      # noqa: E731
    x, up = C.graph_inputs(name, pset)
    xi = x.to(dev).requires_grad_(True)
    out = ops.gcn_adaptive(xi, order, q["nodevec1"], q["nodevec2"], mod("gate1"), mod("gate2"), mod("lin1"), mod("lin2"), mod("mlp"))
    assert type(out.grad_fn).__name__ == "GCNAdaptiveFnBackward"
    out.backward(up.to(dev))
    torch.cuda.synchronize()
    got = {"out": out.detach().cpu(), "dx": xi.grad.cpu()}
    got.update({"g." + k: q[k].grad.cpu() for k in C.GCN_KEYS})
    return got


def _graph_recomputing(name, pset):
    """immtsf_tpatchgnn_gcn_forward / _backward through ctypes: the backward recomputes every cell from x"""
    import ctypes
    from immtsf import _lib
    from immtsf.ops import _struct, ptr, stream_ptr
    dev = _dev()
    lib = _lib.load()
    shape = C.graph_case(name)[1]
    assert lib.immtsf_tpatchgnn_gcn_lds_bytes(*shape[1:]) > 0
    p = C.graph_params(name, pset)
    params = [p[k].to(dev).contiguous() for k in C.GCN_KEYS]
    grads = [torch.zeros_like(t) for t in params]
    x, up = (t.to(dev).contiguous() for t in C.graph_inputs(name, pset))
    out, dx = torch.empty_like(x), torch.empty_like(x)
    ps, gs = _struct(_lib.GCNParams, params), _struct(_lib.GCNParams, grads)
    _lib.check(lib.immtsf_tpatchgnn_gcn_forward(*shape, ptr(x), ctypes.byref(ps), ptr(out), stream_ptr()), "gcn_forward")
    _lib.check(lib.immtsf_tpatchgnn_gcn_backward(*shape, ptr(x), ctypes.byref(ps), ptr(up), ptr(dx), ctypes.byref(gs), stream_ptr()), "gcn_backward")
    torch.cuda.synchronize()
    got = {"out": out.cpu(), "dx": dx.cpu()}
    got.update({"g." + k: g.cpu() for k, g in zip(C.GCN_KEYS, grads)})
    return got


@functools.lru_cache(maxsize=None)
def _graph_reference(name, pset):
    return C.graph_reference(name, pset)


GRAPH_IDS = [(c[0], s) for c in C.GRAPH_CASES for s in C.GRAPH_SETS]


@pytest.mark.parametrize("case", GRAPH_IDS, ids=lambda x: f"{x[0]}_{x[1]}")
def test_graph_stage_against_float64(case):
    name, pset = case
    N, D = C.graph_case(name)[1][1], C.graph_case(name)[1][3]
    got, want = _graph_through_ops(name, pset), _graph_reference(name, pset)
    if N == 1:
        for k in C.GCN_KEYS[:10]:
            assert not want["g." + k].any()          # float64: the softmax of one logit is 1 whatever the logit
            assert not got["g." + k].any(), f"{k}: gradient of a one-node graph is not exactly 0: {float(got['g.' + k].abs().max()):.3e}"
    _assert_close(f"graph {name} {pset}", got, want, "fp32", D)


@pytest.mark.parametrize("pset", C.GRAPH_SETS)
@pytest.mark.parametrize("name", ["benchmark", "above_64k", "walk_per_cu_1"])
def test_graph_stage_recomputing_pair_against_float64(name, pset):
    """gcn_fwd_kernel<false> and gcn_bwd_kernel<false> (cell_forward inside the backward's walk over cells)"""
    D = C.graph_case(name)[1][3]
    _assert_close(f"graph recomputing {name} {pset}", _graph_recomputing(name, pset), _graph_reference(name, pset), "fp32", D)


@pytest.mark.parametrize("name", C.DEAD_GATE_CASES)
def test_nodes_with_a_dead_gate_contribute_exactly_nothing_to_their_linear(name):
    """the gates set with every node vector 1 taken off the gate's direction: gate 1 is exactly 0 on every node of every cell, so lin1 and
    gate 1 have gradients of exactly 0 -- in float64, and in the kernel (dL1 = 0 * dNV1, relu'(tanh) = 0), not the residue of a product"""
    D = C.graph_case(name)[1][3]
    p = C.graph_params_dead_gate1(name)
    got, want = _graph_through_ops(name, "gates", p), C.graph_reference(name, "gates", params=p)
    for k in ("lin1.weight", "lin1.bias", "gate1.weight", "gate1.bias"):
        assert not want["g." + k].any()
        assert not got["g." + k].any(), f"{k}: {float(got['g.' + k].abs().max()):.3e}"
    _assert_close(f"graph {name} dead gate 1", got, want, "fp32", D)


# ================================================================================================ the decoder
def _dec_tensors(name, dev, w2_offset=False):
    p, inp = C.dec_params(name), C.dec_inputs(name)
    q = {k: v.to(dev) for k, v in p.items()}
    if w2_offset:            # a contiguous view one float into its storage: 4 bytes off the allocation's alignment
        base = torch.zeros(C.H * C.H + 1, device=dev)
        base[1:] = q["W2"].reshape(-1)
        q["W2"] = base[1:].view(C.H, C.H).detach()
        assert q["W2"].is_contiguous() and q["W2"].data_ptr() % 16 == 4
    else:
        assert q["W2"].data_ptr() % 16 == 0
    return {k: v.requires_grad_(True) for k, v in q.items()}, {k: v.to(dev) for k, v in inp.items()}


def _decoder_through_ops(name, precision, te_inside, w2_offset=False):
    from immtsf import _lib, ops
    dev = _dev()
    assert _lib.load().immtsf_tpatchgnn_decoder_lds_bytes(*C.dec_case(name)[1][1:], C.H) > 0
    q, inp = _dec_tensors(name, dev, w2_offset)
    lin = lambda i: types.SimpleNamespace(weight=q[C.DEC_KEYS[2 * i]], bias=q[C.DEC_KEYS[2 * i + 1]])      # noqa: E731
    seq = [lin(0), None, lin(1), None, lin(2)]
    h = inp["h"].clone().requires_grad_(True)
    if te_inside:
        out = ops.tpatch_decoder_te(seq, h, inp["t"], *[q[k] for k in C.TE_KEYS], precision=precision)
        assert type(out.grad_fn).__name__ == "TPatchDecoderTEFnBackward"
    else:
        te = inp["te"].clone().requires_grad_(True)
        out = ops.tpatch_decoder(seq, h, te, precision=precision)
        assert type(out.grad_fn).__name__ == "TPatchDecoderFnBackward"
    if w2_offset:
        assert q["W2"].contiguous().data_ptr() == q["W2"].data_ptr()           # what ops hands to the library
    out.backward(inp["up"])
    torch.cuda.synchronize()
    got = {"out": out.detach().cpu(), "dh": h.grad.cpu()}
    got.update({"g." + k: q[k].grad.cpu() for k in C.DEC_KEYS})
    if te_inside:
        got.update({"g." + k: q[k].grad.cpu() for k in C.TE_KEYS})
    else:
        got["dte"] = te.grad.cpu()
    return got


@functools.lru_cache(maxsize=None)
def _dec_reference(name, te_inside, bf16):
    return C.dec_reference(name, te_inside, bf16=bf16)


DEC_IDS = [(c[0], pr, ti) for c in C.DEC_CASES for pr in c[2] for ti in (False, True)]


@pytest.mark.parametrize("case", DEC_IDS, ids=lambda x: f"{x[0]}_{x[1]}_{'te_inside' if x[2] else 'te_tensor'}")
def test_decoder_against_float64(case):
    """fp32: against oracle decode (and LearnableTE as [w0 t + b0 ; sin(w t + b)]) in float64; bf16: against the same with the second
    layer's two operands rounded to bf16"""
    name, precision, te_inside = case
    D = C.dec_case(name)[1][3]
    got, want = _decoder_through_ops(name, precision, te_inside), _dec_reference(name, te_inside, precision == "bf16")
    _assert_close(f"decoder {name} {precision} {'te inside' if te_inside else 'te tensor'}", got, want, precision, D)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("te_inside", [False, True], ids=["te_tensor", "te_inside"])
def test_decoder_forward_at_the_benchmark_shape_with_64_distinct_windows(te_inside, precision):
    """the benchmark case above repeats four (h, t) for the kink condition's sake; the forward is continuous in its pre-activations and
    needs none, so here every window is different and every output is compared.  (Backward over distinct windows: walk_fp32's 260 and
    walk_mfma's 516, per window.)"""
    from immtsf import ops
    dev = _dev()
    name = "benchmark"
    q, _ = _dec_tensors(name, dev)
    inp = {k: v.to(dev) for k, v in C.dec_inputs(name, distinct=True).items()}
    lin = lambda i: types.SimpleNamespace(weight=q[C.DEC_KEYS[2 * i]], bias=q[C.DEC_KEYS[2 * i + 1]])      # noqa: E731
    seq = [lin(0), None, lin(1), None, lin(2)]
    with torch.no_grad():
        if te_inside:
            out = ops.tpatch_decoder_te(seq, inp["h"], inp["t"], *[q[k] for k in C.TE_KEYS], precision=precision)
        else:
            out = ops.tpatch_decoder(seq, inp["h"], inp["te"], precision=precision)
    torch.cuda.synchronize()
    want = C.dec_forward_reference(name, te_inside, precision == "bf16")
    _assert_close(f"decoder {name} 64 distinct windows {precision} {'te inside' if te_inside else 'te tensor'}", {"out": out.cpu()}, {"out": want}, precision)


@pytest.mark.parametrize("te_inside", [False, True], ids=["te_tensor", "te_inside"])
def test_bf16_mode_with_a_misaligned_W2_runs_the_fp32_kernels(te_inside):
    """dec_mfma_ok: W2 is not 16-byte aligned (ops hands the view's pointer on as it is), so bf16 mode takes dec_fwd_kernel / dec_bwd_kernel:
    the result meets the fp32 bars against PLAIN float64, which the MFMA route (2e-3 away by design) cannot"""
    name = "partial_chunk_e1"
    D = C.dec_case(name)[1][3]
    got = _decoder_through_ops(name, "bf16", te_inside, w2_offset=True)
    _assert_close(f"decoder {name} bf16 mode, W2 4 bytes off", got, _dec_reference(name, te_inside, False), "fp32", D)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_decoder_gradient_buffers_accumulate(precision):
    """immtsf_tpatchgnn_decoder_backward_te ADDS the six + four parameter gradients to what the buffers hold (FlatTrainer's shared sinks
    rely on it): buffers that start at 0.125 end at 0.125 + the gradient"""
    import ctypes
    from immtsf import _lib
    from immtsf.ops import _struct, ptr, stream_ptr
    dev = _dev()
    lib = _lib.load()
    name, fill = "e16_slabs", 0.125
    B, N, Lp, D, E = C.dec_case(name)[1]
    q, inp = _dec_tensors(name, dev)
    params, tparams = [q[k].detach().contiguous() for k in C.DEC_KEYS], [q[k].detach().contiguous() for k in C.TE_KEYS]
    grads, tgrads = [torch.full_like(t, fill) for t in params], [torch.full_like(t, fill) for t in tparams]
    ps, gs = _struct(_lib.DecoderParams, params), _struct(_lib.DecoderParams, grads)
    ts, tg = _struct(_lib.Time2VecParams, tparams), _struct(_lib.Time2VecParams, tgrads)
    code = 1 if precision == "bf16" else 0
    dh = torch.empty_like(inp["h"])
    _lib.check(lib.immtsf_tpatchgnn_decoder_backward_te(B, N, Lp, D, E, C.H, code, ptr(inp["h"]), ptr(inp["t"]), ctypes.byref(ts), ctypes.byref(ps),
                                                        ptr(inp["up"].contiguous()), ptr(dh), ctypes.byref(gs), ctypes.byref(tg), stream_ptr()),
               "decoder_backward_te")
    torch.cuda.synchronize()
    want = dict(_dec_reference(name, True, precision == "bf16"))
    del want["out"]
    got = {"dh": dh.cpu()}
    got.update({"g." + k: (g.cpu().double() - fill) for k, g in zip(C.DEC_KEYS + C.TE_KEYS, grads + tgrads)})
    _assert_close(f"decoder {name} {precision} from buffers at {fill}", got, want, precision, D)
