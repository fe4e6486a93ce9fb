"""GPU parity of the NeuralFlow backbone with nf_time_net='TimeTanh' on the fused path (the TimeTanh instance of the kernels of
csrc/neural_flow.hip, admitted by config.neuralflow_tanh_fused): outputs and every parameter gradient against the float64 yardstick
(tests/neuralflow_tanh_ref.py, pinned to the module's composed path in tests/test_neuralflow_tanh_ref.py) over the shapes of
tests/neuralflow_tanh_cases.py, whose un-normalised times put 1 - phi^2 anywhere between 0 and 1; which path ran; the composed path
under IMMTSF_NEURALFLOW_FUSED=0 against the same yardstick; TimeLinear models untouched, bit for bit, and never on the TimeTanh
instance; hipGraph capture; the envelope.  Bars (neuralflow_tanh_cases): outputs 1e-4 relative to max, gradients 3e-4 relative to
max(|want|, 1e-2 of the largest gradient)."""
import copy
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neuralflow_tanh_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu
BASE = TC.CASES["a_defaults"]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


class _knobs:
    """config.neuralflow_fused (IMMTSF_NEURALFLOW_FUSED) and config.neuralflow_tanh_fused (IMMTSF_NEURALFLOW_TANH_FUSED) for a block"""

    def __init__(self, fused=True, tanh=True):
        self.want = (fused, tanh)

    def __enter__(self):
        from immtsf import config
        self.was = (config.neuralflow_fused, getattr(config, "neuralflow_tanh_fused", False))
        config.neuralflow_fused, config.neuralflow_tanh_fused = self.want

    def __exit__(self, *a):
        from immtsf import config
        config.neuralflow_fused, config.neuralflow_tanh_fused = self.was


def _run(m, batch):
    tpp, data, tp, mask, up, eps = batch
    m.zero_grad(set_to_none=True)
    m.eps_override = eps
    out = m.forecasting(tpp, data, tp, mask)
    (out * up).sum().backward()
    return out, {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def _check(name, out, grads, want_out, want):
    e = TC.rel(out, want_out)
    diff, errs = TC.grad_errors(grads, want)
    worst = max(errs, key=errs.get)
    scales = {k: errs[k] for k in TC.scale_keys(errs)}
    print(f"{name}: out {e:.2e} (bar {TC.OUT_TOL:.1e})  worst gradient {worst} {errs[worst]:.2e} (bar {TC.GRAD_TOL:.1e})")
    print("   time_net.scale:", {k: f"{v:.2e}" for k, v in scales.items()})
    assert not diff, diff
    assert e < TC.OUT_TOL
    assert scales
    for k, v in scales.items():
        assert v <= TC.GRAD_TOL, f"gradient of {k}: {v:.3e} against float64 (bar {TC.GRAD_TOL:.1e})"
    assert not {k: v for k, v in errs.items() if not v <= TC.GRAD_TOL}


@pytest.fixture(scope="module")
def references():
    cache = {}

    def get(name, time_net="TimeTanh"):
        if (name, time_net) not in cache:
            case = TC.CASES[name]
            m = TC.make_model("cpu", case, time_net)
            cache[name, time_net] = TC.reference(m, TC.make_batch("cpu", case, unit=time_net == "TimeLinear"))[:2]
        return cache[name, time_net]
    return get


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_time_tanh_against_float64(name, fused, references):
    """fused: the TimeTanh kernels ran (fused_calls goes up by one per call, the node carries the kind) and meet the yardstick, and
    every gradient is None exactly where the composed path's is.  composed (IMMTSF_NEURALFLOW_FUSED=0): fused_calls stays, the same
    comparison holds."""
    dev = _dev()
    from immtsf import ops
    case = TC.CASES[name]
    m, batch = TC.make_model(dev, case), TC.make_batch(dev, case)
    n_tanh, n_lin = ops.neural_flow_launches["TimeTanh"], ops.neural_flow_launches["TimeLinear"]
    with _knobs(fused=fused):
        out, grads = _run(m, batch)
        assert m.fused_calls == (1 if fused else 0)
        out2, _ = _run(m, batch)
        assert m.fused_calls == (2 if fused else 0)
    assert ops.neural_flow_launches["TimeTanh"] - n_tanh == (2 if fused else 0) and ops.neural_flow_launches["TimeLinear"] == n_lin
    assert tuple(out.shape) == (case[0], case[2], case[3]) and m.immtsf_graphable
    if fused:
        assert type(out.grad_fn).__name__ == "NeuralFlowFnBackward" and out.grad_fn.time_net == "TimeTanh"
        assert torch.equal(out, out2)
        _, g_composed = TC.composed(copy.deepcopy(m), batch)
        assert {k for k, g in grads.items() if g is None} == {k for k, g in g_composed.items() if g is None}
    _check(name, out.detach(), grads, *references(name))


def test_two_fused_time_tanh_runs_agree_bit_for_bit():
    """no atomics, a fixed summation order: the same bits in two runs over two workgroups, every gradient the kernels' and non-zero"""
    dev = _dev()
    case = TC.CASES["b_tile_edges"]
    m, batch = TC.make_model(dev, case), TC.make_batch(dev, case)
    with _knobs():
        out1, g1 = _run(m, batch)
        out2, g2 = _run(m, batch)
    assert m.fused_calls == 2 and torch.equal(out1, out2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]) and float(g1[k].abs().max()) > 0, k


def test_time_tanh_with_nothing_set_keeps_the_composed_path():
    """config.neuralflow_tanh_fused is off unless asked for: what a TimeTanh model ran before the kernels had a TimeTanh instance"""
    dev = _dev()
    from immtsf import config
    if os.environ.get("IMMTSF_NEURALFLOW_TANH_FUSED", "0") == "1":
        assert config.neuralflow_tanh_fused
        return
    assert not config.neuralflow_tanh_fused
    m, batch = TC.make_model(dev, BASE), TC.make_batch(dev, BASE)
    _run(m, batch)
    assert m.fused_calls == 0


def test_time_linear_is_untouched(references):
    """a TimeLinear model with the TimeTanh knob on: the TimeLinear instance alone runs, two calls give the same bits, and the numbers
    are those the float64 yardstick (with the TimeLinear time net) accepts, as the composed path's are"""
    dev = _dev()
    from immtsf import ops
    m = TC.make_model(dev, BASE, "TimeLinear")
    batch = TC.make_batch(dev, BASE, unit=True)
    n_tanh, n_lin = ops.neural_flow_launches["TimeTanh"], ops.neural_flow_launches["TimeLinear"]
    with _knobs():
        out1, g1 = _run(m, batch)
        kind = out1.grad_fn.time_net
        out2, g2 = _run(m, batch)
    with _knobs(tanh=False):
        out3, g3 = _run(m, batch)
    assert m.fused_calls == 3 and kind == out2.grad_fn.time_net == out3.grad_fn.time_net == "TimeLinear"
    assert ops.neural_flow_launches["TimeTanh"] == n_tanh and ops.neural_flow_launches["TimeLinear"] == n_lin + 3
    assert torch.equal(out1, out2) and torch.equal(out1, out3)
    for k in g1:
        assert torch.equal(g1[k], g2[k]) and torch.equal(g1[k], g3[k]), k
    want_out, want = references("a_defaults", "TimeLinear")
    _check("a_defaults TimeLinear fused", out1.detach(), g1, want_out, want)
    with _knobs(fused=False):
        out_c, g_c = _run(m, batch)
    assert m.fused_calls == 3
    _check("a_defaults TimeLinear composed", out_c.detach(), g_c, want_out, want)


def test_forward_backward_under_graph_capture():
    """one forward + backward of case A captured and replayed twice: the eager call's outputs and gradients, bit for bit"""
    dev = _dev()
    m, batch = TC.make_model(dev, BASE), TC.make_batch(dev, BASE)
    with _knobs():
        assert m.immtsf_graphable
        want_out, want_g = _run(copy.deepcopy(m), batch)
        static = tuple(t.clone() for t in batch)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _run(m, static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        m.zero_grad(set_to_none=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m.forecasting(static[0], static[1], static[2], static[3])
            (out * static[4]).sum().backward()
    assert m.fused_calls == 2      # the warm-up and the capture
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.detach(), want_out.detach())
        for k, p in m.named_parameters():
            assert torch.equal(p.grad, want_g[k]), k


def test_unknown_time_net_returns_an_error_code_and_launches_nothing():
    dev = _dev()
    from immtsf import _lib
    lib = _lib.load()
    B, L, Lp, C, o = BASE
    d = _lib.NeuralFlowDims(B, L, Lp, C, o["nf_rec_dims"], o["nf_latents"], o["nf_hidden_dim"], o["nf_hidden_layers"], o["nf_flow_layers"])
    assert lib.immtsf_neural_flow_tn_supported(ctypes.byref(d), 1) == 1
    buf = torch.zeros(1 << 16, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    for kind in (2, -1):
        assert lib.immtsf_neural_flow_tn_supported(ctypes.byref(d), kind) == 0
        assert lib.immtsf_neural_flow_tn_forward(ctypes.byref(d), kind, p, p, p, p, p, p, p, p, p, p, None) == -3      # IMMTSF_EUNSUPPORTED
        assert lib.immtsf_neural_flow_tn_backward(ctypes.byref(d), kind, p, p, p, p, p, p, p, p, p, p, p, p, 1 << 18, None) == -3
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0


def test_width_outside_the_envelope_takes_the_composed_path():
    """hidden_dim 129 is past the kernels' limit: a TimeTanh model of that width runs composed with every knob on, fused_calls stays"""
    dev = _dev()
    from immtsf import ops
    m = TC.make_model(dev, BASE, nf_hidden_dim=129)
    batch = TC.make_batch(dev, BASE)
    n = dict(ops.neural_flow_launches)
    with _knobs():
        out, grads = _run(m, batch)
    assert m.fused_calls == 0 and ops.neural_flow_launches == n
    assert out.grad_fn is not None and type(out.grad_fn).__name__ != "NeuralFlowFnBackward"
    assert torch.isfinite(out).all() and all(g is not None and torch.isfinite(g).all() for g in grads.values())
