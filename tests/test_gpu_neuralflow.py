"""GPU parity of the NeuralFlow backbone (models/NeuralFlow.py::forecasting): the fused kernels (csrc/neural_flow.hip) and the composed
path against the goldens of the reference's own code (with the recorded noise) and against the float64 restatement
(tests/neuralflow_ref.py, pinned to those goldens in tests/test_neuralflow_ref.py) over the shapes of tests/neuralflow_cases.py;
determinism, the fall-backs to the composed path, the knob, the constructor's errors, hipGraph capture and the evaluation engine.
Tolerances (neuralflow_cases.bars): the project's fp32 bars -- 1e-4 outputs / 3e-4 gradients relative to max, the gradient floor at 1e-2
of the largest gradient -- on every shape: tests/test_neuralflow_ref.py holds torch's own fp32 CPU run of the restatement 4x inside
them everywhere."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neuralflow_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BASE = TC.CASES["a_small"]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


class _knob:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from immtsf import config
        self.was = config.neuralflow_fused
        config.neuralflow_fused = self.on

    def __exit__(self, *a):
        from immtsf import config
        config.neuralflow_fused = self.was


def _run(m, batch):
    tpp, data, tp, mask, up, eps = batch
    m.zero_grad(set_to_none=True)
    m.eps_override = eps
    out = m.forecasting(tpp, data, tp, mask)
    (out * up).sum().backward()
    return out.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def _check(name, out, grads, want_out, want):
    o_bar, g_bar = TC.bars(name)
    e = TC.rel(out, want_out)
    diff, errs = TC.grad_errors(grads, want)
    worst = max(errs, key=errs.get)
    print(f"{name}: out {e:.2e} (bar {o_bar:.1e})  worst gradient {worst} {errs[worst]:.2e} (bar {g_bar:.1e})")
    assert not diff, diff
    assert e < o_bar
    assert not {k: v for k, v in errs.items() if not v <= g_bar}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("name", sorted(TC.GOLDENS))
def test_reference_golden(name, fused):
    """every golden through NeuralFlow(configs).forecasting: output, every gradient, and the set without one"""
    dev = _dev()
    from models.NeuralFlow import NeuralFlow
    C, L, Lp, options, _ = TC.GOLDENS[name]
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    m = NeuralFlow(TC.config(C, L, Lp, device=str(dev), **options)).train()
    m.load_state_dict({key[2:]: torch.from_numpy(z[key]) for key in z.files if key.startswith("p.")}, strict=True)
    m = m.to(dev)
    batch = tuple(torch.from_numpy(z[key]).to(dev) for key in ("tpp", "data", "tp", "mask", "upstream")) + (torch.from_numpy(z["eps"])[None].to(dev),)
    with _knob(fused):
        out, grads = _run(m, batch)
    assert m.fused_calls == (1 if fused and name != "model_neuralflow_tanh" else 0)      # TimeTanh: composed whatever the knob says
    none = set(str(z["none"]).split("\n")) - {""}
    want = {key: (None if key in none else torch.from_numpy(z["g." + key])) for key in grads}
    _check(name, out, grads, torch.from_numpy(z["out"]), want)


@pytest.fixture(scope="module")
def references():
    cache = {}

    def get(name):
        if name not in cache:
            case = TC.case_of(name)
            cache[name] = TC.reference(TC.make_model("cpu", case), TC.make_batch("cpu", case))
        return cache[name]
    return get


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_float64_restatement(name, fused, references):
    dev = _dev()
    case = TC.CASES[name]
    m, batch = TC.make_model(dev, case), TC.make_batch(dev, case)
    with _knob(fused):
        out, grads = _run(m, batch)
    assert m.fused_calls == (1 if fused else 0)
    assert tuple(out.shape) == (case[0], case[3], case[1])
    _check(name, out, grads, *references(name))


def test_two_fused_runs_agree_bit_for_bit():
    """the kernels use no atomics: the forecast and every gradient (all of them are the kernels') are the same bits in two runs, over
    two workgroups"""
    dev = _dev()
    case = TC.CASES["b_nine_windows"]
    m, batch = TC.make_model(dev, case), TC.make_batch(dev, case)
    out1, g1 = _run(m, batch)
    out2, g2 = _run(m, batch)
    assert m.fused_calls == 2 and torch.equal(out1, out2)
    assert len(g1) == 4 + 2 * 2 * 7 + 4 + 2
    for k in g1:
        assert torch.equal(g1[k], g2[k]) and float(g1[k].abs().max()) > 0, k


def test_time_tanh_runs_the_composed_path_and_meets_the_restatement(references):
    dev = _dev()
    case = TC.case_of("time_tanh")
    m, batch = TC.make_model(dev, case), TC.make_batch(dev, case)
    out, grads = _run(m, batch)
    assert m.fused_calls == 0
    _check("time_tanh", out, grads, *references("time_tanh"))


def test_data_gradient_runs_the_composed_path(references):
    dev = _dev()
    m = TC.make_model(dev, BASE)
    tpp, data, tp, mask, up, eps = TC.make_batch(dev, BASE)
    data = data.clone().requires_grad_(True)
    out, grads = _run(m, (tpp, data, tp, mask, up, eps))
    assert m.fused_calls == 0
    assert data.grad is not None and float(data.grad.abs().max()) > 0
    _check("a_small", out, grads, *references("a_small"))


def test_knob_off_runs_the_composed_path_and_the_noise_is_drawn_by_default():
    dev = _dev()
    m, batch = TC.make_model(dev, BASE), TC.make_batch(dev, BASE)
    with _knob(True):
        out_f, g_f = _run(m, batch)
    with _knob(False):
        out_c, g_c = _run(m, batch)
    assert m.fused_calls == 1
    assert TC.rel(out_f, out_c) < TC.OUT_TOL
    diff, errs = TC.grad_errors(g_f, g_c)
    assert not diff and max(errs.values()) <= TC.GRAD_TOL
    m.eps_override = None      # two draws differ, in eval as in train
    m.eval()
    with torch.no_grad():
        a, b = m.forecasting(*batch[:4]), m.forecasting(*batch[:4])
    assert m.fused_calls == 3 and not torch.equal(a, b) and torch.isfinite(a).all()


def test_the_constructors_errors():
    dev = _dev()
    from models.NeuralFlow import NeuralFlow
    with pytest.raises(NotImplementedError, match="nf_flow_model='resnet'"):
        NeuralFlow(TC.config(3, 7, 4, device=str(dev), nf_flow_model="resnet"))
    with pytest.raises(ValueError, match="Unknown flow transformation"):
        NeuralFlow(TC.config(3, 7, 4, device=str(dev), nf_flow_model="attention"))


def test_dims_outside_supported_return_an_error_code_and_launch_nothing():
    dev = _dev()
    import ctypes
    from immtsf import _lib
    lib = _lib.load()
    d = _lib.NeuralFlowDims(2, 3, 2, 3, 65, 6, 12, 2, 2)      # rec_dims above the limit
    buf = torch.zeros(1 << 16, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    assert lib.immtsf_neural_flow_forward(ctypes.byref(d), p, p, p, p, p, p, p, p, p, p, None) == -3
    assert lib.immtsf_neural_flow_backward(ctypes.byref(d), p, p, p, p, p, p, p, p, p, p, p, p, 1 << 18, None) == -3
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0


def _capture(m, static):
    dev = static[0].device
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
    return graph, out


def test_forward_backward_under_graph_capture():
    """forward + backward captured once, replayed three times on a second batch with other observed and forecast times, read from
    device memory: the numbers of an eager run on that batch, bit for bit"""
    dev = _dev()
    m = TC.make_model(dev, BASE)
    first = TC.make_batch(dev, BASE, seed=7)
    second = TC.make_batch(dev, BASE, seed=8)
    assert not torch.equal(first[2], second[2]) and not torch.equal(first[0], second[0])
    want_out, want_g = _run(copy.deepcopy(m), second)
    static = tuple(t.clone() for t in first)
    graph, out = _capture(m, static)
    for s, t in zip(static, second):
        s.copy_(t)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.detach(), want_out)
        for k, p in m.named_parameters():
            assert torch.equal(p.grad, want_g[k]), k
    assert m.fused_calls == 2      # the warm-up and the capture


def test_captured_graph_holds_two_forward_and_three_backward_kernels():
    """the backbone's share of ONE replay of the captured forward + backward, by kernel name; the draw of eps (here: the override) and
    the flattening of the parameters run beside them"""
    dev = _dev()
    m = TC.make_model(dev, BASE)
    static = tuple(t.clone() for t in TC.make_batch(dev, BASE))
    graph, _ = _capture(m, static)
    graph.replay()
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        graph.replay()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if "nf_" in e.name and "kernel" in e.name]
    print(names)
    assert sum("nf_enc_fwd_kernel" in n for n in names) == 1 and sum("nf_dec_fwd_kernel" in n for n in names) == 1
    assert sum("nf_dec_bwd_kernel" in n for n in names) == 1 and sum("nf_enc_bwd_kernel" in n for n in names) == 1
    assert sum("nf_fold_kernel" in n for n in names) == 1
    assert len(names) == 5


def test_evalstep_serves_a_neuralflow_and_keys_the_knob():
    dev = _dev()
    import immtsf
    m = TC.make_model(dev, BASE).eval()
    batches = []
    for seed in (11, 12):
        tpp, data, tp, mask, truth, eps = TC.make_batch(dev, BASE, seed=seed)
        batches.append({"tp_to_predict": tpp, "observed_data": data, "observed_tp": tp, "observed_mask": mask, "data_to_predict": truth,
                        "mask_predicted_data": (truth > -0.5).float()})
    m.eps_override = eps      # one recorded draw for both engines
    ev = immtsf.EvalStep(m, None)
    n0 = m.fused_calls
    for b in batches:
        ev(b)
    assert (ev.eager, ev.captures, ev.replays) == (1, 1, 1)
    assert m.fused_calls > n0
    got = ev.result()
    nog = immtsf.EvalStep(m, None, graph=False)
    for b in batches:
        nog(b)
    ref = nog.result()
    for key in ref:
        assert got[key] == pytest.approx(ref[key], rel=1e-12), key
    with _knob(True):
        k_on = ev._key(batches[0], sorted(batches[0]))
    with _knob(False):
        k_off = ev._key(batches[0], sorted(batches[0]))
    assert k_on != k_off
