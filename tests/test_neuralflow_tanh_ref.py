"""CPU checks behind the fused TimeTanh kernels of the NeuralFlow backbone: the float64 yardstick (tests/neuralflow_tanh_ref.py) against
the module's own composed path run in float64, outputs and every gradient at 1e-10, with either time net; the input condition of
tests/neuralflow_tanh_cases.py (1 - phi^2 far from 1, |scale t| past 2, an unobserved point, a padded window); torch's fp32 CPU run of
the yardstick 4x inside the project's bars on every case (the record the GPU bars rest on); the library's time-net queries and the
module's knobs, which need no GPU."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neuralflow_tanh_cases as TC  # noqa: E402

PIN = 1e-10


@pytest.fixture(scope="module")
def references():
    cache = {}

    def get(name, time_net="TimeTanh"):
        if (name, time_net) not in cache:
            case = TC.CASES[name]
            m = TC.make_model("cpu", case, time_net)
            cache[name, time_net] = TC.reference(m, TC.make_batch("cpu", case, unit=time_net == "TimeLinear"))
        return cache[name, time_net]
    return get


@pytest.mark.parametrize("time_net", ["TimeTanh", "TimeLinear"])
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_yardstick_matches_the_composed_module_in_float64(name, time_net, references):
    case = TC.CASES[name]
    m = TC.make_model("cpu", case, time_net).double()
    batch = TC.make_batch("cpu", case, unit=time_net == "TimeLinear")
    out, grads = TC.composed(m, batch)
    want_out, want, _ = references(name, time_net)
    assert out.dtype == torch.float64 and tuple(out.shape) == (case[0], case[2], case[3])
    diff, errs = TC.grad_errors(grads, want)
    e = TC.rel(out, want_out)
    print(name, time_net, "out", e, "worst gradient", max(errs.values()))
    assert not diff, diff
    assert list(grads) == list(want) and all(g is not None and float(g.abs().max()) > 0 for g in want.values())
    assert e <= PIN
    assert not {k: v for k, v in errs.items() if not v <= PIN}


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_inputs_put_the_tanh_factor_far_from_one(name, references):
    """on each case's inputs, by the float64 yardstick alone: 1 - phi^2 deviates from 1 by at least 0.5 and |scale t| passes 2, in the
    encoder's flow and in the generative one; times are sorted; a point is unobserved everywhere; window 0 ends in padding"""
    stats = references(name)[2]
    print(name, stats)
    for flow in ("enc", "gen"):
        assert stats[flow + "_phi2"] >= 0.5, (flow, stats)
        assert stats[flow + "_arg"] > 2, (flow, stats)
    tpp, data, tp, mask, up, eps = TC.make_batch("cpu", TC.CASES[name])
    assert (tp[:, 1:] > tp[:, :-1]).all() and (tpp[:, 1:] > tpp[:, :-1]).all() and (tpp[:, 0] > tp[:, -1]).all()
    assert not mask[:, 1].any() and not mask[0, -2:].any() and mask[1:, -1].any() and not data[mask == 0].any()


def test_yardstick_tells_the_two_time_nets_apart(references):
    """the same parameters and batch under the other time net give another forecast and another gradient of time_net.scale"""
    case = TC.CASES["a_defaults"]
    m, batch = TC.make_model("cpu", case, "TimeTanh"), TC.make_batch("cpu", case)
    out_t, g_t, _ = references("a_defaults")
    m.nf_args.time_net = "TimeLinear"
    out_l, g_l, _ = TC.reference(m, batch)
    assert TC.rel(out_l, out_t) > 1e-2
    assert all(TC.rel(g_l[k], g_t[k]) > 1e-2 for k in TC.scale_keys(g_t))


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_fp32_cpu_run_of_the_yardstick_sits_4x_inside_the_bars(name, references):
    case = TC.CASES[name]
    got_out, got, _ = TC.reference(TC.make_model("cpu", case), TC.make_batch("cpu", case), dtype=torch.float32)
    want_out, want, _ = references(name)
    diff, errs = TC.grad_errors(got, want)
    e = TC.rel(got_out, want_out)
    print(name, "out", e, "worst gradient", max(errs, key=errs.get), max(errs.values()))
    assert not diff and e <= TC.OUT_TOL / 4 and max(errs.values()) <= TC.GRAD_TOL / 4


def test_time_net_queries_run_without_gpu():
    from immtsf import _lib, ops
    lib = _lib.load()
    D = _lib.NeuralFlowDims      # B, L, Lp, C, rec_dims, latents, hidden_dim, hidden_layers, flow_layers
    main = (40, 20, 32, 3, 2)
    for dims in ((64, 24, 24, 5) + main, (8, 3, 2, 64) + main, (3, 5, 4, 3, 8, 6, 8, 2, 2), (4, 4, 4, 5, 65, 20, 32, 3, 2),
                 (4, 4, 4, 5, 64, 64, 128, 4, 4), (0, 24, 24, 5) + main):
        d = D(*dims)
        for kind in (0, 1):      # the same limits, parameter layout and workspace for both time nets: no phi tile is saved
            assert lib.immtsf_neural_flow_tn_supported(ctypes.byref(d), kind) == lib.immtsf_neural_flow_supported(ctypes.byref(d))
            assert lib.immtsf_neural_flow_tn_param_count(ctypes.byref(d), kind) == lib.immtsf_neural_flow_param_count(ctypes.byref(d))
            assert lib.immtsf_neural_flow_tn_workspace_bytes(ctypes.byref(d), kind) == lib.immtsf_neural_flow_workspace_bytes(ctypes.byref(d))
        for kind in (-1, 2, 7):
            assert lib.immtsf_neural_flow_tn_supported(ctypes.byref(d), kind) == 0
            assert lib.immtsf_neural_flow_tn_param_count(ctypes.byref(d), kind) == -1
            assert lib.immtsf_neural_flow_tn_workspace_bytes(ctypes.byref(d), kind) == 0
    assert lib.immtsf_neural_flow_tn_supported(None, 1) == 0
    assert lib.immtsf_neural_flow_tn_supported(ctypes.byref(D(8, 3, 2, 64, *main)), 1) == 1      # c_envelope, the top of the envelope
    assert ops.NEURAL_FLOW_TIME_NETS == {"TimeLinear": 0, "TimeTanh": 1}
    assert ops.neural_flow_supported(64, 24, 24, 5, *main, call=True, time_net="TimeTanh")
    assert ops.neural_flow_supported(64, 24, 24, 5, *main, call=True) and not ops.neural_flow_supported(0, 24, 24, 5, *main, call=True, time_net="TimeTanh")
    assert not ops.neural_flow_supported(64, 24, 24, 5, *main, time_net="TimeFourier")


def test_the_knobs_and_the_state_dict_do_not_depend_on_the_time_net():
    from immtsf import config
    assert config.neuralflow_tanh_fused is (os.environ.get("IMMTSF_NEURALFLOW_TANH_FUSED", "0") == "1")
    case = TC.CASES["a_defaults"]
    a, b = TC.make_model("cpu", case, "TimeTanh"), TC.make_model("cpu", case, "TimeLinear")
    assert list(a.state_dict()) == list(b.state_dict())
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())      # the same draws, the same initial values
    assert a.immtsf_graphable and a.fused_calls == 0
    was = config.neuralflow_fused, config.neuralflow_tanh_fused
    try:
        for fused, tanh, want_t in ((True, True, True), (True, False, False), (False, True, False), (False, False, False)):
            config.neuralflow_fused, config.neuralflow_tanh_fused = fused, tanh
            assert a._static_fused_ok() is want_t and b._static_fused_ok() is fused
        config.neuralflow_fused, config.neuralflow_tanh_fused = True, True
        wide = TC.make_model("cpu", case, "TimeTanh", nf_hidden_dim=129)
        assert not wide._static_fused_ok()
    finally:
        config.neuralflow_fused, config.neuralflow_tanh_fused = was
