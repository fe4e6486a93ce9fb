"""CPU checks of the NeuralFlow backbone's yardstick, module layout and limits: the float64 restatement (tests/neuralflow_ref.py) against
the goldens of the reference's own code (tests/golden/model_neuralflow*.npz, written by tests/golden/make_golden_neuralflow.py with the
recorded noise; the coupling layer inside them is a stand-in of `stribor`'s, see there), gradients, the set of gradient-less parameters
and the state_dict's key order included; for every shape of tests/neuralflow_cases.py, how far torch's own fp32 CPU run of the
restatement is from its float64 run (the record the GPU bars are built on); the product module's import without `stribor`, its
state-dict keys, initial values, option handling and refusal of CPU tensors; the library's limit and workspace queries (host
arithmetic)."""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neuralflow_cases as TC  # noqa: E402
import neuralflow_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    params = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p.")}
    return z, params, set(str(z["none"]).split("\n")) - {""}


def _golden_run(name, dtype):
    z, params, none = _golden(name)
    return R.run(params, z["tpp"], z["data"], z["tp"], z["mask"], z["eps"], z["upstream"], dtype=dtype,
                 time_net=TC.time_net_of(TC.GOLDENS[name][3]))


@pytest.mark.parametrize("name", sorted(TC.GOLDENS))
def test_restatement_matches_reference_golden(name):
    """the golden is the reference's fp32 run: the float64 restatement agrees with it to 4x the restatement's own fp32 error, has the
    same parameters without a gradient, and names its parameters as the golden's state_dict does, in order"""
    z, params, none = _golden(name)
    out, grads = _golden_run(name, torch.float64)
    e_out, e_grad = TC.FP32_ERR[name]
    assert tuple(out.shape) == z["out"].shape
    assert list(grads) == str(z["keys"]).split("\n")
    assert {k for k, g in grads.items() if g is None} == none
    assert sorted("g." + k for k in grads if k not in none) == sorted(f for f in z.files if f.startswith("g."))
    want = {k: (None if k in none else torch.from_numpy(z["g." + k])) for k in grads}
    diff, errs = TC.grad_errors(grads, want)
    print(name, "out", TC.rel(out, z["out"]), "worst grad", max(errs.values()))
    assert not diff
    assert TC.rel(out, z["out"]) <= 4 * e_out
    assert max(errs.values()) <= 4 * e_grad, max(errs, key=errs.get)


def test_goldens_have_the_shapes_and_masks_they_are_named_for():
    z = _golden("model_neuralflow")[0]
    assert z["tp"].shape == (3, 7) and z["tpp"].shape == (3, 4) and not np.array_equal(z["tp"][0], z["tp"][1])
    assert not z["mask"][1].any() and z["mask"][0, 2].any() and not z["mask"][1:, 2].any()
    for name in TC.GOLDENS:
        g = _golden(name)[0]
        assert 0 <= g["tp"].min() and g["tpp"].max() <= 1 and (np.diff(g["tp"], axis=1) > 0).all()
    one = _golden("model_neuralflow_L1")[0]
    assert one["tp"].shape == (3, 1) and one["out"].shape == (3, 1, 3)
    d = _golden("model_neuralflow_default")[0]
    assert d["out"].shape == (2, 2, 5) and d["p.nf_model_core.encoder_z0.lstm.weight_hh"].shape == (160, 40)
    assert d["p.nf_model_core.diffeq_solver.solver.flow.transforms.1.time_net.scale"].shape == (1, 40)


@pytest.mark.parametrize("name", sorted(TC.GOLDENS))
def test_fp32_cpu_error_on_the_goldens_is_the_recorded_one(name):
    want_out, want = _golden_run(name, torch.float64)
    got_out, got = _golden_run(name, torch.float32)
    diff, errs = TC.grad_errors(got, want)
    print(name, "out", TC.rel(got_out, want_out), "worst grad", max(errs.values()))
    assert not diff and TC.rel(got_out, want_out) <= TC.FP32_ERR[name][0] and max(errs.values()) <= TC.FP32_ERR[name][1]
    assert TC.bars(name) == (TC.OUT_TOL, TC.GRAD_TOL)


@pytest.mark.parametrize("name", sorted(TC.CASES) + sorted(TC.UNSUPPORTED))
def test_fp32_cpu_error_is_the_recorded_one(name):
    """torch's fp32 CPU run of the restatement against float64 on every shape of the GPU parity list: within the record the bars are
    built on (neuralflow_cases.FP32_ERR), which sits 4x inside the project's bars"""
    case = TC.case_of(name)
    m, batch = TC.make_model("cpu", case), TC.make_batch("cpu", case)
    want_out, want = TC.reference(m, batch)
    got_out, got = TC.reference(m, batch, dtype=torch.float32)
    e_out = TC.rel(got_out, want_out)
    diff, errs = TC.grad_errors(got, want)
    print(name, "out", e_out, "worst grad", max(errs.values()))
    assert not diff and not torch.isnan(want_out).any()
    assert all(g is not None and float(g.abs().max()) > 0 for g in want.values())
    assert e_out <= TC.FP32_ERR[name][0] and max(errs.values()) <= TC.FP32_ERR[name][1], max(errs, key=errs.get)
    assert TC.bars(name) == (TC.OUT_TOL, TC.GRAD_TOL)
    assert tuple(want_out.shape) == (case[0], case[3], case[1])


@pytest.mark.parametrize("name", sorted(TC.GOLDENS))
def test_product_module_has_the_goldens_state_dict_and_initial_values(name):
    from models.NeuralFlow import NeuralFlow
    C, L, Lp, options, seed = TC.GOLDENS[name]
    z, params, none = _golden(name)
    torch.manual_seed(seed + 2)
    m = NeuralFlow(TC.config(C, L, Lp, **options))
    sd = m.state_dict()
    assert list(sd) == str(z["keys"]).split("\n") == [k[2:] for k in z.files if k.startswith("i.")]
    assert [k for k, _ in m.named_parameters()] == list(sd)      # the flat parameter buffer of the fused path is in this order
    for key, v in sd.items():
        assert np.array_equal(v.numpy(), z["i." + key]), key
    assert m.fused_calls == 0 and m.immtsf_graphable


def test_state_dict_keys_option_defaults_and_errors():
    from models.NeuralFlow import NeuralFlow
    m = NeuralFlow(TC.config(5, 24, 24))
    a = m.nf_args
    assert (a.latents, a.rec_dims, a.hidden_layers, a.hidden_dim, a.flow_model, a.flow_layers, a.time_net) == (20, 40, 3, 32, "coupling", 2,
                                                                                                               "TimeLinear")
    assert (m.input_len, m.pred_len, m.enc_in, m.obsrv_std_val) == (24, 24, 5, 0.01)
    flow = [f"transforms.{i}.{n}" for i in (0, 1) for n in [f"latent_net.net.{j}.{w}" for j in (0, 2, 4, 6) for w in ("weight", "bias")] +
            ["time_net.scale"]]
    want = [f"nf_model_core.encoder_z0.lstm.{n}" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    want += [f"nf_model_core.encoder_z0.z0_diffeq_solver.solver.flow.{n}" for n in flow]
    want += [f"nf_model_core.encoder_z0.transform_z0.{i}.{w}" for i in (0, 2) for w in ("weight", "bias")]
    want += [f"nf_model_core.diffeq_solver.solver.flow.{n}" for n in flow]
    want += [f"nf_model_core.decoder.decoder.0.{w}" for w in ("weight", "bias")]
    assert list(m.state_dict()) == want
    sd = m.state_dict()
    assert sd["nf_model_core.encoder_z0.lstm.weight_ih"].shape == (160, 10)
    assert sd["nf_model_core.encoder_z0.z0_diffeq_solver.solver.flow.transforms.0.latent_net.net.0.weight"].shape == (32, 41)
    assert sd["nf_model_core.diffeq_solver.solver.flow.transforms.1.latent_net.net.6.weight"].shape == (40, 32)
    with pytest.raises(NotImplementedError, match="nf_flow_model"):
        NeuralFlow(TC.config(5, 24, 24, nf_flow_model="resnet"))
    with pytest.raises(NotImplementedError, match="nf_time_net"):
        NeuralFlow(TC.config(5, 24, 24, nf_time_net="TimeFourier"))
    with pytest.raises(ValueError, match="Unknown flow transformation"):
        NeuralFlow(TC.config(5, 24, 24, nf_flow_model="gru"))
    one = NeuralFlow(TC.config(1, 4, 4, nf_rec_dims=1, nf_latents=1))
    assert all(float(f.mask.abs().max()) == 0 for f in one.nf_model_core.diffeq_solver.solver.flow.transforms)      # 'none' at dim == 1
    odd = NeuralFlow(TC.config(3, 4, 4, nf_latents=5, nf_flow_layers=3)).nf_model_core.diffeq_solver.solver.flow.transforms
    assert [f.mask.tolist() for f in odd] == [[1, 1, 0, 0, 0], [0, 0, 1, 1, 1], [1, 1, 0, 0, 0]]


def test_refuses_cpu_tensors():
    from immtsf._lib import ImmtsfError
    case = TC.CASES["a_small"]
    m, batch = TC.make_model("cpu", case), TC.make_batch("cpu", case)
    with pytest.raises(ImmtsfError):
        m.forecasting(*batch[:4])


def test_imports_with_no_stribor_and_no_reference_tree():
    """`import models.NeuralFlow` needs neither stribor nor lib.neural_flow_components nor lib.utils"""
    pkg = os.path.join(ROOT, "imm-tsf_amd")
    code = """
        import sys, models.NeuralFlow as M
        assert 'imm-tsf_amd' in M.__file__
        assert not any(k == 'stribor' or k.startswith('stribor.') or k.startswith('lib.neural_flow_components') or k == 'lib.utils'
                       or k == 'torchdiffeq' for k in sys.modules)
        assert M.NeuralFlow.__module__ == 'models.NeuralFlow'
        from immtsf.ops import neural_flow, neural_flow_supported
        print('ok')
        """
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=dict(os.environ, PYTHONPATH=pkg), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_supported_count_and_workspace_queries_run_without_gpu():
    from immtsf import _lib, config, ops
    lib = _lib.load()
    D = _lib.NeuralFlowDims      # B, L, Lp, C, rec_dims, latents, hidden_dim, hidden_layers, flow_layers
    sup = lambda *a: lib.immtsf_neural_flow_supported(ctypes.byref(D(*a)))      # noqa: E731
    main = (40, 20, 32, 3, 2)      # the widths the reference's main.py forces for this model
    assert sup(64, 24, 24, 5, *main) == 1 and sup(64, 24, 24, 64, *main) == 1 and sup(0, 1, 1, 1, 1, 1, 1, 1, 1) == 1
    assert sup(3, 7, 4, 3, 8, 6, 12, 2, 2) == 1 and sup(3, 7, 4, 3, 7, 5, 12, 2, 3) == 1 and sup(1, 1 << 20, 1 << 20, 5, *main) == 1
    assert sup(4, 0, 4, 5, *main) == 0 and sup(4, 4, 0, 5, *main) == 0 and sup(-1, 4, 4, 5, *main) == 0 and sup(4, 4, 4, 0, *main) == 0
    assert sup(4, 4, 4, 65, *main) == 0 and sup(4, 4, 4, 5, 65, 20, 32, 3, 2) == 0 and sup(4, 4, 4, 5, 40, 65, 32, 3, 2) == 0
    assert sup(4, 4, 4, 5, 40, 20, 129, 3, 2) == 0 and sup(4, 4, 4, 5, 40, 20, 32, 5, 2) == 0 and sup(4, 4, 4, 5, 40, 20, 32, 3, 5) == 0
    assert sup(4, 4, 4, 5, 40, 20, 32, 0, 2) == 0 and sup(4, 4, 4, 5, 40, 20, 32, 3, 0) == 0
    assert sup(4, 4, 4, 5, 64, 64, 128, 4, 4) == 0          # inside every limit, but the nets do not fit the LDS plan
    assert lib.immtsf_neural_flow_supported(None) == 0
    count = lambda *a: lib.immtsf_neural_flow_param_count(ctypes.byref(D(*a)))      # noqa: E731
    for name in ("a_small", "f_odd_widths", "h_three_flow_layers", "i_defaults"):
        case = TC.CASES[name]
        m = TC.make_model("cpu", case)
        assert count(1, 1, 1, case[1], *m._widths()) == sum(p.numel() for p in m.parameters()), name
    assert count(1, 1, 1, 5, 65, 20, 32, 3, 2) == -1
    ws = lambda *a: lib.immtsf_neural_flow_workspace_bytes(ctypes.byref(D(*a)))      # noqa: E731
    up64 = lambda n: (n + 63) & ~63      # noqa: E731
    nve = 160 * 10 + 160 * 40 + 320 + 2 * (32 * 41 + 32 + 2 * (32 * 32 + 32) + 80 * 32 + 80 + 80) + 100 * 40 + 100 + 40 * 100 + 40
    nvd = 2 * (32 * 21 + 32 + 2 * (32 * 32 + 32) + 40 * 32 + 40 + 40) + 5 * 20 + 5
    assert nve + nvd == count(1, 1, 1, 5, *main)
    assert ws(64, 24, 24, 5, *main) == 4 * (up64(8 * nve) + up64(192 * nvd) + 64 * 24 * 20) + 256
    assert ws(64, 24, 48, 5, *main) == 4 * (up64(8 * nve) + up64(256 * nvd) + 64 * 48 * 20) + 256      # the decode grid stops at 256
    assert ws(0, 24, 24, 5, *main) == 0 and ws(4, 24, 24, 5, 65, 20, 32, 3, 2) == 0 and ws(1 << 20, 1 << 20, 4, 5, *main) == 0
    assert ops.neural_flow_supported(64, 24, 24, 5, *main, call=True) and not ops.neural_flow_supported(0, 24, 24, 5, *main, call=True)
    assert config.neuralflow_fused is (os.environ.get("IMMTSF_NEURALFLOW_FUSED", "1") != "0")
