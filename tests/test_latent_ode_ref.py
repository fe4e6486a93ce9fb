"""CPU checks of the LatentODE backbone's yardstick, module layout and limits: the float64 restatement (tests/latent_ode_ref.py) against
the real reference's goldens (tests/golden/model_latentode*.npz, written by tests/golden/make_golden_latentode.py with the recorded
noise), gradients and the set of gradient-less parameters included; for every shape of tests/latent_ode_cases.py, how far torch's own
fp32 CPU run of the restatement is from its float64 run (the record the GPU bars are built on); the step plan's vectorised float32
form against the reference's scalar loop; the product module's state-dict keys, initial values, option handling and refusal of CPU
tensors; the library's limit and workspace queries (host arithmetic).

Measured fp32-against-float64 errors (output / worst gradient): 6.5e-8 .. 3.3e-7 / 1.7e-7 .. 1.1e-6 over all shapes and goldens, so
every shape keeps the project's 1e-4 / 3e-4 bars; the float64 restatement against the goldens (the reference's fp32 run): 8.1e-8 ..
1.2e-7 / 2.6e-7 .. 7.1e-7."""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_ode_cases as TC  # noqa: E402
import latent_ode_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    params = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p.")}
    return z, params, set(str(z["none"]).split("\n")) - {""}


def _golden_run(name, dtype):
    z, params, none = _golden(name)
    return R.run(params, z["tpp"], z["data"], z["tp"], z["mask"], z["eps"], z["upstream"], dtype=dtype)


@pytest.mark.parametrize("name", sorted(TC.GOLDENS))
def test_restatement_matches_reference_golden(name):
    """the golden is the reference's fp32 run: the float64 restatement agrees with it to 4x the restatement's own fp32 error"""
    z, params, none = _golden(name)
    out, grads = _golden_run(name, torch.float64)
    e_out, e_grad = TC.FP32_ERR[name]
    assert tuple(out.shape) == z["out"].shape
    assert {k for k, g in grads.items() if g is None} == none
    assert sorted("g." + k for k in grads if k not in none) == sorted(f for f in z.files if f.startswith("g."))
    want = {k: (None if k in none else torch.from_numpy(z["g." + k])) for k in grads}
    diff, errs = TC.grad_errors(grads, want)
    print(name, "out", TC.rel(out, z["out"]), "worst grad", max(errs.values()))
    assert not diff
    assert TC.rel(out, z["out"]) <= 4 * e_out
    assert max(errs.values()) <= 4 * e_grad, max(errs, key=errs.get)


def test_goldens_reach_the_branches_they_are_named_for():
    steps = {name: R.plan(_golden(name)[0]["tp"]) for name in ("model_latentode", "model_latentode_span", "model_latentode_default")}
    small = steps["model_latentode"]
    assert not small[-1][0] and small[-1][1] == 1          # span < 0.5: the 0.01 lead-in is one RK4 step
    assert small[0][0]                                      # a gap below minimum_step: Euler
    assert small[1] [:2] == (False, 1) and max(n for _, n, _ in small) == 21
    assert steps["model_latentode_span"][-1][0] and steps["model_latentode_default"][-1][0]      # span > 0.5: the lead-in is Euler
    z = _golden("model_latentode")[0]
    assert not z["mask"][1].any() and z["mask"][0, 2].any() and not z["mask"][1:, 2].any()
    assert _golden("model_latentode_L1")[0]["tp"].shape == (1,) and _golden("model_latentode_L1")[0]["out"].shape == (3, 1, 3)


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
    built on (latent_ode_cases.FP32_ERR), which sits 4x inside the project's bars"""
    case = TC.case_of(name)
    m, batch = TC.make_model("cpu", case), TC.make_batch("cpu", case)
    want_out, want = TC.reference(m, batch)
    got_out, got = TC.reference(m, batch, dtype=torch.float32)
    e_out = TC.rel(got_out, want_out)
    diff, errs = TC.grad_errors(got, want)
    print(name, "out", e_out, "worst grad", max(errs.values()))
    assert not diff and not torch.isnan(want_out).any()
    assert e_out <= TC.FP32_ERR[name][0] and max(errs.values()) <= TC.FP32_ERR[name][1], max(errs, key=errs.get)
    assert TC.bars(name) == (TC.OUT_TOL, TC.GRAD_TOL)
    assert tuple(want_out.shape) == (case[0], len(case[3]), case[1])


@pytest.mark.parametrize("times", [TC.T7, TC.T7_WIDE, TC.T5, [0.0, 0.001, 0.002, 0.0035]])
def test_step_plan_is_the_references_decision(times):
    """the vectorised float32 plan against the reference's scalar loop (Encoder_z0_ODE_RNN.run_odernn), decision by decision"""
    from models.LatentODE import step_plan
    t = torch.tensor(times)
    euler, nsub, gap = step_plan(t)
    prev_t, t_i = t[-1] + 0.01, t[-1]
    minimum_step = (t[-1] - t[0]) / 50
    for i in reversed(range(len(t))):
        is_euler = bool((prev_t - t_i) < minimum_step)
        assert bool(euler[i]) == is_euler and torch.equal(gap[i], t_i - prev_t)
        if not is_euler:
            assert int(nsub[i]) == max(2, ((prev_t - t_i) / minimum_step).int())
        prev_t, t_i = t[i], t[i - 1]
    if times[-1] < 0.01:      # a span of 0.0035: the lead-in asks for 0.01 / 7e-5 = 142 grid points
        assert int(nsub[-1]) == 142


@pytest.mark.parametrize("name", sorted(TC.GOLDENS))
def test_product_module_has_the_goldens_state_dict_and_initial_values(name):
    from models.LatentODE import LatentODE
    C, options = TC.GOLDENS[name]
    z, params, none = _golden(name)
    torch.manual_seed(TC.GOLDEN_SEEDS[name] + 2)
    m = LatentODE(TC.config(C, **options))
    sd = m.state_dict()
    assert list(sd) == str(z["keys"]).split("\n") == [k[2:] for k in z.files if k.startswith("i.")]
    for key, v in sd.items():
        assert np.array_equal(v.numpy(), z["i." + key]), key
    assert m.fused_calls == 0 and m.immtsf_graphable == (options.get("ode_z0_encoder", "odernn") == "odernn")


def test_state_dict_keys_option_defaults_and_errors():
    from models.LatentODE import LatentODE
    m = LatentODE(TC.config(5))
    a = m.args_for_ode
    assert (a.latents, a.units, a.gen_layers, a.rec_dims, a.rec_layers, a.gru_units, a.z0_encoder) == (20, 32, 1, 32, 1, 32, "odernn")
    assert m.obsrv_std_val == 0.01
    want = [f"latent_ode_model_core.encoder_z0.GRU_update.{n}.{i}.{w}" for n in ("update_gate", "reset_gate", "new_state_net") for i in (0, 2)
            for w in ("weight", "bias")]
    want += [f"latent_ode_model_core.encoder_z0.z0_diffeq_solver.ode_func.gradient_net.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")]
    want += [f"latent_ode_model_core.encoder_z0.transform_z0.{i}.{w}" for i in (0, 2) for w in ("weight", "bias")]
    want += [f"latent_ode_model_core.diffeq_solver.ode_func.gradient_net.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")]
    want += [f"latent_ode_model_core.decoder.decoder.0.{w}" for w in ("weight", "bias")]
    assert list(m.state_dict()) == want
    assert all(float(v.abs().max()) == 0 for k, v in m.state_dict().items() if k.endswith("bias"))
    assert LatentODE(TC.config(5, ode_gru_units=None, hid_dim=48)).args_for_ode.gru_units == 48
    for option in ("ode_poisson", "ode_classif", "ode_linear_classif"):
        with pytest.raises(NotImplementedError, match=option):
            LatentODE(TC.config(5, **{option: True}))
    with pytest.raises(Exception, match="Unknown encoder"):
        LatentODE(TC.config(5, ode_z0_encoder="mlp"))


def test_refuses_cpu_tensors():
    from immtsf._lib import ImmtsfError
    case = TC.CASES["a_small"]
    m, batch = TC.make_model("cpu", case), TC.make_batch("cpu", case)
    with pytest.raises(ImmtsfError):
        m.forecasting(*batch[:4])


def test_imports_with_no_reference_tree_on_the_path():
    pkg = os.path.join(ROOT, "imm-tsf_amd")
    code = """
        import sys, models.LatentODE as M
        assert 'imm-tsf_amd' in M.__file__
        assert not any(k.startswith('lib.latent_ode_components') or k == 'torchdiffeq' for k in sys.modules)
        from immtsf.ops import latent_ode
        print('ok')
        """
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=dict(os.environ, PYTHONPATH=pkg), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_supported_count_and_workspace_queries_run_without_gpu():
    from immtsf import _lib, config, ops
    lib = _lib.load()
    D = _lib.LatentODEDims      # B, L, Lp, C, rec_dims, units, gru_units, latents
    sup = lambda *a: lib.immtsf_latent_ode_supported(ctypes.byref(D(*a)))      # noqa: E731
    assert sup(64, 24, 24, 5, 32, 32, 32, 20) == 1 and sup(0, 1, 1, 1, 1, 1, 1, 1) == 1 and sup(3, 7, 4, 3, 8, 12, 10, 6) == 1
    assert sup(1, 1 << 20, 1 << 20, 5, 32, 32, 32, 20) == 1
    assert sup(4, 0, 4, 5, 32, 32, 32, 20) == 0 and sup(4, 4, 0, 5, 32, 32, 32, 20) == 0 and sup(-1, 4, 4, 5, 32, 32, 32, 20) == 0
    assert sup(4, 4, 4, 65, 32, 32, 32, 20) == 0 and sup(4, 4, 4, 5, 65, 32, 32, 20) == 0 and sup(4, 4, 4, 5, 32, 129, 32, 20) == 0
    assert sup(4, 4, 4, 5, 32, 32, 129, 20) == 0 and sup(4, 4, 4, 5, 32, 32, 32, 65) == 0 and sup(4, 4, 4, 0, 32, 32, 32, 20) == 0
    assert sup(4, 4, 4, 64, 64, 128, 128, 64) == 0          # inside every limit, but the weights do not fit the LDS plan
    assert lib.immtsf_latent_ode_supported(None) == 0
    count = lambda *a: lib.immtsf_latent_ode_param_count(ctypes.byref(D(*a)))      # noqa: E731
    for case in (TC.CASES["a_small"], TC.CASES["e_defaults"]):
        m = TC.make_model("cpu", case)
        a = m.args_for_ode
        assert count(1, 1, 1, case[1], a.rec_dims, a.units, a.gru_units, a.latents) == sum(p.numel() for p in m.parameters())
    assert count(1, 1, 1, 5, 65, 32, 32, 20) == -1
    ws = lambda *a: lib.immtsf_latent_ode_workspace_bytes(ctypes.byref(D(*a)))      # noqa: E731
    nv = count(1, 1, 1, 5, 32, 32, 32, 20)
    assert ws(64, 24, 24, 5, 32, 32, 32, 20) == 4 * (((8 * nv + 63) & ~63) + 8 * 256 * 8 * 32) + 256
    assert ws(9, 7, 4, 3, 8, 12, 10, 6) == 4 * (((2 * count(1, 1, 1, 3, 8, 12, 10, 6) + 63) & ~63) + 2 * 256 * 8 * 8) + 256
    assert ws(0, 24, 24, 5, 32, 32, 32, 20) == 0 and ws(4, 24, 24, 5, 65, 32, 32, 20) == 0 and ws(1 << 20, 1 << 20, 4, 5, 32, 32, 32, 20) == 0
    assert ops.latent_ode_supported(64, 24, 24, 5, 32, 32, 32, 20, call=True) and not ops.latent_ode_supported(0, 24, 24, 5, 32, 32, 32, 20, call=True)
    assert config.latentode_fused is (os.environ.get("IMMTSF_LATENTODE_FUSED", "1") != "0")
