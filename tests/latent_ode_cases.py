"""Shapes, models and batches shared by tests/test_latent_ode_ref.py (CPU: the restatement's own fp32 error) and
tests/test_gpu_latent_ode.py (GPU parity): the goldens' shapes plus the smallest extra ones at which csrc/latent_ode.hip takes another
path -- nine windows (a tile of eight and a second workgroup with one), one channel, two forecast points, one observed point.  A model's
parameters are drawn on the CPU from a fixed seed, so both files see the same numbers.  The observed times are the goldens': every
(prev_t - t_i) / minimum_step lies 1e-3 away from an integer and from 1 (tests/golden/make_golden_latentode.py asserts it), so float32
and float64 take the same step plan.

FP32_ERR is the record of tests/test_latent_ode_ref.py: torch's fp32 CPU run of the restatement against its float64 run (output relative
to max; worst gradient relative to max(|want|, 1e-2 of the largest gradient)), doubled and rounded up to two digits: at 1e-7 .. 1e-6 the
figure is a few float32 roundings and moves with the summation order of the CPU's BLAS.  The project's fp32 bars (1e-4 /
3e-4) hold for a shape whose recorded error sits 4x inside them; for any other the bar is 4x the recorded error -- bars() below.
Nothing here comes from the kernel."""
import types

import torch

import latent_ode_ref as R

OUT_TOL, GRAD_TOL, GRAD_FLOOR = 1e-4, 3e-4, 1e-2      # the project's fp32 bars (test_gpu_timemixer.py)
TILE = 8                                              # LO_WT of csrc/latent_ode.hip

SMALL = dict(ode_latents=6, ode_rec_dims=8, ode_units=12, ode_gru_units=10)
T7 = [0.10, 0.105, 0.125, 0.20, 0.36, 0.40, 0.45]      # span 0.35: RK4 lead-in, one Euler gap, one single RK4 step, one of 21 steps
T7_WIDE = [0.0, 0.09, 0.2, 0.33, 0.5, 0.71, 0.93]      # span 0.93: Euler lead-in
T5 = [0.06, 0.2, 0.3, 0.55, 0.8]
P4, P4_WIDE = [0.5, 0.58, 0.7, 0.95], [1.02, 1.2, 1.45, 1.5]

# name: (B, C, observed times, forecast times, options)
CASES = {
    "a_small": (3, 3, T7, P4, SMALL),
    "b_nine_windows": (TILE + 1, 3, T7, P4, SMALL),
    "c_one_channel": (3, 1, T7_WIDE, P4_WIDE, SMALL),
    "d_two_forecast_points": (2, 3, T7, [0.5, 0.9], SMALL),
    "e_defaults": (2, 5, T5, [1.1, 1.35], {}),
    "f_one_observed_point": (3, 3, [0.3], [1.2], SMALL),
}
# options outside the fused path (the composed path's shapes, a_small otherwise)
UNSUPPORTED = {
    "rec_layers_2": dict(SMALL, ode_rec_layers=2),
    "gen_layers_2": dict(SMALL, ode_gen_layers=2),
    "n_traj_samples_3": dict(SMALL, ode_n_traj_samples=3),
    "rnn_encoder": dict(SMALL, ode_z0_encoder="rnn"),
}
# the goldens of the real reference (tests/golden/model_latentode*.npz): name -> (C, options)
GOLDENS = {
    "model_latentode_default": (5, {}),
    "model_latentode": (3, SMALL),
    "model_latentode_span": (3, SMALL),
    "model_latentode_L1": (3, SMALL),
    "model_latentode_rnn": (3, dict(SMALL, ode_z0_encoder="rnn")),
}
GOLDEN_SEEDS = {"model_latentode_default": 91, "model_latentode": 93, "model_latentode_span": 95, "model_latentode_L1": 97,
                "model_latentode_rnn": 99}

# name: (output, worst gradient) of torch's fp32 CPU run of the restatement against float64
FP32_ERR = {
    "a_small": (1.6e-07, 2.2e-06),
    "b_nine_windows": (3.2e-07, 1.1e-06),
    "c_one_channel": (1.7e-07, 1.3e-06),
    "d_two_forecast_points": (2e-07, 7e-07),
    "e_defaults": (6.2e-07, 1.2e-06),
    "f_one_observed_point": (1.4e-07, 3.6e-07),
    "rec_layers_2": (2.6e-07, 2.4e-06),
    "gen_layers_2": (1.6e-07, 2.2e-06),
    "n_traj_samples_3": (2.6e-07, 1.1e-06),
    "rnn_encoder": (6.6e-07, 1.6e-06),
    "model_latentode_default": (3e-07, 1.4e-06),
    "model_latentode": (2.2e-07, 2e-06),
    "model_latentode_span": (2.8e-07, 1.3e-06),
    "model_latentode_L1": (2.2e-07, 5.2e-07),
    "model_latentode_rnn": (2.4e-07, 1e-06),
}


def bars(name):
    """-> (output bar, gradient bar) of a case: the project's where the recorded fp32 error is 4x inside them, else 4x that error"""
    e_out, e_grad = FP32_ERR[name]
    return (OUT_TOL if e_out <= OUT_TOL / 4 else 4 * e_out), (GRAD_TOL if e_grad <= GRAD_TOL / 4 else 4 * e_grad)


def config(C, device="cpu", **options):
    return types.SimpleNamespace(C=C, device=torch.device(device), dataset="cases", **options)


def case_of(name):
    """a CASES entry, or a_small under the options of an UNSUPPORTED entry"""
    if name in CASES:
        return CASES[name]
    return CASES["a_small"][:4] + (UNSUPPORTED[name],)


def make_model(dev, case, seed=0):
    """the product's LatentODE on `dev`, every parameter 0.1 randn off its init (the biases start at zero)"""
    from models.LatentODE import LatentODE
    B, C, tp, tpp, options = case
    torch.manual_seed(1000 + seed)
    m = LatentODE(config(C, **options))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    m.device = torch.device(dev)
    return m.to(dev).train()


def make_batch(dev, case, seed=7):
    """-> (tpp, data, tp, mask, upstream, eps): masks about 70 % ones; window 1 has no observation at all, point 2 is observed by
    window 0 only (where there are that many); eps (n_traj_samples, B, latents)"""
    B, C, tp, tpp, options = case
    L, Lp = len(tp), len(tpp)
    g = torch.Generator().manual_seed(seed)
    data = torch.randn(B, L, C, generator=g)
    mask = (torch.rand(B, L, C, generator=g) < 0.7).float()
    if L > 2:
        mask[:, L // 2, 0] = 1
        mask[1] = 0
        mask[:, 2] = 0
        mask[0, 2, 0] = 1
    up = torch.randn(B, Lp, C, generator=g)
    eps = torch.randn(options.get("ode_n_traj_samples", 1), B, options.get("ode_latents", 20), generator=g)
    return tuple(t.to(dev) for t in (torch.tensor(tpp), data * mask, torch.tensor(tp), mask, up, eps))


def ref_params(m):
    return {k: v.detach().cpu() for k, v in m.state_dict().items()}


def reference(m, batch, dtype=torch.float64):
    """-> (out, name -> gradient or None) of the restatement on the module's parameters"""
    tpp, data, tp, mask, up, eps = (t.cpu() for t in batch)
    return R.run(ref_params(m), tpp, data, tp, mask, eps, up, dtype=dtype)


def rel(a, b, floor=1e-3):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / max(float(b.abs().max()), floor))


def grad_errors(got, want):
    """got / want: name -> gradient or None.  -> (the names whose None-ness differs, name -> error relative to max(|want|, 1e-2 of the
    largest gradient))"""
    gmax = max(float(w.abs().max()) for w in want.values() if w is not None)
    diff = sorted(k for k in want if (want[k] is None) != (got[k] is None))
    return diff, {k: rel(got[k], w, floor=GRAD_FLOOR * gmax) for k, w in want.items() if w is not None and got[k] is not None}
