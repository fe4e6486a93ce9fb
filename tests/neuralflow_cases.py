"""Shapes, models and batches shared by tests/test_neuralflow_ref.py (CPU: the restatement's own fp32 error) and
tests/test_gpu_neuralflow.py (GPU parity): the goldens' shapes plus the smallest extra ones at which csrc/neural_flow.hip takes another
path -- nine windows (a tile of eight and a second workgroup with one), one channel, one observed point, one forecast time, odd
rec_dims and latents (the coupling mask splits at dim // 2), one and three flow layers (the mask alternates), the defaults.  Wherever
there are three or more observed points window 1 has no observation at all.  A model's parameters are drawn on the CPU from a fixed
seed, so both files see the same numbers.  Every window has its own times, in [0, 1].

FP32_ERR is the record of tests/test_neuralflow_ref.py: torch's fp32 CPU run of the restatement against its float64 run (output
relative to max; worst gradient relative to max(|want|, 1e-2 of the largest gradient)), doubled and rounded up to two digits.  The
project's fp32 bars (1e-4 / 3e-4) hold for a shape whose recorded error sits 4x inside them; for any other the bar is 4x the recorded
error -- bars() below, the rule of tests/latent_ode_cases.py.  Nothing here comes from the kernel."""
import types

import torch

import neuralflow_ref as R

OUT_TOL, GRAD_TOL, GRAD_FLOOR = 1e-4, 3e-4, 1e-2      # the project's fp32 bars (test_gpu_timemixer.py)
TILE = 8                                              # NF_WT of csrc/neural_flow.hip

SMALL = dict(nf_latents=6, nf_rec_dims=8, nf_hidden_dim=12, nf_hidden_layers=2)

# name: (B, C, L, Lp, options)
CASES = {
    "a_small": (3, 3, 7, 4, SMALL),
    "b_nine_windows": (TILE + 1, 3, 7, 4, SMALL),
    "c_one_channel": (3, 1, 7, 4, SMALL),
    "d_one_observed_point": (3, 3, 1, 4, SMALL),
    "e_one_forecast_time": (3, 3, 7, 1, SMALL),
    "f_odd_widths": (3, 3, 7, 4, dict(SMALL, nf_rec_dims=7, nf_latents=5)),
    "g_one_flow_layer": (3, 3, 7, 4, dict(SMALL, nf_flow_layers=1)),
    "h_three_flow_layers": (3, 3, 7, 4, dict(SMALL, nf_flow_layers=3)),
    "i_defaults": (2, 5, 5, 2, {}),
}
# options outside the fused path (the composed path's, a_small otherwise)
UNSUPPORTED = {
    "time_tanh": dict(SMALL, nf_time_net="TimeTanh"),
}
# the goldens of the reference's own code (tests/golden/model_neuralflow*.npz): name -> (C, L, Lp, options, seed)
GOLDENS = {
    "model_neuralflow_default": (5, 5, 2, {}, 191),
    "model_neuralflow": (3, 7, 4, SMALL, 193),
    "model_neuralflow_L1": (3, 1, 1, SMALL, 195),
    "model_neuralflow_tanh": (3, 7, 4, dict(SMALL, nf_time_net="TimeTanh"), 197),
}

# name: (output, worst gradient) of torch's fp32 CPU run of the restatement against float64
FP32_ERR = {
    "a_small": (4.3e-07, 8.6e-07),
    "b_nine_windows": (5.1e-07, 6.7e-07),
    "c_one_channel": (2.3e-07, 4.6e-07),
    "d_one_observed_point": (3.9e-07, 1.3e-06),
    "e_one_forecast_time": (1.8e-07, 5.9e-07),
    "f_odd_widths": (2.6e-07, 7.2e-07),
    "g_one_flow_layer": (1.4e-07, 8.8e-07),
    "h_three_flow_layers": (1.7e-07, 1.1e-06),
    "i_defaults": (3.6e-07, 9.4e-07),
    "time_tanh": (3.6e-07, 7.7e-07),
    "model_neuralflow_default": (2.8e-07, 8.3e-07),
    "model_neuralflow": (2.1e-07, 5.5e-07),
    "model_neuralflow_L1": (2.7e-07, 4.8e-07),
    "model_neuralflow_tanh": (2.2e-07, 7.3e-07),
}


def bars(name):
    """-> (output bar, gradient bar) of a case: the project's where the recorded fp32 error is 4x inside them, else 4x that error"""
    e_out, e_grad = FP32_ERR[name]
    return (OUT_TOL if e_out <= OUT_TOL / 4 else 4 * e_out), (GRAD_TOL if e_grad <= GRAD_TOL / 4 else 4 * e_grad)


def config(C, L, Lp, device="cpu", **options):
    return types.SimpleNamespace(input_len=L, pred_len=Lp, enc_in=C, device=torch.device(device), **options)


def case_of(name):
    """a CASES entry, or a_small under the options of an UNSUPPORTED entry"""
    if name in CASES:
        return CASES[name]
    return CASES["a_small"][:4] + (UNSUPPORTED[name],)


def time_net_of(options):
    return options.get("nf_time_net", "TimeLinear")


def make_model(dev, case, seed=0):
    """the product's NeuralFlow on `dev`, every parameter 0.1 randn off its init (transform_z0's and the decoder's biases start at zero)"""
    from models.NeuralFlow import NeuralFlow
    B, C, L, Lp, options = case
    torch.manual_seed(1000 + seed)
    m = NeuralFlow(config(C, L, Lp, **options))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    m.device = torch.device(dev)
    return m.to(dev).train()


def make_batch(dev, case, seed=7):
    """-> (tpp (B, Lp), data, tp (B, L), mask, upstream, eps (1, B, latents)): observed times in [0, 0.6], forecast times in [0.62, 1],
    increasing per window; masks about 70 % ones; window 1 has no observation at all, point 2 is observed by window 0 only (where there
    are that many)"""
    B, C, L, Lp, options = case
    g = torch.Generator().manual_seed(seed)
    tp = torch.sort(torch.rand(B, L, generator=g) * 0.6, dim=1).values
    tpp = 0.62 + torch.sort(torch.rand(B, Lp, generator=g) * 0.38, dim=1).values
    data = torch.randn(B, L, C, generator=g)
    mask = (torch.rand(B, L, C, generator=g) < 0.7).float()
    if L > 2:
        mask[:, L // 2, 0] = 1
        mask[1] = 0
        mask[:, 2] = 0
        mask[0, 2, 0] = 1
    up = torch.randn(B, Lp, C, generator=g)
    eps = torch.randn(1, B, options.get("nf_latents", 20), generator=g)
    return tuple(t.to(dev) for t in (tpp, data * mask, tp, mask, up, eps))


def ref_params(m):
    return {k: v.detach().cpu() for k, v in m.state_dict().items()}


def reference(m, batch, dtype=torch.float64):
    """-> (out, name -> gradient or None) of the restatement on the module's parameters"""
    tpp, data, tp, mask, up, eps = (t.cpu() for t in batch)
    return R.run(ref_params(m), tpp, data, tp, mask, eps, up, dtype=dtype, time_net=m.nf_args.time_net)


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
