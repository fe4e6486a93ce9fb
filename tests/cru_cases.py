"""Shapes, models and batches shared by tests/test_cru_ref.py (CPU: the restatement's own fp32 error, the branches the cases reach) and
tests/test_gpu_cru.py (GPU parity): the smallest shapes that reach each branch of csrc/cru.hip.  A model's parameters are drawn on the
CPU from a fixed seed, so both files see the same numbers.

FP32_ERR is the record of tests/test_cru_ref.py::test_fp32_cpu_error_is_the_recorded_one: torch's fp32 CPU run of the restatement against
its float64 run (output relative to max; worst gradient relative to max(|want|, 1e-2 of the largest gradient)), rounded UP to two
digits.  The project's fp32 bars (1e-4 / 3e-4) hold for a shape whose recorded error sits 4x inside them; for the others the bar is 4x
the recorded error (the margin for another, equally valid summation order) -- bars() below.  Nothing here comes from the kernel."""
import types

import torch

import cru_ref as R

OUT_TOL, GRAD_TOL, GRAD_FLOOR = 1e-4, 3e-4, 1e-2      # the project's fp32 bars (test_gpu_timemixer.py)

# name: B, C, L, Lp, lsd, num_basis, bandwidth, hidden, basis scale, batch kind, enc_var_activation, trans_var_activation
CASES = {
    "a_lsd2_band_covers_all": (3, 3, 5, 2, 2, 3, 1, 8, 1.0, "mix", "square", "elup1"),
    "b_lsd8": (3, 3, 6, 3, 8, 4, 2, 16, 1.0, "mix", "square", "elup1"),
    "c_lsd32_defaults": (2, 5, 5, 2, 32, 15, 3, 32, 1.0, "mix", "square", "elup1"),
    "d_full_band": (2, 3, 4, 2, 8, 3, 3, 8, 1.0, "mix", "exp", "exp"),
    "e_one_basis": (2, 3, 4, 2, 8, 1, 2, 8, 1.0, "mix", "relu", "relu"),
    "f_two_points": (3, 3, 1, 1, 8, 4, 2, 8, 1.0, "all", "abs", "abs"),
    "g_one_window": (1, 3, 6, 2, 8, 4, 2, 8, 1.0, "mix", "elup1", "square"),
    "h_no_squaring": (2, 3, 5, 2, 8, 4, 2, 8, 0.05, "mix", "square", "elup1"),
    "i_three_squarings": (2, 3, 5, 2, 8, 4, 2, 8, 7.5, "mix", "square", "elup1"),
    "j_all_valid": (2, 3, 5, 2, 8, 4, 2, 8, 1.0, "all", "square", "elup1"),
    "k_none_valid": (2, 3, 5, 2, 8, 4, 2, 8, 1.0, "none", "square", "elup1"),
    "l_65_windows": (65, 2, 3, 2, 6, 2, 1, 8, 1.0, "mix", "square", "elup1"),
}

# name: (output, worst gradient) of torch's fp32 CPU run against float64
FP32_ERR = {
    "a_lsd2_band_covers_all": (3.7e-7, 6.4e-5),
    "b_lsd8": (2.3e-6, 1.7e-5),
    "c_lsd32_defaults": (4.9e-5, 1.1e-4),
    "d_full_band": (4.8e-7, 7.2e-7),
    "e_one_basis": (4.8e-7, 3.1e-5),
    "f_two_points": (6.2e-7, 1.1e-6),
    "g_one_window": (4.1e-7, 2.0e-6),
    "h_no_squaring": (2.2e-6, 1.1e-5),
    "i_three_squarings": (2.5e-6, 4.0e-5),
    "j_all_valid": (1.9e-6, 2.2e-5),
    "k_none_valid": (3.7e-7, 3.0e-7),
    "l_65_windows": (8.1e-6, 1.5e-5),
}


# outside the kernel (lsd 34: immtsf_cru_supported says no): the composed path's shape, b_lsd8 otherwise
WIDE = CASES["b_lsd8"][:4] + (34,) + CASES["b_lsd8"][5:]
FP32_ERR["wide_lsd34"] = (1.2e-5, 5.0e-5)

# the same for the two goldens of the real reference (tests/golden/model_cru*.npz): name -> (C, L, Lp, lsd, num_basis, bandwidth, hidden, seed)
GOLDENS = {"model_cru": (3, 6, 3, 8, 4, 2, 16, 71), "model_cru_default": (5, 5, 2, 32, 15, 3, 32, 73), "model_cru_rkn": (3, 6, 3, 8, 4, 2, 16, 79)}
FP32_ERR.update({"model_cru": (2.1e-6, 1.9e-5), "model_cru_default": (4.4e-5, 5.0e-4), "model_cru_rkn": (2.9e-7, 2.6e-6)})
# model_cru_rkn: the discrete cell with a time-sensitive coefficient net of one hidden layer -- the composed path's other branches.
# name -> (the module's options, the restatement's)
GOLDEN_OPTIONS = {"model_cru_rkn": (dict(cru_rkn=True, cru_t_sensitive_trans_net=True, cru_trans_net_hidden_units=[6],
                                         cru_trans_net_hidden_activation="Tanh"), dict(rkn=True, t_sensitive=True, hidden_act="Tanh"))}


def bars(name):
    """-> (output bar, gradient bar) of a case: the project's where the recorded fp32 error is 4x inside them, else 4x that error"""
    e_out, e_grad = FP32_ERR[name]
    return (OUT_TOL if e_out <= OUT_TOL / 4 else 4 * e_out), (GRAD_TOL if e_grad <= GRAD_TOL / 4 else 4 * e_grad)


def config(C, L, Lp, lsd, K, bw, hidden, batch_size=4, device="cpu", **over):
    cfg = types.SimpleNamespace(input_len=L, pred_len=Lp, enc_in=C, batch_size=batch_size, device=torch.device(device), cru_lsd=lsd,
                                cru_num_basis=K, cru_bandwidth=bw, cru_hidden_units=hidden)
    cfg.__dict__.update(over)
    return cfg


def make_model(dev, case, seed=0, **over):
    """the product's CRU on `dev`, every parameter 0.1 randn off its init (the bases start at zero), the bases then scaled"""
    from models.CRU import CRU
    B, C, L, Lp, lsd, K, bw, hidden, scale, kind, enc_var, trans_var = case
    torch.manual_seed(1000 + seed)
    m = CRU(config(C, L, Lp, lsd, K, bw, hidden, batch_size=B, device="cpu", cru_enc_var_activation=enc_var, cru_trans_var_activation=trans_var,
                   **over))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
            if name.endswith("_basis"):
                p.mul_(scale)
    m.device = torch.device(dev)
    return m.to(dev).train()


def make_batch(dev, case, seed=7):
    """history times in [0, 1], horizon times in (1, 2].  "mix": masks about 70 % ones; window 0 ends in three zero-padded points (time 0,
    mask 0: one step back in time, then two steps of dt = 0) where L >= 5, and the last window starts with an invalid point.  "all" /
    "none": every / no point observed"""
    B, C, L, Lp, lsd, K, bw, hidden, scale, kind, enc_var, trans_var = case
    g = torch.Generator().manual_seed(seed)
    data = torch.randn(B, L, C, generator=g)
    mask = (torch.rand(B, L, C, generator=g) < 0.7).float()
    tp = torch.sort(torch.rand(B, L, generator=g), 1).values
    tpp = 1.0 + torch.sort(torch.rand(B, Lp, generator=g) * 0.999 + 0.001, 1).values
    up = torch.randn(B, Lp, C, generator=g)
    if kind == "all":
        mask[:] = 1
    elif kind == "none":
        mask[:] = 0
    else:
        mask[:, L // 2, 0] = 1
        if L >= 5:
            mask[0, L - 3:] = 0
            tp[0, L - 3:] = 0
        mask[B - 1, 0] = 0
    return tuple(t.to(dev) for t in (tpp, data * mask, tp, mask, up))


def ref_params(m):
    return {k: v.detach().cpu() for k, v in m.state_dict().items()}


def reference(m, case, batch, dtype=torch.float64, norms=None):
    """-> (out, name -> gradient or None) of the restatement on the module's parameters"""
    tpp, data, tp, mask, up = (t.cpu() for t in batch)
    if norms is not None:
        p = {k: v.double() for k, v in ref_params(m).items()}
        R.forecast(p, tpp, data, tp, mask, case[6], case[10], case[11], norms=norms)
    return R.run(ref_params(m), tpp, data, tp, mask, up, case[6], case[10], case[11], dtype=dtype)


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
