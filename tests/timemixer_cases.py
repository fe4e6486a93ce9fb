"""Shapes, models and batches shared by tests/test_timemixer_ref.py (CPU: the margin check) and tests/test_gpu_timemixer.py (GPU parity):
the smallest shapes that reach each branch of csrc/timemixer.hip.  A model's parameters are drawn on the CPU from a fixed seed, so both
files see the same numbers."""
import types

import torch

import timemixer_ref as R

OUT_TOL, GRAD_TOL, GRAD_FLOOR = 1e-4, 3e-4, 1e-2      # the project's fp32 bars (test_gpu_dlinear.py)

# name: B, C, input_len, pred_len, L, Lp, d_model, d_ff, e_layers, moving_avg
CASES = {
    "a_one_halving": (3, 3, 3, 4, 3, 4, 8, 12, 2, 5),
    "b_6_3_1": (3, 3, 6, 4, 6, 4, 8, 12, 2, 5),
    "c_coarsest_of_one": (3, 3, 8, 6, 8, 6, 8, 12, 2, 5),
    "d_dropped_tail": (3, 3, 33, 7, 33, 7, 16, 32, 2, 25),
    "e_i_defaults_no_padding": (4, 5, 24, 24, 24, 24, 16, 32, 2, 25),
    "f_window_of_one": (3, 3, 8, 6, 8, 6, 8, 12, 2, 1),
    "g_one_block": (3, 3, 8, 6, 8, 6, 8, 12, 1, 5),
    "h_three_blocks": (3, 3, 12, 6, 12, 6, 8, 12, 3, 5),
    "j_padding": (4, 5, 24, 24, 17, 9, 16, 32, 2, 25),
    "k_one_channel": (3, 1, 8, 6, 8, 6, 8, 12, 2, 5),
    "k_eight_channels": (3, 8, 8, 6, 8, 6, 8, 12, 2, 5),
    "l_one_window": (1, 3, 8, 6, 6, 4, 8, 12, 2, 5),
    "m_300_windows": (300, 3, 8, 6, 6, 4, 8, 12, 2, 5),
    "m_301_windows": (301, 3, 8, 6, 6, 4, 8, 12, 2, 5),       # 151 shares of two windows, the last share holds one
    "n_limit_corner": (2, 3, 64, 64, 64, 64, 32, 64, 2, 25),
}


def config(C, S, P, d, dff, E, k, batch_size, device="cpu", dropout=0.0, **over):
    cfg = types.SimpleNamespace(input_len=S, pred_len=P, enc_in=C, c_out=C, batch_size=batch_size, device=device, d_model=d, d_ff=dff,
                                e_layers=E, moving_avg=k, dropout=dropout, embed="timeF", freq="h", top_k=5, decomp_method="moving_avg",
                                channel_independence=1, down_sampling_layers=3, down_sampling_method="avg", down_sampling_window=2)
    cfg.__dict__.update(over)
    return cfg


def make_model(dev, case, seed=0, dropout=0.0, **over):
    """the product's TimeMixer on `dev`, every parameter 0.1 randn off its init (no two maps coincide, biases are not zero)"""
    from models.TimeMixer import TimeMixer
    B, C, S, P, L, Lp, d, dff, E, k = case
    torch.manual_seed(1000 + seed)
    m = TimeMixer(config(C, S, P, d, dff, E, k, batch_size=B, device=str(dev), dropout=dropout, **over))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    return m.to(dev).train()


def make_batch(dev, case, seed=7):
    """masks about 70 % ones; column (0, 0) has no observation at all, column (B-1, C-1) exactly one"""
    B, C, S, P, L, Lp, d, dff, E, k = case
    g = torch.Generator().manual_seed(seed)
    data = torch.randn(B, L, C, generator=g)
    mask = (torch.rand(B, L, C, generator=g) < 0.7).float()
    mask[0, :, 0] = 0
    mask[B - 1, :, C - 1] = 0
    mask[B - 1, L // 2, C - 1] = 1
    tp = torch.sort(torch.rand(B, L, generator=g), 1).values
    tpp = torch.sort(torch.rand(B, Lp, generator=g), 1).values
    up = torch.randn(B, Lp, C, generator=g)
    return tuple(t.to(dev) for t in (tpp, data, tp, mask, up))


def ref_params(m, S):
    """the module's state as the restatement takes it (the sinusoid table cut to the rows forecasting() reads)"""
    return {k: (v[:, :S] if k.endswith(".pe") else v).detach().cpu() for k, v in m.state_dict().items()}


def reference(m, case, batch, keep=None, dtype=torch.float64):
    B, C, S, P, L, Lp, d, dff, E, k = case
    tpp, data, tp, mask, up = (t.cpu() for t in batch)
    return R.run(ref_params(m, S), data, mask, tp, up, S, P, E, k, keep=keep, dtype=dtype)


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
