"""Fixtures' options, error measures and seeded tensors shared by tests/test_ttm_ref.py (CPU) and tests/test_gpu_ttm.py (GPU)."""
import os
import types

import numpy as np
import torch

OUT_TOL, GRAD_TOL, GRAD_FLOOR = 1e-4, 3e-4, 1e-2      # the project's fp32 bars (test_gpu_timemixer.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

FIXTURES = {
    "model_ttm": dict(enc_in=3, input_len=8, pred_len=6, patch_size=2, stride=2, d_model=16, AP_levels=2, e_layers=2, d_layers=2, d_d_model=8,
                      mode="mix_channel", use_decoder=True, use_norm=1),
    "model_ttm_odd": dict(enc_in=2, input_len=33, pred_len=7, patch_size=6, stride=24, d_model=24, AP_levels=3, e_layers=1, d_layers=1,
                          d_d_model=10, mode="mix_channel", use_decoder=True, use_norm=1),
    "model_ttm_plain": dict(enc_in=3, input_len=8, pred_len=6, patch_size=2, stride=8, d_model=16, AP_levels=0, e_layers=2, d_layers=2,
                            d_d_model=8, mode="common_channel", use_decoder=False, use_norm=0),
}
PATCHES = {"model_ttm": 4, "model_ttm_odd": 2, "model_ttm_plain": 1}


def config(opts, batch_size=4, device="cpu", dropout=0.0, **over):
    cfg = types.SimpleNamespace(batch_size=batch_size, device=device, dropout=dropout, **opts)
    cfg.__dict__.update(over)
    return cfg


def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    params = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p.")}
    none = {s for s in str(z["none"]).split("\n") if s}
    return z, params, none


def golden_model(name, dev, **over):
    """the product's TTM with the fixture's state, in train mode on `dev`; -> (module, (tpp, data, tp, mask, upstream), golden)"""
    from models.TTM import TTM
    z, params, none = golden(name)
    m = TTM(config(FIXTURES[name], device=str(dev), **over))
    m.load_state_dict(params, strict=True)
    m = m.to(dev).train()
    batch = tuple(torch.from_numpy(z[k]).to(dev) for k in ("tpp", "data", "tp", "mask", "upstream"))
    return m, batch, (z, params, none)


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


def block_tensors(B, M, N, D, mode, seed=0):
    """x, upstream (B, M, N, D) and a block's eight parameters (ttm_ref.BLOCK_KEYS order) for the mixed axis of `mode`, on the CPU"""
    g = torch.Generator().manual_seed(seed)
    Fm = N if mode == "patch" else M
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    x, up = r(B, M, N, D) * 1.5 + 0.3, r(B, M, N, D)
    params = [1 + 0.2 * r(D), 0.2 * r(D), r(2 * Fm, Fm) / Fm ** 0.5, 0.2 * r(2 * Fm), r(Fm, 2 * Fm) / (2 * Fm) ** 0.5, 0.2 * r(Fm),
              r(Fm, Fm) / Fm ** 0.5, 0.2 * r(Fm)]
    return x, up, params
