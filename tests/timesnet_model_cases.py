"""Shapes, seeded inputs and float64 references (computed once, never changed) shared by tests/test_timesnet_model_ref.py (CPU) and
tests/test_gpu_timesnet_model.py (GPU): the two stages of models/TimesNet.py around its TimesBlock loop (tests/timesnet_model_ref.py).
The bars are the project's fp32 bars as tests/test_gpu_informer_model.py uses them (informer_cases.py): 1e-4 on outputs and 3e-4 on
gradients, relative to the tensor's largest magnitude (gradients: floored at 1e-2 of the largest gradient of the case)."""
import os
import types

import numpy as np
import torch

import informer_cases as IC
import timesnet_model_ref as MR

OUT_TOL, GRAD_TOL = IC.OUT_TOL, IC.GRAD_TOL
rel, grad_errors = IC.rel, IC.grad_errors
GOLDEN = IC.GOLDEN

#        name: (B, L, input_len, Lp, pred_len, C, d_model)
CASES = {
    "ragged": (3, 5, 8, 3, 4, 3, 8),             # history and horizon both padded
    "full": (2, 8, 8, 4, 4, 3, 8),               # nothing padded
    "degenerate": (1, 1, 1, 1, 1, 1, 4),         # the circular convolution over one row: all three taps are that row
    "odd": (2, 5, 7, 2, 3, 2, 20),               # T = 10 is no multiple of 4; d_model 20: two column tiles, the second 4 wide
    "cfg4": (4, 32, 32, 32, 32, 8, 16),          # cfg4's tile
    "flat": (3, 8, 8, 3, 4, 3, 8),               # a constant channel (variance 0) and a window whose mask is all zero
    "slices": (70, 3, 4, 2, 2, 1, 4),            # more windows than backward slices: a workgroup adds a second window onto its partial
    "long": (1, 70, 70, 3, 5, 1, 4),             # input_len > 64 and T = 75 > 64: every strided loop of the kernels takes a second round
}
_cache = {}


def inputs(name):
    """-> dict of fp32 CPU tensors: the batch, the front end's parameters and upstream, the tail's input, parameters and upstream"""
    B, L, S, Lp, P, C, D = CASES[name]
    T = S + P
    g = torch.Generator().manual_seed(9100 + sorted(CASES).index(name))
    mask = (torch.rand(B, L, C, generator=g) < 0.7).float()
    data = (torch.randn(B, L, C, generator=g) * 2 + 1) * mask
    if name == "flat":
        data[0, :, 1] = 2.5                      # L == input_len: the channel is constant over all rows, stdev = sqrt(1e-5)
        mask[0, :, 1] = 1
        mask[1] = 0
    t = dict(data=data, mask=mask, tp=torch.sort(torch.rand(B, L, generator=g), 1).values,
             tpp=torch.sort(torch.rand(B, Lp, generator=g), 1).values,
             W_token=torch.randn(D, 2 * C + 1, 3, generator=g) * 0.3, pe=torch.randn(S + 3, D, generator=g),
             W_predict=torch.randn(T, T, generator=g) / T ** 0.5, b_predict=0.3 * torch.randn(T, generator=g),
             up_enc=torch.randn(B, T, D, generator=g),
             x=torch.randn(B, T, D, generator=g) * 1.5 + 0.3, gamma=1 + 0.2 * torch.randn(D, generator=g), beta=0.2 * torch.randn(D, generator=g),
             W=torch.randn(C, D, generator=g) / D ** 0.5, b=0.3 * torch.randn(C, generator=g), means=torch.randn(B, 1, C, generator=g),
             stdev=0.2 + torch.rand(B, 1, C, generator=g), up_y=torch.randn(B, Lp, C, generator=g))
    return t


def front_reference(name, scale=None):
    """the float64 front end of the case -> dict(want=outputs, grads=parameter gradients); cached when there is no dropout"""
    if scale is None and ("front", name) in _cache:
        return _cache["front", name]
    B, L, S, Lp, P, C, D = CASES[name]
    t = {k: v.double() for k, v in inputs(name).items()}
    sc = None if scale is None else scale.double()
    enc, means, stdev, E, inp = MR.front(t["data"], t["mask"], t["tp"], t["tpp"], S, P, t["W_token"], t["pe"], t["W_predict"], t["b_predict"], sc)
    r = dict(want=dict(enc=enc, means=means, stdev=stdev), grads=MR.front_grads(t["up_enc"], E, inp, t["W_predict"], S, sc))
    if scale is None:
        _cache["front", name] = r
    return r


def tail_reference(name):
    if ("tail", name) in _cache:
        return _cache["tail", name]
    B, L, S, Lp, P, C, D = CASES[name]
    t = {k: v.double() for k, v in inputs(name).items()}
    y = MR.tail(t["x"], t["gamma"], t["beta"], t["W"], t["b"], t["means"], t["stdev"], S, Lp)
    r = dict(out=y, grads=MR.tail_grads(t["up_y"], t["x"], t["gamma"], t["beta"], t["W"], t["stdev"], S, Lp))
    _cache["tail", name] = r
    return r


# ---- the whole model: the committed golden of the unmodified reference (tests/golden/make_golden.py gen_models)
GOLDEN_CFG = dict(input_len=8, pred_len=6, d_model=8, d_ff=16, n_heads=2, e_layers=1, dropout=0.0, factor=5, activation="gelu", enc_in=3,
                  c_out=3, batch_size=4, moving_avg=5, top_k=2, num_kernels=2, embed="fixed", freq="h")


def golden():
    z = np.load(os.path.join(GOLDEN, "model_timesnet.npz"))
    return z, {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p.")}


def config(device="cpu", **over):
    return types.SimpleNamespace(**dict(GOLDEN_CFG, device=str(device), **over))
