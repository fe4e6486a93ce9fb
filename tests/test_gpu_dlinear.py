"""GPU parity of the fused DLinear path (csrc/dlinear.hip behind models/DLinear.py::forecasting): against the real reference's goldens,
against the float64 restatement (tests/dlinear_ref.py, pinned to those goldens in tests/test_dlinear_ref.py) over the shapes where the
kernels take different routes, its determinism, the fall-backs to the composed path, the knob, and hipGraph capture.
Tolerances: the project's fp32 bars of test_gpu_backbone.py -- 1e-4 outputs / 3e-4 gradients relative to max, the gradient floor at 1e-2
of the largest gradient."""
import copy
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dlinear_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODS = ("Linear_Seasonal", "Linear_Trend", "Linear_Time")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rel(a, b, floor=1e-3):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / max(float(b.abs().max()), floor))


def _l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def _model(dev, S, P, C, k, individual, batch_size, seed=0):
    from models.DLinear import DLinear
    cfg = types.SimpleNamespace(input_len=S, pred_len=P, enc_in=C, c_out=C, batch_size=batch_size, device=str(dev), moving_avg=k)
    m = DLinear(cfg, individual=individual).to(dev).train()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():      # off the constant init: the three maps and the channels differ
            p.add_((0.1 * torch.randn(p.shape, generator=g)).to(dev))
    return m


def _batch(dev, B, C, L, Lp, seed):
    """masks about 70 % ones; column (0, 0) has no observation, column (B-1, C-1) exactly one"""
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


def _stacked(m, grad):
    """the six (G, ...) arrays of the module's parameters (or their gradients) in dlinear_ref's order"""
    out = []
    for leaf in ("weight", "bias"):
        for name in MODS:
            mod = getattr(m, name)
            ps = [getattr(l, leaf) for l in (mod if m.individual else [mod])]
            out.append(torch.stack([p.grad if grad else p.detach() for p in ps]).cpu().numpy())
    return out


def _run(m, batch):
    tpp, data, tp, mask, up = batch
    m.zero_grad(set_to_none=True)
    out = m.forecasting(tpp, data, tp, mask)
    (out * up).sum().backward()
    return out.detach(), _stacked(m, True)


def _check_grads(got, want, tol=3e-4):
    gmax = max(float(np.abs(w).max()) for w in want)
    bad = {}
    for i, (g, w) in enumerate(zip(got, want)):
        e = _rel(g, w, floor=1e-2 * gmax)
        if not e <= tol:
            bad[i] = e
    assert not bad, bad


@pytest.mark.parametrize("name,individual", [("model_dlinear", False), ("model_dlinear_individual", True)])
def test_fused_vs_reference_golden(name, individual):
    """both goldens of the real reference through DLinear(cfg).forecasting on the fused path: output and all six gradient groups"""
    dev = _dev()
    from models.DLinear import DLinear
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = types.SimpleNamespace(input_len=8, pred_len=6, enc_in=3, c_out=3, batch_size=4, device=str(dev), moving_avg=5)
    m = DLinear(cfg, individual=individual).to(dev).train()
    m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p.")}, strict=True)
    n0 = m.fused_calls
    out = m.forecasting(*[torch.from_numpy(z[k]).to(dev) for k in ("tpp", "data", "tp", "mask")])
    assert m.fused_calls == n0 + 1
    assert out.shape == z["out"].shape
    assert _rel(out, z["out"]) < 1e-4
    (out * torch.from_numpy(z["upstream"]).to(dev)).sum().backward()
    gmax = max(float(np.abs(z[k]).max()) for k in z.files if k.startswith("g."))
    bad = {}
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        e = _rel(p.grad, z["g." + k], floor=1e-2 * gmax)
        if not e <= 3e-4:
            bad[k] = e
    assert not bad, bad


CASES = [      # B, C, S, P, L, Lp, k, individual
    (4, 5, 24, 24, 24, 24, 25, False),        # cfg1; the window is wider than the series
    (4, 5, 24, 24, 17, 9, 25, True),          # both paddings; the replicate pad lands on a zero-padded row
    (3, 3, 8, 6, 8, 6, 1, False),             # trend = x, seasonal = 0
    (2, 1, 1, 1, 1, 1, 3, False),             # degenerate
    (5, 7, 33, 31, 20, 31, 7, False),         # nothing a multiple of 4
    (130, 8, 32, 32, 32, 32, 25, False),      # 1040 rows: more than one workgroup's share; the cross-workgroup fold
    (16, 8, 128, 128, 100, 128, 25, True),    # the limit's edge
    (520, 8, 128, 128, 128, 128, 25, False),  # 4160 rows over 256 slabs: a share of 17 rows is two staged chunks (16 + 1)
    (80, 64, 128, 128, 128, 128, 5, True),    # per channel 80 windows over 4 slabs: shares of 20 = chunks of 16 + 4
]


@pytest.mark.parametrize("B,C,S,P,L,Lp,k,individual", CASES)
def test_fused_vs_float64_restatement(B, C, S, P, L, Lp, k, individual):
    dev = _dev()
    m = _model(dev, S, P, C, k, individual, batch_size=B)
    batch = _batch(dev, B, C, L, Lp, seed=7)
    tpp, data, tp, mask, up = batch
    n0 = m.fused_calls
    out, grads = _run(m, batch)
    assert m.fused_calls == n0 + 1
    assert tuple(out.shape) == (B, Lp, C)
    d, mk, t = (x.cpu().numpy() for x in (data, mask, tp))
    want = R.forward(d, mk, t, Lp, k, *_stacked(m, False))
    assert _rel(out, want) < 1e-4
    dWs, dWt, dWu, db = R.backward(d, mk, t, k, S, P, up.cpu().numpy(), individual)
    _check_grads(grads, (dWs, dWt, dWu, db, db, db))


def test_backward_is_bit_reproducible():
    dev = _dev()
    B, C, S, P, L, Lp, k, individual = CASES[5]
    m = _model(dev, S, P, C, k, individual, batch_size=B)
    batch = _batch(dev, B, C, L, Lp, seed=7)
    out1, g1 = _run(m, batch)
    out2, g2 = _run(m, batch)
    assert torch.equal(out1, out2)
    for a, b in zip(g1, g2):
        assert np.array_equal(a, b)


def test_even_window_raises_the_composed_paths_error():
    dev = _dev()
    from immtsf import config
    m = _model(dev, 24, 24, 5, 4, False, batch_size=4)
    tpp, data, tp, mask, _ = _batch(dev, 4, 5, 24, 24, seed=3)
    kinds = []
    try:
        for knob in (True, False):
            config.dlinear_fused = knob
            with pytest.raises(Exception) as ei:
                m.forecasting(tpp, data, tp, mask)
            kinds.append(type(ei.value))
    finally:
        config.dlinear_fused = True
    assert kinds[0] is kinds[1]
    assert m.fused_calls == 0


def test_beyond_the_limit_runs_the_composed_path():
    """the first input_len immtsf_dlinear_supported refuses: the counter stands and the forecast is the knob-off run's, bit for bit.
    The composed path's gradients are not reproducible to the bit from one run to the next, knob or no knob (immtsf_linear_backward
    adds partial sums by fp32 atomics: with the knob off both times the three bias gradients moved by 2e-7 .. 1e-6 absolute, values of
    about 10, over four runs of this very case), so the gradients are held to the fp32 gradient bar instead of to equality."""
    dev = _dev()
    from immtsf import _lib, config
    lib = _lib.load()
    S = 129
    while lib.immtsf_dlinear_supported(S, 24, 5, 25, 0):
        S += 1
    assert lib.immtsf_dlinear_supported(S - 1, 24, 5, 25, 0)
    m = _model(dev, S, 24, 5, 25, False, batch_size=4)
    batch = _batch(dev, 4, 5, S - 3, 20, seed=5)
    out_on, g_on = _run(m, batch)
    try:
        config.dlinear_fused = False
        out_off, g_off = _run(m, batch)
    finally:
        config.dlinear_fused = True
    assert m.fused_calls == 0
    assert torch.equal(out_on, out_off)
    _check_grads(g_on, g_off)


def test_data_gradient_runs_the_composed_path():
    dev = _dev()
    m = _model(dev, 24, 24, 5, 25, False, batch_size=4)
    tpp, data, tp, mask, up = _batch(dev, 4, 5, 24, 24, seed=3)
    data = data.clone().requires_grad_(True)
    out = m.forecasting(tpp, data, tp, mask)
    (out * up).sum().backward()
    assert m.fused_calls == 0
    assert data.grad is not None and float(data.grad.abs().max()) > 0
    assert all(p.grad is not None for p in m.parameters())


def test_more_windows_than_the_padding_buffer_raises():
    dev = _dev()
    m = _model(dev, 24, 24, 5, 25, False, batch_size=4)
    tpp, data, tp, mask, _ = _batch(dev, 6, 5, 17, 24, seed=3)
    with pytest.raises(RuntimeError):
        m.forecasting(tpp, data, tp, mask)
    assert m.fused_calls == 0
    tpp, data, tp, mask, _ = _batch(dev, 6, 5, 24, 24, seed=3)      # a full history needs no padding: the reference takes it
    assert m.forecasting(tpp, data, tp, mask).shape == (6, 24, 5)
    assert m.fused_calls == 1


def test_knob_fused_vs_composed():
    dev = _dev()
    from immtsf import config
    B, C, S, P, L, Lp, k, individual = CASES[0]
    m = _model(dev, S, P, C, k, individual, batch_size=B)
    batch = _batch(dev, B, C, L, Lp, seed=7)
    res = {}
    try:
        for prec in ("fp32", "bf16"):
            config.precision = prec
            config.dlinear_fused = True
            n0 = m.fused_calls
            res[prec, "fused"] = _run(m, batch)
            assert m.fused_calls == n0 + 1
            config.dlinear_fused = False
            res[prec, "composed"] = _run(m, batch)
            assert m.fused_calls == n0 + 1
    finally:
        config.dlinear_fused = True
        config.precision = "fp32"
    out_f, g_f = res["fp32", "fused"]
    out_c, g_c = res["fp32", "composed"]
    assert _rel(out_f, out_c) < 1e-5
    _check_grads(g_f, g_c)      # both single precision; the sums over the rows round differently
    # the fused path is fp32 in bf16 mode too: it gives the fp32 run's bits, inside the bf16 band of the composed path
    out_b, g_b = res["bf16", "fused"]
    assert torch.equal(out_b, out_f)
    out_cb, g_cb = res["bf16", "composed"]
    assert _l2(out_b, out_cb) < 3e-2
    for i, (a, b) in enumerate(zip(g_b, g_cb)):
        assert _l2(torch.from_numpy(a), torch.from_numpy(b)) < 4e-2, i


def test_forward_backward_under_graph_capture():
    """forward + backward captured once, replayed on a second batch: the numbers of an eager run on that batch, bit for bit"""
    dev = _dev()
    B, C, S, P, L, Lp, k, individual = CASES[0]
    m = _model(dev, S, P, C, k, individual, batch_size=B)
    first, second = _batch(dev, B, C, L, Lp, seed=7), _batch(dev, B, C, L, Lp, seed=8)
    want_out, want_g = _run(copy.deepcopy(m), second)
    static = tuple(t.clone() for t in first)
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
    for s, t in zip(static, second):
        s.copy_(t)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), want_out)
    for a, b in zip(_stacked(m, True), want_g):
        assert np.array_equal(a, b)


def test_evalstep_captures_a_dlinear_forward():
    dev = _dev()
    import immtsf
    B, C, S, P, L, Lp, k, individual = CASES[0]
    m = _model(dev, S, P, C, k, individual, batch_size=B).eval()
    batches = []
    for seed in (11, 12):
        tpp, data, tp, mask, truth = _batch(dev, B, C, L, Lp, seed=seed)
        batches.append({"tp_to_predict": tpp, "observed_data": data, "observed_tp": tp, "observed_mask": mask, "data_to_predict": truth,
                        "mask_predicted_data": (truth > -0.5).float()})
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
    assert (nog.eager, nog.replays) == (2, 0)
    ref = nog.result()
    for key in ref:
        assert got[key] == pytest.approx(ref[key], rel=1e-12), key
