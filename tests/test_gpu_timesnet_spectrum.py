"""immtsf.ops.timesnet_spectrum (csrc/timesnet_spectrum.hip: TimesBlock's period selection as a direct DFT, two launches forward and one
backward) against the float64 restatement tests/timesnet_spectrum_ref.py (pinned on the CPU by tests/test_timesnet_spectrum_ref.py, which
also shows that fp32 round-off cannot change a selection of the case table: a selection mismatch here is a bug).

Bars.  Forward quantities (amp_mean, freq, weight: error relative to the largest mean amplitude of the case; w: relative to the largest w)
and the gradient dx (relative to the largest |dx|) are judged against the EXISTING route measured in the same test on the same input
-- models/TimesNet.py fft_for_period_device + softmax + the padded transpose in fp32 on the GPU, and autograd through it -- against the same
float64 values: the fused error may be at most 4 x that (a direct sum carries T terms where the FFT carries log2 T stages; expected ratio
about sqrt(T / log2 T) = 4 - 5 at T <= 192), with a floor of T 2^-23, the first-order worst case of a T-term fp32 sum.  top / period /
rows / xl, the pass-through of g_xl, the exact tie and the zero series are exact.  The block is judged knob on against knob off on the bars
tests/test_gpu_timesnet_periods.py uses for a TimesBlock (fp32: 1e-4 outputs / 3e-4 gradients relative to the tensor's maximum; bf16:
relative L2 3e-2 / 4e-2; a kernel gradient against the largest gradient of the block, floor 1e-2 gmax).

Every test prints its figures ("MEASURED | case | quantity | fused | torch route | bar") before it asserts.

Measured on an MI355X, fused / torch route (DESIGN 4e has the table): amp_mean 3.2e-8 .. 1.4e-7 / 2.8e-8 .. 8.7e-8, freq 3.2e-8 .. 1.3e-7 /
1.9e-8 .. 9.7e-8, w 0 .. 2.0e-7 / 0 .. 9.3e-8, dx 0 .. 4.1e-8 / 0 .. 4.5e-8, against floors of 8.3e-7 (T 7) .. 2.3e-5 (T 192); the block
knob on against off: at most 2.6e-7 in fp32 and 8.9e-8 in bf16 mode (the two routes feed the same convolutions); the captured
forecasting() + backward graph at cfg4's dimensions holds 273 kernel nodes against 321.
"""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import timesnet_periods_ref as P  # noqa: E402
import timesnet_spectrum_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
CASE_NAMES = sorted(S.CASES)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _err(got, ref, scale=None):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = float(ref.abs().max()) if scale is None else scale
    return float((got - ref).abs().max() / max(scale, 1e-300))


def _judge(case, T, errs):
    """errs: quantity -> (fused error, torch-route error)"""
    bad = {}
    for q, (e, e_t) in errs.items():
        bar = max(4.0 * e_t, T * 2.0 ** -23)
        print(f"MEASURED | {case} | {q} | {e:.3g} | {e_t:.3g} | {bar:.3g}")
        if not e <= bar:       # (a NaN is bad)
            bad[q] = (e, e_t, bar)
    assert not bad, (case, bad)


def _torch_route(x, k):
    """the existing route, fp32 on the GPU: (amp_mean, freq, top, weight, w, xl)"""
    from models.TimesNet import fft_for_period_device
    B, T, N = x.shape
    amp = torch.fft.rfft(x, dim=1).abs()
    freq = amp.mean(0).mean(-1)
    freq = torch.cat([freq.new_zeros(1), freq[1:]])
    top, weight = fft_for_period_device(x, k)
    xl = F.pad(x.transpose(0, 1), (0, 0, 0, 0, 0, T)).reshape(2 * T * B, N)
    return amp.mean(-1), freq, top, weight, F.softmax(weight, dim=1), xl


def _block_cfg(T, N, k, d_ff=8, num_kernels=1):
    return types.SimpleNamespace(input_len=T // 2, pred_len=T - T // 2, d_model=N, d_ff=d_ff, num_kernels=num_kernels, top_k=k)


class _Knob:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from immtsf import config
        self.was = config.timesnet_spectrum_fused
        config.timesnet_spectrum_fused = self.on

    def __exit__(self, *a):
        from immtsf import config
        config.timesnet_spectrum_fused = self.was


# ---------------------------------------------------------------------------------------------------------------- route
@pytest.mark.parametrize("name", CASE_NAMES + [S.PAST[0]])
def test_route(name):
    dev = _dev()
    from immtsf import ops
    from models.TimesNet import TimesBlock
    B, T, N, k = (S.PAST[1] if name == S.PAST[0] else S.CASES[name])[:4]
    takes = name != S.PAST[0]
    assert ops.timesnet_spectrum_ok(T, N, k) is takes
    torch.manual_seed(5)
    blk = TimesBlock(_block_cfg(T, N, k)).to(dev)
    x = S.case_input(name).to(dev)
    assert blk.spectrum_calls == 0
    with _Knob(True):
        out = blk(x)
    assert blk.spectrum_calls == (1 if takes else 0)
    with _Knob(False):
        off = blk(x)
    assert blk.spectrum_calls == (1 if takes else 0)
    torch.cuda.synchronize()
    assert out.shape == (B, T, N) and bool(torch.isfinite(out).all())
    assert _err(out, off) <= 1e-4          # (the fp32 bar of a TimesBlock's output)
    if not takes:
        with pytest.raises(Exception):
            ops.timesnet_spectrum(x, k)


# ---------------------------------------------------------------------------------------------------------------- forward, selection
@functools.lru_cache(maxsize=None)
def _forward(name):
    """the operator and the torch route on the case's input, once: everything on the CPU"""
    from immtsf import ops
    dev = torch.device("cuda:0")
    k = S.CASES[name][3]
    x = S.case_input(name).to(dev)
    amp_mean, freq, weight = ops.timesnet_spectrum_stats(x, k)
    top, period, rows, w, xl = ops.timesnet_spectrum(x, k)
    route = _torch_route(x, k)
    torch.cuda.synchronize()
    cpu = lambda ts: tuple(t.cpu() for t in ts)      # noqa: E731
    return cpu((amp_mean, freq, weight, top, period, rows, w, xl)), cpu(route)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_forward_vs_float64(name):
    _dev()
    B, T, N, k = S.CASES[name][:4]
    r = S.case_reference(name)
    (amp_mean, freq, weight, top, period, rows, w, xl), (t_amp_mean, t_freq, t_top, t_weight, t_w, t_xl) = _forward(name)
    assert amp_mean.shape == (B, T // 2 + 1) and freq.shape == (T // 2 + 1,) and weight.shape == (B, k) and w.shape == (B, k)
    for t in (amp_mean, freq, weight, w):
        assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
    scale = float(r["amp_mean"].max())
    assert float(freq[0]) == 0.0
    _judge(f"spectrum {name}", T, {
        "amp_mean": (_err(amp_mean, r["amp_mean"], scale), _err(t_amp_mean, r["amp_mean"], scale)),
        "freq": (_err(freq, r["freq"], scale), _err(t_freq, r["freq"], scale)),
        "weight": (_err(weight, r["weight"], scale), _err(t_weight, r["weight"], scale)),
        "w": (_err(w, r["w"]), _err(t_w, r["w"])),
    })


@pytest.mark.parametrize("name", CASE_NAMES)
def test_selection_is_exact(name):
    _dev()
    B, T, N, k = S.CASES[name][:4]
    r = S.case_reference(name)
    (amp_mean, freq, weight, top, period, rows, w, xl), route = _forward(name)
    assert top.dtype == torch.int64 and period.dtype == torch.int32 and rows.dtype == torch.int32
    assert top.tolist() == r["top"], (top.tolist(), r["top"])
    want_p, want_r = P.period_rows_ref(r["top"], T, B)
    assert np.array_equal(period.numpy(), want_p) and np.array_equal(rows.numpy(), want_r)
    x = S.case_input(name)
    assert xl.shape == (2 * T * B, N)
    assert torch.equal(xl, F.pad(x.transpose(0, 1), (0, 0, 0, 0, 0, T)).reshape(2 * T * B, N))
    assert torch.equal(xl, route[5])


# ---------------------------------------------------------------------------------------------------------------- backward
def _grads(name, scaled):
    B, T, N, k, freqs, amps, seed = S.CASES[name]
    x = (S.case_input(name).double() * (4.0 / T)).float() if scaled else S.case_input(name)
    g = torch.Generator().manual_seed(seed + 200)
    return x, torch.randn(B, k, generator=g), torch.randn(2 * T * B, N, generator=g)


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_backward_vs_float64(name, scaled):
    """scaled: the case's input times 4 / T -- the same lines and the same selection with amplitudes of order one, where the softmax is not
    saturated and the gradient through w is a visible part of dx"""
    dev = _dev()
    from immtsf import ops
    B, T, N, k = S.CASES[name][:4]
    x0, g_w, g_xl = _grads(name, scaled)
    want = S.spectrum_grad_ref(x0, k, g_w, g_xl)
    x = x0.to(dev).requires_grad_(True)
    top, period, rows, w, xl = ops.timesnet_spectrum(x, k)
    assert not top.requires_grad and not period.requires_grad and not rows.requires_grad and w.requires_grad and xl.requires_grad
    ((w * g_w.to(dev)).sum() + (xl * g_xl.to(dev)).sum()).backward()
    xt = x0.to(dev).requires_grad_(True)
    _, _, t_top, _, t_w, t_xl = _torch_route(xt, k)
    ((t_w * g_w.to(dev)).sum() + (t_xl * g_xl.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    assert top.tolist() == S.spectrum_ref(x0, k)["top"] == t_top.tolist()
    assert bool(torch.isfinite(x.grad).all())
    _judge(f"spectrum {name}{' scaled' if scaled else ''}", T, {"dx": (_err(x.grad, want), _err(xt.grad, want))})


@pytest.mark.parametrize("name", CASE_NAMES)
def test_image_gradient_alone_comes_back_transposed(name):
    dev = _dev()
    from immtsf import ops
    B, T, N, k = S.CASES[name][:4]
    x0, _, g_xl = _grads(name, False)
    x = x0.to(dev).requires_grad_(True)
    xl = ops.timesnet_spectrum(x, k)[4]
    xl.backward(gradient=g_xl.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(x.grad.cpu(), g_xl.reshape(2 * T, B, N)[:T].transpose(0, 1))


# ---------------------------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("B,N,k", [(2, 3, 4), (1, 8, 8)])
def test_exact_tie_goes_to_the_lower_index(B, N, k):
    """the unit impulse at t = 0 in every channel, T = 16: Re = 1 and Im = 0 with no rounding, so every amplitude is exactly 1"""
    dev = _dev()
    from immtsf import ops
    T = 16
    x = torch.zeros(B, T, N, device=dev)
    x[:, 0] = 1.0
    amp_mean, freq, weight = ops.timesnet_spectrum_stats(x, k)
    top, period, rows, w, xl = ops.timesnet_spectrum(x, k)
    torch.cuda.synchronize()
    assert bool((amp_mean == 1.0).all()) and freq.tolist() == [0.0] + [1.0] * (T // 2)
    assert top.tolist() == list(range(1, k + 1))
    assert bool((weight == 1.0).all())
    assert bool((w == torch.tensor(1.0 / k, dtype=torch.float32)).all()), w.tolist()
    want_p, want_r = P.period_rows_ref(top.tolist(), T, B)
    assert np.array_equal(period.cpu().numpy(), want_p) and np.array_equal(rows.cpu().numpy(), want_r)


def test_zero_series():
    """x = 0: every output finite, w = 1 / k, dx exactly g_xl transposed -- the spectral term is 0 where the amplitude is 0, no NaN"""
    dev = _dev()
    from immtsf import ops
    B, T, N, k = 3, 16, 5, 3
    g = torch.Generator().manual_seed(7)
    g_w, g_xl = torch.randn(B, k, generator=g), torch.randn(2 * T * B, N, generator=g)
    x = torch.zeros(B, T, N, device=dev, requires_grad=True)
    amp_mean, freq, weight = ops.timesnet_spectrum_stats(x, k)
    top, period, rows, w, xl = ops.timesnet_spectrum(x, k)
    ((w * g_w.to(dev)).sum() + (xl * g_xl.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    assert not amp_mean.any() and not freq.any() and not weight.any() and not xl.any()
    assert top.tolist() == [0, 1, 2]                       # (all equal: the lower index; f = 0 -> period = T, the documented guard)
    want_p, want_r = P.period_rows_ref(top.tolist(), T, B)
    assert np.array_equal(period.cpu().numpy(), want_p) and np.array_equal(rows.cpu().numpy(), want_r)
    assert bool((w == torch.tensor(1.0 / k, dtype=torch.float32)).all()), w.tolist()
    assert torch.equal(x.grad.cpu(), g_xl.reshape(2 * T, B, N)[:T].transpose(0, 1))


@pytest.mark.parametrize("name", ["a", "odd", "wide"])
def test_two_calls_give_the_same_bits(name):
    dev = _dev()
    from immtsf import ops
    B, T, N, k = S.CASES[name][:4]
    x0, g_w, g_xl = _grads(name, True)
    runs = []
    for _ in range(2):
        x = x0.to(dev).requires_grad_(True)
        stats = ops.timesnet_spectrum_stats(x, k)
        outs = ops.timesnet_spectrum(x, k)
        ((outs[3] * g_w.to(dev)).sum() + (outs[4] * g_xl.to(dev)).sum()).backward()
        torch.cuda.synchronize()
        runs.append([t.detach().cpu() for t in (*stats, *outs, x.grad)])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ---------------------------------------------------------------------------------------------------------------- block level
BLOCKS = {      # precision, input_len, pred_len, d_model, d_ff, num_kernels (tests/test_gpu_timesnet_periods.py BLOCKS "a" and "c")
    "a": ("fp32", 18, 12, 8, 16, 3),
    "c": ("bf16", 40, 26, 8, 16, 2),
}


def _rel(a, b, floor=1e-3):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), floor))


def _l2err(a, b, floor=1e-3):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), floor * max(1.0, b.numel() ** 0.5)))


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_timesblock_knob_on_vs_off(name):
    dev = _dev()
    from immtsf import config
    from models.TimesNet import TimesBlock
    precision, input_len, pred_len, d_model, d_ff, nk = BLOCKS[name]
    B, total, N, freqs, amps, seed = P.BLOCK_BATCHES[name]
    cfg = types.SimpleNamespace(input_len=input_len, pred_len=pred_len, d_model=d_model, d_ff=d_ff, num_kernels=nk, top_k=len(freqs))
    torch.manual_seed(21)
    blocks = {True: TimesBlock(cfg).to(dev)}
    with torch.no_grad():
        for c in blocks[True].modules():
            if isinstance(c, torch.nn.Conv2d):
                c.bias.uniform_(-0.2, 0.2)
    blocks[False] = TimesBlock(cfg).to(dev)
    blocks[False].load_state_dict(blocks[True].state_dict())
    x0 = P.spectral_batch(B, total, N, freqs, amps, seed)
    up = torch.randn(B, total, N, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
    res = {}
    config.precision = precision
    try:
        for on, blk in blocks.items():
            with _Knob(on):
                x = x0.to(dev).requires_grad_(True)
                out = blk(x)
                (out * up).sum().backward()
                torch.cuda.synchronize()
                res[on] = (out.detach(), x.grad, {k: p.grad for k, p in blk.named_parameters()})
    finally:
        config.precision = "fp32"
    assert blocks[True].spectrum_calls == 1 and blocks[False].spectrum_calls == 0
    err, tol_o, tol_g = (_rel, 1e-4, 3e-4) if precision == "fp32" else (_l2err, 3e-2, 4e-2)
    gmax = max(float(g.abs().max()) for g in res[False][2].values())
    errs = {"out": (err(res[True][0], res[False][0]), tol_o), "dx": (err(res[True][1], res[False][1]), tol_g)}
    for key, g in res[False][2].items():
        assert g is not None and res[True][2][key] is not None, key
        errs[key] = (err(res[True][2][key], g, floor=1e-2 * gmax), tol_g)
    assert len(errs) == 2 + 4 * nk
    for q, (e, bar) in errs.items():
        print(f"MEASURED | block ({name}) on vs off | {q} | {e:.3g} | - | {bar:.3g}")
    bad = {q: v for q, v in errs.items() if not v[0] <= v[1]}
    assert not bad, bad


def test_forecasting_replays_from_a_graph_with_fewer_kernels():
    """tools/timesnet_bench.py's step (TimesNet.forecasting() + backward at cfg4's dimensions, 4 windows) captured into a torch.cuda.graph
    with the knob on: the replay reproduces the eager step, and the tool counts strictly fewer kernels in it than in the knob-off graph"""
    _dev()
    import timesnet_bench as TB
    models, step = TB.make("cfg4", B=4)
    m = models["fused"]
    m.zero_grad(set_to_none=True)
    out_e = step("fused").detach().clone()
    torch.cuda.synchronize()
    grads_e = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    graph, out = TB.capture(models, step, "fused")
    assert TB.spectrum_calls(m) > 0
    out.zero_()
    for p in m.parameters():
        if p.grad is not None:
            p.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and _rel(out, out_e) <= 1e-4
    gmax = max(float(g.abs().max()) for g in grads_e.values())
    bad = {k: _rel(p.grad, grads_e[k], floor=1e-2 * gmax) for k, p in m.named_parameters() if k in grads_e}
    bad = {k: v for k, v in bad.items() if not v <= 3e-4}
    assert not bad, bad
    graph_off, _ = TB.capture(models, step, "torch")
    assert TB.spectrum_calls(models["torch"]) == 0
    n_on, n_off = TB.count_kernels(graph), TB.count_kernels(graph_off)
    print(f"MEASURED | graph kernels, cfg4 dimensions | fused {n_on} | torch route {n_off}")
    assert 0 < n_on < n_off, (n_on, n_off)
