"""TimesNet's period-on-the-device kernels (csrc/conv.hip: period_rows, conv2d_period(s)_forward/backward, period_aggregate) against the
float64 restatement tests/timesnet_periods_ref.py (pinned on the CPU by tests/test_timesnet_periods_ref.py): the fp32 form (k single-image
calls, im2col with 8 channels or 1 per item, device row count / reduction length in the GEMMs), the batched bf16 im2col form (the images
along grid.y / grid.z, the kernel gradient summed by atomics), the aggregation kernels, and a whole TimesBlock in each of its three forms
against TimesBlock(cfg).double() on the CPU.

The contract the design rests on -- "rows beyond `rows` are neither read nor written" (csrc/conv.hip, the comment above period_rows_kernel)
-- is tested through poison: every row an image does not hold is NaN in x and dy (in production they are torch.empty memory), and every
result on the rows that count must stay finite and match.  Each poisoned case also runs clean, which tells a contract failure from a
numerical one.

Bars: the project's own for this operation against this reference (test_gpu_layers.py test_inception_block_as_one_merged_convolution):
fp32 1e-4 outputs / 3e-4 gradients relative to the tensor's maximum, bf16 relative L2 3e-2 outputs / 4e-2 gradients; a kernel gradient
is judged against the largest gradient of the block (floor 1e-2 gmax).  period_aggregate: n fp32 fused multiply-adds per element (k + 1
for out, 1 for dY, total N for dw), allowed 2 n 2^-24 sum|terms| per element with the sum from the float64 reference; "ratio" below is
the largest error / allowance.

Measured on an MI355X: the worst over shared / per-image x, GELU / none, poisoned / clean (a poisoned run gave its clean run's figures
but for the fp32 db_eff, which moves in its last digit between any two runs), and over the kernels of an Inception block.  Every test prints its figures ("MEASURED | case | quantity | measured | bar") before it asserts.

    case                               quantity                    measured   bar
    conv2d_periods 1 (fp32 8->16)      y                           4.0e-07    1e-4
                                       dx                          5.0e-07    3e-4
                                       dW_eff                      1.8e-07    3e-4
                                       db_eff                      1.3e-07    3e-4
                                       dx, rows beyond total       4.8e-07    3e-4
    conv2d_periods 2 (fp32 6->10)      y                           2.4e-07    1e-4
                                       dx                          2.7e-07    3e-4
                                       dW_eff                      1.5e-07    3e-4
                                       db_eff                      1.8e-07    3e-4
                                       dx, rows beyond total       2.0e-07    3e-4
    conv2d_periods 3 (fp32 5->8)       y                           2.4e-07    1e-4
                                       dx                          1.7e-07    3e-4
                                       dW_eff                      2.4e-07    3e-4
                                       db_eff                      1.5e-07    3e-4
                                       dx, rows beyond total       1.8e-07    3e-4
    conv2d_periods 4 (bf16 8->16)      y                           2.4e-03    3e-2
                                       dx                          2.8e-03    4e-2
                                       dW_eff                      2.9e-03    4e-2
                                       db_eff                      2.4e-03    4e-2
                                       dx, rows beyond total       2.8e-03    4e-2
    conv2d_periods 5 (bf16 16->8)      y                           2.5e-03    3e-2
                                       dx                          3.0e-03    4e-2
                                       dW_eff                      3.1e-03    4e-2
                                       db_eff                      2.3e-03    4e-2
                                       dx, rows beyond total       3.2e-03    4e-2
    conv2d_periods 6 (bf16 72->8)      y                           2.3e-03    3e-2
                                       dx                          2.8e-03    4e-2
                                       dW_eff                      3.1e-03    4e-2
                                       db_eff                      3.4e-03    4e-2
                                       dx, rows beyond total       3.9e-03    4e-2
    period_aggregate (3, 15, 5, 1)     out / dY / dw (ratio)       0.24 / 0 / 0.0020       1
    period_aggregate (2, 30, 8, 5)     out / dY / dw (ratio)       0.23 / 0.48 / 0.00068   1
    period_aggregate (5, 14, 7, 16)    out / dY / dw (ratio)       0.11 / 0.49 / 0.0025    1
    TimesBlock (a) fp32                out                         1.8e-07    1e-4
                                       dx                          1.4e-07    3e-4
                                       Conv2d weights / biases     4.4e-07 / 1.7e-07       3e-4
    TimesBlock (b) bf16 implicit       out                         5.5e-04    3e-2
                                       dx                          6.9e-04    4e-2
                                       Conv2d weights / biases     3.7e-03 / 3.0e-03       4e-2
    TimesBlock (c) bf16 batched im2col out                         1.2e-03    3e-2
                                       dx                          1.5e-03    4e-2
                                       Conv2d weights / biases     3.6e-03 / 3.0e-03       4e-2

Within a factor of 3 of its bar: only period_aggregate's dY, at 0.48 - 0.49 of its allowance -- by construction, not by accident: dY is ONE
fp32 product, whose rounding error is at most 2^-24 of it, half of the 2 x 2^-24 allowed, and some element always comes close to that.
Everything else keeps a factor of 4 (period_aggregate's out) to several hundred (the fp32 forms).
"""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timesnet_periods_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rel(a, b, floor=1e-3):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / max(float(b.abs().max()), floor))


def _l2err(a, b, floor=1e-3):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).norm() / max(float(b.norm()), floor * max(1.0, b.numel() ** 0.5)))


def _bars(precision):
    """(error measure, bar on outputs, bar on gradients)"""
    return (_rel, 1e-4, 3e-4) if precision == "fp32" else (_l2err, 3e-2, 4e-2)


def _note(case, quantity, measured, bar):
    print(f"MEASURED | {case} | {quantity} | {measured:.3g} | {bar:.3g}")


def _check(case, errs, bar):
    for q, e in errs.items():
        _note(case, q, e, bar)
    bad = {q: e for q, e in errs.items() if not e <= bar}       # (a NaN is bad)
    assert not bad, (case, bad)


# ---------------------------------------------------------------------------------------------------------------- period_rows
def _tops(total):
    """16 frequency indices: 0 (the kernel's guard), 1 (period == total), total // 2 and two more of period 2 (coinciding periods), the
    first whose period does not divide total, then the remaining small ones round robin"""
    half = total // 2
    pair = (25, 26) if total == 64 else (half - 1, half - 2)
    nd = next(f for f in range(2, half) if total % (total // f))
    assert total // half == 2 and total // pair[0] == 2 and total // pair[1] == 2
    pool = [0, 1, half, pair[0], nd, pair[1]]
    f = 2
    while len(pool) < 16:
        pool.append(f)
        f = f + 1 if f < half else 2
    return pool


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("total", [14, 30, 64, 65])
def test_period_rows_is_bit_exact(total, B, k):
    dev = _dev()
    from immtsf import ops
    pool = _tops(total)
    tops = [[f] for f in pool] if k == 1 else [pool[:k]]       # (k == 1: every value of the pool on its own)
    for top in tops:
        period, rows = ops.period_rows(torch.tensor(top, dtype=torch.int64, device=dev), total, B)
        want_p, want_r = R.period_rows_ref(top, total, B)
        assert period.dtype == torch.int32 and rows.dtype == torch.int32
        assert np.array_equal(period.cpu().numpy(), want_p), (top, period.tolist(), want_p.tolist())
        assert np.array_equal(rows.cpu().numpy(), want_r), (top, rows.tolist(), want_r.tolist())


# ---------------------------------------------------------------------------------------------------------------- conv2d_periods
# device periods: period == total (a one-row image), periods that do not divide total, period 2 twice (the duplicate), period 1 (a
# one-column image: no frequency yields it, the kernels accept it)
PERIODS = {15: [15, 7, 5, 2, 2, 1], 14: [14, 4, 7, 2, 2, 1], 33: [33, 7, 11, 2, 2, 1]}
CONV_CASES = {     # precision, Cin, Cout, KS, B, total
    1: ("fp32", 8, 16, 5, 3, 15),      # im2col with 8 channels per item
    2: ("fp32", 6, 10, 3, 2, 14),      # one channel per item; channel counts that are no multiple of 4
    3: ("fp32", 5, 8, 3, 3, 15),       # a shared x with B, total and Cin odd: (Lmax B Cin) % 4 == 2 in the sum over the images
    4: ("bf16", 8, 16, 5, 3, 15),      # the batched im2col form
    5: ("bf16", 16, 8, 3, 2, 33),      # Lmax 66: a second layer's shape
    6: ("bf16", 72, 8, 1, 2, 14),      # more than 64 channels
}
CONV_PARAMS = [(c, s) for c in (1, 2, 4, 5) for s in (True, False)] + [(3, True), (6, True)]


def _conv_dims(case):
    precision, Cin, Cout, KS, B, total = CONV_CASES[case]
    periods = PERIODS[total]
    rows = [-(-total // p) * p * B for p in periods]
    return precision, Cin, Cout, KS, B, total, 2 * total, periods, rows


@functools.lru_cache(maxsize=None)
def _conv_inputs(case, shared):
    """finite inputs (CPU, float32): x on every row, dy zero beyond each image, the kernel and its bias"""
    precision, Cin, Cout, KS, B, total, Lmax, periods, rows = _conv_dims(case)
    k, Rr = len(periods), Lmax * B
    g = torch.Generator().manual_seed(100 * case + int(shared))
    x = torch.randn(*(() if shared else (k,)), Rr, Cin, generator=g)
    dy = torch.randn(k, Rr, Cout, generator=g)
    for j, r in enumerate(rows):
        dy[j, r:] = 0
    K = KS * KS * Cin
    Weff = torch.randn(Cout, K, generator=g) / K ** 0.5
    beff = torch.rand(Cout, generator=g) * 0.4 - 0.2
    return x, dy, Weff, beff


@functools.lru_cache(maxsize=None)
def _conv_reference(case, shared, act):
    """float64 on the CPU, once per (case, shared, act): y, valid, dx, dW_eff, db_eff"""
    precision, Cin, Cout, KS, B, total, Lmax, periods, rows = _conv_dims(case)
    x, dy, Weff, beff = (t.double() for t in _conv_inputs(case, shared))
    x.requires_grad_(True), Weff.requires_grad_(True), beff.requires_grad_(True)
    y, valid = R.conv_periods_ref(x, periods, Weff, beff, KS, B, Lmax, act, rows=rows)
    y.backward(gradient=dy)
    return y.detach(), valid, x.grad, Weff.grad, beff.grad


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("case,shared", CONV_PARAMS)
def test_conv2d_periods_vs_float64(case, shared, poison):
    dev = _dev()
    from immtsf import ops
    precision, Cin, Cout, KS, B, total, Lmax, periods, rows = _conv_dims(case)
    hf = precision == "bf16"
    if hf:      # the shapes period_hf (csrc/conv.hip) takes: channel counts multiples of 8
        assert Cin % 8 == 0 and Cout % 8 == 0
    k = len(periods)
    err, tol_o, tol_g = _bars(precision)
    x0, dy0, W0, b0 = _conv_inputs(case, shared)
    period = torch.tensor(periods, dtype=torch.int32, device=dev)
    rows_d = torch.tensor(rows, dtype=torch.int32, device=dev)
    x0, dy0 = x0.clone(), dy0.clone()
    if poison:
        if shared:
            x0[max(rows):] = NAN
        for j, r in enumerate(rows):
            dy0[j, r:] = NAN
            if not shared:
                x0[j, r:] = NAN
    for act in ("gelu", None):
        name = f"conv {case} {'shared' if shared else 'per-image'} {act or 'none'} {'poison' if poison else 'clean'}"
        y_ref, valid, dx_ref, dW_ref, db_ref = _conv_reference(case, shared, act)
        x = x0.to(dev).requires_grad_(True)
        Weff, beff = W0.to(dev).requires_grad_(True), b0.to(dev).requires_grad_(True)
        y = ops.conv2d_periods(x, period, rows_d, Weff, beff, KS, B, Lmax, act=act, precision=precision)
        # the form: the im2col image this call kept (never the implicit one), as bf16 exactly in the batched bf16 form
        col = y.grad_fn.saved_tensors[0]
        assert col.shape == (k, Lmax * B, KS * KS * Cin) and col.dtype == (torch.bfloat16 if hf else torch.float32)
        y.backward(gradient=dy0.to(dev))
        torch.cuda.synchronize()
        yv, dx = y.detach().cpu()[valid], x.grad.cpu()
        assert bool(torch.isfinite(yv).all()), name
        _check(name, {"y": err(yv, y_ref[valid])}, tol_o)
        head, head_ref = (dx[:total * B], dx_ref[:total * B]) if shared else (dx[:, :total * B], dx_ref[:, :total * B])
        dW, db = Weff.grad.cpu(), beff.grad.cpu()
        for q, t in (("dx", head), ("dW_eff", dW), ("db_eff", db)):
            assert bool(torch.isfinite(t).all()), (name, q)
        gmax = max(float(dW_ref.abs().max()), float(db_ref.abs().max()))
        _check(name, {"dx": err(head, head_ref), "dW_eff": err(dW, dW_ref, floor=1e-2 * gmax), "db_eff": err(db, db_ref, floor=1e-2 * gmax)},
               tol_g)
        if shared:
            # the whole of a shared dx is written: the sum over the images that hold the row, exact zeros where none does
            body = dx[total * B:max(rows)]
            assert bool(torch.isfinite(body).all()), name
            _check(name, {"dx rows beyond total": err(body, dx_ref[total * B:max(rows)])}, tol_g)
            assert not dx[max(rows):].any(), name
            assert max(rows) < Lmax * B


# ---------------------------------------------------------------------------------------------------------------- period_aggregate
@pytest.mark.parametrize("B,total,N,k", [(3, 15, 5, 1), (2, 30, 8, 5), (5, 14, 7, 16)])
def test_period_aggregate_vs_float64(B, total, N, k):
    dev = _dev()
    from immtsf import ops
    Lmax = 2 * total
    g = torch.Generator().manual_seed(B * 100 + k)
    Y0 = torch.randn(k, Lmax * B, N, generator=g)
    w0 = torch.softmax(torch.randn(B, k, generator=g), 1)
    x0 = torch.randn(B, total, N, generator=g)
    dout = torch.randn(B, total, N, generator=g)
    Yd, wd, xd = (t.double().requires_grad_(True) for t in (Y0, w0, x0))
    want = R.period_aggregate_ref(Yd, wd, xd, B, total, Lmax)
    want.backward(gradient=dout.double())
    Yp = Y0.clone()
    Yp[:, total * B:] = NAN                     # positions >= total: the crop drops them, nothing may read them
    Y, w, x = (t.to(dev).requires_grad_(True) for t in (Yp, w0, x0))
    out = ops.period_aggregate(Y, w, x, B, total, Lmax)
    out.backward(gradient=dout.to(dev))
    torch.cuda.synchronize()
    eps = 2.0 ** -24
    Yc = Y0.double().reshape(k, Lmax, B, N)[:, :total].permute(2, 1, 3, 0)                    # (B, total, N, k)
    prod = Yc.abs() * w0.double().reshape(B, 1, 1, k)
    allow = {"out": 2 * (k + 1) * eps * (x0.double().abs() + prod.sum(-1)),
             "dY": 2 * eps * Yd.grad.abs(),
             "dw": 2 * (total * N) * eps * (dout.double().abs().unsqueeze(-1) * Yc.abs()).sum((1, 2))}
    got = {"out": out.detach().cpu(), "dY": Y.grad.cpu(), "dw": w.grad.cpu()}
    ref = {"out": want.detach(), "dY": Yd.grad, "dw": wd.grad}
    name = f"aggregate B{B} total{total} N{N} k{k}"
    ratios = {}
    for q in ("out", "dY", "dw"):
        assert bool(torch.isfinite(got[q]).all()), (name, q)
        d, a = (got[q].double() - ref[q]).abs(), allow[q]
        ratios[q + " (ratio)"] = float((d / a.clamp(min=1e-300)).max()) if bool((a > 0).any()) else 0.0
        assert bool((d[a == 0] == 0).all()), (name, q)
    _check(name, ratios, 1.0)
    assert not got["dY"][:, total * B:].any()                  # exact zeros on the rows the crop dropped
    assert torch.equal(x.grad.cpu(), dout)                     # the residual passes the gradient through


# ---------------------------------------------------------------------------------------------------------------- a whole TimesBlock
BLOCKS = {      # precision, input_len, pred_len, d_model, d_ff, num_kernels, form
    "a": ("fp32", 18, 12, 8, 16, 3, "fp32"),
    "b": ("bf16", 18, 12, 8, 16, 3, "implicit"),
    "c": ("bf16", 40, 26, 8, 16, 2, "batched im2col"),
}


@functools.lru_cache(maxsize=None)
def _block_reference(name):
    """TimesBlock(cfg).double() on the CPU (the plain-torch loop over host periods), once per configuration: state dict, x, upstream
    gradient, output, dx, the Conv2d gradients by name"""
    from models.TimesNet import TimesBlock
    precision, input_len, pred_len, d_model, d_ff, nk, _ = BLOCKS[name]
    B, total, N, freqs, amps, seed = R.BLOCK_BATCHES[name]
    assert total == input_len + pred_len and N == d_model
    cfg = types.SimpleNamespace(input_len=input_len, pred_len=pred_len, d_model=d_model, d_ff=d_ff, num_kernels=nk, top_k=len(freqs))
    torch.manual_seed(21)
    ref = TimesBlock(cfg).double()
    with torch.no_grad():
        for c in ref.modules():
            if isinstance(c, torch.nn.Conv2d):
                c.bias.uniform_(-0.2, 0.2)
    x = R.spectral_batch(B, total, N, freqs, amps, seed)
    up = torch.randn(B, total, N, generator=torch.Generator().manual_seed(seed + 1))
    xd = x.double().requires_grad_(True)
    out = ref(xd)
    (out * up.double()).sum().backward()
    grads = {k: p.grad for k, p in ref.named_parameters()}
    return cfg, {k: v.float() for k, v in ref.state_dict().items()}, x, up, out.detach(), xd.grad, grads


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_timesblock_vs_float64_block(name, monkeypatch):
    dev = _dev()
    import models.TimesNet as TN
    from immtsf import config, ops
    precision, input_len, pred_len, d_model, d_ff, nk, form = BLOCKS[name]
    cfg, state, x0, up, out_ref, dx_ref, g_ref = _block_reference(name)
    B, total, N, freqs, amps, seed = R.BLOCK_BATCHES[name]
    Lmax, k = 2 * total, len(freqs)
    blk = TN.TimesBlock(cfg).to(dev)
    blk.load_state_dict(state)
    calls = {"conv2d_periods": [], "inception_periods": []}

    def spy(fn_name):
        fn = getattr(TN, fn_name)

        def wrapped(*a, **kw):
            y = fn(*a, **kw)
            calls[fn_name].append(y.grad_fn.saved_tensors[0].dtype if fn_name == "conv2d_periods" else None)
            return y
        monkeypatch.setattr(TN, fn_name, wrapped)
    spy("conv2d_periods")
    spy("inception_periods")
    config.precision = precision
    try:
        # the form this configuration is meant to take, from the conditions csrc/conv.hip states (period_hf, conv_period_mfma_ok)
        hf = precision == "bf16" and d_model % 8 == 0 and d_ff % 8 == 0
        fits = Lmax <= 128 and Lmax * max(d_model, d_ff) * 2 <= 16 * 1024
        assert {"fp32": not hf, "implicit": hf and fits, "batched im2col": hf and not fits}[form]
        for inc in (blk.conv[0], blk.conv[2]):
            assert ops.inception_periods_ok(inc, Lmax) == (form == "implicit")
        x = x0.to(dev).requires_grad_(True)
        top, _ = TN.fft_for_period_device(x.detach(), k)
        assert set(top.tolist()) == set(freqs)       # (the gap that guarantees it: tests/test_timesnet_periods_ref.py)
        out = blk(x)
        (out * up.to(dev)).sum().backward()
        torch.cuda.synchronize()
    finally:
        config.precision = "fp32"
    if form == "implicit":
        assert calls == {"conv2d_periods": [], "inception_periods": [None, None]}
    else:
        assert calls == {"conv2d_periods": [torch.float32 if form == "fp32" else torch.bfloat16] * 2, "inception_periods": []}
    err, tol_o, tol_g = _bars(precision)
    case = f"block ({name}) {form}"
    _check(case, {"out": err(out, out_ref)}, tol_o)
    gmax = max(float(g.abs().max()) for g in g_ref.values())
    errs = {"dx": err(x.grad, dx_ref)}
    for key, p in blk.named_parameters():
        assert p.grad is not None, key
        errs[key] = err(p.grad, g_ref[key], floor=1e-2 * gmax)
    assert len(errs) == 1 + 4 * nk
    _check(case, errs, tol_g)
