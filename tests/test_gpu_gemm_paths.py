"""Every route of the GEMM family (csrc/gemm.hip, gemm2.hip, gemm3.hip, linear_small.hip) through the C ABI, exactly.

Each case of tests/gemm_cases.py (1) asserts the route the launcher took -- the kernel code and grid of immtsf_debug_last_gemm_launch
and, for entries behind immtsf_launch_gemm, the timing tap's record -- against the route the table derives; (2) runs integer operands and
demands torch.equal with tests/gemm_ref.exact on every element of C, Ch and the bias gradient: no tolerance, any summation order
(see gemm_ref.py); (3) allocates every output at its full pitch over a sentinel and demands that pitch padding, and rows at and beyond
a device-side row count, still hold what they held (the contract include/immtsf.h states for `dyn` / `dyn_rows`), with NaN planted in the
operand rows no result may depend on; (4) where the table says so runs a real-operand instance at the same shape against the derived
per-element gemm_ref.bound.

Observed on an MI355X: erf GELU (cases gelu-p0 / gelu-p1: z exact, so the error is the fp32 evaluation of
0.5 z (1 + erf(z / sqrt 2)) alone) at most 0.081 of its bar 8 * 2^-24 * max(|z|, 1); real operands at most 0.149 of gemm_ref.bound."""
import ctypes
import os
import sys
import zlib

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "imm-tsf_amd"), os.path.dirname(os.path.abspath(__file__))]
import gemm_cases as T      # noqa: E402
import gemm_ref as R        # noqa: E402

pytestmark = pytest.mark.gpu
SENT, SENT_H = 7777.0, -512.0
NAN = float("nan")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _lib():
    from immtsf import _lib
    return _lib, _lib.load()


def _route(lib):
    g = ctypes.c_int64(0)
    code = lib.immtsf_debug_last_gemm_launch(ctypes.byref(g))
    return code, g.value


class Tap:
    """the GEMM timing tap around a call: .records = the (layout, precision, M, N, K, nprob, nbatch, dyn, grid threads, path) tuples"""

    def __init__(self, lib):
        self.lib, self.records = lib, []

    def __enter__(self):
        self.lib.immtsf_timing_enable(1)
        return self

    def __exit__(self, *exc):
        try:
            meta, ms = (ctypes.c_int32 * 160)(), (ctypes.c_float * 16)()
            n = self.lib.immtsf_timing_collect(16, meta, ms, None)
            self.records = [tuple(meta[10 * i:10 * i + 10]) for i in range(n)]
        finally:
            self.lib.immtsf_timing_enable(0)
        return False


def _pitched(t, ld, dev, fill=NAN):
    """t (rows, cols) inside a (rows, ld) device buffer whose padding holds `fill`"""
    buf = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf.to(dev)


def _assert_route(c, got, rec=None):
    want = (c["code"], c["grid"])
    assert got == want, (f"{c['id']}: the table derives kernel {want[0]} on {want[1]} grid threads ({c['why']}); the launcher took kernel "
                         f"{got[0]} on {got[1]} grid threads")
    if c["path"] is not None:
        assert rec is not None and len(rec) == 1, (c["id"], rec)
        r = rec[0]
        assert r[:5] == (c["layout"], c["opt"]["prec"], c["M"], c["N"], c["K"]) and r[8] == c["grid"] and r[9] == c["path"], (c["id"], r)


RATIOS = {"gelu": 0.0, "real": 0.0}


def _run(c, real):
    dev = _dev()
    L, lib = _lib()
    ptr, sp = L.ptr, L.stream_ptr
    o, lay, M, N, K, entry = c["opt"], c["layout"], c["M"], c["N"], c["K"], c["entry"]
    seed = zlib.crc32(c["id"].encode()) % 100000
    prec = o.get("prec", 1)
    bf = entry != "gemm"                # operands are bf16 in memory
    pa, pb, pc, ph = o.get("pad", (0, 0, 0, 0))
    a_shape = (K, M) if lay == 2 else (M, K)
    b_shape = (N, K) if lay == 0 else (K, N)

    def operand(shape, s):
        """(what the kernel is given, what the reference multiplies)"""
        if not real:
            v = R.int_operands(shape, s)
            return v, v
        v, img = R.real_operands(shape, s)
        return (img, img) if bf else (v, img if (prec == 1 and not o.get("f32")) else v)

    def vec(n, s):
        return R.real_operands((n,), s)[0] if real else R.int_operands((n,), s)

    A, Aref = operand(a_shape, seed)
    B, Bref = operand(b_shape, seed + 1)
    alpha = o.get("alpha", 1.0)
    bias = vec(N, seed + 2) if o.get("bias") else None
    add_vec = vec(N, seed + 3) if o.get("add_vec") else None
    c_old = (R.real_operands((M, N), seed + 4)[0] if real else R.int_operands((M, N), seed + 4)) if o.get("acc") else None
    dyn = o.get("dyn")
    rows = dyn if (dyn and lay != 2) else None
    kk = dyn if (dyn and lay == 2) else None
    rowmap = None
    if o.get("rowmap"):
        rowmap = torch.randint(0, M, (M,), generator=torch.Generator().manual_seed(seed + 5)).int()
        rowmap[1] = rowmap[0]           # a repeat for certain
    flag, div = None, o.get("flag_div", 1)
    if o.get("flag_div"):
        flag = torch.randint(0, 4, (T.cdiv(M, div),), generator=torch.Generator().manual_seed(seed + 6)).int()
        e = 128 // div                  # the group that straddles the 128-row tile edge is dead, its neighbours live
        flag[e - 1], flag[e], flag[e + 1] = 2, 0, 1
    ref = R.exact(lay, Aref, Bref, alpha, bias, add_vec, flag, div, c_old, o.get("act", 0), None, rowmap, rows, kk)
    mrows = rows if rows is not None else M

    # operands as the kernel sees them: NaN wherever no asserted element may depend on the value
    Ak, Bk = A.clone(), B.clone()
    if rows is not None:
        used = rowmap[:rows].long() if rowmap is not None else torch.arange(rows)
        dead = torch.ones(M, dtype=torch.bool)
        dead[used] = False
        Ak[dead] = NAN
    if kk is not None:
        Ak[kk:] = NAN
        Bk[kk:] = NAN
    dt = torch.bfloat16 if bf else torch.float32
    lda, ldb, ldc = a_shape[1] + pa, b_shape[1] + pb, N + pc
    ldch = N + ph if o.get("ch") else 0
    Ad, Bd = _pitched(Ak.to(dt), lda, dev), _pitched(Bk.to(dt), ldb, dev)
    Cd = None if o.get("no_c") else _pitched(c_old if c_old is not None else torch.full((M, N), SENT), ldc, dev, SENT)
    Hd = torch.full((M, ldch), SENT_H, dtype=torch.bfloat16, device=dev) if o.get("ch") else None
    bg_old = (R.int_operands((M,), seed + 7) if (o.get("acc") and entry == "gemm3_tn") else torch.full((M,), SENT)) if o.get("bgrad") else None
    Gd = torch.cat([bg_old, torch.full((3,), SENT)]).to(dev) if o.get("bgrad") else None
    biasd = bias.to(dev) if bias is not None else None
    addd = add_vec.to(dev) if add_vec is not None else None
    flagd = flag.to(dev) if flag is not None else None
    mapd = rowmap.to(dev) if rowmap is not None else None
    dynd = torch.tensor([dyn], dtype=torch.int32, device=dev) if dyn else None
    C0 = Cd.clone() if Cd is not None else None

    twin = None
    tap = Tap(lib)
    try:
        if o.get("twin"):
            twin = Bd.bfloat16()
            L.check(lib.immtsf_bf16_twin_register(ptr(Bd), ptr(twin), Bd.numel()), "twin_register")
        if o.get("g3cfg"):
            lib.immtsf_debug_gemm3_config(o["g3cfg"], 0)
        with tap:
            if entry == "gemm":
                rc = lib.immtsf_gemm(lay, prec, ptr(Ad), lda, ptr(Bd), ldb, ptr(Cd), ldc, ptr(biasd), M, N, K, alpha, o.get("acc", 0), o.get("act", 0), sp())
            elif entry == "gemm_bf16":
                rc = lib.immtsf_gemm_bf16(lay, ptr(Ad), lda, ptr(Bd), ldb, ptr(Cd), ldc, ptr(Hd), ldch, ptr(biasd), ptr(Gd), M, N, K, alpha, o.get("acc", 0),
                                          o.get("act", 0), ptr(dynd), 1 if lay == 2 else 0, ptr(mapd), sp())
            elif entry == "gemm3":
                rc = lib.immtsf_gemm3_bf16(lay, ptr(Ad), lda, ptr(Bd), ldb, ptr(Cd), ldc, ptr(Hd), ldch, ptr(biasd), ptr(addd), ptr(flagd), div, M, N, K,
                                           alpha, 0, ptr(dynd), sp())
            else:
                wsb = lib.immtsf_gemm3_tn_workspace_bytes(M, N, K)
                assert wsb > 0, c["id"]
                ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
                rc = lib.immtsf_gemm3_tn_bf16(ptr(Ad), lda, ptr(Bd), ldb, ptr(Cd), ldc, ptr(Gd), M, N, K, alpha, o.get("acc", 0), ptr(dynd), ptr(ws), wsb, sp())
            L.check(rc, c["id"])
            got = _route(lib)
        torch.cuda.synchronize()
    finally:
        if o.get("g3cfg"):
            lib.immtsf_debug_gemm3_config(0, 0)
        if twin is not None:
            lib.immtsf_bf16_twin_unregister(ptr(Bd))
    _assert_route(c, got, tap.records)

    act = o.get("act", 0)
    if Cd is not None:
        out = Cd.cpu()
        want = C0.cpu()
        if real or act == 2:
            if real:
                a64, b64 = R.ops(lay, Aref, Bref, rowmap, rows, kk)
                addends = [x.abs().double() for x in (bias, add_vec, c_old[:mrows] if c_old is not None else None) if x is not None]
                extra = sum(addends) if addends else None
                bar = R.bound(a64, b64, alpha, extra, kk or K)
                key = "real"
            else:
                bar = 8 * 2.0 ** -24 * ref.z.abs().clamp(min=1.0)
                key = "gelu"
            err = (out[:mrows, :N].double() - ref.C).abs()
            ratio = float((err / bar.clamp(min=1e-300)).max())
            RATIOS[key] = max(RATIOS[key], ratio)
            print(f"{c['id']}: {key} worst error / bar = {ratio:.4f}")
            assert bool((err <= bar).all()), (c["id"], ratio)
            want[:mrows, :N] = out[:mrows, :N]      # (the rest of the buffer is compared below)
        else:
            want[:mrows, :N] = ref.C.float()
        assert torch.equal(out, want), (c["id"], "C", int((out != want).sum()), float((out[:mrows, :N].double() - ref.C).abs().max()))
    if Hd is not None and not real:
        want = torch.full((M, ldch), SENT_H, dtype=torch.bfloat16)
        want[:mrows, :N] = ref.Ch
        outh = Hd.cpu()
        assert torch.equal(outh, want), (c["id"], "Ch", int((outh != want).sum()))
    if Gd is not None and not real:
        want = torch.cat([bg_old, torch.full((3,), SENT)])
        want[:M] = ref.bias_grad.float() + (bg_old if (o.get("acc") and entry == "gemm3_tn") else 0.0)
        outg = Gd.cpu()
        assert torch.equal(outg, want), (c["id"], "bias_grad", int((outg != want).sum()))


@pytest.mark.parametrize("cid", [c["id"] for c in T.CASES])
def test_route_exact_on_integers(cid):
    """integer operands: every element exact.  The two erf-GELU cases instead hold 8 * 2^-24 * max(|z|, 1) on an exact z; largest
    observed ratio to that bar: 0.081"""
    _run(T.BY_ID[cid], real=False)


@pytest.mark.parametrize("cid", [c["id"] for c in T.CASES if c["opt"].get("real")])
def test_route_within_bound_on_reals(cid):
    """randn operands at the route's smallest K: every element within gemm_ref.bound of the float64 product of the RNE bf16 images (of
    the fp32 values for precision 0 and the skinny kernels); largest observed fraction of the bound: 0.149"""
    assert T.BY_ID[cid]["K"] <= 136
    _run(T.BY_ID[cid], real=True)


# ------------------------------------------------------------------------------------------------------------ immtsf_linear_backward
def _linear_data(M, N, K, relu, dev):
    x, W, dy = R.int_operands((M, K), M), R.int_operands((N, K), N + 1), R.int_operands((M, N), K + 2)
    rx = R.int_operands((M, K), 3) if relu else None
    dx = dy.double() @ W.double()
    if relu:
        dx = torch.where(rx.double() <= 0, torch.zeros_like(dx), dx)
    return x, W, dy, rx, dx.float(), (dy.double().t() @ x.double()).float(), dy.double().sum(0).float()


@pytest.mark.parametrize("which", ["both", "dx", "dw"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("M,N,K", T.LINEAR_SMALL)
@pytest.mark.parametrize("prec", [0, 1])
def test_linear_backward_small_route(prec, M, N, K, relu, which):
    """linear_small.hip: one launch, dW / db ADDED by atomics to sinks that hold 5 and -2; the tap records no GEMM launch for the call"""
    dev = _dev()
    L, lib = _lib()
    x, W, dy, rx, rdx, rdW, rdb = _linear_data(M, N, K, relu, dev)
    dx = torch.full((M * K + 5,), SENT, device=dev) if which != "dw" else None
    dW = torch.full((N * K + 5,), 5.0, device=dev) if which != "dx" else None
    db = torch.full((N + 5,), -2.0, device=dev) if which != "dx" else None
    xd, Wd, dyd, rxd = x.to(dev), W.to(dev), dy.to(dev), (rx.to(dev) if relu else None)
    before = _route(lib)
    with Tap(lib) as tap:
        L.check(lib.immtsf_linear_backward(prec, L.ptr(xd), L.ptr(Wd), L.ptr(dyd), M, N, K, L.ptr(dx), L.ptr(rxd), L.ptr(dW), L.ptr(db), 1, L.stream_ptr()), "linear_backward")
    torch.cuda.synchronize()
    assert tap.records == [] and _route(lib) == before, ("expected linear_small.hip (N <= 32, K <= 64, M <= 4096), GEMM launches were made", tap.records)
    if dx is not None:
        assert torch.equal(dx.cpu(), torch.cat([rdx.flatten(), torch.full((5,), SENT)]))
    if dW is not None:
        assert torch.equal(dW.cpu(), torch.cat([rdW.flatten() + 5.0, torch.full((5,), 5.0)]))
        assert torch.equal(db.cpu(), torch.cat([rdb - 2.0, torch.full((5,), -2.0)]))


@pytest.mark.parametrize("which", ["both", "dx", "dw"])
@pytest.mark.parametrize("prezeroed", [0, 1])
@pytest.mark.parametrize("M,N,K", list(T.LINEAR_GEMM))
@pytest.mark.parametrize("prec", [0, 1])
def test_linear_backward_gemm_route(prec, M, N, K, prezeroed, which):
    """just outside linear_small's limits: dx on an NN product (ReLU mask in the epilogue), dW on a TN product whose ones_col reduction gives db"""
    dev = _dev()
    L, lib = _lib()
    x, W, dy, rx, rdx, rdW, rdb = _linear_data(M, N, K, 1, dev)
    fill = 0.0 if prezeroed else SENT
    dx = torch.full((M * K + 5,), SENT, device=dev) if which != "dw" else None
    dW = torch.full((N * K,), fill, device=dev) if which != "dx" else None
    db = torch.full((N,), fill, device=dev) if which != "dx" else None
    xd, Wd, dyd, rxd = x.to(dev), W.to(dev), dy.to(dev), rx.to(dev)
    with Tap(lib) as tap:
        L.check(lib.immtsf_linear_backward(prec, L.ptr(xd), L.ptr(Wd), L.ptr(dyd), M, N, K, L.ptr(dx), L.ptr(rxd), L.ptr(dW), L.ptr(db), prezeroed, L.stream_ptr()), "linear_backward")
        last = _route(lib)
    torch.cuda.synchronize()
    (cx, gx, whyx), (cw, gw, whyw) = T.LINEAR_GEMM[(M, N, K)][prec]
    want = ([(1, prec, M, K, N, gx, 1)] if dx is not None else []) + ([(2, prec, N, K, M, gw, 1)] if dW is not None else [])
    got = [r[:5] + (r[8], r[9]) for r in tap.records]
    assert got == want, (f"table: {want} ({whyx}; {whyw}); launcher: {got}")
    assert last == ((cw, gw) if dW is not None else (cx, gx)), (last, whyx, whyw)
    if dx is not None:
        assert torch.equal(dx.cpu(), torch.cat([rdx.flatten(), torch.full((5,), SENT)]))
    if dW is not None:
        assert torch.equal(dW.cpu(), rdW.flatten())
        assert torch.equal(db.cpu(), rdb)


# ------------------------------------------------------------------------------------------------------------ immtsf_gemm_bf16_group_tn
@pytest.mark.parametrize("real", [0, 1])
@pytest.mark.parametrize("n", sorted(T.GROUPS))
def test_group_tn(n, real):
    dev = _dev()
    L, lib = _lib()
    mem = T.GROUPS[n]
    As, Bs, Cs, refs = [], [], [], []
    for i, (M, N, K) in enumerate(mem):
        a = R.real_operands((K, M), 50 + i)[1] if real else R.int_operands((K, M), 50 + i)
        b = R.real_operands((K, N), 70 + i)[1] if real else R.int_operands((K, N), 70 + i)
        As.append(a.bfloat16().to(dev))
        Bs.append(b.bfloat16().to(dev))
        Cs.append(torch.full((M * N + 4,), SENT, device=dev))
        refs.append((a, b))
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])      # noqa: E731
    ints = lambda j: (ctypes.c_int32 * n)(*[m[j] for m in mem])             # noqa: E731
    L.check(lib.immtsf_gemm_bf16_group_tn(n, arr(As), ints(0), arr(Bs), ints(1), arr(Cs), ints(1), ints(0), ints(1), ints(2), L.stream_ptr()), "group_tn")
    got = _route(lib)
    torch.cuda.synchronize()
    tiles = sum(T.cdiv(M, 64) * T.cdiv(N, 64) for M, N, K in mem)
    assert sum(T.cdiv(M, 128) * T.cdiv(N, 128) for M, N, K in mem) < 192
    assert got == (2900, tiles * 1024), (got, "table: 64x64 K-group tiles (fewer than 192 tiles of 128), one workgroup of 1024 threads per tile")
    for (M, N, K), (a, b), Cd in zip(mem, refs, Cs):
        out = Cd.cpu()
        assert torch.equal(out[M * N:], torch.full((4,), SENT))
        ref = R.exact(R.TN, a, b).C
        if real:
            a64, b64 = R.ops(R.TN, a, b)
            err, bar = (out[:M * N].view(M, N).double() - ref).abs(), R.bound(a64, b64, 1.0, None, K)
            ratio = float((err / bar.clamp(min=1e-300)).max())
            RATIOS["real"] = max(RATIOS["real"], ratio)
            print(f"group n={n} member {(M, N, K)}: real worst error / bar = {ratio:.4f}")
            assert bool((err <= bar).all()), ((M, N, K), ratio)
        else:
            assert torch.equal(out[:M * N].view(M, N), ref.float()), (M, N, K)


# ------------------------------------------------------------------------------------------------------------ immtsf_linear_bf16_*
@pytest.mark.parametrize("nl,act", [(1, 1), (3, 0)])
def test_linear_bf16_forward_backward(nl, act):
    """nn.Linear in the bf16 dataflow: forward (nl problems in one launch), the one-call backward, the same with db NULL, and the two-call
    form (data gradient first; then dx NULL with grads_prezeroed bit 1: weight gradients only, from the dy16 the first call left)"""
    dev = _dev()
    L, lib = _lib()
    M, N, K = T.LINEAR_BF16["M"], T.LINEAR_BF16["N"], T.LINEAR_BF16["K"]
    why = T.LINEAR_BF16["why"]
    x = R.int_operands((M, K), 1)
    Ws = [R.int_operands((N, K), 10 + i) for i in range(nl)]
    bs = [R.int_operands((N,), 20 + i) for i in range(nl)]
    dys = [R.int_operands((M, N), 30 + i) for i in range(nl)]
    xd, Wd, bd, dyd = x.to(dev), [w.to(dev) for w in Ws], [b.to(dev) for b in bs], [d.to(dev) for d in dys]
    x16 = torch.full((M * K + 8,), SENT_H, dtype=torch.bfloat16, device=dev)
    w16 = [torch.empty(N * K, dtype=torch.bfloat16, device=dev) for _ in range(nl)]
    ys = [torch.full((M * N + 4,), SENT, device=dev) for _ in range(nl)]
    arr = lambda ts: (ctypes.c_void_p * nl)(*[t.data_ptr() for t in ts])     # noqa: E731
    with Tap(lib) as tap:
        L.check(lib.immtsf_linear_bf16_forward(nl, L.ptr(xd), L.ptr(x16), arr(Wd), arr(w16), arr(bd), arr(ys), M, N, K, act, L.stream_ptr()), "linear_bf16_forward")
        last = _route(lib)
    torch.cuda.synchronize()
    v17 = 2 * 1024
    assert [r[:6] + r[8:] for r in tap.records] == [(0, 1, M, N, K, nl, v17 * nl, 2)] and last == (2017, v17 * nl), (tap.records, last, why)
    assert torch.equal(x16.cpu(), torch.cat([x.bfloat16().flatten(), torch.full((8,), SENT_H, dtype=torch.bfloat16)]))
    for i in range(nl):
        ref = R.exact(R.NT, x, Ws[i], bias=bs[i], act=act).C.float()
        assert torch.equal(ys[i].cpu(), torch.cat([ref.flatten(), torch.full((4,), SENT)])), i

    rdx = sum(dys[i].double() @ Ws[i].double() for i in range(nl)).float()
    rdW = [(dys[i].double().t() @ x.double()).float() for i in range(nl)]
    rdb = [dys[i].double().sum(0).float() for i in range(nl)]
    dx_rec = [(1, 1, M, K, N, 1, v17, 2)] * nl
    dw_rec = [(2, 1, N, K, M, 1, 1024, 2)] if nl == 1 else [(3, 1, N, K, M, nl, nl * 1024, 3)]

    def backward(dx_on, dw_on, db_on, flags):
        dy16 = backward.dy16
        dx = torch.full((M * K + 4,), SENT, device=dev) if dx_on else None
        dW = [torch.full((N * K + 4,), SENT, device=dev) for _ in range(nl)] if dw_on else None
        db = [torch.full((N + 4,), SENT, device=dev) for _ in range(nl)] if db_on else None
        with Tap(lib) as t:
            L.check(lib.immtsf_linear_bf16_backward(nl, L.ptr(x16), arr(Wd), arr(w16), arr(dyd), L.ptr(dy16), L.ptr(dx), arr(dW) if dW else None,
                                                    arr(db) if db else None, M, N, K, flags, L.stream_ptr()), "linear_bf16_backward")
        torch.cuda.synchronize()
        assert [r[:6] + r[8:] for r in t.records] == (dx_rec if dx_on else []) + (dw_rec if dw_on else []), (t.records, why)
        if dx_on:
            assert torch.equal(dx.cpu(), torch.cat([rdx.flatten(), torch.full((4,), SENT)]))
        for i in range(nl if dw_on else 0):
            assert torch.equal(dW[i].cpu(), torch.cat([rdW[i].flatten(), torch.full((4,), SENT)])), i
            if db_on:
                assert torch.equal(db[i].cpu(), torch.cat([rdb[i], torch.full((4,), SENT)])), i

    backward.dy16 = torch.full((nl * M * N,), SENT_H, dtype=torch.bfloat16, device=dev)
    backward(True, True, True, 0)               # one call
    backward(True, True, False, 0)              # db NULL
    backward.dy16 = torch.full((nl * M * N,), SENT_H, dtype=torch.bfloat16, device=dev)
    backward(True, False, False, 0)             # two calls: the data gradient (casts dy16) ...
    backward(False, True, True, 2)              # ... then the weight gradients alone from the images the first call left


def test_zz_report_ratios():
    """the figures the module docstring and DESIGN.md quote (printed; asserted per case above)"""
    _dev()
    print(f"worst GELU error / bar = {RATIOS['gelu']:.4f}; worst real-operand error / bound = {RATIOS['real']:.4f}")
