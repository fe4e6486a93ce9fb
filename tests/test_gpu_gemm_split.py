"""GPU checks of the split-bf16 product kernel (csrc/gemm_split.hip) through the C ABI: immtsf_split_bf16,
immtsf_gemm_split_supported and immtsf_gemm_split against tests/split_ref.py and float64.
Shapes: M in {1, 15, 16, 17, 129} x N in {8, 24, 136} x K in {8, 40, 264}, both layouts, with and without bias: one and several tiles
in every direction, ragged edges of the 16 / 64-row, 64-column tiles and of the 64-deep K step, the 16-row tiles (M <= 32) and the
64 x 64 ones; M = 32 / 33 (the two sides of that switch) and one 2049 x 1928 x 72 product on the 128 x 128 tiles.
Bar, per element and with no element left out: |C - C64| <= (2^-16 + 3 K 2^-24) (|A| |B|) + 1e-30 (derivation: tests/split_ref.py).

The exact-integer check: A and B hold integers |x| <= 300 and K <= 64, so every product and partial sum is an integer below 2^24 and
the kernel's fp32 sums are exact.  The scheme drops a_lo b_lo, which for these operands is not zero (257 x 259 = (256 + 1)(260 - 1):
the dropped term is -1), so the bits to match are those of the int64 value of the three KEPT terms, A B - A_lo B_lo -- a transposed
read or write, a lost or doubled term or a swapped image cannot reproduce it -- and, where one side has no lo image (an even A
against the same B, and the reverse), the int64 product itself."""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu
MS, NS, KS = (1, 15, 16, 17, 129), (8, 24, 136), (8, 40, 264)
EUNSUPPORTED = -3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _images(w):
    """(hi, lo) of a device fp32 tensor by immtsf_split_bf16"""
    from immtsf import _lib
    hi, lo = torch.empty_like(w, dtype=torch.bfloat16), torch.empty_like(w, dtype=torch.bfloat16)
    _lib.check(_lib.load().immtsf_split_bf16(_lib.ptr(w), w.numel(), _lib.ptr(hi), _lib.ptr(lo), _lib.stream_ptr()), "split_bf16")
    return hi, lo


def _product(layout, a, b, bias=None, out=None, c_off=0, ldc=None, w_rows=None):
    """a (M, K) b (K, N) on the device through immtsf_gemm_split; the weight is stored (N, K) for layout 0 and (K, N) for layout 1.
    w_rows = (r0, R) (layout 0): the weight is rows r0 .. r0 + N - 1 of an (R, K) matrix of other values"""
    from immtsf import _lib
    lib = _lib.load()
    M, K = a.shape
    N = b.shape[1]
    w = (b.t() if layout == 0 else b).contiguous()
    w_off = 0
    if w_rows is not None:
        r0, R = w_rows
        big = torch.full((R, K), 7.0, device=a.device)
        big[r0:r0 + N] = w
        w, w_off = big, r0 * K
    hi, lo = _images(w)
    ldb = w.shape[1]
    ldc = N if ldc is None else ldc
    if out is None:
        out = torch.full((M, ldc), float("nan"), device=a.device)
    adr = lambda t, off: C.c_void_p(t.data_ptr() + off * t.element_size())      # noqa: E731
    assert lib.immtsf_gemm_split_supported(layout, M, N, K, K, ldb, ldc)
    _lib.check(lib.immtsf_gemm_split(layout, _lib.ptr(a), K, adr(hi, w_off), adr(lo, w_off), ldb, adr(out, c_off), ldc, _lib.ptr(bias),
                                     M, N, K, _lib.stream_ptr()), "gemm_split")
    return out


@functools.lru_cache(maxsize=None)
def _case(M, N, K, kind):
    """operands and their float64 product and bar, computed once, shared"""
    a, b, bias = SR.operands(M, N, K, kind)
    return a, b, bias, a.double() @ b.double(), SR.bound(a, b)


def _worst(got, want, bar):
    return float(((got.double().cpu() - want).abs() / bar).max())


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("M", MS)
def test_exact_integers_bit_for_bit(layout, M):
    dev = _dev()
    for N in NS:
        for K in (8, 40, 64):
            a, b = SR.int_operands(M, N, K)
            (_, al), (_, bl) = SR.split(a), SR.split(b)
            assert int((bl != 0).sum()) > 0 and (M < 15 or int((al != 0).sum()) > 0)
            full = a.long() @ b.long()
            kept = full - al.float().long() @ bl.float().long()
            got = _product(layout, a.to(dev), b.to(dev)).cpu()
            assert torch.equal(got, kept.float()), (M, N, K, "three kept terms")
            even_a, even_b = 2 * (a / 2).trunc(), 2 * (b / 2).trunc()
            got = _product(layout, even_a.to(dev), b.to(dev)).cpu()
            assert torch.equal(got, (even_a.long() @ b.long()).float()), (M, N, K, "a_hi b_lo")
            got = _product(layout, a.to(dev), even_b.to(dev)).cpu()
            assert torch.equal(got, (a.long() @ even_b.long()).float()), (M, N, K, "a_lo b_hi")


@pytest.mark.parametrize("kind", ["normal", "scaled"])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("M", MS)
def test_random_operands_against_float64(M, layout, kind):
    dev = _dev()
    worst = 0.0
    for N in NS:
        for K in KS:
            a, b, bias, want, bar = _case(M, N, K, kind)
            for with_bias in (False, True):
                got = _product(layout, a.to(dev), b.to(dev), bias.to(dev) if with_bias else None)
                assert torch.isfinite(got).all()
                r = _worst(got, want + bias.double() if with_bias else want, bar)
                worst = max(worst, r)
                assert r <= 1.0, (M, N, K, layout, kind, with_bias, r)
    print(f"M {M} layout {layout} {kind}: worst error / bar {worst:.3f}")


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("shape", [(32, 136, 264), (33, 136, 264), (2049, 1928, 72)], ids=lambda s: "x".join(map(str, s)))
def test_tile_switches(shape, layout):
    """M = 32 is the last shape on the 16-row tiles, 33 the first on 64 x 64; 17 x 16 tiles of 128 x 128 are past the switch to those"""
    dev = _dev()
    a, b, bias, want, bar = _case(*shape, "normal")
    got = _product(layout, a.to(dev), b.to(dev), bias.to(dev))
    r = _worst(got, want + bias.double(), bar)
    print(f"{shape} layout {layout}: worst error / bar {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("layout", [0, 1])
def test_column_block_of_a_wider_result_leaves_the_guard_cells(layout):
    dev = _dev()
    M, N, K = 17, 136, 40
    a, b, bias, want, bar = _case(M, N, K, "normal")
    ldc, c_off, sentinel = N + 24, 16, -12345.5
    out = torch.full((M + 2, ldc), sentinel, device=dev)
    _product(layout, a.to(dev), b.to(dev), bias.to(dev), out=out[1:], c_off=c_off, ldc=ldc)
    out = out.cpu()
    assert _worst(out[1:M + 1, c_off:c_off + N], want + bias.double(), bar) <= 1.0
    guard = torch.ones_like(out, dtype=torch.bool)
    guard[1:M + 1, c_off:c_off + N] = False
    assert bool((out[guard] == sentinel).all())


def test_row_block_of_a_concatenated_weight():
    """BERT's q | k | v use: rows d .. 3 d - 1 of the (3 d, d) weight and of its bias into columns d .. of a (rows, 3 d) result"""
    from immtsf import _lib
    dev = _dev()
    M, d = 17, 40
    a, b, bias, want, bar = _case(M, 2 * d, d, "normal")
    got = _product(0, a.to(dev), b.to(dev), bias.to(dev), w_rows=(d, 3 * d))
    assert _worst(got, want + bias.double(), bar) <= 1.0
    assert _lib.load().immtsf_gemm_split_supported(0, M, 2 * d, d, d, d, 3 * d)


def test_two_runs_give_the_same_bits():
    dev = _dev()
    for layout in (0, 1):
        for shape in ((17, 136, 264), (129, 136, 264)):
            a, b, bias, _, _ = _case(*shape, "scaled")
            x, y = (_product(layout, a.to(dev), b.to(dev), bias.to(dev)) for _ in range(2))
            assert torch.equal(x, y)


def test_split_images_equal_the_restatement():
    from immtsf import _lib
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    w = torch.randn(1031, generator=g) * torch.exp2(torch.randint(-30, 31, (1031,), generator=g).float())
    w[:4] = torch.tensor([257.0, 259.0, -65535.0, 0.0])
    want_hi, want_lo = SR.split(w)
    for n, start in ((1031, 0), (1028, 0), (3, 0), (1030, 1)):          # whole vectors + a tail; a tail alone; an unaligned start
        src = w.to(dev)[start:start + n]
        hi, lo = torch.zeros(n + 1, dtype=torch.bfloat16, device=dev), torch.zeros(n + 1, dtype=torch.bfloat16, device=dev)
        _lib.check(_lib.load().immtsf_split_bf16(C.c_void_p(src.data_ptr()), n, _lib.ptr(hi), _lib.ptr(lo), _lib.stream_ptr()), "split_bf16")
        assert torch.equal(hi[:n].cpu().view(torch.int16), want_hi[start:start + n].view(torch.int16)), (n, start)
        assert torch.equal(lo[:n].cpu().view(torch.int16), want_lo[start:start + n].view(torch.int16)), (n, start)
        assert float(hi[n]) == 0.0 and float(lo[n]) == 0.0


def test_unsupported_shapes_are_refused_before_a_launch():
    from immtsf import _lib
    lib = _lib.load()
    dev = _dev()
    M, N, K = 16, 24, 7
    a = torch.randn(M, 8, device=dev)
    hi, lo = _images(torch.randn(N, 8, device=dev))
    out = torch.full((M, N), 3.25, device=dev)
    assert not lib.immtsf_gemm_split_supported(0, M, N, K, 8, 8, N)
    rc = lib.immtsf_gemm_split(0, _lib.ptr(a), 8, _lib.ptr(hi), _lib.ptr(lo), 8, _lib.ptr(out), N, None, M, N, K, _lib.stream_ptr())
    assert rc == EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 3.25).all())
    for bad in ((0, 16, 20, 8, 8, 8, 20), (1, 16, 24, 8, 8, 20, 24), (2, 16, 24, 8, 8, 8, 24), (0, 16, 24, 8, 6, 8, 24), (0, 16, 24, 8, 8, 8, 16)):
        assert not lib.immtsf_gemm_split_supported(*bad), bad
    assert lib.immtsf_gemm_split_supported(0, 1, 8, 8, 8, 8, 8) and lib.immtsf_gemm_split_supported(1, 1, 8, 8, 8, 8, 8)
