"""GPU checks of immtsf_gemm_asplit (csrc/gemm_split.hip with the Blo image absent): an fp32 activation cut in registers against a weight
that is STORED in bf16, exactly, on integer operands.
A holds integers in [-300, 300] as fp32: values such as 257 are not bf16 numbers, so a_lo is exercised, and hi + lo is exact below 2^16.
B holds integers in [-8, 8] as bf16 (exact).  K <= 200, so every partial sum stays below 300 * 8 * 200 < 2^24 and every fp32 sum is exact:
C must EQUAL the float64 product, with and without an integer bias, whatever the summation order.
Shapes (M, N, K), both layouts: (1, 8, 8); (17, 72, 200) the 16 x 64 tile, ragged N, K no multiple of 64; (33, 136, 72) the 64 x 64 tile;
(2041, 2048, 72): 16 x 16 = 256 tiles of 128 x 128, the first size on the 128 x 128 kernel."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
SHAPES = [(1, 8, 8), (17, 72, 200), (33, 136, 72), (2041, 2048, 72)]
EUNSUPPORTED = -3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _adr(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off * t.element_size())


@functools.lru_cache(maxsize=None)
def _operands(layout, M, N, K):
    """(A fp32 (M, K), B bf16 (N, K) | (K, N), bias fp32 (N), the float64 product (M, N)) on the host, made once"""
    g = torch.Generator().manual_seed(1000 * layout + M + 3 * N + 7 * K)
    A = torch.randint(-300, 301, (M, K), generator=g).float()
    B = torch.randint(-8, 9, (N, K) if layout == 0 else (K, N), generator=g).float()
    bias = torch.randint(-50, 51, (N,), generator=g).float()
    if K >= 8:
        A[0, :4] = torch.tensor([257.0, -259.0, 300.0, 129.0])          # not bf16 numbers: the low part carries them
    want = A.double() @ (B.double().T if layout == 0 else B.double())
    return A, B.to(torch.bfloat16), bias, want


def _asplit(layout, A, lda, B, ldb, Cm, ldc, bias, M, N, K, a_off=0, b_off=0, c_off=0):
    from immtsf import _lib
    lib = _lib.load()
    return lib.immtsf_gemm_asplit(layout, _adr(A, a_off), lda, _adr(B, b_off), ldb, _adr(Cm, c_off), ldc, _adr(bias), M, N, K, _lib.stream_ptr())


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_exact_on_integer_operands(layout, M, N, K):
    from immtsf import _lib
    dev = _dev()
    A, B, bias, want = _operands(layout, M, N, K)
    A, B, bias = A.to(dev), B.to(dev), bias.to(dev)
    ldb = K if layout == 0 else N
    assert _lib.load().immtsf_gemm_asplit_supported(layout, M, N, K, K, ldb, N)
    for b, ref in ((None, want), (bias, want + bias.double().cpu())):
        out = torch.full((M, N), -7.0, device=dev)
        assert _asplit(layout, A, K, B, ldb, out, N, b, M, N, K) == 0
        assert torch.equal(out.double().cpu(), ref)
    again = torch.full((M, N), -7.0, device=dev)
    assert _asplit(layout, A, K, B, ldb, again, N, bias, M, N, K) == 0
    assert torch.equal(again, out)                               # two runs: the same bits


@pytest.mark.parametrize("layout", [0, 1])
def test_pitches_a_weight_block_and_a_column_offset_into_a_wider_result(layout):
    """lda, ldb, ldc longer than the rows; the weight is a block of a larger one (rows 8 .. of a layout-0 weight, columns 16 .. of a layout-1
    weight); the result goes to columns 8 .. 8 + N - 1 of a wider C whose other columns keep their sentinel"""
    dev = _dev()
    M, N, K = 33, 72, 104
    A, B, bias, want = _operands(layout, M, N, K)
    lda, ldc, c_off = K + 4, N + 24, 8
    Ap = torch.full((M, lda), 999.0, device=dev)
    Ap[:, :K] = A.to(dev)
    if layout == 0:
        ldb, b_off = K + 8, 8 * (K + 8)
        Bp = torch.full((N + 8, ldb), 5.0, dtype=torch.bfloat16, device=dev)
        Bp[8:, :K] = B.to(dev)
    else:
        ldb, b_off = N + 32, 16
        Bp = torch.full((K, ldb), 5.0, dtype=torch.bfloat16, device=dev)
        Bp[:, 16:16 + N] = B.to(dev)
    out = torch.full((M, ldc), -7.0, device=dev)
    assert _asplit(layout, Ap, lda, Bp, ldb, out, ldc, bias.to(dev), M, N, K, b_off=b_off, c_off=c_off) == 0
    got = out.double().cpu()
    assert torch.equal(got[:, c_off:c_off + N], want + bias.double())
    assert bool((got[:, :c_off] == -7.0).all()) and bool((got[:, c_off + N:] == -7.0).all())


def test_outside_the_support_set_nothing_is_launched():
    from immtsf import _lib
    lib = _lib.load()
    dev = _dev()
    M = 9
    for layout in (0, 1):
        assert not lib.immtsf_gemm_asplit_supported(layout, M, 16, 12, 12, 12 if layout == 0 else 16, 16)       # K = 12
        assert not lib.immtsf_gemm_asplit_supported(layout, M, 12, 16, 16, 16 if layout == 0 else 12, 12)       # N = 12
        assert lib.immtsf_gemm_asplit_supported(layout, M, 16, 16, 16, 16, 16)
        for N, K in ((16, 12), (12, 16)):
            A = torch.ones(M, K, device=dev)
            B = torch.ones((N, K) if layout == 0 else (K, N), dtype=torch.bfloat16, device=dev)
            out = torch.full((M, N), -7.0, device=dev)
            assert _asplit(layout, A, K, B, K if layout == 0 else N, out, N, None, M, N, K) == EUNSUPPORTED
            assert bool((out == -7.0).all())
        # a supported shape behind a misaligned pointer: A one float (4 bytes) in, then the weight one element (2 bytes) in
        A = torch.ones(M * 16 + 8, device=dev)
        B = torch.ones(16 * 16 + 8, dtype=torch.bfloat16, device=dev)
        out = torch.full((M, 16), -7.0, device=dev)
        assert _asplit(layout, A, 16, B, 16, out, 16, None, M, 16, 16, a_off=1) == EUNSUPPORTED
        assert _asplit(layout, A, 16, B, 16, out, 16, None, M, 16, 16, b_off=1) == EUNSUPPORTED
        assert bool((out == -7.0).all())
        assert _asplit(layout, A, 16, B, 16, out, 16, None, M, 16, 16) == 0
        assert bool((out == 16.0).all())
