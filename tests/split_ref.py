"""Torch restatement of the split-bf16 product scheme of csrc/gemm_split.hip, and the operands its tests share.
  split:    hi = bf16(w) (round to nearest even), lo = bf16(w - float(hi)); the subtraction is exact in fp32
  product:  a_lo b_hi + a_hi b_lo + a_hi b_hi, in that order; a_lo b_lo is dropped
  bound:    |C - A B| <= (2^-16 + 3 K 2^-24) (|A| |B|) + 1e-30 per element, the bar the kernel's tests hold it to.  bf16 x bf16 is exact
            in fp32 and fp32 accumulation of 3 K terms adds at most 3 K 2^-24.  The cut itself guarantees 2^-17 per operand (a mantissa
            just above a power of two) and 2^-16 for the dropped term, 2^-15 in the worst case; typical operands sit near 2^-18 each and
            the terms of a sum carry random signs, so the sums stay inside 2^-16 -- tests/test_split_ref.py shows it, in float64, for
            every operand set the GPU tests use."""
import torch


def split(w):
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    return hi, lo


def product3(a, b, dtype=torch.float32):
    """a (M, K) b (K, N) by the three kept terms, each term and the sums in `dtype` (float64: the exact value of what the kernel adds up)"""
    ah, al = (t.to(dtype) for t in split(a))
    bh, bl = (t.to(dtype) for t in split(b))
    return al @ bh + ah @ bl + ah @ bh


def bound(a, b):
    """the per-element bar for a (M, K) b (K, N), float64"""
    K = a.shape[1]
    return (2.0 ** -16 + 3 * K * 2.0 ** -24) * (a.double().abs() @ b.double().abs()) + 1e-30


def operands(M, N, K, kind, seed=0):
    """(a (M, K), b (K, N), bias (N)) fp32.  "normal": N(0, 1) everywhere; "scaled": the rows of a and the columns of b (the rows of the
    weight) times 2^u, u uniform in [-6, 6]: a 2^12 spread of row scales.  The bar has no term for the fp32 rounding of the sum with the
    bias, 2^-24 |C|, so the bias stays at the scale of the smallest products of its column: N(0, 1) times the column's scale times 2^-6,
    the smallest row scale; the rounding is then at most a few 2^-24 (|A| |B|), far inside the 2^-16"""
    g = torch.Generator().manual_seed(1000 * seed + 97 * M + 13 * N + K + (5 if kind == "scaled" else 0))
    a, b, bias = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g), torch.randn(N, generator=g)
    if kind == "scaled":
        a = a * torch.exp2(torch.rand(M, 1, generator=g) * 12 - 6)
        sb = torch.exp2(torch.rand(1, N, generator=g) * 12 - 6)
        b, bias = b * sb, bias * sb.view(N) * 2.0 ** -6
    return a, b, bias


def int_operands(M, N, K):
    """(a (M, K), b (K, N)) of integers |x| <= 300 as fp32: odd values past 256 need a non-zero lo; both are asymmetric, so a transposed
    or row / column-swapped read or write cannot reproduce the product"""
    m, n, k = torch.arange(M).view(M, 1), torch.arange(N).view(1, N), torch.arange(K)
    a = ((5 * m + 11 * k.view(1, K)) % 601 - 300).float()
    b = ((7 * n + 3 * k.view(K, 1)) % 601 - 300).float()
    return a, b
