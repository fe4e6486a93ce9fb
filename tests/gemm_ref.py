"""Plain restatement of what the GEMM family computes (csrc/gemm.hpp lines 20-23), on the CPU in float64, with no import of the library:

    C[m, n] = act( rowflag( alpha * sum_k opA(m, k) opB(n, k) + bias[n] ) + add_vec[n] )  (* relu mask)  (+ C_old[m, n])

Two instruments are built on it.

EXACT.  Operands from int_operands hold integers of magnitude <= 3 (bf16-exact), alpha is a power of two, bias / add_vec / C_old hold
integers.  Every partial sum of every summation order is then an integer (or a multiple of alpha) below 2^24, which fp32 represents
exactly: the kernel's result is ONE bit pattern whatever its order -- MFMA k-chains, K groups summed through LDS, split-K atomics, a
reduce launch -- and must equal the float64 product element for element (float64 holds these integers exactly, too).  The condition,
|alpha| 9 K + |extras| < 2^24, is headroom(); tests/test_gemm_ref.py checks it for every case of tests/gemm_cases.py.

BOUND.  For real operands, bound() is the per-element worst case of an fp32 accumulation of K exact products in ANY order (Higham,
Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1: |fl(s) - s| <= gamma_{K-1} sum |x_i y_i| whatever the order), with
the unit round-off doubled to 2^-23 so that an accumulator that truncates instead of rounding to nearest still fits, and four more
steps for alpha, the bias, add_vec and the old C: (K + 4) 2^-23 (|alpha| |opA| |opB| + |extra|).  A derivation, not a measurement."""
import collections

import torch

NT, NN, TN = 0, 1, 2
Result = collections.namedtuple("Result", "C bias_grad Ch z")


def int_operands(shape, seed, dtype=torch.float32):
    """integers in [-3, 3], about one entry in eight forced to zero; exact in fp32 and in bf16"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-3, 4, shape, generator=g).float()
    v[torch.rand(shape, generator=g) < 0.125] = 0.0
    return v.to(dtype)


def real_operands(shape, seed):
    """randn as fp32, and the round-to-nearest-even bf16 image (as fp32) that a bf16 kernel must multiply"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(shape, generator=g)
    return v, v.bfloat16().float()


def ops(layout, A, B, a_rowmap=None, rows=None, k=None):
    """op(A) (M, K) and op(B) (K, N) in float64.  a_rowmap: source row of A per logical row (NT / NN).  rows: a device-side row count
    (NT / NN: only the first `rows` logical rows exist).  k: a device-side reduction length (only the first k terms)."""
    A, B = A.double(), B.double()
    if layout == TN:
        assert a_rowmap is None and rows is None
        a, b = A.t(), B
    else:
        a = A if a_rowmap is None else A[a_rowmap.long()]
        if rows is not None:
            a = a[:rows]
        b = B.t() if layout == NT else B
    if k is not None:
        a, b = a[:, :k], b[:k]
    return a, b


def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))


def exact(layout, A, B, alpha=1.0, bias=None, add_vec=None, row_flag=None, row_flag_div=1, c_old=None, act=0, relu_ref=None, a_rowmap=None,
          rows=None, k=None):
    """float64 result C, the TN bias gradient (alpha * column sums of A over the reduction: the kernels scale it like the product), the
    RNE bf16 image of C (what Ch must hold) and the pre-activation z"""
    a, b = ops(layout, A, B, a_rowmap, rows, k)
    z = alpha * (a @ b)
    if bias is not None:
        z = z + bias.double()
    if row_flag is not None:
        live = row_flag.long()[torch.arange(z.shape[0]) // row_flag_div] != 0
        z = z * live[:, None].double()
    if add_vec is not None:
        z = z + add_vec.double()
    c = torch.relu(z) if act == 1 else gelu64(z) if act == 2 else z
    if relu_ref is not None:
        c = torch.where(relu_ref.double()[:c.shape[0]] <= 0, torch.zeros_like(c), c)
    if c_old is not None:
        c = c + c_old.double()[:c.shape[0]]
    bias_grad = alpha * a.sum(1) if layout == TN else None
    return Result(c, bias_grad, c.float().bfloat16(), z)


def bound(opA, opB, alpha, extra, K):
    """per-element bar for real operands: opA (M, K), opB (K, N) as ops() returns them, extra = |bias| + |add_vec| + |C_old| (broadcast)"""
    mag = abs(alpha) * (opA.abs() @ opB.abs())
    if extra is not None:
        mag = mag + extra.double().abs()
    return (K + 4) * 2.0 ** -23 * mag


def headroom(alpha, K, extras=0.0):
    """largest magnitude any partial result of an integer case can reach; exactness needs it below 2^24"""
    return abs(alpha) * 9.0 * K + extras
