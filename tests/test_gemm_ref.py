"""The GEMM reference (tests/gemm_ref.py) and the case table (tests/gemm_cases.py) checked on the CPU: the table's integer cases have the
headroom exactness needs, `exact` equals a hand-written triple loop, and `bound` holds for an fp32 accumulation in a scrambled order."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as T      # noqa: E402
import gemm_ref as R        # noqa: E402


def test_integer_cases_have_headroom_and_consistent_grids():
    """|alpha| 9 K + |extras| < 2^24 for every case (operands are integers of magnitude <= 3): every partial sum is exact in fp32, so no
    GPU case can fail for lack of headroom, and every result is finite: its bf16 image is defined.  alpha is a power of two."""
    ids = [c["id"] for c in T.CASES]
    assert len(ids) == len(set(ids))
    for c in T.CASES:
        o = c["opt"]
        alpha = o.get("alpha", 1.0)
        assert math.frexp(alpha)[0] == 0.5, c["id"]
        assert R.headroom(alpha, c["K"], T.extras(o)) < 2 ** 24, c["id"]
        if c["tile"]:
            assert c["grid"] == T.cdiv(c["M"], c["tile"][0]) * T.cdiv(c["N"], c["tile"][1]) * c["splits"] * c["block"], c["id"]
        assert c["why"]
    for members in T.GROUPS.values():
        for M, N, K in members:
            assert R.headroom(1.0, K) < 2 ** 24
    for M, N, K in list(T.LINEAR_SMALL) + list(T.LINEAR_GEMM):
        assert R.headroom(1.0, max(M, N, K), 3.0) < 2 ** 24
    assert R.headroom(1.0, 3 * T.LINEAR_BF16["N"]) < 2 ** 24
    v = R.int_operands((64, 64), 1)
    assert float(v.abs().max()) == 3.0 and torch.equal(v, v.round()) and torch.equal(v.bfloat16().float(), v)
    assert 0.05 < float((v == 0).float().mean()) < 0.40


def test_exact_against_a_triple_loop_with_every_option():
    M, N, K = 3, 4, 5
    for layout in (R.NT, R.NN, R.TN):
        A = R.int_operands((K, M) if layout == R.TN else (M + 2, K), 10 + layout)
        B = R.int_operands((N, K) if layout == R.NT else (K, N), 20 + layout)
        bias, add_vec = R.int_operands((N,), 30), R.int_operands((N,), 31)
        c_old, relu_ref = R.int_operands((M, N), 32), R.int_operands((M, N), 33)
        flag = torch.tensor([1, 0], dtype=torch.int32)
        rowmap = None if layout == R.TN else torch.tensor([4, 0, 4], dtype=torch.int32)
        kk, alpha = 4, 0.5
        for act in (0, 1, 2):
            got = R.exact(layout, A, B, alpha, bias, add_vec, flag, 2, c_old, act, relu_ref, rowmap, None if layout == R.TN else M, kk)
            for m in range(M):
                for n in range(N):
                    s = 0.0
                    for k in range(kk):
                        a = float(A[k, m]) if layout == R.TN else float(A[int(rowmap[m]), k])
                        b = float(B[n, k]) if layout == R.NT else float(B[k, n])
                        s += a * b
                    z = alpha * s + float(bias[n])
                    if int(flag[m // 2]) == 0:
                        z = 0.0
                    z += float(add_vec[n])
                    c = max(z, 0.0) if act == 1 else 0.5 * z * (1.0 + math.erf(z / math.sqrt(2.0))) if act == 2 else z
                    if float(relu_ref[m, n]) <= 0:
                        c = 0.0
                    c += float(c_old[m, n])
                    assert abs(float(got.C[m, n]) - c) <= 1e-14 * max(1.0, abs(c)), (layout, act, m, n)
                    assert act == 2 or float(got.Ch[m, n]) == float(torch.tensor(c, dtype=torch.float32).bfloat16())
            if layout == R.TN:
                for m in range(M):
                    assert float(got.bias_grad[m]) == alpha * sum(float(A[k, m]) for k in range(kk))


def test_bound_holds_for_a_permuted_fp32_accumulation():
    """the reference stays inside its own bar: products summed in fp32, one term at a time, in a scrambled order"""
    rng = np.random.default_rng(0)
    for K in (136, 16384):
        M, N = 6, 5
        _, a = R.real_operands((M, K), K)
        _, b = R.real_operands((K, N), K + 1)
        bias = torch.randn(N, generator=torch.Generator().manual_seed(2))
        ref = a.double() @ b.double() + bias.double()
        bar = R.bound(a.double(), b.double(), 1.0, bias, K)
        perm = rng.permutation(K)
        prod = (a.numpy()[:, perm, None] * b.numpy()[perm][None, :, :]).astype(np.float32)      # exact: 16 significant bits
        acc = np.zeros((M, N), np.float32)
        for k in range(K):
            acc = (acc + prod[:, k, :]).astype(np.float32)
        acc = (acc + bias.numpy()).astype(np.float32)
        err = np.abs(acc.astype(np.float64) - ref.numpy())
        assert (err <= bar.numpy()).all(), (K, float((err / bar.numpy()).max()))
