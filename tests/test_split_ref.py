"""CPU checks of tests/split_ref.py, the torch restatement of the split-bf16 product (csrc/gemm_split.hip): the cut keeps 17
bits, 16-bit integers split exactly, and the three kept terms, summed exactly, stay inside the bar of tests/test_gpu_gemm_split.py on the
operands that file uses -- the reference alone does not eat the bar."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref as SR  # noqa: E402

SHAPES = [(M, N, K) for M in (1, 15, 16, 17, 129) for N in (8, 24, 136) for K in (8, 40, 264)] + [(32, 136, 264), (33, 136, 264), (2049, 1928, 72)]


def test_the_cut_keeps_seventeen_bits():
    g = torch.Generator().manual_seed(3)
    w = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-40, 41, (1 << 16,), generator=g).float())
    w = torch.cat([w, torch.tensor([1.0, -1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, 257.0, 3.0e38, 1.5e-30])])
    hi, lo = SR.split(w)
    assert hi.dtype == lo.dtype == torch.bfloat16
    err = (w.double() - hi.double() - lo.double()).abs()
    assert bool((err <= 2.0 ** -17 * w.double().abs()).all()), float((err / w.double().abs()).max())
    # the residue the second cut sees is exact in fp32: hi + (w - hi) gives w back
    assert torch.equal(hi.float() + (w - hi.float()), w)


def test_sixteen_bit_integers_split_exactly():
    x = torch.arange(-65535, 65536, dtype=torch.float32)
    hi, lo = SR.split(x)
    assert torch.equal(hi.float() + lo.float(), x)
    h, l = SR.split(torch.tensor([257.0, 259.0, 300.0, 65535.0]))
    assert h.tolist() == [256.0, 260.0, 300.0, 65536.0] and l.tolist() == [1.0, -1.0, 0.0, -1.0]
    assert int((lo != 0).sum()) > 60000          # most of them need the second image


@pytest.mark.parametrize("kind", ["normal", "scaled"])
def test_three_terms_stay_inside_the_bar(kind):
    worst = 0.0
    for M, N, K in SHAPES:
        a, b, _ = SR.operands(M, N, K, kind)
        exact = a.double() @ b.double()
        ratio = float(((SR.product3(a, b, torch.float64) - exact).abs() / SR.bound(a, b)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (M, N, K, ratio)
    print(f"{kind}: three kept terms in float64, worst error / bar {worst:.3f}")
    # (worst case of the scheme: 2^-17 per operand and 2^-16 for the dropped term, 2^-15 together, twice the bar; the terms of a sum carry
    # random signs, and on these operands the short sums, K = 8, come closest: 0.74 of the bar on the normal set, 0.96 on the scaled one)


def test_integer_operands_and_their_dropped_term():
    """|x| <= 300, K <= 64: every product and partial sum is an integer below 2^24, so fp32 adds them exactly; the three kept terms are
    the int64 product less the int64 product of the two lo images, and equal the int64 product wherever one side has no lo"""
    a, b = SR.int_operands(129, 136, 64)
    assert float(a.abs().max()) <= 300 and float(b.abs().max()) <= 300
    (_, al), (_, bl) = SR.split(a), SR.split(b)
    assert int((al != 0).sum()) > a.numel() // 25 and int((bl != 0).sum()) > b.numel() // 25
    full = a.long() @ b.long()
    kept = full - al.float().long() @ bl.float().long()
    assert int((a.abs().long() @ b.abs().long()).max()) < 2 ** 24
    assert not torch.equal(b[:64, :64], b[:64, :64].t()) and not torch.equal(full[:129, :129], full[:129, :129].t())
    assert torch.equal(SR.product3(a, b, torch.float32).long(), kept)
    assert torch.equal(SR.product3(a, b, torch.float64).long(), kept)
    even_a = 2 * (a / 2).trunc()
    assert int((SR.split(even_a)[1] != 0).sum()) == 0
    assert torch.equal(SR.product3(even_a, b, torch.float32).long(), even_a.long() @ b.long())
