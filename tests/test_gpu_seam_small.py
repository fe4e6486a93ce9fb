"""The rank-PW seam's small-row kernels (csrc/seam_small.hip, layernorm_bwd_lr_kernel's launch rule below 8192 rows) against the same
formulas in float64 on the CPU, computed from the very inputs the kernels get (bf16 operands rounded first, then widened).

No tolerance is fixed in advance.  Each case runs the form these shapes took before -- gemm2's tiles (immtsf_gemm_bf16) for the
forward product, one row per wave (form 1) for the LayerNorm backward -- on the same inputs and measures its largest absolute error against
float64; the small-row kernel must stay within twice that plus one ulp of the output type at the output's largest magnitude (fp32:
2^-23, bf16: 2^-7 of max |reference|).  The factor two covers a different summation order and nothing else: operands, operand precision
and accumulator width are the same on both sides.  Every case prints both errors."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "imm-tsf_amd")]
pytestmark = pytest.mark.gpu

EUNSUPPORTED = -3
ULP = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _lib_():
    from immtsf import _lib
    from immtsf.ops import ptr, stream_ptr
    return _lib, _lib.load(), ptr, stream_ptr


def _err(out, ref64):
    return float((out.detach().cpu().double() - ref64).abs().max())


def _bound(what, new, old, ref64, dtype):
    """prints both errors, then: new <= 2 old + one ulp of the output type at the output's largest magnitude"""
    e_new, e_old = _err(new, ref64), _err(old, ref64)
    ulp = ULP[dtype] * float(ref64.abs().max())
    print(f"  {what}: before {e_old:.3e}  small-row {e_new:.3e}  (ulp {ulp:.3e})")
    assert e_new <= 2.0 * e_old + ulp, (what, e_new, e_old, ulp)


@pytest.mark.parametrize("PW", [24, 40])
@pytest.mark.parametrize("d", [256, 768, 1024])
@pytest.mark.parametrize("rows", [512, 520, 2048])
def test_p_product_vs_float64(rows, d, PW):
    """P = A W^T + bias on bf16 operands: the skinny kernel against gemm2's 64 x 64 tiles, both against float64."""
    dev = _dev()
    _lib, lib, ptr, stream_ptr = _lib_()
    torch.manual_seed(rows + d + PW)
    A = torch.randn(rows, d, device=dev).bfloat16().contiguous()
    W = (torch.randn(PW, d, device=dev) / d ** 0.5).bfloat16().contiguous()
    bias = torch.randn(PW, device=dev)
    ref = A.cpu().double() @ W.cpu().double().t() + bias.cpu().double()
    assert lib.immtsf_seam_route(rows, d, PW) == 1
    old = torch.full((rows, PW), 7.0, device=dev)
    _lib.check(lib.immtsf_gemm_bf16(0, ptr(A), d, ptr(W), d, ptr(old), PW, None, PW, ptr(bias), None, rows, PW, d, 1.0, 0, 0, None, 0, None,
                                    stream_ptr()), "gemm_bf16")
    new = torch.full((rows + 1, PW), 7.0, device=dev)         # (one row of canaries behind the result)
    _lib.check(lib.immtsf_seam_p_bf16(ptr(A), ptr(W), ptr(bias), ptr(new), rows, d, PW, stream_ptr()), "seam_p_bf16")
    torch.cuda.synchronize()
    assert bool((new[rows] == 7.0).all())
    _bound(f"P rows={rows} d={d} PW={PW}", new[:rows], old, ref, torch.float32)


@pytest.mark.parametrize("rows", [1, 33])
def test_few_rows_stay_on_gemm2(rows):
    """below 512 rows the product stays on the GEMM family: the route says so and the small-row entry refuses the shape"""
    dev = _dev()
    _lib, lib, ptr, stream_ptr = _lib_()
    d, PW = 768, 24
    assert lib.immtsf_seam_route(rows, d, PW) == 0
    A = torch.randn(rows, d, device=dev).bfloat16()
    W = torch.randn(PW, d, device=dev).bfloat16()
    out = torch.zeros(rows, PW, device=dev)
    assert lib.immtsf_seam_p_bf16(ptr(A), ptr(W), None, ptr(out), rows, d, PW, stream_ptr()) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


def _keep_words(keep, windows, T, d):
    """the forward's export of a dropout site's keep bits (t2v_mix_ln_fwd_kernel): word ((w * 2 + t / 16) * 256 + q) holds, at bits
    4 (t % 16) .. + 3, the keep bits of the four elements of column chunk q of row w * T + t"""
    k = keep.view(windows, T, d // 4, 4).to(torch.int64)
    nib = k[..., 0] | (k[..., 1] << 1) | (k[..., 2] << 2) | (k[..., 3] << 3)          # (windows, T, d / 4)
    words = torch.zeros(windows, 2, 256, dtype=torch.int64)
    for t in range(T):
        words[:, t // 16, :d // 4] |= nib[:, t] << (4 * (t % 16))
    return words.contiguous()


_LN_CASES = [(0.0, 8), (0.25, 8), (0.25, 32)]        # (p, T): dropout off; on through exported keep words with T = 8 and 32


@pytest.mark.parametrize("dxmode", ["f32", "bf16", "both"])
@pytest.mark.parametrize("xh_bf16", [False, True])
@pytest.mark.parametrize("d", [256, 768, 1024])
@pytest.mark.parametrize("p,T", _LN_CASES)
def test_layernorm_backward_lowrank_vs_float64(p, T, d, xh_bf16, dxmode):
    """dx (fp32 and / or bf16) and the three column sums of the low-rank LayerNorm backward, product rule (two rows per wave) against
    one row per wave, both against float64.  rows = 65 x 8 = 520 or 17 x 32 = 544: no multiple of every rows-per-workgroup choice."""
    dev = _dev()
    _lib, lib, ptr, stream_ptr = _lib_()
    PW = 24
    windows = 65 if T == 8 else 17
    rows = windows * T
    gen = torch.Generator().manual_seed(rows + d + int(100 * p) + 2 * xh_bf16)
    G = torch.randn(rows, PW, generator=gen)
    Wb = torch.randn(PW, d, generator=gen) / PW ** 0.5
    gamma = 1.0 + 0.1 * torch.randn(d, generator=gen)
    x = torch.randn(rows, d, generator=gen)
    xhat = (x - x.mean(1, keepdim=True)) / x.std(1, unbiased=False, keepdim=True)
    rstd = 0.5 + torch.rand(rows, generator=gen)
    flag = (torch.rand(windows, generator=gen) > 0.3).to(torch.uint8)
    flag[0], flag[1] = 1, 0
    keep = (torch.rand(rows, d, generator=gen) >= p) if p > 0 else torch.ones(rows, d, dtype=torch.bool)
    xh16 = xhat.bfloat16()
    h = (xh16 if xh_bf16 else xhat).double()
    # float64 reference
    y = (G.double() @ Wb.double()) * keep.double() * (float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))) if p > 0 else 1.0)
    tv = y * gamma.double()
    c1 = tv.mean(1, keepdim=True)
    c2 = (tv * h).mean(1, keepdim=True)
    o = rstd.double()[:, None] * (tv - c1 - h * c2)
    ref_gw, ref_gb, ref_q = (y * h).sum(0), y.sum(0), o.sum(0)
    ref_dx = o * flag.double().repeat_interleave(T)[:, None]

    dG, dWb, dgamma, drstd, dflag = (t.to(dev).contiguous() for t in (G, Wb, gamma, rstd, flag))
    dxhat = None if xh_bf16 else xhat.to(dev).contiguous()
    dxh16 = xh16.to(dev).contiguous() if xh_bf16 else None
    kw = _keep_words(keep, windows, T, d).to(dev) if p > 0 else None
    scratch = torch.empty(256 * 3 * d, device=dev)

    def run(form):
        dx = torch.full((rows + 1, d), 7.0, device=dev) if dxmode in ("f32", "both") else None
        dxh = torch.full((rows + 1, d), 7.0, dtype=torch.bfloat16, device=dev) if dxmode in ("bf16", "both") else None
        sums = torch.full((3, d), 7.0, device=dev)
        _lib.check(lib.immtsf_layernorm_backward_lowrank(ptr(dG), PW, PW, ptr(dWb), rows, d, ptr(dgamma), ptr(dxhat), ptr(dxh16), ptr(drstd),
                                                         ptr(dx), ptr(dxh), p, ptr(kw), T, ptr(dflag), T, ptr(sums[0]), ptr(sums[1]),
                                                         ptr(sums[2]), ptr(scratch), scratch.numel() * 4, form, stream_ptr()),
                   "layernorm_backward_lowrank")
        torch.cuda.synchronize()
        for t in (dx, dxh):
            assert t is None or bool((t[rows] == 7.0).all())
        return dx, dxh, sums

    old, new = run(1), run(0)
    tag = f"LN p={p} T={T} d={d} xhat={'bf16' if xh_bf16 else 'f32'} dx={dxmode}"
    if new[0] is not None:
        _bound(tag + " dx", new[0][:rows], old[0][:rows], ref_dx, torch.float32)
    if new[1] is not None:
        _bound(tag + " dx bf16", new[1][:rows], old[1][:rows], ref_dx, torch.bfloat16)
    for i, (name, ref) in enumerate((("dgamma", ref_gw), ("dbeta", ref_gb), ("dxsum", ref_q))):
        _bound(tag + " " + name, new[2][i], old[2][i], ref, torch.float32)
