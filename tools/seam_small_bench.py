#!/usr/bin/env python3
"""The seam's small-row kernels beside what these shapes ran before, at d = 768, PW = 24 over a sweep of row counts: the forward
product P = A W^T + bias on gemm2's tiles (immtsf_gemm_bf16) against the skinny kernel (csrc/seam_small.hip), and the low-rank LayerNorm
backward with one row per wave (form 1) against the product rule (form 0).  50 launches per hipGraph (bench.graph_kernel_us).
usage: seam_small_bench.py [rows ...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "imm-tsf_amd")]
import torch  # noqa: E402
import bench  # noqa: E402


def main():
    from immtsf import _lib
    from immtsf.ops import ptr, stream_ptr
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    d, PW, T = 768, 24, 32
    sweep = [int(a) for a in sys.argv[1:]] or [512, 1024, 2048, 4096, 8160, 16384]
    print("rows    P gemm2  P skinny | LN 1 row/wave  LN rule   (us per call)")
    for rows in sweep:
        torch.manual_seed(rows)
        A = torch.randn(rows, d, device=dev).bfloat16()
        W = torch.randn(PW, d, device=dev).bfloat16()
        bias = torch.randn(PW, device=dev)
        P = torch.empty(rows, PW, device=dev)

        def p_old():
            _lib.check(lib.immtsf_gemm_bf16(0, ptr(A), d, ptr(W), d, ptr(P), PW, None, PW, ptr(bias), None, rows, PW, d, 1.0, 0, 0, None, 0, None,
                                            stream_ptr()), "gemm_bf16")

        def p_new():
            _lib.check(lib.immtsf_seam_p_bf16(ptr(A), ptr(W), ptr(bias), ptr(P), rows, d, PW, stream_ptr()), "seam_p")

        Gf, Wb = torch.randn(rows, PW, device=dev), torch.randn(PW, d, device=dev)
        gamma, xhat, rstd = torch.ones(d, device=dev), torch.randn(rows, d, device=dev), torch.ones(rows, device=dev)
        dx, dxh = torch.empty(rows, d, device=dev), torch.empty(rows, d, dtype=torch.bfloat16, device=dev)
        kw = torch.randint(-2 ** 62, 2 ** 62, (rows // T, 2, 256), dtype=torch.int64, device=dev)
        flag = torch.ones(rows // T, dtype=torch.uint8, device=dev)
        sums, scr = torch.empty(3, d, device=dev), torch.empty(256 * 3 * d, device=dev)

        def ln(form):
            _lib.check(lib.immtsf_layernorm_backward_lowrank(ptr(Gf), PW, PW, ptr(Wb), rows, d, ptr(gamma), ptr(xhat), None, ptr(rstd), ptr(dx),
                                                             ptr(dxh), 0.1, ptr(kw), T, ptr(flag), T, ptr(sums[0]), ptr(sums[1]), ptr(sums[2]),
                                                             ptr(scr), scr.numel() * 4, form, stream_ptr()), "ln_lr")

        small = lib.immtsf_seam_route(rows, d, PW) == 1
        t = [bench.graph_kernel_us(p_old), bench.graph_kernel_us(p_new) if small else float("nan"), bench.graph_kernel_us(lambda: ln(1)),
             bench.graph_kernel_us(lambda: ln(0))]
        print("%5d  %8.2f  %8.2f | %13.2f  %7.2f" % (rows, *t), flush=True)


if __name__ == "__main__":
    main()
