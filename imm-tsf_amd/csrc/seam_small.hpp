// The forward product that crosses the low-rank seam (csrc/xrank.hip, the "_z" form) at small row counts: see seam_small.hip
#pragma once
#include "common.hpp"

// out (rows x PW fp32, row pitch PW) = A (rows x d bf16) W (PW x d bf16)^T + bias (PW, may be null).
// applies: 512 <= rows < 8192, PW <= 64, 32 | d, d <= 1024, 16-byte aligned operands (else the caller stays on immtsf_launch_gemm)
bool seam_p_fwd_shape_ok(int rows, int d, int PW);
bool seam_p_fwd_ok(int rows, int d, int PW, const void* A, const void* W, const void* out);
int launch_seam_p_fwd(const void* A, const void* W, const float* bias, float* out, int rows, int d, int PW, hipStream_t s);
