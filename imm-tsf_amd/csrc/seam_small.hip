// The forward product of the rank-PW seam between TTF_T2V_XAttn and MMF_XAttn_Add (csrc/xrank.hip, the "_z" form: P = [Z | 1] Wc^T) at
// a few thousand rows.  PW is 24 at cfg2 ((2C + 1) H = 17, pitch 24), so on gemm2's 64 x 64 tiles it filled 24 of 64 tile columns on
// rows / 64 workgroups (profiles/seam_small_rows_summary.md): a few MB of operands and 75 MFLOP that want waves in flight, not tiles.
#include "seam_small.hpp"

namespace {

// ---- forward.  A workgroup owns 16 rows; its four waves split the reduction over d in steps of 32 and meet in LDS.  Both MFMA operand
// fragments of v_mfma_f32_16x16x32_bf16 are eight consecutive reduction elements of one row (of A, of W): one 16-byte load each straight
// from memory, no staging.  NT = ceil(PW / 16) column tiles; columns >= PW read zeros and are not written.
template <int NT>
__global__ __launch_bounds__(256) void seam_p_fwd_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ W, const float* __restrict__ bias,
                                                          float* __restrict__ out, int rows, int d, int PW) {
    __shared__ f32x4 red[3][NT][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int row = blockIdx.x * 16 + fr;
    const bool rok = row < rows;
    const bf16_t* ap = A + (size_t)(rok ? row : 0) * d + fq * 8;
    const bf16_t* wp[NT];
    bool wok[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        wok[j] = j * 16 + fr < PW;
        wp[j] = W + (size_t)(wok[j] ? j * 16 + fr : 0) * d + fq * 8;
    }
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 zero;
#pragma unroll
    for (int e = 0; e < 8; ++e) zero[e] = (bf16_t)0.0f;
    const int nk = d >> 5;
#pragma unroll 4
    for (int ks = wave; ks < nk; ks += 4) {
        const bf16x8 a = rok ? *reinterpret_cast<const bf16x8*>(ap + ks * 32) : zero;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const bf16x8 b = wok[j] ? *reinterpret_cast<const bf16x8*>(wp[j] + ks * 32) : zero;
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[j], 0, 0, 0);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < NT; ++j) red[wave - 1][j][lane] = acc[j];
    }
    __syncthreads();
    if (wave > 0) return;
    // C/D map: column = lane & 15, row = (lane >> 4) * 4 + register
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int w = 0; w < 3; ++w) acc[j] += red[w][j][lane];
        const int n = j * 16 + fr;
        if (n >= PW) continue;
        const float b = bias ? bias[n] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int orow = blockIdx.x * 16 + fq * 4 + r;
            if (orow < rows) out[(size_t)orow * PW + n] = acc[j][r] + b;
        }
    }
}

constexpr int SEAM_MIN_ROWS = 512, SEAM_MAX_ROWS = 8192;      // [min, max): from max on the many-rows paths take over

}  // namespace

bool seam_p_fwd_shape_ok(int rows, int d, int PW) {
    return rows >= SEAM_MIN_ROWS && rows < SEAM_MAX_ROWS && PW >= 1 && PW <= 64 && d >= 32 && d <= 1024 && (d & 31) == 0;
}
bool seam_p_fwd_ok(int rows, int d, int PW, const void* A, const void* W, const void* out) {
    const uintptr_t al = reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(W);
    return seam_p_fwd_shape_ok(rows, d, PW) && (al & 15) == 0 && A && W && out;
}

int launch_seam_p_fwd(const void* A, const void* W, const float* bias, float* out, int rows, int d, int PW, hipStream_t s) {
    if (!seam_p_fwd_ok(rows, d, PW, A, W, out)) return IMMTSF_EUNSUPPORTED;
    const bf16_t* a = static_cast<const bf16_t*>(A);
    const bf16_t* w = static_cast<const bf16_t*>(W);
    const dim3 grid((rows + 15) / 16);
    switch ((PW + 15) / 16) {
        case 1: hipLaunchKernelGGL((seam_p_fwd_kernel<1>), grid, dim3(256), 0, s, a, w, bias, out, rows, d, PW); break;
        case 2: hipLaunchKernelGGL((seam_p_fwd_kernel<2>), grid, dim3(256), 0, s, a, w, bias, out, rows, d, PW); break;
        case 3: hipLaunchKernelGGL((seam_p_fwd_kernel<3>), grid, dim3(256), 0, s, a, w, bias, out, rows, d, PW); break;
        default: hipLaunchKernelGGL((seam_p_fwd_kernel<4>), grid, dim3(256), 0, s, a, w, bias, out, rows, d, PW); break;
    }
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}
