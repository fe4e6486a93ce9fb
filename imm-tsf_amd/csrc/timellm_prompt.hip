// TimeLLM's prompt statistics (reference models/TimeLLM.py:167-194, here models/TimeLLM.py _get_prompt) as ONE launch for the whole batch:
// a workgroup per window, the window's (L, C) tile staged in LDS once, one packed row of 3 C + 1 floats and top_k int32 per window, so
// that a single device-to-host copy brings every number the prompt text spells.  All fp32.
//
//   min / max:  per channel, a thread walks the channel in time order with strict comparisons, so among elements that compare equal
//               (-0.0 and 0.0) the one of lowest time index stays; a NaN in the channel gives that NaN (the first one).
//   median:     torch's lower median, the element of sorted position (L - 1) / 2, by rank counting -- rank_t = #{j : x_j < x_t or
//               (x_j == x_t and j < t)}, a strict order, so exactly one element has that rank; no sort.  NaN in the channel gives NaN.
//   trend:      per channel the differences x[t] - x[t-1] summed in time order (the same thread's walk), then the channels summed in
//               index order and divided by C.  The FLOAT is written; the host takes > 0.  0 at L == 1.
//   lags:       corr[tau] = (sum_c sum_t x[t, c] x[(t + tau) mod L, c]) / C directly (no FFT) for tau <= L / 2 only -- an aligned group of
//               CP lanes (CP the power of two >= C) per lag, a lane per channel, t in order, the group folded in a fixed tree -- and
//               mirrored bit for bit into corr[L - tau].  The min(top_k, L) largest by rank counting with ties to the lower lag (NaN counts
//               as -inf), descending; entries past L repeat the last lag.
//
// No atomics: every output word has one writer and every sum a fixed order, so two runs give the same bits.
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

constexpr int TP_THREADS = 256;
constexpr int TP_MAX_L = 2048, TP_MAX_C = 64, TP_MAX_K = 64, TP_MAX_TILE = 16384;      // the limits immtsf_timellm_prompt_supported reports
// LDS at the limits: tile 64 KB + corr 8 KB + per-channel flags and sums 512 B = 72.5 KB of the 160 KB

__host__ __device__ __forceinline__ int tp_pad4(int n) { return (n + 3) & ~3; }
inline size_t tp_lds_bytes(int L, int C) { return sizeof(float) * (size_t)(tp_pad4(L * C) + tp_pad4(L) + 2 * TP_MAX_C); }

// grid (B): out row b = [min (C) | max (C) | median (C) | trend | lags (K, int32)]
__global__ __launch_bounds__(TP_THREADS) void timellm_prompt_kernel(int L, int C, int K, int CP, int vec, const float* __restrict__ x,
                                                                    float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float tp_lds[];
    float* tile = tp_lds;                            // [L][C]
    float* corr = tile + tp_pad4(L * C);             // [L]
    float* chsum = corr + tp_pad4(L);                // [C] the channel's summed differences
    int* hasnan = reinterpret_cast<int*>(chsum + TP_MAX_C);      // [C]
    const int tid = threadIdx.x, n = L * C;
    const float* xb = x + (size_t)blockIdx.x * n;
    float* row = out + (size_t)blockIdx.x * (3 * C + 1 + K);
    int* lags = reinterpret_cast<int*>(row + 3 * C + 1);
    if (vec) {      // n % 4 == 0 and x 16-byte aligned (the host checked)
        for (int e = tid; e < (n >> 2); e += TP_THREADS)
            reinterpret_cast<f32x4*>(tile)[e] = reinterpret_cast<const f32x4*>(xb)[e];
    } else {
        for (int e = tid; e < n; e += TP_THREADS) tile[e] = xb[e];
    }
    __syncthreads();
    // ---- per channel: min, max, the first NaN, the summed differences; a thread per channel, time order ----
    if (tid < C) {
        const float* xc = tile + tid;
        float mn = xc[0], mx = mn, prev = mn, sum = 0.f, nanv = mn;
        bool nan = mn != mn;
        for (int t = 1; t < L; ++t) {
            const float v = xc[t * C];
            if (v < mn) mn = v;      // strict: the first of equal elements stays
            if (v > mx) mx = v;
            if (v != v && !nan) { nan = true; nanv = v; }
            sum += v - prev;
            prev = v;
        }
        row[tid] = nan ? nanv : mn;
        row[C + tid] = nan ? nanv : mx;
        if (nan) row[2 * C + tid] = nanv;
        hasnan[tid] = nan ? 1 : 0;
        chsum[tid] = sum;
    }
    // ---- corr[tau], tau <= L / 2: CP lanes per lag; every lane of a wave takes every group_sum (the trip count is block-uniform) ----
    {
        const int G = TP_THREADS / CP, g = tid / CP, c = tid - g * CP, nl = L / 2 + 1;
        const float* xc = tile + c;
        for (int t0 = 0; t0 < nl; t0 += G) {
            const int tau = t0 + g;
            float a = 0.f;
            if (tau < nl && c < C) {
                int t = 0;
                for (; t < L - tau; ++t) a = fmaf(xc[t * C], xc[(t + tau) * C], a);
                for (; t < L; ++t) a = fmaf(xc[t * C], xc[(t + tau - L) * C], a);
            }
            a = group_sum(a, CP) / (float)C;
            if (tau < nl && c == 0) {
                a = a == a ? a : -INFINITY;
                corr[tau] = a;
                if (tau > 0) corr[L - tau] = a;      // (tau == L - tau at the middle lag of an even L: the same word, the same value)
            }
        }
    }
    __syncthreads();
    // ---- median: the element of rank (L - 1) / 2 in its channel ----
    const int mid = (L - 1) >> 1;
    for (int e = tid; e < n; e += TP_THREADS) {
        const int t = e / C, c = e - t * C;
        if (hasnan[c]) continue;
        const float v = tile[e];
        const float* xc = tile + c;
        int r = 0;
        for (int j = 0; j < L; ++j) {
            const float o = xc[j * C];
            r += (o < v || (o == v && j < t)) ? 1 : 0;
        }
        if (r == mid) row[2 * C + c] = v;
    }
    // ---- the min(K, L) largest corr, descending, ties to the lower lag ----
    const int kk = min(K, L);
    for (int tau = tid; tau < L; tau += TP_THREADS) {
        const float v = corr[tau];
        int r = 0;
        for (int j = 0; j < L; ++j) {
            const float o = corr[j];
            r += (o > v || (o == v && j < tau)) ? 1 : 0;
        }
        if (r < kk) lags[r] = tau;
        if (r == kk - 1)
            for (int p = kk; p < K; ++p) lags[p] = tau;
    }
    if (tid == TP_THREADS - 1) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += chsum[c];
        row[3 * C] = s / (float)C;
    }
}

}  // namespace

extern "C" {

int immtsf_timellm_prompt_supported(int32_t L, int32_t C, int32_t top_k) {
    return L >= 1 && L <= TP_MAX_L && C >= 1 && C <= TP_MAX_C && top_k >= 1 && top_k <= TP_MAX_K && L * C <= TP_MAX_TILE ? 1 : 0;
}

int immtsf_timellm_prompt_stats(const float* x, int64_t B, int32_t L, int32_t C, int32_t top_k, void* out, immtsf_stream_t stream) {
    if (B < 0 || L < 1 || C < 1 || top_k < 1) return IMMTSF_EINVAL;
    if (!immtsf_timellm_prompt_supported(L, C, top_k)) return IMMTSF_EUNSUPPORTED;
    if (B >= (1ll << 31)) return IMMTSF_EINVAL;
    if (B == 0) return IMMTSF_OK;
    if (!x || !out || (reinterpret_cast<uintptr_t>(x) & 3) || (reinterpret_cast<uintptr_t>(out) & 3)) return IMMTSF_EINVAL;
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(timellm_prompt_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)tp_lds_bytes(TP_MAX_L, TP_MAX_TILE / TP_MAX_L));
    if (attr != hipSuccess) return (int)attr;
    int CP = 1;
    while (CP < C) CP <<= 1;
    const int vec = ((L * C) & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? 1 : 0;
    hipLaunchKernelGGL(timellm_prompt_kernel, dim3((unsigned)B), dim3(TP_THREADS), tp_lds_bytes(L, C), static_cast<hipStream_t>(stream), L, C,
                       top_k, CP, vec, x, static_cast<float*>(out));
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
