// TimesNet's period selection (reference models/TimesNet.py:9-18 FFT_for_Period, here models/TimesNet.py fft_for_period_device + the softmax
// and the position-major copy of TimesBlock.forward) as three launches of the project's own -- no FFT library in the step.  At TimesNet's
// lengths (total = input_len + pred_len of tens to a couple of hundred points) a direct DFT is a few hundred thousand FMAs per window, and
// the backward needs only the k selected frequencies, not an inverse transform.  All fp32, whatever the precision mode.
//
//   spectrum_fwd:    a workgroup per window.  The (T, N) tile and a T-entry cos / sin table -- sincospif(2 m / T), m = 0..T-1; term (f, t)
//                    takes entry (f t) mod T, kept as a running integer, so no large argument reaches a trig function -- go to LDS.  A
//                    thread per (f, n), f <= T / 2: Re = sum_t x cos, Im = -sum_t x sin in t order, amp = sqrt(Re^2 + Im^2) into LDS; then a
//                    thread per f: amp_mean[b, f] = (sum_n amp in n order) / N.  The same launch writes the position-major image xl
//                    (2T B, N): row t B + b is x[b, t, :] from the tile, rows t >= T are zero.
//   spectrum_select: ONE workgroup.  freq[f] = (sum_b amp_mean[b, f] in b order) / B, freq[0] = 0; the k largest by rank counting -- rank_f =
//                    #{j : freq_j > freq_f or (freq_j == freq_f and j < f)}, a strict order (NaN counts as +inf, as torch.topk ranks it), so
//                    every rank has exactly one owner: equal values go to the lower index, results descend.  The owner of rank r < k writes
//                    top[r] and, with period_rows_kernel's arithmetic (csrc/conv.hip), period[r] = T / f (f == 0: T -- no division by
//                    zero) and rows[r] = B (T rounded up to a multiple of the period).  Then a thread per window: weight[b, j] =
//                    amp_mean[b, top_j], w[b, :] = softmax(weight[b, :]).
//   spectrum_bwd:    a workgroup per window.  gs = w (g_w - sum_j g_w w) (softmax backward); Re, Im recomputed at the k selected
//                    frequencies only; dx[b, t, n] = g_xl[t B + b, n] + (1 / N) sum_j gs_j (Re_j cos th_jt - Im_j sin th_jt) / amp_j, the
//                    spectral term 0 where amp_j == 0 (what torch's complex abs backward returns: no NaN).  g_w or g_xl may be NULL (zero).
//
// No atomics, no flags, no spinning; every loop has a host-known trip count; every output word has one writer and every sum one order,
// so two runs give the same bits.
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

constexpr int TS_FWD_THREADS = 1024, TS_THREADS = 256;
// the limits immtsf_timesnet_spectrum_ok reports.  LDS at the limits: forward tile 64 KB + amplitudes (T / 2 + 1) N <= 33 KB + table 4 KB =
// 101 KB, backward tile 64 KB + table 4 KB + 2 k N coefficients <= 32 KB = 100 KB, of the 160 KB
constexpr int TS_MAX_T = 512, TS_MAX_N = 256, TS_MAX_K = 16, TS_MAX_TILE = 16384;

__host__ __device__ __forceinline__ int ts_pad4(int n) { return (n + 3) & ~3; }
inline size_t ts_fwd_lds(int T, int N) { return sizeof(float) * (size_t)(ts_pad4(T * N) + ts_pad4((T / 2 + 1) * N) + 2 * ts_pad4(T)); }
inline size_t ts_bwd_lds(int T, int N, int k) { return sizeof(float) * (size_t)(ts_pad4(T * N) + 2 * ts_pad4(T) + 2 * ts_pad4(k * N)); }
constexpr size_t TS_FWD_LDS_MAX = sizeof(float) * (size_t)(TS_MAX_TILE + TS_MAX_TILE / 2 + TS_MAX_N + 4 + 2 * TS_MAX_T);
constexpr size_t TS_BWD_LDS_MAX = sizeof(float) * (size_t)(TS_MAX_TILE + 2 * TS_MAX_T + 2 * TS_MAX_K * TS_MAX_N);

// the window's tile into LDS; vec: (T N) % 4 == 0 and x 16-byte aligned (the host checked)
template <int THREADS>
__device__ __forceinline__ void ts_stage(float* tile, const float* __restrict__ xb, int n, int vec) {
    const int tid = threadIdx.x;
    if (vec) {
        for (int e = tid; e < (n >> 2); e += THREADS) reinterpret_cast<f32x4*>(tile)[e] = reinterpret_cast<const f32x4*>(xb)[e];
    } else {
        for (int e = tid; e < n; e += THREADS) tile[e] = xb[e];
    }
}
// ct[m] = cos(2 pi m / T), st[m] = sin(2 pi m / T): the argument 2 m / T of sincospif stays below 2
template <int THREADS>
__device__ __forceinline__ void ts_table(float* ct, float* st, int T) {
    for (int m = threadIdx.x; m < T; m += THREADS) {
        float s, c;
        sincospif(2.f * (float)m / (float)T, &s, &c);
        ct[m] = c;
        st[m] = s;
    }
}

// grid (B)
__global__ __launch_bounds__(TS_FWD_THREADS) void timesnet_spectrum_fwd_kernel(int B, int T, int N, int vec, int vec_xl, const float* __restrict__ x,
                                                                               float* __restrict__ amp_mean, float* __restrict__ xl) {
    extern __shared__ __attribute__((aligned(16))) float ts_lds[];
    const int tid = threadIdx.x, b = blockIdx.x, F = T / 2 + 1;
    float* tile = ts_lds;                             // [T][N]
    float* amp = tile + ts_pad4(T * N);               // [F][N]
    float* ct = amp + ts_pad4(F * N);                 // [T]
    float* st = ct + ts_pad4(T);                      // [T]
    ts_stage<TS_FWD_THREADS>(tile, x + (size_t)b * T * N, T * N, vec);
    ts_table<TS_FWD_THREADS>(ct, st, T);
    __syncthreads();
    // ---- the position-major image: row t B + b, t < 2 T ----
    if (vec_xl) {      // N % 4 == 0 and xl 16-byte aligned
        const int N4 = N >> 2;
        for (int e = tid; e < 2 * T * N4; e += TS_FWD_THREADS) {
            const int t = e / N4, c = e - t * N4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (t < T) v = reinterpret_cast<const f32x4*>(tile)[e];
            reinterpret_cast<f32x4*>(xl)[((size_t)t * B + b) * N4 + c] = v;
        }
    } else {
        for (int e = tid; e < 2 * T * N; e += TS_FWD_THREADS) {
            const int t = e / N, c = e - t * N;
            xl[((size_t)t * B + b) * N + c] = t < T ? tile[e] : 0.f;
        }
    }
    // ---- amplitudes: a thread per (f, n), the sum in t order ----
    for (int e = tid; e < F * N; e += TS_FWD_THREADS) {
        const int f = e / N, n = e - f * N;
        float re = 0.f, im = 0.f;
        int idx = 0;                                  // (f t) mod T
        for (int t = 0; t < T; ++t) {
            const float v = tile[t * N + n];
            re = fmaf(v, ct[idx], re);
            im = fmaf(v, st[idx], im);                // (-Im: the sign does not reach the amplitude)
            idx += f;
            if (idx >= T) idx -= T;
        }
        amp[e] = sqrtf(re * re + im * im);
    }
    __syncthreads();
    for (int f = tid; f < F; f += TS_FWD_THREADS) {
        float s = 0.f;
        for (int n = 0; n < N; ++n) s += amp[f * N + n];
        amp_mean[(size_t)b * F + f] = s / (float)N;
    }
}

__device__ __forceinline__ float ts_key(float v) { return v == v ? v : INFINITY; }

// grid (1)
__global__ __launch_bounds__(TS_THREADS) void timesnet_spectrum_select_kernel(int B, int T, int k, const float* __restrict__ amp_mean,
                                                                              float* __restrict__ freq_out, long long* __restrict__ top,
                                                                              int* __restrict__ period, int* __restrict__ rows,
                                                                              float* __restrict__ weight, float* __restrict__ w) {
    __shared__ float freq[TS_MAX_T / 2 + 1];
    __shared__ int sel[TS_MAX_K];
    const int tid = threadIdx.x, F = T / 2 + 1;
    for (int f = tid; f < F; f += TS_THREADS) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += amp_mean[(size_t)b * F + f];
        s = f == 0 ? 0.f : s / (float)B;
        freq[f] = s;
        if (freq_out) freq_out[f] = s;
    }
    __syncthreads();
    for (int f = tid; f < F; f += TS_THREADS) {
        const float v = ts_key(freq[f]);
        int r = 0;
        for (int j = 0; j < F; ++j) {
            const float o = ts_key(freq[j]);
            r += (o > v || (o == v && j < f)) ? 1 : 0;
        }
        if (r < k) {
            const int p = f > 0 ? T / f : T;
            const int length = (T % p == 0) ? T : (T / p + 1) * p;
            sel[r] = f;
            top[r] = f;
            period[r] = p;
            rows[r] = length * B;
        }
    }
    __syncthreads();
    for (int b = tid; b < B; b += TS_THREADS) {
        const float* a = amp_mean + (size_t)b * F;
        float m = -INFINITY;
        for (int j = 0; j < k; ++j) {
            const float v = a[sel[j]];
            weight[(size_t)b * k + j] = v;
            m = fmaxf(m, v);
        }
        float s = 0.f;
        for (int j = 0; j < k; ++j) s += expf(a[sel[j]] - m);
        for (int j = 0; j < k; ++j) w[(size_t)b * k + j] = expf(a[sel[j]] - m) / s;
    }
}

// grid (B)
__global__ __launch_bounds__(TS_THREADS) void timesnet_spectrum_bwd_kernel(int B, int T, int N, int k, int vec, const float* __restrict__ x,
                                                                           const long long* __restrict__ top, const float* __restrict__ w,
                                                                           const float* __restrict__ g_w, const float* __restrict__ g_xl,
                                                                           float* __restrict__ dx) {
    extern __shared__ __attribute__((aligned(16))) float ts_lds[];
    __shared__ float gs[TS_MAX_K];
    __shared__ int fj[TS_MAX_K];
    const int tid = threadIdx.x, b = blockIdx.x;
    float* dxb = dx + (size_t)b * T * N;
    if (!g_w) {      // no gradient reaches w: the image's gradient, transposed back
        for (int e = tid; e < T * N; e += TS_THREADS) {
            const int t = e / N, n = e - t * N;
            dxb[e] = g_xl ? g_xl[((size_t)t * B + b) * N + n] : 0.f;
        }
        return;
    }
    float* tile = ts_lds;                             // [T][N]
    float* ct = tile + ts_pad4(T * N);                // [T]
    float* st = ct + ts_pad4(T);                      // [T]
    float* cr = st + ts_pad4(T);                      // [k][N]  gs_j Re_j / (N amp_j)
    float* ci = cr + ts_pad4(k * N);                  // [k][N]  gs_j Im_j / (N amp_j)
    ts_stage<TS_THREADS>(tile, x + (size_t)b * T * N, T * N, vec);
    ts_table<TS_THREADS>(ct, st, T);
    if (tid < k) {
        const float* wb = w + (size_t)b * k;
        const float* gb = g_w + (size_t)b * k;
        float dot = 0.f;
        for (int j = 0; j < k; ++j) dot = fmaf(gb[j], wb[j], dot);
        gs[tid] = wb[tid] * (gb[tid] - dot);
        const long long f = top[tid];
        fj[tid] = f < 0 ? 0 : (f >= T ? T - 1 : (int)f);      // (the forward's indices are <= T / 2; nothing else may index the table)
    }
    __syncthreads();
    for (int e = tid; e < k * N; e += TS_THREADS) {
        const int j = e / N, n = e - j * N, f = fj[j];
        float re = 0.f, ims = 0.f;
        int idx = 0;
        for (int t = 0; t < T; ++t) {
            const float v = tile[t * N + n];
            re = fmaf(v, ct[idx], re);
            ims = fmaf(v, st[idx], ims);
            idx += f;
            if (idx >= T) idx -= T;
        }
        const float a = sqrtf(re * re + ims * ims);
        const float g = gs[j] / (float)N;
        cr[e] = a > 0.f ? g * (re / a) : 0.f;
        ci[e] = a > 0.f ? g * (-ims / a) : 0.f;
    }
    __syncthreads();
    for (int e = tid; e < T * N; e += TS_THREADS) {
        const int t = e / N, n = e - t * N;
        float acc = 0.f;
        for (int j = 0; j < k; ++j) {
            const int idx = (fj[j] * t) % T;
            acc = fmaf(cr[j * N + n], ct[idx], acc);
            acc = fmaf(-ci[j * N + n], st[idx], acc);
        }
        dxb[e] = (g_xl ? g_xl[((size_t)t * B + b) * N + n] : 0.f) + acc;
    }
}

inline bool ts_al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace

extern "C" {

int immtsf_timesnet_spectrum_ok(int32_t T, int32_t N, int32_t k) {
    return T >= 2 && T <= TS_MAX_T && N >= 1 && N <= TS_MAX_N && T * N <= TS_MAX_TILE && k >= 1 && k <= TS_MAX_K && k <= T / 2 ? 1 : 0;
}

int immtsf_timesnet_spectrum_fwd(const float* x, int32_t B, int32_t T, int32_t N, float* amp_mean, float* xl, immtsf_stream_t stream) {
    if (B < 0 || T < 1 || N < 1) return IMMTSF_EINVAL;
    if (!immtsf_timesnet_spectrum_ok(T, N, 1)) return IMMTSF_EUNSUPPORTED;
    if (2ll * T * B >= (1ll << 31)) return IMMTSF_EINVAL;
    if (B == 0) return IMMTSF_OK;
    if (!x || !amp_mean || !xl || !ts_al4(x) || !ts_al4(amp_mean) || !ts_al4(xl)) return IMMTSF_EINVAL;
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(timesnet_spectrum_fwd_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)TS_FWD_LDS_MAX);
    if (attr != hipSuccess) return (int)attr;
    const int vec = ((T * N) & 3) == 0 && al16(x) ? 1 : 0, vec_xl = (N & 3) == 0 && al16(xl) ? 1 : 0;
    hipLaunchKernelGGL(timesnet_spectrum_fwd_kernel, dim3((unsigned)B), dim3(TS_FWD_THREADS), ts_fwd_lds(T, N), static_cast<hipStream_t>(stream), B,
                       T, N, vec, vec_xl, x, amp_mean, xl);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_timesnet_spectrum_select(const float* amp_mean, int32_t B, int32_t T, int32_t k, float* freq, int64_t* top, int32_t* period,
                                    int32_t* rows, float* weight, float* w, immtsf_stream_t stream) {
    if (B < 1 || T < 2 || k < 1) return IMMTSF_EINVAL;
    if (T > TS_MAX_T || k > TS_MAX_K || k > T / 2) return IMMTSF_EUNSUPPORTED;
    if (2ll * T * B >= (1ll << 31)) return IMMTSF_EINVAL;
    if (!amp_mean || !top || !period || !rows || !weight || !w || !ts_al4(amp_mean) || !ts_al4(freq) || !ts_al4(period) || !ts_al4(rows) ||
        !ts_al4(weight) || !ts_al4(w) || !al8(top))
        return IMMTSF_EINVAL;
    hipLaunchKernelGGL(timesnet_spectrum_select_kernel, dim3(1), dim3(TS_THREADS), 0, static_cast<hipStream_t>(stream), B, T, k, amp_mean, freq,
                       reinterpret_cast<long long*>(top), period, rows, weight, w);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_timesnet_spectrum_bwd(const float* x, const int64_t* top, const float* w, const float* g_w, const float* g_xl, int32_t B, int32_t T,
                                 int32_t N, int32_t k, float* dx, immtsf_stream_t stream) {
    if (B < 0 || T < 1 || N < 1 || k < 1) return IMMTSF_EINVAL;
    if (!immtsf_timesnet_spectrum_ok(T, N, k)) return IMMTSF_EUNSUPPORTED;
    if (2ll * T * B >= (1ll << 31)) return IMMTSF_EINVAL;
    if (B == 0) return IMMTSF_OK;
    if (!x || !top || !w || !dx || !ts_al4(x) || !ts_al4(w) || !ts_al4(g_w) || !ts_al4(g_xl) || !ts_al4(dx) || !al8(top)) return IMMTSF_EINVAL;
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(timesnet_spectrum_bwd_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)TS_BWD_LDS_MAX);
    if (attr != hipSuccess) return (int)attr;
    const int vec = ((T * N) & 3) == 0 && al16(x) ? 1 : 0;
    hipLaunchKernelGGL(timesnet_spectrum_bwd_kernel, dim3((unsigned)B), dim3(TS_THREADS), ts_bwd_lds(T, N, k), static_cast<hipStream_t>(stream), B,
                       T, N, k, vec, x, reinterpret_cast<const long long*>(top), w, g_w, g_xl, dx);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
