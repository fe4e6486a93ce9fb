// Informer's ProbAttention (reference layers/SelfAttention_Family.py:80-178, utils/masking.py ProbMask) as TWO launches forward and TWO
// backward, all fp32.  q (B, L_Q, H, D), k / v (B, L_K, H, D) are read in the projections' layout; the result is (B, H, L_Q, D) contiguous
// (the caller's reshape to (B, L, H D) without a transpose is part of the reference's function).
//
//   measure:  M[b,h,i] = max_j (q_i . k_s(i,j)) - sum_j (q_i . k_s(i,j)) / L_K over the U sampled keys s(i, :) of query i (one sample for
//             every batch and head; a key drawn twice counts twice).  A wave per query, the lanes split D, a wave reduction per key.
//   context:  workgroup (b h, slab).  Every workgroup ranks M[b,h,:] in LDS -- rank_i = #{j : M_j > M_i or (M_j == M_i and j < i)}, a strict
//             order (NaN counts as -inf), so exactly u queries have rank < u: ties go to the lower index -- and lists them ascending.
//             The selected rows are dealt to the slabs in chunks of PA_RC: scores against every key (a wave per key), the causal mask
//             (key j > i), softmax, P V, written straight into the result; P and the list are kept for the backward.  The other rows are
//             column-independent: slab s fills columns 64 s .. 64 s + 63 with mean(V) or, causal, the running sum of V.
//   backward: launch A (same dealing): dP = dO_sel V^T, dS = P o (dP - rowsum(P o dP)), dQ_sel = scale dS K.  Launch B (column slabs):
//             dK = scale dS^T Q_sel, dV = P^T dO_sel + the fill's transpose (sum of the unselected dO / L_V, or their reverse running sum),
//             and exact zeros into the unselected rows of dQ.  No gradient flows through the measure.
//
// No atomics: every output element has one writer and every sum a fixed order, so two runs give the same bits.
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

constexpr int PA_THREADS = 256;
constexpr int PA_MAX_L = 1024, PA_MAX_D = 512;      // the limits immtsf_prob_attention_supported reports
constexpr int PA_RC = 4;                            // selected rows per chunk: one per wave in the row-wise steps
constexpr int PA_RS = 32;                           // selected rows staged at once by backward B
// LDS of the largest kernel (context): M, flags, list 3 x 4 KB + rows 8 KB + scores 16 KB + partial sums 1 KB = 37 KB of the 160 KB

struct PaDims { int B, H, LQ, LK, D, U, u; };

__host__ __device__ __forceinline__ int pa_cdiv(int a, int b) { return (a + b - 1) / b; }
__device__ __forceinline__ size_t pa_row(int b, int l, int h, int L, int H, int D) { return (((size_t)b * L + l) * H + h) * D; }

__global__ __launch_bounds__(PA_THREADS) void pa_measure_kernel(PaDims d, const float* __restrict__ q, const float* __restrict__ k,
                                                                const int* __restrict__ sample, float* __restrict__ M) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long item = (long long)blockIdx.x * (PA_THREADS / 64) + wave, n = (long long)d.B * d.H * d.LQ;
    if (item >= n) return;      // wave-uniform
    const int i = (int)(item % d.LQ), bh = (int)(item / d.LQ), b = bh / d.H, h = bh - b * d.H;
    const float* qr = q + pa_row(b, i, h, d.LQ, d.H, d.D);
    float qv[PA_MAX_D / 64];
#pragma unroll
    for (int c = 0; c < PA_MAX_D / 64; ++c) {
        const int dd = c * 64 + lane;
        qv[c] = dd < d.D ? qr[dd] : 0.f;
    }
    float mx = -INFINITY, sm = 0.f;
    for (int j = 0; j < d.U; ++j) {
        int idx = sample[(size_t)i * d.U + j];
        idx = min(max(idx, 0), d.LK - 1);      // a sample is a key index; never read outside k whatever it holds
        const float* kr = k + pa_row(b, idx, h, d.LK, d.H, d.D);
        float a = 0.f;
#pragma unroll
        for (int c = 0; c < PA_MAX_D / 64; ++c) {
            const int dd = c * 64 + lane;
            if (dd < d.D) a = fmaf(qv[c], kr[dd], a);
        }
        a = wave_sum(a);
        mx = fmaxf(mx, a);
        sm += a;
    }
    if (lane == 0) M[item] = mx - sm / (float)d.LK;
}

// sc[r][j] = rows[r] . mat[j] for r < PA_RC, j < LK: a wave per key, the lanes split D.  rows [PA_RC][D] in LDS (unused rows zero),
// mat row j at mat + j stride.  Every thread calls it; it ends behind a barrier.
__device__ __forceinline__ void pa_rows_dot(int D, int LK, const float* rows, const float* __restrict__ mat, size_t stride, float* sc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = wave; j < LK; j += PA_THREADS / 64) {      // the trip count is wave-uniform
        const float* mr = mat + (size_t)j * stride;
        float a[PA_RC];
#pragma unroll
        for (int r = 0; r < PA_RC; ++r) a[r] = 0.f;
        for (int dd = lane; dd < D; dd += 64) {
            const float kv = mr[dd];
#pragma unroll
            for (int r = 0; r < PA_RC; ++r) a[r] = fmaf(kv, rows[r * D + dd], a[r]);
        }
#pragma unroll
        for (int r = 0; r < PA_RC; ++r) a[r] = wave_sum(a[r]);
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < PA_RC; ++r) sc[r * LK + j] = a[r];
        }
    }
    __syncthreads();
}

// out[ridx[r]] = alpha sc[r] mat for r < nr: a thread per column, j in index order.  out row i at out + i ostride.
__device__ __forceinline__ void pa_rows_mat(int nr, int D, int LK, const float* sc, const float* __restrict__ mat, size_t stride, float alpha,
                                            const int* ridx, float* __restrict__ out, size_t ostride) {
    for (int dd = threadIdx.x; dd < D; dd += PA_THREADS) {
        float a[PA_RC];
#pragma unroll
        for (int r = 0; r < PA_RC; ++r) a[r] = 0.f;
        for (int j = 0; j < LK; ++j) {
            const float v = mat[(size_t)j * stride + dd];
#pragma unroll
            for (int r = 0; r < PA_RC; ++r) a[r] = fmaf(sc[r * LK + j], v, a[r]);
        }
#pragma unroll
        for (int r = 0; r < PA_RC; ++r)
            if (r < nr) out[(size_t)ridx[r] * ostride + dd] = alpha * a[r];
    }
}

// grid (B H, cdiv(D, 64))
__global__ __launch_bounds__(PA_THREADS) void pa_context_kernel(PaDims d, int causal, float scale, const float* __restrict__ q,
                                                                const float* __restrict__ k, const float* __restrict__ v,
                                                                const float* __restrict__ M, float* __restrict__ out, float* __restrict__ P,
                                                                int* __restrict__ selg) {
    __shared__ float Ms[PA_MAX_L];
    __shared__ int flag[PA_MAX_L], sel[PA_MAX_L], ridx[PA_RC];
    __shared__ float rows[PA_RC * PA_MAX_D], sc[PA_RC * PA_MAX_L], part[PA_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bh = blockIdx.x, s = blockIdx.y, NS = gridDim.y, b = bh / d.H, h = bh - b * d.H;
    const int LQ = d.LQ, LK = d.LK, D = d.D, u = d.u;
    const size_t stride = (size_t)d.H * D;
    // ---- the u queries with the largest measure, ascending ----
    for (int i = tid; i < LQ; i += PA_THREADS) {
        const float m = M[(size_t)bh * LQ + i];
        Ms[i] = m == m ? m : -INFINITY;
    }
    __syncthreads();
    for (int i = tid; i < LQ; i += PA_THREADS) {
        const float m = Ms[i];
        int r = 0;
        for (int j = 0; j < LQ; ++j) {
            const float o = Ms[j];
            r += (o > m || (o == m && j < i)) ? 1 : 0;
        }
        flag[i] = r < u ? 1 : 0;
    }
    __syncthreads();
    for (int i = tid; i < LQ; i += PA_THREADS) {
        if (!flag[i]) continue;
        int p = 0;
        for (int j = 0; j < i; ++j) p += flag[j];
        if (p < u) sel[p] = i;
    }
    __syncthreads();
    if (s == 0)
        for (int r = tid; r < u; r += PA_THREADS) selg[(size_t)bh * u + r] = sel[r];
    // ---- the selected rows, chunks dealt round-robin to the slabs ----
    const float* kb = k + pa_row(b, 0, h, LK, d.H, D);
    const float* vb = v + pa_row(b, 0, h, LK, d.H, D);
    float* ob = out + (size_t)bh * LQ * D;
    for (int r0 = s * PA_RC; r0 < u; r0 += NS * PA_RC) {
        const int nr = min(PA_RC, u - r0);
        if (tid < PA_RC) ridx[tid] = tid < nr ? sel[r0 + tid] : 0;
        for (int e = tid; e < PA_RC * D; e += PA_THREADS) {
            const int r = e / D, dd = e - r * D;
            rows[e] = r < nr ? q[pa_row(b, sel[r0 + r], h, LQ, d.H, D) + dd] : 0.f;
        }
        __syncthreads();
        pa_rows_dot(D, LK, rows, kb, stride, sc);
        if (wave < nr) {      // a wave per row
            float* x = sc + wave * LK;
            const int lim = causal ? min(ridx[wave] + 1, LK) : LK;      // keys j < lim are seen
            float mx = -INFINITY;
            for (int j = lane; j < lim; j += 64) mx = fmaxf(mx, x[j] * scale);
            mx = wave_max(mx);
            float sm = 0.f;
            for (int j = lane; j < lim; j += 64) {
                const float e = expf(x[j] * scale - mx);
                x[j] = e;
                sm += e;
            }
            sm = wave_sum(sm);
            const float inv = 1.f / sm;
            float* pr = P + ((size_t)bh * u + r0 + wave) * LK;
            for (int j = lane; j < LK; j += 64) {
                const float p = j < lim ? x[j] * inv : 0.f;
                x[j] = p;
                pr[j] = p;
            }
        }
        __syncthreads();
        pa_rows_mat(nr, D, LK, sc, vb, stride, 1.f, ridx, ob, (size_t)D);
        __syncthreads();      // the next chunk overwrites rows / sc / ridx
    }
    // ---- every other row: columns 64 s .. 64 s + 63, the rows of V in four contiguous shares (one per wave), folded in wave order ----
    const int col = s * 64 + lane;
    const bool on = col < D;
    const int ch = pa_cdiv(LK, PA_THREADS / 64), j0 = min(LK, wave * ch), j1 = min(LK, j0 + ch);
    float t = 0.f;
    if (on)
        for (int j = j0; j < j1; ++j) t += vb[(size_t)j * stride + col];
    part[tid] = t;
    __syncthreads();
    if (!causal) {
        const float mean = ((part[lane] + part[64 + lane]) + (part[128 + lane] + part[192 + lane])) / (float)LK;
        const int cq = pa_cdiv(LQ, PA_THREADS / 64), i0 = min(LQ, wave * cq), i1 = min(LQ, i0 + cq);
        if (on)
            for (int i = i0; i < i1; ++i)
                if (!flag[i]) ob[(size_t)i * D + col] = mean;
    } else {      // L_Q == L_K
        float run = 0.f;
        for (int w = 0; w < wave; ++w) run += part[w * 64 + lane];
        if (on)
            for (int j = j0; j < j1; ++j) {
                run += vb[(size_t)j * stride + col];
                if (!flag[j]) ob[(size_t)j * D + col] = run;
            }
    }
}

// grid (B H, cdiv(D, 64)): dS and the selected rows of dQ
__global__ __launch_bounds__(PA_THREADS) void pa_bwd_rows_kernel(PaDims d, float scale, const float* __restrict__ k, const float* __restrict__ v,
                                                                 const float* __restrict__ dO, const float* __restrict__ P,
                                                                 const int* __restrict__ selg, float* __restrict__ dS, float* __restrict__ dq) {
    __shared__ int ridx[PA_RC];
    __shared__ float rows[PA_RC * PA_MAX_D], sc[PA_RC * PA_MAX_L];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bh = blockIdx.x, s = blockIdx.y, NS = gridDim.y, b = bh / d.H, h = bh - b * d.H;
    const int LQ = d.LQ, LK = d.LK, D = d.D, u = d.u;
    const size_t stride = (size_t)d.H * D;
    const float* kb = k + pa_row(b, 0, h, LK, d.H, D);
    const float* vb = v + pa_row(b, 0, h, LK, d.H, D);
    const float* gb = dO + (size_t)bh * LQ * D;
    const int* sel = selg + (size_t)bh * u;
    for (int r0 = s * PA_RC; r0 < u; r0 += NS * PA_RC) {
        const int nr = min(PA_RC, u - r0);
        if (tid < PA_RC) ridx[tid] = tid < nr ? min(max(sel[r0 + tid], 0), LQ - 1) : 0;
        __syncthreads();
        for (int e = tid; e < PA_RC * D; e += PA_THREADS) {
            const int r = e / D, dd = e - r * D;
            rows[e] = r < nr ? gb[(size_t)ridx[r] * D + dd] : 0.f;
        }
        __syncthreads();
        pa_rows_dot(D, LK, rows, vb, stride, sc);      // dP
        if (wave < nr) {
            float* x = sc + wave * LK;
            const float* pr = P + ((size_t)bh * u + r0 + wave) * LK;
            float* ds = dS + ((size_t)bh * u + r0 + wave) * LK;
            float rs = 0.f;
            for (int j = lane; j < LK; j += 64) rs = fmaf(pr[j], x[j], rs);
            rs = wave_sum(rs);
            for (int j = lane; j < LK; j += 64) {
                const float g = pr[j] * (x[j] - rs);
                x[j] = g;
                ds[j] = g;
            }
        }
        __syncthreads();
        pa_rows_mat(nr, D, LK, sc, kb, stride, scale, ridx, dq + pa_row(b, 0, h, LQ, d.H, D), stride);
        __syncthreads();
    }
}

// grid (B H, cdiv(D, 64)): columns 64 s .. 64 s + 63 of dK, dV and of the unselected rows of dQ
__global__ __launch_bounds__(PA_THREADS) void pa_bwd_cols_kernel(PaDims d, int causal, float scale, const float* __restrict__ q,
                                                                 const float* __restrict__ dO, const float* __restrict__ P,
                                                                 const float* __restrict__ dS, const int* __restrict__ selg,
                                                                 float* __restrict__ dq, float* __restrict__ dk, float* __restrict__ dv) {
    __shared__ int flag[PA_MAX_L];
    __shared__ float qs[PA_RS * 64], gs[PA_RS * 64], part[PA_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bh = blockIdx.x, s = blockIdx.y, b = bh / d.H, h = bh - b * d.H;
    const int LQ = d.LQ, LK = d.LK, D = d.D, u = d.u;
    const size_t stride = (size_t)d.H * D;
    const int* sel = selg + (size_t)bh * u;
    const float* qb = q + pa_row(b, 0, h, LQ, d.H, D);
    const float* gb = dO + (size_t)bh * LQ * D;
    float* dqb = dq + pa_row(b, 0, h, LQ, d.H, D);
    float* dkb = dk + pa_row(b, 0, h, LK, d.H, D);
    float* dvb = dv + pa_row(b, 0, h, LK, d.H, D);
    const int col = s * 64 + lane;
    const bool on = col < D;
    for (int i = tid; i < LQ; i += PA_THREADS) flag[i] = 0;
    __syncthreads();
    for (int r = tid; r < u; r += PA_THREADS) flag[min(max(sel[r], 0), LQ - 1)] = 1;
    const int ch = pa_cdiv(LK, PA_THREADS / 64), j0 = min(LK, wave * ch), j1 = min(LK, j0 + ch);
    for (int c0 = 0; c0 < u; c0 += PA_RS) {      // the selected rows in chunks: the first chunk writes, the later ones add (same thread, same address)
        const int nrs = min(PA_RS, u - c0);
        __syncthreads();
        for (int e = tid; e < nrs * 64; e += PA_THREADS) {
            const int r = e >> 6, c = s * 64 + (e & 63), i = min(max(sel[c0 + r], 0), LQ - 1);
            qs[e] = c < D ? qb[(size_t)i * stride + c] : 0.f;
            gs[e] = c < D ? gb[(size_t)i * D + c] : 0.f;
        }
        __syncthreads();
        for (int j = j0; j < j1; ++j) {
            float ak = 0.f, av = 0.f;
            for (int r = 0; r < nrs; ++r) {
                const size_t o = ((size_t)bh * u + c0 + r) * LK + j;
                ak = fmaf(dS[o], qs[r * 64 + lane], ak);
                av = fmaf(P[o], gs[r * 64 + lane], av);
            }
            if (on) {
                const size_t o = (size_t)j * stride + col;
                if (c0 == 0) { dkb[o] = scale * ak; dvb[o] = av; }
                else { dkb[o] += scale * ak; dvb[o] += av; }
            }
        }
    }
    // ---- the fill's transpose, and zeros into the unselected rows of dQ ----
    const int cq = pa_cdiv(LQ, PA_THREADS / 64), i0 = min(LQ, wave * cq), i1 = min(LQ, i0 + cq);
    float t = 0.f;
    if (on)
        for (int i = i0; i < i1; ++i) {
            if (flag[i]) continue;
            t += gb[(size_t)i * D + col];
            dqb[(size_t)i * stride + col] = 0.f;
        }
    part[tid] = t;
    __syncthreads();
    if (!causal) {
        const float tot = ((part[lane] + part[64 + lane]) + (part[128 + lane] + part[192 + lane])) / (float)LK;
        if (on)
            for (int j = j0; j < j1; ++j) dvb[(size_t)j * stride + col] += tot;
    } else {      // L_Q == L_K, so i0 / i1 are j0 / j1: dV[j] += sum of the unselected dO[i], i >= j
        float run = 0.f;
        for (int w = PA_THREADS / 64 - 1; w > wave; --w) run += part[w * 64 + lane];
        if (on)
            for (int j = j1 - 1; j >= j0; --j) {
                if (!flag[j]) run += gb[(size_t)j * D + col];
                dvb[(size_t)j * stride + col] += run;
            }
    }
}

inline bool pa_dims_ok(int64_t B, int64_t H, int LQ, int LK, int D, int U, int u, int causal) {
    return B >= 0 && H >= 1 && U >= 1 && U <= LK && immtsf_prob_attention_supported(LQ, LK, D, u) && (!causal || LQ == LK) &&
           B * H * (int64_t)(LQ > LK ? LQ : LK) < (1ll << 31);
}

}  // namespace

extern "C" {

int immtsf_prob_attention_supported(int32_t L_Q, int32_t L_K, int32_t D, int32_t u) {
    return L_Q >= 1 && L_Q <= PA_MAX_L && L_K >= 1 && L_K <= PA_MAX_L && D >= 1 && D <= PA_MAX_D && u >= 1 && u <= L_Q ? 1 : 0;
}

int immtsf_prob_attention_forward(int32_t B, int32_t H, int32_t L_Q, int32_t L_K, int32_t D, int32_t U_part, int32_t u, int32_t causal,
                                  float scale, const float* q, const float* k, const float* v, const int32_t* index_sample, float* M,
                                  float* out, float* P, int32_t* sel, immtsf_stream_t stream) {
    if (L_Q < 1 || L_K < 1 || D < 1 || u < 1) return IMMTSF_EINVAL;
    if (!immtsf_prob_attention_supported(L_Q, L_K, D, u)) return IMMTSF_EUNSUPPORTED;
    if (!pa_dims_ok(B, H, L_Q, L_K, D, U_part, u, causal)) return IMMTSF_EINVAL;
    if (B == 0) return IMMTSF_OK;
    if (!q || !k || !v || !index_sample || !M || !out || !P || !sel) return IMMTSF_EINVAL;
    const PaDims d{B, H, L_Q, L_K, D, U_part, u};
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pa_measure_kernel, dim3(cdiv(B * H * L_Q, PA_THREADS / 64)), dim3(PA_THREADS), 0, s, d, q, k, index_sample, M);
    IMMTSF_LAUNCH_CHECK();
    hipLaunchKernelGGL(pa_context_kernel, dim3(B * H, cdiv(D, 64)), dim3(PA_THREADS), 0, s, d, causal ? 1 : 0, scale, q, k, v, M, out, P, sel);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_prob_attention_backward(int32_t B, int32_t H, int32_t L_Q, int32_t L_K, int32_t D, int32_t u, int32_t causal, float scale,
                                   const float* q, const float* k, const float* v, const float* dO, const float* P, const int32_t* sel,
                                   float* dS, float* dq, float* dk, float* dv, immtsf_stream_t stream) {
    if (L_Q < 1 || L_K < 1 || D < 1 || u < 1) return IMMTSF_EINVAL;
    if (!immtsf_prob_attention_supported(L_Q, L_K, D, u)) return IMMTSF_EUNSUPPORTED;
    if (!pa_dims_ok(B, H, L_Q, L_K, D, 1, u, causal)) return IMMTSF_EINVAL;
    if (B == 0) return IMMTSF_OK;
    if (!q || !k || !v || !dO || !P || !sel || !dS || !dq || !dk || !dv) return IMMTSF_EINVAL;
    const PaDims d{B, H, L_Q, L_K, D, 1, u};
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pa_bwd_rows_kernel, dim3(B * H, cdiv(D, 64)), dim3(PA_THREADS), 0, s, d, scale, k, v, dO, P, sel, dS, dq);
    IMMTSF_LAUNCH_CHECK();
    hipLaunchKernelGGL(pa_bwd_cols_kernel, dim3(B * H, cdiv(D, 64)), dim3(PA_THREADS), 0, s, d, causal ? 1 : 0, scale, q, dO, P, dS, sel, dq,
                       dk, dv);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
