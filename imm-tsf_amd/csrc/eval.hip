// immtsf_eval_metrics_accum: the five per-variable sums of lib.evaluation.evaluation() over one batch -- squared, absolute and
// relative error, observation count, count of non-zero truths -- ADDED to an fp64 accumulator [5][C] that lives for a whole loader.
// One launch, each of truth / pred / mask read once; the torch form is three compute_error(..., "sum") calls (about 35 launches that
// read the three tensors nine times).
//
// Determinism: every element's term is formed in fp32 (the reference's arithmetic) and added in fp64 in an order that depends on
// the shape alone: thread -> workgroup (LDS, two levels) -> slab in `scratch` -> the last workgroup to finish (ticket) folds the slabs
// in index order into `acc`.  No floating-point atomics.
//
// A unit is V consecutive elements (V = 4: one 16-byte load per tensor; V = 1 otherwise).  A workgroup walks its units with a stride
// of S units, S the largest multiple of C / gcd(C, V) within 256 threads: S V is a multiple of C, so the column of element e of a
// thread's units is (tid V + e) % C on every pass and its V x 5 partial sums stay in registers.  Position q = tid V + e of a
// workgroup's S V positions therefore belongs to column q % C.
#include "../../include/immtsf.h"
#include "eval.hpp"

namespace {

constexpr int EV_GMAX = 256;       // most workgroups (slabs) of a launch: one per CU

template <int V>
__global__ __launch_bounds__(256) void eval_metrics_kernel(const float* __restrict__ truth, const float* __restrict__ pred,
                                                            const float* __restrict__ mask, size_t n, int C, int S, size_t K, int J,
                                                            double* __restrict__ slabs, unsigned int* __restrict__ ticket,
                                                            double* __restrict__ acc) {
    __shared__ double red[256 * V];      // a statistic's S V positions
    __shared__ double red2[1024];        // [J][C] first-level partials (C J <= 1024)
    __shared__ unsigned int s_last;
    const int tid = threadIdx.x;
    double a[V][EVAL_STATS];
#pragma unroll
    for (int e = 0; e < V; ++e)
#pragma unroll
        for (int k = 0; k < EVAL_STATS; ++k) a[e][k] = 0.0;
    if (tid < S) {
        size_t u = (size_t)blockIdx.x * S * K + tid;
        for (size_t k = 0; k < K; ++k, u += S) {
            const size_t i = u * V;
            if (i >= n) break;
            float t[V], p[V], m[V];
            bool whole = false;
            if constexpr (V == 4) {
                if (i + 4 <= n) {
                    whole = true;
                    const float4 t4 = *reinterpret_cast<const float4*>(truth + i), p4 = *reinterpret_cast<const float4*>(pred + i),
                                 m4 = *reinterpret_cast<const float4*>(mask + i);
                    t[0] = t4.x; t[1] = t4.y; t[2] = t4.z; t[3] = t4.w;
                    p[0] = p4.x; p[1] = p4.y; p[2] = p4.z; p[3] = p4.w;
                    m[0] = m4.x; m[1] = m4.y; m[2] = m4.z; m[3] = m4.w;
                }
            }
            if (!whole) {
#pragma unroll
                for (int e = 0; e < V; ++e) {      // scalar path, and the last (partial) unit of the vector path
                    const bool in = i + e < n;
                    t[e] = in ? truth[i + e] : 0.f;
                    p[e] = in ? pred[i + e] : 0.f;
                    m[e] = in ? mask[i + e] : 0.f;
                }
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float x[EVAL_STATS];
                eval_terms(t[e], p[e], m[e], x);
#pragma unroll
                for (int k2 = 0; k2 < EVAL_STATS; ++k2) a[e][k2] += (double)x[k2];
            }
        }
    }
    // workgroup sums per (statistic, column): J threads per column take every J-th of its positions, then one thread adds the J
    const int NP = S * V, NV = EVAL_STATS * C;
    double* slab = slabs + (size_t)blockIdx.x * NV;
    for (int k = 0; k < EVAL_STATS; ++k) {
        if (tid < S) {
#pragma unroll
            for (int e = 0; e < V; ++e) red[tid * V + e] = a[e][k];
        }
        __syncthreads();
        for (int w = tid; w < C * J; w += 256) {
            const int j = w / C, c = w - j * C;
            double s = 0.0;
            for (int q = c + j * C; q < NP; q += J * C) s += red[q];
            red2[w] = s;
        }
        __syncthreads();
        for (int c = tid; c < C; c += 256) {
            double s = 0.0;
            for (int j = 0; j < J; ++j) s += red2[j * C + c];
            slab[k * C + c] = s;
        }
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        __threadfence();
        s_last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    eval_fold_slabs(slabs, (int)gridDim.x, NV, acc);
    if (tid == 0) *ticket = 0u;
}

// Any C (the form for C beyond what the unit walk takes): a thread per column, a workgroup per block of rows; a thread's sums ARE
// the workgroup's.
__global__ __launch_bounds__(256) void eval_metrics_wide_kernel(const float* __restrict__ truth, const float* __restrict__ pred,
                                                                 const float* __restrict__ mask, int rows, int C, int rpw,
                                                                 double* __restrict__ slabs, unsigned int* __restrict__ ticket,
                                                                 double* __restrict__ acc) {
    __shared__ unsigned int s_last;
    const int tid = threadIdx.x, NV = EVAL_STATS * C;
    const int r0 = blockIdx.x * rpw, r1 = min(rows, r0 + rpw);
    double* slab = slabs + (size_t)blockIdx.x * NV;
    for (int c = tid; c < C; c += 256) {
        double a[EVAL_STATS] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int r = r0; r < r1; ++r) {
            const size_t i = (size_t)r * C + c;
            float x[EVAL_STATS];
            eval_terms(truth[i], pred[i], mask[i], x);
#pragma unroll
            for (int k = 0; k < EVAL_STATS; ++k) a[k] += (double)x[k];
        }
#pragma unroll
        for (int k = 0; k < EVAL_STATS; ++k) slab[k * C + c] = a[k];
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        __threadfence();
        s_last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    eval_fold_slabs(slabs, (int)gridDim.x, NV, acc);
    if (tid == 0) *ticket = 0u;
}

inline int gcd_i(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

}  // namespace

extern "C" {

size_t immtsf_eval_metrics_scratch_bytes(int32_t rows, int32_t C) {
    if (rows < 0 || C < 1) return 0;
    return (size_t)EV_GMAX * EVAL_STATS * (size_t)C * sizeof(double) + 256;
}

int immtsf_eval_metrics_accum(const float* truth, const float* pred, const float* mask, int32_t rows, int32_t C, double* acc,
                              void* scratch, size_t scratch_bytes, uint32_t* ticket, immtsf_stream_t stream) {
    if (rows < 0 || C < 1 || !acc || !scratch || !ticket) return IMMTSF_EINVAL;
    if (rows == 0) return IMMTSF_OK;
    if (!truth || !pred || !mask) return IMMTSF_EINVAL;
    if (scratch_bytes < immtsf_eval_metrics_scratch_bytes(rows, C)) return IMMTSF_EWORKSPACE;
    double* slabs = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(scratch) + 255) & ~uintptr_t(255));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)rows * C;
    const bool aligned = ((reinterpret_cast<uintptr_t>(truth) | reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(mask)) & 15) == 0;
    const int Cp4 = C / gcd_i(C, 4);
    const int V = (aligned && Cp4 <= 256) ? 4 : 1;
    if (V == 1 && C > 256) {
        int G = rows < EV_GMAX ? rows : EV_GMAX;
        const int rpw = cdiv(rows, G);
        G = cdiv(rows, rpw);
        hipLaunchKernelGGL(eval_metrics_wide_kernel, dim3(G), dim3(256), 0, s, truth, pred, mask, rows, C, rpw, slabs, ticket, acc);
        IMMTSF_LAUNCH_CHECK();
        return IMMTSF_OK;
    }
    const int Cp = V == 4 ? Cp4 : C;
    const int S = (256 / Cp) * Cp;                      // units per pass: S V is a multiple of C
    const size_t units = (n + V - 1) / V;
    size_t K = (units + (size_t)S * EV_GMAX - 1) / ((size_t)S * EV_GMAX);
    if (K < 1) K = 1;
    const int G = (int)((units + (size_t)S * K - 1) / ((size_t)S * K));      // <= EV_GMAX
    int J = C >= 256 ? 1 : 256 / C;
    if (J > 32) J = 32;
    if (V == 4)
        hipLaunchKernelGGL(eval_metrics_kernel<4>, dim3(G), dim3(256), 0, s, truth, pred, mask, n, C, S, K, J, slabs, ticket, acc);
    else
        hipLaunchKernelGGL(eval_metrics_kernel<1>, dim3(G), dim3(256), 0, s, truth, pred, mask, n, C, S, K, J, slabs, ticket, acc);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
