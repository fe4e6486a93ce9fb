// DLinear's forecasting() (reference models/DLinear.py:61-134, layers/Autoformer_EncDec.py:21-52) as ONE launch forward and TWO launches
// backward, all fp32.  Per (window b, channel c) row, with the history zero-padded from L to S inside the kernel:
//
//   cnt = max(sum m, 1); mean = sum d m / cnt; xc[l] = d[l] m[l] - mean (EVERY l < S: masked and padded positions hold -mean);
//   std = sqrt(sum (xc m)^2 / cnt + 1e-5); xn = xc / std;
//   trend[l] = (1/k) sum_{|j| <= (k-1)/2} xn[clamp(l + j, 0, S-1)]; seas = xn - trend;
//   out[p] = (Ws[p,:] seas + bs[p]) + (Wt[p,:] trend + bt[p]) + (Wtau[p,:] tp[b,:] + btau[p]); y[b,p,c] = out[p] std + mean, p < Lp.
//
// Everything after the normalisation is linear and no input takes a gradient, so the backward is parameter gradients only:
// dO[p] = dY[b,p,c] std (0 for p >= Lp); dWs += dO (x) seas, dWt += dO (x) trend, dWtau += dO (x) tp, the three bias gradients = sum dO.
//
// Forward: a workgroup stages RB rows (seas, trend, tp: 3 S floats each) in LDS -- a wave per row for the two masked sums, then every
// thread for the moving average, whose window is the in-range run plus the two clamped ends counted, not walked (k > S costs nothing) --
// and a thread per (row, p) takes the three dot products.  The weight rows come from global memory (shared mode: 3 P S floats that every
// workgroup re-reads from L2); the staged rows are LDS broadcasts.
//
// Backward: the rows of a parameter group (shared mode: all B C rows, one group; individual: the B rows of channel c, C groups) are dealt
// to <= 256 / groups workgroups in contiguous shares.  A workgroup restages its rows from the inputs and the saved mean / std in chunks
// of RB, a thread per (p, l) entry adds the chunk's RB products in row order and accumulates into the workgroup's OWN slab (same thread,
// same address on every chunk: no race, the first chunk writes, so nothing is zero-filled).  The second launch folds a group's slabs in
// index order into the gradients.  No floating-point atomics anywhere: the order depends on the shape alone, two runs give the same bits.
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

constexpr int DL_MAX_S = 128, DL_MAX_P = 128;      // the limits immtsf_dlinear_supported reports
constexpr int DL_MAX_K = (1 << 24) - 1;            // the clamped ends' counts stay exact in fp32
constexpr int DL_THREADS = 256;
constexpr int DL_LDS = 8192;                       // floats of staged rows per workgroup (32 KB)
constexpr int DL_RB_MAX = 64;                      // most rows staged at once
constexpr int DL_GMAX = 256;                       // most slabs of a backward: one workgroup per CU
constexpr int DL_MIN_SHARE = 8;                    // fewest rows worth a slab of their own

struct DlDims { int B, L, C, S, P, Lp, k; };

// unit u of group cg -> (window, channel).  grouped (the individual mode's backward): the group is the channel, the unit the window.
__device__ __forceinline__ void dl_unit(const DlDims& d, int grouped, int cg, int u, int& b, int& c) {
    if (grouped) { b = u; c = cg; }
    else { b = u / d.C; c = u - b * d.C; }
}

// Stages units u0 .. u0+nr of group cg: seas -> xs, trend -> tr, times -> tv (each [nr][S]), mean / std -> st[i], st[DL_RB_MAX + i].
// FWD: the statistics are computed and written to mean / stdev (B, C); otherwise they are read from there (what the forward left).
// Every thread of the workgroup calls it; it ends behind a barrier.
template <bool FWD>
__device__ __forceinline__ void dl_stage(const DlDims& d, int grouped, int cg, int u0, int nr, const float* __restrict__ data,
                                         const float* __restrict__ mask, const float* __restrict__ tp, float* mean, float* stdev,
                                         float* xs, float* tr, float* tv, float* st) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = d.S, L = d.L, C = d.C;
    for (int i = wave; i < nr; i += DL_THREADS / 64) {      // a wave per row: the trip count is wave-uniform
        int b, c;
        dl_unit(d, grouped, cg, u0 + i, b, c);
        const size_t base = (size_t)b * L * C + c, row = (size_t)b * C + c;
        float mu, sd;
        if constexpr (FWD) {
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
            for (int l = lane; l < L; l += 64) {            // rows l >= L are padding: mask 0, no term
                const float mv = mask[base + (size_t)l * C];
                s0 += mv;
                s1 += data[base + (size_t)l * C] * mv;
            }
            s0 = wave_sum(s0);
            s1 = wave_sum(s1);
            const float cnt = fmaxf(s0, 1.f);
            mu = s1 / cnt;
            for (int l = lane; l < L; l += 64) {
                const float mv = mask[base + (size_t)l * C];
                const float q = (data[base + (size_t)l * C] * mv - mu) * mv;
                s2 += q * q;
            }
            s2 = wave_sum(s2);
            sd = sqrtf(s2 / cnt + 1e-5f);
            if (lane == 0) { mean[row] = mu; stdev[row] = sd; }
        } else {
            mu = mean[row];
            sd = stdev[row];
        }
        if (lane == 0) { st[i] = mu; st[DL_RB_MAX + i] = sd; }
        for (int l = lane; l < S; l += 64) {
            const bool in = l < L;
            const float x = in ? data[base + (size_t)l * C] * mask[base + (size_t)l * C] : 0.f;
            xs[i * S + l] = (x - mu) / sd;
            tv[i * S + l] = in ? tp[(size_t)b * L + l] : 0.f;
        }
    }
    __syncthreads();
    const int half = (d.k - 1) / 2;
    for (int idx = tid; idx < nr * S; idx += DL_THREADS) {
        const int i = idx / S, l = idx - i * S;
        const float* x = xs + i * S;
        const int lo = max(l - half, 0), hi = min(l + half, S - 1);
        float s = 0.f;
        for (int j = lo; j <= hi; ++j) s += x[j];
        // the replicate padding: row 0 stands for the half - l positions left of the series, row S-1 for those right of it
        s += (float)max(half - l, 0) * x[0] + (float)max(l + half - (S - 1), 0) * x[S - 1];
        tr[idx] = s / (float)d.k;
    }
    __syncthreads();
    for (int idx = tid; idx < nr * S; idx += DL_THREADS) xs[idx] -= tr[idx];
    __syncthreads();
}

__global__ __launch_bounds__(DL_THREADS) void dlinear_fwd_kernel(DlDims d, int individual, int rows, int RB, const float* __restrict__ data,
                                                                 const float* __restrict__ mask, const float* __restrict__ tp,
                                                                 const float* const* __restrict__ params, float* __restrict__ y,
                                                                 float* __restrict__ mean, float* __restrict__ stdev) {
    __shared__ float lds[DL_LDS + 2 * DL_RB_MAX];
    const int S = d.S, Lp = d.Lp, C = d.C;
    float *xs = lds, *tr = lds + RB * S, *tv = lds + 2 * RB * S, *st = lds + DL_LDS;
    const int u0 = blockIdx.x * RB, nr = min(RB, rows - u0);
    dl_stage<true>(d, 0, 0, u0, nr, data, mask, tp, mean, stdev, xs, tr, tv, st);
    const int NG = individual ? C : 1;
    for (int item = threadIdx.x; item < nr * Lp; item += DL_THREADS) {
        const int i = item / Lp, p = item - i * Lp;
        const int r = u0 + i, b = r / C, c = r - b * C, g = individual ? c : 0;
        const float* ws = params[g] + (size_t)p * S;
        const float* wt = params[NG + g] + (size_t)p * S;
        const float* wu = params[2 * NG + g] + (size_t)p * S;
        const float *x = xs + i * S, *t = tr + i * S, *u = tv + i * S;
        float as = 0.f, at = 0.f, au = 0.f;
        for (int l = 0; l < S; ++l) {
            as = fmaf(ws[l], x[l], as);
            at = fmaf(wt[l], t[l], at);
            au = fmaf(wu[l], u[l], au);
        }
        const float out = ((as + params[3 * NG + g][p]) + (at + params[4 * NG + g][p])) + (au + params[5 * NG + g][p]);
        y[((size_t)b * Lp + p) * C + c] = out * st[DL_RB_MAX + i] + st[i];
    }
}

// grid (Gb, groups): workgroup (g, cg) takes units g share .. min(n, (g + 1) share) of group cg into slab (cg Gb + g): [3][P S] + [P]
__global__ __launch_bounds__(DL_THREADS) void dlinear_bwd_kernel(DlDims d, int grouped, int n, int share, int RB,
                                                                 const float* __restrict__ data, const float* __restrict__ mask,
                                                                 const float* __restrict__ tp, const float* __restrict__ mean,
                                                                 const float* __restrict__ stdev, const float* __restrict__ dY,
                                                                 float* __restrict__ slabs) {
    __shared__ float lds[DL_LDS + 2 * DL_RB_MAX];
    const int tid = threadIdx.x, S = d.S, P = d.P, Lp = d.Lp, C = d.C, PS = P * S, NV = 3 * PS + P;
    float *xs = lds, *tr = lds + RB * S, *tv = lds + 2 * RB * S, *dO = lds + 3 * RB * S, *st = lds + DL_LDS;
    const int cg = blockIdx.y;
    float* slab = slabs + ((size_t)cg * gridDim.x + blockIdx.x) * NV;
    const int ubeg = blockIdx.x * share, uend = min(n, ubeg + share);
    for (int u0 = ubeg; u0 < uend; u0 += RB) {
        const int nr = min(RB, uend - u0);
        const bool first = u0 == ubeg;
        dl_stage<false>(d, grouped, cg, u0, nr, data, mask, tp, const_cast<float*>(mean), const_cast<float*>(stdev), xs, tr, tv, st);
        for (int idx = tid; idx < nr * P; idx += DL_THREADS) {
            const int i = idx / P, p = idx - i * P;
            int b, c;
            dl_unit(d, grouped, cg, u0 + i, b, c);
            dO[idx] = p < Lp ? dY[((size_t)b * Lp + p) * C + c] * st[DL_RB_MAX + i] : 0.f;      // rows p >= Lp were sliced off
        }
        __syncthreads();
        for (int e = tid; e < PS; e += DL_THREADS) {
            const int p = e / S, l = e - p * S;
            float as = 0.f, at = 0.f, au = 0.f;
            for (int i = 0; i < nr; ++i) {
                const float o = dO[i * P + p];
                as = fmaf(o, xs[i * S + l], as);
                at = fmaf(o, tr[i * S + l], at);
                au = fmaf(o, tv[i * S + l], au);
            }
            if (first) { slab[e] = as; slab[PS + e] = at; slab[2 * PS + e] = au; }
            else { slab[e] += as; slab[PS + e] += at; slab[2 * PS + e] += au; }
        }
        for (int p = tid; p < P; p += DL_THREADS) {
            float s = 0.f;
            for (int i = 0; i < nr; ++i) s += dO[i * P + p];
            if (first) slab[3 * PS + p] = s;
            else slab[3 * PS + p] += s;
        }
        __syncthreads();      // the next chunk overwrites the staged rows
    }
}

// grid (cdiv(NV, 256), groups): gradient entry i of group cg = its Gb slabs added in index order (four interleaved chains)
__global__ __launch_bounds__(DL_THREADS) void dlinear_fold_kernel(int P, int S, int Gb, const float* __restrict__ slabs, float* __restrict__ dWs,
                                                                  float* __restrict__ dWt, float* __restrict__ dWu, float* __restrict__ dbs,
                                                                  float* __restrict__ dbt, float* __restrict__ dbu) {
    const int PS = P * S, NV = 3 * PS + P, cg = blockIdx.y;
    const int i = blockIdx.x * DL_THREADS + threadIdx.x;
    if (i >= NV) return;
    const float* s = slabs + (size_t)cg * Gb * NV + i;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int g = 0;
    for (; g + 3 < Gb; g += 4) {
        a0 += s[(size_t)g * NV];
        a1 += s[(size_t)(g + 1) * NV];
        a2 += s[(size_t)(g + 2) * NV];
        a3 += s[(size_t)(g + 3) * NV];
    }
    for (; g < Gb; ++g) a0 += s[(size_t)g * NV];
    const float a = (a0 + a1) + (a2 + a3);
    if (i < PS) dWs[(size_t)cg * PS + i] = a;
    else if (i < 2 * PS) dWt[(size_t)cg * PS + i - PS] = a;
    else if (i < 3 * PS) dWu[(size_t)cg * PS + i - 2 * PS] = a;
    else {
        const size_t o = (size_t)cg * P + i - 3 * PS;
        dbs[o] = a;
        dbt[o] = a;
        dbu[o] = a;
    }
}

struct DlPlan { int groups, n, Gb, share, RB; };

inline bool dl_dims_ok(int64_t B, int L, int C, int S, int P, int Lp, int k, int individual) {
    return B >= 0 && L >= 0 && L <= S && Lp >= 0 && Lp <= P && immtsf_dlinear_supported(S, P, C, k, individual) &&
           B * (int64_t)C < (1ll << 31);
}

// how the backward deals its rows (host arithmetic only: the workspace query shares it)
inline DlPlan dl_plan(int B, int S, int P, int C, int individual) {
    DlPlan pl;
    pl.groups = individual ? C : 1;
    pl.n = individual ? B : B * C;
    const int gmax = DL_GMAX / pl.groups > 1 ? DL_GMAX / pl.groups : 1;
    int Gb = cdiv(pl.n, DL_MIN_SHARE);
    Gb = Gb < 1 ? 1 : (Gb > gmax ? gmax : Gb);
    pl.share = cdiv(pl.n > 0 ? pl.n : 1, Gb);
    pl.Gb = cdiv(pl.n > 0 ? pl.n : 1, pl.share);
    const int rb = DL_LDS / (3 * S + P);
    pl.RB = rb > DL_RB_MAX ? DL_RB_MAX : rb;
    return pl;
}

}  // namespace

extern "C" {

int immtsf_dlinear_supported(int32_t S, int32_t P, int32_t C, int32_t k, int32_t individual) {
    if (individual && C > 65535) return 0;      // a grid row per channel in the backward
    return S >= 1 && S <= DL_MAX_S && P >= 1 && P <= DL_MAX_P && C >= 1 && k >= 1 && k <= DL_MAX_K && (k & 1) ? 1 : 0;
}

size_t immtsf_dlinear_workspace_bytes(int32_t B, int32_t S, int32_t P, int32_t C, int32_t individual) {
    if (B < 1 || !immtsf_dlinear_supported(S, P, C, 1, individual) || (int64_t)B * C >= (1ll << 31)) return 0;
    const DlPlan pl = dl_plan(B, S, P, C, individual);
    return (size_t)pl.groups * pl.Gb * (3 * (size_t)P * S + P) * sizeof(float) + 256;
}

int immtsf_dlinear_forward(int32_t B, int32_t L, int32_t C, int32_t S, int32_t P, int32_t Lp, int32_t k, int32_t individual,
                           const float* data, const float* mask, const float* tp, const float* const* params, float* y, float* mean,
                           float* stdev, immtsf_stream_t stream) {
    if (S < 1 || P < 1 || C < 1 || k < 1) return IMMTSF_EINVAL;
    if (!immtsf_dlinear_supported(S, P, C, k, individual)) return IMMTSF_EUNSUPPORTED;
    if (!dl_dims_ok(B, L, C, S, P, Lp, k, individual)) return IMMTSF_EINVAL;
    if (B == 0) return IMMTSF_OK;
    if (!params || !mean || !stdev || (L > 0 && (!data || !mask || !tp)) || (Lp > 0 && !y)) return IMMTSF_EINVAL;
    const int rows = B * C;
    int RB = DL_LDS / (3 * S);
    RB = RB > DL_RB_MAX ? DL_RB_MAX : RB;
    const int want = cdiv(rows, 512);      // small batches: a row or two per workgroup, spread over the chip
    RB = want < RB ? want : RB;
    const DlDims d{B, L, C, S, P, Lp, k};
    hipLaunchKernelGGL(dlinear_fwd_kernel, dim3(cdiv(rows, RB)), dim3(DL_THREADS), 0, static_cast<hipStream_t>(stream), d, individual ? 1 : 0,
                       rows, RB, data, mask, tp, params, y, mean, stdev);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_dlinear_backward(int32_t B, int32_t L, int32_t C, int32_t S, int32_t P, int32_t Lp, int32_t k, int32_t individual,
                            const float* data, const float* mask, const float* tp, const float* mean, const float* stdev, const float* dY,
                            float* dWs, float* dWt, float* dWtau, float* dbs, float* dbt, float* dbtau, void* workspace,
                            size_t workspace_bytes, immtsf_stream_t stream) {
    if (S < 1 || P < 1 || C < 1 || k < 1) return IMMTSF_EINVAL;
    if (!immtsf_dlinear_supported(S, P, C, k, individual)) return IMMTSF_EUNSUPPORTED;
    if (!dl_dims_ok(B, L, C, S, P, Lp, k, individual) || B < 1) return IMMTSF_EINVAL;
    if (!mean || !stdev || !dWs || !dWt || !dWtau || !dbs || !dbt || !dbtau || !workspace || (L > 0 && (!data || !mask || !tp)) ||
        (Lp > 0 && !dY))
        return IMMTSF_EINVAL;
    if (workspace_bytes < immtsf_dlinear_workspace_bytes(B, S, P, C, individual)) return IMMTSF_EWORKSPACE;
    float* slabs = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t(255));
    const DlPlan pl = dl_plan(B, S, P, C, individual);
    const DlDims d{B, L, C, S, P, Lp, k};
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(dlinear_bwd_kernel, dim3(pl.Gb, pl.groups), dim3(DL_THREADS), 0, s, d, individual ? 1 : 0, pl.n, pl.share, pl.RB, data,
                       mask, tp, mean, stdev, dY, slabs);
    IMMTSF_LAUNCH_CHECK();
    hipLaunchKernelGGL(dlinear_fold_kernel, dim3(cdiv(3 * P * S + P, DL_THREADS), pl.groups), dim3(DL_THREADS), 0, s, P, S, pl.Gb, slabs, dWs,
                       dWt, dWtau, dbs, dbt, dbtau);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
