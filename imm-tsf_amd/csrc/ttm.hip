// TTM's narrow mixer blocks (reference layers/MLP.py, TTMMixerBlock in mode "patch" / "channel") as ONE launch forward and TWO backward,
// and the feature mixer's gate + residual as one launch per direction.  All fp32.
//
// Narrow block.  x is a contiguous (outer, F, inner, D) tensor; the F values along the mixed axis at one (group g = outer index * inner +
// inner index, column c < D) are F floats inner * D apart.  patch mode: x (B, M, N', D') read as (B M, N', 1, D'), F = N'; channel mode:
// x (B, M, N', D') as it stands, F = M.  Per (g, c), with xn = LayerNorm_D(x; gamma, beta, eps):
//   v[f] = xn[g, f, c];  h = drop1(gelu(W1 v + b1)) (2F);  u = drop2(W2 h + b2) (F);  a = softmax_F(Wg u + bg);  out = x + u a
// No permuted copy exists: a thread owns a column, its F values live in registers, the weights (5 F^2 + 4 F floats, zero-padded to the
// template's FM) in LDS, read as broadcast float4.  A workgroup takes a chunk of nG groups (nG D <= 256 where D < 256): a wave per
// (group, f) row for the LayerNorm statistics (two passes, in LDS), then a thread per column.
//
// Dropout (training, p > 0): Philox (common.hpp), key seed (+ the device counter), two sites.
//   site     (drop1): element ((g D + c) S1 + j), j < 2F, S1 = 2F rounded up to a multiple of 4
//   site + 1 (drop2): element ((g D + c) S2 + o), o < F,  S2 = F rounded up to a multiple of 4
// so that a column's draws start on a Philox call; the padding elements are drawn by nobody.  The backward redraws the same bits.
//
// Backward: a workgroup walks a contiguous share of the chunks.  Per chunk it recomputes the statistics and, CP columns at a time (one
// per thread), the forward of each column from x; the per-column vectors the parameter gradients are outer products of (h, du, u, dz,
// dpre, v, the LayerNorm terms) go through an LDS staging buffer [row][CP + 1] and every gradient entry has ONE owner thread that sums
// its columns in index order into the workgroup's slab (the first chunk writes: nothing is zero-filled).  The gradient of the
// normalised rows goes to dx, and once a chunk's columns are done a wave per row finishes the LayerNorm backward (its two row sums over
// D) in place and adds dout.  The second launch folds the slabs in index order into the eight gradients.  No atomics: the same inputs
// give the same bits.
//
// LDS: weights + statistics <= 25 088 bytes (FM = 32), the backward's staging buffer (3F + 2 rows) brings a workgroup to <= 64 KB: two workgroups of 256
// threads per CU at every F.
//
// Gate row kernel: out = res + u softmax_d(g) per row of d, a wave per row looping over d; backward du = dout a,
// dg = a (dout u - sum a dout u) in one launch (dres = dout needs none).
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

constexpr int TT_THREADS = 256, TT_WAVES = TT_THREADS / 64, TT_MAXF = 32, TT_MAXG = 16, TT_MAXD = 65536, TT_MAX_SLABS = 512;
constexpr size_t TT_LDS_TOTAL = 64 * 1024;      // a workgroup's LDS, static + dynamic: what a launch gets without raising the limit
constexpr size_t TT_WS_BUDGET = 32u << 20;      // slabs: fewer workgroups beyond this

struct TtP { const float *gamma, *beta, *W1, *b1, *W2, *b2, *Wg, *bg; };
struct TtDrop { float p, inv_keep; uint64_t seed, site; };
struct TtDims {
    int F, D, inner, groups;      // groups = outer * inner
    int nG, nchunks;              // groups per chunk
    int CP;                       // columns per backward pass (the staging buffer's width)
    int S1q, S2q;                 // Philox calls per column at the two sites
    float eps;
};
struct TtFold { float* dst[8]; int off[9]; };      // slab order: W1 | b1 | W2 | b2 | Wg | bg | gamma | beta

template <int FM>
struct TtLds {
    float W1[2 * FM * FM];      // [j][f]
    float W2T[2 * FM * FM];     // [j][o] = W2[o][j]
    float Wg[FM * FM];          // [o][f]
    float b1[2 * FM], b2[FM], bg[FM];
    float st[TT_MAXG * FM * 2]; // (mean, 1 / std) of the chunk's rows
};

inline int tt_fm(int F) { return F <= 4 ? 4 : F <= 8 ? 8 : F <= 16 ? 16 : F <= 20 ? 20 : 32; }
inline size_t tt_static_bytes(int F) {
    switch (tt_fm(F)) {
        case 4: return sizeof(TtLds<4>);
        case 8: return sizeof(TtLds<8>);
        case 16: return sizeof(TtLds<16>);
        case 20: return sizeof(TtLds<20>);
        default: return sizeof(TtLds<32>);
    }
}
inline int tt_nv(int F, int D) { return 5 * F * F + 4 * F + 2 * D; }
inline size_t tt_stage_bytes(int F, int CP) { return (size_t)(3 * F + 2) * (CP + 1) * sizeof(float); }
inline int tt_cp(int F) {
    for (int cp = 256; cp > 64; cp >>= 1)
        if (tt_static_bytes(F) + tt_stage_bytes(F, cp) <= TT_LDS_TOTAL) return cp;
    return 64;
}
inline TtDims tt_dims(int64_t outer, int inner, int F, int D, float eps, bool bwd) {
    TtDims d{};
    d.F = F; d.D = D; d.inner = inner; d.groups = (int)(outer * inner); d.eps = eps;
    d.CP = tt_cp(F);
    int n = (bwd ? d.CP : TT_THREADS) / D;
    d.nG = n < 1 ? 1 : (n > TT_MAXG ? TT_MAXG : n);
    d.nchunks = cdiv(d.groups, d.nG);
    d.S1q = (2 * F + 3) / 4; d.S2q = (F + 3) / 4;
    return d;
}
struct TtPlan { int G, share; };
inline TtPlan tt_plan(const TtDims& d) {
    size_t gmax = TT_WS_BUDGET / ((size_t)tt_nv(d.F, d.D) * sizeof(float));
    gmax = gmax < 1 ? 1 : (gmax > TT_MAX_SLABS ? TT_MAX_SLABS : gmax);
    const int G = d.nchunks < (int)gmax ? d.nchunks : (int)gmax;
    TtPlan pl;
    pl.share = cdiv(d.nchunks, G);
    pl.G = cdiv(d.nchunks, pl.share);
    return pl;
}

__device__ __forceinline__ float tt_gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float tt_dgelu(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * expf(-0.5f * x * x);
}
__device__ __forceinline__ float tt_keep(uint32_t bits, const TtDrop& dr) {
    return (float)(bits >> 8) * (1.0f / 16777216.0f) >= dr.p ? dr.inv_keep : 0.f;
}
__device__ __forceinline__ size_t tt_base(const TtDims& d, int g) {
    const int o = g / d.inner, i = g - o * d.inner;
    return ((size_t)o * d.F * d.inner + i) * d.D;
}
__device__ __forceinline__ void tt_acc(float* slab, int e, float v, bool init) {
    if (init) slab[e] = v;
    else slab[e] += v;
}

template <int FM>
__device__ __forceinline__ void tt_load_weights(TtLds<FM>& L, const TtP& P, int F) {
    for (int i = threadIdx.x; i < 2 * FM * FM; i += TT_THREADS) {
        const int j = i / FM, f = i - j * FM;
        const bool ok = j < 2 * F && f < F;
        L.W1[i] = ok ? P.W1[j * F + f] : 0.f;
        L.W2T[i] = ok ? P.W2[f * 2 * F + j] : 0.f;
    }
    for (int i = threadIdx.x; i < FM * FM; i += TT_THREADS) {
        const int o = i / FM, f = i - o * FM;
        L.Wg[i] = (o < F && f < F) ? P.Wg[o * F + f] : 0.f;
    }
    for (int i = threadIdx.x; i < 2 * FM; i += TT_THREADS) L.b1[i] = i < 2 * F ? P.b1[i] : 0.f;
    for (int i = threadIdx.x; i < FM; i += TT_THREADS) {
        L.b2[i] = i < F ? P.b2[i] : 0.f;
        L.bg[i] = i < F ? P.bg[i] : 0.f;
    }
}

// (mean, 1 / std) over D of the ng F rows of the chunk that starts at group g0: a wave per row, two passes
template <int FM>
__device__ __forceinline__ void tt_stats(TtLds<FM>& L, const TtDims& d, int g0, int ng, const float* __restrict__ x) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t sF = (size_t)d.inner * d.D;
    for (int r = wave; r < ng * d.F; r += TT_WAVES) {
        const int gl = r / d.F, f = r - gl * d.F;
        const float* row = x + tt_base(d, g0 + gl) + (size_t)f * sF;
        float s = 0.f;
        for (int c = lane; c < d.D; c += 64) s += row[c];
        const float mean = wave_sum(s) / (float)d.D;
        float q = 0.f;
        for (int c = lane; c < d.D; c += 64) {
            const float t = row[c] - mean;
            q = fmaf(t, t, q);
        }
        q = wave_sum(q);
        if (lane == 0) {
            L.st[2 * r] = mean;
            L.st[2 * r + 1] = 1.f / sqrtf(q / (float)d.D + d.eps);
        }
    }
}

#define TT_DOT4(acc, W_, arr, q)                                                                                    \
    acc = fmaf((W_).x, (arr)[4 * (q)], fmaf((W_).y, (arr)[4 * (q) + 1], fmaf((W_).z, (arr)[4 * (q) + 2], fmaf((W_).w, (arr)[4 * (q) + 3], acc))))
#define TT_AXPY4(arr, W_, s, q)                           \
    do {                                                 \
        (arr)[4 * (q)] = fmaf((W_).x, s, (arr)[4 * (q)]);         \
        (arr)[4 * (q) + 1] = fmaf((W_).y, s, (arr)[4 * (q) + 1]); \
        (arr)[4 * (q) + 2] = fmaf((W_).z, s, (arr)[4 * (q) + 2]); \
        (arr)[4 * (q) + 3] = fmaf((W_).w, s, (arr)[4 * (q) + 3]); \
    } while (0)

// drop2's four multipliers of Philox call q of column col
__device__ __forceinline__ void tt_drop2(const TtDrop& dr, uint64_t col, int S2q, int q, float (&m)[4]) {
    const Philox4 r = philox4x32_10(dr.seed, dr.site + 1, col * S2q + q);
    m[0] = tt_keep(r.x, dr); m[1] = tt_keep(r.y, dr); m[2] = tt_keep(r.z, dr); m[3] = tt_keep(r.w, dr);
}

// one column forward: v -> u (after drop2), a (the gate's softmax; 0 beyond F).  hst: where h[j] goes (stride hs), the backward's
template <int FM, bool STAGE>
__device__ __forceinline__ void tt_col_fwd(const TtLds<FM>& L, const TtDims& d, const TtDrop& dr, uint64_t col, const float (&v)[FM],
                                           float (&u)[FM], float (&a)[FM], float* hst, int hs) {
    const int F = d.F;
#pragma unroll
    for (int o = 0; o < FM; ++o) u[o] = L.b2[o];
    Philox4 r{};
    for (int j = 0; j < 2 * F; ++j) {
        float acc = L.b1[j];
#pragma unroll
        for (int q = 0; q < FM / 4; ++q)
            if (4 * q < F) {
                const float4 w = *reinterpret_cast<const float4*>(&L.W1[j * FM + 4 * q]);
                TT_DOT4(acc, w, v, q);
            }
        float h = tt_gelu(acc);
        if (dr.p > 0.f) {
            if ((j & 3) == 0) r = philox4x32_10(dr.seed, dr.site, col * d.S1q + (j >> 2));
            const int l = j & 3;
            h *= tt_keep(l == 0 ? r.x : l == 1 ? r.y : l == 2 ? r.z : r.w, dr);
        }
        if (STAGE) hst[j * hs] = h;
#pragma unroll
        for (int q = 0; q < FM / 4; ++q)
            if (4 * q < F) {
                const float4 w = *reinterpret_cast<const float4*>(&L.W2T[j * FM + 4 * q]);
                TT_AXPY4(u, w, h, q);
            }
    }
    if (dr.p > 0.f) {
#pragma unroll
        for (int q = 0; q < FM / 4; ++q)
            if (4 * q < F) {
                float m[4];
                tt_drop2(dr, col, d.S2q, q, m);
                u[4 * q] *= m[0]; u[4 * q + 1] *= m[1]; u[4 * q + 2] *= m[2]; u[4 * q + 3] *= m[3];
            }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int o = 0; o < FM; ++o) {
        float acc = L.bg[o];
        if (o < F) {
#pragma unroll
            for (int q = 0; q < FM / 4; ++q)
                if (4 * q < F) {
                    const float4 w = *reinterpret_cast<const float4*>(&L.Wg[o * FM + 4 * q]);
                    TT_DOT4(acc, w, u, q);
                }
            mx = fmaxf(mx, acc);
        }
        a[o] = acc;
        __builtin_amdgcn_sched_barrier(0);      // one row's weights in flight at a time: hoisting all FM rows' LDS reads spills
    }
    float s = 0.f;
#pragma unroll
    for (int o = 0; o < FM; ++o) {
        a[o] = o < F ? expf(a[o] - mx) : 0.f;
        s += a[o];
    }
    const float inv = 1.f / s;
#pragma unroll
    for (int o = 0; o < FM; ++o) a[o] *= inv;
}

template <int FM>
__global__ __launch_bounds__(TT_THREADS, 2) void ttm_mixer_fwd_kernel(TtDims d, TtDrop dr, const uint64_t* __restrict__ seed_dev, TtP P,
                                                                   const float* __restrict__ x, float* __restrict__ out) {
    __shared__ __align__(16) TtLds<FM> L;
    if (dr.p > 0.f && seed_dev) dr.seed += *seed_dev;
    const int F = d.F, D = d.D;
    const size_t sF = (size_t)d.inner * D;
    tt_load_weights(L, P, F);
    for (int chunk = blockIdx.x; chunk < d.nchunks; chunk += gridDim.x) {
        const int g0 = chunk * d.nG, ng = min(d.nG, d.groups - g0);
        __syncthreads();      // the weights are in place; the last chunk's readers of the statistics are done
        tt_stats(L, d, g0, ng, x);
        __syncthreads();
        for (int it = threadIdx.x; it < ng * D; it += TT_THREADS) {
            const int gl = it / D, c = it - gl * D, g = g0 + gl;
            const size_t at = tt_base(d, g) + c;
            const float gam = P.gamma[c], bet = P.beta[c];
            float v[FM], u[FM], a[FM];
#pragma unroll
            for (int f = 0; f < FM; ++f)
                v[f] = f < F ? fmaf((x[at + f * sF] - L.st[2 * (gl * F + f)]) * L.st[2 * (gl * F + f) + 1], gam, bet) : 0.f;
            tt_col_fwd<FM, false>(L, d, dr, (uint64_t)g * D + c, v, u, a, nullptr, 0);
#pragma unroll
            for (int f = 0; f < FM; ++f)
                if (f < F) out[at + f * sF] = fmaf(u[f], a[f], x[at + f * sF]);
        }
    }
}

// sum over n columns of a[col] (b[col]) in index order
__device__ __forceinline__ float tt_colsum(const float* a, const float* b, int n) {
    float s = 0.f;
    if (b)
        for (int c = 0; c < n; ++c) s = fmaf(a[c], b[c], s);
    else
        for (int c = 0; c < n; ++c) s += a[c];
    return s;
}

// workgroup w: chunks w share .. min(nchunks, (w + 1) share) into slab w (NV floats)
template <int FM>
__global__ __launch_bounds__(TT_THREADS, 2) void ttm_mixer_bwd_kernel(TtDims d, TtDrop dr, const uint64_t* __restrict__ seed_dev, TtP P, int share,
                                                                   const float* __restrict__ x, const float* __restrict__ dout,
                                                                   float* __restrict__ dx, float* __restrict__ ws) {
    __shared__ __align__(16) TtLds<FM> L;
    extern __shared__ float S[];      // [3F + 2][CP + 1]
    if (dr.p > 0.f && seed_dev) dr.seed += *seed_dev;
    const int F = d.F, D = d.D, CP = d.CP, ld = CP + 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t sF = (size_t)d.inner * D;
    const int oW1 = 0, ob1 = 2 * F * F, oW2 = ob1 + 2 * F, ob2 = oW2 + 2 * F * F, oWg = ob2 + F, obg = oWg + F * F, oga = obg + F, obe = oga + D;
    float* slab = ws + (size_t)blockIdx.x * (obe + D);
    tt_load_weights(L, P, F);
    const int cbeg = blockIdx.x * share, cend = min(d.nchunks, cbeg + share);
    for (int chunk = cbeg; chunk < cend; ++chunk) {
        const bool first = chunk == cbeg;
        const int g0 = chunk * d.nG, ng = min(d.nG, d.groups - g0);
        __syncthreads();
        tt_stats(L, d, g0, ng, x);
        __syncthreads();
        for (int c0 = 0; c0 < D; c0 += CP) {      // D > CP: one group per chunk, CP of its columns per pass
            const int Dc = min(CP, D - c0), items = ng * Dc;
            const bool active = tid < items, init = first && c0 == 0;
            const int gl = active ? tid / Dc : 0, cl = tid - gl * Dc, c = c0 + cl, g = g0 + gl;
            const size_t at = tt_base(d, g) + c;
            const uint64_t col = (uint64_t)g * D + c;
            float v[FM], dup[FM];
            {
                float u[FM], a[FM], dz[FM];
                if (active) {
                    const float gam = P.gamma[c], bet = P.beta[c];
#pragma unroll
                    for (int f = 0; f < FM; ++f)
                        v[f] = f < F ? fmaf((x[at + f * sF] - L.st[2 * (gl * F + f)]) * L.st[2 * (gl * F + f) + 1], gam, bet) : 0.f;
                    tt_col_fwd<FM, true>(L, d, dr, col, v, u, a, S + tid, ld);      // rows 0 .. 2F-1 <- h
                    // out = x + u a, a = softmax(z), z = Wg u + bg
                    float dot = 0.f;      // (dout is read twice rather than kept: FM registers less)
#pragma unroll
                    for (int f = 0; f < FM; ++f) {
                        dup[f] = f < F ? dout[at + f * sF] : 0.f;
                        dot = fmaf(a[f], dup[f] * u[f], dot);
                    }
#pragma unroll
                    for (int f = 0; f < FM; ++f) {
                        dz[f] = a[f] * (dup[f] * u[f] - dot);
                        dup[f] *= a[f];
                    }
#pragma unroll
                    for (int o = 0; o < FM; ++o)
                        if (o < F) {
#pragma unroll
                            for (int q = 0; q < FM / 4; ++q)
                                if (4 * q < F) {
                                    const float4 w = *reinterpret_cast<const float4*>(&L.Wg[o * FM + 4 * q]);
                                    TT_AXPY4(dup, w, dz[o], q);
                                }
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    if (dr.p > 0.f) {      // u = drop2(W2 h + b2): the gradient of the undropped value
#pragma unroll
                        for (int q = 0; q < FM / 4; ++q)
                            if (4 * q < F) {
                                float m[4];
                                tt_drop2(dr, col, d.S2q, q, m);
                                dup[4 * q] *= m[0]; dup[4 * q + 1] *= m[1]; dup[4 * q + 2] *= m[2]; dup[4 * q + 3] *= m[3];
                            }
                    }
#pragma unroll
                    for (int o = 0; o < FM; ++o)
                        if (o < F) S[(2 * F + o) * ld + tid] = dup[o];
                }
                __syncthreads();
                for (int e = tid; e < 2 * F * F + F; e += TT_THREADS) {      // dW2 (o, j), db2 (o)
                    if (e < 2 * F * F) {
                        const int o = e / (2 * F), j = e - o * 2 * F;
                        tt_acc(slab, oW2 + e, tt_colsum(S + (2 * F + o) * ld, S + j * ld, items), init);
                    } else {
                        const int o = e - 2 * F * F;
                        tt_acc(slab, ob2 + o, tt_colsum(S + (2 * F + o) * ld, nullptr, items), init);
                    }
                }
                __syncthreads();
                if (active) {
#pragma unroll
                    for (int f = 0; f < FM; ++f)
                        if (f < F) {
                            S[f * ld + tid] = u[f];
                            S[(F + f) * ld + tid] = dz[f];
                        }
                }
            }
            __syncthreads();
            for (int e = tid; e < F * F + F; e += TT_THREADS) {      // dWg (o, f), dbg (o)
                if (e < F * F) {
                    const int o = e / F, f = e - o * F;
                    tt_acc(slab, oWg + e, tt_colsum(S + (F + o) * ld, S + f * ld, items), init);
                } else {
                    const int o = e - F * F;
                    tt_acc(slab, obg + o, tt_colsum(S + (F + o) * ld, nullptr, items), init);
                }
            }
            __syncthreads();
            if (active) {      // the hidden layer again, row by row: dpre -> rows 0 .. 2F-1, dv in registers
                float dv[FM];
#pragma unroll
                for (int f = 0; f < FM; ++f) dv[f] = 0.f;
                Philox4 r{};
                for (int j = 0; j < 2 * F; ++j) {
                    float acc = L.b1[j], dh = 0.f;
#pragma unroll
                    for (int q = 0; q < FM / 4; ++q)
                        if (4 * q < F) {
                            const float4 w = *reinterpret_cast<const float4*>(&L.W1[j * FM + 4 * q]);
                            TT_DOT4(acc, w, v, q);
                            const float4 w2 = *reinterpret_cast<const float4*>(&L.W2T[j * FM + 4 * q]);
                            TT_DOT4(dh, w2, dup, q);
                        }
                    if (dr.p > 0.f) {
                        if ((j & 3) == 0) r = philox4x32_10(dr.seed, dr.site, col * d.S1q + (j >> 2));
                        const int l = j & 3;
                        dh *= tt_keep(l == 0 ? r.x : l == 1 ? r.y : l == 2 ? r.z : r.w, dr);
                    }
                    const float dpre = dh * tt_dgelu(acc);
                    S[j * ld + tid] = dpre;
#pragma unroll
                    for (int q = 0; q < FM / 4; ++q)
                        if (4 * q < F) {
                            const float4 w = *reinterpret_cast<const float4*>(&L.W1[j * FM + 4 * q]);
                            TT_AXPY4(dv, w, dpre, q);
                        }
                }
                const float gam = P.gamma[c];
                float dg = 0.f, db = 0.f;
#pragma unroll
                for (int f = 0; f < FM; ++f)
                    if (f < F) {
                        const float xh = (x[at + f * sF] - L.st[2 * (gl * F + f)]) * L.st[2 * (gl * F + f) + 1];
                        S[(2 * F + f) * ld + tid] = v[f];
                        dg = fmaf(dv[f], xh, dg);
                        db += dv[f];
                        dx[at + f * sF] = dv[f] * gam;      // the gradient of the normalised value: finished per row below
                    }
                S[3 * F * ld + tid] = dg;
                S[(3 * F + 1) * ld + tid] = db;
            }
            __syncthreads();
            for (int e = tid; e < 2 * F * F + 2 * F + 2 * Dc; e += TT_THREADS) {      // dW1 (j, f), db1 (j), dgamma / dbeta (c0 + cl)
                if (e < 2 * F * F) {
                    const int j = e / F, f = e - j * F;
                    tt_acc(slab, oW1 + e, tt_colsum(S + j * ld, S + (2 * F + f) * ld, items), init);
                } else if (e < 2 * F * F + 2 * F) {
                    const int j = e - 2 * F * F;
                    tt_acc(slab, ob1 + j, tt_colsum(S + j * ld, nullptr, items), init);
                } else {
                    const int k = e - 2 * F * F - 2 * F, which = k / Dc, cc = k - which * Dc;
                    const float* row = S + (3 * F + which) * ld + cc;
                    float s = 0.f;
                    for (int q = 0; q < ng; ++q) s += row[q * Dc];
                    tt_acc(slab, (which ? obe : oga) + c0 + cc, s, first);
                }
            }
            __syncthreads();      // also: every column's dx store is visible to the workgroup
        }
        // LayerNorm backward per row: dx = dout + (g - mean(g) - xhat mean(g xhat)) / std, g = what the columns left in dx
        for (int r = wave; r < ng * F; r += TT_WAVES) {
            const int gl = r / F, f = r - gl * F;
            const size_t at = tt_base(d, g0 + gl) + (size_t)f * sF;
            const float mean = L.st[2 * r], rstd = L.st[2 * r + 1];
            float s1 = 0.f, s2 = 0.f;
            for (int c = lane; c < D; c += 64) {
                const float gv = dx[at + c];
                s1 += gv;
                s2 = fmaf(gv, (x[at + c] - mean) * rstd, s2);
            }
            s1 = wave_sum(s1) / (float)D;
            s2 = wave_sum(s2) / (float)D;
            for (int c = lane; c < D; c += 64) {
                const float xh = (x[at + c] - mean) * rstd;
                dx[at + c] = fmaf(rstd, dx[at + c] - s1 - xh * s2, dout[at + c]);
            }
        }
    }
}

// gradient entry i = the G slabs added in index order (four interleaved chains), written to the tensor that owns it
__global__ __launch_bounds__(TT_THREADS) void ttm_mixer_fold_kernel(int NV, int G, TtFold fo, const float* __restrict__ slabs) {
    const int i = blockIdx.x * TT_THREADS + threadIdx.x;
    if (i >= NV) return;
    const float* s = slabs + i;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int g = 0;
    for (; g + 3 < G; g += 4) {
        a0 += s[(size_t)g * NV];
        a1 += s[(size_t)(g + 1) * NV];
        a2 += s[(size_t)(g + 2) * NV];
        a3 += s[(size_t)(g + 3) * NV];
    }
    for (; g < G; ++g) a0 += s[(size_t)g * NV];
    int k = 0;
    while (k < 7 && i >= fo.off[k + 1]) ++k;
    if (fo.dst[k]) fo.dst[k][i - fo.off[k]] = (a0 + a1) + (a2 + a3);
}

// ---- gate + residual rows: a wave per row
__global__ __launch_bounds__(TT_THREADS) void ttm_gate_fwd_kernel(int64_t rows, int d, const float* __restrict__ res, const float* __restrict__ u,
                                                                  const float* __restrict__ g, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t r = (int64_t)blockIdx.x * TT_WAVES + wave; r < rows; r += (int64_t)gridDim.x * TT_WAVES) {
        const size_t at = (size_t)r * d;
        float mx = -INFINITY;
        for (int c = lane; c < d; c += 64) mx = fmaxf(mx, g[at + c]);
        mx = wave_max(mx);
        float s = 0.f;
        for (int c = lane; c < d; c += 64) s += expf(g[at + c] - mx);
        const float inv = 1.f / wave_sum(s);
        for (int c = lane; c < d; c += 64) out[at + c] = fmaf(u[at + c], expf(g[at + c] - mx) * inv, res[at + c]);
    }
}

__global__ __launch_bounds__(TT_THREADS) void ttm_gate_bwd_kernel(int64_t rows, int d, const float* __restrict__ u, const float* __restrict__ g,
                                                                  const float* __restrict__ dout, float* __restrict__ du,
                                                                  float* __restrict__ dg) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t r = (int64_t)blockIdx.x * TT_WAVES + wave; r < rows; r += (int64_t)gridDim.x * TT_WAVES) {
        const size_t at = (size_t)r * d;
        float mx = -INFINITY;
        for (int c = lane; c < d; c += 64) mx = fmaxf(mx, g[at + c]);
        mx = wave_max(mx);
        float s = 0.f, t = 0.f;
        for (int c = lane; c < d; c += 64) {
            const float e = expf(g[at + c] - mx);
            s += e;
            t = fmaf(e, dout[at + c] * u[at + c], t);
        }
        const float inv = 1.f / wave_sum(s), dot = wave_sum(t) * inv;
        for (int c = lane; c < d; c += 64) {
            const float a = expf(g[at + c] - mx) * inv, go = dout[at + c];
            du[at + c] = go * a;
            dg[at + c] = a * (go * u[at + c] - dot);
        }
    }
}

template <int FM>
void tt_launch_fwd(const TtDims& d, const TtDrop& dr, const uint64_t* seed_dev, const TtP& P, const float* x, float* out, hipStream_t s) {
    const int grid = d.nchunks < 2048 ? d.nchunks : 2048;
    hipLaunchKernelGGL(ttm_mixer_fwd_kernel<FM>, dim3(grid), dim3(TT_THREADS), 0, s, d, dr, seed_dev, P, x, out);
}
template <int FM>
void tt_launch_bwd(const TtDims& d, const TtDrop& dr, const uint64_t* seed_dev, const TtP& P, const TtPlan& pl, const float* x,
                   const float* dout, float* dx, float* ws, hipStream_t s) {
    hipLaunchKernelGGL(ttm_mixer_bwd_kernel<FM>, dim3(pl.G), dim3(TT_THREADS), tt_stage_bytes(d.F, d.CP), s, d, dr, seed_dev, P, pl.share, x,
                       dout, dx, ws);
}

inline bool tt_gate_ok(int64_t rows, int32_t d) { return rows >= 0 && d >= 1 && rows <= ((int64_t)1 << 40) / d; }
inline int tt_gate_grid(int64_t rows) {
    const int64_t n = (rows + TT_WAVES - 1) / TT_WAVES;
    return (int)(n < 8192 ? n : 8192);
}

}  // namespace

extern "C" {

int immtsf_ttm_mixer_supported(int32_t mode, int64_t outer, int32_t inner, int32_t F, int32_t D) {
    if ((mode != 0 && mode != 1) || outer < 1 || inner < 1 || (mode == 0 && inner != 1) || F < 1 || F > TT_MAXF || D < 1 || D > TT_MAXD) return 0;
    if (outer > (((int64_t)1 << 31) - 1) / ((int64_t)inner * F * D)) return 0;      // every element index fits an int32
    return tt_static_bytes(F) + tt_stage_bytes(F, tt_cp(F)) <= TT_LDS_TOTAL ? 1 : 0;
}

size_t immtsf_ttm_mixer_workspace_bytes(int32_t mode, int64_t outer, int32_t inner, int32_t F, int32_t D) {
    if (!immtsf_ttm_mixer_supported(mode, outer, inner, F, D)) return 0;
    const TtDims d = tt_dims(outer, inner, F, D, 0.f, true);
    return (size_t)tt_plan(d).G * tt_nv(F, D) * sizeof(float) + 256;
}

int immtsf_ttm_mixer_forward(int32_t mode, int64_t outer, int32_t inner, int32_t F, int32_t D, const float* x, const float* gamma,
                             const float* beta, const float* W1, const float* b1, const float* W2, const float* b2, const float* Wg,
                             const float* bg, float eps, float* out, float p_drop, uint64_t seed, uint64_t site, const uint64_t* seed_step_dev,
                             immtsf_stream_t stream) {
    if (!(p_drop >= 0.f && p_drop < 1.f) || !(eps >= 0.f)) return IMMTSF_EINVAL;
    if (!immtsf_ttm_mixer_supported(mode, outer, inner, F, D)) return IMMTSF_EUNSUPPORTED;
    if (!x || !out || !gamma || !beta || !W1 || !b1 || !W2 || !b2 || !Wg || !bg) return IMMTSF_EINVAL;
    const TtDims d = tt_dims(outer, inner, F, D, eps, false);
    const TtDrop dr{p_drop, 1.f / (1.f - p_drop), seed, site};
    const TtP P{gamma, beta, W1, b1, W2, b2, Wg, bg};
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (tt_fm(F)) {
        case 4: tt_launch_fwd<4>(d, dr, seed_step_dev, P, x, out, s); break;
        case 8: tt_launch_fwd<8>(d, dr, seed_step_dev, P, x, out, s); break;
        case 16: tt_launch_fwd<16>(d, dr, seed_step_dev, P, x, out, s); break;
        case 20: tt_launch_fwd<20>(d, dr, seed_step_dev, P, x, out, s); break;
        default: tt_launch_fwd<32>(d, dr, seed_step_dev, P, x, out, s); break;
    }
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_ttm_mixer_backward(int32_t mode, int64_t outer, int32_t inner, int32_t F, int32_t D, const float* x, const float* gamma,
                              const float* beta, const float* W1, const float* b1, const float* W2, const float* b2, const float* Wg,
                              const float* bg, float eps, const float* dout, float* dx, float* dgamma, float* dbeta, float* dW1, float* db1,
                              float* dW2, float* db2, float* dWg, float* dbg, float p_drop, uint64_t seed, uint64_t site,
                              const uint64_t* seed_step_dev, void* workspace, size_t workspace_bytes, immtsf_stream_t stream) {
    if (!(p_drop >= 0.f && p_drop < 1.f) || !(eps >= 0.f)) return IMMTSF_EINVAL;
    if (!immtsf_ttm_mixer_supported(mode, outer, inner, F, D)) return IMMTSF_EUNSUPPORTED;
    if (!x || !dout || !dx || dx == dout || !workspace || !gamma || !beta || !W1 || !b1 || !W2 || !b2 || !Wg || !bg) return IMMTSF_EINVAL;
    if (workspace_bytes < immtsf_ttm_mixer_workspace_bytes(mode, outer, inner, F, D)) return IMMTSF_EWORKSPACE;
    float* ws = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t(255));
    const TtDims d = tt_dims(outer, inner, F, D, eps, true);
    const TtPlan pl = tt_plan(d);
    const TtDrop dr{p_drop, 1.f / (1.f - p_drop), seed, site};
    const TtP P{gamma, beta, W1, b1, W2, b2, Wg, bg};
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (tt_fm(F)) {
        case 4: tt_launch_bwd<4>(d, dr, seed_step_dev, P, pl, x, dout, dx, ws, s); break;
        case 8: tt_launch_bwd<8>(d, dr, seed_step_dev, P, pl, x, dout, dx, ws, s); break;
        case 16: tt_launch_bwd<16>(d, dr, seed_step_dev, P, pl, x, dout, dx, ws, s); break;
        case 20: tt_launch_bwd<20>(d, dr, seed_step_dev, P, pl, x, dout, dx, ws, s); break;
        default: tt_launch_bwd<32>(d, dr, seed_step_dev, P, pl, x, dout, dx, ws, s); break;
    }
    IMMTSF_LAUNCH_CHECK();
    const int NV = tt_nv(F, D);
    TtFold fo;
    float* dst[8] = {dW1, db1, dW2, db2, dWg, dbg, dgamma, dbeta};
    const int len[8] = {2 * F * F, 2 * F, 2 * F * F, F, F * F, F, D, D};
    fo.off[0] = 0;
    for (int k = 0; k < 8; ++k) { fo.dst[k] = dst[k]; fo.off[k + 1] = fo.off[k] + len[k]; }
    hipLaunchKernelGGL(ttm_mixer_fold_kernel, dim3(cdiv(NV, TT_THREADS)), dim3(TT_THREADS), 0, s, NV, pl.G, fo, ws);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_ttm_gate_forward(int64_t rows, int32_t d, const float* res, const float* u, const float* g, float* out, immtsf_stream_t stream) {
    if (!tt_gate_ok(rows, d)) return IMMTSF_EINVAL;
    if (rows == 0) return IMMTSF_OK;
    if (!res || !u || !g || !out) return IMMTSF_EINVAL;
    hipLaunchKernelGGL(ttm_gate_fwd_kernel, dim3(tt_gate_grid(rows)), dim3(TT_THREADS), 0, static_cast<hipStream_t>(stream), rows, d, res, u, g,
                       out);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_ttm_gate_backward(int64_t rows, int32_t d, const float* u, const float* g, const float* dout, float* du, float* dg,
                             immtsf_stream_t stream) {
    if (!tt_gate_ok(rows, d)) return IMMTSF_EINVAL;
    if (rows == 0) return IMMTSF_OK;
    if (!u || !g || !dout || !du || !dg) return IMMTSF_EINVAL;
    hipLaunchKernelGGL(ttm_gate_bwd_kernel, dim3(tt_gate_grid(rows)), dim3(TT_THREADS), 0, static_cast<hipStream_t>(stream), rows, d, u, g, dout,
                       du, dg);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
