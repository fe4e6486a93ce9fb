// TimeMixer's forecasting() (reference models/TimeMixer.py:268-326) at the reference's default options -- moving-average decomposition
// with an odd window, channel independence, average pooling, window 2 -- as ONE launch forward and TWO launches backward, all fp32.
//
// Per window b, with scale lengths T_i = S >> i (i = 0..n), row offsets off_i = T_0 + .. + T_{i-1}, K = 2 C + 1:
//   pad L -> S with zeros; cnt = max(sum m, 1); mean = sum d m / cnt; xn = (d m - mean) / std, std = sqrt(sum ((d m - mean) m)^2 / cnt + 1e-5);
//   enc_0[t] = (xn[t, :], m[t, :], tp[t]); enc_{i+1}[t] = (enc_i[2t] + enc_i[2t+1]) / 2;
//   x_i[t, f] = (sum_{j<3,k<K} Wc[f,k,j] enc_i[(t+j-1) mod T_i, k] + pe[t, f]) keep(i, b, t, f)
//   e_layers blocks: trend_i = moving average of x_i over t (replicate padded), season_i = x_i - trend_i;
//     os_0 = season_0, os_{i+1} = season_{i+1} + MLP_i^s(os_i) over the time axis; ot_n = trend_n, ot_i = trend_i + MLP_i^t(ot_{i+1});
//     x_i += out_layer(os_i + ot_i) over the feature axis.  The LAST block does the coarsest x_n alone with ot_n = trend_n: nothing
//     else of it has a reader.  MLP = Linear, exact (erf) GELU, Linear.
//   dec[p, f] = bp[p] + sum_t Wp[p, t] x_n[t, f]; y[b, p, c] = (bo[c] + sum_f Wo[c, f] dec[p, f]) std_c + mean_c, p < Lp.
//
// Dropout (training, p > 0): Philox (common.hpp), one site, element index ((off_i B + b T_i + t) d + f): the scales' (B, T_i, d) arrays
// one after the other.  The backward redraws the same bits.
//
// A workgroup holds one window in LDS: x, season, trend as [sum T_i][d] rows, and a scratch region; weights come from global memory
// (every workgroup re-reads the same few thousand floats from L2).  Forward: a workgroup per window.
// Backward (parameter gradients only): windows are dealt to G <= 256 workgroups in contiguous shares.  A workgroup RECOMPUTES the
// forward of each of its windows with the same code, leaving what the chain rule needs (the pyramid, per block the mixed season / trend
// rows and the two chains' pre-GELU rows, the head's dec) in its own region of the workspace, then walks the chain backwards in LDS.
// Every gradient entry has one owner thread per step and the steps are separated by barriers, so a workgroup's slab is accumulated in
// window order without atomics (the first window writes: nothing is zero-filled); the fold launch adds the slabs in index order.
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

constexpr int TM_MAX_S = 64, TM_MAX_P = 64, TM_MAX_D = 32, TM_MAX_DFF = 64, TM_MAX_E = 4, TM_MAX_N = 6, TM_MAX_K = 64;
constexpr int TM_MAX_MA = (1 << 24) - 1;           // the clamped ends' counts stay exact in fp32
constexpr int TM_THREADS = 256;
constexpr int TM_LDS_BYTES = 160 * 1024;           // LDS of a CU: what one workgroup may declare at most
constexpr int TM_LDS_STATIC = 64 * 1024;           // what a launch gets without raising the function's dynamic-LDS attribute
constexpr int TM_GMAX = 256;                       // most slabs of a backward: one workgroup per CU
constexpr size_t TM_WS_BUDGET = 32u << 20;         // slabs + activation regions: fewer workgroups beyond this
constexpr int TM_MAX_PRM = 2 + TM_MAX_E * (8 * TM_MAX_N + 4) + 4;

struct TmDims {
    int B, L, C, S, P, Lp, d, dff, E, n, k, K, sumT, hsz;
    int T[TM_MAX_N + 1], off[TM_MAX_N + 1];
};
struct TmOff { int o[TM_MAX_PRM]; int NV; };       // slab offset of every table entry, -1: no gradient

// table entries
__host__ __device__ inline int tm_blk(const TmDims& d, int j) { return 2 + j * (8 * d.n + 4); }
__host__ __device__ inline int tm_seas(const TmDims& d, int j, int i) { return tm_blk(d, j) + 4 * i; }
__host__ __device__ inline int tm_trnd(const TmDims& d, int j, int i) { return tm_blk(d, j) + 4 * d.n + 4 * i; }
__host__ __device__ inline int tm_outl(const TmDims& d, int j) { return tm_blk(d, j) + 8 * d.n; }
__host__ __device__ inline int tm_head(const TmDims& d) { return tm_blk(d, d.E); }

inline TmDims tm_dims(int B, int L, int C, int S, int P, int Lp, int dm, int dff, int E, int n, int k) {
    TmDims d{};
    d.B = B; d.L = L; d.C = C; d.S = S; d.P = P; d.Lp = Lp; d.d = dm; d.dff = dff; d.E = E; d.n = n; d.k = k; d.K = 2 * C + 1;
    int o = 0;
    for (int i = 0; i <= n; ++i) { d.T[i] = S >> i; d.off[i] = o; o += d.T[i]; }
    d.sumT = o;
    int h = dm * S;
    if (P * dm > h) h = P * dm;
    if (2 * dff > h) h = 2 * dff;
    d.hsz = h;
    return d;
}
// LDS floats: x | region 2 = (season | trend | scratch), which the pyramid's two live scales alias while the embedding runs | mean, std
__host__ __device__ inline size_t tm_r2(const TmDims& d) {
    const size_t a = 2 * (size_t)d.sumT * d.d + d.hsz, b = (size_t)(d.T[0] + d.T[1]) * d.K;
    return a > b ? a : b;
}
inline size_t tm_lds_bytes(const TmDims& d) { return ((size_t)d.sumT * d.d + tm_r2(d) + 2 * d.C) * sizeof(float); }

inline TmOff tm_offsets(const TmDims& d) {
    TmOff f;
    for (int i = 0; i < TM_MAX_PRM; ++i) f.o[i] = -1;
    int nv = 0;
    auto put = [&](int e, int sz) { f.o[e] = nv; nv += sz; };
    put(0, d.d * d.K * 3);
    for (int j = 0; j < d.E; ++j) {
        for (int i = 0; i < d.n; ++i) {
            const int a = d.T[i], b = d.T[i + 1], e = tm_seas(d, j, i);
            put(e, b * a); put(e + 1, b); put(e + 2, b * b); put(e + 3, b);
        }
        if (j < d.E - 1)
            for (int i = 0; i < d.n; ++i) {
                const int a = d.T[i + 1], b = d.T[i], e = tm_trnd(d, j, i);
                put(e, b * a); put(e + 1, b); put(e + 2, b * b); put(e + 3, b);
            }
        const int e = tm_outl(d, j);
        put(e, d.dff * d.d); put(e + 1, d.dff); put(e + 2, d.d * d.dff); put(e + 3, d.d);
    }
    const int h = tm_head(d);
    put(h, d.P * d.T[d.n]); put(h + 1, d.P); put(h + 2, d.C * d.d); put(h + 3, d.C);
    f.NV = nv;
    return f;
}
// the backward's activation region of one workgroup (floats): pyramid | per block os, ot, season-chain and trend-chain pre-GELU rows | dec
inline size_t tm_act_floats(const TmDims& d) { return (size_t)d.sumT * d.K + (size_t)d.E * 4 * d.sumT * d.d + (size_t)d.P * d.d; }
struct TmPlan { int G, share; };
inline TmPlan tm_plan(const TmDims& d, int NV) {
    const size_t per = ((size_t)NV + tm_act_floats(d)) * sizeof(float);
    size_t gmax = TM_WS_BUDGET / per;
    gmax = gmax < 1 ? 1 : (gmax > TM_GMAX ? TM_GMAX : gmax);
    const int B = d.B > 0 ? d.B : 1;
    int G = B < (int)gmax ? B : (int)gmax;
    TmPlan pl;
    pl.share = cdiv(B, G);
    pl.G = cdiv(B, pl.share);
    return pl;
}

__device__ __forceinline__ float tm_gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float tm_dgelu(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}
__device__ __forceinline__ void tm_acc(float* slab, int e, float v, bool init) {
    if (init) slab[e] = v;
    else slab[e] += v;
}

// Linear(Tin -> Tout) GELU Linear(Tout -> Tout) over the time axis of buf's rows [oin, oin + Tin), added to rows [oout, oout + Tout).
// h1: where the pre-GELU rows [Tout][d] go (the backward's region), or null.  Ends behind a barrier.
__device__ __forceinline__ void tm_time_mlp(float* buf, int dm, int oin, int Tin, int oout, int Tout, const float* const* prm, int e, float* H,
                                            float* h1) {
    const float *W1 = prm[e], *b1 = prm[e + 1], *W2 = prm[e + 2], *b2 = prm[e + 3];
    for (int it = threadIdx.x; it < Tout * dm; it += TM_THREADS) {
        const int m = it / dm, f = it - m * dm;
        float a = b1[m];
        for (int t = 0; t < Tin; ++t) a = fmaf(W1[m * Tin + t], buf[(oin + t) * dm + f], a);
        if (h1) h1[it] = a;
        H[it] = tm_gelu(a);
    }
    __syncthreads();
    for (int it = threadIdx.x; it < Tout * dm; it += TM_THREADS) {
        const int o = it / dm, f = it - o * dm;
        float a = b2[o];
        for (int m = 0; m < Tout; ++m) a = fmaf(W2[o * Tout + m], H[m * dm + f], a);
        buf[(oout + o) * dm + f] += a;
    }
    __syncthreads();
}

// its backward: dbuf rows [oout ..) hold the gradient of the MLP's result; in / h1: the forward's input rows [Tin][d] and pre-GELU rows
// [Tout][d].  Adds the four parameter gradients to the slab and W1^T dh to dbuf rows [oin ..).  Ends behind a barrier.
__device__ __forceinline__ void tm_time_mlp_bwd(float* dbuf, int dm, int oin, int Tin, int oout, int Tout, const float* const* prm,
                                                const TmOff& po, int e, const float* in, const float* h1, float* H, float* slab, bool init) {
    const float *W1 = prm[e], *W2 = prm[e + 2];
    for (int it = threadIdx.x; it < Tout * dm; it += TM_THREADS) {
        const int m = it / dm, f = it - m * dm;
        float a = 0.f;
        for (int o = 0; o < Tout; ++o) a = fmaf(W2[o * Tout + m], dbuf[(oout + o) * dm + f], a);
        H[it] = a * tm_dgelu(h1[it]);
    }
    __syncthreads();
    float* s;
    s = slab + po.o[e + 2];
    for (int it = threadIdx.x; it < Tout * Tout; it += TM_THREADS) {
        const int o = it / Tout, m = it - o * Tout;
        float a = 0.f;
        for (int f = 0; f < dm; ++f) a = fmaf(dbuf[(oout + o) * dm + f], tm_gelu(h1[m * dm + f]), a);
        tm_acc(s, it, a, init);
    }
    s = slab + po.o[e];
    for (int it = threadIdx.x; it < Tout * Tin; it += TM_THREADS) {
        const int m = it / Tin, t = it - m * Tin;
        float a = 0.f;
        for (int f = 0; f < dm; ++f) a = fmaf(H[m * dm + f], in[t * dm + f], a);
        tm_acc(s, it, a, init);
    }
    for (int it = threadIdx.x; it < 2 * Tout; it += TM_THREADS) {
        const bool second = it >= Tout;
        const int m = second ? it - Tout : it;
        const float* src = second ? dbuf + (oout + m) * dm : H + m * dm;
        float a = 0.f;
        for (int f = 0; f < dm; ++f) a += src[f];
        tm_acc(slab + po.o[second ? e + 3 : e + 1], m, a, init);
    }
    for (int it = threadIdx.x; it < Tin * dm; it += TM_THREADS) {
        const int t = it / dm, f = it - t * dm;
        float a = 0.f;
        for (int m = 0; m < Tout; ++m) a = fmaf(W1[m * Tin + t], H[m * dm + f], a);
        dbuf[(oin + t) * dm + f] += a;
    }
    __syncthreads();
}

// how many positions of the replicate-padded window around row m land on row l of a series of T rows (half = (k - 1) / 2)
__device__ __forceinline__ int tm_ma_count(int m, int l, int T, int half) {
    if (T == 1) return 2 * half + 1;
    int c = (l >= m - half && l <= m + half) ? 1 : 0;
    if (l == 0) c += max(half - m, 0);
    if (l == T - 1) c += max(m + half - (T - 1), 0);
    return c;
}

struct TmDrop { float p, inv_keep; uint64_t seed, site; };

// The forward of window b in LDS.  act: the workgroup's activation region (backward) or null (forward).  On return X rows off_n .. hold
// the final coarsest scale, H holds dec [P][d], st the mean / std of the C channels; behind a barrier.
__device__ __forceinline__ void tm_forward_window(const TmDims& d, int b, const float* __restrict__ data, const float* __restrict__ mask,
                                                  const float* __restrict__ tp, const float* const* __restrict__ prm, const TmDrop& dr,
                                                  float* X, float* R2, float* st, float* act) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = d.S, L = d.L, C = d.C, K = d.K, dm = d.d, n = d.n, SD = d.sumT * d.d;
    float *Sx = R2, *Tx = R2 + SD, *H = R2 + 2 * SD;
    for (int c = wave; c < C; c += TM_THREADS / 64) {       // a wave per channel: the trip count is wave-uniform
        const size_t base = (size_t)b * L * C + c;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int l = lane; l < L; l += 64) {                // rows l >= L are padding: mask 0, no term
            const float mv = mask[base + (size_t)l * C];
            s0 += mv;
            s1 += data[base + (size_t)l * C] * mv;
        }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        const float cnt = fmaxf(s0, 1.f), mu = s1 / cnt;
        for (int l = lane; l < L; l += 64) {
            const float mv = mask[base + (size_t)l * C];
            const float q = (data[base + (size_t)l * C] * mv - mu) * mv;
            s2 += q * q;
        }
        s2 = wave_sum(s2);
        if (lane == 0) { st[c] = mu; st[C + c] = sqrtf(s2 / cnt + 1e-5f); }
    }
    __syncthreads();
    float* enc = R2;                                        // scale i's rows [T_i][K]; the next scale's go behind them, then swap
    float* nxt = R2 + S * K;
    for (int it = tid; it < S * K; it += TM_THREADS) {
        const int t = it / K, c = it - t * K;
        const bool in = t < L;
        float v;
        if (c < C) v = ((in ? data[((size_t)b * L + t) * C + c] * mask[((size_t)b * L + t) * C + c] : 0.f) - st[c]) / st[C + c];
        else if (c < 2 * C) v = in ? mask[((size_t)b * L + t) * C + c - C] : 0.f;
        else v = in ? tp[(size_t)b * L + t] : 0.f;
        enc[it] = v;
    }
    __syncthreads();
    const float *Wc = prm[0], *pe = prm[1];
    for (int i = 0; i <= n; ++i) {
        const int T = d.T[i];
        for (int it = tid; it < T * dm; it += TM_THREADS) {
            const int t = it / dm, f = it - t * dm;
            const float* r0 = enc + (t == 0 ? T - 1 : t - 1) * K;
            const float* r1 = enc + t * K;
            const float* r2 = enc + (t == T - 1 ? 0 : t + 1) * K;
            const float* w = Wc + (size_t)f * K * 3;
            float a = 0.f;
            for (int c = 0; c < K; ++c) a = fmaf(w[3 * c], r0[c], fmaf(w[3 * c + 1], r1[c], fmaf(w[3 * c + 2], r2[c], a)));
            a += pe[t * dm + f];
            if (dr.p > 0.f) a *= dropout_scale(dr.seed, dr.site, (((uint64_t)d.off[i] * d.B + (uint64_t)b * T + t) * dm + f), dr.p, dr.inv_keep);
            X[(d.off[i] + t) * dm + f] = a;
        }
        if (act)
            for (int it = tid; it < T * K; it += TM_THREADS) act[d.off[i] * K + it] = enc[it];
        if (i < n) {
            const int Tn = d.T[i + 1];
            for (int it = tid; it < Tn * K; it += TM_THREADS) {
                const int t = it / K, c = it - t * K;
                nxt[it] = 0.5f * (enc[(2 * t) * K + c] + enc[(2 * t + 1) * K + c]);
            }
        }
        __syncthreads();
        float* sw = enc; enc = nxt; nxt = sw;
    }
    const int half = (d.k - 1) / 2;
    float* ablk = act ? act + (size_t)d.sumT * K : nullptr;
    for (int j = 0; j < d.E; ++j, ablk = ablk ? ablk + 4 * (size_t)SD : nullptr) {
        const bool last = j == d.E - 1;
        for (int it = tid; it < SD; it += TM_THREADS) {
            const int r = it / dm, f = it - r * dm;
            int i = 0;
            while (i < n && r >= d.off[i + 1]) ++i;
            const int T = d.T[i], l = r - d.off[i];
            const float* x = X + d.off[i] * dm + f;
            const int lo = max(l - half, 0), hi = min(l + half, T - 1);
            float s = 0.f;
            for (int q = lo; q <= hi; ++q) s += x[q * dm];
            // the replicate padding: row 0 stands for the half - l positions left of the series, row T-1 for those right of it
            s += (float)max(half - l, 0) * x[0] + (float)max(l + half - (T - 1), 0) * x[(T - 1) * dm];
            s /= (float)d.k;
            Tx[it] = s;
            Sx[it] = X[it] - s;
        }
        __syncthreads();
        for (int i = 0; i < n; ++i)
            tm_time_mlp(Sx, dm, d.off[i], d.T[i], d.off[i + 1], d.T[i + 1], prm, tm_seas(d, j, i), H, ablk ? ablk + 2 * SD + d.off[i + 1] * dm : nullptr);
        if (!last)
            for (int i = n - 1; i >= 0; --i)
                tm_time_mlp(Tx, dm, d.off[i + 1], d.T[i + 1], d.off[i], d.T[i], prm, tm_trnd(d, j, i), H, ablk ? ablk + 3 * SD + d.off[i] * dm : nullptr);
        if (ablk)
            for (int it = tid; it < SD; it += TM_THREADS) { ablk[it] = Sx[it]; ablk[SD + it] = Tx[it]; }
        const int e = tm_outl(d, j), dff = d.dff, RC = d.hsz / dff;
        const float *W1 = prm[e], *b1 = prm[e + 1], *W2 = prm[e + 2], *b2 = prm[e + 3];
        const int rbeg = last ? d.off[n] : 0;
        for (int r0 = rbeg; r0 < d.sumT; r0 += RC) {
            const int nr = min(RC, d.sumT - r0);
            for (int it = tid; it < nr * dff; it += TM_THREADS) {
                const int rr = it / dff, q = it - rr * dff;
                const float *sx = Sx + (r0 + rr) * dm, *tx = Tx + (r0 + rr) * dm;
                float a = b1[q];
                for (int f = 0; f < dm; ++f) a = fmaf(W1[q * dm + f], sx[f] + tx[f], a);
                H[it] = tm_gelu(a);
            }
            __syncthreads();
            for (int it = tid; it < nr * dm; it += TM_THREADS) {
                const int rr = it / dm, f = it - rr * dm;
                float a = b2[f];
                for (int q = 0; q < dff; ++q) a = fmaf(W2[f * dff + q], H[rr * dff + q], a);
                X[(r0 + rr) * dm + f] += a;
            }
            __syncthreads();
        }
    }
    const int hd = tm_head(d), Tn = d.T[n];
    const float *Wp = prm[hd], *bp = prm[hd + 1];
    for (int it = tid; it < d.P * dm; it += TM_THREADS) {
        const int p = it / dm, f = it - p * dm;
        float a = bp[p];
        for (int t = 0; t < Tn; ++t) a = fmaf(Wp[p * Tn + t], X[(d.off[n] + t) * dm + f], a);
        H[it] = a;
        if (act) act[(size_t)d.sumT * K + (size_t)d.E * 4 * SD + it] = a;
    }
    __syncthreads();
}

__global__ __launch_bounds__(TM_THREADS) void timemixer_fwd_kernel(TmDims d, TmDrop dr, const uint64_t* __restrict__ seed_dev,
                                                                   const float* __restrict__ data, const float* __restrict__ mask,
                                                                   const float* __restrict__ tp, const float* const* __restrict__ prm,
                                                                   float* __restrict__ y) {
    extern __shared__ float lds[];
    float *X = lds, *R2 = lds + d.sumT * d.d, *st = R2 + tm_r2(d);
    if (dr.p > 0.f && seed_dev) dr.seed += *seed_dev;
    const int b = blockIdx.x;
    tm_forward_window(d, b, data, mask, tp, prm, dr, X, R2, st, nullptr);
    const float* H = R2 + 2 * d.sumT * d.d;
    const int hd = tm_head(d), C = d.C, dm = d.d;
    const float *Wo = prm[hd + 2], *bo = prm[hd + 3];
    for (int it = threadIdx.x; it < d.Lp * C; it += TM_THREADS) {
        const int p = it / C, c = it - p * C;
        float a = bo[c];
        for (int f = 0; f < dm; ++f) a = fmaf(Wo[c * dm + f], H[p * dm + f], a);
        y[((size_t)b * d.Lp + p) * C + c] = a * st[C + c] + st[c];
    }
}

// workgroup g: windows g share .. min(B, (g + 1) share) into slab g (NV floats); its activation region follows the G slabs
__global__ __launch_bounds__(TM_THREADS) void timemixer_bwd_kernel(TmDims d, TmOff po, TmDrop dr, const uint64_t* __restrict__ seed_dev, int share,
                                                                   size_t act_floats, const float* __restrict__ data,
                                                                   const float* __restrict__ mask, const float* __restrict__ tp,
                                                                   const float* const* __restrict__ prm, const float* __restrict__ dY,
                                                                   float* __restrict__ ws) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, dm = d.d, n = d.n, C = d.C, K = d.K, P = d.P, SD = d.sumT * d.d, dff = d.dff;
    float *X = lds, *R2 = lds + SD, *st = R2 + tm_r2(d);
    float *dX = X, *dS = R2, *dT = R2 + SD, *H = R2 + 2 * SD;
    float* slab = ws + (size_t)blockIdx.x * po.NV;
    float* act = ws + (size_t)gridDim.x * po.NV + (size_t)blockIdx.x * act_floats;
    if (dr.p > 0.f && seed_dev) dr.seed += *seed_dev;
    const int half = (d.k - 1) / 2, hd = tm_head(d), Tn = d.T[n];
    const int wbeg = blockIdx.x * share, wend = min(d.B, wbeg + share);
    for (int b = wbeg; b < wend; ++b) {
        const bool init = b == wbeg;
        tm_forward_window(d, b, data, mask, tp, prm, dr, X, R2, st, act);
        const float* dec = act + (size_t)d.sumT * K + (size_t)d.E * 4 * SD;
        // ---- head: y = (bo + Wo dec) std + mean, dec = bp + Wp x_n.  X rows off_n .. still hold x_n; H <- ddec [P][d]
        const float *Wo = prm[hd + 2], *Wp = prm[hd];
        for (int it = tid; it < P * dm; it += TM_THREADS) {
            const int p = it / dm, f = it - p * dm;
            float a = 0.f;
            if (p < d.Lp)
                for (int c = 0; c < C; ++c) a = fmaf(Wo[c * dm + f], dY[((size_t)b * d.Lp + p) * C + c] * st[C + c], a);
            H[it] = a;
        }
        for (int it = tid; it < C * dm + C; it += TM_THREADS) {
            const bool bias = it >= C * dm;
            const int c = bias ? it - C * dm : it / dm, f = bias ? 0 : it - c * dm;
            float a = 0.f;
            for (int p = 0; p < d.Lp; ++p) {
                const float g = dY[((size_t)b * d.Lp + p) * C + c] * st[C + c];
                a = bias ? a + g : fmaf(g, dec[p * dm + f], a);
            }
            tm_acc(slab + po.o[bias ? hd + 3 : hd + 2], bias ? c : it, a, init);
        }
        __syncthreads();
        for (int it = tid; it < P * Tn + P; it += TM_THREADS) {
            const bool bias = it >= P * Tn;
            const int p = bias ? it - P * Tn : it / Tn, t = bias ? 0 : it - p * Tn;
            float a = 0.f;
            for (int f = 0; f < dm; ++f) a = bias ? a + H[p * dm + f] : fmaf(H[p * dm + f], X[(d.off[n] + t) * dm + f], a);
            tm_acc(slab + po.o[bias ? hd + 1 : hd], bias ? p : it, a, init);
        }
        __syncthreads();
        for (int it = tid; it < SD; it += TM_THREADS) {      // dX: zero on the finer scales, Wp^T ddec on the coarsest
            const int r = it / dm, f = it - r * dm;
            float a = 0.f;
            if (r >= d.off[n]) {
                const int t = r - d.off[n];
                for (int p = 0; p < P; ++p) a = fmaf(Wp[p * Tn + t], H[p * dm + f], a);
            }
            dX[it] = a;      // overwrites x_n: its readers finished before the barrier above
        }
        __syncthreads();
        // ---- the blocks, last to first
        for (int j = d.E - 1; j >= 0; --j) {
            const bool last = j == d.E - 1;
            const float* ablk = act + (size_t)d.sumT * K + (size_t)j * 4 * SD;
            const float *OS = ablk, *OT = ablk + SD, *H1S = ablk + 2 * SD, *H1T = ablk + 3 * SD;
            for (int it = tid; it < SD; it += TM_THREADS) { dS[it] = 0.f; dT[it] = 0.f; }
            __syncthreads();
            // out_layer on rows r0 ..: Ha = pre-GELU -> GELU [nr][dff], Hb = its gradient
            const int e = tm_outl(d, j), RC = d.hsz / (2 * dff);
            const float *W1 = prm[e], *b1 = prm[e + 1], *W2 = prm[e + 2];
            const int rbeg = last ? d.off[n] : 0;
            for (int r0 = rbeg; r0 < d.sumT; r0 += RC) {
                const int nr = min(RC, d.sumT - r0);
                const bool ini = init && r0 == rbeg;
                float *Ha = H, *Hb = H + RC * dff;
                for (int it = tid; it < nr * dff; it += TM_THREADS) {
                    const int rr = it / dff, q = it - rr * dff;
                    const float *sx = OS + (r0 + rr) * dm, *tx = OT + (r0 + rr) * dm, *g = dX + (r0 + rr) * dm;
                    float a = b1[q], dg = 0.f;
                    for (int f = 0; f < dm; ++f) {
                        a = fmaf(W1[q * dm + f], sx[f] + tx[f], a);
                        dg = fmaf(W2[f * dff + q], g[f], dg);
                    }
                    Ha[it] = tm_gelu(a);
                    Hb[it] = dg * tm_dgelu(a);
                }
                __syncthreads();
                for (int it = tid; it < dm * dff; it += TM_THREADS) {
                    {   // dW2 [d][dff]
                        const int f = it / dff, q = it - f * dff;
                        float a = 0.f;
                        for (int rr = 0; rr < nr; ++rr) a = fmaf(dX[(r0 + rr) * dm + f], Ha[rr * dff + q], a);
                        tm_acc(slab + po.o[e + 2], it, a, ini);
                    }
                    {   // dW1 [dff][d]
                        const int q = it / dm, f = it - q * dm;
                        float a = 0.f;
                        for (int rr = 0; rr < nr; ++rr)
                            a = fmaf(Hb[rr * dff + q], OS[(r0 + rr) * dm + f] + OT[(r0 + rr) * dm + f], a);
                        tm_acc(slab + po.o[e], it, a, ini);
                    }
                }
                for (int it = tid; it < dff + dm; it += TM_THREADS) {
                    const bool second = it >= dff;
                    const int q = second ? it - dff : it;
                    float a = 0.f;
                    for (int rr = 0; rr < nr; ++rr) a += second ? dX[(r0 + rr) * dm + q] : Hb[rr * dff + q];
                    tm_acc(slab + po.o[second ? e + 3 : e + 1], q, a, ini);
                }
                for (int it = tid; it < nr * dm; it += TM_THREADS) {
                    const int rr = it / dm, f = it - rr * dm;
                    float a = 0.f;
                    for (int q = 0; q < dff; ++q) a = fmaf(W1[q * dm + f], Hb[rr * dff + q], a);
                    dS[(r0 + rr) * dm + f] = a;
                    dT[(r0 + rr) * dm + f] = a;
                }
                __syncthreads();
            }
            if (!last)
                for (int i = 0; i < n; ++i)
                    tm_time_mlp_bwd(dT, dm, d.off[i + 1], d.T[i + 1], d.off[i], d.T[i], prm, po, tm_trnd(d, j, i), OT + d.off[i + 1] * dm,
                                    H1T + d.off[i] * dm, H, slab, init);
            for (int i = n - 1; i >= 0; --i)
                tm_time_mlp_bwd(dS, dm, d.off[i], d.T[i], d.off[i + 1], d.T[i + 1], prm, po, tm_seas(d, j, i), OS + d.off[i] * dm,
                                H1S + d.off[i + 1] * dm, H, slab, init);
            // decomposition: season = x - A x, trend = A x  =>  dx += dS + A^T (dT - dS)
            for (int it = tid; it < SD; it += TM_THREADS) dT[it] -= dS[it];
            __syncthreads();
            for (int it = tid; it < SD; it += TM_THREADS) {
                const int r = it / dm, f = it - r * dm;
                int i = 0;
                while (i < n && r >= d.off[i + 1]) ++i;
                const int T = d.T[i], l = r - d.off[i];
                const float* v = dT + d.off[i] * dm + f;
                float a = 0.f;
                if (T == 1 || l == 0 || l == T - 1) {
                    for (int m = 0; m < T; ++m) a = fmaf((float)tm_ma_count(m, l, T, half), v[m * dm], a);
                } else {
                    const int lo = max(l - half, 0), hi = min(l + half, T - 1);
                    for (int m = lo; m <= hi; ++m) a += v[m * dm];
                }
                dX[it] += dS[it] + a / (float)d.k;
            }
            __syncthreads();
        }
        // ---- embedding: dX is the gradient of the dropped-out rows; the token convolution's weight (d, K, 3)
        if (dr.p > 0.f) {
            for (int it = tid; it < SD; it += TM_THREADS) {
                const int r = it / dm, f = it - r * dm;
                int i = 0;
                while (i < n && r >= d.off[i + 1]) ++i;
                const int T = d.T[i], t = r - d.off[i];
                dX[it] *= dropout_scale(dr.seed, dr.site, (((uint64_t)d.off[i] * d.B + (uint64_t)b * T + t) * dm + f), dr.p, dr.inv_keep);
            }
            __syncthreads();
        }
        for (int it = tid; it < dm * K * 3; it += TM_THREADS) {
            const int f = it / (K * 3), rem = it - f * K * 3, c = rem / 3, jj = rem - c * 3;
            float a = 0.f;
            for (int i = 0; i <= n; ++i) {
                const int T = d.T[i];
                const float* en = act + d.off[i] * K + c;
                for (int t = 0; t < T; ++t) {
                    int u = t + jj - 1;
                    u = u < 0 ? T - 1 : (u >= T ? 0 : u);
                    a = fmaf(dX[(d.off[i] + t) * dm + f], en[u * K], a);
                }
            }
            tm_acc(slab + po.o[0], it, a, init);
        }
        __syncthreads();      // the next window overwrites the LDS and the activation region
    }
}

// gradient entry i = the G slabs added in index order (four interleaved chains)
__global__ __launch_bounds__(TM_THREADS) void timemixer_fold_kernel(int NV, int G, const float* __restrict__ slabs, float* __restrict__ grads) {
    const int i = blockIdx.x * TM_THREADS + threadIdx.x;
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
    grads[i] = (a0 + a1) + (a2 + a3);
}

inline bool tm_call_ok(int64_t B, int L, int C, int S, int P, int Lp, int dm, int dff, int E, int n, int k) {
    return B >= 0 && B < (1ll << 31) && L >= 0 && L <= S && Lp >= 0 && Lp <= P && immtsf_timemixer_supported(S, P, C, dm, dff, E, n, k);
}

}  // namespace

extern "C" {

int immtsf_timemixer_supported(int32_t S, int32_t P, int32_t C, int32_t d_model, int32_t d_ff, int32_t e_layers, int32_t down_layers,
                               int32_t moving_avg) {
    if (S < 2 || S > TM_MAX_S || P < 1 || P > TM_MAX_P || C < 1 || 2 * C + 1 > TM_MAX_K || d_model < 1 || d_model > TM_MAX_D || d_ff < 1 ||
        d_ff > TM_MAX_DFF || e_layers < 1 || e_layers > TM_MAX_E || down_layers < 1 || down_layers > TM_MAX_N || (S >> down_layers) < 1 ||
        moving_avg < 1 || moving_avg > TM_MAX_MA || !(moving_avg & 1))
        return 0;
    const TmDims d = tm_dims(1, 0, C, S, P, 0, d_model, d_ff, e_layers, down_layers, moving_avg);
    const size_t lds = tm_lds_bytes(d);
    return lds <= (size_t)TM_LDS_BYTES && lds <= (size_t)TM_LDS_STATIC ? 1 : 0;
}

int32_t immtsf_timemixer_grad_layout(int32_t S, int32_t P, int32_t C, int32_t d_model, int32_t d_ff, int32_t e_layers, int32_t down_layers,
                                     int32_t* offsets, int32_t n_offsets) {
    if (!immtsf_timemixer_supported(S, P, C, d_model, d_ff, e_layers, down_layers, 1)) return -1;
    const TmDims d = tm_dims(1, 0, C, S, P, 0, d_model, d_ff, e_layers, down_layers, 1);
    const TmOff f = tm_offsets(d);
    const int np = tm_head(d) + 4;
    if (offsets) {
        if (n_offsets < np) return -1;
        for (int i = 0; i < np; ++i) offsets[i] = f.o[i];
    }
    return f.NV;
}

size_t immtsf_timemixer_workspace_bytes(int32_t B, int32_t S, int32_t P, int32_t C, int32_t d_model, int32_t d_ff, int32_t e_layers,
                                        int32_t down_layers) {
    if (B < 1 || !immtsf_timemixer_supported(S, P, C, d_model, d_ff, e_layers, down_layers, 1)) return 0;
    const TmDims d = tm_dims(B, 0, C, S, P, 0, d_model, d_ff, e_layers, down_layers, 1);
    const int NV = tm_offsets(d).NV;
    const TmPlan pl = tm_plan(d, NV);
    return (size_t)pl.G * ((size_t)NV + tm_act_floats(d)) * sizeof(float) + 256;
}

int immtsf_timemixer_forward(int32_t B, int32_t L, int32_t C, int32_t S, int32_t P, int32_t Lp, int32_t d_model, int32_t d_ff, int32_t e_layers,
                             int32_t down_layers, int32_t moving_avg, const float* data, const float* mask, const float* tp,
                             const float* const* params, float* y, float p_drop, uint64_t seed, uint64_t site, const uint64_t* seed_step_dev,
                             immtsf_stream_t stream) {
    if (S < 1 || P < 1 || C < 1 || moving_avg < 1 || !(p_drop >= 0.f && p_drop < 1.f)) return IMMTSF_EINVAL;
    if (!immtsf_timemixer_supported(S, P, C, d_model, d_ff, e_layers, down_layers, moving_avg)) return IMMTSF_EUNSUPPORTED;
    if (!tm_call_ok(B, L, C, S, P, Lp, d_model, d_ff, e_layers, down_layers, moving_avg)) return IMMTSF_EINVAL;
    if (B == 0 || Lp == 0) return IMMTSF_OK;
    if (!params || !y || (L > 0 && (!data || !mask || !tp))) return IMMTSF_EINVAL;
    const TmDims d = tm_dims(B, L, C, S, P, Lp, d_model, d_ff, e_layers, down_layers, moving_avg);
    const TmDrop dr{p_drop, 1.f / (1.f - p_drop), seed, site};
    hipLaunchKernelGGL(timemixer_fwd_kernel, dim3(B), dim3(TM_THREADS), tm_lds_bytes(d), static_cast<hipStream_t>(stream), d, dr, seed_step_dev,
                       data, mask, tp, params, y);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_timemixer_backward(int32_t B, int32_t L, int32_t C, int32_t S, int32_t P, int32_t Lp, int32_t d_model, int32_t d_ff,
                              int32_t e_layers, int32_t down_layers, int32_t moving_avg, const float* data, const float* mask, const float* tp,
                              const float* const* params, const float* dY, float* grads, float p_drop, uint64_t seed, uint64_t site,
                              const uint64_t* seed_step_dev, void* workspace, size_t workspace_bytes, immtsf_stream_t stream) {
    if (S < 1 || P < 1 || C < 1 || moving_avg < 1 || !(p_drop >= 0.f && p_drop < 1.f)) return IMMTSF_EINVAL;
    if (!immtsf_timemixer_supported(S, P, C, d_model, d_ff, e_layers, down_layers, moving_avg)) return IMMTSF_EUNSUPPORTED;
    if (!tm_call_ok(B, L, C, S, P, Lp, d_model, d_ff, e_layers, down_layers, moving_avg) || B < 1) return IMMTSF_EINVAL;
    if (!params || !grads || !workspace || (L > 0 && (!data || !mask || !tp)) || (Lp > 0 && !dY)) return IMMTSF_EINVAL;
    if (workspace_bytes < immtsf_timemixer_workspace_bytes(B, S, P, C, d_model, d_ff, e_layers, down_layers)) return IMMTSF_EWORKSPACE;
    float* ws = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t(255));
    const TmDims d = tm_dims(B, L, C, S, P, Lp, d_model, d_ff, e_layers, down_layers, moving_avg);
    const TmOff po = tm_offsets(d);
    const TmPlan pl = tm_plan(d, po.NV);
    const TmDrop dr{p_drop, 1.f / (1.f - p_drop), seed, site};
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(timemixer_bwd_kernel, dim3(pl.G), dim3(TM_THREADS), tm_lds_bytes(d), s, d, po, dr, seed_step_dev, pl.share,
                       tm_act_floats(d), data, mask, tp, params, dY, ws);
    IMMTSF_LAUNCH_CHECK();
    hipLaunchKernelGGL(timemixer_fold_kernel, dim3(cdiv(po.NV, TM_THREADS)), dim3(TM_THREADS), 0, s, po.NV, pl.G, ws, grads);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
