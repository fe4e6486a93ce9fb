// Dense attention at head_dim 64, fp32 on the VALU, with dropout on the probabilities: the forward and the two backward kernels that
// the frozen GPT-2 body (gpt2.hip, CAUSAL) and the frozen BERT body (bert_body.hip, not CAUSAL) share.  Rows are (b, s), s < S; the
// forward computes the queries q_from .. S-1 (query t < Sq = S - q_from is position q_from + t, row b Sq + t of q / out / dout, lse
// (B, H, Sq)), K / V are read in the projections' layout (row pitch ldkv, head h at columns 64 h).  The dropout index of probability
// (b, h, i, j) is ((b H + h) S + i) ATT_STRIDE + j: four keys per Philox call at any S <= ATT_STRIDE.  The backward recomputes the
// probabilities from the log-sum-exp and redraws the mask.  One writer per output element, sums in key / query order, no atomics.
//   CAUSAL: key j is visible to position i when j <= i; the key loops end at the last key some query of the wave sees, and the dK / dV
//           query loop starts at the first query that sees a key of the wave.
//   else:   every key j < S is visible; a key at or past S in a partial tile scores -inf (there is no causal mask to hide it).
#pragma once
#include "common.hpp"

namespace dense64 {

constexpr int HD = 64;           // head_dim
constexpr int KT = 32;           // keys per LDS tile
constexpr int KC = 4;            // keys per softmax chunk = keys per Philox call
constexpr int QT = 16;           // queries per LDS tile of the dK / dV kernel

// K / V rows j0 .. j0 + KT - 1 of (b, head h) into LDS; a row at or past kend is zero
__device__ __forceinline__ void load_kv_tile(const float* __restrict__ k, const float* __restrict__ v, int ldkv, int b, int S, int h, int j0,
                                             int kend, int lane, float4* Ks, float4* Vs) {
#pragma unroll
    for (int i = 0; i < KT * HD / 4 / 64; ++i) {
        const int idx = lane + 64 * i, kk = idx >> 4, part = idx & 15, j = j0 + kk;
        float4 a = {0.f, 0.f, 0.f, 0.f}, c = a;
        if (j < kend) {
            a = reinterpret_cast<const float4*>(k + ((size_t)b * S + j) * ldkv + h * HD)[part];
            c = reinterpret_cast<const float4*>(v + ((size_t)b * S + j) * ldkv + h * HD)[part];
        }
        Ks[idx] = a;
        Vs[idx] = c;
    }
}

// ---- forward --------------------------------------------------------------------------------------------------------------------------
// one wave per 64 consecutive queries of one (b, head); a thread owns one query (q, the output row and the softmax state in registers),
// K / V tiles of KT keys go through LDS and are read as broadcasts.
template <bool CAUSAL>
__global__ void __launch_bounds__(64) attn_fwd_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k,
                                                      const float* __restrict__ v, int ldkv, int S, int H, int q_from, float scale,
                                                      DropCfg drop, uint64_t site, float* __restrict__ o32, bf16_t* __restrict__ o16,
                                                      float* __restrict__ lse) {
    __shared__ float4 Ks[KT * HD / 4];
    __shared__ float4 Vs[KT * HD / 4];
    const int Sq = S - q_from, lane = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int t0 = blockIdx.x * 64;
    const bool live = t0 + lane < Sq;
    const int t = live ? t0 + lane : Sq - 1;              // clamped: an idle lane repeats the last query and writes nothing
    const int qi = q_from + t;
    float qr[HD], acc[HD];
    {
        const float4* qp = reinterpret_cast<const float4*>(q + ((size_t)b * Sq + t) * ldq + h * HD);
#pragma unroll
        for (int e = 0; e < HD / 4; ++e) {
            const float4 x = qp[e];
            qr[4 * e] = x.x * scale; qr[4 * e + 1] = x.y * scale; qr[4 * e + 2] = x.z * scale; qr[4 * e + 3] = x.w * scale;
        }
    }
#pragma unroll
    for (int e = 0; e < HD; ++e) acc[e] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int kend = CAUSAL ? q_from + min(t0 + 63, Sq - 1) + 1 : S;   // keys 0 .. kend-1 are visible to some query of the wave (kend <= S)
    const size_t drow = (((size_t)b * H + h) * S + qi) * ATT_STRIDE;
    for (int j0 = 0; j0 < kend; j0 += KT) {
        __syncthreads();
        load_kv_tile(k, v, ldkv, b, S, h, j0, kend, lane, Ks, Vs);
        __syncthreads();
#pragma unroll 1
        for (int c4 = 0; c4 < KT && j0 + c4 < kend; c4 += KC) {
            float sc[KC];
            float cmax = -INFINITY;
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                float a = 0.f;
#pragma unroll
                for (int e = 0; e < HD / 4; ++e) {
                    const float4 kk = Ks[(c4 + c) * (HD / 4) + e];
                    a += qr[4 * e] * kk.x + qr[4 * e + 1] * kk.y + qr[4 * e + 2] * kk.z + qr[4 * e + 3] * kk.w;
                }
                sc[c] = (CAUSAL ? j0 + c4 + c <= qi : j0 + c4 + c < S) ? a : -INFINITY;
                cmax = fmaxf(cmax, sc[c]);
            }
            // (the running maximum is finite from the first chunk on: key 0 is real and visible to every query; it rarely grows later, so
            // the rescale of the output row is a branch most chunks skip)
            if (cmax > m) {
                const float corr = __expf(m - cmax);
                m = cmax;
                l *= corr;
#pragma unroll
                for (int e = 0; e < HD; ++e) acc[e] *= corr;
            }
            float ds[KC];
            dropout_scale4(drop, site, drow + (size_t)(j0 + c4), ds);
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const float p = __expf(sc[c] - m);
                l += p;
                const float pa = p * ds[c];
#pragma unroll
                for (int e = 0; e < HD / 4; ++e) {
                    const float4 vv = Vs[(c4 + c) * (HD / 4) + e];
                    acc[4 * e] += pa * vv.x; acc[4 * e + 1] += pa * vv.y; acc[4 * e + 2] += pa * vv.z; acc[4 * e + 3] += pa * vv.w;
                }
            }
        }
    }
    if (!live) return;
    const float inv = 1.f / l;
    const size_t orow = ((size_t)b * Sq + t) * ((size_t)H * HD) + h * HD;
    if (o32) {
#pragma unroll
        for (int e = 0; e < HD / 4; ++e)
            reinterpret_cast<float4*>(o32 + orow)[e] = float4{acc[4 * e] * inv, acc[4 * e + 1] * inv, acc[4 * e + 2] * inv, acc[4 * e + 3] * inv};
    }
    if (o16) {
#pragma unroll
        for (int e = 0; e < HD / 4; ++e)
            reinterpret_cast<bf16x4*>(o16 + orow)[e] = bf16x4{(bf16_t)(acc[4 * e] * inv), (bf16_t)(acc[4 * e + 1] * inv),
                                                             (bf16_t)(acc[4 * e + 2] * inv), (bf16_t)(acc[4 * e + 3] * inv)};
    }
    if (lse) lse[((size_t)b * H + h) * Sq + t] = m + __logf(l);
}

// ---- backward: dQ of the queries dq_from .. S-1 against the keys they see ---------------------------------------------------------------
// q / dout / out / lse are the forward's (queries q_from .. S-1, q_from <= dq_from; pitch ldq for q, H 64 for dout / out); dq row
// b dq_rows + (position - dq_from), pitch ldd.
template <bool CAUSAL>
__global__ void __launch_bounds__(64) attn_bwd_q_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k,
                                                        const float* __restrict__ v, int ldkv, const float* __restrict__ dout,
                                                        const float* __restrict__ out, const float* __restrict__ lse, int S, int H,
                                                        int q_from, int dq_from, float scale, DropCfg drop, uint64_t site,
                                                        float* __restrict__ dq, int dq_rows, int ldd) {
    __shared__ float4 Ks[KT * HD / 4];
    __shared__ float4 Vs[KT * HD / 4];
    const int Sq = S - q_from, Sd = S - dq_from, lane = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int u0 = blockIdx.x * 64;
    const bool live = u0 + lane < Sd;
    const int u = live ? u0 + lane : Sd - 1;
    const int qi = dq_from + u, t = qi - q_from;
    float qr[HD], go[HD], acc[HD];
    float D = 0.f;
    {
        const float4* qp = reinterpret_cast<const float4*>(q + ((size_t)b * Sq + t) * ldq + h * HD);
        const float4* gp = reinterpret_cast<const float4*>(dout + ((size_t)b * Sq + t) * ((size_t)H * HD) + h * HD);
        const float4* op = reinterpret_cast<const float4*>(out + ((size_t)b * Sq + t) * ((size_t)H * HD) + h * HD);
#pragma unroll
        for (int e = 0; e < HD / 4; ++e) {
            const float4 x = qp[e], g = gp[e], o = op[e];
            qr[4 * e] = x.x * scale; qr[4 * e + 1] = x.y * scale; qr[4 * e + 2] = x.z * scale; qr[4 * e + 3] = x.w * scale;
            go[4 * e] = g.x; go[4 * e + 1] = g.y; go[4 * e + 2] = g.z; go[4 * e + 3] = g.w;
            D += g.x * o.x + g.y * o.y + g.z * o.z + g.w * o.w;
        }
    }
#pragma unroll
    for (int e = 0; e < HD; ++e) acc[e] = 0.f;
    const float L = lse[((size_t)b * H + h) * Sq + t];
    const int kend = CAUSAL ? dq_from + min(u0 + 63, Sd - 1) + 1 : S;
    const size_t drow = (((size_t)b * H + h) * S + qi) * ATT_STRIDE;
    for (int j0 = 0; j0 < kend; j0 += KT) {
        __syncthreads();
        load_kv_tile(k, v, ldkv, b, S, h, j0, kend, lane, Ks, Vs);
        __syncthreads();
#pragma unroll 1
        for (int c4 = 0; c4 < KT && j0 + c4 < kend; c4 += KC) {
            float ds[KC];
            dropout_scale4(drop, site, drow + (size_t)(j0 + c4), ds);
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                float s = 0.f, dA = 0.f;
#pragma unroll
                for (int e = 0; e < HD / 4; ++e) {
                    const float4 kk = Ks[(c4 + c) * (HD / 4) + e], vv = Vs[(c4 + c) * (HD / 4) + e];
                    s += qr[4 * e] * kk.x + qr[4 * e + 1] * kk.y + qr[4 * e + 2] * kk.z + qr[4 * e + 3] * kk.w;
                    dA += go[4 * e] * vv.x + go[4 * e + 1] * vv.y + go[4 * e + 2] * vv.z + go[4 * e + 3] * vv.w;
                }
                const float p = (CAUSAL ? j0 + c4 + c <= qi : j0 + c4 + c < S) ? __expf(s - L) : 0.f;
                const float dS = p * (ds[c] * dA - D);
#pragma unroll
                for (int e = 0; e < HD / 4; ++e) {
                    const float4 kk = Ks[(c4 + c) * (HD / 4) + e];
                    acc[4 * e] += dS * kk.x; acc[4 * e + 1] += dS * kk.y; acc[4 * e + 2] += dS * kk.z; acc[4 * e + 3] += dS * kk.w;
                }
            }
        }
    }
    if (!live) return;
    float4* dp = reinterpret_cast<float4*>(dq + ((size_t)b * dq_rows + u) * ldd + h * HD);
#pragma unroll
    for (int e = 0; e < HD / 4; ++e) dp[e] = float4{acc[4 * e] * scale, acc[4 * e + 1] * scale, acc[4 * e + 2] * scale, acc[4 * e + 3] * scale};
}

// ---- backward: dK / dV of the keys k_from .. S-1, summed over the forward's queries that see them, in query order -----------------------
// a thread owns key u (position k_from + u); the queries' q | dout rows, lse and D = dout . out go through LDS, QT at a time.  dk / dv
// row b dkv_rows + u, pitch ldd.  CAUSAL: no query before position k_from + u0 sees a key of the wave, so the loop starts there (and not
// at a multiple of QT below it: a thread sums its queries serially, the start fixes the order).
template <bool CAUSAL>
__global__ void __launch_bounds__(64) attn_bwd_kv_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k,
                                                         const float* __restrict__ v, int ldkv, const float* __restrict__ dout,
                                                         const float* __restrict__ out, const float* __restrict__ lse, int S, int H,
                                                         int q_from, int k_from, float scale, DropCfg drop, uint64_t site,
                                                         float* __restrict__ dk, float* __restrict__ dv, int dkv_rows, int ldd) {
    __shared__ float4 Qs[QT * HD / 4];
    __shared__ float4 Gs[QT * HD / 4];
    __shared__ float Ls[QT], Ds[QT];
    const int Sq = S - q_from, Sk = S - k_from, lane = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int u0 = blockIdx.x * 64;
    const bool live = u0 + lane < Sk;
    const int u = live ? u0 + lane : Sk - 1;
    const int kj = k_from + u;
    float kr[HD], vr[HD], ak[HD], av[HD];
    {
        const float4* kp = reinterpret_cast<const float4*>(k + ((size_t)b * S + kj) * ldkv + h * HD);
        const float4* vp = reinterpret_cast<const float4*>(v + ((size_t)b * S + kj) * ldkv + h * HD);
#pragma unroll
        for (int e = 0; e < HD / 4; ++e) {
            const float4 x = kp[e], y = vp[e];
            kr[4 * e] = x.x; kr[4 * e + 1] = x.y; kr[4 * e + 2] = x.z; kr[4 * e + 3] = x.w;
            vr[4 * e] = y.x; vr[4 * e + 1] = y.y; vr[4 * e + 2] = y.z; vr[4 * e + 3] = y.w;
        }
    }
#pragma unroll
    for (int e = 0; e < HD; ++e) { ak[e] = 0.f; av[e] = 0.f; }
    for (int tq0 = CAUSAL ? max(k_from + u0 - q_from, 0) : 0; tq0 < Sq; tq0 += QT) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < QT * HD / 4 / 64; ++i) {
            const int idx = lane + 64 * i, tt = idx >> 4, part = idx & 15, t = tq0 + tt;
            float4 a = {0.f, 0.f, 0.f, 0.f}, c = a;
            if (t < Sq) {
                a = reinterpret_cast<const float4*>(q + ((size_t)b * Sq + t) * ldq + h * HD)[part];
                c = reinterpret_cast<const float4*>(dout + ((size_t)b * Sq + t) * ((size_t)H * HD) + h * HD)[part];
            }
            Qs[idx] = a;
            Gs[idx] = c;
        }
        if (lane < QT) {
            const int t = tq0 + lane;
            float L = 0.f, D = 0.f;
            if (t < Sq) {
                L = lse[((size_t)b * H + h) * Sq + t];
                const float4* gp = reinterpret_cast<const float4*>(dout + ((size_t)b * Sq + t) * ((size_t)H * HD) + h * HD);
                const float4* op = reinterpret_cast<const float4*>(out + ((size_t)b * Sq + t) * ((size_t)H * HD) + h * HD);
                for (int e = 0; e < HD / 4; ++e) {
                    const float4 g = gp[e], o = op[e];
                    D += g.x * o.x + g.y * o.y + g.z * o.z + g.w * o.w;
                }
            }
            Ls[lane] = L;
            Ds[lane] = D;
        }
        __syncthreads();
#pragma unroll 1
        for (int c = 0; c < QT && tq0 + c < Sq; ++c) {
            const int t = tq0 + c;
            float s = 0.f, dA = 0.f;
#pragma unroll
            for (int e = 0; e < HD / 4; ++e) {
                const float4 qq = Qs[c * (HD / 4) + e], gg = Gs[c * (HD / 4) + e];
                s += kr[4 * e] * qq.x + kr[4 * e + 1] * qq.y + kr[4 * e + 2] * qq.z + kr[4 * e + 3] * qq.w;
                dA += vr[4 * e] * gg.x + vr[4 * e + 1] * gg.y + vr[4 * e + 2] * gg.z + vr[4 * e + 3] * gg.w;
            }
            const float p = (!CAUSAL || kj <= q_from + t) ? __expf(s * scale - Ls[c]) : 0.f;
            const float dsc = dropout_scale(drop, site, (((size_t)b * H + h) * S + q_from + t) * ATT_STRIDE + (size_t)kj);
            const float A = p * dsc;
            const float dS = p * (dsc * dA - Ds[c]) * scale;
#pragma unroll
            for (int e = 0; e < HD / 4; ++e) {
                const float4 qq = Qs[c * (HD / 4) + e], gg = Gs[c * (HD / 4) + e];
                ak[4 * e] += dS * qq.x; ak[4 * e + 1] += dS * qq.y; ak[4 * e + 2] += dS * qq.z; ak[4 * e + 3] += dS * qq.w;
                av[4 * e] += A * gg.x; av[4 * e + 1] += A * gg.y; av[4 * e + 2] += A * gg.z; av[4 * e + 3] += A * gg.w;
            }
        }
    }
    if (!live) return;
    float4* dkp = reinterpret_cast<float4*>(dk + ((size_t)b * dkv_rows + u) * ldd + h * HD);
    float4* dvp = reinterpret_cast<float4*>(dv + ((size_t)b * dkv_rows + u) * ldd + h * HD);
#pragma unroll
    for (int e = 0; e < HD / 4; ++e) {
        dkp[e] = float4{ak[4 * e], ak[4 * e + 1], ak[4 * e + 2], ak[4 * e + 3]};
        dvp[e] = float4{av[4 * e], av[4 * e + 1], av[4 * e + 2], av[4 * e + 3]};
    }
}

}  // namespace dense64
