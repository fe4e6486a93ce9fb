// TimeLLM's frozen Llama body (reference models/TimeLLM.py: llm_model(inputs_embeds=cat([prompt, patches])) with llm_model_timellm =
// "LLAMA"): what immtsf.ops.llama_body needs beside the GEMM family and the forward row kernels of llama_embed.hip (the cos / sin table,
// SwiGLU).  Rows are (b, s) with s < S = S_p + S_t, dense; the last S_t rows (the reprogrammed patches) are the only ones a gradient flows
// to, there is no attention mask, positions are arange(S) and attention is plain causal, so no prefix row ever depends on a tail row: the
// backward runs over the B S_t tail rows alone (dQ of the tail queries against all keys, dK / dV of the tail keys from the tail queries),
// and it is exact.  head_dim 128, H query heads over H_kv K/V heads, G = H / H_kv in {1, 2, 4, 8}.
//   * RMSNorm rows (b, s_from + t) of a (B, S_in, d) tensor into compact outputs, behind an optional residual add whose sum is written
//     too; fp32 statistics, rstd saved for the backward; and its data gradient with an optional residual gradient in the same launch
//   * RoPE over dense rows, in place, position pos0 + (row mod rows_per_b), forward or transposed (the backward: the rotation by the
//     negated angle, same cos / sin table); optionally the bf16 image of the whole row for the next bf16-in-memory product
//   * causal attention forward with a query offset q_from (the last layer computes the tail queries only): the kernels of
//     attn_gqa128.hpp, which llama_embed.hip shares, over dense sequences -- fp32 on the VALU, or both products on bf16 MFMA 16x16x32
//     with fp32 online softmax -- that also write the per-(row, head) log-sum-exp
//   * its backward for the tail queries, fp32 on the VALU in either precision mode: probabilities recomputed from the log-sum-exp; dK and
//     dV of a K/V head sum over its G query heads in head order, then in query order: one writer per output element, no atomics
//   * SwiGLU backward: dgate | dup in one buffer from the saved gate | up product
// No dropout (Llama has none but attention_dropout, which the caller keeps on the stock path).  Two runs give the same bits.
#include "../../include/immtsf.h"
#include "attn_gqa128.hpp"
#include "common.hpp"

namespace {

using gqa128::HD;             // head_dim 128
using gqa128::QT;             // 32 queries per wave
using gqa128::KT;             // 32 keys per LDS tile
constexpr int HP = HD / 2;    // rotary pairs of a head
constexpr int MAXS = 1024;    // longest sequence
constexpr int UT = 16;        // tail keys per wave of the dK / dV kernel (four lanes a key)
constexpr int QB = 16;        // queries per LDS tile of the dK / dV kernel

// ---- RMSNorm of the rows (b, s_from + t), t < Sn, of xin (B, S_in, d); compact outputs; one wave per row ----------------------------------
// y given: the row is xin + y[r] (y compact), written to xout[r] (compact; may be xin itself when the rows coincide).  Lane l writes, and
// alone reads back, its own elements.  PT: the type of the weight w (float, or bf16_t for a model stored in bf16; up-cast in registers).
template <typename PT>
__global__ void __launch_bounds__(256) llama_body_rms_kernel(const float* xin, int S_in, int s_from, int Sn, const float* __restrict__ y,
                                                             float* xout, long rows, int d, const PT* __restrict__ w, float eps,
                                                             float* __restrict__ out32, bf16_t* __restrict__ out16,
                                                             float* __restrict__ rstd_out) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const long b = r / Sn, t = r - b * Sn;
    const float4* src = reinterpret_cast<const float4*>(xin + ((size_t)b * S_in + s_from + t) * d);
    const int d4 = d >> 2;
    float ss = 0.f;
    if (y) {
        const float4* yr = reinterpret_cast<const float4*>(y + (size_t)r * d);
        float4* xo = reinterpret_cast<float4*>(xout + (size_t)r * d);
        for (int e = lane; e < d4; e += 64) {
            const float4 a = src[e], c = yr[e];
            const float4 v = {a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w};
            xo[e] = v;
            ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
        src = xo;
    } else {
        for (int e = lane; e < d4; e += 64) {
            const float4 v = src[e];
            ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
    }
    const float rstd = rsqrtf(wave_sum(ss) / (float)d + eps);
    if (rstd_out && lane == 0) rstd_out[r] = rstd;
    if (!out32 && !out16) return;
    for (int e = lane; e < d4; e += 64) {
        const float4 v = src[e], g = param4(w, e);
        const float4 z = {v.x * rstd * g.x, v.y * rstd * g.y, v.z * rstd * g.z, v.w * rstd * g.w};
        if (out32) reinterpret_cast<float4*>(out32 + (size_t)r * d)[e] = z;
        if (out16) reinterpret_cast<bf16x4*>(out16 + (size_t)r * d)[e] = bf16x4{(bf16_t)z.x, (bf16_t)z.y, (bf16_t)z.z, (bf16_t)z.w};
    }
}

// dx[r] = resid[r] + rstd (g - x rstd^2 mean(g x)), g = w dy; the weights are frozen: data gradient only.  Rows compact, one wave per row.
template <typename PT>
__global__ void __launch_bounds__(256) llama_body_rms_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                 const float* __restrict__ rstd, const PT* __restrict__ w,
                                                                 const float* __restrict__ resid, long rows, int d, float* __restrict__ dx32,
                                                                 bf16_t* __restrict__ dx16) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float rs = rstd[r];
    const float4* xr = reinterpret_cast<const float4*>(x + (size_t)r * d);
    const float4* gr = reinterpret_cast<const float4*>(dy + (size_t)r * d);
    const int d4 = d >> 2;
    float s = 0.f;
    for (int e = lane; e < d4; e += 64) {
        const float4 g = gr[e], ww = param4(w, e), xx = xr[e];
        s += g.x * ww.x * xx.x + g.y * ww.y * xx.y + g.z * ww.z * xx.z + g.w * ww.w * xx.w;
    }
    const float c = wave_sum(s) / (float)d * rs * rs;
    for (int e = lane; e < d4; e += 64) {
        const float4 g = gr[e], ww = param4(w, e), xx = xr[e];
        float4 v = {rs * (g.x * ww.x - xx.x * c), rs * (g.y * ww.y - xx.y * c), rs * (g.z * ww.z - xx.z * c), rs * (g.w * ww.w - xx.w * c)};
        if (resid) {
            const float4 q = reinterpret_cast<const float4*>(resid + (size_t)r * d)[e];
            v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
        }
        if (dx32) reinterpret_cast<float4*>(dx32 + (size_t)r * d)[e] = v;
        if (dx16) reinterpret_cast<bf16x4*>(dx16 + (size_t)r * d)[e] = bf16x4{(bf16_t)v.x, (bf16_t)v.y, (bf16_t)v.z, (bf16_t)v.w};
    }
}

// ---- RoPE in place on the first `heads` heads of each row of buf (pitch ld), one wave per row: lane i owns the pair (i, i + 64) ----------
// position pos0 + (r mod rows_per_b), clamped into the table; sgn = -1 rotates by the negated angle (the transposed rotation).  img16
// (rows, ld) given: the bf16 image of the whole row after the rotation, the columns behind the rotated heads included.
__global__ void __launch_bounds__(256) llama_body_rope_kernel(float* __restrict__ buf, int ld, long rows, int rows_per_b, int pos0, int heads,
                                                              int max_len, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                              float sgn, bf16_t* __restrict__ img16) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    int p = pos0 + (int)(r % rows_per_b);
    p = p < 0 ? 0 : p >= max_len ? max_len - 1 : p;
    const float c = cos_t[p * HP + lane], s = sin_t[p * HP + lane] * sgn;
    float* row = buf + (size_t)r * ld;
    bf16_t* img = img16 ? img16 + (size_t)r * ld : nullptr;
    for (int hh = 0; hh < heads; ++hh) {
        float* b = row + hh * HD;
        const float x1 = b[lane], x2 = b[lane + HP];
        const float y1 = x1 * c - x2 * s, y2 = x2 * c + x1 * s;
        b[lane] = y1;
        b[lane + HP] = y2;
        if (img) {
            img[hh * HD + lane] = (bf16_t)y1;
            img[hh * HD + lane + HP] = (bf16_t)y2;
        }
    }
    if (img)
        for (int e = heads * HD + lane; e < ld; e += 64) img[e] = (bf16_t)row[e];
}

// ---- dense causal attention forward: the kernels of attn_gqa128.hpp over these rows -------------------------------------------------------
// grid (b, K/V head, query tile REVERSED out of `tiles`).  Query position p >= q_from is row b Sq + p - q_from of q / out / lse
// (Sq = S - q_from); a tile that lies wholly below q_from or past S is empty.
struct DenseRows {
    const float *q, *k, *v;
    int ldq, ldkv, S, q_from, tiles;
    float* lse;
    struct Tile {
        const float *q, *k, *v;
        int ldq, ldkv, t0, from, S;
        size_t row0;
        float* lse;
        bool empty;
    };
    __device__ __forceinline__ Tile tile(int) const {
        const int b = blockIdx.x, kvh = blockIdx.y, t0 = (tiles - 1 - (int)blockIdx.z) * QT;
        return Tile{q, k + (size_t)b * S * ldkv + kvh * HD, v + (size_t)b * S * ldkv + kvh * HD, ldq, ldkv, t0, q_from, S,
                    (size_t)b * (S - q_from), lse, t0 >= S || t0 + QT <= q_from};
    }
};

// ---- backward, tail queries: dQ against all keys --------------------------------------------------------------------------------------------
// grid (b, head, query tile), one wave: 32 aligned positions, two lanes a query (head columns 64 hf .. 64 hf + 63 of q, dout and dq in
// registers), K / V tiles through LDS.  q / dout / out: the tail rows b Sq + t (pitch ldq for q, 128 H for dout / out); lse (B Sq, H).
__global__ void __launch_bounds__(64) llama_body_attn_bwd_q_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k,
                                                                   const float* __restrict__ v, int ldkv, const float* __restrict__ dout,
                                                                   const float* __restrict__ out, const float* __restrict__ lse, int S,
                                                                   int H, int G, int q_from, float scale, float* __restrict__ dqo, int ldd) {
    __shared__ float4 Ks[KT * HD / 4];
    __shared__ float4 Vs[KT * HD / 4];
    const int lane = threadIdx.x, qi = lane >> 1, hf = lane & 1;
    const int b = blockIdx.x, h = blockIdx.y, kvh = h / G;
    const int t0 = (q_from / QT + (int)blockIdx.z) * QT;
    if (t0 >= S) return;
    const int Sq = S - q_from, dq = H * HD;
    const int pn = t0 + qi;
    const bool live = pn >= q_from && pn < S;
    const int pc = pn < q_from ? q_from : pn >= S ? S - 1 : pn;
    const size_t qrow = (size_t)b * Sq + (pc - q_from);
    const float* kb = k + (size_t)b * S * ldkv + kvh * HD;
    const float* vb = v + (size_t)b * S * ldkv + kvh * HD;
    float qr[HD / 2], go[HD / 2], acc[HD / 2];
    float D = 0.f;
    {
        const float4* qp = reinterpret_cast<const float4*>(q + qrow * ldq + h * HD + (HD / 2) * hf);
        const float4* gp = reinterpret_cast<const float4*>(dout + qrow * dq + h * HD + (HD / 2) * hf);
        const float4* op = reinterpret_cast<const float4*>(out + qrow * dq + h * HD + (HD / 2) * hf);
#pragma unroll
        for (int e = 0; e < HD / 8; ++e) {
            const float4 x = qp[e], gg = gp[e], o = op[e];
            qr[4 * e] = x.x * scale; qr[4 * e + 1] = x.y * scale; qr[4 * e + 2] = x.z * scale; qr[4 * e + 3] = x.w * scale;
            go[4 * e] = gg.x; go[4 * e + 1] = gg.y; go[4 * e + 2] = gg.z; go[4 * e + 3] = gg.w;
            D += gg.x * o.x + gg.y * o.y + gg.z * o.z + gg.w * o.w;
        }
        D += IMMTSF_DPP(D, 0xB1);
    }
#pragma unroll
    for (int e = 0; e < HD / 2; ++e) acc[e] = 0.f;
    const float Lq = lse[qrow * H + h];
    const int kend = min(t0 + QT, S);
    for (int j0 = 0; j0 < kend; j0 += KT) {
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < KT * HD / 4 / 64; ++i) {
            const int idx = lane + 64 * i, kk = idx >> 5, part = idx & 31, j = j0 + kk;
            float4 a = {0.f, 0.f, 0.f, 0.f}, c = a;
            if (j < kend) {
                a = reinterpret_cast<const float4*>(kb + (size_t)j * ldkv)[part];
                c = reinterpret_cast<const float4*>(vb + (size_t)j * ldkv)[part];
            }
            Ks[idx] = a;
            Vs[idx] = c;
        }
        __syncthreads();
#pragma unroll 1
        for (int c = 0; c < KT && j0 + c < kend; ++c) {
            float s = 0.f, dA = 0.f;
#pragma unroll
            for (int e = 0; e < HD / 8; ++e) {
                const float4 kk = Ks[c * (HD / 4) + (HD / 8) * hf + e], vv = Vs[c * (HD / 4) + (HD / 8) * hf + e];
                s += qr[4 * e] * kk.x + qr[4 * e + 1] * kk.y + qr[4 * e + 2] * kk.z + qr[4 * e + 3] * kk.w;
                dA += go[4 * e] * vv.x + go[4 * e + 1] * vv.y + go[4 * e + 2] * vv.z + go[4 * e + 3] * vv.w;
            }
            s += IMMTSF_DPP(s, 0xB1);
            dA += IMMTSF_DPP(dA, 0xB1);
            const float p = (j0 + c <= pn) ? __expf(s - Lq) : 0.f;
            const float dS = p * (dA - D);
#pragma unroll
            for (int e = 0; e < HD / 8; ++e) {
                const float4 kk = Ks[c * (HD / 4) + (HD / 8) * hf + e];
                acc[4 * e] += dS * kk.x; acc[4 * e + 1] += dS * kk.y; acc[4 * e + 2] += dS * kk.z; acc[4 * e + 3] += dS * kk.w;
            }
        }
    }
    if (!live) return;
    float4* dp = reinterpret_cast<float4*>(dqo + qrow * ldd + h * HD + (HD / 2) * hf);
#pragma unroll
    for (int e = 0; e < HD / 8; ++e) dp[e] = float4{acc[4 * e] * scale, acc[4 * e + 1] * scale, acc[4 * e + 2] * scale, acc[4 * e + 3] * scale};
}

// ---- backward, tail keys: dK / dV from the tail queries (no other query sees a tail key) -----------------------------------------------------
// grid (b, K/V head, tile of UT tail keys), one wave: four lanes a key (head columns 32 qu .. 32 qu + 31 of k, v, dk and dv in
// registers).  The G query heads of the K/V head in order, inside a head the queries t >= u0 in order, QB at a time through LDS (q and
// dout rows, lse and D = dout . out).
__global__ void __launch_bounds__(64) llama_body_attn_bwd_kv_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k,
                                                                    const float* __restrict__ v, int ldkv, const float* __restrict__ dout,
                                                                    const float* __restrict__ out, const float* __restrict__ lse, int S,
                                                                    int H, int G, int q_from, float scale, float* __restrict__ dk,
                                                                    float* __restrict__ dv, int ldd) {
    __shared__ float4 Qs[QB * HD / 4];
    __shared__ float4 Gs[QB * HD / 4];
    __shared__ float Ls[QB], Ds[QB];
    const int lane = threadIdx.x, ki = lane >> 2, qu = lane & 3;
    const int b = blockIdx.x, kvh = blockIdx.y, u0 = blockIdx.z * UT;
    const int Sq = S - q_from, dq = H * HD;
    if (u0 >= Sq) return;
    const bool live = u0 + ki < Sq;
    const int u = live ? u0 + ki : Sq - 1;
    float kr[HD / 4], vr[HD / 4], ak[HD / 4], av[HD / 4];
    {
        const float4* kp = reinterpret_cast<const float4*>(k + ((size_t)b * S + q_from + u) * ldkv + kvh * HD + (HD / 4) * qu);
        const float4* vp = reinterpret_cast<const float4*>(v + ((size_t)b * S + q_from + u) * ldkv + kvh * HD + (HD / 4) * qu);
#pragma unroll
        for (int e = 0; e < HD / 16; ++e) {
            const float4 x = kp[e], y = vp[e];
            kr[4 * e] = x.x; kr[4 * e + 1] = x.y; kr[4 * e + 2] = x.z; kr[4 * e + 3] = x.w;
            vr[4 * e] = y.x; vr[4 * e + 1] = y.y; vr[4 * e + 2] = y.z; vr[4 * e + 3] = y.w;
        }
    }
#pragma unroll
    for (int e = 0; e < HD / 4; ++e) { ak[e] = 0.f; av[e] = 0.f; }
    for (int gh = 0; gh < G; ++gh) {
        const int h = kvh * G + gh;
        for (int tq0 = u0; tq0 < Sq; tq0 += QB) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < QB * HD / 4 / 64; ++i) {
                const int idx = lane + 64 * i, tt = idx >> 5, part = idx & 31, t = tq0 + tt;
                float4 a = {0.f, 0.f, 0.f, 0.f}, c = a;
                if (t < Sq) {
                    a = reinterpret_cast<const float4*>(q + ((size_t)b * Sq + t) * ldq + h * HD)[part];
                    c = reinterpret_cast<const float4*>(dout + ((size_t)b * Sq + t) * dq + h * HD)[part];
                }
                Qs[idx] = a;
                Gs[idx] = c;
            }
            {       // D of query tq0 + ki by its four lanes (every lane takes part in the exchange; a row past the end gives 0)
                const int t = tq0 + ki;
                float Dp = 0.f;
                if (t < Sq) {
                    const float4* gp = reinterpret_cast<const float4*>(dout + ((size_t)b * Sq + t) * dq + h * HD + (HD / 4) * qu);
                    const float4* op = reinterpret_cast<const float4*>(out + ((size_t)b * Sq + t) * dq + h * HD + (HD / 4) * qu);
#pragma unroll
                    for (int e = 0; e < HD / 16; ++e) {
                        const float4 gg = gp[e], o = op[e];
                        Dp += gg.x * o.x + gg.y * o.y + gg.z * o.z + gg.w * o.w;
                    }
                }
                Dp += IMMTSF_DPP(Dp, 0xB1);
                Dp += IMMTSF_DPP(Dp, 0x4E);
                if (qu == 0) {
                    Ds[ki] = Dp;
                    Ls[ki] = t < Sq ? lse[((size_t)b * Sq + t) * H + h] : 0.f;
                }
            }
            __syncthreads();
#pragma unroll 1
            for (int c = 0; c < QB && tq0 + c < Sq; ++c) {
                const int t = tq0 + c;
                float s = 0.f, dA = 0.f;
#pragma unroll
                for (int e = 0; e < HD / 16; ++e) {
                    const float4 qq = Qs[c * (HD / 4) + (HD / 16) * qu + e], gg = Gs[c * (HD / 4) + (HD / 16) * qu + e];
                    s += kr[4 * e] * qq.x + kr[4 * e + 1] * qq.y + kr[4 * e + 2] * qq.z + kr[4 * e + 3] * qq.w;
                    dA += vr[4 * e] * gg.x + vr[4 * e + 1] * gg.y + vr[4 * e + 2] * gg.z + vr[4 * e + 3] * gg.w;
                }
                s += IMMTSF_DPP(s, 0xB1);
                s += IMMTSF_DPP(s, 0x4E);
                dA += IMMTSF_DPP(dA, 0xB1);
                dA += IMMTSF_DPP(dA, 0x4E);
                const float p = (u <= t) ? __expf(s * scale - Ls[c]) : 0.f;
                const float dS = p * (dA - Ds[c]) * scale;
#pragma unroll
                for (int e = 0; e < HD / 16; ++e) {
                    const float4 qq = Qs[c * (HD / 4) + (HD / 16) * qu + e], gg = Gs[c * (HD / 4) + (HD / 16) * qu + e];
                    ak[4 * e] += dS * qq.x; ak[4 * e + 1] += dS * qq.y; ak[4 * e + 2] += dS * qq.z; ak[4 * e + 3] += dS * qq.w;
                    av[4 * e] += p * gg.x; av[4 * e + 1] += p * gg.y; av[4 * e + 2] += p * gg.z; av[4 * e + 3] += p * gg.w;
                }
            }
        }
    }
    if (!live) return;
    float4* dkp = reinterpret_cast<float4*>(dk + ((size_t)b * Sq + u) * ldd + kvh * HD + (HD / 4) * qu);
    float4* dvp = reinterpret_cast<float4*>(dv + ((size_t)b * Sq + u) * ldd + kvh * HD + (HD / 4) * qu);
#pragma unroll
    for (int e = 0; e < HD / 16; ++e) {
        dkp[e] = float4{ak[4 * e], ak[4 * e + 1], ak[4 * e + 2], ak[4 * e + 3]};
        dvp[e] = float4{av[4 * e], av[4 * e + 1], av[4 * e + 2], av[4 * e + 3]};
    }
}

// ---- SwiGLU backward: act = silu(a) b over gu = a | b (rows, 2 inner); dgu = dact b silu'(a) | dact silu(a) -----------------------------------
__device__ __forceinline__ void swiglu_grad(float a, float b, float g, float& da, float& db) {
    const float sg = 1.f / (1.f + expf(-a));
    da = g * b * sg * (1.f + a * (1.f - sg));
    db = g * a * sg;
}

__global__ void __launch_bounds__(256) llama_body_swiglu_bwd_kernel(const float* __restrict__ gu, const float* __restrict__ dact, size_t n4,
                                                                    int inner4, float* __restrict__ d32, bf16_t* __restrict__ d16) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / (size_t)inner4, c = i - r * (size_t)inner4;
        const size_t ia = r * 2 * inner4 + c, ib = ia + inner4;
        const float4 a = reinterpret_cast<const float4*>(gu)[ia], b = reinterpret_cast<const float4*>(gu)[ib];
        const float4 g = reinterpret_cast<const float4*>(dact)[i];
        float4 da, db;
        swiglu_grad(a.x, b.x, g.x, da.x, db.x);
        swiglu_grad(a.y, b.y, g.y, da.y, db.y);
        swiglu_grad(a.z, b.z, g.z, da.z, db.z);
        swiglu_grad(a.w, b.w, g.w, da.w, db.w);
        if (d32) {
            reinterpret_cast<float4*>(d32)[ia] = da;
            reinterpret_cast<float4*>(d32)[ib] = db;
        }
        if (d16) {
            reinterpret_cast<bf16x4*>(d16)[ia] = bf16x4{(bf16_t)da.x, (bf16_t)da.y, (bf16_t)da.z, (bf16_t)da.w};
            reinterpret_cast<bf16x4*>(d16)[ib] = bf16x4{(bf16_t)db.x, (bf16_t)db.y, (bf16_t)db.z, (bf16_t)db.w};
        }
    }
}

inline bool group_ok(int H, int Hkv) {
    if (H <= 0 || Hkv <= 0 || H % Hkv) return false;
    const int G = H / Hkv;
    return G == 1 || G == 2 || G == 4 || G == 8;
}

int attn_args_ok(const float* q, int32_t ldq, const float* k, const float* v, int32_t ldkv, int32_t B, int32_t S, int32_t H, int32_t H_kv,
                 int32_t q_from) {
    if (!q || !k || !v || B <= 0 || H <= 0 || H_kv <= 0 || S <= 0 || q_from < 0 || q_from >= S) return IMMTSF_EINVAL;
    if (!group_ok(H, H_kv) || H > 65535 || S > MAXS || (int64_t)B * S > 0x7fffffffLL / 4) return IMMTSF_EUNSUPPORTED;
    if (ldq < H * HD || ldkv < H_kv * HD || (ldq & 3) || (ldkv & 3) || !al16(q) || !al16(k) || !al16(v)) return IMMTSF_EUNSUPPORTED;
    return IMMTSF_OK;
}

template <int G>
void launch_fwd(dim3 grid, hipStream_t s, int32_t precision, const float* q, int32_t ldq, const float* k, const float* v, int32_t ldkv, int32_t S,
                int32_t H, int32_t q_from, int32_t tiles, float scale, float* out32, void* out16, float* lse) {
    const DenseRows rows = {q, k, v, ldq, ldkv, S, q_from, tiles, lse};
    if (precision == 1)
        hipLaunchKernelGGL((gqa128::attn_mfma_kernel<G, DenseRows>), grid, dim3(64 * G), 0, s, rows, H, scale, out32, static_cast<bf16_t*>(out16));
    else
        hipLaunchKernelGGL((gqa128::attn_valu_kernel<G, DenseRows>), grid, dim3(64 * G), 0, s, rows, H, scale, out32, static_cast<bf16_t*>(out16));
}

// a parameter pointer is aligned for the four-element loads of its type
inline bool param_al(const float* p) { return al16(p); }
inline bool param_al(const bf16_t* p) { return al8(p); }

template <typename PT>
int launch_rms(const float* xin, int32_t B, int32_t S_in, int32_t s_from, int32_t d, const float* y, float* xout, const PT* w, float eps,
               float* out32, void* out16, float* rstd, immtsf_stream_t stream) {
    if (!xin || !w || B <= 0 || d <= 0 || s_from < 0 || s_from >= S_in || (!out32 && !out16 && !rstd) || (y && !xout)) return IMMTSF_EINVAL;
    if ((d & 3) || !al16(xin) || !param_al(w) || (y && (!al16(y) || !al16(xout))) || (out32 && !al16(out32)) || (out16 && !al8(out16)))
        return IMMTSF_EUNSUPPORTED;
    const int Sn = S_in - s_from;
    const long rows = (long)B * Sn;
    if (rows > 0x7fffffffL) return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(llama_body_rms_kernel<PT>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), xin, S_in,
                       s_from, Sn, y, xout, rows, d, w, eps, out32, static_cast<bf16_t*>(out16), rstd);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

template <typename PT>
int launch_rms_bwd(const float* dy, const float* x, const float* rstd, const PT* w, const float* resid, int64_t rows, int32_t d, float* dx32,
                   void* dx16, immtsf_stream_t stream) {
    if (!dy || !x || !rstd || !w || (!dx32 && !dx16) || rows <= 0 || d <= 0) return IMMTSF_EINVAL;
    if (rows > 0x7fffffffLL || (d & 3) || !al16(dy) || !al16(x) || !param_al(w) || (resid && !al16(resid)) || (dx32 && !al16(dx32)) ||
        (dx16 && !al8(dx16)))
        return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(llama_body_rms_bwd_kernel<PT>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), dy, x, rstd,
                       w, resid, (long)rows, d, dx32, static_cast<bf16_t*>(dx16));
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // namespace

extern "C" {

int immtsf_llama_body_supported(int32_t d, int32_t H, int32_t H_kv, int32_t inner, int32_t S, int32_t max_positions) {
    return d > 0 && (d & 7) == 0 && inner > 0 && (inner & 7) == 0 && group_ok(H, H_kv) && H <= 65535 && S >= 1 && S <= max_positions &&
           S <= MAXS;
}

int immtsf_llama_body_rmsnorm(const float* xin, int32_t B, int32_t S_in, int32_t s_from, int32_t d, const float* y, float* xout, const float* w,
                              float eps, float* out32, void* out16, float* rstd, immtsf_stream_t stream) {
    return launch_rms(xin, B, S_in, s_from, d, y, xout, w, eps, out32, out16, rstd, stream);
}

// the _p16 entry points: the same kernels with the RMSNorm weight read as bf16 (a model stored in bf16)
int immtsf_llama_body_rmsnorm_p16(const float* xin, int32_t B, int32_t S_in, int32_t s_from, int32_t d, const float* y, float* xout,
                                  const void* w16, float eps, float* out32, void* out16, float* rstd, immtsf_stream_t stream) {
    return launch_rms(xin, B, S_in, s_from, d, y, xout, static_cast<const bf16_t*>(w16), eps, out32, out16, rstd, stream);
}

int immtsf_llama_body_rmsnorm_backward_p16(const float* dy, const float* x, const float* rstd, const void* w16, const float* resid,
                                           int64_t rows, int32_t d, float* dx32, void* dx16, immtsf_stream_t stream) {
    return launch_rms_bwd(dy, x, rstd, static_cast<const bf16_t*>(w16), resid, rows, d, dx32, dx16, stream);
}

int immtsf_llama_body_rmsnorm_backward(const float* dy, const float* x, const float* rstd, const float* w, const float* resid, int64_t rows,
                                       int32_t d, float* dx32, void* dx16, immtsf_stream_t stream) {
    return launch_rms_bwd(dy, x, rstd, w, resid, rows, d, dx32, dx16, stream);
}

int immtsf_llama_body_rope(float* buf, int32_t ld, int64_t rows, int32_t rows_per_b, int32_t pos0, int32_t heads, int32_t max_len,
                           const float* cos_t, const float* sin_t, int32_t transposed, void* img16, immtsf_stream_t stream) {
    if (!buf || !cos_t || !sin_t || rows <= 0 || rows_per_b <= 0 || pos0 < 0 || heads <= 0 || max_len <= 0) return IMMTSF_EINVAL;
    if (rows > 0x7fffffffLL || max_len > MAXS || (int64_t)ld < (int64_t)heads * HD) return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(llama_body_rope_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), buf, ld,
                       (long)rows, rows_per_b, pos0, heads, max_len, cos_t, sin_t, transposed ? -1.f : 1.f, static_cast<bf16_t*>(img16));
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_llama_body_attention_forward(const float* q, int32_t ldq, const float* k, const float* v, int32_t ldkv, int32_t B, int32_t S,
                                        int32_t H, int32_t H_kv, int32_t q_from, float scale, int32_t precision, float* out32, void* out16,
                                        float* lse, immtsf_stream_t stream) {
    if (int rc = attn_args_ok(q, ldq, k, v, ldkv, B, S, H, H_kv, q_from)) return rc;
    if ((!out32 && !out16) || precision < 0 || precision > 1) return IMMTSF_EINVAL;
    if ((out32 && !al16(out32)) || (out16 && !al8(out16))) return IMMTSF_EUNSUPPORTED;
    const int tiles = (S + QT - 1) / QT;
    const dim3 grid((unsigned)B, (unsigned)H_kv, (unsigned)(tiles - q_from / QT));
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (H / H_kv) {
        case 1: launch_fwd<1>(grid, s, precision, q, ldq, k, v, ldkv, S, H, q_from, tiles, scale, out32, out16, lse); break;
        case 2: launch_fwd<2>(grid, s, precision, q, ldq, k, v, ldkv, S, H, q_from, tiles, scale, out32, out16, lse); break;
        case 4: launch_fwd<4>(grid, s, precision, q, ldq, k, v, ldkv, S, H, q_from, tiles, scale, out32, out16, lse); break;
        default: launch_fwd<8>(grid, s, precision, q, ldq, k, v, ldkv, S, H, q_from, tiles, scale, out32, out16, lse); break;
    }
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_llama_body_attention_backward(const float* q, int32_t ldq, const float* k, const float* v, int32_t ldkv, const float* dout,
                                         const float* out, const float* lse, int32_t B, int32_t S, int32_t H, int32_t H_kv, int32_t q_from,
                                         float scale, float* dq, float* dk, float* dv, int32_t ldd, immtsf_stream_t stream) {
    if (int rc = attn_args_ok(q, ldq, k, v, ldkv, B, S, H, H_kv, q_from)) return rc;
    if (!dout || !out || !lse || !dq || !dk || !dv) return IMMTSF_EINVAL;
    if (ldd < H * HD || (ldd & 3) || !al16(dout) || !al16(out) || !al16(dq) || !al16(dk) || !al16(dv)) return IMMTSF_EUNSUPPORTED;
    const int Sq = S - q_from, G = H / H_kv;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(llama_body_attn_bwd_q_kernel, dim3((unsigned)B, (unsigned)H, (unsigned)((S + QT - 1) / QT - q_from / QT)), dim3(64), 0, s, q,
                       ldq, k, v, ldkv, dout, out, lse, S, H, G, q_from, scale, dq, ldd);
    IMMTSF_LAUNCH_CHECK();
    hipLaunchKernelGGL(llama_body_attn_bwd_kv_kernel, dim3((unsigned)B, (unsigned)H_kv, (unsigned)((Sq + UT - 1) / UT)), dim3(64), 0, s, q, ldq, k,
                       v, ldkv, dout, out, lse, S, H, G, q_from, scale, dk, dv, ldd);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_llama_body_swiglu_backward(const float* gu, const float* dact, int64_t rows, int32_t inner, float* dgu32, void* dgu16,
                                      immtsf_stream_t stream) {
    if (!gu || !dact || (!dgu32 && !dgu16) || rows <= 0 || inner <= 0) return IMMTSF_EINVAL;
    if ((inner & 3) || !al16(gu) || !al16(dact) || (dgu32 && !al16(dgu32)) || (dgu16 && !al8(dgu16))) return IMMTSF_EUNSUPPORTED;
    const size_t n4 = (size_t)rows * (inner / 4);
    hipLaunchKernelGGL(llama_body_swiglu_bwd_kernel, dim3(grid_for(n4, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), gu, dact, n4,
                       inner / 4, dgu32, static_cast<bf16_t*>(dgu16));
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
