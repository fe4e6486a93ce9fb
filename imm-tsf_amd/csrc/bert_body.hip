// TimeLLM's frozen BERT body (reference models/TimeLLM.py: llm_model(inputs_embeds=cat([prompt, patches])) with llm_model_timellm =
// "BERT"): what immtsf.ops.bert_body needs beside the GEMM family and the erf GELU of bert_embed.hip.  Rows are (b, s) with
// s < S = S_p + S_t, dense; the last S_t rows (the reprogrammed patches) are the only ones a gradient is wanted for.  BERT is
// bidirectional and the reference passes no attention mask, so every row of every layer depends on every patch row: unlike the GPT-2 and
// Llama bodies, the backward of a middle layer covers all B S rows.  head_dim 64, d = 64 H, post-LN.
//   * embedding row: dropout(LayerNorm([prefix | tail] + pos[s] + type[0])) without the concatenated copy; for the tail rows the pre-norm
//     sum and the statistics when a backward follows
//   * add + LayerNorm with dropout on the branch: LayerNorm(x + dropout(y)) over a row range of x, compact outputs (fp32, bf16 image, the
//     pre-norm sum, mean / rstd), and its data gradient: dy = dy_a (+ dy_b), d_sum = LayerNorm'(dy), d_branch = undrop(d_sum) -- or, for
//     the embedding (dropout behind the norm), d_sum = LayerNorm'(undrop(dy)).  No parameter gradients: the body is frozen
//   * erf-GELU backward
//   * non-causal attention forward over a query range q_from .. S-1 against all S keys, K / V read from the fused q | k | v product as it
//     lies; dropout on the probabilities (index ((b H + h) S + i) 1024 + j, the GPT-2 convention); the log-sum-exp when a backward
//     follows.  fp32 on the VALU, or both products on bf16 MFMA 16x16x32 with fp32 online softmax (the transposed form of
//     llama_body.hip: S^T = K Q^T, O^T += V^T P^T).  A key at or past S in a partial tile scores -inf: there is no causal mask to hide it
//   * its backward: probabilities recomputed from the log-sum-exp, the mask redrawn; dQ of a query range against all keys, dK / dV of a
//     key range summed over ALL the forward's queries in query order.  fp32 on the VALU, or all four products (S^T / dA^T and the two
//     accumulations) on bf16 MFMA with fp32 softmax arithmetic and accumulators
// One writer per output element, every sum in a fixed order, no atomics: two runs give the same bits.
// The three fp32 VALU attention kernels are the non-CAUSAL instances of attn_dense64.hpp, which the GPT-2 body shares.
#include "../../include/immtsf.h"
#include "attn_dense64.hpp"
#include "common.hpp"

namespace {

using dense64::HD;               // head_dim 64
using dense64::KT;               // 32 keys (or queries) per LDS tile, in the MFMA kernels as in the VALU ones
constexpr int MQ = 32;           // rows (queries, or keys in the dK / dV kernel) a wave owns in the MFMA kernels
constexpr int MW = 4;            // waves per workgroup of the MFMA kernels: they share the streamed tiles
constexpr int RM_LD = HD + 8;    // bf16 tile, row-major [row][e]
constexpr int TR_LD = KT + 8;    // bf16 tile, transposed [e][row]

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return float4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }
__device__ __forceinline__ bf16x4 to_bf4(float4 a) { return bf16x4{(bf16_t)a.x, (bf16_t)a.y, (bf16_t)a.z, (bf16_t)a.w}; }

// LayerNorm of a row whose pre-norm values lane l holds in `stage` (elements 4 (l + 64 i) ..; lane l wrote, and alone reads back, its
// own elements), times the dropout scale of `didx`; writes o32 / o16 (o32 may be the staging row)
__device__ __forceinline__ void ln_finish(const float4* stage, int d4, int lane, float sum, const float* __restrict__ gamma,
                                          const float* __restrict__ beta, float eps, const DropCfg& drop, uint64_t site, size_t didx,
                                          bool drop_out, float4* o32, bf16x4* o16, float* mean_out, float* rstd_out) {
    const float mean = wave_sum(sum) / (float)(4 * d4);
    float v = 0.f;
    for (int e = lane; e < d4; e += 64) {
        const float4 c = stage[e];
        const float a0 = c.x - mean, a1 = c.y - mean, a2 = c.z - mean, a3 = c.w - mean;
        v += a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
    }
    const float rstd = rsqrtf(wave_sum(v) / (float)(4 * d4) + eps);
    for (int e = lane; e < d4; e += 64) {
        const float4 c = stage[e], g = reinterpret_cast<const float4*>(gamma)[e], bb = reinterpret_cast<const float4*>(beta)[e];
        float4 z = {(c.x - mean) * rstd * g.x + bb.x, (c.y - mean) * rstd * g.y + bb.y, (c.z - mean) * rstd * g.z + bb.z,
                    (c.w - mean) * rstd * g.w + bb.w};
        if (drop_out) {
            float sc[4];
            dropout_scale4(drop, site, didx + 4 * (size_t)e, sc);
            z.x *= sc[0]; z.y *= sc[1]; z.z *= sc[2]; z.w *= sc[3];
        }
        if (o32) o32[e] = z;
        if (o16) o16[e] = to_bf4(z);
    }
    if (lane == 0) {
        if (mean_out) *mean_out = mean;
        if (rstd_out) *rstd_out = rstd;
    }
}

// ---- x0[b, s, :] = drop(LayerNorm([prefix | tail][b, s, :] + pos[s, :] + type0)); one wave per row ----------------------------------------
__global__ void __launch_bounds__(256) bert_body_embed_kernel(const float* __restrict__ prefix, const float* __restrict__ tail,
                                                              const float* __restrict__ pos, const float* __restrict__ type0, int B, int S_p,
                                                              int S_t, int d, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, DropCfg drop, uint64_t site,
                                                              float* out32, bf16_t* __restrict__ out16, float* __restrict__ sum_t,
                                                              float* __restrict__ mean_t, float* __restrict__ rstd_t) {
    const int S = S_p + S_t, d4 = d >> 2, lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (long)B * S) return;
    const int b = (int)(r / S), s = (int)(r % S);
    const bool is_tail = s >= S_p;
    const long rt = (long)b * S_t + (s - S_p);
    const float4* src = reinterpret_cast<const float4*>(is_tail ? tail + (size_t)rt * d : prefix + ((size_t)b * S_p + s) * d);
    const float4* pp = reinterpret_cast<const float4*>(pos + (size_t)s * d);
    const float4* tp = reinterpret_cast<const float4*>(type0);
    float4* o = reinterpret_cast<float4*>(out32 + (size_t)r * d);
    float4* st = (is_tail && sum_t) ? reinterpret_cast<float4*>(sum_t + (size_t)rt * d) : nullptr;
    float sum = 0.f;
    for (int e = lane; e < d4; e += 64) {
        const float4 v = add4(add4(src[e], pp[e]), tp[e]);
        o[e] = v;
        if (st) st[e] = v;
        sum += v.x + v.y + v.z + v.w;
    }
    ln_finish(o, d4, lane, sum, gamma, beta, eps, drop, site, (size_t)r * d, true, o,
              out16 ? reinterpret_cast<bf16x4*>(out16 + (size_t)r * d) : nullptr, (is_tail && mean_t) ? mean_t + rt : nullptr,
              (is_tail && rstd_t) ? rstd_t + rt : nullptr);
}

// ---- out[b, t, :] = LayerNorm(xin[b, s_from + t, :] + drop(y[b, t, :])), t < Sn; one wave per row ---------------------------------------
// the dropout index is that of row (b, q_from + t) of a (B, S, d) tensor.  The pre-norm sum is staged in `sum` when given, else in out32.
__global__ void __launch_bounds__(256) bert_body_add_ln_kernel(const float* __restrict__ xin, int S_in, int s_from, int Sn,
                                                               const float* __restrict__ y, int S, int q_from, int d,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                               DropCfg drop, uint64_t site, long rows, float* out32,
                                                               bf16_t* __restrict__ out16, float* sum, float* __restrict__ mean,
                                                               float* __restrict__ rstd) {
    const int d4 = d >> 2, lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const long b = r / Sn, t = r - b * Sn;
    const float4* xr = reinterpret_cast<const float4*>(xin + ((size_t)b * S_in + s_from + t) * d);
    const float4* yr = reinterpret_cast<const float4*>(y + (size_t)r * d);
    float4* o = out32 ? reinterpret_cast<float4*>(out32 + (size_t)r * d) : nullptr;
    float4* stage = sum ? reinterpret_cast<float4*>(sum + (size_t)r * d) : o;
    const size_t didx = ((size_t)b * S + q_from + t) * d;
    float s = 0.f;
    for (int e = lane; e < d4; e += 64) {
        const float4 yv = yr[e], xv = xr[e];
        float sc[4];
        dropout_scale4(drop, site, didx + 4 * (size_t)e, sc);
        const float4 v = {xv.x + yv.x * sc[0], xv.y + yv.y * sc[1], xv.z + yv.z * sc[2], xv.w + yv.w * sc[3]};
        stage[e] = v;
        s += v.x + v.y + v.z + v.w;
    }
    ln_finish(stage, d4, lane, s, gamma, beta, eps, drop, site, 0, false, o, out16 ? reinterpret_cast<bf16x4*>(out16 + (size_t)r * d) : nullptr,
              mean ? mean + r : nullptr, rstd ? rstd + r : nullptr);
}

// ---- data gradient of the two kernels above; rows (b, t), t < Sn; one wave per row --------------------------------------------------------
// dy[b, t] = dy_a[b, sa_from + t] (dy_a (B, Sa, d)) + dy_b[b, t - tb_from] for t >= tb_from (dy_b (B, Sn - tb_from, d), may be NULL);
// sum / mean / rstd compact.  drop_first 0: d_sum = LayerNorm'(dy) -> dx32, undrop(d_sum) -> dbr32 / dbr16.  drop_first 1 (the embedding:
// dropout behind the norm): d_sum = LayerNorm'(undrop(dy)) -> dx32.  The mask is that of row (b, q_from + t) of a (B, S, d) tensor.
__global__ void __launch_bounds__(256) bert_body_ln_bwd_kernel(const float* __restrict__ dy_a, int Sa, int sa_from, int Sn,
                                                               const float* __restrict__ dy_b, int tb_from, const float* __restrict__ sum,
                                                               const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               const float* __restrict__ gamma, int d, int S, int q_from, DropCfg drop,
                                                               uint64_t site, int drop_first, long rows, float* __restrict__ dx32,
                                                               float* __restrict__ dbr32, bf16_t* __restrict__ dbr16) {
    const int d4 = d >> 2, lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const long b = r / Sn, t = r - b * Sn;
    const float4* ga = reinterpret_cast<const float4*>(dy_a + ((size_t)b * Sa + sa_from + t) * d);
    const float4* gb = (dy_b && t >= tb_from) ? reinterpret_cast<const float4*>(dy_b + ((size_t)b * (Sn - tb_from) + (t - tb_from)) * d) : nullptr;
    const float4* xs = reinterpret_cast<const float4*>(sum + (size_t)r * d);
    const float4* gm = reinterpret_cast<const float4*>(gamma);
    const float mu = mean[r], rs = rstd[r];
    const size_t didx = ((size_t)b * S + q_from + t) * d;
    float s1 = 0.f, s2 = 0.f;
    for (int e = lane; e < d4; e += 64) {
        float4 g = ga[e];
        if (gb) g = add4(g, gb[e]);
        if (drop_first) {
            float sc[4];
            dropout_scale4(drop, site, didx + 4 * (size_t)e, sc);
            g.x *= sc[0]; g.y *= sc[1]; g.z *= sc[2]; g.w *= sc[3];
        }
        const float4 w = gm[e], x = xs[e];
        g.x *= w.x; g.y *= w.y; g.z *= w.z; g.w *= w.w;
        s1 += g.x + g.y + g.z + g.w;
        s2 += g.x * ((x.x - mu) * rs) + g.y * ((x.y - mu) * rs) + g.z * ((x.z - mu) * rs) + g.w * ((x.w - mu) * rs);
    }
    s1 = wave_sum(s1) / (float)d;
    s2 = wave_sum(s2) / (float)d;
    for (int e = lane; e < d4; e += 64) {
        float4 g = ga[e];
        if (gb) g = add4(g, gb[e]);
        float sc[4];
        dropout_scale4(drop, site, didx + 4 * (size_t)e, sc);
        if (drop_first) { g.x *= sc[0]; g.y *= sc[1]; g.z *= sc[2]; g.w *= sc[3]; }
        const float4 w = gm[e], x = xs[e];
        const float4 v = {rs * (g.x * w.x - s1 - (x.x - mu) * rs * s2), rs * (g.y * w.y - s1 - (x.y - mu) * rs * s2),
                          rs * (g.z * w.z - s1 - (x.z - mu) * rs * s2), rs * (g.w * w.w - s1 - (x.w - mu) * rs * s2)};
        if (dx32) reinterpret_cast<float4*>(dx32 + (size_t)r * d)[e] = v;
        if (!drop_first && (dbr32 || dbr16)) {
            const float4 u = {v.x * sc[0], v.y * sc[1], v.z * sc[2], v.w * sc[3]};
            if (dbr32) reinterpret_cast<float4*>(dbr32 + (size_t)r * d)[e] = u;
            if (dbr16) reinterpret_cast<bf16x4*>(dbr16 + (size_t)r * d)[e] = to_bf4(u);
        }
    }
}

// ---- dpre = dact gelu'(pre), gelu(x) = x Phi(x): gelu' = Phi(x) + x phi(x) ------------------------------------------------------------------
__device__ __forceinline__ float gelu_erf_grad(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * expf(-0.5f * x * x);
}

__global__ void __launch_bounds__(256) bert_body_gelu_bwd_kernel(const float* __restrict__ pre, const float* __restrict__ dact, size_t n4,
                                                                 float* __restrict__ d32, bf16_t* __restrict__ d16) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(pre)[i], g = reinterpret_cast<const float4*>(dact)[i];
        const float4 o = {g.x * gelu_erf_grad(v.x), g.y * gelu_erf_grad(v.y), g.z * gelu_erf_grad(v.z), g.w * gelu_erf_grad(v.w)};
        if (d32) reinterpret_cast<float4*>(d32)[i] = o;
        if (d16) reinterpret_cast<bf16x4*>(d16)[i] = to_bf4(o);
    }
}

// ---- bf16 MFMA kernels ---------------------------------------------------------------------------------------------------------------------
// v_mfma_f32_16x16x32_bf16, D (16 x 16) += A (16 x 32) B (32 x 16): lane (fr = lane & 15, g = lane >> 4) gives A[fr][8 g .. 8 g + 7] and
// B[8 g .. 8 g + 7][fr] and holds D[4 g .. 4 g + 3][fr].  All kernels compute the score tile TRANSPOSED against the rows a wave owns, so
// that a lane's four results are four consecutive STREAMED rows of one OWNED row: they become the B operand of the accumulating product
// with the streamed index renumbered (the A operand's loads apply the same renumbering: 4 g .. 4 g + 3, then 16 + 4 g .. 16 + 4 g + 3).
__device__ __forceinline__ f32x4 bb_mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// a (rows of a (.., ld) fp32 matrix at `base`, row r0 + kk for kk < KT, valid while row < r_end) -> bf16 row-major tile and, when Tt is
// given, the transposed tile; the whole workgroup (64 MW threads) takes part
__device__ __forceinline__ void stage_tile(const float* __restrict__ base, int ld, int r0, int r_end, int tid, bf16_t* Rm, bf16_t* Tt) {
#pragma unroll
    for (int i = 0; i < KT * HD / 4 / (64 * MW); ++i) {
        const int idx = tid + 64 * MW * i, kk = idx >> 4, part = idx & 15;
        float4 a = {0.f, 0.f, 0.f, 0.f};
        if (r0 + kk < r_end) a = reinterpret_cast<const float4*>(base + (size_t)(r0 + kk) * ld)[part];
        if (Rm) *reinterpret_cast<bf16x4*>(&Rm[kk * RM_LD + 4 * part]) = to_bf4(a);
        if (Tt) {
            Tt[(4 * part + 0) * TR_LD + kk] = (bf16_t)a.x;
            Tt[(4 * part + 1) * TR_LD + kk] = (bf16_t)a.y;
            Tt[(4 * part + 2) * TR_LD + kk] = (bf16_t)a.z;
            Tt[(4 * part + 3) * TR_LD + kk] = (bf16_t)a.w;
        }
    }
}

// the 32 e-columns 32 ks + 8 g .. of row `row` (fp32, global) as a B-operand fragment
__device__ __forceinline__ bf16x8 row_frag(const float* __restrict__ row, int ks, int g) {
    const float4 a = reinterpret_cast<const float4*>(row)[8 * ks + 2 * g], c = reinterpret_cast<const float4*>(row)[8 * ks + 2 * g + 1];
    return bf16x8{(bf16_t)a.x, (bf16_t)a.y, (bf16_t)a.z, (bf16_t)a.w, (bf16_t)c.x, (bf16_t)c.y, (bf16_t)c.z, (bf16_t)c.w};
}
// A-operand fragments out of the LDS tiles: row-major tile rows 16 nt + fr, columns 32 ks + 8 g ..; transposed tile row 16 et + fr,
// streamed rows 4 g .. 4 g + 3 and 16 + 4 g .. 16 + 4 g + 3
__device__ __forceinline__ bf16x8 rm_frag(const bf16_t* Rm, int nt, int ks, int fr, int g) {
    return *reinterpret_cast<const bf16x8*>(&Rm[(16 * nt + fr) * RM_LD + 32 * ks + 8 * g]);
}
__device__ __forceinline__ bf16x8 tr_frag(const bf16_t* Tt, int et, int fr, int g) {
    const bf16x4 lo = *reinterpret_cast<const bf16x4*>(&Tt[(16 * et + fr) * TR_LD + 4 * g]);
    const bf16x4 hi = *reinterpret_cast<const bf16x4*>(&Tt[(16 * et + fr) * TR_LD + 16 + 4 * g]);
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// forward.  grid (b, head, blocks of MW query tiles); wave w owns the MQ aligned positions t0 .. t0 + 31; a position below q_from or at /
// past S is idle: it repeats a live query and writes nothing.  A wave whose tile starts at or past S only helps to stage the tiles.
__global__ void __launch_bounds__(64 * MW) bert_body_attn_mfma_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k,
                                                                      const float* __restrict__ v, int ldkv, int S, int H, int q_from,
                                                                      float scale, DropCfg drop, uint64_t site, float* __restrict__ o32,
                                                                      bf16_t* __restrict__ o16, float* __restrict__ lse) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[KT * RM_LD];
    __shared__ __attribute__((aligned(16))) bf16_t Vt[HD * TR_LD];
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, g = lane >> 4;
    const int b = blockIdx.x, h = blockIdx.y;
    const int t0 = (q_from / MQ + ((int)blockIdx.z * MW + (tid >> 6))) * MQ;
    const bool active = t0 < S;
    const int Sq = S - q_from, dq = H * HD;
    const float* kb = k + (size_t)b * S * ldkv + h * HD;
    const float* vb = v + (size_t)b * S * ldkv + h * HD;
    bf16x8 qf[2][2];
    size_t drow[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int pn = t0 + 16 * mt + fr;
        const int pc = pn < q_from ? q_from : pn >= S ? S - 1 : pn;
        const float* qp = q + ((size_t)b * Sq + (pc - q_from)) * ldq + h * HD;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) qf[mt][ks] = row_frag(qp, ks, g);
        drow[mt] = (((size_t)b * H + h) * S + pc) * ATT_STRIDE;
    }
    f32x4 O[2][4];
    float m[2], ls[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        m[mt] = -INFINITY;
        ls[mt] = 0.f;
#pragma unroll
        for (int et = 0; et < 4; ++et) O[mt][et] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int j0 = 0; j0 < S; j0 += KT) {
        __syncthreads();
        stage_tile(kb, ldkv, j0, S, tid, Ks, nullptr);
        stage_tile(vb, ldkv, j0, S, tid, nullptr, Vt);
        __syncthreads();
        if (!active) continue;
        bf16x8 kf[2][2], vf[4];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) kf[nt][ks] = rm_frag(Ks, nt, ks, fr, g);
#pragma unroll
        for (int et = 0; et < 4; ++et) vf[et] = tr_frag(Vt, et, fr, g);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            float s[2][4];
            float cmax = -INFINITY;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                f32x4 Sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) Sc = bb_mfma(kf[nt][ks], qf[mt][ks], Sc);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    s[nt][i] = (j0 + 16 * nt + 4 * g + i < S) ? Sc[i] * scale : -INFINITY;
                    cmax = fmaxf(cmax, s[nt][i]);
                }
            }
            cmax = xor32_max(xor16_max(cmax));              // over the 32 keys of the tile (key j0 is real: finite)
            const float mn = fmaxf(m[mt], cmax);
            const float corr = __expf(m[mt] - mn);
            m[mt] = mn;
            float psum = 0.f;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                float ds[4];
                dropout_scale4(drop, site, drow[mt] + (size_t)(j0 + 16 * nt + 4 * g), ds);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float p = __expf(s[nt][i] - mn);
                    psum += p;
                    s[nt][i] = p * ds[i];
                }
            }
            ls[mt] = ls[mt] * corr + psum;
            const bf16x8 pf = bf16x8{(bf16_t)s[0][0], (bf16_t)s[0][1], (bf16_t)s[0][2], (bf16_t)s[0][3],
                                     (bf16_t)s[1][0], (bf16_t)s[1][1], (bf16_t)s[1][2], (bf16_t)s[1][3]};
#pragma unroll
            for (int et = 0; et < 4; ++et) {
                f32x4 o = O[mt][et];
                o[0] *= corr; o[1] *= corr; o[2] *= corr; o[3] *= corr;
                O[mt][et] = bb_mfma(vf[et], pf, o);
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const float l = xor32_sum(xor16_sum(ls[mt]));        // shares of lanes fr, fr + 16, fr + 32, fr + 48 in one fixed order
        const int pn = t0 + 16 * mt + fr;
        if (pn < q_from || pn >= S) continue;
        const float inv = 1.f / l;
        const size_t qrow = (size_t)b * Sq + (pn - q_from);
        const size_t orow = qrow * dq + h * HD + 4 * g;
#pragma unroll
        for (int et = 0; et < 4; ++et) {
            const f32x4 o = O[mt][et];
            if (o32) *reinterpret_cast<float4*>(o32 + orow + 16 * et) = float4{o[0] * inv, o[1] * inv, o[2] * inv, o[3] * inv};
            if (o16)
                *reinterpret_cast<bf16x4*>(o16 + orow + 16 * et) =
                    bf16x4{(bf16_t)(o[0] * inv), (bf16_t)(o[1] * inv), (bf16_t)(o[2] * inv), (bf16_t)(o[3] * inv)};
        }
        if (lse && g == 0) lse[((size_t)b * H + h) * Sq + (pn - q_from)] = m[mt] + __logf(l);
    }
}

// D[t] = dout[t] . out[t] per (query row, head): one lane a (row, head), for the MFMA backward kernels.  dsum (B Sq, H).
__global__ void __launch_bounds__(256) bert_body_attn_dsum_kernel(const float* __restrict__ dout, const float* __restrict__ out, long n, int H,
                                                                  float* __restrict__ dsum) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4* gp = reinterpret_cast<const float4*>(dout + (size_t)i * HD);
    const float4* op = reinterpret_cast<const float4*>(out + (size_t)i * HD);
    float D = 0.f;
#pragma unroll
    for (int e = 0; e < HD / 4; ++e) {
        const float4 gg = gp[e], o = op[e];
        D += gg.x * o.x + gg.y * o.y + gg.z * o.z + gg.w * o.w;
    }
    dsum[i] = D;
}

// MFMA backward, dQ: wave w owns the MQ aligned query positions t0 .. (as the forward, from dq_from on); key tiles stream through LDS
// (K row-major and transposed, V row-major).  S^T = K Q^T and dA^T = V dO^T give, per lane, four keys of query fr; dS^T = P^T (mask dA^T
// - D) becomes the B operand of dQ^T += K^T dS^T.
__global__ void __launch_bounds__(64 * MW) bert_body_attn_bwd_q_mfma_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k,
                                                                            const float* __restrict__ v, int ldkv,
                                                                            const float* __restrict__ dout, const float* __restrict__ dsum,
                                                                            const float* __restrict__ lse, int S, int H, int q_from,
                                                                            int dq_from, float scale, DropCfg drop, uint64_t site,
                                                                            float* __restrict__ dqo, int dq_rows, int ldd) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[KT * RM_LD];
    __shared__ __attribute__((aligned(16))) bf16_t Vs[KT * RM_LD];
    __shared__ __attribute__((aligned(16))) bf16_t Kt[HD * TR_LD];
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, g = lane >> 4;
    const int b = blockIdx.x, h = blockIdx.y;
    const int t0 = (dq_from / MQ + ((int)blockIdx.z * MW + (tid >> 6))) * MQ;
    const bool active = t0 < S;
    const int Sq = S - q_from, dq = H * HD;
    const float* kb = k + (size_t)b * S * ldkv + h * HD;
    const float* vb = v + (size_t)b * S * ldkv + h * HD;
    bf16x8 qf[2][2], gf[2][2];
    size_t drow[2];
    float Lq[2], Dq[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int pn = t0 + 16 * mt + fr;
        const int pc = pn < dq_from ? dq_from : pn >= S ? S - 1 : pn;
        const size_t qrow = (size_t)b * Sq + (pc - q_from);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            qf[mt][ks] = row_frag(q + qrow * ldq + h * HD, ks, g);
            gf[mt][ks] = row_frag(dout + qrow * dq + h * HD, ks, g);
        }
        drow[mt] = (((size_t)b * H + h) * S + pc) * ATT_STRIDE;
        Lq[mt] = lse[((size_t)b * H + h) * Sq + (pc - q_from)];
        Dq[mt] = dsum[qrow * H + h];
    }
    f32x4 A[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int et = 0; et < 4; ++et) A[mt][et] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < S; j0 += KT) {
        __syncthreads();
        stage_tile(kb, ldkv, j0, S, tid, Ks, Kt);
        stage_tile(vb, ldkv, j0, S, tid, Vs, nullptr);
        __syncthreads();
        if (!active) continue;
        bf16x8 kf[2][2], vf[2][2], ktf[4];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                kf[nt][ks] = rm_frag(Ks, nt, ks, fr, g);
                vf[nt][ks] = rm_frag(Vs, nt, ks, fr, g);
            }
#pragma unroll
        for (int et = 0; et < 4; ++et) ktf[et] = tr_frag(Kt, et, fr, g);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            float s[2][4];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                f32x4 Sc = {0.f, 0.f, 0.f, 0.f}, dA = Sc;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    Sc = bb_mfma(kf[nt][ks], qf[mt][ks], Sc);
                    dA = bb_mfma(vf[nt][ks], gf[mt][ks], dA);
                }
                float ds[4];
                dropout_scale4(drop, site, drow[mt] + (size_t)(j0 + 16 * nt + 4 * g), ds);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float p = (j0 + 16 * nt + 4 * g + i < S) ? __expf(Sc[i] * scale - Lq[mt]) : 0.f;
                    s[nt][i] = p * (ds[i] * dA[i] - Dq[mt]);
                }
            }
            const bf16x8 sf = bf16x8{(bf16_t)s[0][0], (bf16_t)s[0][1], (bf16_t)s[0][2], (bf16_t)s[0][3],
                                     (bf16_t)s[1][0], (bf16_t)s[1][1], (bf16_t)s[1][2], (bf16_t)s[1][3]};
#pragma unroll
            for (int et = 0; et < 4; ++et) A[mt][et] = bb_mfma(ktf[et], sf, A[mt][et]);
        }
    }
    if (!active) return;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int pn = t0 + 16 * mt + fr;
        if (pn < dq_from || pn >= S) continue;
        float* dp = dqo + ((size_t)b * dq_rows + (pn - dq_from)) * ldd + h * HD + 4 * g;
#pragma unroll
        for (int et = 0; et < 4; ++et) {
            const f32x4 a = A[mt][et];
            *reinterpret_cast<float4*>(dp + 16 * et) = float4{a[0] * scale, a[1] * scale, a[2] * scale, a[3] * scale};
        }
    }
}

// MFMA backward, dK / dV: the same skeleton with the roles exchanged.  Wave w owns the MQ aligned key positions u0 .. (from k_from on);
// tiles of KT queries stream through LDS (Q and dO row-major and transposed, lse and D).  S = Q K^T and dA = dO V^T give, per lane, four
// queries of key fr; P mask and dS become the B operands of dV^T += dO^T (P mask) and dK^T += Q^T dS.  Queries in tile order: fixed sums.
__global__ void __launch_bounds__(64 * MW) bert_body_attn_bwd_kv_mfma_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k,
                                                                             const float* __restrict__ v, int ldkv,
                                                                             const float* __restrict__ dout, const float* __restrict__ dsum,
                                                                             const float* __restrict__ lse, int S, int H, int q_from,
                                                                             int k_from, float scale, DropCfg drop, uint64_t site,
                                                                             float* __restrict__ dk, float* __restrict__ dv, int dkv_rows,
                                                                             int ldd) {
    __shared__ __attribute__((aligned(16))) bf16_t Qs[KT * RM_LD];
    __shared__ __attribute__((aligned(16))) bf16_t Gs[KT * RM_LD];
    __shared__ __attribute__((aligned(16))) bf16_t Qt[HD * TR_LD];
    __shared__ __attribute__((aligned(16))) bf16_t Gt[HD * TR_LD];
    __shared__ float Ls[KT], Ds[KT];
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, g = lane >> 4;
    const int b = blockIdx.x, h = blockIdx.y;
    const int u0 = (k_from / MQ + ((int)blockIdx.z * MW + (tid >> 6))) * MQ;
    const bool active = u0 < S;
    const int Sq = S - q_from, dq = H * HD;
    const float* qb = q + (size_t)b * Sq * ldq + h * HD;
    const float* gb = dout + (size_t)b * Sq * dq + h * HD;
    bf16x8 kf[2][2], vf[2][2];
    int kpos[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int pn = u0 + 16 * mt + fr;
        kpos[mt] = pn < k_from ? k_from : pn >= S ? S - 1 : pn;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            kf[mt][ks] = row_frag(k + ((size_t)b * S + kpos[mt]) * ldkv + h * HD, ks, g);
            vf[mt][ks] = row_frag(v + ((size_t)b * S + kpos[mt]) * ldkv + h * HD, ks, g);
        }
    }
    f32x4 AK[2][4], AV[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int et = 0; et < 4; ++et) { AK[mt][et] = f32x4{0.f, 0.f, 0.f, 0.f}; AV[mt][et] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int tq0 = 0; tq0 < Sq; tq0 += KT) {
        __syncthreads();
        stage_tile(qb, ldq, tq0, Sq, tid, Qs, Qt);
        stage_tile(gb, dq, tq0, Sq, tid, Gs, Gt);
        if (tid < KT) {
            const int t = tq0 + tid;
            Ls[tid] = t < Sq ? lse[((size_t)b * H + h) * Sq + t] : 0.f;
            Ds[tid] = t < Sq ? dsum[((size_t)b * Sq + t) * H + h] : 0.f;
        }
        __syncthreads();
        if (!active) continue;
        bf16x8 qf[2][2], gf[2][2], qtf[4], gtf[4];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                qf[nt][ks] = rm_frag(Qs, nt, ks, fr, g);
                gf[nt][ks] = rm_frag(Gs, nt, ks, fr, g);
            }
#pragma unroll
        for (int et = 0; et < 4; ++et) {
            qtf[et] = tr_frag(Qt, et, fr, g);
            gtf[et] = tr_frag(Gt, et, fr, g);
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            float pm[2][4], sd[2][4];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                f32x4 Sc = {0.f, 0.f, 0.f, 0.f}, dA = Sc;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    Sc = bb_mfma(qf[nt][ks], kf[mt][ks], Sc);
                    dA = bb_mfma(gf[nt][ks], vf[mt][ks], dA);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int tt = 16 * nt + 4 * g + i, t = tq0 + tt;
                    const float p = t < Sq ? __expf(Sc[i] * scale - Ls[tt]) : 0.f;
                    const float dsc = dropout_scale(drop, site, (((size_t)b * H + h) * S + q_from + (t < Sq ? t : Sq - 1)) * ATT_STRIDE +
                                                                    (size_t)kpos[mt]);
                    pm[nt][i] = p * dsc;
                    sd[nt][i] = p * (dsc * dA[i] - Ds[tt]) * scale;
                }
            }
            const bf16x8 pf = bf16x8{(bf16_t)pm[0][0], (bf16_t)pm[0][1], (bf16_t)pm[0][2], (bf16_t)pm[0][3],
                                     (bf16_t)pm[1][0], (bf16_t)pm[1][1], (bf16_t)pm[1][2], (bf16_t)pm[1][3]};
            const bf16x8 sf = bf16x8{(bf16_t)sd[0][0], (bf16_t)sd[0][1], (bf16_t)sd[0][2], (bf16_t)sd[0][3],
                                     (bf16_t)sd[1][0], (bf16_t)sd[1][1], (bf16_t)sd[1][2], (bf16_t)sd[1][3]};
#pragma unroll
            for (int et = 0; et < 4; ++et) {
                AV[mt][et] = bb_mfma(gtf[et], pf, AV[mt][et]);
                AK[mt][et] = bb_mfma(qtf[et], sf, AK[mt][et]);
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int pn = u0 + 16 * mt + fr;
        if (pn < k_from || pn >= S) continue;
        const size_t row = ((size_t)b * dkv_rows + (pn - k_from)) * ldd + h * HD + 4 * g;
#pragma unroll
        for (int et = 0; et < 4; ++et) {
            const f32x4 a = AK[mt][et], c = AV[mt][et];
            *reinterpret_cast<float4*>(dk + row + 16 * et) = float4{a[0], a[1], a[2], a[3]};
            *reinterpret_cast<float4*>(dv + row + 16 * et) = float4{c[0], c[1], c[2], c[3]};
        }
    }
}

inline unsigned mfma_blocks(int S, int from) { return (unsigned)(((S + MQ - 1) / MQ - from / MQ + MW - 1) / MW); }

int attn_args_ok(const float* q, int32_t ldq, const float* k, const float* v, int32_t ldkv, int32_t B, int32_t S, int32_t H, int32_t q_from,
                 int32_t precision) {
    if (!q || !k || !v || B <= 0 || H <= 0 || S <= 0 || q_from < 0 || q_from >= S || precision < 0 || precision > 1) return IMMTSF_EINVAL;
    if (S > ATT_STRIDE || B > 65535 || H > 65535) return IMMTSF_EUNSUPPORTED;
    if (ldq < H * HD || ldkv < H * HD || (ldq & 3) || (ldkv & 3) || !al16(q) || !al16(k) || !al16(v)) return IMMTSF_EUNSUPPORTED;
    return IMMTSF_OK;
}

}  // namespace

extern "C" {

int immtsf_bert_body_supported(int32_t d, int32_t H, int32_t S, int32_t max_positions) {
    return d > 0 && H > 0 && H <= 65535 && d == H * HD && S >= 1 && S <= max_positions && S <= ATT_STRIDE;
}

int immtsf_bert_body_embed(const float* prefix, const float* tail, const float* pos, const float* type0, int32_t B, int32_t S_p, int32_t S_t,
                           int32_t d, const float* gamma, const float* beta, float eps, float p_drop, uint64_t seed, uint64_t site,
                           float* out32, void* out16, float* sum_tail, float* mean_tail, float* rstd_tail, immtsf_stream_t stream) {
    if (!tail || !pos || !type0 || !gamma || !beta || !out32 || B <= 0 || S_p < 0 || S_t <= 0 || d <= 0 || (S_p > 0 && !prefix))
        return IMMTSF_EINVAL;
    if ((d & 3) || !al16(tail) || !al16(pos) || !al16(type0) || !al16(gamma) || !al16(beta) || !al16(out32) || (prefix && !al16(prefix)) ||
        (out16 && !al8(out16)) || (sum_tail && !al16(sum_tail)))
        return IMMTSF_EUNSUPPORTED;
    const long rows = (long)B * (S_p + S_t);
    if (rows > 0x7fffffffL) return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(bert_body_embed_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), prefix, tail, pos,
                       type0, B, S_p, S_t, d, gamma, beta, eps, mk_drop(p_drop, seed), site, out32, static_cast<bf16_t*>(out16), sum_tail,
                       mean_tail, rstd_tail);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_bert_body_add_layernorm(const float* xin, int32_t B, int32_t S_in, int32_t s_from, const float* y, int32_t S, int32_t q_from,
                                   int32_t d, const float* gamma, const float* beta, float eps, float p_drop, uint64_t seed, uint64_t site,
                                   float* out32, void* out16, float* sum, float* mean, float* rstd, immtsf_stream_t stream) {
    if (!xin || !y || !gamma || !beta || (!out32 && !out16) || B <= 0 || d <= 0 || s_from < 0 || s_from >= S_in || q_from < 0) return IMMTSF_EINVAL;
    const int Sn = S_in - s_from;
    if (q_from + Sn > S) return IMMTSF_EINVAL;
    if (!out32 && !sum) return IMMTSF_EUNSUPPORTED;      // the pre-norm row is staged in one of the two
    if ((d & 3) || !al16(xin) || !al16(y) || !al16(gamma) || !al16(beta) || (out32 && !al16(out32)) || (out16 && !al8(out16)) ||
        (sum && !al16(sum)))
        return IMMTSF_EUNSUPPORTED;
    const long rows = (long)B * Sn;
    if (rows > 0x7fffffffL) return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(bert_body_add_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), xin, S_in, s_from,
                       Sn, y, S, q_from, d, gamma, beta, eps, mk_drop(p_drop, seed), site, rows, out32, static_cast<bf16_t*>(out16), sum, mean,
                       rstd);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_bert_body_layernorm_backward(const float* dy_a, int32_t B, int32_t Sa, int32_t sa_from, int32_t Sn, const float* dy_b,
                                        int32_t tb_from, const float* sum, const float* mean, const float* rstd, const float* gamma, int32_t d,
                                        int32_t S, int32_t q_from, float p_drop, uint64_t seed, uint64_t site, int32_t drop_first, float* dx32,
                                        float* dbr32, void* dbr16, immtsf_stream_t stream) {
    if (!dy_a || !sum || !mean || !rstd || !gamma || (!dx32 && !dbr32 && !dbr16) || B <= 0 || d <= 0 || Sn <= 0 || sa_from < 0 ||
        sa_from + Sn > Sa || q_from < 0 || q_from + Sn > S || (dy_b && (tb_from < 0 || tb_from >= Sn)))
        return IMMTSF_EINVAL;
    if (drop_first && (dbr32 || dbr16)) return IMMTSF_EINVAL;
    if ((d & 3) || !al16(dy_a) || (dy_b && !al16(dy_b)) || !al16(sum) || !al16(gamma) || (dx32 && !al16(dx32)) || (dbr32 && !al16(dbr32)) ||
        (dbr16 && !al8(dbr16)))
        return IMMTSF_EUNSUPPORTED;
    const long rows = (long)B * Sn;
    if (rows > 0x7fffffffL) return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(bert_body_ln_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), dy_a, Sa, sa_from,
                       Sn, dy_b, tb_from, sum, mean, rstd, gamma, d, S, q_from, mk_drop(p_drop, seed), site, drop_first ? 1 : 0, rows, dx32,
                       dbr32, static_cast<bf16_t*>(dbr16));
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_bert_body_gelu_backward(const float* pre, const float* dact, uint64_t n, float* dpre32, void* dpre16, immtsf_stream_t stream) {
    if (!pre || !dact || (!dpre32 && !dpre16) || n == 0) return IMMTSF_EINVAL;
    if ((n & 3) || !al16(pre) || !al16(dact) || (dpre32 && !al16(dpre32)) || (dpre16 && !al8(dpre16))) return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(bert_body_gelu_bwd_kernel, dim3(grid_for(n / 4, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pre, dact,
                       (size_t)(n / 4), dpre32, static_cast<bf16_t*>(dpre16));
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_bert_body_attention_forward(const float* q, int32_t ldq, const float* k, const float* v, int32_t ldkv, int32_t B, int32_t S,
                                       int32_t H, int32_t q_from, float scale, int32_t precision, float p_drop, uint64_t seed, uint64_t site,
                                       float* out32, void* out16, float* lse, immtsf_stream_t stream) {
    if (int rc = attn_args_ok(q, ldq, k, v, ldkv, B, S, H, q_from, precision)) return rc;
    if (!out32 && !out16) return IMMTSF_EINVAL;
    if ((out32 && !al16(out32)) || (out16 && !al8(out16))) return IMMTSF_EUNSUPPORTED;
    const int Sq = S - q_from;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const DropCfg drop = mk_drop(p_drop, seed);
    if (precision == 1)
        hipLaunchKernelGGL(bert_body_attn_mfma_kernel, dim3((unsigned)B, (unsigned)H, mfma_blocks(S, q_from)), dim3(64 * MW), 0, s, q, ldq, k, v,
                           ldkv, S, H, q_from, scale, drop, site, out32, static_cast<bf16_t*>(out16), lse);
    else
        hipLaunchKernelGGL(dense64::attn_fwd_kernel<false>, dim3((Sq + 63) / 64, H, B), dim3(64), 0, s, q, ldq, k, v, ldkv, S, H, q_from, scale, drop,
                           site, out32, static_cast<bf16_t*>(out16), lse);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_bert_body_attention_backward(const float* q, int32_t ldq, const float* k, const float* v, int32_t ldkv, const float* dout,
                                        const float* out, const float* lse, int32_t B, int32_t S, int32_t H, int32_t q_from, int32_t dq_from,
                                        int32_t k_from, float scale, int32_t precision, float p_drop, uint64_t seed, uint64_t site, float* dq,
                                        int32_t dq_rows, float* dk, float* dv, int32_t dkv_rows, int32_t ldd, float* dsum,
                                        immtsf_stream_t stream) {
    if (int rc = attn_args_ok(q, ldq, k, v, ldkv, B, S, H, q_from, precision)) return rc;
    if (!dout || !out || !lse || !dq || !dk || !dv || dq_from < q_from || dq_from >= S || k_from < 0 || k_from >= S) return IMMTSF_EINVAL;
    if (dq_rows < S - dq_from || dkv_rows < S - k_from || (precision == 1 && !dsum)) return IMMTSF_EINVAL;
    if (ldd < H * HD || (ldd & 3) || !al16(dout) || !al16(out) || !al16(dq) || !al16(dk) || !al16(dv)) return IMMTSF_EUNSUPPORTED;
    const int Sq = S - q_from, Sd = S - dq_from, Sk = S - k_from;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const DropCfg drop = mk_drop(p_drop, seed);
    if (precision == 1) {
        const long n = (long)B * Sq * H;
        hipLaunchKernelGGL(bert_body_attn_dsum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dout, out, n, H, dsum);
        IMMTSF_LAUNCH_CHECK();
        hipLaunchKernelGGL(bert_body_attn_bwd_q_mfma_kernel, dim3((unsigned)B, (unsigned)H, mfma_blocks(S, dq_from)), dim3(64 * MW), 0, s, q, ldq,
                           k, v, ldkv, dout, dsum, lse, S, H, q_from, dq_from, scale, drop, site, dq, dq_rows, ldd);
        IMMTSF_LAUNCH_CHECK();
        hipLaunchKernelGGL(bert_body_attn_bwd_kv_mfma_kernel, dim3((unsigned)B, (unsigned)H, mfma_blocks(S, k_from)), dim3(64 * MW), 0, s, q, ldq,
                           k, v, ldkv, dout, dsum, lse, S, H, q_from, k_from, scale, drop, site, dk, dv, dkv_rows, ldd);
        IMMTSF_LAUNCH_CHECK();
        return IMMTSF_OK;
    }
    hipLaunchKernelGGL(dense64::attn_bwd_q_kernel<false>, dim3((Sd + 63) / 64, H, B), dim3(64), 0, s, q, ldq, k, v, ldkv, dout, out, lse, S, H, q_from,
                       dq_from, scale, drop, site, dq, dq_rows, ldd);
    IMMTSF_LAUNCH_CHECK();
    hipLaunchKernelGGL(dense64::attn_bwd_kv_kernel<false>, dim3((Sk + 63) / 64, H, B), dim3(64), 0, s, q, ldq, k, v, ldkv, dout, out, lse, S, H, q_from,
                       k_from, scale, drop, site, dk, dv, dkv_rows, ldd);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
