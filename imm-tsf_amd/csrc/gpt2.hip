// TimeLLM's frozen GPT-2 body (reference models/TimeLLM.py:256: llm_model(inputs_embeds=cat([prompt, patches]))): the pieces the GEMM
// family does not have.  Rows are (b, s) with s < S = S_p + S_t; the last S_t rows (the reprogrammed patches) are the only ones a
// gradient flows to, and attention is causal without a padding mask, so no prefix row ever depends on a tail row: the backward runs
// over the tail rows alone (dQ of the tail queries against all keys, dK / dV of the tail keys from the tail queries), and it is exact.
//   * causal attention forward over (b, head) with a query offset q_from (the last layer computes the tail queries only), Q / K / V read
//     in the projections' layout (row pitch, head h at columns 64 h), online softmax in fp32, output in the layout c_proj reads + the
//     per-row log-sum-exp; attention dropout drawn from Philox (index ((b H + h) S + i) 1024 + j: four keys per call at any S <= 1024)
//   * its backward for the tail queries: probabilities recomputed from the log-sum-exp, the same mask redrawn; one writer per output
//     element, sums in key / query order, no atomics
//   * row kernels: wpe add + embedding dropout over [prefix | tail] without the concatenated copy, LayerNorm that writes the GEMM operand
//     (fp32 or bf16) and the statistics, residual + dropout, gelu_new (tanh form) and their backward forms over compact tail rows
// The products go through the GEMM family (immtsf_gpt2_gemm: its launcher with split-K off, so that every sum has one order).
// head_dim is 64; the arithmetic is fp32 on the VALU in either precision mode (bf16 mode differs in the GEMM operands only).
// The three attention kernels are the CAUSAL instances of attn_dense64.hpp, which the BERT body shares.
#include "../../include/immtsf.h"
#include "attn_dense64.hpp"
#include "block_util.hpp"
#include "common.hpp"

namespace {

using dense64::HD;

__device__ __forceinline__ float gelu_new_f(float x) {
    const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
    return 0.5f * x * (1.f + tanhf(u));
}
__device__ __forceinline__ float gelu_new_grad(float x) {
    const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
    const float t = tanhf(u);
    return 0.5f * (1.f + t) + 0.5f * x * (1.f - t * t) * 0.7978845608028654f * (1.f + 3.f * 0.044715f * x * x);
}

// ---- x[b, s, :] = drop([prefix | tail][b, s, :] + wpe[s, :]) -----------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gpt2_embed_kernel(const float* __restrict__ prefix, const float* __restrict__ tail,
                                                         const float* __restrict__ wpe, int B, int S_p, int S_t, int d, DropCfg drop,
                                                         uint64_t site, float* __restrict__ out) {
    const int S = S_p + S_t, d4 = d >> 2;
    const size_t n4 = (size_t)B * S * d4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const int e4 = (int)(i % d4);
        const size_t row = i / d4;
        const int s = (int)(row % S), b = (int)(row / S);
        const float4 v = s < S_p ? reinterpret_cast<const float4*>(prefix + ((size_t)b * S_p + s) * d)[e4]
                                 : reinterpret_cast<const float4*>(tail + ((size_t)b * S_t + (s - S_p)) * d)[e4];
        const float4 w = reinterpret_cast<const float4*>(wpe + (size_t)s * d)[e4];
        float sc[4];
        dropout_scale4(drop, site, row * d + 4 * (size_t)e4, sc);
        float4 o;
        o.x = (v.x + w.x) * sc[0]; o.y = (v.y + w.y) * sc[1]; o.z = (v.z + w.z) * sc[2]; o.w = (v.w + w.w) * sc[3];
        reinterpret_cast<float4*>(out + row * d)[e4] = o;
    }
}

// ---- LayerNorm of the rows (b, s_from + t), t < Sn = S_in - s_from, of a (B, S_in, d) tensor; compact outputs, one wave per row --------
__global__ void __launch_bounds__(256) gpt2_ln_kernel(const float* __restrict__ x, int B, int S_in, int s_from, int d,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                      float* __restrict__ y32, bf16_t* __restrict__ y16, float* __restrict__ mean_out,
                                                      float* __restrict__ rstd_out) {
    const int Sn = S_in - s_from, lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (long)B * Sn) return;
    const int b = (int)(r / Sn), t = (int)(r % Sn);
    const float* xr = x + ((size_t)b * S_in + s_from + t) * d;
    float s = 0.f;
    for (int e = lane; e < d; e += 64) s += xr[e];
    const float mean = wave_sum(s) / (float)d;
    float v = 0.f;
    for (int e = lane; e < d; e += 64) { const float c = xr[e] - mean; v += c * c; }
    const float rstd = rsqrtf(wave_sum(v) / (float)d + eps);
    for (int e = lane; e < d; e += 64) {
        const float z = (xr[e] - mean) * rstd * gamma[e] + beta[e];
        if (y32) y32[(size_t)r * d + e] = z;
        if (y16) y16[(size_t)r * d + e] = (bf16_t)z;
    }
    if (lane == 0) {
        if (mean_out) mean_out[r] = mean;
        if (rstd_out) rstd_out[r] = rstd;
    }
}

// dx[r] = resid[r] + rstd (g - mean(g) - xhat mean(g xhat)), g = gamma dy; rows compact, one wave per row
__global__ void __launch_bounds__(256) gpt2_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const float* __restrict__ gamma, const float* __restrict__ resid, long rows, int d,
                                                          float* __restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float mu = mean[r], rs = rstd[r];
    const float* xr = x + (size_t)r * d;
    const float* gr = dy + (size_t)r * d;
    float s1 = 0.f, s2 = 0.f;
    for (int e = lane; e < d; e += 64) {
        const float g = gr[e] * gamma[e], xh = (xr[e] - mu) * rs;
        s1 += g;
        s2 += g * xh;
    }
    s1 = wave_sum(s1) / (float)d;
    s2 = wave_sum(s2) / (float)d;
    for (int e = lane; e < d; e += 64) {
        const float g = gr[e] * gamma[e], xh = (xr[e] - mu) * rs;
        const float v = rs * (g - s1 - xh * s2);
        dx[(size_t)r * d + e] = resid ? resid[(size_t)r * d + e] + v : v;
    }
}

// ---- out[b, t, :] = xin[b, s_off + t, :] + drop(y[b, t, :]), t < Sn; the dropout index is that of row (b, q_from + t) of (B, S, d) -------
__global__ void __launch_bounds__(256) gpt2_residual_kernel(const float* __restrict__ xin, int B, int S_in, int s_off, int Sn, int S,
                                                            int q_from, int d, const float* __restrict__ y, DropCfg drop, uint64_t site,
                                                            float* __restrict__ out) {
    const int d4 = d >> 2;
    const size_t n4 = (size_t)B * Sn * d4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const int e4 = (int)(i % d4);
        const size_t r = i / d4;
        const int t = (int)(r % Sn), b = (int)(r / Sn);
        const float4 yv = reinterpret_cast<const float4*>(y + r * d)[e4];
        float sc[4];
        dropout_scale4(drop, site, ((size_t)b * S + q_from + t) * d + 4 * (size_t)e4, sc);
        float4 o = {yv.x * sc[0], yv.y * sc[1], yv.z * sc[2], yv.w * sc[3]};
        if (xin) {
            const float4 xv = reinterpret_cast<const float4*>(xin + ((size_t)b * S_in + s_off + t) * d)[e4];
            o.x += xv.x; o.y += xv.y; o.z += xv.z; o.w += xv.w;
        }
        reinterpret_cast<float4*>(out + r * d)[e4] = o;
    }
}

__global__ void __launch_bounds__(256) gpt2_gelu_kernel(const float* __restrict__ pre, size_t n4, float* __restrict__ o32,
                                                        bf16_t* __restrict__ o16) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(pre)[i];
        const float4 o = {gelu_new_f(v.x), gelu_new_f(v.y), gelu_new_f(v.z), gelu_new_f(v.w)};
        if (o32) reinterpret_cast<float4*>(o32)[i] = o;
        if (o16) {
            const bf16x4 h = {(bf16_t)o.x, (bf16_t)o.y, (bf16_t)o.z, (bf16_t)o.w};
            reinterpret_cast<bf16x4*>(o16)[i] = h;
        }
    }
}

__global__ void __launch_bounds__(256) gpt2_gelu_bwd_kernel(const float* __restrict__ pre, const float* __restrict__ dact, size_t n4,
                                                            float* __restrict__ dpre) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(pre)[i], g = reinterpret_cast<const float4*>(dact)[i];
        const float4 o = {g.x * gelu_new_grad(v.x), g.y * gelu_new_grad(v.y), g.z * gelu_new_grad(v.z), g.w * gelu_new_grad(v.w)};
        reinterpret_cast<float4*>(dpre)[i] = o;
    }
}

}  // namespace

extern "C" {

int immtsf_gpt2_supported(int32_t d, int32_t H, int32_t S, int32_t n_positions) {
    return d > 0 && H > 0 && d == H * HD && S >= 1 && S <= n_positions && S <= ATT_STRIDE;
}

// C (M, N; pitch ldc) = op(A) op(B) + bias through immtsf_launch_gemm with split-K (fp32 atomics) switched off.  layout 1 (NN): A (M, K),
// B (K, N) -- a Conv1D forward on the weight as stored; layout 0 (NT): A (M, K), B (N, K) -- its data gradient on the same weight.
// precision 1 with both bf16 images given runs the bf16-in-memory kernels; otherwise the fp32 operands are used.
int immtsf_gpt2_gemm(int32_t layout, int32_t precision, const float* A, const void* A16, int32_t lda, const float* B, const void* B16,
                     int32_t ldb, float* C, int32_t ldc, const float* bias, int32_t M, int32_t N, int32_t K, immtsf_stream_t stream) {
    if ((layout != GEMM_NT && layout != GEMM_NN) || (!A && !A16) || (!B && !B16) || !C || M <= 0 || N <= 0 || K <= 0) return IMMTSF_EINVAL;
    if (precision < 0 || precision > 1) return IMMTSF_EINVAL;
    GemmArgs g = gemm_args(M, N, K, lda, ldb, ldc);
    set_problem2(g, 0, cmat(A, A16), cmat(B, B16), mat(C), bias);
    g.no_split = 1;
    return immtsf_launch_gemm(layout, precision, g, static_cast<hipStream_t>(stream));
}

int immtsf_gpt2_embed(const float* prefix, const float* tail, const float* wpe, int32_t B, int32_t S_p, int32_t S_t, int32_t d, float p_drop,
                      uint64_t seed, uint64_t site, float* out, immtsf_stream_t stream) {
    if (!tail || !wpe || !out || B <= 0 || S_p < 0 || S_t <= 0 || d <= 0 || (S_p > 0 && !prefix)) return IMMTSF_EINVAL;
    if ((d & 3) || !al16(tail) || !al16(wpe) || !al16(out) || (prefix && !al16(prefix))) return IMMTSF_EUNSUPPORTED;
    const size_t n4 = (size_t)B * (S_p + S_t) * (d / 4);
    hipLaunchKernelGGL(gpt2_embed_kernel, dim3(grid_for(n4, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), prefix, tail, wpe, B, S_p,
                       S_t, d, mk_drop(p_drop, seed), site, out);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_gpt2_layernorm(const float* x, int32_t B, int32_t S_in, int32_t s_from, int32_t d, const float* gamma, const float* beta, float eps,
                          float* y32, void* y16, float* mean, float* rstd, immtsf_stream_t stream) {
    if (!x || !gamma || !beta || (!y32 && !y16) || B <= 0 || d <= 0 || s_from < 0 || s_from >= S_in) return IMMTSF_EINVAL;
    const long rows = (long)B * (S_in - s_from);
    hipLaunchKernelGGL(gpt2_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), x, B, S_in, s_from, d,
                       gamma, beta, eps, y32, static_cast<bf16_t*>(y16), mean, rstd);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_gpt2_layernorm_backward(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                                   const float* resid, int64_t rows, int32_t d, float* dx, immtsf_stream_t stream) {
    if (!dy || !x || !mean || !rstd || !gamma || !dx || rows <= 0 || d <= 0) return IMMTSF_EINVAL;
    hipLaunchKernelGGL(gpt2_ln_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), dy, x, mean, rstd,
                       gamma, resid, (long)rows, d, dx);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_gpt2_residual(const float* xin, int32_t B, int32_t S_in, int32_t s_off, int32_t Sn, int32_t S, int32_t q_from, int32_t d,
                         const float* y, float p_drop, uint64_t seed, uint64_t site, float* out, immtsf_stream_t stream) {
    if (!y || !out || B <= 0 || Sn <= 0 || d <= 0 || q_from < 0 || q_from + Sn > S) return IMMTSF_EINVAL;
    if (xin && (s_off < 0 || s_off + Sn > S_in)) return IMMTSF_EINVAL;
    if ((d & 3) || !al16(y) || !al16(out) || (xin && !al16(xin))) return IMMTSF_EUNSUPPORTED;
    const size_t n4 = (size_t)B * Sn * (d / 4);
    hipLaunchKernelGGL(gpt2_residual_kernel, dim3(grid_for(n4, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), xin, B, S_in, s_off, Sn,
                       S, q_from, d, y, mk_drop(p_drop, seed), site, out);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_gpt2_gelu(const float* pre, uint64_t n, float* out32, void* out16, immtsf_stream_t stream) {
    if (!pre || (!out32 && !out16) || n == 0) return IMMTSF_EINVAL;
    if ((n & 3) || !al16(pre) || (out32 && !al16(out32)) || (out16 && !al8(out16))) return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(gpt2_gelu_kernel, dim3(grid_for(n / 4, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pre, (size_t)(n / 4), out32,
                       static_cast<bf16_t*>(out16));
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_gpt2_gelu_backward(const float* pre, const float* dact, uint64_t n, float* dpre, immtsf_stream_t stream) {
    if (!pre || !dact || !dpre || n == 0) return IMMTSF_EINVAL;
    if ((n & 3) || !al16(pre) || !al16(dact) || !al16(dpre)) return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(gpt2_gelu_bwd_kernel, dim3(grid_for(n / 4, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pre, dact,
                       (size_t)(n / 4), dpre);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

static int attn_args_ok(const float* q, int32_t ldq, const float* k, const float* v, int32_t ldkv, int32_t B, int32_t S, int32_t H,
                        int32_t q_from) {
    if (!q || !k || !v || B <= 0 || H <= 0 || S <= 0 || q_from < 0 || q_from >= S) return IMMTSF_EINVAL;
    if (S > ATT_STRIDE || B > 65535 || H > 65535) return IMMTSF_EUNSUPPORTED;
    if (ldq < H * HD || ldkv < H * HD || (ldq & 3) || (ldkv & 3) || !al16(q) || !al16(k) || !al16(v)) return IMMTSF_EUNSUPPORTED;
    return IMMTSF_OK;
}

int immtsf_gpt2_attention_forward(const float* q, int32_t ldq, const float* k, const float* v, int32_t ldkv, int32_t B, int32_t S, int32_t H,
                                  int32_t q_from, float scale, float p_drop, uint64_t seed, uint64_t site, float* out32, void* out16,
                                  float* lse, immtsf_stream_t stream) {
    if (int rc = attn_args_ok(q, ldq, k, v, ldkv, B, S, H, q_from)) return rc;
    if (!out32 && !out16) return IMMTSF_EINVAL;
    if ((out32 && !al16(out32)) || (out16 && !al8(out16))) return IMMTSF_EUNSUPPORTED;
    const int Sq = S - q_from;
    hipLaunchKernelGGL(dense64::attn_fwd_kernel<true>, dim3((Sq + 63) / 64, H, B), dim3(64), 0, static_cast<hipStream_t>(stream), q, ldq, k, v,
                       ldkv, S, H, q_from, scale, mk_drop(p_drop, seed), site, out32, static_cast<bf16_t*>(out16), lse);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_gpt2_attention_backward(const float* q, int32_t ldq, const float* k, const float* v, int32_t ldkv, const float* dout,
                                   const float* out, const float* lse, int32_t B, int32_t S, int32_t H, int32_t q_from, float scale,
                                   float p_drop, uint64_t seed, uint64_t site, float* dq, float* dk, float* dv, int32_t ldd,
                                   immtsf_stream_t stream) {
    if (int rc = attn_args_ok(q, ldq, k, v, ldkv, B, S, H, q_from)) return rc;
    if (!dout || !out || !lse || !dq || !dk || !dv) return IMMTSF_EINVAL;
    if (ldd < H * HD || (ldd & 3) || !al16(dout) || !al16(out) || !al16(dq) || !al16(dk) || !al16(dv)) return IMMTSF_EUNSUPPORTED;
    const int Sq = S - q_from;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const DropCfg drop = mk_drop(p_drop, seed);
    // the shared kernels take a sub-range of the forward's queries / keys: here it is the whole tail (dq_from = k_from = q_from)
    hipLaunchKernelGGL(dense64::attn_bwd_q_kernel<true>, dim3((Sq + 63) / 64, H, B), dim3(64), 0, s, q, ldq, k, v, ldkv, dout, out, lse, S, H,
                       q_from, q_from, scale, drop, site, dq, Sq, ldd);
    IMMTSF_LAUNCH_CHECK();
    hipLaunchKernelGGL(dense64::attn_bwd_kv_kernel<true>, dim3((Sq + 63) / 64, H, B), dim3(64), 0, s, q, ldq, k, v, ldkv, dout, out, lse, S, H,
                       q_from, q_from, scale, drop, site, dk, dv, Sq, ldd);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
