// Raw-text mode: a frozen BERT over the RAGGED tokens of a batch of notes, mean-pooled per note (reference fusions/load_llm.py embed_notes).
// BERT is not causal, but a padded key enters every real query's softmax with an additive minimum (its weight is an exact 0) and the
// mean-pool reads real rows only, so each note's real tokens run alone give the padded call's result: the function is computed over the
// sum(L) real tokens, notes back to back (`cu` = N + 1 prefix sums of the token counts, on the device).  The attention is the non-causal
// instance of the ragged kernels of note_embed.hip (immtsf_bert_embed_attention, defined there); the products are immtsf_gpt2_gemm layout
// 0 (an nn.Linear weight as stored) over the packed rows as one sequence.  This file has the row kernels of the post-LN body:
//   * embedding row: LayerNorm(word[ids[r]] + pos[r - cu[n]] + type[0]), one launch, one wave per row
//   * residual + LayerNorm: LayerNorm(y + x), one launch per site
//   * erf GELU (hidden_act "gelu"; the tanh form is gpt2.hip's)
//   * mean-pool without a final LayerNorm: the rows of a note summed in position order, / max(L, 1); no tokens: an exact 0 row
// The row kernels write the fp32 row and, when asked, the bf16 image the next bf16-in-memory product reads.  Statistics are fp32, two
// passes (mean, then the centred squares), as the row kernels of gpt2.hip take them.
// Forward only, no dropout, no atomics, one writer per output element, every sum in a fixed order: two runs give the same bits.
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

constexpr int HD = 64;        // head_dim
constexpr int MAXL = 1024;    // longest note (tokens)

// LayerNorm of the row a wave has just written to y32 (lane l wrote, and alone reads back, elements l, l + 64, ...), in place; the bf16
// image beside it when y16 is given
__device__ __forceinline__ void ln_row_in_place(float* __restrict__ y32, bf16_t* __restrict__ y16, int d, int lane, float sum,
                                                const float* __restrict__ gamma, const float* __restrict__ beta, float eps) {
    const float mean = wave_sum(sum) / (float)d;
    float v = 0.f;
    for (int e = lane; e < d; e += 64) { const float c = y32[e] - mean; v += c * c; }
    const float rstd = rsqrtf(wave_sum(v) / (float)d + eps);
    for (int e = lane; e < d; e += 64) {
        const float z = (y32[e] - mean) * rstd * gamma[e] + beta[e];
        y32[e] = z;
        if (y16) y16[e] = (bf16_t)z;
    }
}

// ---- x[r, :] = LayerNorm(word[ids[r], :] + pos[p, :] + type[0, :]), p = r - cu[n]; one wave per row -------------------------------------
// an id outside the word table or a position outside the position table is not read: the row is written as zeros (the host raises first)
__global__ void __launch_bounds__(256) bert_rows_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ cu, int N, int rows,
                                                        const float* __restrict__ word, int vocab, const float* __restrict__ pos,
                                                        int max_positions, const float* __restrict__ type0, int d,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                        float* __restrict__ x32, bf16_t* __restrict__ x16) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    int lo = 0, hi = N;               // the last n in [0, N) with cu[n] <= r (notes of no tokens share their successor's start)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cu[mid] <= (int)r) lo = mid; else hi = mid;
    }
    const int p = (int)r - cu[lo], id = ids[r];
    float* y32 = x32 + (size_t)r * d;
    bf16_t* y16 = x16 ? x16 + (size_t)r * d : nullptr;
    if (id < 0 || id >= vocab || p < 0 || p >= max_positions) {
        for (int e = lane; e < d; e += 64) {
            y32[e] = 0.f;
            if (y16) y16[e] = (bf16_t)0.f;
        }
        return;
    }
    const float* a = word + (size_t)id * d;
    const float* b = pos + (size_t)p * d;
    float s = 0.f;
    for (int e = lane; e < d; e += 64) {
        const float v = a[e] + b[e] + type0[e];
        y32[e] = v;
        s += v;
    }
    ln_row_in_place(y32, y16, d, lane, s, gamma, beta, eps);
}

// ---- out[r, :] = LayerNorm(y[r, :] + x[r, :]); one wave per row; out32 may be x ----------------------------------------------------------
__global__ void __launch_bounds__(256) bert_add_ln_kernel(const float* __restrict__ y, const float* x, long rows, int d,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                          float* out32, bf16_t* __restrict__ out16) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* yr = y + (size_t)r * d;
    const float* xr = x + (size_t)r * d;
    float* o32 = out32 + (size_t)r * d;
    float s = 0.f;
    for (int e = lane; e < d; e += 64) {
        const float v = yr[e] + xr[e];
        o32[e] = v;
        s += v;
    }
    ln_row_in_place(o32, out16 ? out16 + (size_t)r * d : nullptr, d, lane, s, gamma, beta, eps);
}

// ---- gelu(x) = x Phi(x), the erf form ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_erf_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }

__global__ void __launch_bounds__(256) bert_gelu_kernel(const float* __restrict__ pre, size_t n4, float* __restrict__ o32,
                                                        bf16_t* __restrict__ o16) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(pre)[i];
        const float4 o = {gelu_erf_f(v.x), gelu_erf_f(v.y), gelu_erf_f(v.z), gelu_erf_f(v.w)};
        if (o32) reinterpret_cast<float4*>(o32)[i] = o;
        if (o16) {
            const bf16x4 h = {(bf16_t)o.x, (bf16_t)o.y, (bf16_t)o.z, (bf16_t)o.w};
            reinterpret_cast<bf16x4*>(o16)[i] = h;
        }
    }
}

// ---- pooled[n, :] = sum over the rows of note n, in position order, / max(L, 1) ---------------------------------------------------------
// grid (note, 256-column slice): a thread owns one output column and walks the note's rows (coalesced across the workgroup).  A range
// that does not lie inside [0, rows) or is longer than MAXL counts as empty, as in note_embed.hip.
__global__ void __launch_bounds__(256) bert_pool_kernel(const float* __restrict__ x, const int32_t* __restrict__ cu, int rows, int d,
                                                        float* __restrict__ pooled) {
    const int n = blockIdx.x, e = blockIdx.y * 256 + threadIdx.x;
    if (e >= d) return;
    const int a = cu[n], b = cu[n + 1];
    int L = b - a;
    if (a < 0 || b < a || b > rows || L > MAXL) L = 0;
    const float* xb = x + (size_t)a * d + e;
    float acc = 0.f;
    for (int p = 0; p < L; ++p) acc += xb[(size_t)p * d];
    pooled[(size_t)n * d + e] = acc / (float)(L > 1 ? L : 1);
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int immtsf_bert_embed_supported(int32_t d, int32_t H, int32_t max_len, int32_t max_positions) {
    return d > 0 && H > 0 && H <= 65535 && d == H * HD && max_len >= 1 && max_len <= max_positions && max_len <= MAXL;
}

// the activations of one pass over `rows` packed tokens, each buffer rounded up to 256 bytes, in this order: x, x1 (rows, d) fp32; h
// (rows, d) bf16, precision 1 only (the image of x or x1 the next product reads); qkv (rows, 3 d) fp32; ao (rows, d) fp32 | bf16; proj
// (rows, d) fp32; pre (rows, inner) fp32; act (rows, inner) fp32 | bf16  (bf16 in precision 1)
size_t immtsf_bert_embed_workspace_bytes(int64_t rows, int32_t d, int32_t inner, int32_t precision) {
    if (rows <= 0 || d <= 0 || inner <= 0) return 0;
    const size_t r = (size_t)rows, op = precision == 1 ? 2 : 4;
    return 2 * up256(r * d * 4) + (precision == 1 ? up256(r * d * 2) : 0) + up256(r * 3 * d * 4) + up256(r * d * op) + up256(r * d * 4) +
           up256(r * inner * 4) + up256(r * inner * op);
}

int immtsf_bert_embed_rows(const int32_t* ids, const int32_t* cu, int32_t N, int32_t rows, const float* word, int32_t vocab, const float* pos,
                           int32_t max_positions, const float* type0, int32_t d, const float* gamma, const float* beta, float eps,
                           float* out32, void* out16, immtsf_stream_t stream) {
    if (!ids || !cu || !word || !pos || !type0 || !gamma || !beta || !out32 || N <= 0 || rows <= 0 || vocab <= 0 || max_positions <= 0 || d <= 0)
        return IMMTSF_EINVAL;
    hipLaunchKernelGGL(bert_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), ids, cu, N, rows, word,
                       vocab, pos, max_positions, type0, d, gamma, beta, eps, out32, static_cast<bf16_t*>(out16));
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_bert_embed_add_layernorm(const float* y, const float* x, int64_t rows, int32_t d, const float* gamma, const float* beta, float eps,
                                    float* out32, void* out16, immtsf_stream_t stream) {
    if (!y || !x || !gamma || !beta || !out32 || rows <= 0 || d <= 0) return IMMTSF_EINVAL;
    if (rows > 0x7fffffffLL) return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(bert_add_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), y, x, (long)rows, d,
                       gamma, beta, eps, out32, static_cast<bf16_t*>(out16));
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_bert_embed_gelu(const float* pre, uint64_t n, float* out32, void* out16, immtsf_stream_t stream) {
    if (!pre || (!out32 && !out16) || n == 0) return IMMTSF_EINVAL;
    if ((n & 3) || !al16(pre) || (out32 && !al16(out32)) || (out16 && !al8(out16))) return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(bert_gelu_kernel, dim3(grid_for(n / 4, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pre, (size_t)(n / 4), out32,
                       static_cast<bf16_t*>(out16));
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_bert_embed_pool(const float* x, const int32_t* cu, int32_t N, int32_t rows, int32_t d, float* pooled, immtsf_stream_t stream) {
    if (!cu || !pooled || N <= 0 || rows < 0 || d <= 0 || (rows > 0 && !x)) return IMMTSF_EINVAL;
    if ((d + 255) / 256 > 65535) return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(bert_pool_kernel, dim3((unsigned)N, (unsigned)((d + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, cu,
                       rows, d, pooled);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
