// Raw-text mode: a frozen Llama (transformers LlamaModel: Llama-3.1, deepseek-llm) over the RAGGED tokens of a batch of notes, mean-pooled
// per note (reference fusions/load_llm.py embed_notes).  The model is causal, its positions are arange(seq) whatever the attention mask is,
// and its tokenizers pad on the right here, so a real token's hidden state never depends on a pad token and the pool never reads a pad
// row: the function is computed over the sum(L) real tokens, notes back to back (`cu` = N + 1 prefix sums of the token counts, on the
// device).  The products are immtsf_gpt2_gemm layout 0 (an nn.Linear weight as stored, no bias) over the packed rows as one sequence.
// This file has the rest of the pre-norm body:
//   * token gather: x[r] = embed_tokens[ids[r]] (no position table: positions enter through RoPE)
//   * RMSNorm rows, x rsqrt(mean(x^2) + eps) w with fp32 statistics, alone or behind the residual add x <- x + y (one launch per site);
//     the row is written as fp32 or as the bf16 operand of the next bf16-in-memory product
//   * RoPE: a cos / sin table (max_len, 64) built per call from the model's own inv_freq and attention_scaling (angle = float(p) inv_freq[i]
//     as ONE fp32 product, precise cosf / sinf: angles reach ~1000 rad), and a row kernel that rotates the Q and K columns of the QKV
//     buffer in place with transformers' rotate_half pairing (i, i + 64); V is left alone
//   * causal attention over ragged sequences, head_dim 128, grouped K/V heads: Q / K / V read in the concatenated q_proj | k_proj | v_proj
//     layout (row pitch (H + 2 H_kv) 128), output in the layout o_proj reads.  fp32 mode on the VALU, bf16 mode with both products on
//     bf16 MFMA and fp32 online softmax: the kernels of attn_gqa128.hpp (which llama_body.hip shares) over the rows of a note
//   * SwiGLU: silu(gate) up over the output of one product on gate_proj | up_proj
//   * final RMSNorm + mean-pool; a note of no tokens gives an exact 0 row
// Forward only, no dropout, no atomics, one writer per output element, every sum in a fixed order: two runs give the same bits.
#include "../../include/immtsf.h"
#include "attn_gqa128.hpp"
#include "common.hpp"

namespace {

using gqa128::HD;             // head_dim 128
using gqa128::QT;             // 32 queries per wave
constexpr int HP = HD / 2;    // rotary pairs of a head
constexpr int MAXL = 1024;    // longest note (tokens)

struct NoteRange { int r0, L; };
// rows of note n; a range that does not lie inside [0, rows) counts as empty
__device__ __forceinline__ NoteRange note_range(const int32_t* __restrict__ cu, int n, int rows) {
    const int a = cu[n], b = cu[n + 1];
    NoteRange r = {a, b - a};
    if (a < 0 || b < a || b > rows || r.L > MAXL) r.L = 0;
    return r;
}

// where the attention kernels of attn_gqa128.hpp find note blockIdx.x: its L rows of the fused q | k | v buffer (pitch ld), queries from
// position 0, no log-sum-exp.  grid (note, K/V head, query tile of the longest note REVERSED): a tile past the note's end is empty.
struct RaggedRows {
    const float* qkv;
    int ld;
    const int32_t* cu;
    int rows, Hkv;
    struct Tile {
        const float *q, *k, *v;
        int ldq, ldkv, t0, S;
        size_t row0;
        bool empty;
        static constexpr int from = 0;
        static constexpr float* lse = nullptr;
    };
    __device__ __forceinline__ Tile tile(int H) const {
        const NoteRange nr = note_range(cu, blockIdx.x, rows);
        const int t0 = ((int)gridDim.z - 1 - (int)blockIdx.z) * QT;
        const float* kb = qkv + (size_t)nr.r0 * ld + (H + (int)blockIdx.y) * HD;
        return Tile{qkv, kb, kb + Hkv * HD, ld, ld, t0, nr.L, (size_t)nr.r0, t0 >= nr.L};
    }
};

// ---- x[r, :] = embed[ids[r], :], one wave per row; an id outside the table is clamped into it (the host raises first) --------------------
// PT: the table's element type (float, or bf16_t for a model stored in bf16: the row is up-cast, exactly)
template <typename PT>
__global__ void __launch_bounds__(256) llama_tokens_kernel(const int32_t* __restrict__ ids, int rows, const PT* __restrict__ embed, int vocab,
                                                           int d, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    int id = ids[r];
    id = id < 0 ? 0 : id >= vocab ? vocab - 1 : id;
    const PT* a = embed + (size_t)id * d;
    float4* o = reinterpret_cast<float4*>(out + (size_t)r * d);
    for (int e = lane; e < (d >> 2); e += 64) o[e] = param4(a, e);
}

// ---- RMSNorm rows, one wave per row -------------------------------------------------------------------------------------------------------
// y given: x[r] <- x[r] + y[r] first (the residual add of the product before).  Then, each when its pointer is given: out32 / out16[r] =
// x[r] rsqrt(mean(x[r]^2) + eps) w, and rstd[r] = that rsqrt alone (what the pool reads).  Lane l writes, and alone reads back, its own
// elements of x.  PT: the type of the weight w (float | bf16_t).
template <typename PT>
__global__ void __launch_bounds__(256) llama_rms_rows_kernel(float* x, const float* __restrict__ y, long rows, int d, const PT* __restrict__ w,
                                                             float eps, float* __restrict__ out32, bf16_t* __restrict__ out16,
                                                             float* __restrict__ rstd_out) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    float4* xr = reinterpret_cast<float4*>(x + (size_t)r * d);
    const int d4 = d >> 2;
    float ss = 0.f;
    if (y) {
        const float4* yr = reinterpret_cast<const float4*>(y + (size_t)r * d);
        for (int e = lane; e < d4; e += 64) {
            const float4 a = xr[e], b = yr[e];
            const float4 v = {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
            xr[e] = v;
            ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
    } else {
        for (int e = lane; e < d4; e += 64) {
            const float4 v = xr[e];
            ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
    }
    const float rstd = rsqrtf(wave_sum(ss) / (float)d + eps);
    if (rstd_out && lane == 0) rstd_out[r] = rstd;
    if (!out32 && !out16) return;
    for (int e = lane; e < d4; e += 64) {
        const float4 v = xr[e], g = param4(w, e);
        const float4 z = {v.x * rstd * g.x, v.y * rstd * g.y, v.z * rstd * g.z, v.w * rstd * g.w};
        if (out32) reinterpret_cast<float4*>(out32 + (size_t)r * d)[e] = z;
        if (out16) reinterpret_cast<bf16x4*>(out16 + (size_t)r * d)[e] = bf16x4{(bf16_t)z.x, (bf16_t)z.y, (bf16_t)z.z, (bf16_t)z.w};
    }
}

// ---- cos / sin table (max_len, 64): angle = float(p) * inv_freq[i], one fp32 product, as transformers' LlamaRotaryEmbedding forms it --------
__global__ void __launch_bounds__(256) llama_rope_table_kernel(const float* __restrict__ inv_freq, float scaling, int max_len,
                                                               float* __restrict__ cos_t, float* __restrict__ sin_t) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= max_len * HP) return;
    const float angle = mul_rounded((float)(idx / HP), inv_freq[idx % HP]);
    cos_t[idx] = cosf(angle) * scaling;
    sin_t[idx] = sinf(angle) * scaling;
}

// ---- RoPE in place on the Q and K columns of qkv, one wave per row: lane i owns the pair (i, i + 64) of every head ------------------------
// the row's position is r - cu[n]; n by bisection as in note_embed.hip, the position clamped into the table
__global__ void __launch_bounds__(256) llama_rope_kernel(float* __restrict__ qkv, int ld, const int32_t* __restrict__ cu, int N, int rows,
                                                         int heads, int max_len, const float* __restrict__ cos_t,
                                                         const float* __restrict__ sin_t) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    int lo = 0, hi = N;               // the last n in [0, N) with cu[n] <= r (notes of no tokens share their successor's start)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cu[mid] <= (int)r) lo = mid; else hi = mid;
    }
    int p = (int)r - cu[lo];
    p = p < 0 ? 0 : p >= max_len ? max_len - 1 : p;
    const float c = cos_t[p * HP + lane], s = sin_t[p * HP + lane];
    float* row = qkv + (size_t)r * ld;
    for (int hh = 0; hh < heads; ++hh) {          // the H query heads, then the H_kv key heads: they are adjacent in the row
        float* b = row + hh * HD;
        const float x1 = b[lane], x2 = b[lane + HP];
        b[lane] = x1 * c - x2 * s;
        b[lane + HP] = x2 * c + x1 * s;
    }
}


// ---- act[r, c] = silu(gu[r, c]) gu[r, inner + c]: gu (rows, 2 inner) is the product on gate_proj | up_proj -------------------------------
__device__ __forceinline__ float silu_f(float x) { return x / (1.f + expf(-x)); }

__global__ void __launch_bounds__(256) llama_swiglu_kernel(const float* __restrict__ gu, size_t n4, int inner4, float* __restrict__ o32,
                                                           bf16_t* __restrict__ o16) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / (size_t)inner4, c = i - r * (size_t)inner4;
        const float4 a = reinterpret_cast<const float4*>(gu)[r * 2 * inner4 + c];
        const float4 b = reinterpret_cast<const float4*>(gu)[r * 2 * inner4 + inner4 + c];
        const float4 o = {silu_f(a.x) * b.x, silu_f(a.y) * b.y, silu_f(a.z) * b.z, silu_f(a.w) * b.w};
        if (o32) reinterpret_cast<float4*>(o32)[i] = o;
        if (o16) reinterpret_cast<bf16x4*>(o16)[i] = bf16x4{(bf16_t)o.x, (bf16_t)o.y, (bf16_t)o.z, (bf16_t)o.w};
    }
}

// ---- pooled[n, e] = w[e] sum over the rows of note n, in position order, of x[row, e] rstd[row], / max(L, 1) -------------------------------
// grid (note, 256-column slice): a thread owns one output column and walks the note's rows (coalesced across the workgroup); rstd comes
// from llama_rms_rows_kernel.  A range that does not lie inside [0, rows) or is longer than MAXL counts as empty.
template <typename PT>
__global__ void __launch_bounds__(256) llama_pool_kernel(const float* __restrict__ x, const float* __restrict__ rstd,
                                                         const int32_t* __restrict__ cu, int rows, int d, const PT* __restrict__ w,
                                                         float* __restrict__ pooled) {
    const int n = blockIdx.x, e = blockIdx.y * 256 + threadIdx.x;
    if (e >= d) return;
    const NoteRange nr = note_range(cu, n, rows);
    const float* xb = x + (size_t)nr.r0 * d + e;
    float acc = 0.f;
    for (int p = 0; p < nr.L; ++p) acc += xb[(size_t)p * d] * rstd[nr.r0 + p];
    pooled[(size_t)n * d + e] = acc * (float)w[e] / (float)(nr.L > 1 ? nr.L : 1);
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
inline bool group_ok(int H, int Hkv) {
    if (H <= 0 || Hkv <= 0 || H % Hkv) return false;
    const int G = H / Hkv;
    return G == 1 || G == 2 || G == 4 || G == 8;
}

// a parameter pointer is aligned for the four-element loads of its type
inline bool param_al(const float* p) { return al16(p); }
inline bool param_al(const bf16_t* p) { return al8(p); }

template <typename PT>
int launch_rms_rows(float* x, const float* y, int64_t rows, int32_t d, const PT* w, float eps, float* out32, void* out16, float* rstd,
                    immtsf_stream_t stream) {
    if (!x || !w || rows <= 0 || d <= 0 || (!out32 && !out16 && !rstd)) return IMMTSF_EINVAL;
    if (rows > 0x7fffffffLL || (d & 3) || !al16(x) || !param_al(w) || (y && !al16(y)) || (out32 && !al16(out32)) ||
        (out16 && !al8(out16)))
        return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(llama_rms_rows_kernel<PT>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, (long)rows, d,
                       w, eps, out32, static_cast<bf16_t*>(out16), rstd);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

template <int G>
void launch_attention(dim3 grid, hipStream_t s, int32_t precision, const float* qkv, int32_t ld, const int32_t* cu, int32_t rows, int32_t H,
                      int32_t Hkv, float scale, float* out32, void* out16) {
    const RaggedRows notes = {qkv, ld, cu, rows, Hkv};
    if (precision == 1)
        hipLaunchKernelGGL((gqa128::attn_mfma_kernel<G, RaggedRows>), grid, dim3(64 * G), 0, s, notes, H, scale, out32, static_cast<bf16_t*>(out16));
    else
        hipLaunchKernelGGL((gqa128::attn_valu_kernel<G, RaggedRows>), grid, dim3(64 * G), 0, s, notes, H, scale, out32, static_cast<bf16_t*>(out16));
}

template <typename PT>
int launch_tokens(const int32_t* ids, int32_t rows, const PT* embed, int32_t vocab, int32_t d, float* out, immtsf_stream_t stream) {
    if (!ids || !embed || !out || rows <= 0 || vocab <= 0 || d <= 0) return IMMTSF_EINVAL;
    if ((d & 3) || !param_al(embed) || !al16(out)) return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(llama_tokens_kernel<PT>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), ids, rows, embed,
                       vocab, d, out);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

template <typename PT>
int launch_pool(float* x, const float* y, const int32_t* cu, int32_t N, int32_t rows, int32_t d, const PT* w, float eps, float* rstd,
                float* pooled, immtsf_stream_t stream) {
    if (!cu || !w || !pooled || N <= 0 || rows < 0 || d <= 0 || (rows > 0 && (!x || !rstd))) return IMMTSF_EINVAL;
    if ((d + 255) / 256 > 65535) return IMMTSF_EUNSUPPORTED;
    if (rows > 0) {
        const int rc = launch_rms_rows(x, y, rows, d, w, eps, nullptr, nullptr, rstd, stream);
        if (rc != IMMTSF_OK) return rc;
    }
    hipLaunchKernelGGL(llama_pool_kernel<PT>, dim3((unsigned)N, (unsigned)((d + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                       rstd, cu, rows, d, w, pooled);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // namespace

extern "C" {

int immtsf_llama_embed_supported(int32_t d, int32_t H, int32_t H_kv, int32_t inner, int32_t max_len, int32_t max_positions) {
    return d > 0 && (d & 7) == 0 && inner > 0 && (inner & 7) == 0 && group_ok(H, H_kv) && H_kv <= 65535 && max_len >= 1 &&
           max_len <= max_positions && max_len <= MAXL;
}

// the buffers of one pass over `rows` packed tokens, each rounded up to 256 bytes, in this order: x (rows, d) fp32; h (rows, d) fp32 |
// bf16; qkv (rows, (H + 2 H_kv) 128) fp32; ao (rows, 128 H) fp32 | bf16; proj (rows, d) fp32; gu (rows, 2 inner) fp32; act (rows, inner)
// fp32 | bf16; cos, sin (max_len, 64) fp32; rstd (rows) fp32  (bf16 in precision 1: the images the bf16-in-memory GEMMs read)
size_t immtsf_llama_embed_workspace_bytes(int64_t rows, int32_t d, int32_t H, int32_t H_kv, int32_t inner, int32_t max_len, int32_t precision) {
    if (rows <= 0 || d <= 0 || H <= 0 || H_kv <= 0 || inner <= 0 || max_len <= 0) return 0;
    const size_t r = (size_t)rows, op = precision == 1 ? 2 : 4;
    return up256(r * d * 4) + up256(r * d * op) + up256(r * ((size_t)H + 2 * (size_t)H_kv) * HD * 4) + up256(r * H * HD * op) + up256(r * d * 4) +
           up256(r * 2 * inner * 4) + up256(r * inner * op) + 2 * up256((size_t)max_len * HP * 4) + up256(r * 4);
}

int immtsf_llama_embed_tokens(const int32_t* ids, int32_t rows, const float* embed, int32_t vocab, int32_t d, float* out, immtsf_stream_t stream) {
    return launch_tokens(ids, rows, embed, vocab, d, out, stream);
}

// the _p16 entry points: the same kernels with the model's parameter (the table, an RMSNorm weight) read as bf16
int immtsf_llama_embed_tokens_p16(const int32_t* ids, int32_t rows, const void* embed16, int32_t vocab, int32_t d, float* out,
                                  immtsf_stream_t stream) {
    return launch_tokens(ids, rows, static_cast<const bf16_t*>(embed16), vocab, d, out, stream);
}

int immtsf_llama_embed_rmsnorm_p16(const float* x, int64_t rows, int32_t d, const void* w16, float eps, float* out32, void* out16,
                                   immtsf_stream_t stream) {
    if (!out32 && !out16) return IMMTSF_EINVAL;
    return launch_rms_rows(const_cast<float*>(x), nullptr, rows, d, static_cast<const bf16_t*>(w16), eps, out32, out16, nullptr, stream);
}

int immtsf_llama_embed_add_rmsnorm_p16(float* x, const float* y, int64_t rows, int32_t d, const void* w16, float eps, float* out32, void* out16,
                                       immtsf_stream_t stream) {
    if (!y || (!out32 && !out16)) return IMMTSF_EINVAL;
    return launch_rms_rows(x, y, rows, d, static_cast<const bf16_t*>(w16), eps, out32, out16, nullptr, stream);
}

int immtsf_llama_embed_pool_p16(float* x, const float* y, const int32_t* cu, int32_t N, int32_t rows, int32_t d, const void* w16, float eps,
                                float* rstd, float* pooled, immtsf_stream_t stream) {
    return launch_pool(x, y, cu, N, rows, d, static_cast<const bf16_t*>(w16), eps, rstd, pooled, stream);
}

int immtsf_llama_embed_rmsnorm(const float* x, int64_t rows, int32_t d, const float* w, float eps, float* out32, void* out16,
                               immtsf_stream_t stream) {
    if (!out32 && !out16) return IMMTSF_EINVAL;
    return launch_rms_rows(const_cast<float*>(x), nullptr, rows, d, w, eps, out32, out16, nullptr, stream);      // (x is only read without y)
}

int immtsf_llama_embed_add_rmsnorm(float* x, const float* y, int64_t rows, int32_t d, const float* w, float eps, float* out32, void* out16,
                                   immtsf_stream_t stream) {
    if (!y || (!out32 && !out16)) return IMMTSF_EINVAL;
    return launch_rms_rows(x, y, rows, d, w, eps, out32, out16, nullptr, stream);
}

int immtsf_llama_embed_rope_table(const float* inv_freq, float attention_scaling, int32_t max_len, float* cos_out, float* sin_out,
                                  immtsf_stream_t stream) {
    if (!inv_freq || !cos_out || !sin_out || max_len <= 0) return IMMTSF_EINVAL;
    if (max_len > MAXL) return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(llama_rope_table_kernel, dim3((unsigned)((max_len * HP + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       inv_freq, attention_scaling, max_len, cos_out, sin_out);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_llama_embed_rope(float* qkv, int32_t ld, const int32_t* cu, int32_t N, int32_t rows, int32_t H, int32_t H_kv, int32_t max_len,
                            const float* cos_t, const float* sin_t, immtsf_stream_t stream) {
    if (!qkv || !cu || !cos_t || !sin_t || N <= 0 || rows <= 0 || H <= 0 || H_kv <= 0 || max_len <= 0) return IMMTSF_EINVAL;
    if (max_len > MAXL || (int64_t)ld < ((int64_t)H + 2 * (int64_t)H_kv) * HD) return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(llama_rope_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), qkv, ld, cu, N, rows,
                       H + H_kv, max_len, cos_t, sin_t);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_llama_embed_attention(const float* qkv, int32_t ld, const int32_t* cu, int32_t N, int32_t rows, int32_t H, int32_t H_kv,
                                 int32_t max_len, float scale, int32_t precision, float* out32, void* out16, immtsf_stream_t stream) {
    if (!qkv || !cu || (!out32 && !out16) || N <= 0 || rows <= 0 || H <= 0 || H_kv <= 0 || max_len <= 0) return IMMTSF_EINVAL;
    if (precision < 0 || precision > 1) return IMMTSF_EINVAL;
    if (!group_ok(H, H_kv) || H_kv > 65535 || max_len > MAXL || (int64_t)ld < ((int64_t)H + 2 * (int64_t)H_kv) * HD || (ld & 3) || !al16(qkv) ||
        (out32 && !al16(out32)) || (out16 && !al8(out16)))
        return IMMTSF_EUNSUPPORTED;
    const dim3 grid((unsigned)N, (unsigned)H_kv, (unsigned)((max_len + QT - 1) / QT));
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (H / H_kv) {
        case 1: launch_attention<1>(grid, s, precision, qkv, ld, cu, rows, H, H_kv, scale, out32, out16); break;
        case 2: launch_attention<2>(grid, s, precision, qkv, ld, cu, rows, H, H_kv, scale, out32, out16); break;
        case 4: launch_attention<4>(grid, s, precision, qkv, ld, cu, rows, H, H_kv, scale, out32, out16); break;
        default: launch_attention<8>(grid, s, precision, qkv, ld, cu, rows, H, H_kv, scale, out32, out16); break;
    }
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_llama_embed_swiglu(const float* gu, int64_t rows, int32_t inner, float* out32, void* out16, immtsf_stream_t stream) {
    if (!gu || (!out32 && !out16) || rows <= 0 || inner <= 0) return IMMTSF_EINVAL;
    if ((inner & 3) || !al16(gu) || (out32 && !al16(out32)) || (out16 && !al8(out16))) return IMMTSF_EUNSUPPORTED;
    const size_t n4 = (size_t)rows * (inner / 4);
    hipLaunchKernelGGL(llama_swiglu_kernel, dim3(grid_for(n4, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), gu, n4, inner / 4, out32,
                       static_cast<bf16_t*>(out16));
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_llama_embed_pool(float* x, const float* y, const int32_t* cu, int32_t N, int32_t rows, int32_t d, const float* w, float eps,
                            float* rstd, float* pooled, immtsf_stream_t stream) {
    return launch_pool(x, y, cu, N, rows, d, w, eps, rstd, pooled, stream);
}

}  // extern "C"
