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
//     bf16 MFMA and fp32 online softmax
//   * SwiGLU: silu(gate) up over the output of one product on gate_proj | up_proj
//   * final RMSNorm + mean-pool; a note of no tokens gives an exact 0 row
// Forward only, no dropout, no atomics, one writer per output element, every sum in a fixed order: two runs give the same bits.
//
// Launch of the attention kernels: grid (note, K/V head, query tile of 32 REVERSED), a workgroup of G = H / H_kv waves, one per query head
// of the K/V head; the waves fill the K / V tiles of 32 keys in LDS together and each reads them for its own head.  Workgroups are handed
// out in x, y, z order, so the last query tiles of the long notes -- the ones with the most keys -- start first and the short tiles fill
// in behind them; a (note, tile) past the note's end leaves at once (the whole workgroup: the test does not depend on the wave).
// A query tile is 32 and not the 64 of note_embed.hip: at head_dim 128 a wave's 64 queries need q + the output in 256 + registers and
// the G = 8 workgroup (512 threads) leaves a wave 256 in all; with 32 no instance spills.
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

constexpr int HD = 128;       // head_dim
constexpr int HP = HD / 2;    // rotary pairs of a head
constexpr int QT = 32;        // queries per wave (= per query head of a workgroup)
constexpr int KT = 32;        // keys per LDS tile
constexpr int KC = 4;         // keys per softmax chunk of the VALU form
constexpr int MAXL = 1024;    // longest note (tokens)
constexpr int KS_LD = HD + 8; // bf16 K tile [key][e]: 272-byte rows (16-byte fragments)
constexpr int VT_LD = KT + 8; // bf16 V tile transposed [e][key]: 80-byte rows (8-byte fragments)

struct NoteRange { int r0, L; };
// rows of note n; a range that does not lie inside [0, rows) counts as empty
__device__ __forceinline__ NoteRange note_range(const int32_t* __restrict__ cu, int n, int rows) {
    const int a = cu[n], b = cu[n + 1];
    NoteRange r = {a, b - a};
    if (a < 0 || b < a || b > rows || r.L > MAXL) r.L = 0;
    return r;
}

// ---- x[r, :] = embed[ids[r], :], one wave per row; an id outside the table is clamped into it (the host raises first) --------------------
__global__ void __launch_bounds__(256) llama_tokens_kernel(const int32_t* __restrict__ ids, int rows, const float* __restrict__ embed, int vocab,
                                                           int d, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    int id = ids[r];
    id = id < 0 ? 0 : id >= vocab ? vocab - 1 : id;
    const float4* a = reinterpret_cast<const float4*>(embed + (size_t)id * d);
    float4* o = reinterpret_cast<float4*>(out + (size_t)r * d);
    for (int e = lane; e < (d >> 2); e += 64) o[e] = a[e];
}

// ---- RMSNorm rows, one wave per row -------------------------------------------------------------------------------------------------------
// y given: x[r] <- x[r] + y[r] first (the residual add of the product before).  Then, each when its pointer is given: out32 / out16[r] =
// x[r] rsqrt(mean(x[r]^2) + eps) w, and rstd[r] = that rsqrt alone (what the pool reads).  Lane l writes, and alone reads back, its own
// elements of x.
__global__ void __launch_bounds__(256) llama_rms_rows_kernel(float* x, const float* __restrict__ y, long rows, int d, const float* __restrict__ w,
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
    const float4* w4 = reinterpret_cast<const float4*>(w);
    for (int e = lane; e < d4; e += 64) {
        const float4 v = xr[e], g = w4[e];
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

// ---- ragged causal attention, fp32 on the VALU ---------------------------------------------------------------------------------------
// wave w of the workgroup is query head G kvh + w.  TWO lanes own one query: lane 2 q + hf holds head columns 64 hf .. 64 hf + 63 of q
// and of the output row (64 + 64 registers), the halves of a score meet through one DPP exchange with lane ^ 1, and both lanes carry
// the same softmax state.  K / V tiles of KT keys go through LDS as broadcasts (two addresses per read).
template <int G>
__global__ void __launch_bounds__(64 * G) llama_attn_valu_kernel(const float* __restrict__ qkv, int ld, const int32_t* __restrict__ cu, int rows,
                                                                 int H, int Hkv, float scale, float* __restrict__ o32,
                                                                 bf16_t* __restrict__ o16) {
    __shared__ float4 Ks[KT * HD / 4];
    __shared__ float4 Vs[KT * HD / 4];
    const int tid = threadIdx.x, lane = tid & 63, qi = lane >> 1, hf = lane & 1;
    const int n = blockIdx.x, kvh = blockIdx.y, h = kvh * G + (tid >> 6);
    const int t0 = ((int)gridDim.z - 1 - (int)blockIdx.z) * QT;
    const NoteRange nr = note_range(cu, n, rows);
    if (t0 >= nr.L) return;
    const int L = nr.L, dq = H * HD;
    const bool live = t0 + qi < L;
    const int t = live ? t0 + qi : L - 1;                   // clamped: an idle lane repeats the last query and writes nothing
    const float* kb = qkv + (size_t)nr.r0 * ld + dq + kvh * HD;
    const float* vb = kb + Hkv * HD;
    float qr[HD / 2], acc[HD / 2];
    {
        const float4* qp = reinterpret_cast<const float4*>(qkv + ((size_t)nr.r0 + t) * ld + h * HD + (HD / 2) * hf);
#pragma unroll
        for (int e = 0; e < HD / 8; ++e) {
            const float4 x = qp[e];
            qr[4 * e] = x.x * scale; qr[4 * e + 1] = x.y * scale; qr[4 * e + 2] = x.z * scale; qr[4 * e + 3] = x.w * scale;
        }
    }
#pragma unroll
    for (int e = 0; e < HD / 2; ++e) acc[e] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int kend = min(t0 + QT, L);                       // keys 0 .. kend-1 are visible to some query of the workgroup
    for (int j0 = 0; j0 < kend; j0 += KT) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KT * HD / 4 / (64 * G); ++i) {
            const int idx = tid + 64 * G * i, kk = idx >> 5, part = idx & 31, j = j0 + kk;
            float4 a = {0.f, 0.f, 0.f, 0.f}, c = a;
            if (j < kend) {
                a = reinterpret_cast<const float4*>(kb + (size_t)j * ld)[part];
                c = reinterpret_cast<const float4*>(vb + (size_t)j * ld)[part];
            }
            Ks[idx] = a;
            Vs[idx] = c;
        }
        __syncthreads();
#pragma unroll 1
        for (int c4 = 0; c4 < KT && j0 + c4 < kend; c4 += KC) {
            float sc[KC];
            float cmax = -INFINITY;
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                float a = 0.f;
#pragma unroll
                for (int e = 0; e < HD / 8; ++e) {
                    const float4 kk = Ks[(c4 + c) * (HD / 4) + (HD / 8) * hf + e];
                    a += qr[4 * e] * kk.x + qr[4 * e + 1] * kk.y + qr[4 * e + 2] * kk.z + qr[4 * e + 3] * kk.w;
                }
                a += IMMTSF_DPP(a, 0xB1);                   // quad_perm [1,0,3,2]: the other half of the head (every lane is active here)
                sc[c] = (j0 + c4 + c <= t) ? a : -INFINITY;
                cmax = fmaxf(cmax, sc[c]);
            }
            // (the running maximum is finite from the first chunk on: key 0 is visible to every query; a later chunk that lies wholly
            // above the query leaves the state alone: cmax = -inf, every p = exp(-inf - m) = 0)
            if (cmax > m) {
                const float corr = __expf(m - cmax);
                m = cmax;
                l *= corr;
#pragma unroll
                for (int e = 0; e < HD / 2; ++e) acc[e] *= corr;
            }
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const float p = __expf(sc[c] - m);
                l += p;
#pragma unroll
                for (int e = 0; e < HD / 8; ++e) {
                    const float4 vv = Vs[(c4 + c) * (HD / 4) + (HD / 8) * hf + e];
                    acc[4 * e] += p * vv.x; acc[4 * e + 1] += p * vv.y; acc[4 * e + 2] += p * vv.z; acc[4 * e + 3] += p * vv.w;
                }
            }
        }
    }
    if (!live) return;
    const float inv = 1.f / l;
    const size_t orow = ((size_t)nr.r0 + t) * dq + h * HD + (HD / 2) * hf;
    if (o32) {
#pragma unroll
        for (int e = 0; e < HD / 8; ++e)
            reinterpret_cast<float4*>(o32 + orow)[e] = float4{acc[4 * e] * inv, acc[4 * e + 1] * inv, acc[4 * e + 2] * inv, acc[4 * e + 3] * inv};
    }
    if (o16) {
#pragma unroll
        for (int e = 0; e < HD / 8; ++e)
            reinterpret_cast<bf16x4*>(o16 + orow)[e] = bf16x4{(bf16_t)(acc[4 * e] * inv), (bf16_t)(acc[4 * e + 1] * inv),
                                                             (bf16_t)(acc[4 * e + 2] * inv), (bf16_t)(acc[4 * e + 3] * inv)};
    }
}

// ---- ragged causal attention, bf16 MFMA -------------------------------------------------------------------------------------------------
// The transposed form of note_embed.hip widened to head_dim 128.  Wave w owns 32 queries of head G kvh + w as two 16-query column tiles.
// mfma_f32_16x16x32_bf16, lane l: fr = l & 15, g = l >> 4; A[row fr][k = 8 g + j], B[k = 8 g + j][col fr], C[row 4 g + i][col fr]:
//   S^T (keys x queries) = K (A: a key row from the LDS tile, k = head column, FOUR k-steps) . Q^T (B: a query row from global memory,
//   held for the whole key loop).  A lane holds, for ITS query fr, the scores of keys 4 g + i of each 16-key subtile: the row maximum
//   and sum are an in-register reduction plus two cross-row steps (lanes fr, fr + 16, fr + 32, fr + 48), all fp32.
//   O^T (head columns x queries) += V^T (A) . P^T (B), EIGHT 16-column output tiles.  The B fragment of lane (fr, g) is k-slot j -> key
//   4 g + j (j < 4) or 16 + 4 g + (j - 4): exactly the eight probabilities the lane already holds, rounded to bf16.  The A fragment takes
//   V in the same k order: row e = 16 et + fr of the transposed V tile, keys 4 g .. 4 g + 3 and 16 + 4 g .. 16 + 4 g + 3.
// Query tile and key tile are both 32 and aligned, so every key tile of the loop starts at or below every query of the workgroup: no
// 16-query tile is ever skipped, and the running maximum is finite from the first tile on (key j0 is visible to each query).
__device__ __forceinline__ f32x4 le_mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

template <int G>
__global__ void __launch_bounds__(64 * G) llama_attn_mfma_kernel(const float* __restrict__ qkv, int ld, const int32_t* __restrict__ cu, int rows,
                                                                 int H, int Hkv, float scale, float* __restrict__ o32,
                                                                 bf16_t* __restrict__ o16) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[KT * KS_LD];
    __shared__ __attribute__((aligned(16))) bf16_t Vt[HD * VT_LD];
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, g = lane >> 4;
    const int n = blockIdx.x, kvh = blockIdx.y, h = kvh * G + (tid >> 6);
    const int t0 = ((int)gridDim.z - 1 - (int)blockIdx.z) * QT;
    const NoteRange nr = note_range(cu, n, rows);
    if (t0 >= nr.L) return;
    const int L = nr.L, dq = H * HD;
    const float* kb = qkv + (size_t)nr.r0 * ld + dq + kvh * HD;
    const float* vb = kb + Hkv * HD;
    bf16x8 qf[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int t = min(t0 + 16 * mt + fr, L - 1);        // clamped: a query past the end repeats the last one and is not written
        const float4* qp = reinterpret_cast<const float4*>(qkv + ((size_t)nr.r0 + t) * ld + h * HD);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const float4 a = qp[8 * ks + 2 * g], b = qp[8 * ks + 2 * g + 1];
            qf[mt][ks] = bf16x8{(bf16_t)a.x, (bf16_t)a.y, (bf16_t)a.z, (bf16_t)a.w, (bf16_t)b.x, (bf16_t)b.y, (bf16_t)b.z, (bf16_t)b.w};
        }
    }
    f32x4 O[2][8];
    float m[2], ls[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        m[mt] = -INFINITY;
        ls[mt] = 0.f;
#pragma unroll
        for (int et = 0; et < 8; ++et) O[mt][et] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int kend = min(t0 + QT, L);
    for (int j0 = 0; j0 < kend; j0 += KT) {
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < KT * HD / 4 / (64 * G); ++i) {
            const int idx = tid + 64 * G * i, kk = idx >> 5, part = idx & 31, j = j0 + kk;
            float4 a = {0.f, 0.f, 0.f, 0.f}, c = a;
            if (j < kend) {
                a = reinterpret_cast<const float4*>(kb + (size_t)j * ld)[part];
                c = reinterpret_cast<const float4*>(vb + (size_t)j * ld)[part];
            }
            *reinterpret_cast<bf16x4*>(&Ks[kk * KS_LD + 4 * part]) = bf16x4{(bf16_t)a.x, (bf16_t)a.y, (bf16_t)a.z, (bf16_t)a.w};
            Vt[(4 * part + 0) * VT_LD + kk] = (bf16_t)c.x;
            Vt[(4 * part + 1) * VT_LD + kk] = (bf16_t)c.y;
            Vt[(4 * part + 2) * VT_LD + kk] = (bf16_t)c.z;
            Vt[(4 * part + 3) * VT_LD + kk] = (bf16_t)c.w;
        }
        __syncthreads();
        bf16x8 kf[2][4], vf[8];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) kf[nt][ks] = *reinterpret_cast<const bf16x8*>(&Ks[(16 * nt + fr) * KS_LD + 32 * ks + 8 * g]);
#pragma unroll
        for (int et = 0; et < 8; ++et) {
            const bf16x4 lo = *reinterpret_cast<const bf16x4*>(&Vt[(16 * et + fr) * VT_LD + 4 * g]);
            const bf16x4 hi = *reinterpret_cast<const bf16x4*>(&Vt[(16 * et + fr) * VT_LD + 16 + 4 * g]);
            vf[et] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int qi = t0 + 16 * mt + fr;               // the last key this lane's query sees
            float s[2][4];
            float cmax = -INFINITY;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                f32x4 S = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) S = le_mfma(kf[nt][ks], qf[mt][ks], S);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    s[nt][i] = (j0 + 16 * nt + 4 * g + i <= qi) ? S[i] * scale : -INFINITY;
                    cmax = fmaxf(cmax, s[nt][i]);
                }
            }
            cmax = xor32_max(xor16_max(cmax));
            const float mn = fmaxf(m[mt], cmax);
            const float corr = __expf(m[mt] - mn);
            m[mt] = mn;
            float psum = 0.f;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    s[nt][i] = __expf(s[nt][i] - mn);
                    psum += s[nt][i];
                }
            ls[mt] = ls[mt] * corr + psum;                   // (the lane's share of the row sum; the four shares meet after the loop)
            const bf16x8 pf = bf16x8{(bf16_t)s[0][0], (bf16_t)s[0][1], (bf16_t)s[0][2], (bf16_t)s[0][3],
                                     (bf16_t)s[1][0], (bf16_t)s[1][1], (bf16_t)s[1][2], (bf16_t)s[1][3]};
#pragma unroll
            for (int et = 0; et < 8; ++et) {
                f32x4 o = O[mt][et];
                o[0] *= corr; o[1] *= corr; o[2] *= corr; o[3] *= corr;
                O[mt][et] = le_mfma(vf[et], pf, o);
            }
        }
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const float l = xor32_sum(xor16_sum(ls[mt]));        // shares of lanes fr, fr + 16, fr + 32, fr + 48 in one fixed order
        const int t = t0 + 16 * mt + fr;
        if (t >= L) continue;
        const float inv = 1.f / l;
        const size_t orow = ((size_t)nr.r0 + t) * dq + h * HD + 4 * g;
#pragma unroll
        for (int et = 0; et < 8; ++et) {
            const f32x4 o = O[mt][et];
            if (o32) *reinterpret_cast<float4*>(o32 + orow + 16 * et) = float4{o[0] * inv, o[1] * inv, o[2] * inv, o[3] * inv};
            if (o16)
                *reinterpret_cast<bf16x4*>(o16 + orow + 16 * et) =
                    bf16x4{(bf16_t)(o[0] * inv), (bf16_t)(o[1] * inv), (bf16_t)(o[2] * inv), (bf16_t)(o[3] * inv)};
        }
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
__global__ void __launch_bounds__(256) llama_pool_kernel(const float* __restrict__ x, const float* __restrict__ rstd,
                                                         const int32_t* __restrict__ cu, int rows, int d, const float* __restrict__ w,
                                                         float* __restrict__ pooled) {
    const int n = blockIdx.x, e = blockIdx.y * 256 + threadIdx.x;
    if (e >= d) return;
    const NoteRange nr = note_range(cu, n, rows);
    const float* xb = x + (size_t)nr.r0 * d + e;
    float acc = 0.f;
    for (int p = 0; p < nr.L; ++p) acc += xb[(size_t)p * d] * rstd[nr.r0 + p];
    pooled[(size_t)n * d + e] = acc * w[e] / (float)(nr.L > 1 ? nr.L : 1);
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
inline unsigned grid_for(size_t n, int per) {
    const size_t g = (n + per - 1) / per;
    return (unsigned)(g < 1 ? 1 : g > 65536 ? 65536 : g);
}
inline bool group_ok(int H, int Hkv) {
    if (H <= 0 || Hkv <= 0 || H % Hkv) return false;
    const int G = H / Hkv;
    return G == 1 || G == 2 || G == 4 || G == 8;
}

int launch_rms_rows(float* x, const float* y, int64_t rows, int32_t d, const float* w, float eps, float* out32, void* out16, float* rstd,
                    immtsf_stream_t stream) {
    if (!x || !w || rows <= 0 || d <= 0 || (!out32 && !out16 && !rstd)) return IMMTSF_EINVAL;
    if (rows > 0x7fffffffLL || (d & 3) || !al16(x) || !al16(w) || (y && !al16(y)) || (out32 && !al16(out32)) ||
        (out16 && (reinterpret_cast<uintptr_t>(out16) & 7)))
        return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(llama_rms_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, (long)rows, d,
                       w, eps, out32, static_cast<bf16_t*>(out16), rstd);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

template <int G>
void launch_attention(dim3 grid, hipStream_t s, int32_t precision, const float* qkv, int32_t ld, const int32_t* cu, int32_t rows, int32_t H,
                      int32_t Hkv, float scale, float* out32, void* out16) {
    if (precision == 1)
        hipLaunchKernelGGL(llama_attn_mfma_kernel<G>, grid, dim3(64 * G), 0, s, qkv, ld, cu, rows, H, Hkv, scale, out32,
                           static_cast<bf16_t*>(out16));
    else
        hipLaunchKernelGGL(llama_attn_valu_kernel<G>, grid, dim3(64 * G), 0, s, qkv, ld, cu, rows, H, Hkv, scale, out32,
                           static_cast<bf16_t*>(out16));
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
    if (!ids || !embed || !out || rows <= 0 || vocab <= 0 || d <= 0) return IMMTSF_EINVAL;
    if ((d & 3) || !al16(embed) || !al16(out)) return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(llama_tokens_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), ids, rows, embed,
                       vocab, d, out);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
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
        (out32 && !al16(out32)) || (out16 && (reinterpret_cast<uintptr_t>(out16) & 7)))
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
    if ((inner & 3) || !al16(gu) || (out32 && !al16(out32)) || (out16 && (reinterpret_cast<uintptr_t>(out16) & 7))) return IMMTSF_EUNSUPPORTED;
    const size_t n4 = (size_t)rows * (inner / 4);
    hipLaunchKernelGGL(llama_swiglu_kernel, dim3(grid_for(n4, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), gu, n4, inner / 4, out32,
                       static_cast<bf16_t*>(out16));
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_llama_embed_pool(float* x, const float* y, const int32_t* cu, int32_t N, int32_t rows, int32_t d, const float* w, float eps,
                            float* rstd, float* pooled, immtsf_stream_t stream) {
    if (!cu || !w || !pooled || N <= 0 || rows < 0 || d <= 0 || (rows > 0 && (!x || !rstd))) return IMMTSF_EINVAL;
    if ((d + 255) / 256 > 65535) return IMMTSF_EUNSUPPORTED;
    if (rows > 0) {
        const int rc = launch_rms_rows(x, y, rows, d, w, eps, nullptr, nullptr, rstd, stream);
        if (rc != IMMTSF_OK) return rc;
    }
    hipLaunchKernelGGL(llama_pool_kernel, dim3((unsigned)N, (unsigned)((d + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, rstd,
                       cu, rows, d, w, pooled);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
