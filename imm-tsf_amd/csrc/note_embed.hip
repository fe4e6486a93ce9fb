// Raw-text mode: a frozen GPT-2 over the RAGGED tokens of a batch of notes, mean-pooled per note (reference fusions/load_llm.py
// embed_notes: every note padded to max_length, the padded batch through the LLM, the mean over the real tokens).  GPT-2 is causal and
// its tokenizer pads on the right, so a real token's hidden state never depends on a pad token and the pool never reads a pad row: the
// function is computed over the sum(L) real tokens, notes back to back (`cu` = N + 1 prefix sums of the token counts, on the device).
// This file has what the packed form needs beside the GEMM family and the row kernels of gpt2.hip (which run over the packed rows as
// one sequence, B = 1):
//   * token embedding: row r of note n at position p = wte[ids[r]] + wpe[p]
//   * causal attention forward over ragged sequences, Q / K / V read in c_attn's output layout (row pitch 3 d, head h at columns 64 h),
//     output in the layout c_proj reads.  fp32 mode: one query per thread, keys through LDS (the form of attn_dense64.hpp with the
//     key range taken from cu).  bf16 mode: both products on bf16 MFMA with fp32 accumulation, fp32 online softmax.
//   * ln_f + mean-pool: LayerNorm of each row of a note, summed in position order, / max(L, 1); a note of no tokens gives an exact 0 row
// Forward only, no dropout, no atomics, one writer per output element, every sum in a fixed order: two runs give the same bits.
// The two attention kernels are templates on a CAUSAL switch: the non-causal instances (every query of a note sees all its keys) serve
// the frozen BERT of bert_embed.hip through immtsf_bert_embed_attention, defined at the end of this file.
//
// Launch of the attention kernels: grid (note, head, query tile of 64 REVERSED), one wave per workgroup.  Workgroups are handed out in
// x, y, z order, so the last query tiles of the long notes -- the ones with the most keys -- start first and the short tiles fill in
// behind them; a (note, tile) past the note's end leaves at once.  A 1024-token note is 16 independent workgroups per head, the longest
// of which reads 32 key tiles.
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

constexpr int HD = 64;        // head_dim
constexpr int QT = 64;        // queries per workgroup (one wave)
constexpr int KT = 32;        // keys per LDS tile
constexpr int KC = 4;         // keys per softmax chunk of the VALU form
constexpr int MAXL = 1024;    // longest note (tokens)
constexpr int KS_LD = HD + 8; // bf16 K tile [key][e]: 144-byte rows (16-byte fragments, no 2-way bank repeat between key rows)
constexpr int VT_LD = KT + 8; // bf16 V tile transposed [e][key]: 80-byte rows (8-byte fragments)

struct NoteRange { int r0, L; };
// rows of note n; a range that does not lie inside [0, rows) counts as empty
__device__ __forceinline__ NoteRange note_range(const int32_t* __restrict__ cu, int n, int rows) {
    const int a = cu[n], b = cu[n + 1];
    NoteRange r = {a, b - a};
    if (a < 0 || b < a || b > rows || r.L > MAXL) r.L = 0;
    return r;
}

// ---- x[r, :] = wte[ids[r], :] + wpe[p, :], one wave per row ----------------------------------------------------------------------------
__global__ void __launch_bounds__(256) note_tokens_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ cu, int N, int rows,
                                                          const float* __restrict__ wte, int vocab, const float* __restrict__ wpe,
                                                          int n_positions, int d, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    int lo = 0, hi = N;               // the last n in [0, N) with cu[n] <= r (notes of no tokens share their successor's start)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cu[mid] <= (int)r) lo = mid; else hi = mid;
    }
    int p = (int)r - cu[lo];
    p = p < 0 ? 0 : p >= n_positions ? n_positions - 1 : p;
    int id = ids[r];
    id = id < 0 ? 0 : id >= vocab ? vocab - 1 : id;
    const float4* a = reinterpret_cast<const float4*>(wte + (size_t)id * d);
    const float4* b = reinterpret_cast<const float4*>(wpe + (size_t)p * d);
    float4* o = reinterpret_cast<float4*>(out + (size_t)r * d);
    for (int e = lane; e < (d >> 2); e += 64) {
        const float4 x = a[e], y = b[e];
        o[e] = float4{x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w};
    }
}

// ---- ragged causal attention, fp32 on the VALU ---------------------------------------------------------------------------------------
// a thread owns one query (q, the output row and the softmax state in registers); K / V tiles of KT keys go through LDS as broadcasts.
// CAUSAL (GPT-2): query t sees keys 0 .. t.  Not CAUSAL (BERT): every query of a note sees keys 0 .. L - 1, so the bound of the last key
// tile is L itself and not the query's position.
template <bool CAUSAL>
__global__ void __launch_bounds__(64) note_attn_valu_kernel(const float* __restrict__ qkv, int ld, const int32_t* __restrict__ cu, int rows,
                                                            int d, float scale, float* __restrict__ o32, bf16_t* __restrict__ o16) {
    __shared__ float4 Ks[KT * HD / 4];
    __shared__ float4 Vs[KT * HD / 4];
    const int lane = threadIdx.x, n = blockIdx.x, h = blockIdx.y;
    const int t0 = ((int)gridDim.z - 1 - (int)blockIdx.z) * QT;
    const NoteRange nr = note_range(cu, n, rows);
    if (t0 >= nr.L) return;
    const int L = nr.L;
    const bool live = t0 + lane < L;
    const int t = live ? t0 + lane : L - 1;                 // clamped: an idle lane repeats the last query and writes nothing
    const float* kb = qkv + (size_t)nr.r0 * ld + d + h * HD;
    const float* vb = kb + d;
    float qr[HD], acc[HD];
    {
        const float4* qp = reinterpret_cast<const float4*>(qkv + ((size_t)nr.r0 + t) * ld + h * HD);
#pragma unroll
        for (int e = 0; e < HD / 4; ++e) {
            const float4 x = qp[e];
            qr[4 * e] = x.x * scale; qr[4 * e + 1] = x.y * scale; qr[4 * e + 2] = x.z * scale; qr[4 * e + 3] = x.w * scale;
        }
    }
#pragma unroll
    for (int e = 0; e < HD; ++e) acc[e] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int kend = CAUSAL ? min(t0 + QT, L) : L;          // keys 0 .. kend-1 are visible to some query of the wave
    for (int j0 = 0; j0 < kend; j0 += KT) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KT * HD / 4 / 64; ++i) {
            const int idx = lane + 64 * i, kk = idx >> 4, part = idx & 15, j = j0 + kk;
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
                for (int e = 0; e < HD / 4; ++e) {
                    const float4 kk = Ks[(c4 + c) * (HD / 4) + e];
                    a += qr[4 * e] * kk.x + qr[4 * e + 1] * kk.y + qr[4 * e + 2] * kk.z + qr[4 * e + 3] * kk.w;
                }
                sc[c] = (j0 + c4 + c < (CAUSAL ? t + 1 : L)) ? a : -INFINITY;
                cmax = fmaxf(cmax, sc[c]);
            }
            // (the running maximum is finite from the first chunk on: key 0 is visible to every query; a chunk is entered only when its
            // first key lies below kend, so without the causal bound every chunk has a visible key too)
            if (cmax > m) {
                const float corr = __expf(m - cmax);
                m = cmax;
                l *= corr;
#pragma unroll
                for (int e = 0; e < HD; ++e) acc[e] *= corr;
            }
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const float p = __expf(sc[c] - m);
                l += p;
#pragma unroll
                for (int e = 0; e < HD / 4; ++e) {
                    const float4 vv = Vs[(c4 + c) * (HD / 4) + e];
                    acc[4 * e] += p * vv.x; acc[4 * e + 1] += p * vv.y; acc[4 * e + 2] += p * vv.z; acc[4 * e + 3] += p * vv.w;
                }
            }
        }
    }
    if (!live) return;
    const float inv = 1.f / l;
    const size_t orow = ((size_t)nr.r0 + t) * d + h * HD;
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
}

// ---- ragged causal attention, bf16 MFMA -------------------------------------------------------------------------------------------------
// One wave owns 64 queries as four 16-query column tiles.  Both products are computed TRANSPOSED with mfma_f32_16x16x32_bf16 (lane l:
// fr = l & 15, g = l >> 4; A[row fr][k = 8 g + j], B[k = 8 g + j][col fr], C[row 4 g + i][col fr]):
//   S^T (keys x queries) = K (A: a key row from the LDS tile, k = head column) . Q^T (B: a query row from global memory, held for the
//   whole key loop).  A lane then holds, for ITS query fr, the scores of keys 4 g + i of each 16-key subtile: the row maximum and sum are
//   an in-register reduction plus two cross-row steps (lanes fr, fr + 16, fr + 32, fr + 48), all fp32.
//   O^T (head columns x queries) += V^T (A) . P^T (B).  The B fragment of lane (fr, g) is k-slot j -> key 4 g + j (j < 4) or
//   16 + 4 g + (j - 4): exactly the eight probabilities the lane already holds, rounded to bf16 -- no LDS round trip and no lane
//   movement.  The A fragment takes V in the same k order: row e = 16 et + fr of the transposed V tile, keys 4 g .. 4 g + 3 and
//   16 + 4 g .. 16 + 4 g + 3 (two 8-byte LDS reads).
// The output row of a query lies across the 4 lanes with its fr: 4 consecutive head columns per 16-column tile each (16-byte stores).
__device__ __forceinline__ f32x4 ne_mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// Not CAUSAL: the key loop runs to L for every query tile, the last 32-key tile is masked by L, and a 16-query tile that starts past the
// note's end is skipped (its queries are clamped copies and nothing of it is written).
template <bool CAUSAL>
__global__ void __launch_bounds__(64) note_attn_mfma_kernel(const float* __restrict__ qkv, int ld, const int32_t* __restrict__ cu, int rows,
                                                            int d, float scale, float* __restrict__ o32, bf16_t* __restrict__ o16) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[KT * KS_LD];
    __shared__ __attribute__((aligned(16))) bf16_t Vt[HD * VT_LD];
    const int lane = threadIdx.x, fr = lane & 15, g = lane >> 4, n = blockIdx.x, h = blockIdx.y;
    const int t0 = ((int)gridDim.z - 1 - (int)blockIdx.z) * QT;
    const NoteRange nr = note_range(cu, n, rows);
    if (t0 >= nr.L) return;
    const int L = nr.L;
    const float* kb = qkv + (size_t)nr.r0 * ld + d + h * HD;
    const float* vb = kb + d;
    bf16x8 qf[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int t = min(t0 + 16 * mt + fr, L - 1);        // clamped: a query past the end repeats the last one and is not written
        const float4* qp = reinterpret_cast<const float4*>(qkv + ((size_t)nr.r0 + t) * ld + h * HD);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const float4 a = qp[8 * ks + 2 * g], b = qp[8 * ks + 2 * g + 1];
            qf[mt][ks] = bf16x8{(bf16_t)a.x, (bf16_t)a.y, (bf16_t)a.z, (bf16_t)a.w, (bf16_t)b.x, (bf16_t)b.y, (bf16_t)b.z, (bf16_t)b.w};
        }
    }
    f32x4 O[4][4];
    float m[4], ls[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        m[mt] = -INFINITY;
        ls[mt] = 0.f;
#pragma unroll
        for (int et = 0; et < 4; ++et) O[mt][et] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int kend = CAUSAL ? min(t0 + QT, L) : L;
    for (int j0 = 0; j0 < kend; j0 += KT) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KT * HD / 4 / 64; ++i) {
            const int idx = lane + 64 * i, kk = idx >> 4, part = idx & 15, j = j0 + kk;
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
        bf16x8 kf[2][2], vf[4];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) kf[nt][ks] = *reinterpret_cast<const bf16x8*>(&Ks[(16 * nt + fr) * KS_LD + 32 * ks + 8 * g]);
#pragma unroll
        for (int et = 0; et < 4; ++et) {
            const bf16x4 lo = *reinterpret_cast<const bf16x4*>(&Vt[(16 * et + fr) * VT_LD + 4 * g]);
            const bf16x4 hi = *reinterpret_cast<const bf16x4*>(&Vt[(16 * et + fr) * VT_LD + 16 + 4 * g]);
            vf[et] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            // a 16-query tile that ends below the key tile sees none of it; one that is not skipped has j0 <= its first query (j0 is a
            // multiple of 32, the tile base of 16), so each of its queries sees key j0 and the running maximum below is finite
            // (without the causal bound: j0 < L, so key j0 is visible to every query)
            if (CAUSAL ? j0 > t0 + 16 * mt + 15 : t0 + 16 * mt >= L) continue;
            const int qi = CAUSAL ? t0 + 16 * mt + fr : L - 1;     // the last key this lane's query sees
            float s[2][4];
            float cmax = -INFINITY;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                f32x4 S = ne_mfma(kf[nt][0], qf[mt][0], f32x4{0.f, 0.f, 0.f, 0.f});
                S = ne_mfma(kf[nt][1], qf[mt][1], S);
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
            for (int et = 0; et < 4; ++et) {
                f32x4 o = O[mt][et];
                o[0] *= corr; o[1] *= corr; o[2] *= corr; o[3] *= corr;
                O[mt][et] = ne_mfma(vf[et], pf, o);
            }
        }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const float l = xor32_sum(xor16_sum(ls[mt]));        // shares of lanes fr, fr + 16, fr + 32, fr + 48 in one fixed order
        const int t = t0 + 16 * mt + fr;
        if (t >= L) continue;
        const float inv = 1.f / l;
        const size_t orow = ((size_t)nr.r0 + t) * d + h * HD + 4 * g;
#pragma unroll
        for (int et = 0; et < 4; ++et) {
            const f32x4 o = O[mt][et];
            if (o32) *reinterpret_cast<float4*>(o32 + orow + 16 * et) = float4{o[0] * inv, o[1] * inv, o[2] * inv, o[3] * inv};
            if (o16)
                *reinterpret_cast<bf16x4*>(o16 + orow + 16 * et) =
                    bf16x4{(bf16_t)(o[0] * inv), (bf16_t)(o[1] * inv), (bf16_t)(o[2] * inv), (bf16_t)(o[3] * inv)};
        }
    }
}

// ---- pooled[n, :] = sum over the rows of note n, in position order, of LayerNorm(x[row]) / max(L, 1) -----------------------------------
// one workgroup per note: its waves take the rows' statistics (a row per wave at a time) into LDS, then a thread owns output columns
__global__ void __launch_bounds__(256) note_pool_kernel(const float* __restrict__ x, const int32_t* __restrict__ cu, int rows, int d,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                        float* __restrict__ pooled) {
    __shared__ float mean_s[MAXL];
    __shared__ float rstd_s[MAXL];
    const int n = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const NoteRange nr = note_range(cu, n, rows);
    const float* xb = x + (size_t)nr.r0 * d;
    for (int p = w; p < nr.L; p += 4) {
        const float* xr = xb + (size_t)p * d;
        float s = 0.f;
        for (int e = lane; e < d; e += 64) s += xr[e];
        const float mean = wave_sum(s) / (float)d;
        float v = 0.f;
        for (int e = lane; e < d; e += 64) { const float c = xr[e] - mean; v += c * c; }
        const float rstd = rsqrtf(wave_sum(v) / (float)d + eps);
        if (lane == 0) { mean_s[p] = mean; rstd_s[p] = rstd; }
    }
    __syncthreads();
    const float div = (float)(nr.L > 1 ? nr.L : 1);
    for (int e = threadIdx.x; e < d; e += 256) {
        const float ga = gamma[e], be = beta[e];
        float acc = 0.f;
        for (int p = 0; p < nr.L; ++p) acc += (xb[(size_t)p * d + e] - mean_s[p]) * rstd_s[p] * ga + be;
        pooled[(size_t)n * d + e] = acc / div;
    }
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

template <bool CAUSAL>
int launch_attention(const float* qkv, int32_t ld, const int32_t* cu, int32_t N, int32_t rows, int32_t H, int32_t max_len, float scale,
                            int32_t precision, float* out32, void* out16, immtsf_stream_t stream) {
    if (!qkv || !cu || (!out32 && !out16) || N <= 0 || rows <= 0 || H <= 0 || max_len <= 0) return IMMTSF_EINVAL;
    if (precision < 0 || precision > 1) return IMMTSF_EINVAL;
    if (H > 65535 || max_len > MAXL || ld < 3 * H * HD || (ld & 3) || !al16(qkv) || (out32 && !al16(out32)) ||
        (out16 && !al8(out16)))
        return IMMTSF_EUNSUPPORTED;
    const dim3 grid((unsigned)N, (unsigned)H, (unsigned)((max_len + QT - 1) / QT));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (precision == 1)
        hipLaunchKernelGGL(note_attn_mfma_kernel<CAUSAL>, grid, dim3(64), 0, s, qkv, ld, cu, rows, H * HD, scale, out32,
                           static_cast<bf16_t*>(out16));
    else
        hipLaunchKernelGGL(note_attn_valu_kernel<CAUSAL>, grid, dim3(64), 0, s, qkv, ld, cu, rows, H * HD, scale, out32,
                           static_cast<bf16_t*>(out16));
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // namespace

extern "C" {

int immtsf_note_embed_supported(int32_t d, int32_t H, int32_t max_len, int32_t n_positions) {
    return d > 0 && H > 0 && H <= 65535 && d == H * HD && max_len >= 1 && max_len <= n_positions && max_len <= MAXL;
}

// the activations of one pass over `rows` packed tokens, each buffer rounded up to 256 bytes, in this order: x, x1 (rows, d) fp32;
// h (rows, d) fp32 | bf16; qkv (rows, 3 d) fp32; ao (rows, d) fp32 | bf16; proj (rows, d) fp32; pre (rows, inner) fp32; act (rows, inner)
// fp32 | bf16  (bf16 in precision 1: the images the bf16-in-memory GEMMs read)
size_t immtsf_note_embed_workspace_bytes(int64_t rows, int32_t d, int32_t inner, int32_t precision) {
    if (rows <= 0 || d <= 0 || inner <= 0) return 0;
    const size_t r = (size_t)rows, op = precision == 1 ? 2 : 4;
    return 2 * up256(r * d * 4) + up256(r * d * op) + up256(r * 3 * d * 4) + up256(r * d * op) + up256(r * d * 4) + up256(r * inner * 4) +
           up256(r * inner * op);
}

int immtsf_note_embed_tokens(const int32_t* ids, const int32_t* cu, int32_t N, int32_t rows, const float* wte, int32_t vocab, const float* wpe,
                             int32_t n_positions, int32_t d, float* out, immtsf_stream_t stream) {
    if (!ids || !cu || !wte || !wpe || !out || N <= 0 || rows <= 0 || vocab <= 0 || n_positions <= 0 || d <= 0) return IMMTSF_EINVAL;
    if ((d & 3) || !al16(wte) || !al16(wpe) || !al16(out)) return IMMTSF_EUNSUPPORTED;
    hipLaunchKernelGGL(note_tokens_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), ids, cu, N, rows, wte,
                       vocab, wpe, n_positions, d, out);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_note_embed_attention(const float* qkv, int32_t ld, const int32_t* cu, int32_t N, int32_t rows, int32_t H, int32_t max_len,
                                float scale, int32_t precision, float* out32, void* out16, immtsf_stream_t stream) {
    return launch_attention<true>(qkv, ld, cu, N, rows, H, max_len, scale, precision, out32, out16, stream);
}

// the same launch without the causal bound (csrc/bert_embed.hip has the rest of the BERT body)
int immtsf_bert_embed_attention(const float* qkv, int32_t ld, const int32_t* cu, int32_t N, int32_t rows, int32_t H, int32_t max_len,
                                float scale, int32_t precision, float* out32, void* out16, immtsf_stream_t stream) {
    return launch_attention<false>(qkv, ld, cu, N, rows, H, max_len, scale, precision, out32, out16, stream);
}

int immtsf_note_embed_pool(const float* x, const int32_t* cu, int32_t N, int32_t rows, int32_t d, const float* gamma, const float* beta,
                           float eps, float* pooled, immtsf_stream_t stream) {
    if (!cu || !gamma || !beta || !pooled || N <= 0 || rows < 0 || d <= 0 || (rows > 0 && !x)) return IMMTSF_EINVAL;
    hipLaunchKernelGGL(note_pool_kernel, dim3((unsigned)N), dim3(256), 0, static_cast<hipStream_t>(stream), x, cu, rows, d, gamma, beta, eps,
                       pooled);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
