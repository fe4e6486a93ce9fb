// Causal attention forward at head_dim 128 with grouped K/V heads (H query heads over H_kv K/V heads, G = H / H_kv): the fp32 VALU kernel
// and the bf16 MFMA kernel that the Llama note embedder (llama_embed.hip, ragged notes) and TimeLLM's Llama body (llama_body.hip, dense
// sequences with a query offset and the log-sum-exp) share.  No dropout, no atomics, one writer per output element, every sum in a fixed
// order.
//
// Launch: grid (sequence, K/V head, query tile of 32 REVERSED), a workgroup of G waves, one per query head of the K/V head; the waves fill
// the K / V tiles of 32 keys in LDS together and each reads them for its own head.  Workgroups are handed out in x, y, z order, so the
// last query tiles of the long sequences -- the ones with the most keys -- start first and the short tiles fill in behind them; a tile
// with no live query leaves at once (the whole workgroup: the test does not depend on the wave).  A query tile is the 32 absolute
// positions t0 .. t0 + 31, aligned like the key tiles; a position below the first query or at / past the end is idle: it repeats a live
// query and writes nothing.  The tile is 32 and not the 64 of note_embed.hip: at head_dim 128 a wave's 64 queries need q + the output in
// 256 + registers and the G = 8 workgroup (512 threads) leaves a wave 256 in all; with 32 no instance spills.
//
// `Rows` says where a workgroup's rows lie.  rows.tile(H) turns blockIdx into a struct with
//   empty        the tile holds no live query
//   t0, from, S  the tile's first position (>= 0), the first query position and the sequence length
//   q, ldq       position p of query head h is the row q + (row0 + p - from) ldq + 128 h; row0 + p - from is also its output row
//   k, v, ldkv   key j of the workgroup's K/V head is the row k + j ldkv, resp. v + j ldkv
//   lse          the log-sum-exp of (output row r, head h) goes to lse[r H + h]; NULL: not stored
// A policy whose `from` and `lse` are compile-time constants (ragged notes: 0 and NULL) pays nothing for the other's generality.
#pragma once
#include "common.hpp"

namespace gqa128 {

constexpr int HD = 128;       // head_dim
constexpr int QT = 32;        // queries per wave (= per query head of a workgroup)
constexpr int KT = 32;        // keys per LDS tile
constexpr int KC = 4;         // keys per softmax chunk of the VALU form
constexpr int KS_LD = HD + 8; // bf16 K tile [key][e]: 272-byte rows (16-byte fragments)
constexpr int VT_LD = KT + 8; // bf16 V tile transposed [e][key]: 80-byte rows (8-byte fragments)

// ---- fp32 on the VALU ---------------------------------------------------------------------------------------------------------------------
// wave w of the workgroup is query head G kvh + w.  TWO lanes own one query: lane 2 q + hf holds head columns 64 hf .. 64 hf + 63 of q
// and of the output row (64 + 64 registers), the halves of a score meet through one DPP exchange with lane ^ 1, and both lanes carry
// the same softmax state.  K / V tiles of KT keys go through LDS as broadcasts (two addresses per read).
template <int G, class Rows>
__global__ void __launch_bounds__(64 * G) attn_valu_kernel(Rows rows, int H, float scale, float* __restrict__ o32, bf16_t* __restrict__ o16) {
    __shared__ float4 Ks[KT * HD / 4];
    __shared__ float4 Vs[KT * HD / 4];
    const int tid = threadIdx.x, lane = tid & 63, qi = lane >> 1, hf = lane & 1;
    const int h = blockIdx.y * G + (tid >> 6);
    const auto w = rows.tile(H);
    if (w.empty) return;
    __builtin_assume(w.t0 >= 0);
    const int t0 = w.t0, S = w.S, dq = H * HD;
    const int pn = t0 + qi;                                  // the nominal position: what the causal bound reads
    const bool live = pn >= w.from && pn < S;
    const int pc = pn < w.from ? w.from : pn >= S ? S - 1 : pn;
    const size_t qrow = w.row0 + (pc - w.from);
    float qr[HD / 2], acc[HD / 2];
    {
        const float4* qp = reinterpret_cast<const float4*>(w.q + qrow * w.ldq + h * HD + (HD / 2) * hf);
#pragma unroll
        for (int e = 0; e < HD / 8; ++e) {
            const float4 x = qp[e];
            qr[4 * e] = x.x * scale; qr[4 * e + 1] = x.y * scale; qr[4 * e + 2] = x.z * scale; qr[4 * e + 3] = x.w * scale;
        }
    }
#pragma unroll
    for (int e = 0; e < HD / 2; ++e) acc[e] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int kend = min(t0 + QT, S);                       // keys 0 .. kend-1 are visible to some query of the workgroup
    for (int j0 = 0; j0 < kend; j0 += KT) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KT * HD / 4 / (64 * G); ++i) {
            const int idx = tid + 64 * G * i, kk = idx >> 5, part = idx & 31, j = j0 + kk;
            float4 a = {0.f, 0.f, 0.f, 0.f}, c = a;
            if (j < kend) {
                a = reinterpret_cast<const float4*>(w.k + (size_t)j * w.ldkv)[part];
                c = reinterpret_cast<const float4*>(w.v + (size_t)j * w.ldkv)[part];
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
                sc[c] = (j0 + c4 + c <= pn) ? a : -INFINITY;
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
    const size_t orow = qrow * dq + h * HD + (HD / 2) * hf;
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
    if (w.lse && hf == 0) w.lse[qrow * H + h] = m + __logf(l);
}

// ---- bf16 MFMA ----------------------------------------------------------------------------------------------------------------------------
// The transposed form of note_embed.hip widened to head_dim 128.  Wave w owns 32 queries of head G kvh + w as two 16-query column tiles.
// mfma_f32_16x16x32_bf16, lane l: fr = l & 15, g = l >> 4; A[row fr][k = 8 g + j], B[k = 8 g + j][col fr], C[row 4 g + i][col fr]:
//   S^T (keys x queries) = K (A: a key row from the LDS tile, k = head column, FOUR k-steps) . Q^T (B: a query row from global memory,
//   held for the whole key loop).  A lane holds, for ITS query fr, the scores of keys 4 g + i of each 16-key subtile: the row maximum
//   and sum are an in-register reduction plus two cross-row steps (lanes fr, fr + 16, fr + 32, fr + 48), all fp32.
//   O^T (head columns x queries) += V^T (A) . P^T (B), EIGHT 16-column output tiles.  The B fragment of lane (fr, g) is k-slot j -> key
//   4 g + j (j < 4) or 16 + 4 g + (j - 4): exactly the eight probabilities the lane already holds, rounded to bf16.  The A fragment takes
//   V in the same k order: row e = 16 et + fr of the transposed V tile, keys 4 g .. 4 g + 3 and 16 + 4 g .. 16 + 4 g + 3.
// Query tile and key tile are both 32 and aligned to absolute positions, so every key tile of the loop starts at or below every query of
// the workgroup: no 16-query tile is ever skipped, and the running maximum is finite from the first tile on (key j0 is visible to each
// query).
__device__ __forceinline__ f32x4 mfma_bf16(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

template <int G, class Rows>
__global__ void __launch_bounds__(64 * G) attn_mfma_kernel(Rows rows, int H, float scale, float* __restrict__ o32, bf16_t* __restrict__ o16) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[KT * KS_LD];
    __shared__ __attribute__((aligned(16))) bf16_t Vt[HD * VT_LD];
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, g = lane >> 4;
    const int h = blockIdx.y * G + (tid >> 6);
    const auto w = rows.tile(H);
    if (w.empty) return;
    __builtin_assume(w.t0 >= 0);
    const int t0 = w.t0, S = w.S, dq = H * HD;
    bf16x8 qf[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int pn = t0 + 16 * mt + fr;
        const int pc = pn < w.from ? w.from : pn >= S ? S - 1 : pn;      // an idle query repeats a live one and is not written
        const float4* qp = reinterpret_cast<const float4*>(w.q + (w.row0 + (pc - w.from)) * w.ldq + h * HD);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const float4 a = qp[8 * ks + 2 * g], c = qp[8 * ks + 2 * g + 1];
            qf[mt][ks] = bf16x8{(bf16_t)a.x, (bf16_t)a.y, (bf16_t)a.z, (bf16_t)a.w, (bf16_t)c.x, (bf16_t)c.y, (bf16_t)c.z, (bf16_t)c.w};
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
    const int kend = min(t0 + QT, S);
    for (int j0 = 0; j0 < kend; j0 += KT) {
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < KT * HD / 4 / (64 * G); ++i) {
            const int idx = tid + 64 * G * i, kk = idx >> 5, part = idx & 31, j = j0 + kk;
            float4 a = {0.f, 0.f, 0.f, 0.f}, c = a;
            if (j < kend) {
                a = reinterpret_cast<const float4*>(w.k + (size_t)j * w.ldkv)[part];
                c = reinterpret_cast<const float4*>(w.v + (size_t)j * w.ldkv)[part];
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
            const int qi = t0 + 16 * mt + fr;               // the last key this lane's query sees (>= j0: the tiles are aligned)
            float s[2][4];
            float cmax = -INFINITY;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                f32x4 Sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) Sc = mfma_bf16(kf[nt][ks], qf[mt][ks], Sc);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    s[nt][i] = (j0 + 16 * nt + 4 * g + i <= qi) ? Sc[i] * scale : -INFINITY;
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
                O[mt][et] = mfma_bf16(vf[et], pf, o);
            }
        }
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const float l = xor32_sum(xor16_sum(ls[mt]));        // shares of lanes fr, fr + 16, fr + 32, fr + 48 in one fixed order
        const int pn = t0 + 16 * mt + fr;
        if (pn < w.from || pn >= S) continue;
        const float inv = 1.f / l;
        const size_t qrow = w.row0 + (pn - w.from);
        const size_t orow = qrow * dq + h * HD + 4 * g;
#pragma unroll
        for (int et = 0; et < 8; ++et) {
            const f32x4 o = O[mt][et];
            if (o32) *reinterpret_cast<float4*>(o32 + orow + 16 * et) = float4{o[0] * inv, o[1] * inv, o[2] * inv, o[3] * inv};
            if (o16)
                *reinterpret_cast<bf16x4*>(o16 + orow + 16 * et) =
                    bf16x4{(bf16_t)(o[0] * inv), (bf16_t)(o[1] * inv), (bf16_t)(o[2] * inv), (bf16_t)(o[3] * inv)};
        }
        if (w.lse && g == 0) w.lse[qrow * H + h] = m[mt] + __logf(l);
    }
}

}  // namespace gqa128
