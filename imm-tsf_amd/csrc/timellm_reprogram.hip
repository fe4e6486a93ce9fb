// TimeLLM's word prototypes in folded form (reference models/TimeLLM.py:256-257 with :44-47, here models/TimeLLM.py forecasting() and
// ReprogrammingLayer): the keys and values key/value_projection(mapping_layer(E^T)^T) regrouped so that the (S, d_llm) table of mapped
// words is never formed.  D2 = 2 D, Wkv = [Wk; Wv] (D2, d_llm), G = [dk | dv] (S, D2):
//
//   forward    P = E Wkv^T                        (V, D2)   tr_p_kernel      a tile of 64 rows of E per workgroup
//              part[sp] = W_map[:, sp] P[sp]      (S, D2)   tr_fwd_kernel    64 rows x one slice of V per workgroup; + 1 workgroup: r
//              [k|v] = sum_sp part + b (x) r + c            tr_fwd_reduce    the slices in order
//   backward   dW_map[:, slab] = G P[slab]^T                tr_bwd_kernel    a slab of 64 columns per workgroup, all S rows:
//              dP[slab] = W_map[:, slab]^T G                                 W_map read once, both products from the same registers
//              part2[sp] = dP[sp]^T E[sp]         (D2, d)   tr_dwkv_kernel   128 columns x one slice of V per workgroup; further
//                                                                            workgroups: colsum(G), colsum(G b), G r
//              dWkv = sum_sp part2 + t 1^T                  tr_dwkv_reduce   the slices in order
//
// Every product runs on the matrix cores, a wave per 16 x 16 (x NT) output tile and 32 reduction indices per step: in fp32 mode eight
// v_mfma_f32_16x16x4_f32, in bf16 mode one v_mfma_f32_16x16x32_bf16 over operands rounded in registers.  A lane (i = lane % 16,
// q = lane / 16) holds eight reduction indices of row / column i; WHICH eight is free as long as both operands agree, so an operand
// that is contiguous along the reduction index takes k = 8 q + j (two 16-byte loads; E, Wkv, P and G rows) and one that is strided along
// it, or whose rows have no alignment (W_map: V is odd for GPT-2), takes k = q + 4 j (a dword per load, 16-byte runs per row).
// Loads past an edge read a clamped address and select zero, so no load hangs on a branch.
// No atomics: every output word has one writer and every sum a fixed order, so two runs give the same bits.
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

constexpr int TR_THREADS = 256;      // 4 waves
constexpr int TR_MAX_D2 = 128;

template <bool BF> struct Frag;
template <> struct Frag<false> {
    float v[8];
    __device__ __forceinline__ void set(int j, float x) { v[j] = x; }
};
template <> struct Frag<true> {
    bf16x8 v;
    __device__ __forceinline__ void set(int j, float x) { v[j] = (bf16_t)x; }
};

// c[4 q' + i][n] += sum over (q, j) of a(lane (m, q))[j] b(lane (q, n))[j]
__device__ __forceinline__ void mma(const Frag<false>& a, const Frag<false>& b, f32x4& c) {
#pragma unroll
    for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[j], b.v[j], c, 0, 0, 0);
}
__device__ __forceinline__ void mma(const Frag<true>& a, const Frag<true>& b, f32x4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, c, 0, 0, 0);
}

// eight consecutive floats at p (16-byte aligned), or zeros
template <bool BF> __device__ __forceinline__ void load8(Frag<BF>& f, const float* __restrict__ p, bool ok) {
    const f32x4 lo = reinterpret_cast<const f32x4*>(p)[0], hi = reinterpret_cast<const f32x4*>(p)[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f.set(j, ok ? lo[j] : 0.f);
        f.set(4 + j, ok ? hi[j] : 0.f);
    }
}

// row j of [Wk; Wv] / element (s, j) of [dk | dv]
__device__ __forceinline__ const float* kv_row(const float* __restrict__ a, const float* __restrict__ b, int D, size_t ld, int j) {
    return j < D ? a + (size_t)j * ld : b + (size_t)(j - D) * ld;
}

// ---- P = E Wkv^T: grid (ceil(V / 64)); a wave per 16 rows of E, all D2 columns -----------------------------------------------------
template <bool BF, int NT>
__global__ __launch_bounds__(TR_THREADS) void tr_p_kernel(long V, int d, int D, const float* __restrict__ E32, const bf16_t* __restrict__ E16,
                                                          const float* __restrict__ Wk, const float* __restrict__ Wv, float* __restrict__ P) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const long row0 = (long)blockIdx.x * 64 + w * 16;
    const long row = min(row0 + i, V - 1);
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < d; kc += 32) {
        const bool ok = kc + 8 * q < d;                  // d % 8 == 0: a lane's eight are all inside or all outside
        const int k0 = ok ? kc + 8 * q : 0;
        Frag<BF> a;
        if constexpr (BF) {
            const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            const bf16x8 t = *reinterpret_cast<const bf16x8*>(E16 + (size_t)row * d + k0);
            a.v = ok ? t : z;
        } else {
            load8<BF>(a, E32 + (size_t)row * d + k0, ok);
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            Frag<BF> b;
            load8<BF>(b, kv_row(Wk, Wv, D, d, n * 16 + i) + k0, ok);
            mma(a, b, acc[n]);
        }
    }
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long r = row0 + 4 * q + e;
            if (r < V) P[(size_t)r * (NT * 16) + n * 16 + i] = acc[n][e];
        }
}

// ---- part[sp] = W_map[:, slice sp] P[slice sp]: grid (row_tiles * nsplit + 1); a wave per 16 rows of W_map; the last workgroup sums r
template <bool BF, int NT>
__global__ __launch_bounds__(TR_THREADS) void tr_fwd_kernel(long S, long V, long slice, int nsplit, int main_blocks, const float* __restrict__ W,
                                                            const float* __restrict__ P, float* __restrict__ part, int d, int D,
                                                            const float* __restrict__ Wk, const float* __restrict__ Wv,
                                                            float* __restrict__ rvec) {
    constexpr int D2 = NT * 16;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    if ((int)blockIdx.x == main_blocks) {      // r[j] = sum_e Wkv[j][e]: a wave per row, lanes strided, one fixed tree
        for (int j = w; j < D2; j += TR_THREADS / 64) {
            const float* wr = kv_row(Wk, Wv, D, d, j);
            float s = 0.f;
            for (int e = lane; e < d; e += 64) s += wr[e];
            s = wave_sum(s);
            if (lane == 0) rvec[j] = s;
        }
        return;
    }
    const int tile = blockIdx.x / nsplit, sp = blockIdx.x - tile * nsplit;
    const long row0 = (long)tile * 64 + w * 16;
    const bool rok = row0 + i < S;
    const float* wrow = W + (size_t)min(row0 + i, S - 1) * V;
    const long v0 = sp * slice, v1 = min(V, v0 + slice);
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (long vc = v0; vc < v1; vc += 32) {
        Frag<BF> a;
        long kk[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long k = vc + q + 4 * j;
            kk[j] = min(k, v1 - 1);
            const float x = wrow[kk[j]];
            a.set(j, rok && k < v1 ? x : 0.f);
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            Frag<BF> b;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = P[(size_t)kk[j] * D2 + n * 16 + i];
                b.set(j, vc + q + 4 * j < v1 ? x : 0.f);
            }
            mma(a, b, acc[n]);
        }
    }
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long r = row0 + 4 * q + e;
            if (r < S) part[((size_t)sp * S + r) * D2 + n * 16 + i] = acc[n][e];
        }
}

// ---- [k|v][s][j] = sum_sp part[sp][s][j] + b_map[s] r[j] + [bk|bv][j]: a thread per element ----------------------------------------
__global__ __launch_bounds__(TR_THREADS) void tr_fwd_reduce(long S, int D, int nsplit, const float* __restrict__ part, const float* __restrict__ b_map,
                                                            const float* __restrict__ rvec, const float* __restrict__ bk,
                                                            const float* __restrict__ bv, float* __restrict__ k, float* __restrict__ v) {
    const int D2 = 2 * D;
    const size_t n = (size_t)S * D2, e = (size_t)blockIdx.x * TR_THREADS + threadIdx.x;
    if (e >= n) return;
    const long s = (long)(e / D2);
    const int j = (int)(e - (size_t)s * D2);
    float a = 0.f;
    for (int sp = 0; sp < nsplit; ++sp) a += part[(size_t)sp * n + e];
    a += b_map[s] * rvec[j] + (j < D ? bk[j] : bv[j - D]);
    if (j < D) k[(size_t)s * D + j] = a;
    else v[(size_t)s * D + j - D] = a;
}

// ---- one pass over W_map: grid (ceil(V / 64)); a wave owns 16 columns and walks all S rows, 32 at a step ------------------------------
//   dP[cols][j]       += sum_s W_map[s][cols] G[s][j]     rows = the wave's columns, reduction over the step's 32 rows (k = q + 4 j)
//   dW_map[s][cols]    = sum_j G[s][j] P[cols][j]         two tiles of 16 rows, reduction over D2 (k = 8 q + j), P[cols] kept in registers
template <bool BF, int NT>
__global__ __launch_bounds__(TR_THREADS) void tr_bwd_kernel(long S, long V, int D, const float* __restrict__ W, const float* __restrict__ P,
                                                            const float* __restrict__ dk, const float* __restrict__ dv, float* __restrict__ dW,
                                                            float* __restrict__ dP) {
    constexpr int D2 = NT * 16, KC = (NT + 1) / 2;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const long col0 = (long)blockIdx.x * 64 + w * 16;
    const long col = col0 + i;
    const bool cok = col < V;
    const long colc = min(col, V - 1);
    Frag<BF> pf[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        const bool ok = c * 32 + 8 * q < D2;
        load8<BF>(pf[c], P + (size_t)colc * D2 + (ok ? c * 32 + 8 * q : 0), ok);
    }
    f32x4 dpa[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) dpa[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (long s0 = 0; s0 < S; s0 += 32) {
        Frag<BF> a;
        long ss[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long s = s0 + q + 4 * j;
            ss[j] = min(s, S - 1);
            const float x = W[(size_t)ss[j] * V + colc];
            a.set(j, s < S && cok ? x : 0.f);
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            Frag<BF> b;
            const int jc = n * 16 + i;
            const float* g = jc < D ? dk + jc : dv + (jc - D);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = g[(size_t)ss[j] * D];
                b.set(j, s0 + q + 4 * j < S ? x : 0.f);
            }
            mma(a, b, dpa[n]);
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const long s = s0 + m * 16 + i;
            const long sc = min(s, S - 1);
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
                const int j0 = kc * 32 + 8 * q;            // D % 8 == 0: the eight lie in dk or in dv, inside D2 or outside
                const bool ok = j0 < D2 && s < S;
                const int jc = j0 < D2 ? j0 : 0;
                Frag<BF> ga;
                load8<BF>(ga, (jc < D ? dk + jc : dv + (jc - D)) + (size_t)sc * D, ok);
                mma(ga, pf[kc], c);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long r = s0 + m * 16 + 4 * q + e;
                if (r < S && cok) dW[(size_t)r * V + col] = c[e];
            }
        }
    }
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long r = col0 + 4 * q + e;
            if (r < V) dP[(size_t)r * D2 + n * 16 + i] = dpa[n][e];
        }
}

// ---- part2[sp] = dP[slice sp]^T E[slice sp]: grid (col_blocks * nsplit + 1 + ceil(S / 256)); a wave per 32 columns of E, all D2 rows.
// Workgroup main_blocks: t[j] = sum_s G[s][j] b_map[s] and d[bk|bv][j] = sum_s G[s][j]; the ones behind it: db_map[s] = sum_j G[s][j] r[j]
template <bool BF, int NT, typename ET>
__global__ __launch_bounds__(TR_THREADS) void tr_dwkv_kernel(long S, long V, int d, int D, long slice, int nsplit, int main_blocks,
                                                             const float* __restrict__ dP, const ET* __restrict__ E, float* __restrict__ part2,
                                                             const float* __restrict__ dk, const float* __restrict__ dv,
                                                             const float* __restrict__ b_map, const float* __restrict__ rvec,
                                                             float* __restrict__ tvec, float* __restrict__ dbk, float* __restrict__ dbv,
                                                             float* __restrict__ db_map) {
    constexpr int D2 = NT * 16;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    if ((int)blockIdx.x == main_blocks) {
        for (int j = w; j < D2; j += TR_THREADS / 64) {
            const float* g = j < D ? dk + j : dv + (j - D);
            float c = 0.f, t = 0.f;
            for (long s = lane; s < S; s += 64) {
                const float x = g[(size_t)s * D];
                c += x;
                t = fmaf(x, b_map[s], t);
            }
            c = wave_sum(c);
            t = wave_sum(t);
            if (lane == 0) {
                tvec[j] = t;
                if (j < D) dbk[j] = c;
                else dbv[j - D] = c;
            }
        }
        return;
    }
    if ((int)blockIdx.x > main_blocks) {
        const long s = (long)(blockIdx.x - main_blocks - 1) * TR_THREADS + threadIdx.x;
        if (s < S) {
            float a = 0.f;
            for (int j = 0; j < D; ++j) a = fmaf(dk[(size_t)s * D + j], rvec[j], a);
            for (int j = 0; j < D; ++j) a = fmaf(dv[(size_t)s * D + j], rvec[D + j], a);
            db_map[s] = a;
        }
        return;
    }
    const int cb = blockIdx.x / nsplit, sp = blockIdx.x - cb * nsplit;
    const int e0 = cb * 128 + w * 32;
    const long v0 = sp * slice, v1 = min(V, v0 + slice);
    f32x4 acc[NT][2];
#pragma unroll
    for (int m = 0; m < NT; ++m) acc[m][0] = acc[m][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (long vc = v0; vc < v1; vc += 32) {
        long kk[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) kk[j] = min(vc + q + 4 * j, v1 - 1);
        Frag<BF> b[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int e = e0 + t * 16 + i;
            const int ec = min(e, d - 1);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = (float)E[(size_t)kk[j] * d + ec];
                b[t].set(j, vc + q + 4 * j < v1 && e < d ? x : 0.f);
            }
        }
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            Frag<BF> a;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = dP[(size_t)kk[j] * D2 + m * 16 + i];
                a.set(j, vc + q + 4 * j < v1 ? x : 0.f);
            }
            mma(a, b[0], acc[m][0]);
            mma(a, b[1], acc[m][1]);
        }
    }
#pragma unroll
    for (int m = 0; m < NT; ++m)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int col = e0 + t * 16 + i;
                if (col < d) part2[((size_t)sp * D2 + m * 16 + 4 * q + e) * d + col] = acc[m][t][e];
            }
}

// ---- d[Wk; Wv][j][e] = sum_sp part2[sp][j][e] + t[j]: a thread per element ----------------------------------------------------------
__global__ __launch_bounds__(TR_THREADS) void tr_dwkv_reduce(int d, int D, int nsplit, const float* __restrict__ part2, const float* __restrict__ tvec,
                                                             float* __restrict__ dWk, float* __restrict__ dWv) {
    const size_t n = (size_t)2 * D * d, e = (size_t)blockIdx.x * TR_THREADS + threadIdx.x;
    if (e >= n) return;
    const int j = (int)(e / d);
    float a = 0.f;
    for (int sp = 0; sp < nsplit; ++sp) a += part2[(size_t)sp * n + e];
    a += tvec[j];
    if (j < D) dWk[e] = a;
    else dWv[e - (size_t)D * d] = a;
}

// ---- the split of V, shared by the scratch query and the launches ------------------------------------------------------------------
struct TrPlan {
    int row_tiles, nsplit_f, col_blocks, nsplit_b;
    long slice_f, slice_b;
    size_t part_off, dp_off, part2_off, t_off, fwd_bytes, bwd_bytes;
};

inline size_t tr_up(size_t n) { return (n + 255) & ~(size_t)255; }

inline void tr_split(long V, long want, long min_chunks, int& nsplit, long& slice) {
    const long chunks = (V + 31) / 32;                                  // steps of 32 reduction indices
    long n = chunks / min_chunks < want ? chunks / min_chunks : want;
    if (n < 1) n = 1;
    slice = (chunks + n - 1) / n * 32;
    nsplit = (int)((V + slice - 1) / slice);                           // no empty slice
}

inline TrPlan tr_plan(long S, long V, int d, int D) {
    TrPlan p;
    const size_t D2 = 2 * (size_t)D;
    p.row_tiles = (int)((S + 63) / 64);
    tr_split(V, (1024 + p.row_tiles - 1) / p.row_tiles, 8, p.nsplit_f, p.slice_f);          // about four workgroups per CU
    p.col_blocks = (d + 127) / 128;
    tr_split(V, (512 + p.col_blocks - 1) / p.col_blocks, 4, p.nsplit_b, p.slice_b);
    p.part_off = 0;
    p.fwd_bytes = tr_up(sizeof(float) * (size_t)p.nsplit_f * S * D2);
    p.dp_off = 0;
    p.part2_off = tr_up(sizeof(float) * (size_t)V * D2);
    p.t_off = p.part2_off + tr_up(sizeof(float) * (size_t)p.nsplit_b * D2 * d);
    p.bwd_bytes = p.t_off + tr_up(sizeof(float) * D2);
    return p;
}

inline bool tr_aligned(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

#define TR_NT_SWITCH(NT, ...)                              \
    switch (NT) {                                          \
        case 1: { constexpr int NT_ = 1; __VA_ARGS__; } break; \
        case 2: { constexpr int NT_ = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int NT_ = 3; __VA_ARGS__; } break; \
        case 4: { constexpr int NT_ = 4; __VA_ARGS__; } break; \
        case 5: { constexpr int NT_ = 5; __VA_ARGS__; } break; \
        case 6: { constexpr int NT_ = 6; __VA_ARGS__; } break; \
        case 7: { constexpr int NT_ = 7; __VA_ARGS__; } break; \
        default: { constexpr int NT_ = 8; __VA_ARGS__; } break; \
    }

}  // namespace

extern "C" {

int immtsf_timellm_prototypes_supported(int64_t S, int64_t V, int32_t d_llm, int32_t D) {
    const int64_t lim = (int64_t)1 << 31;
    return S >= 1 && V >= 1 && S < lim && V < lim && d_llm >= 8 && d_llm % 8 == 0 && D >= 8 && 2 * D <= TR_MAX_D2 && (2 * D) % 16 == 0 &&
                   (V + 63) / 64 < lim ? 1 : 0;
}

size_t immtsf_timellm_prototypes_scratch_bytes(int64_t S, int64_t V, int32_t d_llm, int32_t D, int32_t backward) {
    if (!immtsf_timellm_prototypes_supported(S, V, d_llm, D)) return 0;
    const TrPlan p = tr_plan(S, V, d_llm, D);
    return backward ? p.bwd_bytes : p.fwd_bytes;
}

int immtsf_timellm_prototypes_forward(int32_t precision, const float* E, const void* E16, const float* W_map, const float* b_map,
                                      const float* Wk, const float* bk, const float* Wv, const float* bv, int64_t S, int64_t V,
                                      int32_t d_llm, int32_t D, float* P, float* r, float* k, float* v, void* scratch,
                                      size_t scratch_bytes, immtsf_stream_t stream) {
    if (precision != 0 && precision != 1) return IMMTSF_EINVAL;
    if (!immtsf_timellm_prototypes_supported(S, V, d_llm, D)) return IMMTSF_EUNSUPPORTED;
    if (!tr_aligned(E) || (precision == 1 && !tr_aligned(E16)) || !tr_aligned(W_map) || !tr_aligned(b_map) || !tr_aligned(Wk) ||
        !tr_aligned(Wv) || !bk || !bv || !tr_aligned(P) || !r || !k || !v || !tr_aligned(scratch))
        return IMMTSF_EINVAL;
    const TrPlan p = tr_plan(S, V, d_llm, D);
    if (scratch_bytes < p.fwd_bytes) return IMMTSF_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* part = reinterpret_cast<float*>(static_cast<char*>(scratch) + p.part_off);
    const int NT = 2 * D / 16, main_blocks = p.row_tiles * p.nsplit_f;
    const bf16_t* e16 = static_cast<const bf16_t*>(E16);
    const unsigned pgrid = (unsigned)((V + 63) / 64);
    TR_NT_SWITCH(NT, {
        if (precision == 1) {
            hipLaunchKernelGGL((tr_p_kernel<true, NT_>), dim3(pgrid), dim3(TR_THREADS), 0, st, (long)V, d_llm, D, E, e16, Wk, Wv, P);
            hipLaunchKernelGGL((tr_fwd_kernel<true, NT_>), dim3(main_blocks + 1), dim3(TR_THREADS), 0, st, (long)S, (long)V, p.slice_f,
                               p.nsplit_f, main_blocks, W_map, P, part, d_llm, D, Wk, Wv, r);
        } else {
            hipLaunchKernelGGL((tr_p_kernel<false, NT_>), dim3(pgrid), dim3(TR_THREADS), 0, st, (long)V, d_llm, D, E, e16, Wk, Wv, P);
            hipLaunchKernelGGL((tr_fwd_kernel<false, NT_>), dim3(main_blocks + 1), dim3(TR_THREADS), 0, st, (long)S, (long)V, p.slice_f,
                               p.nsplit_f, main_blocks, W_map, P, part, d_llm, D, Wk, Wv, r);
        }
    })
    IMMTSF_LAUNCH_CHECK();
    const size_t n = (size_t)S * 2 * D;
    hipLaunchKernelGGL(tr_fwd_reduce, dim3((unsigned)((n + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, st, (long)S, D, p.nsplit_f,
                       part, b_map, r, bk, bv, k, v);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_timellm_prototypes_backward(int32_t precision, const float* E, const void* E16, const float* W_map, const float* b_map,
                                       const float* P, const float* r, const float* dk, const float* dv, int64_t S, int64_t V,
                                       int32_t d_llm, int32_t D, float* dW_map, float* db_map, float* dWk, float* dbk, float* dWv,
                                       float* dbv, void* scratch, size_t scratch_bytes, immtsf_stream_t stream) {
    if (precision != 0 && precision != 1) return IMMTSF_EINVAL;
    if (!immtsf_timellm_prototypes_supported(S, V, d_llm, D)) return IMMTSF_EUNSUPPORTED;
    if (!tr_aligned(E) || (precision == 1 && !tr_aligned(E16)) || !tr_aligned(W_map) || !b_map || !tr_aligned(P) || !r || !tr_aligned(dk) ||
        !tr_aligned(dv) || !dW_map || !db_map || !dWk || !dbk || !dWv || !dbv || !tr_aligned(scratch))
        return IMMTSF_EINVAL;
    const TrPlan p = tr_plan(S, V, d_llm, D);
    if (scratch_bytes < p.bwd_bytes) return IMMTSF_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(scratch);
    float* dP = reinterpret_cast<float*>(base + p.dp_off);
    float* part2 = reinterpret_cast<float*>(base + p.part2_off);
    float* tvec = reinterpret_cast<float*>(base + p.t_off);
    const int NT = 2 * D / 16, main_blocks = p.col_blocks * p.nsplit_b;
    const unsigned grid2 = (unsigned)(main_blocks + 1 + (S + TR_THREADS - 1) / TR_THREADS);
    const bf16_t* e16 = static_cast<const bf16_t*>(E16);
    TR_NT_SWITCH(NT, {
        if (precision == 1) {
            hipLaunchKernelGGL((tr_bwd_kernel<true, NT_>), dim3((unsigned)((V + 63) / 64)), dim3(TR_THREADS), 0, st, (long)S, (long)V, D, W_map,
                               P, dk, dv, dW_map, dP);
            hipLaunchKernelGGL((tr_dwkv_kernel<true, NT_, bf16_t>), dim3(grid2), dim3(TR_THREADS), 0, st, (long)S, (long)V, d_llm, D, p.slice_b,
                               p.nsplit_b, main_blocks, dP, e16, part2, dk, dv, b_map, r, tvec, dbk, dbv, db_map);
        } else {
            hipLaunchKernelGGL((tr_bwd_kernel<false, NT_>), dim3((unsigned)((V + 63) / 64)), dim3(TR_THREADS), 0, st, (long)S, (long)V, D, W_map,
                               P, dk, dv, dW_map, dP);
            hipLaunchKernelGGL((tr_dwkv_kernel<false, NT_, float>), dim3(grid2), dim3(TR_THREADS), 0, st, (long)S, (long)V, d_llm, D, p.slice_b,
                               p.nsplit_b, main_blocks, dP, E, part2, dk, dv, b_map, r, tvec, dbk, dbv, db_map);
        }
    })
    IMMTSF_LAUNCH_CHECK();
    const size_t n = (size_t)2 * D * d_llm;
    hipLaunchKernelGGL(tr_dwkv_reduce, dim3((unsigned)((n + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, st, d_llm, D, p.nsplit_b, part2,
                       tvec, dWk, dWv);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
