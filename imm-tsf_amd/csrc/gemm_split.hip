// fp32-grade products of a frozen weight on the bf16 MFMA: C (M, N; pitch ldc) = op(A) op(B) + bias with A fp32 in HBM and B
// given as TWO bf16 images of the same shape and pitch, Bhi = bf16(B) and Blo = bf16(B - Bhi), made once per weight by
// immtsf_split_bf16.  A is cut the same way in registers while it is staged (a_hi = bf16(a), a_lo = bf16(a - a_hi); no image of A
// goes back to HBM), and every 16 x 16 x 32 step of an output fragment is three MFMAs in one fixed order,
//     acc += a_lo b_hi;  acc += a_hi b_lo;  acc += a_hi b_hi        (a_lo b_lo, <= 2^-18 relative, is dropped)
// with fp32 accumulation: 16 - 17 significant bits per operand at three bf16 MFMA passes per tile.  bf16 x bf16 is exact in fp32,
// so the only roundings are the two cuts and the fp32 sums.  No split-K, no atomics: one writer per output element and one
// summation order, so the same inputs give the same bits.
//
// Structure: the 64-deep K step and the LDS images of gemm2.hip.  The B images travel global -> LDS by LDS-DMA (lane-linear
// destination, every permutation in the per-lane SOURCE address): layout 0 (B (N, K), an nn.Linear weight as stored) as gemm2's R
// image read by ds_read_b128, layout 1 (B (K, N)) as its T image of 64-column blocks read by ds_read_b64_tr_b16.  A goes through
// registers (it has to be cut) into two R images.  Two LDS stages and ONE barrier per K step:
//     wait vmcnt(0); barrier        -- stage t has landed everywhere (the DMA and everybody's ds_writes), and everybody has left t-1
//     issue B DMA of t+1, load A of t+1 into registers
//     fragments + MFMAs of stage t
//     cut A of t+1 and ds_write it into the other stage
// A stage holds A hi | A lo | B hi | B lo: (BM + BN) * 256 bytes, twice gemm2's for the same tile.
// Out-of-range k chunks and T-image columns come from a 16-byte zero page (B) or are zero registers (A); out-of-range rows of an R
// image are clamped to the last row (their products only reach output elements that are never stored).
// immtsf_gemm_asplit: the same kernel for a weight that is STORED in bf16 (a Llama checkpoint read in place): B is the one image, bit for
// bit the weight, so there is no Blo (template flag LO off), a stage holds A hi | A lo | B, (2 BM + BN) * 128 bytes, and a step is two MFMAs,
//     acc += a_lo b;  acc += a_hi b
// in that order -- fp32-grade in A, exact in B.  Same tiles, same selection, same support set.
// Supported (immtsf_gemm_split_supported): layout 0 | 1, K and N multiples of 8, lda a multiple of 4, ldb a multiple of 8, pitches
// at least as long as their rows; pointers: A, Bhi, Blo 16-byte aligned.  Anything else returns IMMTSF_EUNSUPPORTED before a launch.
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

typedef __attribute__((address_space(3))) void* lds_vp;
typedef const __attribute__((address_space(1))) void* glb_vp;

__device__ __attribute__((aligned(16))) const unsigned int gs_zero_page[4] = {0u, 0u, 0u, 0u};

struct SplitArgs {
    const float* A;
    const bf16_t* Bhi;
    const bf16_t* Blo;
    float* C;
    const float* bias;
    int M, N, K, lda, ldb, ldc;
};

constexpr int SBK = 64;

template <bool TB, bool LO, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(WM* WN * 64) void gemm_split_kernel(const SplitArgs g) {
    constexpr int NT = WM * WN * 64;
    constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
    constexpr int CA = (BM * 8 + NT - 1) / NT, CB = BN * 8 / NT;      // 16-byte bf16 chunks per thread, stage and image
    static_assert((BN * 8) % NT == 0 && CB >= 1, "whole LDS-DMA pieces per wave");
    static_assert((BM / WM) % 16 == 0 && (BN / WN) % 16 == 0 && TM >= 1 && TN >= 1, "wave tile = whole 16x16 MFMA tiles");
    static_assert(BN % 64 == 0, "T images come in 64-column blocks");
    constexpr int A_IMG = BM * 128, B_IMG = BN * 128;                 // bytes of one image of one stage
    constexpr int SB = 2 * A_IMG + (LO ? 2 : 1) * B_IMG;           // LO: B comes as (hi, lo); else B is the weight itself, one image

    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * SB];

    const int M = g.M, N = g.N, K = g.K;
    const int tiles_n = (N + BN - 1) / BN;
    const int tile_m = blockIdx.x / tiles_n, tile_n = blockIdx.x - tile_m * tiles_n;
    const int row0 = tile_m * BM, col0 = tile_n * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm0 = (wave / WN) * (BM / WM), wn0 = (wave % WN) * (BN / WN);
    const bf16_t* zp = reinterpret_cast<const bf16_t*>(gs_zero_page);
    const int nk = (K + SBK - 1) / SBK;

    // ---- A: chunk p = (row p >> 3, k chunk p & 7) of the tile; eight fp32 a chunk
    const float* pa[CA];
    int ka[CA], la[CA];
#pragma unroll
    for (int i = 0; i < CA; ++i) {
        const int p = tid + i * NT, r = (p >> 3) % BM, c = p & 7;
        pa[i] = g.A + (size_t)min(row0 + r, M - 1) * g.lda + c * 8;
        ka[i] = (p < BM * 8) ? c * 8 : (1 << 30);
        la[i] = r * 128 + ((c ^ ((r >> 1) & 7)) << 4);
    }
    // ---- B: per-thread source offsets of its chunks at k = 0 (the same for both images)
    size_t ob[CB];
    int kb[CB];
#pragma unroll
    for (int i = 0; i < CB; ++i) {
        const int p = tid + i * NT;
        if (!TB) {
            const int r = p >> 3, c = (p & 7) ^ ((r >> 1) & 7);
            ob[i] = (size_t)min(col0 + r, N - 1) * g.ldb + c * 8;
            kb[i] = c * 8;
        } else {
            const int b = p >> 9, pk = p & 511, k = pk >> 3;
            const int n8 = (pk & 7) ^ ((((k >> 1) & 1) << 1) | (((k >> 3) & 1) << 2));
            const int col = col0 + b * 64 + n8 * 8;
            ob[i] = (size_t)k * g.ldb + col;
            kb[i] = (col + 8 <= N) ? k : (1 << 30);        // columns past N: always the zero page
        }
    }
    const size_t stepB = TB ? (size_t)SBK * g.ldb : (size_t)SBK;

    auto issue_b = [&](int t, int slot) {
        const int k0 = t * SBK;
        unsigned char* sb = smem + slot * SB + 2 * A_IMG + wave * 1024;
#pragma unroll
        for (int i = 0; i < CB; ++i) {
            const bool ok = k0 + kb[i] < K;
            const size_t o = ob[i] + (size_t)t * stepB;
            __builtin_amdgcn_global_load_lds((glb_vp)(ok ? g.Bhi + o : zp), (lds_vp)(sb + i * (NT * 16)), 16, 0, 0);
            if (LO) __builtin_amdgcn_global_load_lds((glb_vp)(ok ? g.Blo + o : zp), (lds_vp)(sb + B_IMG + i * (NT * 16)), 16, 0, 0);
        }
    };
    float4 ra[CA][2];
    auto load_a = [&](int t) {
        const int k0 = t * SBK;
#pragma unroll
        for (int i = 0; i < CA; ++i) {
            if (k0 + ka[i] < K) {
                const float4* s = reinterpret_cast<const float4*>(pa[i] + k0);
                ra[i][0] = s[0];
                ra[i][1] = s[1];
            } else {
                ra[i][0] = make_float4(0.f, 0.f, 0.f, 0.f);
                ra[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };
    auto store_a = [&](int slot) {
        unsigned char* sa = smem + slot * SB;
#pragma unroll
        for (int i = 0; i < CA; ++i) {
            if (CA * NT != BM * 8 && tid + i * NT >= BM * 8) continue;
            const float v[8] = {ra[i][0].x, ra[i][0].y, ra[i][0].z, ra[i][0].w, ra[i][1].x, ra[i][1].y, ra[i][1].z, ra[i][1].w};
            bf16x8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                hi[e] = (bf16_t)v[e];
                lo[e] = (bf16_t)(v[e] - (float)hi[e]);
            }
            *reinterpret_cast<bf16x8*>(sa + la[i]) = hi;
            *reinterpret_cast<bf16x8*>(sa + A_IMG + la[i]) = lo;
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // fragment byte offsets inside an image (gemm2.hip's maps): lane (fr, fq) holds row / column fr, k = 32 kk + 8 fq .. + 7
    const int fr = lane & 15, fq = lane >> 4;
    int offA[TM], offB[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) offA[i] = (wm0 + i * 16 + fr) * 128;
    if (!TB) {
#pragma unroll
        for (int j = 0; j < TN; ++j) offB[j] = (wn0 + j * 16 + fr) * 128;
    } else {
        const int q = fr >> 2, p = fr & 3, sw = ((q >> 1) << 1) | ((fq & 1) << 2);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int rb = wn0 + j * 16, n8 = 2 * ((rb & 63) >> 4) + (p >> 1);
            offB[j] = (rb >> 6) * 8192 + ((((fq * 8 + q) << 3) + (n8 ^ sw)) << 4) + (p & 1) * 8;
        }
    }
    const int rsw = fr >> 1;      // R image: chunk c of row r sits in slot c ^ ((r >> 1) & 7), and (r >> 1) & 7 == fr >> 1 here
    auto frag_r = [&](const unsigned char* img, int off, int kk) -> bf16x8 {
        return *reinterpret_cast<const bf16x8*>(img + off + (((kk * 4 + fq) ^ rsw) << 4));
    };
    auto frag_t = [&](const unsigned char* img, int off, int kk) -> bf16x8 {
        typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
        const unsigned char* a0 = img + off + kk * (32 * 128);      // k-lines 32 kk + 8 fq + q and + 4; a k-line of a block is 128 bytes
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 4 * 128));
        return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    };

    issue_b(0, 0);
    load_a(0);
    store_a(0);
    int slot = 0;
    for (int t = 0; t < nk; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const bool more = t + 1 < nk;
        if (more) {
            issue_b(t + 1, slot ^ 1);
            load_a(t + 1);
        }
        const unsigned char* st = smem + slot * SB;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                ah[i] = frag_r(st, offA[i], kk);
                al[i] = frag_r(st + A_IMG, offA[i], kk);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                bh[j] = TB ? frag_t(st + 2 * A_IMG, offB[j], kk) : frag_r(st + 2 * A_IMG, offB[j], kk);
                if (LO) bl[j] = TB ? frag_t(st + 2 * A_IMG + B_IMG, offB[j], kk) : frag_r(st + 2 * A_IMG + B_IMG, offB[j], kk);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                    if (LO) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                }
        }
        if (more) store_a(slot ^ 1);
        slot ^= 1;
    }

    // C/D map: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = col0 + wn0 + j * 16 + fr;
        if (col >= N) continue;
        const float bv = g.bias ? g.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + wm0 + i * 16 + fq * 4 + r;
                if (row < M) g.C[(size_t)row * g.ldc + col] = acc[i][j][r] + bv;
            }
    }
}

// hi = bf16(src), lo = bf16(src - hi): four elements a thread where the pointers allow, the rest one by one
__global__ void __launch_bounds__(256) split_bf16_kernel(const float* __restrict__ src, size_t n4, size_t n, bf16_t* __restrict__ hi,
                                                         bf16_t* __restrict__ lo) {
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = i0; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(src)[i];
        const bf16x4 h = {(bf16_t)v.x, (bf16_t)v.y, (bf16_t)v.z, (bf16_t)v.w};
        const bf16x4 l = {(bf16_t)(v.x - (float)h[0]), (bf16_t)(v.y - (float)h[1]), (bf16_t)(v.z - (float)h[2]), (bf16_t)(v.w - (float)h[3])};
        reinterpret_cast<bf16x4*>(hi)[i] = h;
        reinterpret_cast<bf16x4*>(lo)[i] = l;
    }
    for (size_t i = 4 * n4 + i0; i < n; i += stride) {
        const float v = src[i];
        const bf16_t h = (bf16_t)v;
        hi[i] = h;
        lo[i] = (bf16_t)(v - (float)h);
    }
}

template <bool LO, int BM, int BN, int WM, int WN>
int launch_split(int layout, const SplitArgs& g, hipStream_t stream) {
    const dim3 grid((unsigned)(cdiv(g.M, BM) * cdiv(g.N, BN))), block(WM * WN * 64);
    if (layout == 0) hipLaunchKernelGGL((gemm_split_kernel<false, LO, BM, BN, WM, WN>), grid, block, 0, stream, g);
    else hipLaunchKernelGGL((gemm_split_kernel<true, LO, BM, BN, WM, WN>), grid, block, 0, stream, g);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

// few rows (the bodies' tail-row products): 16-row tiles, a wave per 16 columns; up to a CU's worth of 128 x 128 tiles: 64 x 64, two
// workgroups per CU (three without Blo); beyond: 128 x 128 on eight waves, one workgroup per CU (128 KiB of LDS, 96 KiB without Blo)
template <bool LO>
int route_split(int layout, const SplitArgs& g, hipStream_t s) {
    if (g.M <= 32) return launch_split<LO, 16, 64, 1, 4>(layout, g, s);
    if ((long)cdiv(g.M, 128) * cdiv(g.N, 128) < 256) return launch_split<LO, 64, 64, 2, 2>(layout, g, s);
    return launch_split<LO, 128, 128, 2, 4>(layout, g, s);
}

SplitArgs split_args(const float* A, int lda, const void* Bhi, const void* Blo, int ldb, float* C, int ldc, const float* bias, int M, int N,
                     int K) {
    SplitArgs g;
    g.A = A;
    g.Bhi = static_cast<const bf16_t*>(Bhi);
    g.Blo = static_cast<const bf16_t*>(Blo);
    g.C = C;
    g.bias = bias;
    g.M = M; g.N = N; g.K = K;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    return g;
}

}  // namespace

extern "C" {

int immtsf_split_bf16(const float* src, uint64_t n, void* hi, void* lo, immtsf_stream_t stream) {
    if (!src || !hi || !lo) return IMMTSF_EINVAL;
    if (n == 0) return IMMTSF_OK;
    const size_t n4 = (al16(src) && al8(hi) && al8(lo)) ? (size_t)(n / 4) : 0;
    hipLaunchKernelGGL(split_bf16_kernel, dim3(grid_for(n4 ? n4 : (size_t)n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), src, n4,
                       (size_t)n, static_cast<bf16_t*>(hi), static_cast<bf16_t*>(lo));
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_gemm_split_supported(int32_t layout, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t ldc) {
    if ((layout != 0 && layout != 1) || M <= 0 || N <= 0 || K <= 0) return 0;
    if ((K % 8) || (N % 8) || (lda % 4) || (ldb % 8)) return 0;
    if (lda < K || ldc < N || ldb < (layout == 0 ? K : N)) return 0;
    if ((long)cdiv(M, 16) * cdiv(N, 64) >= (1L << 31)) return 0;
    return 1;
}

int immtsf_gemm_split(int32_t layout, const float* A, int32_t lda, const void* Bhi, const void* Blo, int32_t ldb, float* C, int32_t ldc,
                      const float* bias, int32_t M, int32_t N, int32_t K, immtsf_stream_t stream) {
    if (!A || !Bhi || !Blo || !C || (layout != 0 && layout != 1) || M <= 0 || N <= 0 || K <= 0) return IMMTSF_EINVAL;
    if (!immtsf_gemm_split_supported(layout, M, N, K, lda, ldb, ldc) || !al16(A) || !al16(Bhi) || !al16(Blo)) return IMMTSF_EUNSUPPORTED;
    return route_split<true>(layout, split_args(A, lda, Bhi, Blo, ldb, C, ldc, bias, M, N, K), static_cast<hipStream_t>(stream));
}

int immtsf_gemm_asplit_supported(int32_t layout, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t ldc) {
    return immtsf_gemm_split_supported(layout, M, N, K, lda, ldb, ldc);
}

int immtsf_gemm_asplit(int32_t layout, const float* A, int32_t lda, const void* B16, int32_t ldb, float* C, int32_t ldc, const float* bias,
                       int32_t M, int32_t N, int32_t K, immtsf_stream_t stream) {
    if (!A || !B16 || !C || (layout != 0 && layout != 1) || M <= 0 || N <= 0 || K <= 0) return IMMTSF_EINVAL;
    if (!immtsf_gemm_asplit_supported(layout, M, N, K, lda, ldb, ldc) || !al16(A) || !al16(B16)) return IMMTSF_EUNSUPPORTED;
    return route_split<false>(layout, split_args(A, lda, B16, nullptr, ldb, C, ldc, bias, M, N, K), static_cast<hipStream_t>(stream));
}

}  // extern "C"
