// Informer's two non-layer stages (reference models/Informer.py:119-184), fp32 in either precision mode.
//
//   front  the padding to input_len / pred_len, the masked instance norm, the (value | mask | time) concatenation, the zero placeholders
//          of the decoder input and both DataEmbeddings (circular 3-tap token convolution + positional table + dropout) as ONE launch:
//              cnt = max(sum_l mask, 1), mean = sum_l data mask / cnt, x = data mask - mean, stdev = sqrt(sum_l (x mask)^2 / cnt + 1e-5),
//              in = [x / stdev | mask | tp]  (rows l >= L: [-mean / stdev | 0 | 0]), never written to memory,
//              enc[b, l, :] = drop(sum_k sum_c W_enc[:, c, k] in[b, (l + k - 1) mod S, c] + pe[l, :])
//              dec[b, t, :] = drop(sum_k W_dec[:, 2C, k] tpp[b, (t + k - 1) mod P] + pe[t, :])      (tpp = 0 for t >= Lp)
//          A workgroup takes 16 output rows of one window: it forms the window's statistics itself (two passes over <= 512 x 32 values:
//          cheaper than a launch), stages the 18 input rows it needs in LDS and gives every thread one output column of four rows, with
//          that column's three weights per channel read straight from L2 (the weight never sits in LDS: 400 KB at d_model 512, C 32).
//          backward, two launches: dW_enc[d, c, k] = sum_{b, l} g[b, l, d] drop in[b, (l + k - 1) mod S, c] by workgroups that own 64
//          columns and a slice of the (window, row tile) units -- 64 columns x 4 channel groups, <= 51 accumulators a thread -- into
//          per-slice partials; the second launch adds the partials in slice order and writes dW_dec's zero columns.
//   tail   decoder.norm (LayerNorm) -> decoder.projection (d_model -> C, bias) -> * stdev[b, c] + means[b, c], rows t < Lp only, a wave
//          per row with the row in registers: ONE launch.  backward, two launches: dx by a wave per row (exact zeros for t >= Lp) next to
//          workgroups that own 64 columns and a slice of the rows for d gamma, d beta, dW_proj, db_proj partials; then the partials in
//          slice order.
// No atomics anywhere: the same inputs give the same bits.
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

constexpr int IM_TR = 16;          // output rows per workgroup of the front stage
constexpr int IM_CMAX = 32;        // channels
constexpr int IM_KC = 2 * IM_CMAX + 1;
constexpr int IM_CI = (IM_KC + 3) / 4;      // channels of one of the four channel groups of the backward
constexpr int IM_LMAX = 512;
constexpr int IM_DMAX = 1024;
constexpr size_t IM_PART_CAP = (size_t)16 << 20;      // bytes of dW_enc partials

struct FrontDims {
    int B, L, S, Lp, P, C, D;
};

bool front_bad(const FrontDims& f) {
    return f.B < 1 || f.L < 1 || f.L > f.S || f.Lp < 1 || f.Lp > f.P || !immtsf_informer_model_supported(f.S, f.P, f.C, f.D);
}

__device__ __forceinline__ int wrap(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

// in[b, l, 0 .. 2C] of the rows (l0 - 1 + j) mod S, j in [0, nrows + 2), into tile[j * Kc + c]
__device__ __forceinline__ void stage_rows(const FrontDims& f, int b, int l0, int nrows, const float* __restrict__ data,
                                           const float* __restrict__ mask, const float* __restrict__ tp, const float* mean,
                                           const float* stdev, float* tile) {
    const int Kc = 2 * f.C + 1;
    for (int i = threadIdx.x; i < (nrows + 2) * Kc; i += blockDim.x) {
        const int j = i / Kc, c = i - j * Kc;
        const int l = wrap(l0 - 1 + j, f.S);                 // l0 - 1 + j in [-1, S]
        float v;
        if (c < f.C) {
            const float d = l < f.L ? data[((size_t)b * f.L + l) * f.C + c] : 0.f, m = l < f.L ? mask[((size_t)b * f.L + l) * f.C + c] : 0.f;
            v = (d * m - mean[c]) / stdev[c];
        } else if (c < 2 * f.C) {
            v = l < f.L ? mask[((size_t)b * f.L + l) * f.C + (c - f.C)] : 0.f;
        } else {
            v = l < f.L ? tp[(size_t)b * f.L + l] : 0.f;
        }
        tile[i] = v;
    }
}

// grid (ceil(S / 16) + ceil(P / 16), B).  Encoder tiles first; every one of them forms the window's statistics in the same order, tile 0
// writes them out.
__global__ __launch_bounds__(256) void informer_front_fwd_kernel(FrontDims f, const float* __restrict__ data, const float* __restrict__ mask,
                                                                  const float* __restrict__ tp, const float* __restrict__ tpp,
                                                                  const float* __restrict__ W_enc, const float* __restrict__ W_dec,
                                                                  const float* __restrict__ pe_enc, const float* __restrict__ pe_dec,
                                                                  float* __restrict__ means, float* __restrict__ stdevs,
                                                                  float* __restrict__ enc, float* __restrict__ dec, DropCfg drop,
                                                                  uint64_t site_enc, uint64_t site_dec) {
    __shared__ float tile[(IM_TR + 2) * IM_KC];
    __shared__ float red[2][8][IM_CMAX];
    __shared__ float s_cnt[IM_CMAX], s_mean[IM_CMAX], s_std[IM_CMAX];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int nE = (f.S + IM_TR - 1) / IM_TR, Kc = 2 * f.C + 1;
    const int D64 = (f.D + 63) & ~63;
    if ((int)blockIdx.x >= nE) {      // ---- decoder rows: the time channel alone
        const int t0 = ((int)blockIdx.x - nE) * IM_TR, nrows = min(IM_TR, f.P - t0);
        for (int j = tid; j < nrows + 2; j += 256) {
            const int t = wrap(wrap(t0 - 1 + j, f.P), f.P);
            tile[j] = t < f.Lp ? tpp[(size_t)b * f.Lp + t] : 0.f;
        }
        __syncthreads();
        for (int item = tid; item < 4 * D64; item += 256) {
            const int rg = item / D64, d = item - rg * D64;
            if (d >= f.D) continue;
            const float* w = W_dec + ((size_t)d * Kc + 2 * f.C) * 3;
            const float w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int r = rg * 4 + rr;
                if (r < nrows) {
                    const float a = fmaf(w0, tile[r], fmaf(w1, tile[r + 1], fmaf(w2, tile[r + 2], pe_dec[(size_t)(t0 + r) * f.D + d])));
                    const size_t o = ((size_t)b * f.P + t0 + r) * f.D + d;
                    dec[o] = a * dropout_scale(drop, site_dec, (uint64_t)o);
                }
            }
        }
        return;
    }
    // ---- the window's statistics: 8 row lanes x 32 channels, summed over the lanes in lane order
    const int c = tid & 31, g = tid >> 5;
    float s0 = 0.f, s1 = 0.f;
    if (c < f.C)
        for (int l = g; l < f.L; l += 8) {
            const size_t o = ((size_t)b * f.L + l) * f.C + c;
            const float m = mask[o];
            s0 += m;
            s1 = fmaf(data[o], m, s1);
        }
    red[0][g][c] = s0;
    red[1][g][c] = s1;
    __syncthreads();
    if (tid < f.C) {
        float a0 = 0.f, a1 = 0.f;
        for (int j = 0; j < 8; ++j) {
            a0 += red[0][j][tid];
            a1 += red[1][j][tid];
        }
        const float cnt = fmaxf(a0, 1.f);
        s_cnt[tid] = cnt;
        s_mean[tid] = a1 / cnt;
    }
    __syncthreads();
    float s2 = 0.f;
    if (c < f.C) {
        const float mean = s_mean[c];
        for (int l = g; l < f.L; l += 8) {
            const size_t o = ((size_t)b * f.L + l) * f.C + c;
            const float m = mask[o];
            const float v = (data[o] * m - mean) * m;
            s2 = fmaf(v, v, s2);
        }
    }
    red[0][g][c] = s2;
    __syncthreads();
    if (tid < f.C) {
        float a = 0.f;
        for (int j = 0; j < 8; ++j) a += red[0][j][tid];
        const float sd = sqrtf(a / s_cnt[tid] + 1e-5f);
        s_std[tid] = sd;
        if (blockIdx.x == 0) {
            means[(size_t)b * f.C + tid] = s_mean[tid];
            stdevs[(size_t)b * f.C + tid] = sd;
        }
    }
    __syncthreads();
    const int l0 = (int)blockIdx.x * IM_TR, nrows = min(IM_TR, f.S - l0);
    stage_rows(f, b, l0, nrows, data, mask, tp, s_mean, s_std, tile);
    __syncthreads();
    for (int item = tid; item < 4 * D64; item += 256) {
        const int rg = item / D64, d = item - rg * D64;      // a wave: 64 consecutive columns of one row group
        if (d >= f.D) continue;
        float acc[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int r = rg * 4 + rr;
            acc[rr] = r < nrows ? pe_enc[(size_t)(l0 + r) * f.D + d] : 0.f;
        }
        const float* w = W_enc + (size_t)d * Kc * 3;
        const float* t = tile + rg * 4 * Kc;
        for (int cc = 0; cc < Kc; ++cc) {
            const float w0 = w[3 * cc], w1 = w[3 * cc + 1], w2 = w[3 * cc + 2];
            const float x0 = t[cc], x1 = t[Kc + cc], x2 = t[2 * Kc + cc], x3 = t[3 * Kc + cc], x4 = t[4 * Kc + cc], x5 = t[5 * Kc + cc];
            acc[0] = fmaf(w0, x0, fmaf(w1, x1, fmaf(w2, x2, acc[0])));
            acc[1] = fmaf(w0, x1, fmaf(w1, x2, fmaf(w2, x3, acc[1])));
            acc[2] = fmaf(w0, x2, fmaf(w1, x3, fmaf(w2, x4, acc[2])));
            acc[3] = fmaf(w0, x3, fmaf(w1, x4, fmaf(w2, x5, acc[3])));
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int r = rg * 4 + rr;
            if (r < nrows) {
                const size_t o = ((size_t)b * f.S + l0 + r) * f.D + d;
                enc[o] = acc[rr] * dropout_scale(drop, site_enc, (uint64_t)o);
            }
        }
    }
}

// how the backward is cut: (slices of the encoder's (window, tile) units, slices of the decoder's rows)
void front_slices(const FrontDims& f, int& nse, int& nsd) {
    const long units = (long)f.B * ((f.S + IM_TR - 1) / IM_TR);
    nse = (int)(units < 64 ? units : 64);
    const size_t per = (size_t)f.D * (2 * f.C + 1) * 3 * sizeof(float);
    while (nse > 1 && nse * per > IM_PART_CAP) --nse;
    const long rows = (long)f.B * f.P;
    const long s = (rows + 63) / 64;
    nsd = (int)(s < 1 ? 1 : s > 32 ? 32 : s);
}

// grid (ceil(D / 64), nse + nsd).  part_e [nse][D][Kc][3], part_d [nsd][D][3]
__global__ __launch_bounds__(256) void informer_front_bwd_kernel(FrontDims f, int nse, int nsd, const float* __restrict__ data,
                                                                  const float* __restrict__ mask, const float* __restrict__ tp,
                                                                  const float* __restrict__ tpp, const float* __restrict__ means,
                                                                  const float* __restrict__ stdevs, const float* __restrict__ g_enc,
                                                                  const float* __restrict__ g_dec, float* __restrict__ part_e,
                                                                  float* __restrict__ part_d, DropCfg drop, uint64_t site_enc,
                                                                  uint64_t site_dec) {
    __shared__ float tile[(IM_TR + 2) * IM_KC];
    __shared__ float s_mean[IM_CMAX], s_std[IM_CMAX];
    __shared__ float red[4][64][3];
    const int tid = threadIdx.x, dc = tid & 63, cg = tid >> 6;
    const int d = (int)blockIdx.x * 64 + dc, Kc = 2 * f.C + 1;
    const bool live = d < f.D;
    if ((int)blockIdx.y >= nse) {      // ---- decoder rows: three sums per column
        const int s = (int)blockIdx.y - nse;
        const long rows = (long)f.B * f.P, per = (rows + nsd - 1) / nsd, q0 = s * per, q1 = min(rows, q0 + per);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (long q = q0 + cg; q < q1; q += 4) {
            const int b = (int)(q / f.P), t = (int)(q - (long)b * f.P);
            const int tm = wrap(t - 1, f.P), tn = wrap(wrap(t + 1, f.P), f.P);
            const float x0 = tm < f.Lp ? tpp[(size_t)b * f.Lp + tm] : 0.f, x1 = t < f.Lp ? tpp[(size_t)b * f.Lp + t] : 0.f,
                        x2 = tn < f.Lp ? tpp[(size_t)b * f.Lp + tn] : 0.f;
            const size_t o = (size_t)q * f.D + d;
            const float gd = live ? g_dec[o] * dropout_scale(drop, site_dec, (uint64_t)o) : 0.f;
            a0 = fmaf(gd, x0, a0);
            a1 = fmaf(gd, x1, a1);
            a2 = fmaf(gd, x2, a2);
        }
        red[cg][dc][0] = a0;
        red[cg][dc][1] = a1;
        red[cg][dc][2] = a2;
        __syncthreads();
        if (cg == 0 && live)
            for (int k = 0; k < 3; ++k)
                part_d[((size_t)s * f.D + d) * 3 + k] = ((red[0][dc][k] + red[1][dc][k]) + red[2][dc][k]) + red[3][dc][k];
        return;
    }
    const int nE = (f.S + IM_TR - 1) / IM_TR;
    const long units = (long)f.B * nE, per = (units + nse - 1) / nse, u0 = (long)blockIdx.y * per, u1 = min(units, u0 + per);
    float acc[IM_CI][3];
#pragma unroll
    for (int ci = 0; ci < IM_CI; ++ci) acc[ci][0] = acc[ci][1] = acc[ci][2] = 0.f;
    int b_have = -1;
    for (long u = u0; u < u1; ++u) {
        const int b = (int)(u / nE), l0 = (int)(u - (long)b * nE) * IM_TR, nrows = min(IM_TR, f.S - l0);
        __syncthreads();
        if (b != b_have) {
            if (tid < f.C) {
                s_mean[tid] = means[(size_t)b * f.C + tid];
                s_std[tid] = stdevs[(size_t)b * f.C + tid];
            }
            b_have = b;
            __syncthreads();
        }
        stage_rows(f, b, l0, nrows, data, mask, tp, s_mean, s_std, tile);
        __syncthreads();
        for (int r = 0; r < nrows; ++r) {
            const size_t o = ((size_t)b * f.S + l0 + r) * f.D + d;
            const float gd = live ? g_enc[o] * dropout_scale(drop, site_enc, (uint64_t)o) : 0.f;
            const float* t = tile + r * Kc;
#pragma unroll
            for (int ci = 0; ci < IM_CI; ++ci) {
                const int c = cg + 4 * ci;
                if (c < Kc) {
                    acc[ci][0] = fmaf(gd, t[c], acc[ci][0]);
                    acc[ci][1] = fmaf(gd, t[Kc + c], acc[ci][1]);
                    acc[ci][2] = fmaf(gd, t[2 * Kc + c], acc[ci][2]);
                }
            }
        }
    }
    if (live) {
        float* p = part_e + ((size_t)blockIdx.y * f.D + d) * Kc * 3;
#pragma unroll
        for (int ci = 0; ci < IM_CI; ++ci) {
            const int c = cg + 4 * ci;
            if (c < Kc) {
                p[3 * c] = acc[ci][0];
                p[3 * c + 1] = acc[ci][1];
                p[3 * c + 2] = acc[ci][2];
            }
        }
    }
}

// dW_enc = the partials in slice order; dW_dec = the same for the time channel's columns and exact zeros everywhere else
__global__ __launch_bounds__(256) void informer_front_reduce_kernel(int D, int Kc, int nse, int nsd, const float* __restrict__ part_e,
                                                                     const float* __restrict__ part_d, float* __restrict__ dW_enc,
                                                                     float* __restrict__ dW_dec) {
    const size_t N = (size_t)D * Kc * 3;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (size_t)gridDim.x * 256) {
        float a = 0.f;
        for (int s = 0; s < nse; ++s) a += part_e[(size_t)s * N + i];
        dW_enc[i] = a;
        const size_t dck = i / 3;
        const int k = (int)(i - dck * 3), c = (int)(dck % Kc);
        float z = 0.f;
        if (c == Kc - 1) {
            const size_t d = dck / Kc;
            for (int s = 0; s < nsd; ++s) z += part_d[((size_t)s * D + d) * 3 + k];
        }
        dW_dec[i] = z;
    }
}

// ---- tail -----------------------------------------------------------------------------------------------------------------------------
struct TailDims {
    int B, Lp, P, C, D, off;      // x (B, P, D): a window's rows off .. off + Lp - 1 are the ones normalised and projected
};

bool tail_bad(const TailDims& t) {
    return t.B < 1 || t.Lp < 1 || t.off < 0 || t.off + t.Lp > t.P || !immtsf_informer_model_supported(1, t.P, t.C, t.D);
}

int tail_slices(const TailDims& t) {
    const long s = ((long)t.B * t.Lp + 63) / 64;
    return (int)(s < 1 ? 1 : s > 64 ? 64 : s);
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w))); }

// a wave per output row (b, t < Lp); the row's D / 4 <= 256 float4 chunks in registers, chunk lane + 64 i in lane's slot i
__global__ __launch_bounds__(256) void informer_tail_fwd_kernel(TailDims t, const float* __restrict__ x, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float eps, const float* __restrict__ W,
                                                                 const float* __restrict__ bias, const float* __restrict__ means,
                                                                 const float* __restrict__ stdevs, float* __restrict__ y,
                                                                 float* __restrict__ row_mean, float* __restrict__ row_rstd) {
    const int lane = threadIdx.x & 63;
    const long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= (long)t.B * t.Lp) return;
    const int b = (int)(q / t.Lp), tt = (int)(q - (long)b * t.Lp), n4 = t.D >> 2;
    const float4* xr = reinterpret_cast<const float4*>(x + ((size_t)b * t.P + t.off + tt) * t.D);
    float4 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = lane + 64 * i;
        v[i] = j < n4 ? xr[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float mean = wave_sum(s) / (float)t.D;
    float s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = lane + 64 * i;
        if (j < n4) {
            v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
            s2 += dot4(v[i], v[i]);
        }
    }
    const float rstd = 1.f / sqrtf(wave_sum(s2) / (float)t.D + eps);
    if (lane == 0) {
        row_mean[q] = mean;
        row_rstd[q] = rstd;
    }
    const float4* g4 = reinterpret_cast<const float4*>(gamma);
    const float4* b4 = reinterpret_cast<const float4*>(beta);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = lane + 64 * i;
        if (j < n4) {
            const float4 gg = g4[j], bb = b4[j];
            v[i].x = fmaf(v[i].x * rstd, gg.x, bb.x);
            v[i].y = fmaf(v[i].y * rstd, gg.y, bb.y);
            v[i].z = fmaf(v[i].z * rstd, gg.z, bb.z);
            v[i].w = fmaf(v[i].w * rstd, gg.w, bb.w);
        }
    }
    float mine = 0.f;
    for (int c = 0; c < t.C; ++c) {
        const float4* w4 = reinterpret_cast<const float4*>(W + (size_t)c * t.D);
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = lane + 64 * i;
            if (j < n4) a += dot4(v[i], w4[j]);
        }
        a = wave_sum(a);
        if (lane == c) mine = a;
    }
    if (lane < t.C) y[(size_t)q * t.C + lane] = fmaf(mine + bias[lane], stdevs[(size_t)b * t.C + lane], means[(size_t)b * t.C + lane]);
}

// blocks [0, ceil(B P / 4)): dx, a wave per row of x (exact zeros outside the rows off .. off + Lp - 1).  The DT * ns blocks behind them: the parameter partials,
// 64 columns x 4 row lanes over a slice of the B Lp rows, part [ns][2 D + C D + C] = [d gamma | d beta | dW | db]
__global__ __launch_bounds__(256) void informer_tail_bwd_kernel(TailDims t, int ns, const float* __restrict__ x, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, const float* __restrict__ W,
                                                                 const float* __restrict__ stdevs, const float* __restrict__ row_mean,
                                                                 const float* __restrict__ row_rstd, const float* __restrict__ dy,
                                                                 float* __restrict__ dx, float* __restrict__ part) {
    __shared__ float dzs[32][IM_CMAX];
    __shared__ float ms[32], rs[32];
    __shared__ float red[4][64][IM_CMAX + 3];
    const int tid = threadIdx.x, lane = tid & 63;
    const long xrows = (long)t.B * t.P;
    const int nrb = (int)((xrows + 3) / 4);
    if ((int)blockIdx.x < nrb) {
        const long q = (long)blockIdx.x * 4 + (tid >> 6);
        if (q >= xrows) return;
        const int b = (int)(q / t.P), tt = (int)(q - (long)b * t.P) - t.off, n4 = t.D >> 2;
        float4* dxr = reinterpret_cast<float4*>(dx + (size_t)q * t.D);
        if (tt < 0 || tt >= t.Lp) {
            for (int j = lane; j < n4; j += 64) dxr[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            return;
        }
        const long r = (long)b * t.Lp + tt;
        const float mean = row_mean[r], rstd = row_rstd[r];
        const float dzl = lane < t.C ? dy[(size_t)r * t.C + lane] * stdevs[(size_t)b * t.C + lane] : 0.f;
        const float4* xr = reinterpret_cast<const float4*>(x + (size_t)q * t.D);
        const float4* g4 = reinterpret_cast<const float4*>(gamma);
        float4 xh[4], gn[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = lane + 64 * i;
            gn[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            xh[i] = gn[i];
            if (j < n4) {
                const float4 xv = xr[j];
                xh[i] = make_float4((xv.x - mean) * rstd, (xv.y - mean) * rstd, (xv.z - mean) * rstd, (xv.w - mean) * rstd);
            }
        }
        for (int c = 0; c < t.C; ++c) {
            const float dz = lane_bcast(dzl, c);
            const float4* w4 = reinterpret_cast<const float4*>(W + (size_t)c * t.D);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = lane + 64 * i;
                if (j < n4) {
                    const float4 w = w4[j];
                    gn[i].x = fmaf(dz, w.x, gn[i].x);
                    gn[i].y = fmaf(dz, w.y, gn[i].y);
                    gn[i].z = fmaf(dz, w.z, gn[i].z);
                    gn[i].w = fmaf(dz, w.w, gn[i].w);
                }
            }
        }
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = lane + 64 * i;
            if (j < n4) {
                const float4 gg = g4[j];
                gn[i].x *= gg.x; gn[i].y *= gg.y; gn[i].z *= gg.z; gn[i].w *= gg.w;
                s1 += (gn[i].x + gn[i].y) + (gn[i].z + gn[i].w);
                s2 += dot4(gn[i], xh[i]);
            }
        }
        s1 = wave_sum(s1) / (float)t.D;
        s2 = wave_sum(s2) / (float)t.D;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = lane + 64 * i;
            if (j < n4)
                dxr[j] = make_float4(rstd * (gn[i].x - s1 - xh[i].x * s2), rstd * (gn[i].y - s1 - xh[i].y * s2),
                                     rstd * (gn[i].z - s1 - xh[i].z * s2), rstd * (gn[i].w - s1 - xh[i].w * s2));
        }
        return;
    }
    // ---- parameter partials
    const int pb = (int)blockIdx.x - nrb, DT = (t.D + 63) / 64;
    const int s = pb / DT, dt = pb - s * DT;
    const int dc = lane, rl = tid >> 6, d = dt * 64 + dc;
    const bool live = d < t.D;
    const long rows = (long)t.B * t.Lp, per = (rows + ns - 1) / ns, r0 = s * per, r1 = min(rows, r0 + per);
    const size_t N = (size_t)2 * t.D + (size_t)t.C * t.D + t.C;
    float Wc[IM_CMAX], aW[IM_CMAX];
#pragma unroll
    for (int c = 0; c < IM_CMAX; ++c) {
        Wc[c] = (live && c < t.C) ? W[(size_t)c * t.D + d] : 0.f;
        aW[c] = 0.f;
    }
    const float gam = live ? gamma[d] : 0.f, bet = live ? beta[d] : 0.f;
    float ag = 0.f, ab = 0.f;
    for (long rc = r0; rc < r1; rc += 32) {
        __syncthreads();
        for (int i = tid; i < 32 * IM_CMAX; i += 256) {
            const int rr = i >> 5, c = i & 31;
            const long r = rc + rr;
            dzs[rr][c] = (r < r1 && c < t.C) ? dy[(size_t)r * t.C + c] * stdevs[(size_t)(r / t.Lp) * t.C + c] : 0.f;
        }
        if (tid < 32) {
            const long r = rc + tid;
            ms[tid] = r < r1 ? row_mean[r] : 0.f;
            rs[tid] = r < r1 ? row_rstd[r] : 0.f;
        }
        __syncthreads();
#pragma unroll 2
        for (int i = 0; i < 8; ++i) {
            const int rr = rl + 4 * i;
            const long r = rc + rr;
            if (r >= r1) break;
            const int b = (int)(r / t.Lp), tt = (int)(r - (long)b * t.Lp);
            const float xv = live ? x[((size_t)b * t.P + t.off + tt) * t.D + d] : 0.f;
            const float xh = (xv - ms[rr]) * rs[rr], n = fmaf(xh, gam, bet);
            float dn = 0.f;
#pragma unroll
            for (int c = 0; c < IM_CMAX; ++c) {
                if (c < t.C) {
                    const float dz = dzs[rr][c];
                    dn = fmaf(dz, Wc[c], dn);
                    aW[c] = fmaf(dz, n, aW[c]);
                }
            }
            ag = fmaf(dn, xh, ag);
            ab += dn;
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < IM_CMAX; ++c) red[rl][dc][c] = aW[c];
    red[rl][dc][IM_CMAX] = ag;
    red[rl][dc][IM_CMAX + 1] = ab;
    __syncthreads();
    float* p = part + (size_t)s * N;
    for (int i = tid; i < 64 * (t.C + 2); i += 256) {
        const int v = i >> 6, col = i & 63, dd = dt * 64 + col;      // v: 0 .. C-1 = dW row, C = d gamma, C + 1 = d beta
        if (dd >= t.D) continue;
        const int slot = v < t.C ? v : IM_CMAX + (v - t.C);
        const float a = ((red[0][col][slot] + red[1][col][slot]) + red[2][col][slot]) + red[3][col][slot];
        if (v < t.C) p[(size_t)2 * t.D + (size_t)v * t.D + dd] = a;
        else p[(size_t)(v - t.C) * t.D + dd] = a;
    }
    if (dt == 0) {      // db_proj of the slice: 8 row lanes x 32 channels
        __syncthreads();
        const int c = tid & 31, g = tid >> 5;
        float a = 0.f;
        if (c < t.C)
            for (long r = r0 + g; r < r1; r += 8) a = fmaf(dy[(size_t)r * t.C + c], stdevs[(size_t)(r / t.Lp) * t.C + c], a);
        float* rd = &red[0][0][0];
        rd[g * 32 + c] = a;
        __syncthreads();
        if (tid < t.C) {
            float z = 0.f;
            for (int j = 0; j < 8; ++j) z += rd[j * 32 + tid];
            p[(size_t)2 * t.D + (size_t)t.C * t.D + tid] = z;
        }
    }
}

__global__ __launch_bounds__(256) void informer_slice_sum_kernel(size_t N, int ns, const float* __restrict__ part, float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (size_t)gridDim.x * 256) {
        float a = 0.f;
        for (int s = 0; s < ns; ++s) a += part[(size_t)s * N + i];
        out[i] = a;
    }
}

DropCfg im_drop(float p, uint64_t seed, const uint64_t* seed_dev) {
    DropCfg d = mk_drop(p, seed);
    d.seed_dev = seed_dev;
    return d;
}

}  // namespace

extern "C" {

int immtsf_informer_model_supported(int32_t input_len, int32_t pred_len, int32_t C, int32_t d_model) {
    if (input_len < 1 || input_len > IM_LMAX || pred_len < 1 || pred_len > IM_LMAX || C < 1 || C > IM_CMAX) return 0;
    if (d_model < 4 || d_model > IM_DMAX || d_model % 4) return 0;
    return d_model <= 512 || d_model % 64 == 0;      // above 512: whole 64-column tiles only
}

size_t immtsf_informer_front_workspace_bytes(int32_t B, int32_t input_len, int32_t pred_len, int32_t C, int32_t d_model) {
    const FrontDims f{B, 1, input_len, 1, pred_len, C, d_model};
    if (front_bad(f)) return 0;
    int nse, nsd;
    front_slices(f, nse, nsd);
    return ((size_t)nse * d_model * (2 * C + 1) * 3 + (size_t)nsd * d_model * 3) * sizeof(float);
}

int immtsf_informer_front_forward(int32_t B, int32_t L, int32_t input_len, int32_t Lp, int32_t pred_len, int32_t C, int32_t d_model,
                                  const float* data, const float* mask, const float* tp, const float* tpp, const float* W_enc,
                                  const float* W_dec, const float* pe_enc, const float* pe_dec, float* means, float* stdev, float* enc,
                                  float* dec, float p_drop, uint64_t seed, uint64_t site_enc, uint64_t site_dec,
                                  const uint64_t* seed_step_dev, immtsf_stream_t stream) {
    const FrontDims f{B, L, input_len, Lp, pred_len, C, d_model};
    if (!data || !mask || !tp || !tpp || !W_enc || !W_dec || !pe_enc || !pe_dec || !means || !stdev || !enc || !dec) return IMMTSF_EINVAL;
    if (front_bad(f) || B > 65535) return IMMTSF_EUNSUPPORTED;
    const dim3 grid((unsigned)(cdiv(input_len, IM_TR) + cdiv(pred_len, IM_TR)), (unsigned)B);
    hipLaunchKernelGGL(informer_front_fwd_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), f, data, mask, tp, tpp, W_enc,
                       W_dec, pe_enc, pe_dec, means, stdev, enc, dec, im_drop(p_drop, seed, seed_step_dev), site_enc, site_dec);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_informer_front_backward(int32_t B, int32_t L, int32_t input_len, int32_t Lp, int32_t pred_len, int32_t C, int32_t d_model,
                                   const float* data, const float* mask, const float* tp, const float* tpp, const float* means,
                                   const float* stdev, const float* d_enc, const float* d_dec, float* dW_enc, float* dW_dec,
                                   float p_drop, uint64_t seed, uint64_t site_enc, uint64_t site_dec, const uint64_t* seed_step_dev,
                                   void* workspace, size_t workspace_bytes, immtsf_stream_t stream) {
    const FrontDims f{B, L, input_len, Lp, pred_len, C, d_model};
    if (!data || !mask || !tp || !tpp || !means || !stdev || !d_enc || !d_dec || !dW_enc || !dW_dec || !workspace) return IMMTSF_EINVAL;
    if (front_bad(f)) return IMMTSF_EUNSUPPORTED;
    if (workspace_bytes < immtsf_informer_front_workspace_bytes(B, input_len, pred_len, C, d_model)) return IMMTSF_EWORKSPACE;
    int nse, nsd;
    front_slices(f, nse, nsd);
    const int Kc = 2 * C + 1;
    float* part_e = static_cast<float*>(workspace);
    float* part_d = part_e + (size_t)nse * d_model * Kc * 3;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(informer_front_bwd_kernel, dim3((unsigned)cdiv(d_model, 64), (unsigned)(nse + nsd)), dim3(256), 0, s, f, nse, nsd,
                       data, mask, tp, tpp, means, stdev, d_enc, d_dec, part_e, part_d, im_drop(p_drop, seed, seed_step_dev), site_enc,
                       site_dec);
    IMMTSF_LAUNCH_CHECK();
    hipLaunchKernelGGL(informer_front_reduce_kernel, dim3(grid_for((size_t)d_model * Kc * 3, 256)), dim3(256), 0, s, d_model, Kc, nse, nsd,
                       part_e, part_d, dW_enc, dW_dec);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

size_t immtsf_informer_tail_workspace_bytes(int32_t B, int32_t Lp, int32_t C, int32_t d_model) {
    const TailDims t{B, Lp, Lp, C, d_model, 0};
    if (Lp > IM_LMAX || tail_bad(t)) return 0;
    return (size_t)tail_slices(t) * ((size_t)2 * d_model + (size_t)C * d_model + C) * sizeof(float);
}

static int tail_forward(const TailDims& t, const float* x, const float* gamma, const float* beta, float eps, const float* W, const float* bias,
                        const float* means, const float* stdev, float* y, float* row_mean, float* row_rstd, immtsf_stream_t stream) {
    const int B = t.B, Lp = t.Lp;
    if (!x || !gamma || !beta || !W || !bias || !means || !stdev || !y || !row_mean || !row_rstd) return IMMTSF_EINVAL;
    if (!al16(x) || !al16(gamma) || !al16(beta) || !al16(W)) return IMMTSF_EINVAL;
    if (tail_bad(t)) return IMMTSF_EUNSUPPORTED;
    const long rows = (long)B * Lp;
    hipLaunchKernelGGL(informer_tail_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), t, x, gamma,
                       beta, eps, W, bias, means, stdev, y, row_mean, row_rstd);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

static int tail_backward(const TailDims& t, const float* x, const float* gamma, const float* beta, const float* W, const float* stdev,
                         const float* row_mean, const float* row_rstd, const float* dy, float* dx, float* dparams, void* workspace,
                         size_t workspace_bytes, immtsf_stream_t stream) {
    const int B = t.B, Lp = t.Lp, pred_len = t.P, C = t.C, d_model = t.D;
    if (!x || !gamma || !beta || !W || !stdev || !row_mean || !row_rstd || !dy || !dx || !dparams || !workspace) return IMMTSF_EINVAL;
    if (!al16(x) || !al16(gamma) || !al16(W) || !al16(dx)) return IMMTSF_EINVAL;
    if (tail_bad(t)) return IMMTSF_EUNSUPPORTED;
    if (workspace_bytes < immtsf_informer_tail_workspace_bytes(B, Lp, C, d_model)) return IMMTSF_EWORKSPACE;
    const int ns = tail_slices(t);
    const long xrows = (long)B * pred_len;
    const unsigned grid = (unsigned)((xrows + 3) / 4) + (unsigned)(cdiv(d_model, 64) * ns);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(informer_tail_bwd_kernel, dim3(grid), dim3(256), 0, s, t, ns, x, gamma, beta, W, stdev, row_mean, row_rstd, dy, dx,
                       part);
    IMMTSF_LAUNCH_CHECK();
    const size_t N = (size_t)2 * d_model + (size_t)C * d_model + C;
    hipLaunchKernelGGL(informer_slice_sum_kernel, dim3(grid_for(N, 256)), dim3(256), 0, s, N, ns, part, dparams);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_informer_tail_forward(int32_t B, int32_t Lp, int32_t pred_len, int32_t C, int32_t d_model, const float* x, const float* gamma,
                                 const float* beta, float eps, const float* W, const float* bias, const float* means, const float* stdev,
                                 float* y, float* row_mean, float* row_rstd, immtsf_stream_t stream) {
    return tail_forward(TailDims{B, Lp, pred_len, C, d_model, 0}, x, gamma, beta, eps, W, bias, means, stdev, y, row_mean, row_rstd, stream);
}

int immtsf_informer_tail_backward(int32_t B, int32_t Lp, int32_t pred_len, int32_t C, int32_t d_model, const float* x, const float* gamma,
                                  const float* beta, const float* W, const float* stdev, const float* row_mean, const float* row_rstd,
                                  const float* dy, float* dx, float* dparams, void* workspace, size_t workspace_bytes,
                                  immtsf_stream_t stream) {
    return tail_backward(TailDims{B, Lp, pred_len, C, d_model, 0}, x, gamma, beta, W, stdev, row_mean, row_rstd, dy, dx, dparams, workspace,
                         workspace_bytes, stream);
}

// TimesNet's tail (models/TimesNet.py): the same kernels on x (B, T, D) with the horizon at rows row_off .. row_off + Lp - 1 of a window
int immtsf_timesnet_tail_forward(int32_t B, int32_t Lp, int32_t T, int32_t row_off, int32_t C, int32_t d_model, const float* x,
                                 const float* gamma, const float* beta, float eps, const float* W, const float* bias, const float* means,
                                 const float* stdev, float* y, float* row_mean, float* row_rstd, immtsf_stream_t stream) {
    return tail_forward(TailDims{B, Lp, T, C, d_model, row_off}, x, gamma, beta, eps, W, bias, means, stdev, y, row_mean, row_rstd, stream);
}

int immtsf_timesnet_tail_backward(int32_t B, int32_t Lp, int32_t T, int32_t row_off, int32_t C, int32_t d_model, const float* x,
                                  const float* gamma, const float* beta, const float* W, const float* stdev, const float* row_mean,
                                  const float* row_rstd, const float* dy, float* dx, float* dparams, void* workspace, size_t workspace_bytes,
                                  immtsf_stream_t stream) {
    return tail_backward(TailDims{B, Lp, T, C, d_model, row_off}, x, gamma, beta, W, stdev, row_mean, row_rstd, dy, dx, dparams, workspace,
                         workspace_bytes, stream);
}

}  // extern "C"
