// TimesNet's front end (reference models/TimesNet.py:108-131, layers/Embed.py:29-42, 109-126), fp32 in either precision mode.  The output
// tail is informer.hip's tail kernels with a row pitch and a row offset (immtsf_timesnet_tail_forward / _backward there).
//
//   front  the padding to input_len (S) / pred_len (P), the plain instance norm over all S rows, the (value | mask | time) concatenation,
//          DataEmbedding (circular 3-tap token convolution + positional table + dropout), the horizon rows and predict_linear, which mixes
//          along time, as ONE launch; with T = S + P:
//              mean = sum_l data / S, x = data - mean, stdev = sqrt(sum_l x^2 / S + 1e-5)      (rows l >= L are zeros and count)
//              in = [x / stdev | mask | tp]                                                     (S x (2C + 1), LDS only)
//              E[b, s, :] = drop(sum_k sum_c Wc[:, c, k] in[b, (s + k - 1) mod S, c] + pe[s, :])   s < S
//              E[b, S + j, :] = tpp[b, j]  (0 for j >= Lp)
//              enc[b, t, d] = sum_s Wp[t, s] E[b, s, d] + bp[t]
//          A workgroup takes (16 rows t, 16 columns d) of one window: it stages the window's input tile and forms the statistics as
//          immtsf_instance_norm does (a thread per channel walks the S rows in order: the same bits), forms the T x 16 tile of E in LDS and
//          sweeps its 16 rows of Wp (staged in LDS) against it.  E reaches memory only when the caller asks for it (E_save).
//          backward, two launches.  Workgroups own 16 columns and a slice of the windows; per window they rebuild (or load) the E tile, load
//          the d_enc tile, and add
//              dWp[t, s] += sum_d g[t, d] E[s, d]      (4 x 4 register blocks, the workgroup's own partial in memory)
//              dbp[t]    += sum_d g[t, d]
//              dE[s, d]   = drop * sum_t Wp[t, s] g[t, d]   (s < S), then dWc[d, c, k] += sum_s dE[s, d] in[(s + k - 1) mod S, c]
//          into per-workgroup partials; the second launch adds the partials in workgroup order.
// No atomics anywhere: the same inputs give the same bits.
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

constexpr int TM_DT = 16;          // d_model columns per workgroup
constexpr int TM_TT = 16;          // output rows per workgroup of the forward
constexpr int TM_EP = 20;          // row pitch of the E / d_enc tiles of the backward: float4 rows, 16 consecutive rows on 64 distinct banks
constexpr int TM_TMAX = 256;       // input_len + pred_len
constexpr int TM_CMAX = 10;        // channels: 3 (2C + 1) <= 64, where DataEmbedding itself takes immtsf_embed_forward
constexpr int TM_DMAX = 512;
constexpr size_t TM_PART_CAP = (size_t)32 << 20;      // bytes of dWp partials

struct TmDims {
    int B, L, S, Lp, P, C, D;
};

bool tm_bad(const TmDims& f) {
    return f.B < 1 || f.B > 65535 || f.L < 1 || f.L > f.S || f.Lp < 1 || f.Lp > f.P || !immtsf_timesnet_model_supported(f.S, f.P, f.C, f.D);
}

__host__ __device__ __forceinline__ int up4(int n) { return (n + 3) & ~3; }

// the window's raw [data | mask | tp] rows, zero-padded to S rows, into in[s * Kc + c]
__device__ __forceinline__ void stage_raw(const TmDims& f, int b, const float* __restrict__ data, const float* __restrict__ mask,
                                          const float* __restrict__ tp, float* in) {
    const int Kc = 2 * f.C + 1;
    for (int i = threadIdx.x; i < f.S * Kc; i += 256) {
        const int s = i / Kc, c = i - s * Kc;
        float v = 0.f;
        if (s < f.L) v = c < f.C ? data[((size_t)b * f.L + s) * f.C + c] : c < 2 * f.C ? mask[((size_t)b * f.L + s) * f.C + (c - f.C)] : tp[(size_t)b * f.L + s];
        in[i] = v;
    }
}

// in[:, c] = (in[:, c] - mean[c]) / stdev[c] for the value channels
__device__ __forceinline__ void normalise(const TmDims& f, float* in, const float* mu, const float* sd) {
    const int Kc = 2 * f.C + 1;
    for (int i = threadIdx.x; i < f.S * f.C; i += 256) {
        const int s = i / f.C, c = i - s * f.C;
        in[s * Kc + c] = (in[s * Kc + c] - mu[c]) / sd[c];
    }
}

// the token weights of columns d0 .. d0 + 15 into wl[(c * 3 + k) * 16 + dd]
__device__ __forceinline__ void stage_wc(const TmDims& f, int d0, const float* __restrict__ Wc, float* wl) {
    const int K3 = (2 * f.C + 1) * 3;
    for (int i = threadIdx.x; i < K3 * TM_DT; i += 256) {
        const int dd = i / K3, k = i - dd * K3;
        wl[k * TM_DT + dd] = d0 + dd < f.D ? Wc[(size_t)(d0 + dd) * K3 + k] : 0.f;
    }
}

// the (rows x 16) tile of E of window b, columns d0 .. d0 + 15, into Et[s * pitch + dd]; rows T .. rows - 1 and columns >= D are zeros.
// E_load (B, S, D): the embedded rows as the forward saved them, or null to form them here; E_out: where to save them, or null.
__device__ __forceinline__ void form_E(const TmDims& f, int b, int d0, int rows, int pitch, const float* in, const float* wl,
                                       const float* __restrict__ pe, const float* __restrict__ tpp, const float* __restrict__ E_load,
                                       float* __restrict__ E_out, const DropCfg& drop, uint64_t site, float* Et) {
    const int Kc = 2 * f.C + 1, T = f.S + f.P;
    for (int i = threadIdx.x; i < rows * TM_DT; i += 256) {
        const int s = i >> 4, dd = i & 15, d = d0 + dd;
        float a = 0.f;
        if (d < f.D && s < T) {
            if (s >= f.S) {
                const int j = s - f.S;
                a = j < f.Lp ? tpp[(size_t)b * f.Lp + j] : 0.f;
            } else {
                const size_t o = ((size_t)b * f.S + s) * f.D + d;
                if (E_load) {
                    a = E_load[o];
                } else {
                    const int sm = s == 0 ? f.S - 1 : s - 1, sn = s == f.S - 1 ? 0 : s + 1;
                    const float *r0 = in + sm * Kc, *r1 = in + s * Kc, *r2 = in + sn * Kc;
                    a = pe[(size_t)s * f.D + d];
                    for (int c = 0; c < Kc; ++c) {
                        const float* w = wl + c * 3 * TM_DT + dd;
                        a = fmaf(w[0], r0[c], fmaf(w[TM_DT], r1[c], fmaf(w[2 * TM_DT], r2[c], a)));
                    }
                    a *= dropout_scale(drop, site, (uint64_t)o);
                    if (E_out) E_out[o] = a;
                }
            }
        }
        Et[s * pitch + dd] = a;
    }
}

// dynamic LDS of the forward, in floats: in | wl | Et | Wt | mean | stdev
__host__ __device__ __forceinline__ int fwd_lds_floats(int S, int P, int C) {
    const int Kc = 2 * C + 1, T = S + P;
    return up4(S * Kc) + Kc * 3 * TM_DT + T * TM_DT + TM_TT * (T + 1) + 32;
}

// grid (ceil(T / 16), ceil(D / 16), B)
__global__ __launch_bounds__(256) void timesnet_front_fwd_kernel(TmDims f, const float* __restrict__ data, const float* __restrict__ mask,
                                                                  const float* __restrict__ tp, const float* __restrict__ tpp,
                                                                  const float* __restrict__ Wc, const float* __restrict__ pe,
                                                                  const float* __restrict__ Wp, const float* __restrict__ bp,
                                                                  float* __restrict__ means, float* __restrict__ stdevs, float* __restrict__ enc,
                                                                  float* __restrict__ E_save, DropCfg drop, uint64_t site) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Kc = 2 * f.C + 1, T = f.S + f.P, tid = threadIdx.x;
    float* in = lds;
    float* wl = in + up4(f.S * Kc);
    float* Et = wl + Kc * 3 * TM_DT;
    float* Wt = Et + T * TM_DT;
    float* mu = Wt + TM_TT * (T + 1);
    float* sd = mu + 16;
    const int t0 = (int)blockIdx.x * TM_TT, d0 = (int)blockIdx.y * TM_DT, b = (int)blockIdx.z;
    const int nrows = min(TM_TT, T - t0);
    stage_raw(f, b, data, mask, tp, in);
    stage_wc(f, d0, Wc, wl);
    for (int i = tid; i < nrows * T; i += 256) {
        const int r = i / T, s = i - r * T;
        Wt[r * (T + 1) + s] = Wp[(size_t)(t0 + r) * T + s];
    }
    __syncthreads();
    if (tid < f.C) {      // a thread per channel, rows in order: immtsf_instance_norm's sums
        float s = 0.f;
        for (int l = 0; l < f.S; ++l) s += in[l * Kc + tid];
        const float m = s / (float)f.S;
        float v = 0.f;
        for (int l = 0; l < f.S; ++l) {
            const float q = in[l * Kc + tid] - m;
            v = fmaf(q, q, v);
        }
        const float dev = sqrtf(v / (float)f.S + 1e-5f);
        mu[tid] = m;
        sd[tid] = dev;
        if (blockIdx.x == 0 && blockIdx.y == 0) {
            means[(size_t)b * f.C + tid] = m;
            stdevs[(size_t)b * f.C + tid] = dev;
        }
    }
    __syncthreads();
    normalise(f, in, mu, sd);
    __syncthreads();
    form_E(f, b, d0, T, TM_DT, in, wl, pe, tpp, nullptr, blockIdx.x == 0 ? E_save : nullptr, drop, site, Et);
    __syncthreads();
    const int r = tid >> 4, dd = tid & 15;
    if (r < nrows && d0 + dd < f.D) {
        const float* w = Wt + r * (T + 1);
        const float* e = Et + dd;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int s = 0;
        for (; s + 4 <= T; s += 4) {
            a0 = fmaf(w[s], e[s * TM_DT], a0);
            a1 = fmaf(w[s + 1], e[(s + 1) * TM_DT], a1);
            a2 = fmaf(w[s + 2], e[(s + 2) * TM_DT], a2);
            a3 = fmaf(w[s + 3], e[(s + 3) * TM_DT], a3);
        }
        for (; s < T; ++s) a0 = fmaf(w[s], e[s * TM_DT], a0);
        enc[((size_t)b * T + t0 + r) * f.D + d0 + dd] = ((a0 + a1) + (a2 + a3)) + bp[t0 + r];
    }
}

// how the backward is cut: slices of the windows (each times ceil(D / 16) workgroups)
int tm_slices(const TmDims& f) {
    const int DTn = cdiv(f.D, TM_DT), T = f.S + f.P;
    int ns = f.B < 64 ? f.B : 64;
    while (ns > 1 && (size_t)ns * DTn * T * T * sizeof(float) > TM_PART_CAP) --ns;
    const int per = (f.B + ns - 1) / ns;
    return (f.B + per - 1) / per;      // no empty slice: every partial is written
}

// dynamic LDS of the backward, in floats: in | wl | Et | Gt | dEt | mean | stdev
__host__ __device__ __forceinline__ int bwd_lds_floats(int S, int P, int C) {
    const int Kc = 2 * C + 1, T4 = up4(S + P);
    return up4(S * Kc) + Kc * 3 * TM_DT + 2 * T4 * TM_EP + S * TM_DT + 32;
}

// grid (ceil(D / 16), ns).  part_p [ns * DTn][T][T], part_b [ns * DTn][T], part_c [ns][D][Kc][3]
__global__ __launch_bounds__(256) void timesnet_front_bwd_kernel(TmDims f, int ns, const float* __restrict__ data, const float* __restrict__ mask,
                                                                  const float* __restrict__ tp, const float* __restrict__ tpp,
                                                                  const float* __restrict__ Wc, const float* __restrict__ pe,
                                                                  const float* __restrict__ Wp, const float* __restrict__ means,
                                                                  const float* __restrict__ stdevs, const float* __restrict__ E_saved,
                                                                  const float* __restrict__ g, float* __restrict__ part_p,
                                                                  float* __restrict__ part_b, float* __restrict__ part_c, DropCfg drop,
                                                                  uint64_t site) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Kc = 2 * f.C + 1, K3 = Kc * 3, T = f.S + f.P, T4 = up4(T), Q = T4 >> 2, tid = threadIdx.x;
    float* in = lds;
    float* wl = in + up4(f.S * Kc);
    float* Et = wl + K3 * TM_DT;
    float* Gt = Et + T4 * TM_EP;
    float* dEt = Gt + T4 * TM_EP;
    float* mu = dEt + f.S * TM_DT;
    float* sd = mu + 16;
    const int dt = (int)blockIdx.x, d0 = dt * TM_DT, sl = (int)blockIdx.y, DTn = (int)gridDim.x;
    const int per = (f.B + ns - 1) / ns, b0 = sl * per, b1 = min(f.B, b0 + per);
    float* pp = part_p + ((size_t)sl * DTn + dt) * T * T;
    stage_wc(f, d0, Wc, wl);
    float abp = 0.f, ac[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = b0; b < b1; ++b) {
        __syncthreads();
        stage_raw(f, b, data, mask, tp, in);
        if (tid < f.C) {
            mu[tid] = means[(size_t)b * f.C + tid];
            sd[tid] = stdevs[(size_t)b * f.C + tid];
        }
        for (int i = tid; i < T4 * 4; i += 256) {      // the d_enc tile, 16 bytes a thread
            const int t = i >> 2, q = i & 3;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < T && d0 + 4 * q < f.D) v = *reinterpret_cast<const float4*>(g + ((size_t)b * T + t) * f.D + d0 + 4 * q);
            *reinterpret_cast<float4*>(Gt + t * TM_EP + 4 * q) = v;
        }
        __syncthreads();
        normalise(f, in, mu, sd);
        __syncthreads();
        form_E(f, b, d0, T4, TM_EP, in, wl, pe, tpp, E_saved, nullptr, drop, site, Et);
        __syncthreads();
        // ---- dWp: thread block (t = ti + i Q, s = si + j Q)
        for (int blk = tid; blk < Q * Q; blk += 256) {
            const int ti = blk / Q, si = blk - ti * Q;
            float acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float4 gv[4], ev[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    gv[i] = *reinterpret_cast<const float4*>(Gt + (ti + i * Q) * TM_EP + 4 * q);
                    ev[i] = *reinterpret_cast<const float4*>(Et + (si + i * Q) * TM_EP + 4 * q);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = fmaf(gv[i].x, ev[j].x, fmaf(gv[i].y, ev[j].y, fmaf(gv[i].z, ev[j].z, fmaf(gv[i].w, ev[j].w, acc[i][j]))));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = ti + i * Q;
                if (t >= T) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int s = si + j * Q;
                    if (s < T) {
                        float* p = pp + (size_t)t * T + s;      // this thread's own element in every round
                        *p = b == b0 ? acc[i][j] : *p + acc[i][j];
                    }
                }
            }
        }
        // ---- dbp
        if (tid < T) {
            const float* gr = Gt + tid * TM_EP;
            float a = 0.f;
#pragma unroll
            for (int dd = 0; dd < TM_DT; ++dd) a += gr[dd];
            abp += a;
        }
        // ---- dE = Wp^T g on the rows s < S: thread (s lane, column quad)
        {
            const int sq = tid & 63, q = tid >> 6;
            for (int s = sq; s < f.S; s += 64) {
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
                for (int t = 0; t < T; ++t) {
                    const float w = Wp[(size_t)t * T + s];
                    const float4 gv = *reinterpret_cast<const float4*>(Gt + t * TM_EP + 4 * q);
                    a.x = fmaf(w, gv.x, a.x);
                    a.y = fmaf(w, gv.y, a.y);
                    a.z = fmaf(w, gv.z, a.z);
                    a.w = fmaf(w, gv.w, a.w);
                }
                float sc[4];
                dropout_scale4(drop, site, (uint64_t)(((size_t)b * f.S + s) * f.D + d0 + 4 * q), sc);
                float* o = dEt + s * TM_DT + 4 * q;
                o[0] = a.x * sc[0];
                o[1] = a.y * sc[1];
                o[2] = a.z * sc[2];
                o[3] = a.w * sc[3];
            }
        }
        __syncthreads();
        // ---- dWc: element (dd, c, k) = tid + 256 i of the workgroup's 16 x Kc x 3
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            if (e < TM_DT * K3) {
                const int dd = e / K3, ck = e - dd * K3, c = ck / 3, k = ck - 3 * c;
                float a = 0.f;
                for (int s = 0; s < f.S; ++s) {
                    int l = s + k - 1;
                    l = l < 0 ? l + f.S : (l >= f.S ? l - f.S : l);
                    a = fmaf(dEt[s * TM_DT + dd], in[l * Kc + c], a);
                }
                ac[i] += a;
            }
        }
    }
    if (tid < T) part_b[((size_t)sl * DTn + dt) * T + tid] = abp;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = tid + 256 * i;
        if (e < TM_DT * K3) {
            const int dd = e / K3;
            if (d0 + dd < f.D) part_c[(size_t)sl * f.D * K3 + (size_t)d0 * K3 + e] = ac[i];
        }
    }
}

// out = [dWp (T T) | dbp (T) | dWc (D Kc 3)], the partials added in workgroup order
__global__ __launch_bounds__(256) void timesnet_front_reduce_kernel(int T, int DK3, int np, int ns, const float* __restrict__ part_p,
                                                                     const float* __restrict__ part_b, const float* __restrict__ part_c,
                                                                     float* __restrict__ out) {
    const size_t TT = (size_t)T * T, N = TT + T + DK3;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (size_t)gridDim.x * 256) {
        const float* p;
        size_t stride;
        int n;
        if (i < TT) {
            p = part_p + i, stride = TT, n = np;
        } else if (i < TT + T) {
            p = part_b + (i - TT), stride = (size_t)T, n = np;
        } else {
            p = part_c + (i - TT - T), stride = (size_t)DK3, n = ns;
        }
        float a = 0.f;
#pragma unroll 8
        for (int s = 0; s < n; ++s) a += p[(size_t)s * stride];
        out[i] = a;
    }
}

DropCfg tm_drop(float p, uint64_t seed, const uint64_t* seed_dev) {
    DropCfg d = mk_drop(p, seed);
    d.seed_dev = seed_dev;
    return d;
}

}  // namespace

extern "C" {

int immtsf_timesnet_model_supported(int32_t input_len, int32_t pred_len, int32_t C, int32_t d_model) {
    if (input_len < 1 || pred_len < 1 || input_len > TM_TMAX || pred_len > TM_TMAX || input_len + pred_len > TM_TMAX) return 0;
    if (C < 1 || C > TM_CMAX) return 0;
    return d_model >= 4 && d_model <= TM_DMAX && d_model % 4 == 0;
}

size_t immtsf_timesnet_front_workspace_bytes(int32_t B, int32_t input_len, int32_t pred_len, int32_t C, int32_t d_model) {
    const TmDims f{B, 1, input_len, 1, pred_len, C, d_model};
    if (tm_bad(f)) return 0;
    const size_t ns = tm_slices(f), np = ns * cdiv(d_model, TM_DT), T = (size_t)input_len + pred_len;
    return (np * T * T + np * T + ns * d_model * (2 * C + 1) * 3) * sizeof(float);
}

int immtsf_timesnet_front_forward(int32_t B, int32_t L, int32_t input_len, int32_t Lp, int32_t pred_len, int32_t C, int32_t d_model,
                                  const float* data, const float* mask, const float* tp, const float* tpp, const float* W_token,
                                  const float* pe, const float* W_predict, const float* b_predict, float* means, float* stdev, float* enc,
                                  float* E_save, float p_drop, uint64_t seed, uint64_t site, const uint64_t* seed_step_dev,
                                  immtsf_stream_t stream) {
    const TmDims f{B, L, input_len, Lp, pred_len, C, d_model};
    if (!data || !mask || !tp || !tpp || !W_token || !pe || !W_predict || !b_predict || !means || !stdev || !enc) return IMMTSF_EINVAL;
    if (tm_bad(f)) return IMMTSF_EUNSUPPORTED;
    const int T = input_len + pred_len;
    const size_t lds = (size_t)fwd_lds_floats(input_len, pred_len, C) * sizeof(float);      // <= 58 KB
    hipLaunchKernelGGL(timesnet_front_fwd_kernel, dim3((unsigned)cdiv(T, TM_TT), (unsigned)cdiv(d_model, TM_DT), (unsigned)B), dim3(256), lds,
                       static_cast<hipStream_t>(stream), f, data, mask, tp, tpp, W_token, pe, W_predict, b_predict, means, stdev, enc, E_save,
                       tm_drop(p_drop, seed, seed_step_dev), site);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_timesnet_front_backward(int32_t B, int32_t L, int32_t input_len, int32_t Lp, int32_t pred_len, int32_t C, int32_t d_model,
                                   const float* data, const float* mask, const float* tp, const float* tpp, const float* W_token,
                                   const float* pe, const float* W_predict, const float* means, const float* stdev, const float* E_saved,
                                   const float* d_enc, float* dparams, float p_drop, uint64_t seed, uint64_t site,
                                   const uint64_t* seed_step_dev, void* workspace, size_t workspace_bytes, immtsf_stream_t stream) {
    const TmDims f{B, L, input_len, Lp, pred_len, C, d_model};
    if (!data || !mask || !tp || !tpp || !W_token || !pe || !W_predict || !means || !stdev || !d_enc || !dparams || !workspace)
        return IMMTSF_EINVAL;
    if (!al16(d_enc)) return IMMTSF_EINVAL;
    if (tm_bad(f)) return IMMTSF_EUNSUPPORTED;
    if (workspace_bytes < immtsf_timesnet_front_workspace_bytes(B, input_len, pred_len, C, d_model)) return IMMTSF_EWORKSPACE;
    const int ns = tm_slices(f), DTn = cdiv(d_model, TM_DT), T = input_len + pred_len, DK3 = d_model * (2 * C + 1) * 3;
    const size_t np = (size_t)ns * DTn;
    float* part_p = static_cast<float*>(workspace);
    float* part_b = part_p + np * T * T;
    float* part_c = part_b + np * T;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds = (size_t)bwd_lds_floats(input_len, pred_len, C) * sizeof(float);      // <= 84 KB
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(timesnet_front_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(timesnet_front_bwd_kernel, dim3((unsigned)DTn, (unsigned)ns), dim3(256), lds, s, f, ns, data, mask, tp, tpp, W_token, pe,
                       W_predict, means, stdev, E_saved, d_enc, part_p, part_b, part_c, tm_drop(p_drop, seed, seed_step_dev), site);
    IMMTSF_LAUNCH_CHECK();
    const size_t N = (size_t)T * T + T + DK3;
    hipLaunchKernelGGL(timesnet_front_reduce_kernel, dim3(grid_for(N, 256)), dim3(256), 0, s, T, DK3, (int)np, ns, part_p, part_b, part_c,
                       dparams);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
