// Informer's distilling ConvLayer (reference layers/Transformer_EncDec.py:6-24) behind its three-tap product: BatchNorm1d, ELU and
// MaxPool1d(3, 2, 1) on the ROWS y (B, T, d), T = L + 2, of the circular convolution's output -- no permuted copy -- into (B, Lo, d),
// Lo = (L + 1) / 2 + 1:   n = gamma (y - mean) rstd + beta,  a = n > 0 ? n : exp(n) - 1,  out[s] = max a[{2s-1, 2s, 2s+1} within [0, T)].
//
// Forward, training: the rows are dealt to <= CD_GMAX workgroups in contiguous shares; a thread per channel sums y and y^2 in double over
// its share (stage one), and the apply kernel folds the shares in index order (stage two), takes mean and the biased variance, updates
// running_mean / running_var (unbiased, momentum) and the batch counter IN PLACE -- no host scalar, so a captured graph replays it --
// then normalises, applies ELU and pools.  Evaluation: the apply kernel alone, on the running statistics.
// Backward: one kernel routes the pooled gradient to the FIRST maximum of every window (gathered: position t asks the one or two windows
// it belongs to), multiplies by ELU', writes dn and sums dn and dn xhat per share in double; the second folds them into dbeta, dgamma and
// writes dy = gamma rstd (dn - (dbeta + xhat dgamma) / R) (evaluation: gamma rstd dn).  Fixed orders throughout: two runs, same bits.
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

constexpr int CD_THREADS = 256;
constexpr int CD_GMAX = 64;       // most row shares of a reduction
constexpr int CD_MIN_SHARE = 8;   // fewest rows worth a share
constexpr int CD_ROWS = 16;       // rows per workgroup of the element-wise kernels

struct CdPlan { int G, share; };

inline CdPlan cd_plan(int64_t R) {
    int64_t G = (R + CD_MIN_SHARE - 1) / CD_MIN_SHARE;
    G = G < 1 ? 1 : (G > CD_GMAX ? CD_GMAX : G);
    const int64_t share = (R + G - 1) / G;
    return CdPlan{(int)((R + share - 1) / share), (int)share};
}

__device__ __forceinline__ float cd_elu(float n) { return n > 0.f ? n : expm1f(n); }

// grid (G, cdiv(d, 256)): part[g][0][c] = sum y, part[g][1][c] = sum y^2 over the rows of share g
__global__ __launch_bounds__(CD_THREADS) void cd_stats_kernel(int R, int d, int share, const float* __restrict__ y, double* __restrict__ part) {
    const int c = blockIdx.y * CD_THREADS + threadIdx.x;
    if (c >= d) return;
    const int r0 = blockIdx.x * share, r1 = min(R, r0 + share);
    double s1 = 0.0, s2 = 0.0;
    for (int r = r0; r < r1; ++r) {
        const double x = (double)y[(size_t)r * d + c];
        s1 += x;
        s2 += x * x;
    }
    part[((size_t)blockIdx.x * 2) * d + c] = s1;
    part[((size_t)blockIdx.x * 2 + 1) * d + c] = s2;
}

// grid (cdiv(B Lo, CD_ROWS), cdiv(d, 256))
__global__ __launch_bounds__(CD_THREADS) void cd_apply_kernel(int B, int T, int Lo, int d, int training, int G, const float* __restrict__ y,
                                                              const double* __restrict__ part, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, float momentum, float* running_mean,
                                                              float* running_var, long long* batches, float* __restrict__ mean_out,
                                                              float* __restrict__ rstd_out, float* __restrict__ out) {
    const int c = blockIdx.y * CD_THREADS + threadIdx.x;
    if (c >= d) return;
    float mean, rstd;
    if (training) {
        const double R = (double)B * T;
        double s1 = 0.0, s2 = 0.0;
        for (int g = 0; g < G; ++g) {
            s1 += part[((size_t)g * 2) * d + c];
            s2 += part[((size_t)g * 2 + 1) * d + c];
        }
        const double mu = s1 / R;
        double var = s2 / R - mu * mu;
        var = var > 0.0 ? var : 0.0;
        mean = (float)mu;
        rstd = (float)(1.0 / sqrt(var + (double)eps));
        if (blockIdx.x == 0) {      // one writer per channel; nobody reads the running statistics in training mode
            const float unb = (float)(R > 1.0 ? var * R / (R - 1.0) : var);
            running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
            running_var[c] = (1.f - momentum) * running_var[c] + momentum * unb;
            if (c == 0 && batches) *batches += 1;
        }
    } else {
        mean = running_mean[c];
        rstd = 1.f / sqrtf(running_var[c] + eps);
    }
    if (blockIdx.x == 0) { mean_out[c] = mean; rstd_out[c] = rstd; }
    const float w = gamma[c] * rstd, bb = beta[c] - mean * w;
    const int o0 = blockIdx.x * CD_ROWS, o1 = min(B * Lo, o0 + CD_ROWS);
    for (int o = o0; o < o1; ++o) {
        const int b = o / Lo, s = o - b * Lo;
        const float* yb = y + (size_t)b * T * d + c;
        float m = cd_elu(fmaf(yb[(size_t)(2 * s) * d], w, bb));      // 2 s <= T - 1 for every s < Lo
        if (s > 0) m = fmaxf(m, cd_elu(fmaf(yb[(size_t)(2 * s - 1) * d], w, bb)));
        if (2 * s + 1 < T) m = fmaxf(m, cd_elu(fmaf(yb[(size_t)(2 * s + 1) * d], w, bb)));
        out[(size_t)o * d + c] = m;
    }
}

// grid (G, cdiv(d, 256)): dn (B, T, d) and part[g][0][c] = sum dn, part[g][1][c] = sum dn xhat over the rows of share g
__global__ __launch_bounds__(CD_THREADS) void cd_bwd_route_kernel(int B, int T, int Lo, int d, int share, const float* __restrict__ y,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                  const float* __restrict__ dout, float* __restrict__ dn,
                                                                  double* __restrict__ part) {
    const int c = blockIdx.y * CD_THREADS + threadIdx.x;
    if (c >= d) return;
    const int R = B * T, r0 = blockIdx.x * share, r1 = min(R, r0 + share);
    const float mu = mean[c], rs = rstd[c], w = gamma[c] * rs, bb = beta[c] - mu * w;
    double s1 = 0.0, s2 = 0.0;
    for (int r = r0; r < r1; ++r) {
        const int b = r / T, t = r - b * T;
        const float* yb = y + (size_t)b * T * d + c;
        const float* gb = dout + (size_t)b * Lo * d + c;
        float a[5];      // a[t - 2 .. t + 2]; positions outside [0, T) are never compared
#pragma unroll
        for (int e = 0; e < 5; ++e) {
            const int p = t - 2 + e;
            a[e] = p >= 0 && p < T ? cd_elu(fmaf(yb[(size_t)p * d], w, bb)) : 0.f;
        }
        const float at = a[2];
        float g = 0.f;
        if ((t & 1) == 0) {      // the middle of window t / 2: beats t - 1 strictly, t + 1 on a tie
            const bool win = (t == 0 || at > a[1]) && (t + 1 >= T || at >= a[3]);
            if (win) g = gb[(size_t)(t >> 1) * d];
        } else {
            // the last of window (t - 1) / 2 (t - 1 >= 0 always, t - 2 may not exist) ...
            if ((t < 2 || at > a[0]) && at > a[1]) g = gb[(size_t)((t - 1) >> 1) * d];
            // ... and the first of window (t + 1) / 2 where that window exists (t + 1 < T then)
            const int s2w = (t + 1) >> 1;
            if (s2w < Lo && at >= a[3] && (t + 2 >= T || at >= a[4])) g += gb[(size_t)s2w * d];
        }
        const float yv = yb[(size_t)t * d], n = fmaf(yv, w, bb);
        const float v = g * (n > 0.f ? 1.f : expf(n));
        dn[(size_t)r * d + c] = v;
        s1 += (double)v;
        s2 += (double)v * (double)((yv - mu) * rs);
    }
    part[((size_t)blockIdx.x * 2) * d + c] = s1;
    part[((size_t)blockIdx.x * 2 + 1) * d + c] = s2;
}

// grid (cdiv(R, CD_ROWS), cdiv(d, 256))
__global__ __launch_bounds__(CD_THREADS) void cd_bwd_apply_kernel(int R, int d, int training, int G, const float* __restrict__ y,
                                                                  const float* __restrict__ gamma, const float* __restrict__ mean,
                                                                  const float* __restrict__ rstd, const float* __restrict__ dn,
                                                                  const double* __restrict__ part, float* __restrict__ dy,
                                                                  float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.y * CD_THREADS + threadIdx.x;
    if (c >= d) return;
    double s1 = 0.0, s2 = 0.0;
    for (int g = 0; g < G; ++g) {
        s1 += part[((size_t)g * 2) * d + c];
        s2 += part[((size_t)g * 2 + 1) * d + c];
    }
    if (blockIdx.x == 0) { dbeta[c] = (float)s1; dgamma[c] = (float)s2; }
    const float mu = mean[c], rs = rstd[c], w = gamma[c] * rs;
    const float m1 = training ? (float)(s1 / (double)R) : 0.f, m2 = training ? (float)(s2 / (double)R) : 0.f;
    const int r0 = blockIdx.x * CD_ROWS, r1 = min(R, r0 + CD_ROWS);
    for (int r = r0; r < r1; ++r) {
        const size_t o = (size_t)r * d + c;
        dy[o] = w * (dn[o] - m1 - (y[o] - mu) * rs * m2);
    }
}

inline bool cd_dims_ok(int64_t B, int L, int d) { return B >= 1 && L >= 2 && immtsf_conv_distil_supported(d) && B * ((int64_t)L + 2) < (1ll << 31) / 1024; }

}  // namespace

extern "C" {

int immtsf_conv_distil_supported(int32_t d) { return d >= 4 && d % 4 == 0 && d <= 1024 ? 1 : 0; }

size_t immtsf_conv_distil_workspace_bytes(int32_t B, int32_t L, int32_t d) {
    if (!cd_dims_ok(B, L, d)) return 0;
    return (size_t)cd_plan((int64_t)B * (L + 2)).G * 2 * d * sizeof(double) + 256;
}

int immtsf_conv_distil_forward(int32_t B, int32_t L, int32_t d, int32_t training, const float* y, const float* gamma, const float* beta,
                               float eps, float momentum, float* running_mean, float* running_var, int64_t* num_batches, float* mean,
                               float* rstd, float* out, void* workspace, size_t workspace_bytes, immtsf_stream_t stream) {
    if (d < 1 || L < 1 || B < 0) return IMMTSF_EINVAL;
    if (!immtsf_conv_distil_supported(d)) return IMMTSF_EUNSUPPORTED;
    if (B == 0) return IMMTSF_OK;
    if (!cd_dims_ok(B, L, d) || !y || !gamma || !beta || !running_mean || !running_var || !mean || !rstd || !out) return IMMTSF_EINVAL;
    const int T = L + 2, Lo = (L + 1) / 2 + 1, R = B * T;
    const CdPlan pl = cd_plan(R);
    double* part = nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (training) {
        if (!workspace) return IMMTSF_EINVAL;
        if (workspace_bytes < immtsf_conv_distil_workspace_bytes(B, L, d)) return IMMTSF_EWORKSPACE;
        part = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t(255));
        hipLaunchKernelGGL(cd_stats_kernel, dim3(pl.G, cdiv(d, CD_THREADS)), dim3(CD_THREADS), 0, s, R, d, pl.share, y, part);
        IMMTSF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(cd_apply_kernel, dim3(cdiv(B * Lo, CD_ROWS), cdiv(d, CD_THREADS)), dim3(CD_THREADS), 0, s, B, T, Lo, d, training ? 1 : 0,
                       pl.G, y, part, gamma, beta, eps, momentum, running_mean, running_var, reinterpret_cast<long long*>(num_batches), mean,
                       rstd, out);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_conv_distil_backward(int32_t B, int32_t L, int32_t d, int32_t training, const float* y, const float* gamma, const float* beta,
                                const float* mean, const float* rstd, const float* dout, float* dn, float* dy, float* dgamma, float* dbeta,
                                void* workspace, size_t workspace_bytes, immtsf_stream_t stream) {
    if (d < 1 || L < 1 || B < 0) return IMMTSF_EINVAL;
    if (!immtsf_conv_distil_supported(d)) return IMMTSF_EUNSUPPORTED;
    if (B == 0) return IMMTSF_OK;
    if (!cd_dims_ok(B, L, d) || !y || !gamma || !beta || !mean || !rstd || !dout || !dn || !dy || !dgamma || !dbeta || !workspace)
        return IMMTSF_EINVAL;
    if (workspace_bytes < immtsf_conv_distil_workspace_bytes(B, L, d)) return IMMTSF_EWORKSPACE;
    const int T = L + 2, Lo = (L + 1) / 2 + 1, R = B * T;
    const CdPlan pl = cd_plan(R);
    double* part = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t(255));
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cd_bwd_route_kernel, dim3(pl.G, cdiv(d, CD_THREADS)), dim3(CD_THREADS), 0, s, B, T, Lo, d, pl.share, y, gamma, beta, mean,
                       rstd, dout, dn, part);
    IMMTSF_LAUNCH_CHECK();
    hipLaunchKernelGGL(cd_bwd_apply_kernel, dim3(cdiv(R, CD_ROWS), cdiv(d, CD_THREADS)), dim3(CD_THREADS), 0, s, R, d, training ? 1 : 0, pl.G, y,
                       gamma, mean, rstd, dn, part, dy, dgamma, dbeta);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
