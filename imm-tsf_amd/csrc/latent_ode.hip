// The LatentODE backbone's forecasting() (reference models/LatentODE.py over lib/latent_ode_components: Encoder_z0_ODE_RNN.run_odernn,
// GRU_unit, DiffeqSolver with the fixed-grid 3/8-rule RK4, Decoder) as ONE launch forward and TWO launches backward, all fp32.
// R = rec_dims, U = units, G = gru_units, Z = latents, C channels, H = 100 (transform_z0's hidden width), IN = 2R + 2C.
//
// The batch shares one time axis, so every window has the same step plan: steps[i] / hs[i] for the observed point i, computed on the
// device by the caller (no host sync):  steps = -1: one Euler step y += hs f(y);  steps = n >= 1: n RK4 steps of length hs;  steps = 0:
// no ODE step (the L == 1 branch).  n is capped at LO_MAX_SUB.  With the state (y, s) = (0, 0), for i = L-1 .. 0:
//   ODE     f(y) = W3 tanh(W2 tanh(W1 y + b1) + b2) + b3 (the encoder's gradient net);  one RK4 step of length h (torchdiffeq's rk4, the
//           3/8 rule):  k1 = f(y), k2 = f(y + h k1 / 3), k3 = f(y + h (k2 - k1 / 3)), k4 = f(y + h (k1 - k2 + k3)),
//           y += h (k1 + 3 (k2 + k3) + k4) / 8
//   GRU     cat = [y, s, x_i, mask_i];  u = sigmoid(net_u(cat)), r = sigmoid(net_r(cat)), (n, v) = net_n([y r, s r, x_i, mask_i]);
//           y' = (1 - u) n + u y,  s' = (1 - u) |v| + u s  where any feature of point i is observed, (y, s) elsewhere;  s' = |s'|
// then  (mu, sg) = transform_z0([y, s]) (Linear, Tanh, Linear),  z_0 = mu + eps |sg|,  z_j = RK4 step of the generative net over
// tp_to_predict[j] - tp_to_predict[j-1],  out[:, j] = Wd z_j + bd  for j = 0 .. Lp-1.
//
// A workgroup of 256 threads owns a tile of LO_WT = 8 windows: the windows are the rows of every small product.  The weights sit in LDS
// as torch lays them out, (N, K) with rows K | 1 floats apart: the forward product (threads along n, walking k) and the transposed one
// of the backward (threads along k, walking n) both read 32 different banks, and the rows of every activation buffer are an odd number
// of floats apart too.  The encoder's nets (GRU, ODE) and the decoder's (transform_z0, generative ODE, decoder) take turns in the same
// LDS region.  Products are on the VALU: at R = U = 32 a layer has 256 outputs per tile, one per thread, and the launch is bound by its
// chain of barriers (16 per RK4 step, 9 per GRU update), not by arithmetic; fp32 MFMA 16x16x4 would leave half a tile of rows empty and
// shorten no barrier chain.
//
// Forward saves the state entering every observed point (and the final one) and the decode trajectory.  Backward, launch 1, runs time in
// reverse of the forward: the decode steps last to first (each rebuilt from the saved z_{j-1}, its four stages kept in LDS), transform_z0,
// then the observed points i = 0 .. L-1: the interval is rebuilt from the saved entering state with the forward's code, the state before
// every sub-step going onto the workgroup's stack in the workspace; the GRU update is rebuilt and pulled back (sign(0) = 0 for both
// abs), then the sub-steps last to first, each with its four stages rebuilt.  Parameter gradients go into the workgroup's slab of the
// workspace: every entry has one owner thread, steps are separated by barriers.  Launch 2 adds the slabs in index order: no atomics,
// the same inputs give the same bits.  Data, mask, times and eps take no gradient.
//
// LO_HOST_CHECK: the kernels compile as plain C++ with one thread per workgroup, so a host program can check the arithmetic.
#ifndef LO_HOST_CHECK
#include "../../include/immtsf.h"
#include "common.hpp"
#define LO_LDS_DECL extern __shared__ __align__(16) float lo_lds[]
#endif

namespace {

constexpr int LO_WT = 8;                   // windows of a workgroup
constexpr int LO_H = 100;                  // hidden width of transform_z0
constexpr int LO_MAX_SUB = 256;            // most RK4 steps of one interval
constexpr int LO_NL = 15;                  // Linear layers
#ifndef LO_HOST_CHECK
constexpr int LO_THREADS = 256;
#endif
constexpr int LO_MAX_RZ = 64, LO_MAX_UG = 128, LO_MAX_C = 64, LO_MAX_T = 1 << 20;
constexpr size_t LO_LDS_MAX = 160 * 1024;

enum { LU1, LU2, LR1, LR2, LN1, LN2, LE1, LE2, LE3, LT1, LT2, LG1, LG2, LG3, LDC };

// a Linear: weight (N, K) at goff of the flat parameters, bias behind it; in LDS at loff with rows ld apart, bias behind it
struct LoLin { int N, K, ld, goff, loff; };
struct LoPlan {
    int B, L, Lp, C, R, U, G, Z, IN;
    int ldc, ldw, ldu, ldr, ld2, ldo;      // row pitches: cat | hidden (G, H, U) | stage hidden (U) | R or Z | 2R or 2Z | C
    int NV, wfloats;                       // parameters in all; the LDS weight region
    LoLin l[LO_NL];
};

__host__ __device__ inline int lo_max(int a, int b) { return a > b ? a : b; }

inline LoPlan lo_plan(int B, int L, int Lp, int C, int R, int U, int G, int Z) {
    LoPlan p{};
    p.B = B; p.L = L; p.Lp = Lp; p.C = C; p.R = R; p.U = U; p.G = G; p.Z = Z; p.IN = 2 * R + 2 * C;
    const int nk[LO_NL][2] = {{G, p.IN}, {R, G}, {G, p.IN}, {R, G}, {G, p.IN}, {2 * R, G}, {U, R}, {U, U}, {R, U},
                              {LO_H, 2 * R}, {2 * Z, LO_H}, {U, Z}, {U, U}, {Z, U}, {C, Z}};
    int g = 0, lo = 0, wa = 0;
    for (int i = 0; i < LO_NL; ++i) {
        if (i == LT1) { wa = lo; lo = 0; }
        LoLin& l = p.l[i];
        l.N = nk[i][0]; l.K = nk[i][1]; l.ld = l.K | 1; l.goff = g; l.loff = lo;
        g += l.N * l.K + l.N;
        lo += l.N * l.ld + l.N;
    }
    p.NV = g;
    p.wfloats = (lo_max(wa, lo) + 3) & ~3;
    const int rz = lo_max(R, Z);
    p.ldc = p.IN | 1; p.ldw = lo_max(lo_max(U, G), LO_H) | 1; p.ldu = U | 1; p.ldr = rz | 1; p.ld2 = (2 * rz) | 1; p.ldo = C | 1;
    return p;
}

struct LoBuf {
    float *W, *cat, *cat2, *hu, *hr, *hn, *u, *r, *ns, *ks, *xs, *a1, *a2, *z, *co, *mk;      // both directions
    float *g, *gs, *gx, *gk, *gh1, *gh2, *gns, *gcat, *gu, *gr;                              // backward
};

// the activation buffers behind the weight region; returns the floats used.  The backward keeps all four stages of an RK4 step.
__host__ __device__ inline size_t lo_carve(const LoPlan& p, float* lds, bool bwd, LoBuf* s) {
    LoBuf t;
    float* v = lds + p.wfloats;
    const int T = LO_WT, st = bwd ? 4 : 1;
    t.W = lds;
    t.cat = v; v += T * p.ldc; t.cat2 = v; v += T * p.ldc;
    t.hu = v; v += T * p.ldw; t.hr = v; v += T * p.ldw; t.hn = v; v += T * p.ldw;
    t.u = v; v += T * p.ldr; t.r = v; v += T * p.ldr;
    t.ns = v; v += T * p.ld2;
    t.ks = v; v += 4 * T * p.ldr;
    t.xs = v; v += st * T * p.ldr;
    t.a1 = v; v += st * T * p.ldu; t.a2 = v; v += st * T * p.ldu;
    t.z = v; v += T * p.ldr;
    t.co = v; v += T * p.ldo;
    t.mk = v; v += T;
    t.g = t.gs = t.gx = t.gk = t.gh1 = t.gh2 = t.gns = t.gcat = t.gu = t.gr = nullptr;
    if (bwd) {
        t.g = v; v += T * p.ldr; t.gs = v; v += T * p.ldr; t.gx = v; v += T * p.ldr;
        t.gk = v; v += 4 * T * p.ldr;
        t.gh1 = v; v += T * p.ldw; t.gh2 = v; v += T * p.ldw;
        t.gns = v; v += T * p.ld2;
        t.gcat = v; v += T * p.ldc;
        t.gu = v; v += T * p.ldr; t.gr = v; v += T * p.ldr;
    }
    if (s) *s = t;
    return (size_t)(v - lds);
}
inline size_t lo_lds_bytes(const LoPlan& p, bool bwd) { return sizeof(float) * lo_carve(p, nullptr, bwd, nullptr); }

// the weights and biases of layers [first, last) from the flat parameters into LDS.  Starts and ends with a barrier.
__device__ void lo_load(const LoPlan& p, float* W, const float* __restrict__ prm, int first, int last) {
    __syncthreads();
    for (int i = first; i < last; ++i) {
        const LoLin l = p.l[i];
        for (int e = threadIdx.x; e < l.N * l.K; e += LO_THREADS) {
            const int n = e / l.K, k = e - n * l.K;
            W[l.loff + n * l.ld + k] = prm[l.goff + e];
        }
        for (int n = threadIdx.x; n < l.N; n += LO_THREADS) W[l.loff + l.N * l.ld + n] = prm[l.goff + l.N * l.K + n];
    }
    __syncthreads();
}

// out[w, n] = act(b[n] + sum_k in[w, k] W[n, k]);  ACT: 0 none, 1 tanh, 2 sigmoid.  Ends with a barrier.
template <int ACT>
__device__ void lo_lin(const float* Wl, const LoLin& l, const float* in, int ldi, float* out, int ldo) {
    const float *W = Wl + l.loff, *b = W + l.N * l.ld;
    for (int idx = threadIdx.x; idx < LO_WT * l.N; idx += LO_THREADS) {
        const int w = idx / l.N, n = idx - w * l.N;
        const float *x = in + w * ldi, *wr = W + n * l.ld;
        float a0 = b[n], a1 = 0.f;
        int k = 0;
        for (; k + 1 < l.K; k += 2) { a0 += x[k] * wr[k]; a1 += x[k + 1] * wr[k + 1]; }
        if (k < l.K) a0 += x[k] * wr[k];
        const float a = a0 + a1;
        out[w * ldo + n] = ACT == 1 ? tanhf(a) : ACT == 2 ? 1.f / (1.f + expf(-a)) : a;
    }
    __syncthreads();
}

// gin[w, k] = (acc ? gin[w, k] : 0) + (sum_n g[w, n] W[n, k]) (1 - act[w, k]^2 where act is given), k < Klim.  Ends with a barrier.
__device__ void lo_lin_t(const float* Wl, const LoLin& l, const float* g, int ldg, float* gin, int ldi, int Klim, const float* act, int lda,
                         bool acc) {
    const float* W = Wl + l.loff;
    for (int idx = threadIdx.x; idx < LO_WT * Klim; idx += LO_THREADS) {
        const int w = idx / Klim, k = idx - w * Klim;
        const float* gr = g + w * ldg;
        float a = 0.f;
        for (int n = 0; n < l.N; ++n) a += gr[n] * W[n * l.ld + k];
        if (act) { const float t = act[w * lda + k]; a *= 1.f - t * t; }
        gin[w * ldi + k] = acc ? gin[w * ldi + k] + a : a;
    }
    __syncthreads();
}

// slab[W] += g^T in, slab[b] += column sums of g, over the tile's windows.  One owner thread per entry.  No barrier: it only reads LDS.
__device__ void lo_wgrad(float* __restrict__ slab, const LoLin& l, const float* g, int ldg, const float* in, int ldi) {
    for (int e = threadIdx.x; e < l.N * l.K; e += LO_THREADS) {
        const int n = e / l.K, k = e - n * l.K;
        float a = 0.f;
        for (int w = 0; w < LO_WT; ++w) a += g[w * ldg + n] * in[w * ldi + k];
        slab[l.goff + e] += a;
    }
    for (int n = threadIdx.x; n < l.N; n += LO_THREADS) {
        float a = 0.f;
        for (int w = 0; w < LO_WT; ++w) a += g[w * ldg + n];
        slab[l.goff + l.N * l.K + n] += a;
    }
}

// k = f(x) of the net of layers l0, l0+1, l0+2; a1, a2: its hidden activations (pitch ldu)
__device__ void lo_net(const LoPlan& p, const float* W, int l0, const float* x, int ldx, float* a1, float* a2, float* k) {
    lo_lin<1>(W, p.l[l0], x, ldx, a1, p.ldu);
    lo_lin<1>(W, p.l[l0 + 1], a1, p.ldu, a2, p.ldu);
    lo_lin<0>(W, p.l[l0 + 2], a2, p.ldu, k, p.ldr);
}

// one RK4 step of length h on y (D wide, pitch ldy).  save: every stage keeps its input (xs; stage 1 reads y) and hidden activations.
// update: y takes the step.  Ends with a barrier.
__device__ void lo_rk4(const LoPlan& p, const LoBuf& s, int l0, float* y, int ldy, int D, float h, bool save, bool update) {
    const int T = LO_WT, sx = save ? T * p.ldr : 0, sa = save ? T * p.ldu : 0;
    float *k1 = s.ks, *k2 = k1 + T * p.ldr, *k3 = k2 + T * p.ldr, *k4 = k3 + T * p.ldr;
    lo_net(p, s.W, l0, y, ldy, s.a1, s.a2, k1);
    float* x = s.xs + sx;
    for (int idx = threadIdx.x; idx < T * D; idx += LO_THREADS) {
        const int w = idx / D, j = idx - w * D;
        x[w * p.ldr + j] = y[w * ldy + j] + h * k1[w * p.ldr + j] * (1.f / 3.f);
    }
    __syncthreads();
    lo_net(p, s.W, l0, x, p.ldr, s.a1 + sa, s.a2 + sa, k2);
    x = s.xs + 2 * sx;
    for (int idx = threadIdx.x; idx < T * D; idx += LO_THREADS) {
        const int w = idx / D, j = idx - w * D;
        x[w * p.ldr + j] = y[w * ldy + j] + h * (k2[w * p.ldr + j] - k1[w * p.ldr + j] * (1.f / 3.f));
    }
    __syncthreads();
    lo_net(p, s.W, l0, x, p.ldr, s.a1 + 2 * sa, s.a2 + 2 * sa, k3);
    x = s.xs + 3 * sx;
    for (int idx = threadIdx.x; idx < T * D; idx += LO_THREADS) {
        const int w = idx / D, j = idx - w * D;
        x[w * p.ldr + j] = y[w * ldy + j] + h * (k1[w * p.ldr + j] - k2[w * p.ldr + j] + k3[w * p.ldr + j]);
    }
    __syncthreads();
    lo_net(p, s.W, l0, x, p.ldr, s.a1 + 3 * sa, s.a2 + 3 * sa, k4);
    if (update) {
        for (int idx = threadIdx.x; idx < T * D; idx += LO_THREADS) {
            const int w = idx / D, j = idx - w * D, o = w * p.ldr + j;
            y[w * ldy + j] += (k1[o] + 3.f * (k2[o] + k3[o]) + k4[o]) * h * 0.125f;
        }
        __syncthreads();
    }
}

// the x and mask columns of cat for point i, the "any feature observed" flags, both gates, the reset state and the new-state net.
// combine: (y, s) in cat take the update; the backward leaves them as they entered.  Ends with a barrier.
__device__ void lo_gru(const LoPlan& p, const LoBuf& s, const float* __restrict__ data, const float* __restrict__ mask, int b0, int i,
                       bool combine) {
    const int T = LO_WT, R = p.R, C = p.C;
    for (int idx = threadIdx.x; idx < T * C; idx += LO_THREADS) {
        const int w = idx / C, c = idx - w * C, b = b0 + w;
        const size_t at = ((size_t)b * p.L + i) * C + c;
        s.cat[w * p.ldc + 2 * R + c] = b < p.B ? data[at] : 0.f;
        s.cat[w * p.ldc + 2 * R + C + c] = b < p.B ? mask[at] : 0.f;
    }
    __syncthreads();
    for (int w = threadIdx.x; w < T; w += LO_THREADS) {
        float a = 0.f;
        for (int c = 0; c < C; ++c) a += s.cat[w * p.ldc + 2 * R + C + c];
        s.mk[w] = a > 0.f ? 1.f : 0.f;
    }
    lo_lin<1>(s.W, p.l[LU1], s.cat, p.ldc, s.hu, p.ldw);
    lo_lin<2>(s.W, p.l[LU2], s.hu, p.ldw, s.u, p.ldr);
    lo_lin<1>(s.W, p.l[LR1], s.cat, p.ldc, s.hr, p.ldw);
    lo_lin<2>(s.W, p.l[LR2], s.hr, p.ldw, s.r, p.ldr);
    for (int idx = threadIdx.x; idx < T * p.IN; idx += LO_THREADS) {
        const int w = idx / p.IN, j = idx - w * p.IN;
        float v = s.cat[w * p.ldc + j];
        if (j < 2 * R) v *= s.r[w * p.ldr + (j < R ? j : j - R)];
        s.cat2[w * p.ldc + j] = v;
    }
    __syncthreads();
    lo_lin<1>(s.W, p.l[LN1], s.cat2, p.ldc, s.hn, p.ldw);
    lo_lin<0>(s.W, p.l[LN2], s.hn, p.ldw, s.ns, p.ld2);
    if (!combine) return;
    for (int idx = threadIdx.x; idx < T * R; idx += LO_THREADS) {
        const int w = idx / R, j = idx - w * R;
        float y = s.cat[w * p.ldc + j], sd = s.cat[w * p.ldc + R + j];
        if (s.mk[w] != 0.f) {
            const float u = s.u[w * p.ldr + j];
            y = (1.f - u) * s.ns[w * p.ld2 + j] + u * y;
            sd = (1.f - u) * fabsf(s.ns[w * p.ld2 + R + j]) + u * sd;
        }
        s.cat[w * p.ldc + j] = y;
        s.cat[w * p.ldc + R + j] = fabsf(sd);
    }
    __syncthreads();
}

// [y, s] (the first 2R columns of cat) -> zz = transform_z0 (hidden in hu, zz in ns)
__device__ void lo_transform(const LoPlan& p, const LoBuf& s) {
    lo_lin<1>(s.W, p.l[LT1], s.cat, p.ldc, s.hu, p.ldw);
    lo_lin<0>(s.W, p.l[LT2], s.hu, p.ldw, s.ns, p.ld2);
}

__device__ inline float lo_sgn(float x) { return x > 0.f ? 1.f : x < 0.f ? -1.f : 0.f; }

__global__ __launch_bounds__(LO_THREADS) void lo_fwd_kernel(LoPlan p, const float* __restrict__ data, const float* __restrict__ mask,
                                                           const int32_t* __restrict__ steps, const float* __restrict__ hs,
                                                           const float* __restrict__ tpp, const float* __restrict__ prm,
                                                           const float* __restrict__ eps, float* __restrict__ out,
                                                           float* __restrict__ states, float* __restrict__ traj) {
    LO_LDS_DECL;
    LoBuf s;
    lo_carve(p, lo_lds, false, &s);
    const int T = LO_WT, b0 = blockIdx.x * T, R = p.R, Z = p.Z, C = p.C, L = p.L, Lp = p.Lp;
    for (int idx = threadIdx.x; idx < T * p.ldc; idx += LO_THREADS) s.cat[idx] = 0.f;
    lo_load(p, s.W, prm, LU1, LT1);
    for (int q = 0; q <= L; ++q) {
        for (int idx = threadIdx.x; idx < T * 2 * R; idx += LO_THREADS) {      // the state entering point L-1-q; q = L: the last one
            const int w = idx / (2 * R), j = idx - w * 2 * R;
            if (b0 + w < p.B) states[((size_t)(b0 + w) * (L + 1) + q) * 2 * R + j] = s.cat[w * p.ldc + j];
        }
        if (q == L) break;
        const int i = L - 1 - q;
        int n = steps[i];
        const float h = hs[i];
        n = n > LO_MAX_SUB ? LO_MAX_SUB : n;
        if (n < 0) {
            lo_net(p, s.W, LE1, s.cat, p.ldc, s.a1, s.a2, s.ks);
            for (int idx = threadIdx.x; idx < T * R; idx += LO_THREADS) {
                const int w = idx / R, j = idx - w * R;
                s.cat[w * p.ldc + j] += h * s.ks[w * p.ldr + j];
            }
            __syncthreads();
        }
        for (int k = 0; k < n; ++k) lo_rk4(p, s, LE1, s.cat, p.ldc, R, h, false, true);
        lo_gru(p, s, data, mask, b0, i, true);
    }
    lo_load(p, s.W, prm, LT1, LO_NL);
    lo_transform(p, s);
    for (int idx = threadIdx.x; idx < T * Z; idx += LO_THREADS) {
        const int w = idx / Z, j = idx - w * Z, b = b0 + w;
        const float e = b < p.B ? eps[(size_t)b * Z + j] : 0.f;
        s.z[w * p.ldr + j] = s.ns[w * p.ld2 + j] + e * fabsf(s.ns[w * p.ld2 + Z + j]);
    }
    __syncthreads();
    for (int jt = 0; jt < Lp; ++jt) {
        if (jt > 0) lo_rk4(p, s, LG1, s.z, p.ldr, Z, tpp[jt] - tpp[jt - 1], false, true);
        lo_lin<0>(s.W, p.l[LDC], s.z, p.ldr, s.co, p.ldo);
        for (int idx = threadIdx.x; idx < T * Z; idx += LO_THREADS) {
            const int w = idx / Z, j = idx - w * Z;
            if (b0 + w < p.B) traj[((size_t)(b0 + w) * Lp + jt) * Z + j] = s.z[w * p.ldr + j];
        }
        for (int idx = threadIdx.x; idx < T * C; idx += LO_THREADS) {
            const int w = idx / C, c = idx - w * C;
            if (b0 + w < p.B) out[((size_t)(b0 + w) * Lp + jt) * C + c] = s.co[w * p.ldo + c];
        }
        __syncthreads();
    }
}

// the net of layers l0 .. l0+2 backwards: gk (pitch ldr) the cotangent of its output, x / a1 / a2 the stage's input and hidden
// activations -> gx (pitch ldr), the cotangent of x; the parameter gradients into the slab.  Ends with a barrier.
__device__ void lo_net_bwd(const LoPlan& p, const LoBuf& s, float* slab, int l0, const float* x, int ldx, const float* a1, const float* a2,
                           const float* gk, float* gx) {
    lo_wgrad(slab, p.l[l0 + 2], gk, p.ldr, a2, p.ldu);
    lo_lin_t(s.W, p.l[l0 + 2], gk, p.ldr, s.gh2, p.ldw, p.l[l0 + 2].K, a2, p.ldu, false);
    lo_wgrad(slab, p.l[l0 + 1], s.gh2, p.ldw, a1, p.ldu);
    lo_lin_t(s.W, p.l[l0 + 1], s.gh2, p.ldw, s.gh1, p.ldw, p.l[l0 + 1].K, a1, p.ldu, false);
    lo_wgrad(slab, p.l[l0], s.gh1, p.ldw, x, ldx);
    lo_lin_t(s.W, p.l[l0], s.gh1, p.ldw, gx, p.ldr, p.l[l0].K, nullptr, 0, false);
}

// the RK4 step that lo_rk4(save) just rebuilt from y0, backwards: s.g holds the cotangent of the step's result on entry and of y0 on exit
__device__ void lo_rk4_bwd(const LoPlan& p, const LoBuf& s, float* slab, int l0, const float* y0, int ldy, int D, float h) {
    const int T = LO_WT, sx = T * p.ldr, sa = T * p.ldu;
    float *g1 = s.gk, *g2 = g1 + sx, *g3 = g2 + sx, *g4 = g3 + sx;
    for (int idx = threadIdx.x; idx < T * D; idx += LO_THREADS) {
        const int w = idx / D, j = idx - w * D, o = w * p.ldr + j;
        const float g = s.g[o] * h * 0.125f;
        g1[o] = g; g2[o] = 3.f * g; g3[o] = 3.f * g; g4[o] = g;
    }
    __syncthreads();
    lo_net_bwd(p, s, slab, l0, s.xs + 3 * sx, p.ldr, s.a1 + 3 * sa, s.a2 + 3 * sa, g4, s.gx);
    for (int idx = threadIdx.x; idx < T * D; idx += LO_THREADS) {
        const int w = idx / D, j = idx - w * D, o = w * p.ldr + j;
        const float gx = s.gx[o];
        s.g[o] += gx; g1[o] += h * gx; g2[o] -= h * gx; g3[o] += h * gx;
    }
    __syncthreads();
    lo_net_bwd(p, s, slab, l0, s.xs + 2 * sx, p.ldr, s.a1 + 2 * sa, s.a2 + 2 * sa, g3, s.gx);
    for (int idx = threadIdx.x; idx < T * D; idx += LO_THREADS) {
        const int w = idx / D, j = idx - w * D, o = w * p.ldr + j;
        const float gx = s.gx[o];
        s.g[o] += gx; g2[o] += h * gx; g1[o] -= h * gx * (1.f / 3.f);
    }
    __syncthreads();
    lo_net_bwd(p, s, slab, l0, s.xs + sx, p.ldr, s.a1 + sa, s.a2 + sa, g2, s.gx);
    for (int idx = threadIdx.x; idx < T * D; idx += LO_THREADS) {
        const int w = idx / D, j = idx - w * D, o = w * p.ldr + j;
        const float gx = s.gx[o];
        s.g[o] += gx; g1[o] += h * gx * (1.f / 3.f);
    }
    __syncthreads();
    lo_net_bwd(p, s, slab, l0, y0, ldy, s.a1, s.a2, g1, s.gx);
    for (int idx = threadIdx.x; idx < T * D; idx += LO_THREADS) {
        const int w = idx / D, j = idx - w * D, o = w * p.ldr + j;
        s.g[o] += s.gx[o];
    }
    __syncthreads();
}

// the GRU update that lo_gru(combine = false) just rebuilt, backwards: s.g / s.gs hold the cotangents of (y', s') on entry and of the
// (y, s) that entered the update on exit
__device__ void lo_gru_bwd(const LoPlan& p, const LoBuf& s, float* slab) {
    const int T = LO_WT, R = p.R;
    for (int idx = threadIdx.x; idx < T * R; idx += LO_THREADS) {
        const int w = idx / R, j = idx - w * R, o = w * p.ldr + j;
        const float y = s.cat[w * p.ldc + j], sd = s.cat[w * p.ldc + R + j], gy = s.g[o], gsd = s.gs[o];
        if (s.mk[w] != 0.f) {
            const float u = s.u[o], nw = s.ns[w * p.ld2 + j], vr = s.ns[w * p.ld2 + R + j], v = fabsf(vr);
            const float gt = gsd * lo_sgn((1.f - u) * v + u * sd);
            s.gns[w * p.ld2 + j] = gy * (1.f - u);
            s.gns[w * p.ld2 + R + j] = gt * (1.f - u) * lo_sgn(vr);
            s.gu[o] = (gy * (y - nw) + gt * (sd - v)) * u * (1.f - u);
            s.g[o] = gy * u;
            s.gs[o] = gt * u;
        } else {
            s.gns[w * p.ld2 + j] = 0.f;
            s.gns[w * p.ld2 + R + j] = 0.f;
            s.gu[o] = 0.f;
            s.gs[o] = gsd * lo_sgn(sd);
        }
    }
    __syncthreads();
    lo_wgrad(slab, p.l[LN2], s.gns, p.ld2, s.hn, p.ldw);
    lo_lin_t(s.W, p.l[LN2], s.gns, p.ld2, s.gh1, p.ldw, p.G, s.hn, p.ldw, false);
    lo_wgrad(slab, p.l[LN1], s.gh1, p.ldw, s.cat2, p.ldc);
    lo_lin_t(s.W, p.l[LN1], s.gh1, p.ldw, s.gcat, p.ldc, 2 * R, nullptr, 0, false);
    for (int idx = threadIdx.x; idx < T * R; idx += LO_THREADS) {
        const int w = idx / R, j = idx - w * R, o = w * p.ldr + j;
        const float c1 = s.gcat[w * p.ldc + j], c2 = s.gcat[w * p.ldc + R + j], r = s.r[o];
        s.g[o] += c1 * r;
        s.gs[o] += c2 * r;
        s.gr[o] = (c1 * s.cat[w * p.ldc + j] + c2 * s.cat[w * p.ldc + R + j]) * r * (1.f - r);
    }
    __syncthreads();
    lo_wgrad(slab, p.l[LR2], s.gr, p.ldr, s.hr, p.ldw);
    lo_lin_t(s.W, p.l[LR2], s.gr, p.ldr, s.gh1, p.ldw, p.G, s.hr, p.ldw, false);
    lo_wgrad(slab, p.l[LR1], s.gh1, p.ldw, s.cat, p.ldc);
    lo_lin_t(s.W, p.l[LR1], s.gh1, p.ldw, s.gcat, p.ldc, 2 * R, nullptr, 0, false);
    lo_wgrad(slab, p.l[LU2], s.gu, p.ldr, s.hu, p.ldw);
    lo_lin_t(s.W, p.l[LU2], s.gu, p.ldr, s.gh2, p.ldw, p.G, s.hu, p.ldw, false);
    lo_wgrad(slab, p.l[LU1], s.gh2, p.ldw, s.cat, p.ldc);
    lo_lin_t(s.W, p.l[LU1], s.gh2, p.ldw, s.gcat, p.ldc, 2 * R, nullptr, 0, true);
    for (int idx = threadIdx.x; idx < T * R; idx += LO_THREADS) {
        const int w = idx / R, j = idx - w * R, o = w * p.ldr + j;
        s.g[o] += s.gcat[w * p.ldc + j];
        s.gs[o] += s.gcat[w * p.ldc + R + j];
    }
    __syncthreads();
}

__global__ __launch_bounds__(LO_THREADS) void lo_bwd_kernel(LoPlan p, const float* __restrict__ data, const float* __restrict__ mask,
                                                           const int32_t* __restrict__ steps, const float* __restrict__ hs,
                                                           const float* __restrict__ tpp, const float* __restrict__ prm,
                                                           const float* __restrict__ eps, const float* __restrict__ states,
                                                           const float* __restrict__ traj, const float* __restrict__ dout,
                                                           float* __restrict__ slabs, float* __restrict__ stacks) {
    LO_LDS_DECL;
    LoBuf s;
    lo_carve(p, lo_lds, true, &s);
    const int T = LO_WT, b0 = blockIdx.x * T, R = p.R, Z = p.Z, C = p.C, L = p.L, Lp = p.Lp;
    float* slab = slabs + (size_t)blockIdx.x * p.NV;
    float* stack = stacks + (size_t)blockIdx.x * LO_MAX_SUB * T * R;
    for (int e = threadIdx.x; e < p.NV; e += LO_THREADS) slab[e] = 0.f;
    for (int idx = threadIdx.x; idx < T * p.ldr; idx += LO_THREADS) s.g[idx] = 0.f;
    lo_load(p, s.W, prm, LT1, LO_NL);
    // ---- the decode steps, last to first: s.g = the cotangent of z_jt
    for (int jt = Lp - 1; jt >= 0; --jt) {
        for (int idx = threadIdx.x; idx < T * C; idx += LO_THREADS) {
            const int w = idx / C, c = idx - w * C;
            s.co[w * p.ldo + c] = b0 + w < p.B ? dout[((size_t)(b0 + w) * Lp + jt) * C + c] : 0.f;
        }
        for (int idx = threadIdx.x; idx < T * Z; idx += LO_THREADS) {
            const int w = idx / Z, j = idx - w * Z;
            s.u[w * p.ldr + j] = b0 + w < p.B ? traj[((size_t)(b0 + w) * Lp + jt) * Z + j] : 0.f;                // z_jt
            if (jt > 0) s.z[w * p.ldr + j] = b0 + w < p.B ? traj[((size_t)(b0 + w) * Lp + jt - 1) * Z + j] : 0.f;  // z_{jt-1}
        }
        __syncthreads();
        lo_wgrad(slab, p.l[LDC], s.co, p.ldo, s.u, p.ldr);
        lo_lin_t(s.W, p.l[LDC], s.co, p.ldo, s.g, p.ldr, Z, nullptr, 0, true);
        if (jt == 0) break;
        const float h = tpp[jt] - tpp[jt - 1];
        lo_rk4(p, s, LG1, s.z, p.ldr, Z, h, true, false);
        lo_rk4_bwd(p, s, slab, LG1, s.z, p.ldr, Z, h);
    }
    // ---- z_0 = mu + eps |sg|, transform_z0
    for (int idx = threadIdx.x; idx < T * 2 * R; idx += LO_THREADS) {
        const int w = idx / (2 * R), j = idx - w * 2 * R;
        s.cat[w * p.ldc + j] = b0 + w < p.B ? states[((size_t)(b0 + w) * (L + 1) + L) * 2 * R + j] : 0.f;
    }
    __syncthreads();
    lo_transform(p, s);
    for (int idx = threadIdx.x; idx < T * Z; idx += LO_THREADS) {
        const int w = idx / Z, j = idx - w * Z, b = b0 + w;
        const float e = b < p.B ? eps[(size_t)b * Z + j] : 0.f, g = s.g[w * p.ldr + j];
        s.gns[w * p.ld2 + j] = g;
        s.gns[w * p.ld2 + Z + j] = g * e * lo_sgn(s.ns[w * p.ld2 + Z + j]);
    }
    __syncthreads();
    lo_wgrad(slab, p.l[LT2], s.gns, p.ld2, s.hu, p.ldw);
    lo_lin_t(s.W, p.l[LT2], s.gns, p.ld2, s.gh1, p.ldw, LO_H, s.hu, p.ldw, false);
    lo_wgrad(slab, p.l[LT1], s.gh1, p.ldw, s.cat, p.ldc);
    lo_lin_t(s.W, p.l[LT1], s.gh1, p.ldw, s.gcat, p.ldc, 2 * R, nullptr, 0, false);
    for (int idx = threadIdx.x; idx < T * R; idx += LO_THREADS) {
        const int w = idx / R, j = idx - w * R;
        s.g[w * p.ldr + j] = s.gcat[w * p.ldc + j];
        s.gs[w * p.ldr + j] = s.gcat[w * p.ldc + R + j];
    }
    lo_load(p, s.W, prm, LU1, LT1);
    // ---- the observed points, first to last (the forward walked them last to first)
    for (int q = L - 1; q >= 0; --q) {
        const int i = L - 1 - q;
        int n = steps[i];
        const float h = hs[i];
        n = n > LO_MAX_SUB ? LO_MAX_SUB : n;
        for (int idx = threadIdx.x; idx < T * 2 * R; idx += LO_THREADS) {
            const int w = idx / (2 * R), j = idx - w * 2 * R;
            const float v = b0 + w < p.B ? states[((size_t)(b0 + w) * (L + 1) + q) * 2 * R + j] : 0.f;
            s.cat[w * p.ldc + j] = v;
            if (j < R) s.z[w * p.ldr + j] = v;
        }
        __syncthreads();
        if (n < 0) {                                                   // Euler: its stage stays in slot 0 until it is pulled back
            lo_net(p, s.W, LE1, s.z, p.ldr, s.a1, s.a2, s.ks);
            for (int idx = threadIdx.x; idx < T * R; idx += LO_THREADS) {
                const int w = idx / R, j = idx - w * R;
                s.cat[w * p.ldc + j] += h * s.ks[w * p.ldr + j];
            }
            __syncthreads();
        }
        for (int k = 0; k < n; ++k) {
            for (int idx = threadIdx.x; idx < T * R; idx += LO_THREADS) {
                const int w = idx / R, j = idx - w * R;
                stack[(size_t)k * T * R + idx] = s.cat[w * p.ldc + j];
            }
            lo_rk4(p, s, LE1, s.cat, p.ldc, R, h, false, true);
        }
        lo_gru(p, s, data, mask, b0, i, false);
        lo_gru_bwd(p, s, slab);
        if (n < 0) {
            for (int idx = threadIdx.x; idx < T * R; idx += LO_THREADS) {
                const int w = idx / R, j = idx - w * R;
                s.gk[w * p.ldr + j] = h * s.g[w * p.ldr + j];
            }
            __syncthreads();
            lo_net_bwd(p, s, slab, LE1, s.z, p.ldr, s.a1, s.a2, s.gk, s.gx);
            for (int idx = threadIdx.x; idx < T * R; idx += LO_THREADS) {
                const int w = idx / R, j = idx - w * R;
                s.g[w * p.ldr + j] += s.gx[w * p.ldr + j];
            }
            __syncthreads();
        }
        for (int k = n - 1; k >= 0; --k) {
            for (int idx = threadIdx.x; idx < T * R; idx += LO_THREADS) {
                const int w = idx / R, j = idx - w * R;
                s.z[w * p.ldr + j] = stack[(size_t)k * T * R + idx];
            }
            __syncthreads();
            lo_rk4(p, s, LE1, s.z, p.ldr, R, h, true, false);
            lo_rk4_bwd(p, s, slab, LE1, s.z, p.ldr, R, h);
        }
    }
}

#ifndef LO_HOST_CHECK
__global__ __launch_bounds__(LO_THREADS) void lo_fold_kernel(int NV, int nwg, const float* __restrict__ slabs, float* __restrict__ grads) {
    const int i = blockIdx.x * LO_THREADS + threadIdx.x;
    if (i >= NV) return;
    float a = 0.f;
    for (int b = 0; b < nwg; ++b) a += slabs[(size_t)b * NV + i];
    grads[i] = a;
}

bool lo_dims_ok(const immtsf_latent_ode_dims* d) {
    return d && d->L >= 1 && d->L <= LO_MAX_T && d->Lp >= 1 && d->Lp <= LO_MAX_T && d->C >= 1 && d->C <= LO_MAX_C && d->rec_dims >= 1 &&
           d->rec_dims <= LO_MAX_RZ && d->latents >= 1 && d->latents <= LO_MAX_RZ && d->units >= 1 && d->units <= LO_MAX_UG &&
           d->gru_units >= 1 && d->gru_units <= LO_MAX_UG;
}
LoPlan lo_plan_of(const immtsf_latent_ode_dims* d) {
    return lo_plan(d->B, d->L, d->Lp, d->C, d->rec_dims, d->units, d->gru_units, d->latents);
}
bool lo_call_ok(const immtsf_latent_ode_dims* d) {
    if (!immtsf_latent_ode_supported(d) || d->B < 1) return false;
    const int64_t widest = lo_max(lo_max(2 * d->rec_dims, d->latents), d->C);
    return (int64_t)d->B * ((int64_t)lo_max(d->L + 1, d->Lp)) * widest < (1ll << 31);
}
#endif

}  // namespace

#ifndef LO_HOST_CHECK
extern "C" {

int immtsf_latent_ode_supported(const immtsf_latent_ode_dims* dims) {
    if (!lo_dims_ok(dims) || dims->B < 0) return 0;
    return lo_lds_bytes(lo_plan_of(dims), true) <= LO_LDS_MAX;
}

int32_t immtsf_latent_ode_param_count(const immtsf_latent_ode_dims* dims) {
    if (!lo_dims_ok(dims)) return -1;
    return lo_plan_of(dims).NV;
}

size_t immtsf_latent_ode_workspace_bytes(const immtsf_latent_ode_dims* dims) {
    if (!lo_call_ok(dims)) return 0;
    const LoPlan p = lo_plan_of(dims);
    const size_t nwg = (size_t)cdiv(p.B, LO_WT);
    return sizeof(float) * (((nwg * p.NV + 63) & ~size_t(63)) + nwg * LO_MAX_SUB * LO_WT * p.R) + 256;
}

int immtsf_latent_ode_forward(const immtsf_latent_ode_dims* dims, const float* data, const float* mask, const int32_t* steps,
                              const float* step_len, const float* tp_pred, const float* params, const float* eps, float* out,
                              float* states, float* traj, immtsf_stream_t stream) {
    if (!dims || dims->B < 0) return IMMTSF_EINVAL;
    if (!immtsf_latent_ode_supported(dims)) return IMMTSF_EUNSUPPORTED;
    if (dims->B == 0) return IMMTSF_OK;
    if (!lo_call_ok(dims)) return IMMTSF_EINVAL;
    if (!data || !mask || !steps || !step_len || !tp_pred || !params || !eps || !out || !states || !traj) return IMMTSF_EINVAL;
    const LoPlan p = lo_plan_of(dims);
    const size_t lds = lo_lds_bytes(p, false);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lo_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(lo_fwd_kernel, dim3(cdiv(p.B, LO_WT)), dim3(LO_THREADS), lds, static_cast<hipStream_t>(stream), p, data, mask, steps,
                       step_len, tp_pred, params, eps, out, states, traj);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_latent_ode_backward(const immtsf_latent_ode_dims* dims, const float* data, const float* mask, const int32_t* steps,
                               const float* step_len, const float* tp_pred, const float* params, const float* eps, const float* states,
                               const float* traj, const float* d_out, float* grads, void* workspace, size_t workspace_bytes,
                               immtsf_stream_t stream) {
    if (!dims || dims->B < 1) return IMMTSF_EINVAL;
    if (!immtsf_latent_ode_supported(dims)) return IMMTSF_EUNSUPPORTED;
    if (!lo_call_ok(dims)) return IMMTSF_EINVAL;
    if (!data || !mask || !steps || !step_len || !tp_pred || !params || !eps || !states || !traj || !d_out || !grads || !workspace)
        return IMMTSF_EINVAL;
    if (workspace_bytes < immtsf_latent_ode_workspace_bytes(dims)) return IMMTSF_EWORKSPACE;
    const LoPlan p = lo_plan_of(dims);
    const int nwg = cdiv(p.B, LO_WT);
    float* ws = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t(255));
    float* stacks = ws + (((size_t)nwg * p.NV + 63) & ~size_t(63));
    const size_t lds = lo_lds_bytes(p, true);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lo_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(lo_bwd_kernel, dim3(nwg), dim3(LO_THREADS), lds, s, p, data, mask, steps, step_len, tp_pred, params, eps, states, traj,
                       d_out, ws, stacks);
    IMMTSF_LAUNCH_CHECK();
    hipLaunchKernelGGL(lo_fold_kernel, dim3(cdiv(p.NV, LO_THREADS)), dim3(LO_THREADS), 0, s, p.NV, nwg, ws, grads);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
#endif
