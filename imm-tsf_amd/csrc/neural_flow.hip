// The NeuralFlow backbone's forecasting() (reference models/NeuralFlow.py over lib/neural_flow_components: Encoder_z0_ODE_RNN.run_odernn
// with an LSTM cell, the coupling flow of models/flow.py, LatentODE.get_reconstruction, Decoder) as TWO launches forward and THREE
// backward, all fp32.  R = rec_dims, Z = latents, Hd = hidden_dim, HL = hidden_layers, NF = flow_layers, C channels, 100 = the hidden
// width of transform_z0.
//
// A coupling flow of width D at time t (one t per row), for layer i = 0 .. NF-1 with the mask m = ordered_{i % 2} (m_j = 1 for
// j < D / 2 where i is even, for j >= D / 2 where i is odd; all zero where D == 1):
//   (s, b) = MLP([x m, t])  (HL hidden Linears with Tanh, a last Linear to 2D),  phi = scale t  (TimeLinear, scale 2D wide) or
//   tanhf(scale t)  (TimeTanh; the time net is the template argument TN of the four kernels that form phi, one instance each),
//   x_j <- x_j exp(s_j phi_j) + b_j phi_{D+j}  where m_j = 0,  x_j  where m_j = 1.   exp() takes its argument as written: no clamp.
// Encoder, a tile of NF_WT = 8 windows per workgroup, h = c = 0, for i = L-1 .. 0:
//   h <- flow_enc(h, t_i - prev_t)   with prev_t = t_{L-1} + 0.01 at first, then the point before (every window reads its own times);
//   gates = W_ih [x_i, mask_i] + b_ih + W_hh h + b_hh;  c' = sigmoid(f) c + sigmoid(i) tanh(g),  h' = sigmoid(o) tanh(c');
//   (h, c) <- (h', c') where any feature of point i is observed.
// then (mu, sr) = transform_z0(h), sigma = softplus(sr), z0 = mu + eps sigma.  Decode, independent per (window, forecast time):
//   out[b, j] = Wd flow_dec(z0[b], tpp[b, j]) + bd.
//
// W_ih is the one large matrix (4R x 2C) and its product does not depend on the recurrence: the encoder kernel forms
// xg = W_ih [x, mask] + b_ih + b_hh for all L points of its tile before the walk (W_ih read through the cache, xg written to device
// memory, which the backward reads again), so the LDS holds W_hh and the flow's nets only, in torch's (N, K) layout with rows K | 1
// floats apart; transform_z0 takes the region over after the walk.  Products are on the VALU, one output per thread per layer at
// Hd = 32, as in csrc/latent_ode.hip: the launch is bound by its chain of barriers.
//
// Forward saves xg, the (h, c) entering every observed point, the final h, and (mu, sigma, z0).  Backward: launch 1, the decode rows
// (the flow rebuilt from z0 with every layer's activations kept in LDS, pulled back; the cotangent of z0 per row goes to the
// workspace); launch 2, the encoder: transform_z0, then the observed points i = 0 .. L-1, each rebuilt from its saved (h, c) and xg;
// launch 3 adds the per-workgroup parameter-gradient slabs in index order.  Every slab entry has one owner thread: no atomics, the
// same inputs give the same bits.  Data, mask, times and eps take no gradient.  phi is not saved: the backward forms it again with
// nf_phi<TN> from the scale and the t it has in LDS, the forward's expression, so d scale += d phi (1 - phi^2) t (TimeTanh) uses the
// forward's phi bit for bit and the LDS plan is the same for both time nets.  The fold kernel never sees phi and is shared.
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

constexpr int NF_WT = 8;                   // rows (windows, or decode rows) of a tile
constexpr int NF_H = 100;                  // hidden width of transform_z0
constexpr int NF_THREADS = 256;
constexpr int NF_MAX_FL = 4, NF_MAX_HL = 4, NF_MAX_RZ = 64, NF_MAX_HD = 128, NF_MAX_C = 64, NF_MAX_T = 1 << 20;
constexpr int NF_DEC_WG = 256;             // most workgroups of the decode kernels (a workgroup walks tiles grid-stride)
constexpr size_t NF_LDS_MAX = 160 * 1024;
constexpr int NF_LINEAR = IMMTSF_NF_TIME_LINEAR, NF_TANH = IMMTSF_NF_TIME_TANH;      // the time net of a kernel instance (TN)

// a Linear: weight (N, K) at goff of its section of the flat parameters, bias (hb) behind it; in LDS at loff, rows ld apart
struct NfLin { int N, K, ld, goff, loff, hb; };
struct NfFlow {
    int D;
    int sg[NF_MAX_FL], sl[NF_MAX_FL];      // time_net.scale (2D) of layer i: in the section, in LDS
    NfLin l[NF_MAX_FL][NF_MAX_HL + 1];
};
struct NfPlan {
    int B, L, Lp, C, R, Z, Hd, HL, NF;
    int ldd, ldz, ldh, ld2, ldg, ldx, ldo;  // row pitches: D | D + 1 | hidden | 2D | 4R | 2C | C
    int NVe, NVd;                          // parameters of the encoder section (first in the flat buffer) and of the decode section
    int wih, bih, bhh;                     // lstm.weight_ih, bias_ih, bias_hh in the encoder section
    int wenc, wdec;                        // LDS weight floats of the encoder kernels / the decode kernels
    NfLin whh, t1, t2, dcd;
    NfFlow enc, dec;
};

__host__ __device__ inline int nf_max(int a, int b) { return a > b ? a : b; }

inline void nf_set(NfLin& l, int N, int K, bool hb, int& g, int& lo) {
    l.N = N; l.K = K; l.ld = K | 1; l.goff = g; l.loff = lo; l.hb = hb ? 1 : 0;
    g += N * K + (hb ? N : 0);
    lo += N * l.ld + (hb ? N : 0);
}
inline void nf_set_flow(NfFlow& f, int D, int Hd, int HL, int NF, int& g, int& lo) {
    f.D = D;
    for (int i = 0; i < NF; ++i) {
        for (int k = 0; k <= HL; ++k) nf_set(f.l[i][k], k == HL ? 2 * D : Hd, k == 0 ? D + 1 : Hd, true, g, lo);
        f.sg[i] = g; f.sl[i] = lo;
        g += 2 * D; lo += 2 * D;
    }
}

inline NfPlan nf_plan(int B, int L, int Lp, int C, int R, int Z, int Hd, int HL, int NF) {
    NfPlan p{};
    p.B = B; p.L = L; p.Lp = Lp; p.C = C; p.R = R; p.Z = Z; p.Hd = Hd; p.HL = HL; p.NF = NF;
    int g = 0, lo = 0;
    p.wih = g; g += 4 * R * 2 * C;
    nf_set(p.whh, 4 * R, R, false, g, lo);
    p.bih = g; g += 4 * R;
    p.bhh = g; g += 4 * R;
    nf_set_flow(p.enc, R, Hd, HL, NF, g, lo);
    const int walk = lo;
    lo = 0;
    nf_set(p.t1, NF_H, R, true, g, lo);
    nf_set(p.t2, 2 * Z, NF_H, true, g, lo);
    p.NVe = g;
    p.wenc = (nf_max(walk, lo) + 3) & ~3;
    g = 0; lo = 0;
    nf_set_flow(p.dec, Z, Hd, HL, NF, g, lo);
    nf_set(p.dcd, C, Z, true, g, lo);
    p.NVd = g;
    p.wdec = (lo + 3) & ~3;
    const int rz = nf_max(R, Z);
    p.ldd = rz | 1; p.ldz = (rz + 1) | 1; p.ldh = nf_max(Hd, NF_H) | 1; p.ld2 = (2 * rz) | 1; p.ldg = (4 * R) | 1; p.ldx = (2 * C) | 1;
    p.ldo = C | 1;
    return p;
}

struct NfBuf {
    float *W, *x, *c, *tt, *mk, *gates, *xi, *thid, *zz, *co, *slot;      // both directions (c, gates, xi, thid, zz: encoder only)
    int slotsz;                                                            // floats of one flow-layer slot
    float *g, *gc, *gsb, *gsc, *gha, *ghb, *gz, *dgt;                      // backward (gc, dgt: encoder only)
};

// the activation buffers behind the weight region; returns the floats used.  The backward keeps a slot per flow layer.
__host__ __device__ inline size_t nf_carve(const NfPlan& p, float* lds, bool enc, bool bwd, NfBuf* s) {
    NfBuf t{};
    const int T = NF_WT;
    float* v = lds + (enc ? p.wenc : p.wdec);
    t.W = lds;
    t.x = v; v += T * p.ldd;
    t.tt = v; v += T; t.mk = v; v += T;
    t.co = v; v += T * p.ldo;
    if (enc) {
        t.c = v; v += T * p.ldd;
        t.gates = v; v += T * p.ldg;
        t.xi = v; v += T * p.ldx;
        t.thid = v; v += T * p.ldh;
        t.zz = v; v += T * p.ld2;
    }
    t.slotsz = T * (p.ldd + p.ldz + p.HL * p.ldh + p.ld2);
    t.slot = v; v += (size_t)(bwd ? p.NF : 1) * t.slotsz;
    if (bwd) {
        t.g = v; v += T * p.ldd;
        t.gsb = v; v += T * p.ld2; t.gsc = v; v += T * p.ld2;
        t.gha = v; v += T * p.ldh; t.ghb = v; v += T * p.ldh;
        t.gz = v; v += T * p.ldz;
        if (enc) {
            t.gc = v; v += T * p.ldd;
            t.dgt = v; v += T * p.ldg;
        }
    }
    if (s) *s = t;
    return (size_t)(v - lds);
}
inline size_t nf_lds_bytes(const NfPlan& p, bool enc, bool bwd) { return sizeof(float) * nf_carve(p, nullptr, enc, bwd, nullptr); }

// one Linear from its section of the flat parameters into LDS.  No barrier.
__device__ void nf_load_lin(float* W, const NfLin& l, const float* __restrict__ prm) {
    for (int e = threadIdx.x; e < l.N * l.K; e += NF_THREADS) {
        const int n = e / l.K, k = e - n * l.K;
        W[l.loff + n * l.ld + k] = prm[l.goff + e];
    }
    if (l.hb)
        for (int n = threadIdx.x; n < l.N; n += NF_THREADS) W[l.loff + l.N * l.ld + n] = prm[l.goff + l.N * l.K + n];
}
// a flow's nets and scales.  No barrier.
__device__ void nf_load_flow(const NfPlan& p, float* W, const NfFlow& f, const float* __restrict__ prm) {
    for (int i = 0; i < p.NF; ++i) {
        for (int k = 0; k <= p.HL; ++k) nf_load_lin(W, f.l[i][k], prm);
        for (int j = threadIdx.x; j < 2 * f.D; j += NF_THREADS) W[f.sl[i] + j] = prm[f.sg[i] + j];
    }
}

// out[w, n] = act(b[n] + sum_k in[w, k] W[n, k]);  ACT: 0 none, 1 tanh.  Ends with a barrier.
template <int ACT>
__device__ void nf_lin(const float* Wl, const NfLin& l, const float* in, int ldi, float* out, int ldo) {
    const float *W = Wl + l.loff, *b = W + l.N * l.ld;
    for (int idx = threadIdx.x; idx < NF_WT * l.N; idx += NF_THREADS) {
        const int w = idx / l.N, n = idx - w * l.N;
        const float *x = in + w * ldi, *wr = W + n * l.ld;
        float a0 = l.hb ? b[n] : 0.f, a1 = 0.f;
        int k = 0;
        for (; k + 1 < l.K; k += 2) { a0 += x[k] * wr[k]; a1 += x[k + 1] * wr[k + 1]; }
        if (k < l.K) a0 += x[k] * wr[k];
        const float a = a0 + a1;
        out[w * ldo + n] = ACT == 1 ? tanhf(a) : a;
    }
    __syncthreads();
}

// gin[w, k] = (sum_n g[w, n] W[n, k]) (1 - act[w, k]^2 where act is given), k < Klim.  Ends with a barrier.
__device__ void nf_lin_t(const float* Wl, const NfLin& l, const float* g, int ldg, float* gin, int ldi, int Klim, const float* act, int lda) {
    const float* W = Wl + l.loff;
    for (int idx = threadIdx.x; idx < NF_WT * Klim; idx += NF_THREADS) {
        const int w = idx / Klim, k = idx - w * Klim;
        const float* gr = g + w * ldg;
        float a = 0.f;
        for (int n = 0; n < l.N; ++n) a += gr[n] * W[n * l.ld + k];
        if (act) { const float t = act[w * lda + k]; a *= 1.f - t * t; }
        gin[w * ldi + k] = a;
    }
    __syncthreads();
}

// slab[W] += g^T in, slab[b] += column sums of g, over the tile's rows.  One owner thread per entry.  No barrier: it only reads LDS.
__device__ void nf_wgrad(float* __restrict__ slab, const NfLin& l, const float* g, int ldg, const float* in, int ldi) {
    for (int e = threadIdx.x; e < l.N * l.K; e += NF_THREADS) {
        const int n = e / l.K, k = e - n * l.K;
        float a = 0.f;
        for (int w = 0; w < NF_WT; ++w) a += g[w * ldg + n] * in[w * ldi + k];
        slab[l.goff + e] += a;
    }
    if (l.hb)
        for (int n = threadIdx.x; n < l.N; n += NF_THREADS) {
            float a = 0.f;
            for (int w = 0; w < NF_WT; ++w) a += g[w * ldg + n];
            slab[l.goff + l.N * l.K + n] += a;
        }
}

// m_j == 1: coordinate j of layer `layer` passes through and feeds the net
__device__ inline bool nf_masked(int D, int layer, int j) {
    if (D == 1) return false;
    const bool low = j < D / 2;
    return (layer & 1) ? !low : low;
}

// phi = time_net(t) of one coordinate: scale t (TimeLinear), tanhf(scale t) (TimeTanh).  The one definition the forward and the backward of
// an instance share: the backward rebuilds phi from the same scale and t in LDS, so it sees the forward's bits.
template <int TN>
__device__ inline float nf_phi(float sc, float t) {
    const float a = sc * t;
    return TN == NF_TANH ? tanhf(a) : a;
}

struct NfSlot { float *xin, *zin, *hid, *sb; };
__device__ inline NfSlot nf_slot(const NfPlan& p, const NfBuf& s, int i) {
    NfSlot t;
    t.xin = s.slot + (size_t)i * s.slotsz;
    t.zin = t.xin + NF_WT * p.ldd;
    t.hid = t.zin + NF_WT * p.ldz;
    t.sb = t.hid + p.HL * NF_WT * p.ldh;
    return t;
}

// x (pitch ldd) <- flow(x, tt), in place.  keep: layer i leaves its input, net input, hidden activations and (s, b) in slot i.
// Expects a barrier behind the writes of x and tt; ends with a barrier.
template <int TN>
__device__ void nf_flow_fwd(const NfPlan& p, const NfFlow& f, const NfBuf& s, float* x, bool keep) {
    const int T = NF_WT, D = f.D;
    for (int i = 0; i < p.NF; ++i) {
        const NfSlot q = nf_slot(p, s, keep ? i : 0);
        for (int idx = threadIdx.x; idx < T * (D + 1); idx += NF_THREADS) {
            const int w = idx / (D + 1), j = idx - w * (D + 1);
            if (j < D) {
                const float v = x[w * p.ldd + j];
                q.xin[w * p.ldd + j] = v;
                q.zin[w * p.ldz + j] = nf_masked(D, i, j) ? v : 0.f;
            } else {
                q.zin[w * p.ldz + D] = s.tt[w];
            }
        }
        __syncthreads();
        const float* in = q.zin;
        int ldi = p.ldz;
        for (int k = 0; k < p.HL; ++k) {
            float* h = q.hid + k * T * p.ldh;
            nf_lin<1>(s.W, f.l[i][k], in, ldi, h, p.ldh);
            in = h; ldi = p.ldh;
        }
        nf_lin<0>(s.W, f.l[i][p.HL], in, ldi, q.sb, p.ld2);
        const float* sc = s.W + f.sl[i];
        for (int idx = threadIdx.x; idx < T * D; idx += NF_THREADS) {
            const int w = idx / D, j = idx - w * D;
            if (nf_masked(D, i, j)) continue;
            const float t = s.tt[w], sv = q.sb[w * p.ld2 + j], bv = q.sb[w * p.ld2 + D + j];
            x[w * p.ldd + j] = x[w * p.ldd + j] * expf(sv * nf_phi<TN>(sc[j], t)) + bv * nf_phi<TN>(sc[D + j], t);
        }
        __syncthreads();
    }
}

// the flow that nf_flow_fwd(keep) just rebuilt, backwards: s.g holds the cotangent of its result on entry and of its input on exit
template <int TN>
__device__ void nf_flow_bwd(const NfPlan& p, const NfFlow& f, const NfBuf& s, float* slab) {
    const int T = NF_WT, D = f.D;
    for (int i = p.NF - 1; i >= 0; --i) {
        const NfSlot q = nf_slot(p, s, i);
        const float* sc = s.W + f.sl[i];
        for (int idx = threadIdx.x; idx < T * D; idx += NF_THREADS) {
            const int w = idx / D, j = idx - w * D, o = w * p.ld2;
            if (nf_masked(D, i, j)) {
                s.gsb[o + j] = 0.f; s.gsb[o + D + j] = 0.f; s.gsc[o + j] = 0.f; s.gsc[o + D + j] = 0.f;
                continue;
            }
            const float t = s.tt[w], sv = q.sb[o + j], bv = q.sb[o + D + j], ps = nf_phi<TN>(sc[j], t), pb = nf_phi<TN>(sc[D + j], t);
            const float e = expf(sv * ps), xv = q.xin[w * p.ldd + j], gy = s.g[w * p.ldd + j];
            s.g[w * p.ldd + j] = gy * e;
            s.gsb[o + j] = gy * xv * e * ps;
            s.gsb[o + D + j] = gy * pb;
            if (TN == NF_TANH) {                                            // d phi / d scale = (1 - phi^2) t
                s.gsc[o + j] = gy * xv * e * sv * ((1.f - ps * ps) * t);
                s.gsc[o + D + j] = gy * bv * ((1.f - pb * pb) * t);
            } else {
                s.gsc[o + j] = gy * xv * e * sv * t;
                s.gsc[o + D + j] = gy * bv * t;
            }
        }
        __syncthreads();
        for (int j = threadIdx.x; j < 2 * D; j += NF_THREADS) {
            float a = 0.f;
            for (int w = 0; w < T; ++w) a += s.gsc[w * p.ld2 + j];
            slab[f.sg[i] + j] += a;
        }
        const float* gout = s.gsb;
        int ldgo = p.ld2;
        for (int k = p.HL; k >= 1; --k) {
            const float* in = q.hid + (k - 1) * T * p.ldh;
            float* gi = (k & 1) ? s.gha : s.ghb;
            nf_wgrad(slab, f.l[i][k], gout, ldgo, in, p.ldh);
            nf_lin_t(s.W, f.l[i][k], gout, ldgo, gi, p.ldh, f.l[i][k].K, in, p.ldh);
            gout = gi; ldgo = p.ldh;
        }
        nf_wgrad(slab, f.l[i][0], gout, ldgo, q.zin, p.ldz);
        nf_lin_t(s.W, f.l[i][0], gout, ldgo, s.gz, p.ldz, D, nullptr, 0);
        for (int idx = threadIdx.x; idx < T * D; idx += NF_THREADS) {
            const int w = idx / D, j = idx - w * D;
            if (nf_masked(D, i, j)) s.g[w * p.ldd + j] += s.gz[w * p.ldz + j];
        }
        __syncthreads();
    }
}

__device__ inline float nf_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// the times and the "any feature observed" flags of point i, per window of the tile.  No barrier.
__device__ void nf_point(const NfPlan& p, const NfBuf& s, const float* __restrict__ mask, const float* __restrict__ tp, int b0, int i) {
    for (int w = threadIdx.x; w < NF_WT; w += NF_THREADS) {
        const int b = b0 + w;
        float t = 0.f, m = 0.f;
        if (b < p.B) {
            const float* tr = tp + (size_t)b * p.L;
            t = i == p.L - 1 ? tr[i] - (tr[i] + 0.01f) : tr[i] - tr[i + 1];
            const float* mr = mask + ((size_t)b * p.L + i) * p.C;
            for (int c = 0; c < p.C; ++c) m += mr[c];
        }
        s.tt[w] = t;
        s.mk[w] = m > 0.f ? 1.f : 0.f;
    }
}

// gates[w, n] = xg[b, i, n] + sum_k W_hh[n, k] h[w, k].  Ends with a barrier.
__device__ void nf_gates(const NfPlan& p, const NfBuf& s, const float* xg, int b0, int i) {
    const int G = 4 * p.R;
    const float* W = s.W + p.whh.loff;
    for (int idx = threadIdx.x; idx < NF_WT * G; idx += NF_THREADS) {
        const int w = idx / G, n = idx - w * G, b = b0 + w;
        float a0 = b < p.B ? xg[((size_t)b * p.L + i) * G + n] : 0.f, a1 = 0.f;
        const float *h = s.x + w * p.ldd, *wr = W + n * p.whh.ld;
        int k = 0;
        for (; k + 1 < p.R; k += 2) { a0 += h[k] * wr[k]; a1 += h[k + 1] * wr[k + 1]; }
        if (k < p.R) a0 += h[k] * wr[k];
        s.gates[w * p.ldg + n] = a0 + a1;
    }
    __syncthreads();
}

template <int TN>
__global__ __launch_bounds__(NF_THREADS) void nf_enc_fwd_kernel(NfPlan p, const float* __restrict__ data, const float* __restrict__ mask,
                                                               const float* __restrict__ tp, const float* __restrict__ prm,
                                                               const float* __restrict__ eps, float* xg, float* __restrict__ states,
                                                               float* __restrict__ zs) {
    extern __shared__ __align__(16) float nf_lds[];
    NfBuf s;
    nf_carve(p, nf_lds, true, false, &s);
    const int T = NF_WT, b0 = blockIdx.x * T, R = p.R, Z = p.Z, C = p.C, L = p.L, G = 4 * R;
    for (int idx = threadIdx.x; idx < T * p.ldd; idx += NF_THREADS) { s.x[idx] = 0.f; s.c[idx] = 0.f; }
    nf_load_lin(s.W, p.whh, prm);
    nf_load_flow(p, s.W, p.enc, prm);
    // ---- xg = W_ih [x, mask] + b_ih + b_hh for every point of the tile
    const long long total = (long long)T * L * G;
    for (long long idx = threadIdx.x; idx < total; idx += NF_THREADS) {
        const int w = (int)(idx / ((long long)L * G));
        const long long r = idx - (long long)w * L * G;
        const int i = (int)(r / G), n = (int)(r - (long long)i * G), b = b0 + w;
        if (b >= p.B) continue;
        const float *wr = prm + p.wih + (size_t)n * 2 * C, *dr = data + ((size_t)b * L + i) * C, *mr = mask + ((size_t)b * L + i) * C;
        float a = prm[p.bih + n] + prm[p.bhh + n];
        for (int k = 0; k < C; ++k) a += wr[k] * dr[k];
        for (int k = 0; k < C; ++k) a += wr[C + k] * mr[k];
        xg[((size_t)b * L + i) * G + n] = a;
    }
    __syncthreads();
    // ---- the walk, last point first
    for (int q = 0; q <= L; ++q) {
        for (int idx = threadIdx.x; idx < T * 2 * R; idx += NF_THREADS) {      // the state entering point L-1-q; q = L: the last one
            const int w = idx / (2 * R), j = idx - w * 2 * R;
            if (b0 + w < p.B) states[((size_t)(b0 + w) * (L + 1) + q) * 2 * R + j] = j < R ? s.x[w * p.ldd + j] : s.c[w * p.ldd + j - R];
        }
        if (q == L) break;
        const int i = L - 1 - q;
        nf_point(p, s, mask, tp, b0, i);
        __syncthreads();
        nf_flow_fwd<TN>(p, p.enc, s, s.x, false);
        nf_gates(p, s, xg, b0, i);
        for (int idx = threadIdx.x; idx < T * R; idx += NF_THREADS) {
            const int w = idx / R, j = idx - w * R;
            if (s.mk[w] == 0.f) continue;
            const float* gt = s.gates + w * p.ldg;
            const float ig = nf_sigmoid(gt[j]), fg = nf_sigmoid(gt[R + j]), gg = tanhf(gt[2 * R + j]), og = nf_sigmoid(gt[3 * R + j]);
            const float cn = fg * s.c[w * p.ldd + j] + ig * gg;
            s.c[w * p.ldd + j] = cn;
            s.x[w * p.ldd + j] = og * tanhf(cn);
        }
        __syncthreads();
    }
    // ---- transform_z0 and the draw
    __syncthreads();
    nf_load_lin(s.W, p.t1, prm);
    nf_load_lin(s.W, p.t2, prm);
    __syncthreads();
    nf_lin<1>(s.W, p.t1, s.x, p.ldd, s.thid, p.ldh);
    nf_lin<0>(s.W, p.t2, s.thid, p.ldh, s.zz, p.ld2);
    for (int idx = threadIdx.x; idx < T * Z; idx += NF_THREADS) {
        const int w = idx / Z, j = idx - w * Z, b = b0 + w;
        if (b >= p.B) continue;
        const float mu = s.zz[w * p.ld2 + j], sr = s.zz[w * p.ld2 + Z + j];
        const float sg = sr > 20.f ? sr : log1pf(expf(sr));
        zs[((size_t)b * 3 + 0) * Z + j] = mu;
        zs[((size_t)b * 3 + 1) * Z + j] = sg;
        zs[((size_t)b * 3 + 2) * Z + j] = mu + eps[(size_t)b * Z + j] * sg;
    }
}

// z0 and the forecast time of the rows of tile `tile` of the (B Lp) decode rows.  Ends with a barrier.
__device__ void nf_dec_rows(const NfPlan& p, const NfBuf& s, const float* __restrict__ zs, const float* __restrict__ tpp, int tile) {
    const int T = NF_WT, Z = p.Z, rows = p.B * p.Lp, r0 = tile * T;
    for (int idx = threadIdx.x; idx < T * Z; idx += NF_THREADS) {
        const int w = idx / Z, j = idx - w * Z, r = r0 + w;
        s.x[w * p.ldd + j] = r < rows ? zs[((size_t)(r / p.Lp) * 3 + 2) * Z + j] : 0.f;
    }
    for (int w = threadIdx.x; w < T; w += NF_THREADS) s.tt[w] = r0 + w < rows ? tpp[r0 + w] : 0.f;
    __syncthreads();
}

template <int TN>
__global__ __launch_bounds__(NF_THREADS) void nf_dec_fwd_kernel(NfPlan p, const float* __restrict__ zs, const float* __restrict__ tpp,
                                                               const float* __restrict__ prm, float* __restrict__ out) {
    extern __shared__ __align__(16) float nf_lds[];
    NfBuf s;
    nf_carve(p, nf_lds, false, false, &s);
    const int T = NF_WT, C = p.C, rows = p.B * p.Lp, ntiles = (rows + T - 1) / T;
    nf_load_flow(p, s.W, p.dec, prm);
    nf_load_lin(s.W, p.dcd, prm);
    __syncthreads();
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        nf_dec_rows(p, s, zs, tpp, tile);
        nf_flow_fwd<TN>(p, p.dec, s, s.x, false);
        nf_lin<0>(s.W, p.dcd, s.x, p.ldd, s.co, p.ldo);
        for (int idx = threadIdx.x; idx < T * C; idx += NF_THREADS) {
            const int w = idx / C, c = idx - w * C, r = tile * T + w;
            if (r < rows) out[(size_t)r * C + c] = s.co[w * p.ldo + c];
        }
        __syncthreads();
    }
}

template <int TN>
__global__ __launch_bounds__(NF_THREADS) void nf_dec_bwd_kernel(NfPlan p, const float* __restrict__ zs, const float* __restrict__ tpp,
                                                               const float* __restrict__ prm, const float* __restrict__ dout,
                                                               float* __restrict__ slabs, float* __restrict__ gzr) {
    extern __shared__ __align__(16) float nf_lds[];
    NfBuf s;
    nf_carve(p, nf_lds, false, true, &s);
    const int T = NF_WT, C = p.C, Z = p.Z, rows = p.B * p.Lp, ntiles = (rows + T - 1) / T;
    float* slab = slabs + (size_t)blockIdx.x * p.NVd;
    for (int e = threadIdx.x; e < p.NVd; e += NF_THREADS) slab[e] = 0.f;
    nf_load_flow(p, s.W, p.dec, prm);
    nf_load_lin(s.W, p.dcd, prm);
    __syncthreads();
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int idx = threadIdx.x; idx < T * C; idx += NF_THREADS) {
            const int w = idx / C, c = idx - w * C, r = tile * T + w;
            s.co[w * p.ldo + c] = r < rows ? dout[(size_t)r * C + c] : 0.f;
        }
        nf_dec_rows(p, s, zs, tpp, tile);
        nf_flow_fwd<TN>(p, p.dec, s, s.x, true);
        nf_wgrad(slab, p.dcd, s.co, p.ldo, s.x, p.ldd);
        nf_lin_t(s.W, p.dcd, s.co, p.ldo, s.g, p.ldd, Z, nullptr, 0);
        nf_flow_bwd<TN>(p, p.dec, s, slab);
        for (int idx = threadIdx.x; idx < T * Z; idx += NF_THREADS) {
            const int w = idx / Z, j = idx - w * Z, r = tile * T + w;
            if (r < rows) gzr[(size_t)r * Z + j] = s.g[w * p.ldd + j];
        }
        __syncthreads();
    }
}

template <int TN>
__global__ __launch_bounds__(NF_THREADS) void nf_enc_bwd_kernel(NfPlan p, const float* __restrict__ data, const float* __restrict__ mask,
                                                               const float* __restrict__ tp, const float* __restrict__ prm,
                                                               const float* __restrict__ eps, const float* __restrict__ xg,
                                                               const float* __restrict__ states, const float* __restrict__ gzr,
                                                               float* __restrict__ slabs) {
    extern __shared__ __align__(16) float nf_lds[];
    NfBuf s;
    nf_carve(p, nf_lds, true, true, &s);
    const int T = NF_WT, b0 = blockIdx.x * T, R = p.R, Z = p.Z, C = p.C, L = p.L, Lp = p.Lp, G = 4 * R;
    float* slab = slabs + (size_t)blockIdx.x * p.NVe;
    for (int e = threadIdx.x; e < p.NVe; e += NF_THREADS) slab[e] = 0.f;
    nf_load_lin(s.W, p.t1, prm);
    nf_load_lin(s.W, p.t2, prm);
    for (int idx = threadIdx.x; idx < T * R; idx += NF_THREADS) {
        const int w = idx / R, j = idx - w * R;
        s.x[w * p.ldd + j] = b0 + w < p.B ? states[((size_t)(b0 + w) * (L + 1) + L) * 2 * R + j] : 0.f;
    }
    __syncthreads();
    // ---- z0 = mu + eps softplus(sr), transform_z0; the cotangent of z0 is the sum over the window's decode rows, in order
    nf_lin<1>(s.W, p.t1, s.x, p.ldd, s.thid, p.ldh);
    nf_lin<0>(s.W, p.t2, s.thid, p.ldh, s.zz, p.ld2);
    for (int idx = threadIdx.x; idx < T * Z; idx += NF_THREADS) {
        const int w = idx / Z, j = idx - w * Z, b = b0 + w;
        float g = 0.f, e = 0.f;
        if (b < p.B) {
            for (int jt = 0; jt < Lp; ++jt) g += gzr[((size_t)b * Lp + jt) * Z + j];
            e = eps[(size_t)b * Z + j];
        }
        const float sr = s.zz[w * p.ld2 + Z + j];
        s.gsb[w * p.ld2 + j] = g;
        s.gsb[w * p.ld2 + Z + j] = g * e * (sr > 20.f ? 1.f : nf_sigmoid(sr));
    }
    __syncthreads();
    nf_wgrad(slab, p.t2, s.gsb, p.ld2, s.thid, p.ldh);
    nf_lin_t(s.W, p.t2, s.gsb, p.ld2, s.gha, p.ldh, NF_H, s.thid, p.ldh);
    nf_wgrad(slab, p.t1, s.gha, p.ldh, s.x, p.ldd);
    nf_lin_t(s.W, p.t1, s.gha, p.ldh, s.g, p.ldd, R, nullptr, 0);
    for (int idx = threadIdx.x; idx < T * p.ldd; idx += NF_THREADS) s.gc[idx] = 0.f;
    __syncthreads();
    nf_load_lin(s.W, p.whh, prm);
    nf_load_flow(p, s.W, p.enc, prm);
    __syncthreads();
    // ---- the observed points, first to last (the forward walked them last to first): s.g / s.gc = the cotangents of (h, c) behind point i
    for (int q = L - 1; q >= 0; --q) {
        const int i = L - 1 - q;
        for (int idx = threadIdx.x; idx < T * 2 * R; idx += NF_THREADS) {
            const int w = idx / (2 * R), j = idx - w * 2 * R;
            const float v = b0 + w < p.B ? states[((size_t)(b0 + w) * (L + 1) + q) * 2 * R + j] : 0.f;
            if (j < R) s.x[w * p.ldd + j] = v; else s.c[w * p.ldd + j - R] = v;
        }
        for (int idx = threadIdx.x; idx < T * 2 * C; idx += NF_THREADS) {
            const int w = idx / (2 * C), k = idx - w * 2 * C, b = b0 + w;
            float v = 0.f;
            if (b < p.B) v = k < C ? data[((size_t)b * L + i) * C + k] : mask[((size_t)b * L + i) * C + k - C];
            s.xi[w * p.ldx + k] = v;
        }
        nf_point(p, s, mask, tp, b0, i);
        __syncthreads();
        nf_flow_fwd<TN>(p, p.enc, s, s.x, true);
        nf_gates(p, s, xg, b0, i);
        for (int idx = threadIdx.x; idx < T * R; idx += NF_THREADS) {
            const int w = idx / R, j = idx - w * R, o = w * p.ldd + j;
            float* dg = s.dgt + w * p.ldg;
            if (s.mk[w] == 0.f) {                                          // the state passes through: only the flow is pulled back
                dg[j] = 0.f; dg[R + j] = 0.f; dg[2 * R + j] = 0.f; dg[3 * R + j] = 0.f;
                continue;
            }
            const float* gt = s.gates + w * p.ldg;
            const float ig = nf_sigmoid(gt[j]), fg = nf_sigmoid(gt[R + j]), gg = tanhf(gt[2 * R + j]), og = nf_sigmoid(gt[3 * R + j]);
            const float cin = s.c[o], tc = tanhf(fg * cin + ig * gg), gh = s.g[o];
            const float gcn = s.gc[o] + gh * og * (1.f - tc * tc);
            dg[j] = gcn * gg * ig * (1.f - ig);
            dg[R + j] = gcn * cin * fg * (1.f - fg);
            dg[2 * R + j] = gcn * ig * (1.f - gg * gg);
            dg[3 * R + j] = gh * tc * og * (1.f - og);
            s.gc[o] = gcn * fg;
            s.g[o] = 0.f;
        }
        __syncthreads();
        // lstm.weight_ih, weight_hh and both biases
        for (int e = threadIdx.x; e < G * 2 * C; e += NF_THREADS) {
            const int n = e / (2 * C), k = e - n * 2 * C;
            float a = 0.f;
            for (int w = 0; w < T; ++w) a += s.dgt[w * p.ldg + n] * s.xi[w * p.ldx + k];
            slab[p.wih + e] += a;
        }
        for (int n = threadIdx.x; n < G; n += NF_THREADS) {
            float a = 0.f;
            for (int w = 0; w < T; ++w) a += s.dgt[w * p.ldg + n];
            slab[p.bih + n] += a;
            slab[p.bhh + n] += a;
        }
        nf_wgrad(slab, p.whh, s.dgt, p.ldg, s.x, p.ldd);
        for (int idx = threadIdx.x; idx < T * R; idx += NF_THREADS) {      // the cotangent of the h behind the flow
            const int w = idx / R, k = idx - w * R;
            const float *dg = s.dgt + w * p.ldg, *W = s.W + p.whh.loff;
            float a = 0.f;
            for (int n = 0; n < G; ++n) a += dg[n] * W[n * p.whh.ld + k];
            s.g[w * p.ldd + k] += a;
        }
        __syncthreads();
        nf_flow_bwd<TN>(p, p.enc, s, slab);
    }
}

__global__ __launch_bounds__(NF_THREADS) void nf_fold_kernel(int NVe, int NVd, int nwe, int nwd, const float* __restrict__ se,
                                                            const float* __restrict__ sd, float* __restrict__ grads) {
    const int i = blockIdx.x * NF_THREADS + threadIdx.x;
    if (i >= NVe + NVd) return;
    float a = 0.f;
    if (i < NVe) {
        for (int b = 0; b < nwe; ++b) a += se[(size_t)b * NVe + i];
    } else {
        for (int b = 0; b < nwd; ++b) a += sd[(size_t)b * NVd + i - NVe];
    }
    grads[i] = a;
}

bool nf_dims_ok(const immtsf_neural_flow_dims* d) {
    return d && d->L >= 1 && d->L <= NF_MAX_T && d->Lp >= 1 && d->Lp <= NF_MAX_T && d->C >= 1 && d->C <= NF_MAX_C && d->rec_dims >= 1 &&
           d->rec_dims <= NF_MAX_RZ && d->latents >= 1 && d->latents <= NF_MAX_RZ && d->hidden_dim >= 1 && d->hidden_dim <= NF_MAX_HD &&
           d->hidden_layers >= 1 && d->hidden_layers <= NF_MAX_HL && d->flow_layers >= 1 && d->flow_layers <= NF_MAX_FL;
}
NfPlan nf_plan_of(const immtsf_neural_flow_dims* d) {
    return nf_plan(d->B, d->L, d->Lp, d->C, d->rec_dims, d->latents, d->hidden_dim, d->hidden_layers, d->flow_layers);
}
int nf_enc_wgs(const NfPlan& p) { return cdiv(p.B, NF_WT); }
int nf_dec_wgs(const NfPlan& p) {
    const int tiles = cdiv(p.B * p.Lp, NF_WT);
    return tiles < NF_DEC_WG ? tiles : NF_DEC_WG;
}
bool nf_kind_ok(int32_t tn) { return tn == NF_LINEAR || tn == NF_TANH; }
bool nf_call_ok(const immtsf_neural_flow_dims* d) {
    if (!immtsf_neural_flow_supported(d) || d->B < 1) return false;
    const int64_t widest = nf_max(nf_max(4 * d->rec_dims, d->latents), d->C);
    return (int64_t)d->B * ((int64_t)nf_max(d->L + 1, d->Lp)) * widest < (1ll << 31);
}
size_t nf_up64(size_t n) { return (n + 63) & ~size_t(63); }
template <typename K>
void nf_allow_lds(K kernel, size_t lds) {
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// the two forward launches / the three backward launches of one instance (TN fixed at compile time: no branch on it in a kernel)
template <int TN>
int nf_forward(const NfPlan& p, const float* data, const float* mask, const float* tp, const float* tp_pred, const float* params,
               const float* eps, float* out, float* xg, float* states, float* zs, hipStream_t s) {
    const size_t le = nf_lds_bytes(p, true, false), ld = nf_lds_bytes(p, false, false);
    nf_allow_lds(nf_enc_fwd_kernel<TN>, le);
    hipLaunchKernelGGL(nf_enc_fwd_kernel<TN>, dim3(nf_enc_wgs(p)), dim3(NF_THREADS), le, s, p, data, mask, tp, params, eps, xg, states, zs);
    IMMTSF_LAUNCH_CHECK();
    nf_allow_lds(nf_dec_fwd_kernel<TN>, ld);
    hipLaunchKernelGGL(nf_dec_fwd_kernel<TN>, dim3(nf_dec_wgs(p)), dim3(NF_THREADS), ld, s, p, zs, tp_pred, params + p.NVe, out);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

template <int TN>
int nf_backward(const NfPlan& p, const float* data, const float* mask, const float* tp, const float* tp_pred, const float* params,
                const float* eps, const float* xg, const float* states, const float* zs, const float* d_out, float* grads, void* workspace,
                hipStream_t s) {
    const int nwe = nf_enc_wgs(p), nwd = nf_dec_wgs(p);
    float* se = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t(255));
    float* sd = se + nf_up64((size_t)nwe * p.NVe);
    float* gzr = sd + nf_up64((size_t)nwd * p.NVd);
    const size_t le = nf_lds_bytes(p, true, true), ld = nf_lds_bytes(p, false, true);
    nf_allow_lds(nf_dec_bwd_kernel<TN>, ld);
    hipLaunchKernelGGL(nf_dec_bwd_kernel<TN>, dim3(nwd), dim3(NF_THREADS), ld, s, p, zs, tp_pred, params + p.NVe, d_out, sd, gzr);
    IMMTSF_LAUNCH_CHECK();
    nf_allow_lds(nf_enc_bwd_kernel<TN>, le);
    hipLaunchKernelGGL(nf_enc_bwd_kernel<TN>, dim3(nwe), dim3(NF_THREADS), le, s, p, data, mask, tp, params, eps, xg, states, gzr, se);
    IMMTSF_LAUNCH_CHECK();
    hipLaunchKernelGGL(nf_fold_kernel, dim3(cdiv(p.NVe + p.NVd, NF_THREADS)), dim3(NF_THREADS), 0, s, p.NVe, p.NVd, nwe, nwd, se, sd, grads);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // namespace

extern "C" {

int immtsf_neural_flow_supported(const immtsf_neural_flow_dims* dims) {
    if (!nf_dims_ok(dims) || dims->B < 0) return 0;
    const NfPlan p = nf_plan_of(dims);
    return nf_lds_bytes(p, true, true) <= NF_LDS_MAX && nf_lds_bytes(p, false, true) <= NF_LDS_MAX;
}

int32_t immtsf_neural_flow_param_count(const immtsf_neural_flow_dims* dims) {
    if (!nf_dims_ok(dims)) return -1;
    const NfPlan p = nf_plan_of(dims);
    return p.NVe + p.NVd;
}

size_t immtsf_neural_flow_workspace_bytes(const immtsf_neural_flow_dims* dims) {
    if (!nf_call_ok(dims)) return 0;
    const NfPlan p = nf_plan_of(dims);
    return sizeof(float) * (nf_up64((size_t)nf_enc_wgs(p) * p.NVe) + nf_up64((size_t)nf_dec_wgs(p) * p.NVd) + (size_t)p.B * p.Lp * p.Z) + 256;
}

// the TimeTanh instance keeps no phi tile (the backward rebuilds phi from scale and t, both already in LDS), so the LDS plan, the
// parameter layout and the workspace are the TimeLinear instance's: the queries differ in the kind they accept only
int immtsf_neural_flow_tn_supported(const immtsf_neural_flow_dims* dims, int32_t time_net) {
    return nf_kind_ok(time_net) && immtsf_neural_flow_supported(dims);
}

int32_t immtsf_neural_flow_tn_param_count(const immtsf_neural_flow_dims* dims, int32_t time_net) {
    return nf_kind_ok(time_net) ? immtsf_neural_flow_param_count(dims) : -1;
}

size_t immtsf_neural_flow_tn_workspace_bytes(const immtsf_neural_flow_dims* dims, int32_t time_net) {
    return nf_kind_ok(time_net) ? immtsf_neural_flow_workspace_bytes(dims) : 0;
}

int immtsf_neural_flow_tn_forward(const immtsf_neural_flow_dims* dims, int32_t time_net, const float* data, const float* mask,
                                  const float* tp, const float* tp_pred, const float* params, const float* eps, float* out, float* xg,
                                  float* states, float* zs, immtsf_stream_t stream) {
    if (!dims || dims->B < 0) return IMMTSF_EINVAL;
    if (!immtsf_neural_flow_tn_supported(dims, time_net)) return IMMTSF_EUNSUPPORTED;
    if (dims->B == 0) return IMMTSF_OK;
    if (!nf_call_ok(dims)) return IMMTSF_EINVAL;
    if (!data || !mask || !tp || !tp_pred || !params || !eps || !out || !xg || !states || !zs) return IMMTSF_EINVAL;
    const NfPlan p = nf_plan_of(dims);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return time_net == NF_TANH ? nf_forward<NF_TANH>(p, data, mask, tp, tp_pred, params, eps, out, xg, states, zs, s)
                               : nf_forward<NF_LINEAR>(p, data, mask, tp, tp_pred, params, eps, out, xg, states, zs, s);
}

int immtsf_neural_flow_tn_backward(const immtsf_neural_flow_dims* dims, int32_t time_net, const float* data, const float* mask,
                                   const float* tp, const float* tp_pred, const float* params, const float* eps, const float* xg,
                                   const float* states, const float* zs, const float* d_out, float* grads, void* workspace,
                                   size_t workspace_bytes, immtsf_stream_t stream) {
    if (!dims || dims->B < 1) return IMMTSF_EINVAL;
    if (!immtsf_neural_flow_tn_supported(dims, time_net)) return IMMTSF_EUNSUPPORTED;
    if (!nf_call_ok(dims)) return IMMTSF_EINVAL;
    if (!data || !mask || !tp || !tp_pred || !params || !eps || !xg || !states || !zs || !d_out || !grads || !workspace) return IMMTSF_EINVAL;
    if (workspace_bytes < immtsf_neural_flow_workspace_bytes(dims)) return IMMTSF_EWORKSPACE;
    const NfPlan p = nf_plan_of(dims);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return time_net == NF_TANH
               ? nf_backward<NF_TANH>(p, data, mask, tp, tp_pred, params, eps, xg, states, zs, d_out, grads, workspace, s)
               : nf_backward<NF_LINEAR>(p, data, mask, tp, tp_pred, params, eps, xg, states, zs, d_out, grads, workspace, s);
}

// the entry points from before the time-net kind: TimeLinear
int immtsf_neural_flow_forward(const immtsf_neural_flow_dims* dims, const float* data, const float* mask, const float* tp,
                               const float* tp_pred, const float* params, const float* eps, float* out, float* xg, float* states,
                               float* zs, immtsf_stream_t stream) {
    return immtsf_neural_flow_tn_forward(dims, IMMTSF_NF_TIME_LINEAR, data, mask, tp, tp_pred, params, eps, out, xg, states, zs, stream);
}

int immtsf_neural_flow_backward(const immtsf_neural_flow_dims* dims, const float* data, const float* mask, const float* tp,
                                const float* tp_pred, const float* params, const float* eps, const float* xg, const float* states,
                                const float* zs, const float* d_out, float* grads, void* workspace, size_t workspace_bytes,
                                immtsf_stream_t stream) {
    return immtsf_neural_flow_tn_backward(dims, IMMTSF_NF_TIME_LINEAR, data, mask, tp, tp_pred, params, eps, xg, states, zs, d_out, grads,
                                          workspace, workspace_bytes, stream);
}

}  // extern "C"
