// The Kalman recurrence of the CRU backbone (reference lib/cru_components/CRULayer.py:42-109 over CRUCell.py:277-312 and :437-500) as
// ONE launch forward and TWO launches backward, all fp32.  n = lsd (latent state), lod = n / 2, K = num_basis, E = entries of a band.
//
// Per batch element b, with the prior (m-, cu-, cl-, cs-) starting at (0, icu, icl, 0), for i = 0 .. T-1:
//   update (RKNCell._update): den = cu- + yv_i; qu = cu- / den; ql = cs- / den; r = y_i - m-[:lod];
//     m+ = m- + (qu r, ql r); cu+ = (1 - qu) cu-; cl+ = cl- - ql cs-; cs+ = (1 - qu) cs-;  an invalid point keeps the prior.
//     (m+, cu+, cl+, cs+) are the outputs of step i.
//   predict (i < T-1; the one after the last step has no reader), h = t_{i+1} - t_i of any sign:
//     c = softmax(Wc m+ + bc);  A = sum_k c_k A_k, the four (lod x lod) blocks read straight from the flat banded bases
//     F = exp(A h);  W = int_0^h exp(A s) Q exp(A^T s) ds, Q = diag(q)       (= M2 exp(A h)^T of the reference's Van Loan block matrix)
//     m- = F m+;  (cu-, cl-, cs-) = the three block diagonals of F Sigma+ F^T + W, Sigma+ = [[diag cu+, diag cs+], [diag cs+, diag cl+]]
//
// exp and the integral together, by scaling and squaring: s = the least number of halvings that brings ||A h||_1 (computed here, per
// element and per step) to <= 1/2, capped at 16;  M = A h / 2^s, h0 = h / 2^s;
//     F_0 = sum_{j <= 8} M^j / j!  (Horner: R_8 = I + M / 8, R_k = I + M R_{k+1} / k, F_0 = R_1)
//     W_0 = sum_{j = 1..8} P_j,  P_1 = Q h0,  P_{j+1} = (M P_j + (M P_j)^T) / (j + 1)        (the Taylor series of the integral)
//     F_{l+1} = F_l F_l,  W_{l+1} = W_l + F_l W_l F_l^T                                        (s times)
// Truncation at norm 1/2: 0.5^9 / 9! = 5e-9.  The 2 lsd x 2 lsd block matrix and exp(-A^T h) are never formed.
//
// A workgroup of 256 threads owns one batch element and keeps the state and six (forward) / ten (backward) n x n matrices in LDS, rows
// LD = round_up(n, 4) + 4 floats apart (columns n .. LD-1 hold zeros, so a thread's four output columns are one 16-byte read per k and the
// eight rows a wave reads at once fall into eight different banks).  Products are on the VALU: at n = 32 every thread owns four
// outputs of a product, and the launch is bound by the chain of barriers, not by arithmetic.
//
// Backward, launch 1: time in reverse.  For step i the workgroup rebuilds the predict i-1 -> i from the saved posterior of step i-1 with
// the forward's code, leaving R_2..R_8, P_1..P_7 and (F_l, W_l) per squaring in its own stack in the workspace, pulls the cotangent of
// the posterior through the update (-> dy, dy_var), then through F m+, the block diagonals, the squarings
//     gW_l = gW_{l+1} + F_l^T gW_{l+1} F_l;  gF_l = F_l^T gF_{l+1} + gF_{l+1} F_l^T + (gW_{l+1} + gW_{l+1}^T) F_l W_l
// the Horner recurrence and the integral's series (exact adjoints of the recurrences above), the basis mix and the softmax.  The
// squarings' (gW + gW^T) F_l W_l stands for gW F_l W_l^T + gW^T F_l W_l: exact where W_l is symmetric bit for bit (every P_j, hence
// W_0), and up to the rounding of (F W) F^T after a squaring, far inside the fp32 bars.  Parameter
// gradients go into the workgroup's slab of the workspace: every entry has one owner thread, steps are separated by barriers.  Launch
// 2 adds the B slabs in index order: no atomics, the same inputs give the same bits.
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

constexpr int CRU_MAX_N = 32, CRU_MAX_K = 256, CRU_MAX_T = 1 << 20;
constexpr int CRU_THREADS = 256;
constexpr int CRU_DEG = 8;                 // degree of both series
constexpr int CRU_SMAX = 16;               // most squarings of a step
constexpr float CRU_THETA = 0.5f;          // the series run at ||M||_1 <= CRU_THETA
constexpr int CRU_SLOTS = 2 * (CRU_DEG - 1) + 2 * CRU_SMAX;      // matrices of a workgroup's stack
constexpr int CRU_FWD_BUFS = 6, CRU_BWD_BUFS = 10;

struct CruDims { int B, T, n, lod, LD, MS, K, E, bw, NV, vecs; };

__host__ __device__ inline int cru_entries(int lod, int bw) {
    int e = 0;
    for (int r = 0; r < lod; ++r) {
        const int lo = r - bw > 0 ? r - bw : 0, hi = r + bw < lod - 1 ? r + bw : lod - 1;
        e += hi - lo + 1;
    }
    return e;
}

inline CruDims cru_dims(int B, int T, int lsd, int K, int bw) {
    CruDims d{};
    d.B = B; d.T = T; d.n = lsd; d.lod = lsd / 2; d.LD = ((lsd + 3) & ~3) + 4; d.MS = lsd * d.LD; d.K = K; d.bw = bw;
    d.E = cru_entries(d.lod, bw);
    d.NV = 4 * K * d.E + K * lsd + K + lsd + 2 * d.lod;
    d.vecs = 12 * lsd + 2 * K + 64;        // the state vectors, the coefficients, the band's row starts and a reduction row
    return d;
}
inline size_t cru_lds_bytes(const CruDims& d, int bufs) { return sizeof(float) * ((size_t)bufs * d.MS + d.vecs); }

// C = (acc ? C : 0) + alpha op(A) B, op(A) = A^T if ta.  C is neither A nor B.  Ends with a barrier.
__device__ void cru_mm(float* C, const float* A, bool ta, const float* B, float alpha, bool acc, int n, int LD) {
    const int ncg = (n + 3) >> 2;
    for (int w = threadIdx.x; w < n * ncg; w += CRU_THREADS) {
        const int i = w / ncg, j0 = (w - i * ncg) << 2;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < n; ++k) {
            const float a = ta ? A[k * LD + i] : A[i * LD + k];
            s += a * *reinterpret_cast<const f32x4*>(B + k * LD + j0);
        }
        f32x4* c = reinterpret_cast<f32x4*>(C + i * LD + j0);
        *c = acc ? *c + alpha * s : alpha * s;
    }
    __syncthreads();
}
__device__ void cru_tr(float* D, const float* S, int n, int LD) {
    for (int e = threadIdx.x; e < n * n; e += CRU_THREADS) {
        const int i = e / n, j = e - i * n;
        D[j * LD + i] = S[i * LD + j];
    }
    __syncthreads();
}
__device__ void cru_put(float* g, const float* S, int MS) {      // LDS -> the stack; no barrier: nobody writes S before the next one
    if (!g) return;
    for (int e = threadIdx.x; e < MS; e += CRU_THREADS) g[e] = S[e];
}
__device__ void cru_get(float* D, const float* g, int MS) {
    for (int e = threadIdx.x; e < MS; e += CRU_THREADS) D[e] = g[e];
    __syncthreads();
}

struct CruPrm { const float *b11, *b12, *b21, *b22, *Wc, *bc, *q, *icu, *icl; };

// c = softmax(Wc m+ + bc) into cv (zs: K floats of scratch), then A = sum_k c_k A_k into M
__device__ void cru_transition(const CruDims& d, const CruPrm& p, const float* mpost, float* zs, float* cv, const int* rowstart, float* M) {
    const int n = d.n, lod = d.lod, K = d.K, LD = d.LD, E = d.E;
    for (int k = threadIdx.x; k < K; k += CRU_THREADS) {
        float z = p.bc[k];
        for (int j = 0; j < n; ++j) z += p.Wc[k * n + j] * mpost[j];
        zs[k] = z;
    }
    __syncthreads();
    float mx = zs[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, zs[k]);
    float sum = 0.f;
    for (int k = 0; k < K; ++k) sum += expf(zs[k] - mx);
    for (int k = threadIdx.x; k < K; k += CRU_THREADS) cv[k] = expf(zs[k] - mx) / sum;
    __syncthreads();
    for (int idx = threadIdx.x; idx < 4 * lod * lod; idx += CRU_THREADS) {
        const int pq = idx / (lod * lod), rc = idx - pq * lod * lod, r = rc / lod, c = rc - r * lod;
        const int lo = r - d.bw > 0 ? r - d.bw : 0;
        float v = 0.f;
        if (c >= lo && c <= r + d.bw) {
            const float* basis = (pq == 0 ? p.b11 : pq == 1 ? p.b12 : pq == 2 ? p.b21 : p.b22) + rowstart[r] + (c - lo);
            for (int k = 0; k < K; ++k) v += cv[k] * basis[(size_t)k * E];
        }
        M[((pq >> 1) * lod + r) * LD + (pq & 1) * lod + c] = v;
    }
    __syncthreads();
}

// M holds A on entry and A h / 2^s on exit; F -> exp(A h) and W -> the integral on exit (F / Fo swap).  P, X: scratch.  red: >= n floats.
// stack (null in the forward): what the adjoint reads back.  Returns s; h0 = h / 2^s.
__device__ int cru_expm(const CruDims& d, float h, const float* q, float* M, float*& F, float*& Fo, float* P, float* X, float* W, float* red,
                        float* stack, float& h0) {
    const int n = d.n, LD = d.LD, MS = d.MS;
    if (threadIdx.x < n) {
        float a = 0.f;
        for (int i = 0; i < n; ++i) a += fabsf(M[i * LD + threadIdx.x]);
        red[threadIdx.x] = a;
    }
    __syncthreads();
    float nrm = 0.f;
    for (int j = 0; j < n; ++j) nrm = fmaxf(nrm, red[j]);
    nrm *= fabsf(h);
    int s = 0;
    while (nrm > CRU_THETA && s < CRU_SMAX) { nrm *= 0.5f; ++s; }
    h0 = ldexpf(h, -s);
    for (int e = threadIdx.x; e < n * n; e += CRU_THREADS) {
        const int i = e / n, j = e - i * n;
        const float m = M[i * LD + j] * h0;
        M[i * LD + j] = m;
        F[i * LD + j] = (i == j ? 1.f : 0.f) + m * (1.f / CRU_DEG);
        const float p1 = i == j ? q[i] * h0 : 0.f;
        P[i * LD + j] = p1;
        W[i * LD + j] = p1;
    }
    __syncthreads();
    if (stack) { cru_put(stack + (size_t)(CRU_DEG - 2) * MS, F, MS); cru_put(stack + (size_t)(CRU_DEG - 1) * MS, P, MS); }
    for (int k = CRU_DEG - 1; k >= 1; --k) {                       // R_k = I + M R_{k+1} / k
        cru_mm(Fo, M, false, F, 1.f / k, false, n, LD);
        if (threadIdx.x < n) Fo[threadIdx.x * LD + threadIdx.x] += 1.f;
        __syncthreads();
        float* t = F; F = Fo; Fo = t;
        if (stack && k >= 2) cru_put(stack + (size_t)(k - 2) * MS, F, MS);
    }
    for (int j = 1; j < CRU_DEG; ++j) {                            // P_{j+1} = (M P_j + (M P_j)^T) / (j + 1)
        cru_mm(X, M, false, P, 1.f / (j + 1), false, n, LD);
        for (int e = threadIdx.x; e < n * n; e += CRU_THREADS) {
            const int i = e / n, c = e - i * n;
            const float v = X[i * LD + c] + X[c * LD + i];
            P[i * LD + c] = v;
            W[i * LD + c] += v;
        }
        __syncthreads();
        if (stack && j + 1 < CRU_DEG) cru_put(stack + (size_t)(CRU_DEG - 1 + j) * MS, P, MS);
    }
    for (int l = 0; l < s; ++l) {
        if (stack) {
            cru_put(stack + (size_t)(2 * (CRU_DEG - 1) + 2 * l) * MS, F, MS);
            cru_put(stack + (size_t)(2 * (CRU_DEG - 1) + 2 * l + 1) * MS, W, MS);
        }
        cru_tr(X, F, n, LD);
        cru_mm(P, F, false, W, 1.f, false, n, LD);
        cru_mm(W, P, false, X, 1.f, true, n, LD);
        cru_mm(Fo, F, false, F, 1.f, false, n, LD);
        float* t = F; F = Fo; Fo = t;
    }
    return s;
}

// m- = F m+ and the three block diagonals of F Sigma+ F^T + W
__device__ void cru_prior(const CruDims& d, const float* F, const float* W, const float* mpost, const float* cu, const float* cl, const float* cs,
                          float* mprior, float* pcu, float* pcl, float* pcs) {
    const int n = d.n, lod = d.lod, LD = d.LD;
    for (int w = threadIdx.x; w < n + lod; w += CRU_THREADS) {
        if (w < n) {
            float a = 0.f;
            for (int k = 0; k < n; ++k) a += F[w * LD + k] * mpost[k];
            mprior[w] = a;
        } else {
            const int i = w - n;
            const float *r0 = F + i * LD, *r1 = F + (lod + i) * LD;
            float u = 0.f, l = 0.f, s = 0.f;
            for (int k = 0; k < lod; ++k) {
                const float a = r0[k], b = r0[lod + k], a2 = r1[k], b2 = r1[lod + k], vu = cu[k], vl = cl[k], vs = cs[k];
                u += a * a * vu + 2.f * a * b * vs + b * b * vl;
                l += a2 * a2 * vu + 2.f * a2 * b2 * vs + b2 * b2 * vl;
                s += a * a2 * vu + (a * b2 + b * a2) * vs + b * b2 * vl;
            }
            pcu[i] = u + W[i * LD + i];
            pcl[i] = l + W[(lod + i) * LD + lod + i];
            pcs[i] = s + W[i * LD + lod + i];
        }
    }
    __syncthreads();
}

struct CruLds {
    float *mat, *mpost, *cu, *cl, *cs, *mprior, *pcu, *pcl, *pcs, *g0, *g1, *zs, *cv, *red;
    int* rowstart;
};
__device__ CruLds cru_carve(const CruDims& d, float* lds, int bufs) {
    CruLds s;
    s.mat = lds;
    float* v = lds + (size_t)bufs * d.MS;
    const int n = d.n, lod = d.lod;
    s.mpost = v; v += n; s.cu = v; v += lod; s.cl = v; v += lod;
    s.cs = v; v += lod; v += lod;
    s.mprior = v; v += n; s.pcu = v; v += lod; s.pcl = v; v += lod;
    s.pcs = v; v += lod; v += lod;
    s.g0 = v; v += 3 * n;          // backward: cotangent of the posterior (mean n | cu | cl | cs | -)
    s.g1 = v; v += 3 * n;          // backward: cotangent of the prior
    s.zs = v; v += d.K; s.cv = v; v += d.K;
    s.red = v; v += 32;
    s.rowstart = reinterpret_cast<int*>(v);
    return s;
}
__device__ void cru_begin(const CruDims& d, const CruLds& s, float* lds, int bufs) {
    for (int e = threadIdx.x; e < bufs * d.MS; e += CRU_THREADS) lds[e] = 0.f;
    if (threadIdx.x < d.lod) {
        int o = 0;
        for (int r = 0; r < (int)threadIdx.x; ++r) {
            const int lo = r - d.bw > 0 ? r - d.bw : 0, hi = r + d.bw < d.lod - 1 ? r + d.bw : d.lod - 1;
            o += hi - lo + 1;
        }
        s.rowstart[threadIdx.x] = o;
    }
    __syncthreads();
}

__global__ __launch_bounds__(CRU_THREADS) void cru_fwd_kernel(CruDims d, CruPrm p, const float* __restrict__ y, const float* __restrict__ yv,
                                                             const uint8_t* __restrict__ valid, const float* __restrict__ t,
                                                             float* __restrict__ pm, float* __restrict__ ocu, float* __restrict__ ocl,
                                                             float* __restrict__ ocs) {
    extern __shared__ __align__(16) float cru_lds[];
    const int b = blockIdx.x, n = d.n, lod = d.lod, T = d.T;
    const CruLds s = cru_carve(d, cru_lds, CRU_FWD_BUFS);
    cru_begin(d, s, cru_lds, CRU_FWD_BUFS);
    float *M = s.mat, *F = M + d.MS, *Fo = F + d.MS, *P = Fo + d.MS, *X = P + d.MS, *W = X + d.MS;
    if (threadIdx.x < lod) {
        const int i = threadIdx.x;
        s.mprior[i] = 0.f; s.mprior[lod + i] = 0.f;
        s.pcu[i] = p.icu[i]; s.pcl[i] = p.icl[i]; s.pcs[i] = 0.f;
    }
    __syncthreads();
    for (int i = 0; i < T; ++i) {
        const size_t row = (size_t)b * T + i;
        if (threadIdx.x < lod) {
            const int k = threadIdx.x;
            float mu = s.mprior[k], ml = s.mprior[lod + k], u = s.pcu[k], l = s.pcl[k], c = s.pcs[k];
            if (valid[row]) {
                const float den = u + yv[row * lod + k], qu = u / den, ql = c / den, r = y[row * lod + k] - mu;
                mu += qu * r; ml += ql * r;
                l = l - ql * c; c = (1.f - qu) * c; u = (1.f - qu) * u;
            }
            s.mpost[k] = mu; s.mpost[lod + k] = ml; s.cu[k] = u; s.cl[k] = l; s.cs[k] = c;
            pm[row * n + k] = mu; pm[row * n + lod + k] = ml;
            ocu[row * lod + k] = u; ocl[row * lod + k] = l; ocs[row * lod + k] = c;
        }
        __syncthreads();
        if (i == T - 1) break;
        const float h = t[row + 1] - t[row];
        cru_transition(d, p, s.mpost, s.zs, s.cv, s.rowstart, M);
        float h0;
        cru_expm(d, h, p.q, M, F, Fo, P, X, W, s.red, nullptr, h0);
        cru_prior(d, F, W, s.mpost, s.cu, s.cl, s.cs, s.mprior, s.pcu, s.pcl, s.pcs);
    }
}

__global__ __launch_bounds__(CRU_THREADS) void cru_bwd_kernel(CruDims d, CruPrm p, const float* __restrict__ y, const float* __restrict__ yv,
                                                             const uint8_t* __restrict__ valid, const float* __restrict__ t,
                                                             const float* __restrict__ pm, const float* __restrict__ ocu,
                                                             const float* __restrict__ ocl, const float* __restrict__ ocs,
                                                             const float* __restrict__ dpm, float* __restrict__ dy, float* __restrict__ dyv,
                                                             float* __restrict__ slabs, float* __restrict__ stacks) {
    extern __shared__ __align__(16) float cru_lds[];
    const int b = blockIdx.x, n = d.n, lod = d.lod, T = d.T, LD = d.LD, MS = d.MS, K = d.K, E = d.E;
    const CruLds s = cru_carve(d, cru_lds, CRU_BWD_BUFS);
    cru_begin(d, s, cru_lds, CRU_BWD_BUFS);
    float *M = s.mat, *F = M + MS, *Fo = F + MS, *P = Fo + MS, *X = P + MS, *W = X + MS;
    float *gF = W + MS, *gN = gF + MS, *gW = gN + MS, *gM = gW + MS;
    float* slab = slabs + (size_t)b * d.NV;
    float* stack = stacks + (size_t)b * CRU_SLOTS * MS;
    float *sl_b = slab, *sl_Wc = slab + 4 * K * E, *sl_bc = sl_Wc + K * n, *sl_q = sl_bc + K, *sl_icu = sl_q + n, *sl_icl = sl_icu + lod;
    for (int e = threadIdx.x; e < d.NV; e += CRU_THREADS) slab[e] = 0.f;
    // g0 = cotangent of the posterior of step i: mean | cu | cl | cs
    float *g0m = s.g0, *g0u = s.g0 + n, *g0l = g0u + lod, *g0s = g0l + lod;
    float *g1m = s.g1, *g1u = s.g1 + n, *g1l = g1u + lod, *g1s = g1l + lod;
    if (threadIdx.x < lod) { g0u[threadIdx.x] = 0.f; g0l[threadIdx.x] = 0.f; g0s[threadIdx.x] = 0.f; }
    if (threadIdx.x < n) g0m[threadIdx.x] = dpm[((size_t)b * T + T - 1) * n + threadIdx.x];
    __syncthreads();
    for (int i = T - 1; i >= 0; --i) {
        const size_t row = (size_t)b * T + i;
        int sq = 0;
        float h0 = 0.f;
        if (i > 0) {                                                   // the prior of step i, rebuilt from the posterior of step i-1
            if (threadIdx.x < lod) {
                const int k = threadIdx.x;
                s.mpost[k] = pm[(row - 1) * n + k]; s.mpost[lod + k] = pm[(row - 1) * n + lod + k];
                s.cu[k] = ocu[(row - 1) * lod + k]; s.cl[k] = ocl[(row - 1) * lod + k]; s.cs[k] = ocs[(row - 1) * lod + k];
            }
            __syncthreads();
            cru_transition(d, p, s.mpost, s.zs, s.cv, s.rowstart, M);
            sq = cru_expm(d, t[row] - t[row - 1], p.q, M, F, Fo, P, X, W, s.red, stack, h0);
            cru_prior(d, F, W, s.mpost, s.cu, s.cl, s.cs, s.mprior, s.pcu, s.pcl, s.pcs);
        } else {
            if (threadIdx.x < lod) {
                const int k = threadIdx.x;
                s.mprior[k] = 0.f; s.mprior[lod + k] = 0.f; s.pcu[k] = p.icu[k]; s.pcl[k] = p.icl[k]; s.pcs[k] = 0.f;
            }
            __syncthreads();
        }
        if (threadIdx.x < lod) {                                       // the update, backwards: g0 -> g1, dy, dy_var
            const int k = threadIdx.x;
            const float gmu = g0m[k], gml = g0m[lod + k], gu = g0u[k], gl = g0l[k], gs = g0s[k];
            float dyk = 0.f, dvk = 0.f;
            if (valid[row]) {
                const float u = s.pcu[k], c = s.pcs[k];
                const float den = u + yv[row * lod + k], qu = u / den, ql = c / den, r = y[row * lod + k] - s.mprior[k];
                const float gqu = gmu * r - gu * u - gs * c, gql = gml * r - gl * c, gr = gmu * qu + gml * ql;
                const float gden = -(gqu * qu + gql * ql) / den;
                g1m[k] = gmu - gr; g1m[lod + k] = gml;
                g1u[k] = gu * (1.f - qu) + gqu / den + gden;
                g1s[k] = gs * (1.f - qu) - gl * ql + gql / den;
                g1l[k] = gl;
                dyk = gr; dvk = gden;
            } else {
                g1m[k] = gmu; g1m[lod + k] = gml; g1u[k] = gu; g1l[k] = gl; g1s[k] = gs;
            }
            dy[row * lod + k] = dyk; dyv[row * lod + k] = dvk;
        }
        __syncthreads();
        if (i == 0) {
            if (threadIdx.x < lod) { sl_icu[threadIdx.x] += g1u[threadIdx.x]; sl_icl[threadIdx.x] += g1l[threadIdx.x]; }
            break;
        }
        // ---- the predict i-1 -> i, backwards.  gF, gW: cotangents of exp(A h) and of the integral
        for (int e = threadIdx.x; e < n * n; e += CRU_THREADS) {
            const int r = e / n, c = e - r * n, ri = r < lod ? r : r - lod, ck = c < lod ? c : c - lod;
            const float *r0 = F + ri * LD, *r1 = F + (lod + ri) * LD;
            const float a = r0[ck], bb = r0[lod + ck], a2 = r1[ck], b2 = r1[lod + ck], vu = s.cu[ck], vl = s.cl[ck], vs = s.cs[ck];
            const float gd = r < lod ? g1u[ri] : g1l[ri], gx = g1s[ri];
            float v;
            if (r < lod) v = c < lod ? gd * 2.f * (a * vu + bb * vs) + gx * (a2 * vu + b2 * vs) : gd * 2.f * (a * vs + bb * vl) + gx * (a2 * vs + b2 * vl);
            else v = c < lod ? gd * 2.f * (a2 * vu + b2 * vs) + gx * (a * vu + bb * vs) : gd * 2.f * (a2 * vs + b2 * vl) + gx * (a * vs + bb * vl);
            gF[r * LD + c] = v + g1m[r] * s.mpost[c];
            float w = 0.f;
            if (r == c) w = r < lod ? g1u[ri] : g1l[ri];
            else if (r < lod && c == r + lod) w = g1s[ri];
            gW[r * LD + c] = w;
        }
        // cotangent of the posterior of step i-1 through F and the block diagonals (the softmax's share is added below)
        for (int w = threadIdx.x; w < n + lod; w += CRU_THREADS) {
            if (w < n) {
                float a = 0.f;
                for (int k = 0; k < n; ++k) a += F[k * LD + w] * g1m[k];
                g0m[w] = a + dpm[(row - 1) * n + w];
            } else {
                const int k = w - n;
                float u = 0.f, l = 0.f, c = 0.f;
                for (int j = 0; j < lod; ++j) {
                    const float a = F[j * LD + k], bb = F[j * LD + lod + k], a2 = F[(lod + j) * LD + k], b2 = F[(lod + j) * LD + lod + k];
                    const float gu = g1u[j], gl = g1l[j], gs = g1s[j];
                    u += gu * a * a + gl * a2 * a2 + gs * a * a2;
                    c += 2.f * (gu * a * bb + gl * a2 * b2) + gs * (a * b2 + bb * a2);
                    l += gu * bb * bb + gl * b2 * b2 + gs * bb * b2;
                }
                g0u[k] = u; g0l[k] = l; g0s[k] = c;
            }
        }
        __syncthreads();
        for (int l = sq - 1; l >= 0; --l) {                            // the squarings; P = F_l, X = W_l, Fo / W: scratch
            cru_get(P, stack + (size_t)(2 * (CRU_DEG - 1) + 2 * l) * MS, MS);
            cru_get(X, stack + (size_t)(2 * (CRU_DEG - 1) + 2 * l + 1) * MS, MS);
            cru_mm(gN, P, true, gF, 1.f, false, n, LD);
            cru_tr(Fo, P, n, LD);
            cru_mm(gN, gF, false, Fo, 1.f, true, n, LD);
            cru_mm(W, P, false, X, 1.f, false, n, LD);                 // Z = F_l W_l
            for (int e = threadIdx.x; e < n * n; e += CRU_THREADS) {
                const int r = e / n, c = e - r * n;
                X[r * LD + c] = gW[r * LD + c] + gW[c * LD + r];
            }
            __syncthreads();
            cru_mm(gN, X, false, W, 1.f, true, n, LD);
            { float* tp = gF; gF = gN; gN = tp; }
            cru_mm(W, gW, false, P, 1.f, false, n, LD);                // U = gW F_l
            cru_mm(gW, P, true, W, 1.f, true, n, LD);
        }
        // Horner, backwards: g = gF_0;  gM = sum_k g_k R_{k+1}^T / k + g_DEG / DEG,  g_{k+1} = M^T g_k / k
        for (int k = 1; k < CRU_DEG; ++k) {
            cru_get(P, stack + (size_t)(k - 1) * MS, MS);              // R_{k+1}
            cru_tr(X, P, n, LD);
            cru_mm(gM, gF, false, X, 1.f / k, k > 1, n, LD);
            cru_mm(gN, M, true, gF, 1.f / k, false, n, LD);
            { float* tp = gF; gF = gN; gN = tp; }
        }
        for (int e = threadIdx.x; e < n * n; e += CRU_THREADS) {
            const int r = e / n, c = e - r * n;
            gM[r * LD + c] += gF[r * LD + c] * (1.f / CRU_DEG);
        }
        __syncthreads();
        // the integral's series, backwards: H = gP_{j+1} (H = gW at j + 1 = DEG), S = (H + H^T) / (j + 1), gM += S P_j, gP_j = gW + M^T S
        const float* H = gW;
        for (int j = CRU_DEG - 1; j >= 1; --j) {
            for (int e = threadIdx.x; e < n * n; e += CRU_THREADS) {
                const int r = e / n, c = e - r * n;
                X[r * LD + c] = (H[r * LD + c] + H[c * LD + r]) * (1.f / (j + 1));
            }
            __syncthreads();
            cru_get(P, stack + (size_t)(CRU_DEG - 1 + j - 1) * MS, MS);       // P_j
            cru_mm(gM, X, false, P, 1.f, true, n, LD);
            cru_mm(W, M, true, X, 1.f, false, n, LD);
            for (int e = threadIdx.x; e < n * n; e += CRU_THREADS) {
                const int r = e / n, c = e - r * n;
                gN[r * LD + c] = gW[r * LD + c] + W[r * LD + c];
            }
            __syncthreads();
            H = gN;
        }
        if (threadIdx.x < n) sl_q[threadIdx.x] += h0 * H[threadIdx.x * LD + threadIdx.x];      // P_1 = diag(q) h0
        // gA = h0 gM: the bases, the coefficients
        for (int idx = threadIdx.x; idx < 4 * lod * lod; idx += CRU_THREADS) {
            const int pq = idx / (lod * lod), rc = idx - pq * lod * lod, r = rc / lod, c = rc - r * lod;
            const int lo = r - d.bw > 0 ? r - d.bw : 0;
            if (c >= lo && c <= r + d.bw) {
                const float g = h0 * gM[((pq >> 1) * lod + r) * LD + (pq & 1) * lod + c];
                float* dst = sl_b + (size_t)pq * K * E + s.rowstart[r] + (c - lo);
                for (int k = 0; k < K; ++k) dst[(size_t)k * E] += s.cv[k] * g;
            }
        }
        for (int k = threadIdx.x; k < K; k += CRU_THREADS) {
            float a = 0.f;
            for (int pq = 0; pq < 4; ++pq) {
                const float* basis = (pq == 0 ? p.b11 : pq == 1 ? p.b12 : pq == 2 ? p.b21 : p.b22) + (size_t)k * E;
                int e = 0;
                for (int r = 0; r < lod; ++r) {
                    const int lo = r - d.bw > 0 ? r - d.bw : 0, hi = r + d.bw < lod - 1 ? r + d.bw : lod - 1;
                    const float* g = gM + ((pq >> 1) * lod + r) * LD + (pq & 1) * lod;
                    for (int c = lo; c <= hi; ++c) a += basis[e++] * g[c];
                }
            }
            s.zs[k] = a * h0;                                          // cotangent of c_k
        }
        __syncthreads();
        float dot = 0.f;
        for (int k = 0; k < K; ++k) dot += s.cv[k] * s.zs[k];
        __syncthreads();
        for (int k = threadIdx.x; k < K; k += CRU_THREADS) {
            const float gz = s.cv[k] * (s.zs[k] - dot);
            s.zs[k] = gz;
            sl_bc[k] += gz;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < K * n; e += CRU_THREADS) sl_Wc[e] += s.zs[e / n] * s.mpost[e % n];
        if (threadIdx.x < n) {
            float a = 0.f;
            for (int k = 0; k < K; ++k) a += p.Wc[k * n + threadIdx.x] * s.zs[k];
            g0m[threadIdx.x] += a;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(CRU_THREADS) void cru_fold_kernel(int NV, int B, const float* __restrict__ slabs, float* __restrict__ grads) {
    const int i = blockIdx.x * CRU_THREADS + threadIdx.x;
    if (i >= NV) return;
    float a = 0.f;
    for (int b = 0; b < B; ++b) a += slabs[(size_t)b * NV + i];
    grads[i] = a;
}

bool cru_call_ok(int B, int T, int lsd, int K, int bw) {
    return B >= 1 && immtsf_cru_supported(lsd, K, bw, T) && (int64_t)B * T * lsd < (1ll << 31);
}

}  // namespace

extern "C" {

int immtsf_cru_supported(int32_t lsd, int32_t num_basis, int32_t bandwidth, int32_t T) {
    if (lsd < 2 || lsd > CRU_MAX_N || (lsd & 1) || num_basis < 1 || num_basis > CRU_MAX_K || bandwidth < 0 || bandwidth > lsd / 2 ||
        T < 1 || T > CRU_MAX_T)
        return 0;
    return cru_lds_bytes(cru_dims(1, T, lsd, num_basis, bandwidth), CRU_BWD_BUFS) <= 64 * 1024;
}

int32_t immtsf_cru_grad_layout(int32_t lsd, int32_t num_basis, int32_t bandwidth, int32_t* offsets, int32_t n_offsets) {
    if (!immtsf_cru_supported(lsd, num_basis, bandwidth, 1)) return -1;
    const CruDims d = cru_dims(1, 1, lsd, num_basis, bandwidth);
    const int KE = d.K * d.E;
    const int o[9] = {0, KE, 2 * KE, 3 * KE, 4 * KE, 4 * KE + d.K * d.n, 4 * KE + d.K * d.n + d.K, 4 * KE + d.K * d.n + d.K + d.n,
                      4 * KE + d.K * d.n + d.K + d.n + d.lod};
    for (int i = 0; offsets && i < 9 && i < n_offsets; ++i) offsets[i] = o[i];
    return d.NV;
}

size_t immtsf_cru_workspace_bytes(int32_t B, int32_t T, int32_t lsd, int32_t num_basis, int32_t bandwidth) {
    if (!cru_call_ok(B, T, lsd, num_basis, bandwidth)) return 0;
    const CruDims d = cru_dims(B, T, lsd, num_basis, bandwidth);
    return sizeof(float) * ((size_t)B * d.NV + 64 + (size_t)B * CRU_SLOTS * d.MS) + 256;
}

int immtsf_cru_forward(int32_t B, int32_t T, int32_t lsd, int32_t num_basis, int32_t bandwidth, const float* y, const float* y_var,
                       const uint8_t* valid, const float* t, const float* tm11, const float* tm12, const float* tm21, const float* tm22,
                       const float* coef_w, const float* coef_b, const float* trans_var, const float* icu, const float* icl, float* post_mean,
                       float* post_cu, float* post_cl, float* post_cs, immtsf_stream_t stream) {
    if (B < 0 || T < 1 || lsd < 1 || num_basis < 1 || bandwidth < 0) return IMMTSF_EINVAL;
    if (!immtsf_cru_supported(lsd, num_basis, bandwidth, T)) return IMMTSF_EUNSUPPORTED;
    if (B == 0) return IMMTSF_OK;
    if (!cru_call_ok(B, T, lsd, num_basis, bandwidth)) return IMMTSF_EINVAL;
    if (!y || !y_var || !valid || !t || !tm11 || !tm12 || !tm21 || !tm22 || !coef_w || !coef_b || !trans_var || !icu || !icl || !post_mean ||
        !post_cu || !post_cl || !post_cs)
        return IMMTSF_EINVAL;
    const CruDims d = cru_dims(B, T, lsd, num_basis, bandwidth);
    const CruPrm p{tm11, tm12, tm21, tm22, coef_w, coef_b, trans_var, icu, icl};
    hipLaunchKernelGGL(cru_fwd_kernel, dim3(B), dim3(CRU_THREADS), cru_lds_bytes(d, CRU_FWD_BUFS), static_cast<hipStream_t>(stream), d, p, y,
                       y_var, valid, t, post_mean, post_cu, post_cl, post_cs);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_cru_backward(int32_t B, int32_t T, int32_t lsd, int32_t num_basis, int32_t bandwidth, const float* y, const float* y_var,
                        const uint8_t* valid, const float* t, const float* tm11, const float* tm12, const float* tm21, const float* tm22,
                        const float* coef_w, const float* coef_b, const float* trans_var, const float* icu, const float* icl,
                        const float* post_mean, const float* post_cu, const float* post_cl, const float* post_cs, const float* d_post_mean,
                        float* dy, float* dy_var, float* grads, void* workspace, size_t workspace_bytes, immtsf_stream_t stream) {
    if (B < 1 || T < 1 || lsd < 1 || num_basis < 1 || bandwidth < 0) return IMMTSF_EINVAL;
    if (!immtsf_cru_supported(lsd, num_basis, bandwidth, T)) return IMMTSF_EUNSUPPORTED;
    if (!cru_call_ok(B, T, lsd, num_basis, bandwidth)) return IMMTSF_EINVAL;
    if (!y || !y_var || !valid || !t || !tm11 || !tm12 || !tm21 || !tm22 || !coef_w || !coef_b || !trans_var || !icu || !icl || !post_mean ||
        !post_cu || !post_cl || !post_cs || !d_post_mean || !dy || !dy_var || !grads || !workspace)
        return IMMTSF_EINVAL;
    if (workspace_bytes < immtsf_cru_workspace_bytes(B, T, lsd, num_basis, bandwidth)) return IMMTSF_EWORKSPACE;
    float* ws = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t(255));
    const CruDims d = cru_dims(B, T, lsd, num_basis, bandwidth);
    const CruPrm p{tm11, tm12, tm21, tm22, coef_w, coef_b, trans_var, icu, icl};
    float* stacks = ws + (((size_t)B * d.NV + 63) & ~size_t(63));
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cru_bwd_kernel, dim3(B), dim3(CRU_THREADS), cru_lds_bytes(d, CRU_BWD_BUFS), s, d, p, y, y_var, valid, t, post_mean,
                       post_cu, post_cl, post_cs, d_post_mean, dy, dy_var, ws, stacks);
    IMMTSF_LAUNCH_CHECK();
    hipLaunchKernelGGL(cru_fold_kernel, dim3(cdiv(d.NV, CRU_THREADS)), dim3(CRU_THREADS), 0, s, d.NV, B, ws, grads);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
