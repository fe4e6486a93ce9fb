// Evaluation metrics (lib/evaluation.py evaluation()): the per-element terms and the cross-workgroup fold that the standalone
// kernel (eval.hip) and the fused Q-half kernel (xrank.hip) share.
#pragma once
#include "common.hpp"

constexpr int EVAL_STATS = 5;      // se, ae, ape, cnt, cnt_ape

// The reference's definitions per element (fp32, its operation order): se = (t-p)^2 m, ae = |t-p| m, cnt = m; m2 = (t != 0) m,
// ape = |t-p| / t * m2 (the divisor is SIGNED), cnt_ape = m2.  A select stands for the multiply by (t != 0): the two differ only
// where |p| / 1e-8 overflows fp32 (the reference then gets inf * 0).
__device__ __forceinline__ void eval_terms(float t, float p, float m, float (&e)[EVAL_STATS]) {
    const float d = t - p, a = fabsf(d);
    const bool nz = t != 0.f;
    e[0] = d * d * m;
    e[1] = a * m;
    e[2] = nz ? a / t * m : 0.f;
    e[3] = m;
    e[4] = nz ? m : 0.f;
}

// Called by every thread of the LAST workgroup to finish (behind its ticket and a __threadfence): acc[i] += the G slabs' values in a
// fixed order (four interleaved chains, then ((0+1)+(2+3))) in fp64 -- no atomics, so a pass over the same batches repeats bit for bit.
__device__ __forceinline__ void eval_fold_slabs(const double* slabs, int G, int NV, double* __restrict__ acc) {
    for (int i = threadIdx.x; i < NV; i += blockDim.x) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int g = 0;
        for (; g + 3 < G; g += 4) {
            a0 += __builtin_nontemporal_load(slabs + (size_t)g * NV + i);
            a1 += __builtin_nontemporal_load(slabs + (size_t)(g + 1) * NV + i);
            a2 += __builtin_nontemporal_load(slabs + (size_t)(g + 2) * NV + i);
            a3 += __builtin_nontemporal_load(slabs + (size_t)(g + 3) * NV + i);
        }
        for (; g < G; ++g) a0 += __builtin_nontemporal_load(slabs + (size_t)g * NV + i);
        acc[i] += (a0 + a1) + (a2 + a3);
    }
}
