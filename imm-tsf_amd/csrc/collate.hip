// Device-side batch builder: the dataset's windows live in HBM as window-major CSR arrays (the
// "resident store"); a batch is a list of window ids.  These kernels emit exactly what the reference's collate
// functions return -- zero-padded history / prediction tensors with normalised times
// (lib/parse_datasets.py:252-295; CRU's raw-time form, :369-408, is the same kernel with time_max = 1),
// tPatchGNN's per-(patch, variable) compacted patches (:298-366 with lib/utils.py:359-413), LatentODE's grid on
// the batch's shared time axis (:411-471, immtsf_collate_union: a gather, every element written once) and the
// multimodal part, tau + zero-padded note embeddings (:764-824) -- plus the packed
// ragged note index (lengths / offsets / row map into the resident embedding matrix) that the fusion kernels use,
// so the padded embeddings and the |V|-sum mask re-derivation can be skipped.  Pure gathers: HBM-bound, bit-exact.
#include "../../include/immtsf.h"
#include "common.hpp"

namespace {

// the reference normalises with (tp - 0.0) / scale, scale = time_max + (time_max == 0) * 1e-8 (lib/utils.py:335-347)
__device__ __forceinline__ float norm_tp(float t, float scale) { return (t - 0.0f) / scale; }

// grid (B, chunks): history rows are the prefix [0, hist_len) of a window (times ascending), prediction rows the rest
__global__ __launch_bounds__(256) void collate_series_kernel(immtsf_store s, const int32_t* __restrict__ wid, int Lmax, int Lpmax,
                                                              float scale, float* __restrict__ otp, float* __restrict__ odat,
                                                              float* __restrict__ omsk, float* __restrict__ ptp,
                                                              float* __restrict__ pdat, float* __restrict__ pmsk) {
    const int b = blockIdx.x, w = wid[b], C = s.C;
    const long r0 = s.row_off[w];
    const int len = (int)(s.row_off[w + 1] - r0), hl = s.hist_len[w], pl = len - hl;
    const int stride = gridDim.y * 256, t0 = blockIdx.y * 256 + threadIdx.x;
    if (otp) {
        for (int i = t0; i < Lmax; i += stride) otp[(size_t)b * Lmax + i] = i < hl ? norm_tp(s.tt[r0 + i], scale) : 0.f;
        for (int i = t0; i < Lmax * C; i += stride) {
            const int l = i / C;
            const bool live = l < hl;
            odat[(size_t)b * Lmax * C + i] = live ? s.vals[(r0 + l) * C + (i - l * C)] : 0.f;
            omsk[(size_t)b * Lmax * C + i] = live ? s.mask[(r0 + l) * C + (i - l * C)] : 0.f;
        }
    }
    for (int i = t0; i < Lpmax; i += stride) ptp[(size_t)b * Lpmax + i] = i < pl ? norm_tp(s.tt[r0 + hl + i], scale) : 0.f;
    for (int i = t0; i < Lpmax * C; i += stride) {
        const int l = i / C;
        const bool live = l < pl;
        pdat[(size_t)b * Lpmax * C + i] = live ? s.vals[(r0 + hl + l) * C + (i - l * C)] : 0.f;
        pmsk[(size_t)b * Lpmax * C + i] = live ? s.mask[(r0 + hl + l) * C + (i - l * C)] : 0.f;
    }
}

// grid (B, npatch), one wave per variable (waves loop over C): ballot-compaction of the observed rows of variable d
// whose time lies in patch i's range, in time order, into slots 0..count-1 of out[b, i, :, d]; remaining slots zero
__global__ __launch_bounds__(256) void collate_patches_kernel(immtsf_store s, const int32_t* __restrict__ wid, int npatch,
                                                               float patch_size, float patch_stride, float history, int Lp,
                                                               float scale, float* __restrict__ otp, float* __restrict__ odat,
                                                               float* __restrict__ omsk) {
    const int b = blockIdx.x, i = blockIdx.y, w = wid[b], C = s.C;
    const long r0 = s.row_off[w];
    const int hl = s.hist_len[w];
    const float st = (float)i * patch_stride, ed = (i == npatch - 1) ? history : st + patch_size;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const size_t base = ((size_t)b * npatch + i) * Lp * C;
    for (int d = wave; d < C; d += nw) {
        int count = 0;
        for (int j0 = 0; j0 < hl; j0 += 64) {
            const int j = j0 + lane;
            float t = 0.f, m = 0.f;
            bool hit = false;
            if (j < hl) {
                t = s.tt[r0 + j];
                m = s.mask[(r0 + j) * C + d];
                hit = (t >= st) && (t < ed) && (m != 0.f);
            }
            const unsigned long long bal = __ballot(hit);
            if (hit) {
                const int slot = count + __popcll(bal & ((1ull << lane) - 1ull));
                const size_t o = base + (size_t)slot * C + d;
                otp[o] = norm_tp(t, scale);
                odat[o] = s.vals[(r0 + j) * C + d];
                omsk[o] = m;
            }
            count += __popcll(bal);
        }
        for (int l = count + lane; l < Lp; l += 64) {
            const size_t o = base + (size_t)l * C + d;
            otp[o] = 0.f;
            odat[o] = 0.f;
            omsk[o] = 0.f;
        }
    }
}

// LatentODE's axis time (lib/parse_datasets.py:448-454): normalize_masked_tp, then + j * eps; torch rounds the division, the
// product and the sum to fp32 one by one.  hipcc contracts a * b + c into an FMA by default, and its __fmul_rn / __fadd_rn
// are the plain operators, so contraction is switched off for this function: one FMA changes the last bit.
__device__ __forceinline__ float union_tp(float u, int j, float scale, float eps) {
#pragma clang fp contract(off)
    const float jitter = (float)j * eps;
    const float t = norm_tp(u, scale);
    return t + jitter;
}

// the LAST row of a window's non-decreasing time slice whose time equals u (upper bound - 1, tested for equality), or -1.
// Last, because the reference's index_put on the CPU lets the later of two rows with one timestamp win.
__device__ __forceinline__ int union_row(const float* __restrict__ tt, int len, float u) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tt[mid] <= u) lo = mid + 1; else hi = mid;
    }
    return (lo > 0 && tt[lo - 1] == u) ? lo - 1 : -1;
}

// one window's slab (n axis points x C) of one half of the grid; dat / msk point at the slab.  16-byte stores where the slab
// length and both bases allow it (zeros are the bulk of the bytes), scalar stores otherwise
__device__ __forceinline__ void union_half(const immtsf_store& s, long r0, int len, const float* __restrict__ axis, int n,
                                           float* __restrict__ dat, float* __restrict__ msk, int t0, int stride) {
    const int C = s.C, total = n * C;            // T * C <= 2^30 (checked at the entry point)
    const float* __restrict__ tt = s.tt + r0;
    if ((total & 3) == 0 && ((reinterpret_cast<uintptr_t>(dat) | reinterpret_cast<uintptr_t>(msk)) & 15) == 0) {
        for (int q = t0; q < total / 4; q += stride) {
            float v[4], m[4];
            int j = q * 4 / C, c = q * 4 - j * C;
            int row = union_row(tt, len, axis[j]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = row >= 0 ? s.vals[(size_t)(r0 + row) * C + c] : 0.f;
                m[k] = row >= 0 ? s.mask[(size_t)(r0 + row) * C + c] : 0.f;
                if (++c == C && k < 3) {
                    c = 0;
                    ++j;
                    row = union_row(tt, len, axis[j]);
                }
            }
            reinterpret_cast<float4*>(dat)[q] = make_float4(v[0], v[1], v[2], v[3]);
            reinterpret_cast<float4*>(msk)[q] = make_float4(m[0], m[1], m[2], m[3]);
        }
    } else {
        for (int i = t0; i < total; i += stride) {
            const int j = i / C, c = i - j * C;
            const int row = union_row(tt, len, axis[j]);
            dat[i] = row >= 0 ? s.vals[(size_t)(r0 + row) * C + c] : 0.f;
            msk[i] = row >= 0 ? s.mask[(size_t)(r0 + row) * C + c] : 0.f;
        }
    }
}

// grid (B, chunks): cell (b, j) of the (B, T, C) grid holds the row of window b whose time equals axis[j], else zeros; axis points
// below n_obs go to the observed pair, the rest to the predicted pair.  The blocks of b == 0 also write the T axis times.
__global__ __launch_bounds__(256) void collate_union_kernel(immtsf_store s, const int32_t* __restrict__ wid,
                                                             const float* __restrict__ axis, int T, int n_obs, float scale, float eps,
                                                             float* __restrict__ otp, float* __restrict__ odat, float* __restrict__ omsk,
                                                             float* __restrict__ ptp, float* __restrict__ pdat, float* __restrict__ pmsk) {
    const int b = blockIdx.x, w = wid[b], C = s.C, n_pred = T - n_obs;
    const long r0 = s.row_off[w];
    const int len = (int)(s.row_off[w + 1] - r0);
    const int stride = gridDim.y * 256, t0 = blockIdx.y * 256 + threadIdx.x;
    if (b == 0) {
        for (int j = t0; j < T; j += stride) {
            const float t = union_tp(axis[j], j, scale, eps);
            if (j < n_obs) otp[j] = t; else ptp[j - n_obs] = t;
        }
    }
    if (n_obs > 0) union_half(s, r0, len, axis, n_obs, odat + (size_t)b * n_obs * C, omsk + (size_t)b * n_obs * C, t0, stride);
    if (n_pred > 0) union_half(s, r0, len, axis + n_obs, n_pred, pdat + (size_t)b * n_pred * C, pmsk + (size_t)b * n_pred * C, t0, stride);
}

// one block: lengths[b] = notes of window b, offsets = exclusive scan (B+1 entries)
__global__ __launch_bounds__(256) void note_index_kernel(immtsf_store s, const int32_t* __restrict__ wid, int B,
                                                          int32_t* __restrict__ lengths, int32_t* __restrict__ offsets) {
    __shared__ int part[256];
    const int tid = threadIdx.x, per = (B + 255) / 256, b0 = tid * per, b1 = min(B, b0 + per);
    int sum = 0;
    for (int b = b0; b < b1; ++b) {
        const int w = wid[b];
        const int n = (int)(s.note_off[w + 1] - s.note_off[w]);
        lengths[b] = n;
        sum += n;
    }
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = run; run += v; }
        offsets[B] = run;
    }
    __syncthreads();
    int run = part[tid];
    for (int b = b0; b < b1; ++b) {
        offsets[b] = run;
        run += lengths[b];
    }
}

// grid (B, chunks): tau / padded embeddings / packed row map
__global__ __launch_bounds__(256) void collate_notes_kernel(immtsf_store s, const int32_t* __restrict__ wid, int Nmax,
                                                             const int32_t* __restrict__ offsets, float* __restrict__ tau,
                                                             float* __restrict__ notes, int32_t* __restrict__ rowmap) {
    const int b = blockIdx.x, w = wid[b], d_m = s.d_m;
    const long n0 = s.note_off[w];
    const int n = (int)(s.note_off[w + 1] - n0);
    const int stride = gridDim.y * 256, t0 = blockIdx.y * 256 + threadIdx.x;
    for (int i = t0; i < Nmax; i += stride) {
        if (tau) tau[(size_t)b * Nmax + i] = i < n ? s.note_tau[n0 + i] : 0.f;
        if (rowmap && i < n) rowmap[offsets[b] + i] = (int32_t)s.note_src[n0 + i];
    }
    if (notes) {
        const int q = d_m / 4;
        if ((d_m & 3) == 0 && ((reinterpret_cast<uintptr_t>(s.emb) | reinterpret_cast<uintptr_t>(notes)) & 15) == 0) {
            for (long i = t0; i < (long)Nmax * q; i += stride) {
                const int r = (int)(i / q), c = (int)(i - (long)r * q);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r < n) v = reinterpret_cast<const float4*>(s.emb + (size_t)s.note_src[n0 + r] * d_m)[c];
                reinterpret_cast<float4*>(notes + ((size_t)b * Nmax + r) * d_m)[c] = v;
            }
        } else {
            for (long i = t0; i < (long)Nmax * d_m; i += stride) {
                const int r = (int)(i / d_m), c = (int)(i - (long)r * d_m);
                notes[((size_t)b * Nmax + r) * d_m + c] = r < n ? s.emb[(size_t)s.note_src[n0 + r] * d_m + c] : 0.f;
            }
        }
    }
}

// sum over the block's 256 threads, in every thread (integers: the order of the additions does not matter)
__device__ __forceinline__ int block_sum_int(int v, int* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// A whole standard / CRU batch as ONE launch, grid (B, chunks): what collate_series_kernel, note_index_kernel and collate_notes_kernel
// write between them.  offsets[b] is the number of notes of the windows in front of b; every block sums those counts for its own b
// (B is a few thousand at most: at most a few loads per thread; blocks that write no index entry skip the sum), so the prefix sum
// needs no second launch, no atomics and no block reads what another one wrote.  The blocks of chunk 0 write lengths / offsets, the block of the last window also offsets[B].
__global__ __launch_bounds__(256) void collate_batch_kernel(immtsf_store s, const int32_t* __restrict__ wid, int B, int Lmax, int Lpmax,
                                                             int Nmax, float scale, float* __restrict__ otp, float* __restrict__ odat,
                                                             float* __restrict__ omsk, float* __restrict__ ptp, float* __restrict__ pdat,
                                                             float* __restrict__ pmsk, float* __restrict__ tau, float* __restrict__ notes,
                                                             int32_t* __restrict__ lengths, int32_t* __restrict__ offsets,
                                                             int32_t* __restrict__ rowmap) {
    __shared__ int red[4];
    const int b = blockIdx.x, w = wid[b], C = s.C, d_m = s.d_m;
    const int stride = gridDim.y * 256, t0 = blockIdx.y * 256 + threadIdx.x;
    // ---- the note index.  Only the blocks that write lengths / offsets (chunk 0) or a row-map entry (a thread with t0 < n) need the
    // offset; the condition is the same for the whole block, so the barrier inside block_sum_int is met by all of its threads or none
    const long n0 = s.note_off[w];
    const int n = (int)(s.note_off[w + 1] - n0);
    int off = 0;
    if (blockIdx.y == 0 || (int)(blockIdx.y * 256) < n) {
        int before = 0;
        for (int j = threadIdx.x; j < b; j += 256) {
            const int wj = wid[j];
            before += (int)(s.note_off[wj + 1] - s.note_off[wj]);
        }
        off = block_sum_int(before, red);
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        lengths[b] = n;
        offsets[b] = off;
        if (b == B - 1) offsets[B] = off + n;
    }
    // ---- the six series tensors (collate_series_kernel)
    const long r0 = s.row_off[w];
    const int len = (int)(s.row_off[w + 1] - r0), hl = s.hist_len[w], pl = len - hl;
    for (int i = t0; i < Lmax; i += stride) otp[(size_t)b * Lmax + i] = i < hl ? norm_tp(s.tt[r0 + i], scale) : 0.f;
    for (int i = t0; i < Lmax * C; i += stride) {
        const int l = i / C;
        const bool live = l < hl;
        odat[(size_t)b * Lmax * C + i] = live ? s.vals[(r0 + l) * C + (i - l * C)] : 0.f;
        omsk[(size_t)b * Lmax * C + i] = live ? s.mask[(r0 + l) * C + (i - l * C)] : 0.f;
    }
    for (int i = t0; i < Lpmax; i += stride) ptp[(size_t)b * Lpmax + i] = i < pl ? norm_tp(s.tt[r0 + hl + i], scale) : 0.f;
    for (int i = t0; i < Lpmax * C; i += stride) {
        const int l = i / C;
        const bool live = l < pl;
        pdat[(size_t)b * Lpmax * C + i] = live ? s.vals[(r0 + hl + l) * C + (i - l * C)] : 0.f;
        pmsk[(size_t)b * Lpmax * C + i] = live ? s.mask[(r0 + hl + l) * C + (i - l * C)] : 0.f;
    }
    // ---- tau, the packed row map and the padded embeddings (collate_notes_kernel)
    for (int i = t0; i < Nmax; i += stride) {
        tau[(size_t)b * Nmax + i] = i < n ? s.note_tau[n0 + i] : 0.f;
        if (i < n) rowmap[off + i] = (int32_t)s.note_src[n0 + i];
    }
    if (notes) {
        const int q = d_m / 4;
        if ((d_m & 3) == 0 && ((reinterpret_cast<uintptr_t>(s.emb) | reinterpret_cast<uintptr_t>(notes)) & 15) == 0) {
            for (long i = t0; i < (long)Nmax * q; i += stride) {
                const int r = (int)(i / q), c = (int)(i - (long)r * q);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r < n) v = reinterpret_cast<const float4*>(s.emb + (size_t)s.note_src[n0 + r] * d_m)[c];
                reinterpret_cast<float4*>(notes + ((size_t)b * Nmax + r) * d_m)[c] = v;
            }
        } else {
            for (long i = t0; i < (long)Nmax * d_m; i += stride) {
                const int r = (int)(i / d_m), c = (int)(i - (long)r * d_m);
                notes[((size_t)b * Nmax + r) * d_m + c] = r < n ? s.emb[(size_t)s.note_src[n0 + r] * d_m + c] : 0.f;
            }
        }
    }
}

// one wave per window: the largest number of observed history points any (patch, variable) pair of the window holds -- the slot count
// collate_patches_kernel needs, found with the same comparisons (t >= st, t < ed, the last patch ending at `history`, mask != 0)
__global__ __launch_bounds__(256) void patch_max_kernel(immtsf_store s, int W, int npatch, float patch_size, float patch_stride,
                                                         float history, int32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, w = blockIdx.x * 4 + (threadIdx.x >> 6), C = s.C;
    if (w >= W) return;                      // wave-uniform
    const long r0 = s.row_off[w];
    const int hl = s.hist_len[w];
    int best = 0;
    for (int i = 0; i < npatch; ++i) {
        const float st = (float)i * patch_stride, ed = (i == npatch - 1) ? history : st + patch_size;
        for (int d = 0; d < C; ++d) {
            int count = 0;
            for (int j0 = 0; j0 < hl; j0 += 64) {
                const int j = j0 + lane;
                bool hit = false;
                if (j < hl) {
                    const float t = s.tt[r0 + j];
                    hit = (t >= st) && (t < ed) && (s.mask[(r0 + j) * C + d] != 0.f);
                }
                count += __popcll(__ballot(hit));
            }
            best = count > best ? count : best;
        }
    }
    if (lane == 0) out[w] = best;
}

bool store_ok(const immtsf_store* s) {
    return s && s->tt && s->vals && s->mask && s->row_off && s->hist_len && s->C > 0;
}

}  // namespace

extern "C" {

int immtsf_collate_series(const immtsf_store* s, const int32_t* window_ids, int32_t B, int32_t Lmax, int32_t Lpmax,
                          float time_max, float* obs_tp, float* obs_data, float* obs_mask, float* pred_tp,
                          float* pred_data, float* pred_mask, immtsf_stream_t stream) {
    if (!store_ok(s) || !window_ids || B < 0 || Lmax < 0 || Lpmax < 0 || !pred_tp || !pred_data || !pred_mask) return IMMTSF_EINVAL;
    if ((obs_tp != nullptr) != (obs_data != nullptr) || (obs_tp != nullptr) != (obs_mask != nullptr)) return IMMTSF_EINVAL;
    if (B == 0) return IMMTSF_OK;
    float scale = time_max - 0.0f;
    scale = scale + (scale == 0.f ? 1.f : 0.f) * 1e-8f;
    const int work = (Lmax > Lpmax ? Lmax : Lpmax) * s->C;
    hipLaunchKernelGGL(collate_series_kernel, dim3(B, work > 0 ? cdiv(work, 256) : 1), dim3(256), 0,
                       static_cast<hipStream_t>(stream), *s, window_ids, Lmax, Lpmax, scale, obs_tp, obs_data, obs_mask, pred_tp,
                       pred_data, pred_mask);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_collate_patches(const immtsf_store* s, const int32_t* window_ids, int32_t B, int32_t npatch, float patch_size,
                           float patch_stride, float history, int32_t Lp, float time_max, float* obs_tp, float* obs_data,
                           float* obs_mask, immtsf_stream_t stream) {
    if (!store_ok(s) || !window_ids || B < 0 || npatch <= 0 || Lp < 0 || !obs_tp || !obs_data || !obs_mask) return IMMTSF_EINVAL;
    if (B == 0 || Lp == 0) return IMMTSF_OK;
    float scale = time_max - 0.0f;
    scale = scale + (scale == 0.f ? 1.f : 0.f) * 1e-8f;
    hipLaunchKernelGGL(collate_patches_kernel, dim3(B, npatch), dim3(256), 0, static_cast<hipStream_t>(stream), *s, window_ids,
                       npatch, patch_size, patch_stride, history, Lp, scale, obs_tp, obs_data, obs_mask);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_collate_union(const immtsf_store* s, const int32_t* window_ids, int32_t B, const float* axis, int32_t T, int32_t n_obs,
                         float time_max, float* obs_tp, float* obs_data, float* obs_mask, float* pred_tp, float* pred_data,
                         float* pred_mask, immtsf_stream_t stream) {
    if (!store_ok(s) || !window_ids || B < 0 || T < 0 || n_obs < 0 || n_obs > T || (T > 0 && !axis)) return IMMTSF_EINVAL;
    if (n_obs > 0 && (!obs_tp || !obs_data || !obs_mask)) return IMMTSF_EINVAL;
    if (T - n_obs > 0 && (!pred_tp || !pred_data || !pred_mask)) return IMMTSF_EINVAL;
    if ((long)T * s->C > (1L << 30)) return IMMTSF_EINVAL;      // the kernel indexes one window's slab with int
    if (B == 0 || T == 0) return IMMTSF_OK;
    float scale = time_max - 0.0f;
    scale = scale + (scale == 0.f ? 1.f : 0.f) * 1e-8f;
    const float eps = 1.1920928955078125e-07f * time_max;      // torch.finfo(float32).eps * cap: the cap itself, not the guarded scale
    const long work = (long)(n_obs > T - n_obs ? n_obs : T - n_obs) * s->C;
    long gy = (work + 1023) / 1024;                            // about one 16-byte store per thread
    const long ty = ((long)T + 255) / 256;                     // ... and the axis times are spread no thinner
    if (gy < ty) gy = ty;
    if (gy > 64) gy = 64;
    hipLaunchKernelGGL(collate_union_kernel, dim3(B, (unsigned)gy), dim3(256), 0, static_cast<hipStream_t>(stream), *s, window_ids, axis,
                       T, n_obs, scale, eps, obs_tp, obs_data, obs_mask, pred_tp, pred_data, pred_mask);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_collate_notes(const immtsf_store* s, const int32_t* window_ids, int32_t B, int32_t Nmax, float* tau, float* notes,
                         int32_t* lengths, int32_t* offsets, int32_t* rowmap, immtsf_stream_t stream) {
    if (!s || !s->note_off || !s->note_tau || !s->note_src || !window_ids || B < 0 || Nmax < 0 || !lengths || !offsets)
        return IMMTSF_EINVAL;
    if (notes && (!s->emb || s->d_m <= 0)) return IMMTSF_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(note_index_kernel, dim3(1), dim3(256), 0, st, *s, window_ids, B, lengths, offsets);
    IMMTSF_LAUNCH_CHECK();
    if (B == 0 || Nmax == 0) return IMMTSF_OK;
    const long work = notes ? (long)Nmax * (s->d_m / 4 > 0 ? s->d_m / 4 : s->d_m) : Nmax;
    int gy = (int)((work + 255) / 256);
    if (gy > 64) gy = 64;
    hipLaunchKernelGGL(collate_notes_kernel, dim3(B, gy < 1 ? 1 : gy), dim3(256), 0, st, *s, window_ids, Nmax, offsets, tau, notes,
                       rowmap);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_collate_batch(const immtsf_store* s, const int32_t* window_ids, int32_t B, int32_t Lmax, int32_t Lpmax, int32_t Nmax,
                         float time_max, float* obs_tp, float* obs_data, float* obs_mask, float* pred_tp, float* pred_data,
                         float* pred_mask, float* tau, float* notes, int32_t* lengths, int32_t* offsets, int32_t* rowmap,
                         immtsf_stream_t stream) {
    if (!store_ok(s) || !s->note_off || !s->note_tau || !s->note_src || !window_ids || B <= 0 || Lmax < 0 || Lpmax < 0 || Nmax < 0)
        return IMMTSF_EINVAL;
    if (!lengths || !offsets) return IMMTSF_EINVAL;
    if (Lmax > 0 && (!obs_tp || !obs_data || !obs_mask)) return IMMTSF_EINVAL;
    if (Lpmax > 0 && (!pred_tp || !pred_data || !pred_mask)) return IMMTSF_EINVAL;
    if (Nmax > 0 && (!tau || !rowmap)) return IMMTSF_EINVAL;
    if (notes && (!s->emb || s->d_m <= 0)) return IMMTSF_EINVAL;
    if ((long)(Lmax > Lpmax ? Lmax : Lpmax) * s->C > (1L << 30)) return IMMTSF_EINVAL;      // the kernel indexes one window's slab with int
    float scale = time_max - 0.0f;
    scale = scale + (scale == 0.f ? 1.f : 0.f) * 1e-8f;
    const int series = (Lmax > Lpmax ? Lmax : Lpmax) * s->C;
    const long text = (notes && Nmax > 0) ? (long)Nmax * (s->d_m / 4 > 0 ? s->d_m / 4 : s->d_m) : Nmax;
    long gy = (text + 255) / 256;
    if (gy > 64) gy = 64;                                                  // the embedding rows: as immtsf_collate_notes spreads them
    if (gy < cdiv(series, 256)) gy = cdiv(series, 256);                    // the series: as immtsf_collate_series
    if (gy < 1) gy = 1;
    if (gy > 65535) gy = 65535;                                            // every loop of the kernel strides by the grid
    hipLaunchKernelGGL(collate_batch_kernel, dim3(B, (unsigned)gy), dim3(256), 0, static_cast<hipStream_t>(stream), *s, window_ids, B,
                       Lmax, Lpmax, Nmax, scale, obs_tp, obs_data, obs_mask, pred_tp, pred_data, pred_mask, tau, notes, lengths, offsets,
                       rowmap);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

int immtsf_collate_patch_max(const immtsf_store* s, int32_t W, int32_t npatch, float patch_size, float patch_stride, float history,
                             int32_t* out, immtsf_stream_t stream) {
    if (!store_ok(s) || W < 0 || npatch <= 0 || (W > 0 && !out)) return IMMTSF_EINVAL;
    if (W == 0) return IMMTSF_OK;
    hipLaunchKernelGGL(patch_max_kernel, dim3(cdiv(W, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), *s, W, npatch, patch_size,
                       patch_stride, history, out);
    IMMTSF_LAUNCH_CHECK();
    return IMMTSF_OK;
}

}  // extern "C"
