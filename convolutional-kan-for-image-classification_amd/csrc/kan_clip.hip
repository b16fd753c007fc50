// Global-norm gradient clipping for the fused AdamW step: the norm torch.nn.utils.clip_grad_norm_ computes (the reference asks for it at
// evaluations.py:33, `clip_grad_norm_(model.parameters(), max_norm=1.0)`, and for per-parameter gradient norms in its commented-out `GRAD NORM`
// print, evaluations.py:66-71) without a host walk over the parameters, a launch per tensor or a second pass that rescales the gradients: the
// clip coefficient stays in device memory and the segment step (k_adamw_seg / k_adamw_seg_dev in kanconv.hip) multiplies by it on the way.
//
//   k_grad_sqnorm_chunks   the grid of the segment step: workgroup b reads its chunk of the gradient of segment chunk_seg[b] and writes ONE double,
//                          the sum of the squares of that chunk (exactly 0.0 for a segment without a gradient)
//   k_grad_norm_finish     one workgroup: one wave per segment sums that segment's chunk partials -> seg_sq[s]; thread 0 then sums seg_sq in
//                          ascending order -> out[0] = norm, out[1] = min(1, max_norm / (norm + 1e-6))
// Every square is (double)g * (double)g -- exact: 24 x 24 significant bits -- and every sum is a double sum in an order that depends on the
// tables alone (thread, then wave by a fixed shuffle tree, then the four waves in order): no atomics, so two launches give the same bits, and
// the only fp32 roundings are the two final casts.  Double costs nothing here: the chunk kernel reads 4 B per element and is HBM-bound.
// Plain C++ throughout: no inline assembly.
#include <hip/hip_runtime.h>
#include "kanconv.h"
#include "kan_internal.h"

namespace {

constexpr int GN_NT = 256;                               // threads per workgroup of both kernels (4 waves)

__device__ __forceinline__ double sq(float g) { return (double)g * (double)g; }

// lane 0 ends up with the sum over the wave, formed by the same tree every time
__device__ __forceinline__ double wave_sum_down(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ __launch_bounds__(GN_NT) void k_grad_sqnorm_chunks(const unsigned long long* __restrict__ seg_grad, const int* __restrict__ seg_n,
                                                              const int* __restrict__ chunk_seg, const int* __restrict__ chunk_start, int chunk,
                                                              double* __restrict__ partial) {
    __shared__ double sh[GN_NT / 64];
    const int sg = chunk_seg[blockIdx.x], start = chunk_start[blockIdx.x];
    const float* g = (const float*)seg_grad[sg];
    if (!g) {                                                   // uniform over the workgroup: nobody waits at the barrier below
        if (threadIdx.x == 0) partial[blockIdx.x] = 0.0;
        return;
    }
    const int n = min(chunk, seg_n[sg] - start);
    g += start;
    double acc = 0.0;
    if ((((uintptr_t)g) & 15u) == 0) {
        for (int i = threadIdx.x; i < (n >> 2); i += GN_NT) {
            const float4 G = ((const float4*)g)[i];
            acc += sq(G.x); acc += sq(G.y); acc += sq(G.z); acc += sq(G.w);
        }
        const int t = (n & ~3) + threadIdx.x;                   // < 4 tail elements
        if (t < n) acc += sq(g[t]);
    } else {                                                    // bucket views and odd offsets, as in k_adamw_seg
        for (int i = threadIdx.x; i < n; i += GN_NT) acc += sq(g[i]);
    }
    acc = wave_sum_down(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(GN_NT) void k_grad_norm_finish(const double* __restrict__ partial, const int* __restrict__ seg_first_chunk, int n_seg,
                                                            const float* __restrict__ max_norm_dev, double* seg_sq, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    for (int s = threadIdx.x >> 6; s < n_seg; s += GN_NT / 64) {              // whole waves loop: every lane of a wave sees the same s
        double acc = 0.0;
        for (int c = seg_first_chunk[s] + lane, end = seg_first_chunk[s + 1]; c < end; c += 64) acc += partial[c];
        acc = wave_sum_down(acc);
        if (lane == 0) seg_sq[s] = acc;
    }
    __syncthreads();                                                          // seg_sq, written by four waves, is read by thread 0
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int s = 0; s < n_seg; ++s) total += seg_sq[s];
    const double norm = sqrt(total);
    const double coef = (double)max_norm_dev[0] / (norm + 1e-6);              // torch: clip_coef = max_norm / (total_norm + 1e-6)
    out[0] = (float)norm;
    out[1] = (float)(coef < 1.0 || coef != coef ? coef : 1.0);                // torch.clamp(clip_coef, max=1.0): a NaN stays a NaN
}

int gn_done(const char* what) { return hipGetLastError() == hipSuccess ? 0 : kan_fail_msg("%s: launch failed", what); }

}  // namespace

extern "C" {

int kan_grad_sqnorm_chunks(const unsigned long long* seg_grad, const int* seg_n, const int* chunk_seg, const int* chunk_start, int n_chunks,
                           int chunk_elems, double* partial, void* stream) {
    if (!seg_grad || !seg_n || !chunk_seg || !chunk_start || !partial) return kan_fail_msg("kan_grad_sqnorm_chunks: %s", "null pointer");
    if (n_chunks <= 0) return kan_fail_msg("kan_grad_sqnorm_chunks: %s", "n_chunks must be at least 1");
    if (chunk_elems < 4 || (chunk_elems & 3)) return kan_fail_msg("kan_grad_sqnorm_chunks: %s", "chunk_elems must be a positive multiple of 4");
    if ((uintptr_t)partial & 7u) return kan_fail_msg("kan_grad_sqnorm_chunks: %s", "partial must be 8-byte aligned");
    hipLaunchKernelGGL(k_grad_sqnorm_chunks, dim3((unsigned)n_chunks), dim3(GN_NT), 0, static_cast<hipStream_t>(stream), seg_grad, seg_n, chunk_seg,
                       chunk_start, chunk_elems, partial);
    return gn_done("kan_grad_sqnorm_chunks");
}

int kan_grad_norm_finish(const double* partial, const int* seg_first_chunk, int n_seg, const float* max_norm_dev, double* seg_sq, float* out,
                         void* stream) {
    if (!partial || !seg_first_chunk || !max_norm_dev || !seg_sq || !out) return kan_fail_msg("kan_grad_norm_finish: %s", "null pointer");
    if (n_seg <= 0) return kan_fail_msg("kan_grad_norm_finish: %s", "n_seg must be at least 1");
    if (((uintptr_t)partial | (uintptr_t)seg_sq) & 7u) return kan_fail_msg("kan_grad_norm_finish: %s", "partial and seg_sq must be 8-byte aligned");
    if (((uintptr_t)seg_first_chunk | (uintptr_t)max_norm_dev | (uintptr_t)out) & 3u)
        return kan_fail_msg("kan_grad_norm_finish: %s", "seg_first_chunk, max_norm_dev and out must be 4-byte aligned");
    hipLaunchKernelGGL(k_grad_norm_finish, dim3(1), dim3(GN_NT), 0, static_cast<hipStream_t>(stream), partial, seg_first_chunk, n_seg, max_norm_dev,
                       seg_sq, out);
    return gn_done("kan_grad_norm_finish");
}

}  // extern "C"
