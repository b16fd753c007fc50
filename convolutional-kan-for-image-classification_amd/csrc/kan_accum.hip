// Gradient accumulation for the fused AdamW step, decided on the device: a window of k micro-steps whose MEAN gradient the ordinary step kernels
// then consume as if autograd had left it there.  The loop this extends is evaluations.py:44-72 -- one zero_grad / backward / step per batch; the
// reference has no accumulation -- and the arithmetic is that of k data-parallel ranks: the mean of the shard gradients, one step per window.
//
//   k_grad_accumulate   the grid of the segment step (k_adamw_seg, kanconv.hip): workgroup b owns elements [start, start + chunk) of segment
//                       chunk_seg[b], reads the gradient through seg_grad and updates the accumulator row (the layout of the optimizer's flat
//                       block: seg_off, 64-element alignment; the padding is never touched).  m, the micro-step within the window, comes from
//                       device memory (a recorded launch decides at replay) or by value:
//                         m == 0          acc = g            a copy: the bits survive, whatever the last window left is never read;
//                                                            a segment without a gradient is zero-filled
//                         0 < m < k - 1   acc = acc + g      one fp32 add per element; a segment without a gradient is left alone
//                         m == k - 1      acc = (acc + g)*s  s = (float)(1.0 / k): the mean; a segment without a gradient in THIS call is
//                                                            acc * s (it may have had one earlier in the window)
//                       k == 1 is the first row alone.  float4 where the gradient is 16-byte aligned, with a < 4-element tail, scalar accesses
//                       for bucket views and odd offsets, as k_adamw_seg and k_grad_sqnorm_chunks.  12 bytes per element, 8 at m == 0.
//                       seen[s] = 1 for every segment that had a gradient in this call (every workgroup of it stores the same value).
//   k_accum_gate        one workgroup behind the accumulate launches of all groups: on the boundary (m + 1 == k) each group's GATED address table
//                       gets the accumulator address of every segment seen in the window and 0 elsewhere, seen is cleared and m = 0; otherwise
//                       the gated tables are all zeros and m = m + 1.  The statistics, guard, advance and step kernels read the gated table
//                       where they read seg_grad, and all of them skip a zero address: off the boundary they touch nothing.
// No atomics, no inline assembly: plain C++.
#include <hip/hip_runtime.h>
#include "kanconv.h"
#include "kan_internal.h"

namespace {

constexpr int AC_NT = 256;                               // threads per workgroup of both kernels (4 waves)

typedef unsigned long long u64;

enum : int { AC_FIRST = 0, AC_ADD = 1, AC_LAST = 2 };

template <int MODE>
__device__ __forceinline__ float acc1(float a, float g, float s) {
    if (MODE == AC_FIRST) return g;
    if (MODE == AC_ADD) return a + g;
    return (a + g) * s;                                         // an add, then a multiply: nothing here can contract into an fma
}

template <int MODE>
__device__ __forceinline__ void acc_chunk(float* __restrict__ a, const float* __restrict__ g, int n, float s) {
    if ((((uintptr_t)g) & 15u) == 0) {                          // accumulator chunks are 16-byte aligned by construction
        for (int i = threadIdx.x; i < (n >> 2); i += AC_NT) {
            const float4 G = ((const float4*)g)[i];
            float4 A = MODE == AC_FIRST ? G : ((const float4*)a)[i];
            A.x = acc1<MODE>(A.x, G.x, s); A.y = acc1<MODE>(A.y, G.y, s); A.z = acc1<MODE>(A.z, G.z, s); A.w = acc1<MODE>(A.w, G.w, s);
            ((float4*)a)[i] = A;
        }
        const int t = (n & ~3) + threadIdx.x;                   // < 4 tail elements
        if (t < n) a[t] = acc1<MODE>(MODE == AC_FIRST ? 0.f : a[t], g[t], s);
    } else {                                                    // bucket views and odd offsets, as in k_adamw_seg
        for (int i = threadIdx.x; i < n; i += AC_NT) a[i] = acc1<MODE>(MODE == AC_FIRST ? 0.f : a[i], g[i], s);
    }
}

__global__ __launch_bounds__(AC_NT) void k_grad_accumulate(float* __restrict__ acc, const u64* __restrict__ seg_grad, const long long* __restrict__ seg_off,
                                                           const int* __restrict__ seg_n, const int* __restrict__ chunk_seg,
                                                           const int* __restrict__ chunk_start, int chunk, const int* __restrict__ micro_dev, int m_val,
                                                           int k, float s, int* __restrict__ seen) {
    const int sg = chunk_seg[blockIdx.x], start = chunk_start[blockIdx.x];
    const int m = micro_dev ? micro_dev[0] : m_val;
    const bool first = m <= 0, last = m >= k - 1;               // first wins: k == 1 is a plain copy
    const float* g = (const float*)seg_grad[sg];
    const int n = min(chunk, seg_n[sg] - start);
    float* a = acc + seg_off[sg] + start;
    if (!g) {                                                   // uniform over the workgroup
        if (first) {
            for (int i = threadIdx.x; i < (n >> 2); i += AC_NT) ((float4*)a)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            const int t = (n & ~3) + threadIdx.x;
            if (t < n) a[t] = 0.f;
        } else if (last) {                                      // the window's sum so far becomes the mean
            for (int i = threadIdx.x; i < (n >> 2); i += AC_NT) {
                float4 A = ((const float4*)a)[i];
                A.x *= s; A.y *= s; A.z *= s; A.w *= s;
                ((float4*)a)[i] = A;
            }
            const int t = (n & ~3) + threadIdx.x;
            if (t < n) a[t] *= s;
        }
        return;
    }
    if (threadIdx.x == 0) seen[sg] = 1;
    g += start;
    if (first) acc_chunk<AC_FIRST>(a, g, n, s);
    else if (last) acc_chunk<AC_LAST>(a, g, n, s);
    else acc_chunk<AC_ADD>(a, g, n, s);
}

// groups[g] = { address of the group's table of accumulator addresses, address of its gated table, address of its seen flags, number of segments }
// guard_counters: NULL, or the counters of the kan_adamw_guard launch that follows in the same step: that launch counts itself as a guarded step,
// so a call that is no step takes the one back in advance.
__global__ __launch_bounds__(AC_NT) void k_accum_gate(const u64* __restrict__ groups, int n_groups, int* micro, int k, long long* guard_counters) {
    const int m = micro[0];
    const bool boundary = m + 1 >= k;
    __syncthreads();                                            // everybody has read the counter before thread 0 moves it
    for (int g = 0; g < n_groups; ++g) {
        const u64* src = (const u64*)groups[4 * g];
        u64* dst = (u64*)groups[4 * g + 1];
        int* seen = (int*)groups[4 * g + 2];
        const int n = (int)groups[4 * g + 3];
        for (int i = threadIdx.x; i < n; i += AC_NT) {
            dst[i] = boundary && seen[i] ? src[i] : 0ull;
            if (boundary) seen[i] = 0;
        }
    }
    if (threadIdx.x != 0) return;
    // one thread of one workgroup, launches ordered by the stream: plain read-modify-write
    micro[0] = boundary ? 0 : m + 1;
    if (!boundary && guard_counters) guard_counters[0] -= 1;
}

int ac_done(const char* what) { return hipGetLastError() == hipSuccess ? 0 : kan_fail_msg("%s: launch failed", what); }

}  // namespace

extern "C" {

int kan_grad_accumulate(float* acc, const unsigned long long* seg_grad, const long long* seg_off, const int* seg_n, const int* chunk_seg,
                        const int* chunk_start, int n_chunks, int chunk_elems, const int* micro_dev, int m, int k, int* seen, void* stream) {
    if (!acc || !seg_grad || !seg_off || !seg_n || !chunk_seg || !chunk_start || !seen) return kan_fail_msg("kan_grad_accumulate: %s", "null pointer");
    if (n_chunks <= 0) return kan_fail_msg("kan_grad_accumulate: %s", "n_chunks must be at least 1");
    if (chunk_elems < 4 || (chunk_elems & 3)) return kan_fail_msg("kan_grad_accumulate: %s", "chunk_elems must be a positive multiple of 4");
    if (k <= 0) return kan_fail_msg("kan_grad_accumulate: %s", "k must be at least 1");
    if (!micro_dev && (m < 0 || m >= k)) return kan_fail_msg("kan_grad_accumulate: %s", "m must lie in [0, k) when micro_dev is NULL");
    if ((uintptr_t)acc & 15u) return kan_fail_msg("kan_grad_accumulate: %s", "acc must be 16-byte aligned");
    if (((uintptr_t)seg_grad | (uintptr_t)seg_off) & 7u) return kan_fail_msg("kan_grad_accumulate: %s", "seg_grad and seg_off must be 8-byte aligned");
    if (((uintptr_t)seg_n | (uintptr_t)chunk_seg | (uintptr_t)chunk_start | (uintptr_t)micro_dev | (uintptr_t)seen) & 3u)
        return kan_fail_msg("kan_grad_accumulate: %s", "seg_n, chunk_seg, chunk_start, micro_dev and seen must be 4-byte aligned");
    hipLaunchKernelGGL(k_grad_accumulate, dim3((unsigned)n_chunks), dim3(AC_NT), 0, static_cast<hipStream_t>(stream), acc, seg_grad, seg_off, seg_n,
                       chunk_seg, chunk_start, chunk_elems, micro_dev, m, k, (float)(1.0 / (double)k), seen);
    return ac_done("kan_grad_accumulate");
}

int kan_accum_gate(const unsigned long long* groups, int n_groups, int* micro, int k, long long* guard_counters, void* stream) {
    if (!groups || !micro) return kan_fail_msg("kan_accum_gate: %s", "null pointer");
    if (n_groups <= 0 || k <= 0) return kan_fail_msg("kan_accum_gate: %s", "n_groups and k must be at least 1");
    if (((uintptr_t)groups | (uintptr_t)guard_counters) & 7u) return kan_fail_msg("kan_accum_gate: %s", "groups and guard_counters must be 8-byte aligned");
    if ((uintptr_t)micro & 3u) return kan_fail_msg("kan_accum_gate: %s", "micro must be 4-byte aligned");
    hipLaunchKernelGGL(k_accum_gate, dim3(1), dim3(AC_NT), 0, static_cast<hipStream_t>(stream), groups, n_groups, micro, k, guard_counters);
    return ac_done("kan_accum_gate");
}

}  // extern "C"
