// Device-side anomaly mode: what stands in for the reference's unconditional torch.autograd.set_detect_anomaly(True) (train.py:431) and its
// "Prevent exploding gradients" line (evaluations.py:33) in a training loop that the host no longer watches -- both OPT-IN; with neither in use
// nothing here is ever launched.
//
//   k_nonfinite_count   the probe: counts the NaN / +inf / -inf elements of a dense fp32 buffer and adds the count to a three-word int64 record
//                       [elements, first_tick, last_tick].  The shape of k_grad_sqnorm_chunks (kan_clip.hip): 256 threads, float4 loads where
//                       the pointer is 16-byte aligned with a < 4-element tail, scalar loads otherwise; a grid-stride loop, so any n.
//                       An element is non-finite when its exponent bits are all ones -- decided on the bit pattern, no floating comparison.
//                       Each workgroup reduces its count (shuffle tree, then LDS) and, ONLY when it found something, issues three integer
//                       atomics: the add to `elements`, whose return value tells the one workgroup that found the record at zero -- it alone
//                       writes first_tick --, and an exchange on last_tick.  Integers commute: the record is exact and reproducible.
//   k_adamw_guard       the decision of a guarded FusedAdamW step, one workgroup: reads seg_sq (kan_grad_norm_finish's exact double sum of
//                       squares per parameter; finite fp32 squares cannot overflow a double, so seg_sq[s] is non-finite exactly when
//                       gradient s holds a non-finite element -- tested on the double's bits), bumps the counters, and writes per group a
//                       masked copy of the gradient address table: the addresses on a clean step, zeros on a skipped one.  The step kernels
//                       and kan_adamw_advance skip a segment whose address is zero, so a skipped step touches nothing.
// No float atomics, no inline assembly: plain C++.
#include <hip/hip_runtime.h>
#include "kanconv.h"
#include "kan_internal.h"

namespace {

constexpr int GD_NT = 256;                               // threads per workgroup of both kernels (4 waves)
constexpr int GD_MAX_BLOCKS = 2048;                      // grid cap of the probe: 8 workgroups per CU, the loop strides over the rest

typedef unsigned long long u64;

__device__ __forceinline__ int bad32(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ bool bad64(double v) {
    return ((u64)__double_as_longlong(v) & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ __launch_bounds__(GD_NT) void k_nonfinite_count(const float* __restrict__ x, long long n, const long long* __restrict__ tick, u64* record) {
    __shared__ int sh[GD_NT / 64];
    const long long first = (long long)blockIdx.x * GD_NT + threadIdx.x, stride = (long long)gridDim.x * GD_NT;
    int cnt = 0;                                                // per thread: an int holds it for any n below 2^50 at the grid cap
    if ((((uintptr_t)x) & 15u) == 0) {
        const long long n4 = n >> 2;
#pragma unroll 4
        for (long long i = first; i < n4; i += stride) {
            const float4 X = ((const float4*)x)[i];
            cnt += bad32(X.x) + bad32(X.y) + bad32(X.z) + bad32(X.w);
        }
        const long long t = (n & ~3ll) + first;                 // < 4 tail elements: the first threads of workgroup 0
        if (t < n) cnt += bad32(x[t]);
    } else {                                                    // views at odd offsets
#pragma unroll 4
        for (long long i = first; i < n; i += stride) cnt += bad32(x[i]);
    }
    cnt = wave_sum_int(cnt);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int total = sh[0] + sh[1] + sh[2] + sh[3];
    if (total == 0) return;                                     // a clean workgroup writes nothing
    const u64 now = (u64)tick[0];
    if (atomicAdd(record, (u64)total) == 0ull) atomicExch(record + 1, now);      // exactly one workgroup ever sees the record at zero
    atomicExch(record + 2, now);
}

// counters: [0] guarded steps  [1] skipped steps  [2] ordinal of the first skipped step  [3] of the last  [4] 1 if the last step was skipped
// flags[s]: 1 where gradient s was non-finite in the last SKIPPED step (left alone by a clean step)
// groups[g] = { address of the group's seg_grad, address of its masked copy, number of segments }
__global__ __launch_bounds__(GD_NT) void k_adamw_guard(const double* __restrict__ seg_sq, int n_seg, const u64* __restrict__ groups, int n_groups,
                                                      long long* counters, long long* flags) {
    int mine = 0;
    for (int s = threadIdx.x; s < n_seg; s += GD_NT) mine |= bad64(seg_sq[s]) ? 1 : 0;
    const int skip = __syncthreads_or(mine);
    if (skip)
        for (int s = threadIdx.x; s < n_seg; s += GD_NT) flags[s] = bad64(seg_sq[s]) ? 1 : 0;
    for (int g = 0; g < n_groups; ++g) {
        const u64* src = (const u64*)groups[3 * g];
        u64* dst = (u64*)groups[3 * g + 1];
        const int n = (int)groups[3 * g + 2];
        for (int i = threadIdx.x; i < n; i += GD_NT) dst[i] = skip ? 0ull : src[i];
    }
    if (threadIdx.x != 0) return;
    // one thread of one workgroup, launches ordered by the stream: plain read-modify-write
    const long long ordinal = counters[0] + 1;
    counters[0] = ordinal;
    counters[4] = skip ? 1 : 0;
    if (skip) {
        if (counters[1] == 0) counters[2] = ordinal;
        counters[1] += 1;
        counters[3] = ordinal;
    }
}

int gd_done(const char* what) { return hipGetLastError() == hipSuccess ? 0 : kan_fail_msg("%s: launch failed", what); }

}  // namespace

extern "C" {

int kan_nonfinite_count(const float* x, long long n, const long long* tick, long long* record, void* stream) {
    if (!x || !tick || !record) return kan_fail_msg("kan_nonfinite_count: %s", "null pointer");
    if (n < 0) return kan_fail_msg("kan_nonfinite_count: %s", "n must not be negative");
    if (((uintptr_t)tick | (uintptr_t)record) & 7u) return kan_fail_msg("kan_nonfinite_count: %s", "tick and record must be 8-byte aligned");
    if ((uintptr_t)x & 3u) return kan_fail_msg("kan_nonfinite_count: %s", "x must be 4-byte aligned");
    if (n == 0) return 0;
    const long long per = (long long)GD_NT * 4, want = (n + per - 1) / per;
    const unsigned blocks = (unsigned)(want < GD_MAX_BLOCKS ? want : GD_MAX_BLOCKS);
    hipLaunchKernelGGL(k_nonfinite_count, dim3(blocks), dim3(GD_NT), 0, static_cast<hipStream_t>(stream), x, n, tick,
                       reinterpret_cast<u64*>(record));
    return gd_done("kan_nonfinite_count");
}

int kan_adamw_guard(const double* seg_sq, int n_seg, const unsigned long long* groups, int n_groups, long long* counters, long long* flags,
                    void* stream) {
    if (!seg_sq || !groups || !counters || !flags) return kan_fail_msg("kan_adamw_guard: %s", "null pointer");
    if (n_seg <= 0 || n_groups <= 0) return kan_fail_msg("kan_adamw_guard: %s", "n_seg and n_groups must be at least 1");
    if (((uintptr_t)seg_sq | (uintptr_t)groups | (uintptr_t)counters | (uintptr_t)flags) & 7u)
        return kan_fail_msg("kan_adamw_guard: %s", "seg_sq, groups, counters and flags must be 8-byte aligned");
    hipLaunchKernelGGL(k_adamw_guard, dim3(1), dim3(GD_NT), 0, static_cast<hipStream_t>(stream), seg_sq, n_seg, groups, n_groups, counters, flags);
    return gd_done("kan_adamw_guard");
}

}  // extern "C"
