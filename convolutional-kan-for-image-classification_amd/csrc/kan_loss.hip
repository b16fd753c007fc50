// Cross-entropy loss (mean over the batch) of fp32 logits [B][C] against int64 targets [B], its gradient, and the counters behind the test
// metrics of the reference's evaluation loop -- the criterion of generic_train.py:26 as evaluations.py:61 and :131 call it, and what
// evaluations.py:135-140 collects per batch (torch.max's prediction, the correct count, every target and prediction for scikit-learn's macro
// precision / recall / F1), without a host read per batch: the reference reads loss.item() and (target == predicted).sum().item() every batch
// and copies every prediction to the host.
//
//   forward   k_xent_fwd    one 64-lane wave per row, 4 rows per workgroup, lanes stride over C:  m = max_c l[c] with the LOWEST index among the
//                           maxima (torch.max's tie rule),  lse = m + log(sum_c exp(l[c] - m)),  row loss = lse - l[t] -> workspace;  with a
//                           metrics buffer the per-class counters tp / pred / true (integer atomicAdd: commutes, so the counts are exact)
//             k_xent_mean   one workgroup: the B row losses summed in double in an order that depends on B alone (thread i takes rows i, i + 256,
//                           ...; then a fixed LDS tree) -> loss;  with a metrics buffer, one thread adds the batch mean, the batch, the samples
//                           and the correct count (evaluations.py:132, :150 average batch means, not samples)
//   backward  k_xent_bwd    dlogits[b][c] = g * (exp(l[b][c] - lse[b]) - [c == t_b]) / B,  g read from a device scalar
// A row's lse depends on its own C values only (not on the batch it sits in); no floating-point atomic anywhere: two calls give the same bits.
// A target outside [0, C) is compared against the range before it indexes anything: its row adds 0 to the loss, counts in no counter (the
// bad_target word counts such rows instead) and gets a zero gradient row.
// Plain C++ throughout: no inline assembly, and no atomic other than atomicAdd on integers.
#include <hip/hip_runtime.h>
#include "kanconv.h"
#include "kan_internal.h"

namespace {

constexpr int XE_ROWS = 4, XE_NT = 64 * XE_ROWS;        // rows (= waves) per workgroup of the row kernels, their threads
constexpr int XE_MEAN_NT = 256;                         // threads of the one-workgroup mean
// metrics buffer, in 8-byte words: the header, then tp[C], pred[C], true[C]
enum : int { XM_CORRECT = 0, XM_SAMPLES = 1, XM_BATCHES = 2, XM_BAD_TARGET = 3, XM_LOSS_SUM = 4 /* a double */, XM_HEADER = 8 };
// workspace: B row losses (float), then B row states (int)
enum : int { XS_BAD = -1, XS_WRONG = 0, XS_CORRECT = 1 };

typedef unsigned long long u64;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(XE_NT) void k_xent_fwd(const float* __restrict__ logits, const long long* __restrict__ target, int B, int Cn,
                                                    float* __restrict__ lse, float* __restrict__ row_loss, int* __restrict__ row_state,
                                                    u64* metrics) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * XE_ROWS + (threadIdx.x >> 6);
    if (b >= B) return;                                                  // whole waves leave: no lane of a live wave is missing below
    const float* l = logits + (size_t)b * Cn;
    float m = -INFINITY;
    int arg = 0x7fffffff;                                                // a lane that saw no value loses every comparison
    for (int c = lane; c < Cn; c += 64) {
        const float v = l[c];
        if (v > m || arg == 0x7fffffff) { m = v; arg = c; }             // ascending c: a later equal value does not replace the first
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {                            // (value, index) pairs: greater, or equal with the lower index
        const float om = __shfl_xor(m, off, 64);
        const int oa = __shfl_xor(arg, off, 64);
        if (oa != 0x7fffffff && (arg == 0x7fffffff || om > m || (om == m && oa < arg))) { m = om; arg = oa; }
    }
    float s = 0.f;
    for (int c = lane; c < Cn; c += 64) s += expf(l[c] - m);
    const float row_lse = m + logf(wave_sum(s));
    if (lane != 0) return;
    const long long t = target[b];
    const bool ok = t >= 0 && t < (long long)Cn;                         // before t indexes anything
    lse[b] = row_lse;
    row_loss[b] = ok ? row_lse - l[t] : 0.f;
    row_state[b] = !ok ? XS_BAD : (t == (long long)arg ? XS_CORRECT : XS_WRONG);
    if (metrics && ok) {
        u64* tp = metrics + XM_HEADER;
        if (t == (long long)arg) atomicAdd(tp + t, 1ull);
        atomicAdd(tp + Cn + arg, 1ull);
        atomicAdd(tp + 2 * (size_t)Cn + t, 1ull);
    }
}

__global__ __launch_bounds__(XE_MEAN_NT) void k_xent_mean(const float* __restrict__ row_loss, const int* __restrict__ row_state, int B,
                                                          float* __restrict__ loss, u64* metrics) {
    __shared__ double s_sum[XE_MEAN_NT];
    __shared__ int s_cnt[3][XE_MEAN_NT];                                // valid, correct, bad
    double s = 0.0;
    int valid = 0, correct = 0, bad = 0;
    for (int b = threadIdx.x; b < B; b += XE_MEAN_NT) {
        s += (double)row_loss[b];
        const int st = row_state[b];
        valid += st != XS_BAD; correct += st == XS_CORRECT; bad += st == XS_BAD;
    }
    s_sum[threadIdx.x] = s;
    s_cnt[0][threadIdx.x] = valid; s_cnt[1][threadIdx.x] = correct; s_cnt[2][threadIdx.x] = bad;
    __syncthreads();
    for (int w = XE_MEAN_NT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
            for (int k = 0; k < 3; ++k) s_cnt[k][threadIdx.x] += s_cnt[k][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double mean = s_sum[0] / (double)B;
    *loss = (float)mean;
    if (!metrics) return;
    // one thread of one workgroup, launches ordered by the stream: plain read-modify-write
    double* loss_sum = reinterpret_cast<double*>(metrics + XM_LOSS_SUM);
    *loss_sum += (double)(float)mean;                                    // the reference adds loss.item(), an fp32 value
    metrics[XM_CORRECT] += (u64)s_cnt[1][0];
    metrics[XM_SAMPLES] += (u64)s_cnt[0][0];
    metrics[XM_BATCHES] += 1ull;
    metrics[XM_BAD_TARGET] += (u64)s_cnt[2][0];
}

__global__ __launch_bounds__(XE_NT) void k_xent_bwd(const float* __restrict__ logits, const long long* __restrict__ target,
                                                    const float* __restrict__ lse, const float* __restrict__ grad_loss,
                                                    float* __restrict__ dlogits, int B, int Cn) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * XE_ROWS + (threadIdx.x >> 6);
    if (b >= B) return;
    const long long t = target[b];
    const bool ok = t >= 0 && t < (long long)Cn;
    const float scale = grad_loss[0] / (float)B, row_lse = lse[b];
    const float* l = logits + (size_t)b * Cn;
    float* d = dlogits + (size_t)b * Cn;
    for (int c = lane; c < Cn; c += 64)
        d[c] = ok ? scale * (expf(l[c] - row_lse) - ((long long)c == t ? 1.f : 0.f)) : 0.f;
}

int xe_done(const char* what) { return hipGetLastError() == hipSuccess ? 0 : kan_fail_msg("%s: launch failed", what); }

}  // namespace

extern "C" {

long long kan_xent_workspace_bytes(int B) { return B < 1 ? 0 : (long long)B * (sizeof(float) + sizeof(int)); }

long long kan_xent_metrics_bytes(int Cn) { return Cn < 1 ? 0 : (XM_HEADER + 3ll * Cn) * 8; }

int kan_xent_fwd(const float* logits, const long long* target, int B, int Cn, float* loss, float* lse, void* metrics, void* workspace,
                 void* stream) {
    if (!logits || !target || !loss || !lse || !workspace) return kan_fail_msg("kan_xent_fwd: %s", "null pointer");
    if (B < 1 || Cn < 1) return kan_fail_msg("kan_xent_fwd: %s", "B and C must be at least 1");
    float* row_loss = static_cast<float*>(workspace);
    int* row_state = reinterpret_cast<int*>(row_loss + B);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_xent_fwd, dim3((unsigned)(((long long)B + XE_ROWS - 1) / XE_ROWS)), dim3(XE_NT), 0, st, logits, target, B, Cn, lse,
                       row_loss, row_state, static_cast<u64*>(metrics));
    hipLaunchKernelGGL(k_xent_mean, dim3(1), dim3(XE_MEAN_NT), 0, st, row_loss, row_state, B, loss, static_cast<u64*>(metrics));
    return xe_done("kan_xent_fwd");
}

int kan_xent_bwd(const float* logits, const long long* target, const float* lse, const float* grad_loss, float* dlogits, int B, int Cn,
                 void* stream) {
    if (!logits || !target || !lse || !grad_loss || !dlogits) return kan_fail_msg("kan_xent_bwd: %s", "null pointer");
    if (B < 1 || Cn < 1) return kan_fail_msg("kan_xent_bwd: %s", "B and C must be at least 1");
    hipLaunchKernelGGL(k_xent_bwd, dim3((unsigned)(((long long)B + XE_ROWS - 1) / XE_ROWS)), dim3(XE_NT), 0, static_cast<hipStream_t>(stream),
                       logits, target, lse, grad_loss, dlogits, B, Cn);
    return xe_done("kan_xent_bwd");
}

}  // extern "C"
