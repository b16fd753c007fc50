// BatchNorm (batch statistics) [+ PReLU] [+ MaxPool2d(2, 2)] behind the conv stage: the tail of a layer built with norm_layer=BatchNorm2d
// (kan_layers.py:241-243; train.py:67-68 makes it the default of the reference's training script).  HBM-bound fp32 data, statistics in
// double, as the InstanceNorm kernels of kanconv.hip -- whose rules these kernels keep: the slab sum with four loads in flight, the pool
// argmax byte 2*dh + dw (first maximum in scan order, NaN wins), the PReLU negative side !(n > 0).
//
// A statistic spans every image of a channel, so each direction is three launches around a caller-owned workspace of BN_WS doubles per
// (b, channel) plane, value-major (ws[k * planes + plane]):
//   forward   k_bn_fwd_partials  per plane: slab sum -> z_out, count / mean / centred M2
//             k_bn_fwd_finalise  per channel (one wave): the B partials combined in index order (Chan), mean / rstd, running statistics
//             k_bn_fwd_apply     per plane: normalise, affine, PReLU, then y or the pooled y + argmax bytes
//   backward  k_bn_bwd_partials  per plane: s1, s2 (ATen's `sum` and `dotp`), dbeta, dgamma, dslope sums
//             k_bn_bwd_finalise  per channel (one wave): the B partials summed in index order; the last workgroup to finish sums the slope
//                                gradients over the channels of each slope
//             k_bn_bwd_apply     per plane: dz
// Every sum has a fixed order and no value is accumulated with atomics (the one atomic is an integer ticket): two runs give the same
// bits, parameter gradients included.
// G lanes (one wave or a part of it) work on a plane, 256 / G planes per workgroup; G follows from the plane size alone (bn_lanes).
#include <hip/hip_runtime.h>
#include "kanconv.h"
#include "kan_common.h"
#include "kan_internal.h"

namespace {

constexpr int BN_WS = 5;                                  // doubles per plane: what the backward keeps (the forward uses three)
constexpr int BN_FIN_CH = 4, BN_FIN_NT = 64 * BN_FIN_CH;  // finalise: channels (= waves) per workgroup, its threads
constexpr int BN_FIN_IMGS = 256;                          // ... and the images whose partials a wave stages in LDS at once

// Everything the plane kernels share.  W == 0: no pool.
struct BnShape { int planes, Cn, HW, W; long long bstride; FastDiv divCn, divW2, divW; };

__device__ __forceinline__ float bn_activate(float n, bool has_p, float a) { return (has_p && !(n > 0.f)) ? a * n : n; }

template <int G>
__global__ __launch_bounds__(256) void k_bn_fwd_partials(const float* z, int n_slabs, long long slab_elems, float* z_out,     // z_out may alias z (slab 0)
                                                         double* __restrict__ ws, BnShape sh, int stats) {
    const int sub = threadIdx.x % G;
    const int plane = blockIdx.x * (256 / G) + threadIdx.x / G;
    const bool act = plane < sh.planes;
    const int b = act ? fastdiv(plane, sh.divCn) : 0, c = act ? plane - b * sh.Cn : 0;
    const size_t base = (size_t)b * sh.bstride + (size_t)c * sh.HW;
    const bool need_sum = (n_slabs > 1) || (z_out != z);
    double s = 0.0;
    if (act) for (int i = sub; i < sh.HW; i += G) {
        const float* zp = z + base + i;                   // four independent partial sums keep four loads in flight; fixed order
        float v0 = zp[0], v1 = 0.f, v2 = 0.f, v3 = 0.f;
        int sl = 1;
        for (; sl + 4 <= n_slabs; sl += 4) {
            v0 += zp[(size_t)sl * slab_elems]; v1 += zp[(size_t)(sl + 1) * slab_elems];
            v2 += zp[(size_t)(sl + 2) * slab_elems]; v3 += zp[(size_t)(sl + 3) * slab_elems];
        }
        for (; sl < n_slabs; ++sl) v0 += zp[(size_t)sl * slab_elems];
        const float v = (v0 + v1) + (v2 + v3);
        if (need_sum) z_out[base + i] = v;
        s += (double)v;
    }
    if (!stats) return;                                   // statistics come from the running buffers: only the slab sum was wanted
    const double mu = group_sum<G>(s) / (double)sh.HW;
    double q = 0.0;
    if (act) for (int i = sub; i < sh.HW; i += G) { const double d = (double)z_out[base + i] - mu; q += d * d; }     // (a lane reads back what it wrote)
    q = group_sum<G>(q);
    if (act && sub == 0) {
        ws[plane] = (double)sh.HW; ws[(size_t)sh.planes + plane] = mu; ws[2 * (size_t)sh.planes + plane] = q;
    }
}

// Both finalise kernels give a channel to one wave, BN_FIN_CH channels to a workgroup.  The wave's lanes load the partials of BN_FIN_IMGS images at
// once into LDS (that is where the time goes: the values sit B * Cn apart); the combination itself stays strictly in index order, by single lanes
// reading LDS.  Waves without a channel skip the work but keep the barriers.
//
// Forward, Chan et al.: (nA, mA, M2A) + (nB, mB, M2B) -> n = nA + nB, d = mB - mA, m = mA + d nB / n, M2 = M2A + M2B + d^2 nA nB / n.  The counts
// do not depend on the data, so lane 0 first runs their prefix sum, all lanes then take the divisions f = nB / n, g = nA f in parallel, and lane 0
// folds m += d f, M2 += M2B + d^2 g -- the same expressions a plain loop over the images would evaluate, in the same order.
__global__ __launch_bounds__(BN_FIN_NT) void k_bn_fwd_finalise(const double* __restrict__ ws, float* __restrict__ mean_o, float* __restrict__ rstd_o,
                                                               float* __restrict__ run_mean, float* __restrict__ run_var, int B, int Cn,
                                                               float eps, double momentum, int stats, int update) {
    __shared__ double s_f[BN_FIN_CH][BN_FIN_IMGS], s_g[BN_FIN_CH][BN_FIN_IMGS], s_m[BN_FIN_CH][BN_FIN_IMGS], s_q[BN_FIN_CH][BN_FIN_IMGS];
    const int w = threadIdx.x / 64, lane = threadIdx.x % 64, c = blockIdx.x * BN_FIN_CH + w;
    const bool act = c < Cn;
    if (!stats) {                                         // eval mode on running statistics
        if (act && lane == 0) { mean_o[c] = run_mean[c]; rstd_o[c] = (float)(1.0 / sqrt((double)run_var[c] + (double)eps)); }
        return;
    }
    const size_t planes = (size_t)B * Cn;
    double n = 0.0, m = 0.0, M2 = 0.0;                    // lane 0's running statistics
    for (int b0 = 0; b0 < B; b0 += BN_FIN_IMGS) {
        const int nb = min(BN_FIN_IMGS, B - b0);
        __syncthreads();                                  // (the previous chunk has been folded)
        if (act) for (int i = lane; i < nb; i += 64) {
            const size_t p = (size_t)(b0 + i) * Cn + c;
            s_f[w][i] = ws[p]; s_m[w][i] = ws[planes + p]; s_q[w][i] = ws[2 * planes + p];
        }
        __syncthreads();
        if (act && lane == 0) {                           // s_g: the count before image i
#pragma unroll 8
            for (int i = 0; i < nb; ++i) { const double nB = s_f[w][i]; s_g[w][i] = n; n += nB; }
        }
        __syncthreads();
        if (act) for (int i = lane; i < nb; i += 64) {
            const double nB = s_f[w][i], nA = s_g[w][i], f = nB / (nA + nB);
            s_f[w][i] = f; s_g[w][i] = nA * f;
        }
        __syncthreads();
        if (act && lane == 0) {
#pragma unroll 8
            for (int i = 0; i < nb; ++i) {
                const double d = s_m[w][i] - m;
                m += d * s_f[w][i];
                M2 += s_q[w][i] + d * d * s_g[w][i];
            }
        }
    }
    if (!act || lane != 0) return;
    mean_o[c] = (float)m;
    rstd_o[c] = (float)(1.0 / sqrt(M2 / n + (double)eps));
    if (update) {                                         // ATen: the running variance takes the unbiased estimate
        run_mean[c] = (float)((1.0 - momentum) * (double)run_mean[c] + momentum * m);
        run_var[c] = (float)((1.0 - momentum) * (double)run_var[c] + momentum * (M2 / (n - 1.0)));
    }
}

template <int G, bool POOL>
__global__ __launch_bounds__(256) void k_bn_fwd_apply(const float* __restrict__ z, const float* __restrict__ mean_i, const float* __restrict__ rstd_i,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ prelu_a, float* __restrict__ y, unsigned char* __restrict__ pidx,
                                                      BnShape sh, int prelu_span) {
    const int sub = threadIdx.x % G;
    const int plane = blockIdx.x * (256 / G) + threadIdx.x / G;
    if (plane >= sh.planes) return;
    const int b = fastdiv(plane, sh.divCn), c = plane - b * sh.Cn;
    const size_t base = (size_t)b * sh.bstride + (size_t)c * sh.HW;
    const float mu = mean_i[c], rs = rstd_i[c];
    const float ga = gamma ? gamma[c] : 1.f, be = beta ? beta[c] : 0.f;
    const bool has_p = prelu_a != nullptr;
    const float a = has_p ? prelu_a[prelu_span > 0 ? c / prelu_span : 0] : 1.f;
    if constexpr (POOL) {
        // dense pooled [B][Cn][H/2][W/2] y and argmax bytes; the full-size activation is never written
        const int W = sh.W, W2 = W >> 1, Q = sh.HW >> 2;
        const size_t pbase = (size_t)plane * Q;
        for (int q = sub; q < Q; q += G) {
            const int h2 = fastdiv(q, sh.divW2), w2 = q - h2 * W2, i0 = 2 * h2 * W + 2 * w2;
            float best = 0.f; int arg = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v = bn_activate((z[base + i0 + (k >> 1) * W + (k & 1)] - mu) * rs * ga + be, has_p, a);
                if (k == 0 || v > best || v != v) { best = v; arg = k; }
            }
            y[pbase + q] = best; pidx[pbase + q] = (unsigned char)arg;
        }
    } else {
        for (int i = sub; i < sh.HW; i += G) y[base + i] = bn_activate((z[base + i] - mu) * rs * ga + be, has_p, a);
    }
}

// What the two backward plane kernels share: the plane's constants and k_in_prelu_bwd's `visit` at channel scope.
struct BnBwdPlane {
    float mu, rs, ga, be, a; bool has_p;
    // zc = z - mean, dn = dL/d(affine output), nh = normalised value, dnh = dL/d nh; neg: the PReLU negative side took the element
    __device__ __forceinline__ void visit(float zv, float g, float& zc, float& nh, float& n, float& dn, float& dnh, bool& neg) const {
        zc = zv - mu; nh = zc * rs; n = nh * ga + be;
        neg = has_p && !(n > 0.f);
        dn = neg ? a * g : g;
        dnh = dn * ga;
    }
};

template <bool POOL>
__device__ __forceinline__ float bn_upstream(const float* __restrict__ dy, const unsigned char* __restrict__ pidx, const BnShape& sh, int plane,
                                             size_t base, int i) {
    if constexpr (!POOL) return dy[base + i];
    else {                                                // dy is the dense pooled gradient: only the element the forward marked receives it
        const int h = fastdiv(i, sh.divW), w = i - h * sh.W;
        const size_t pq = (size_t)plane * (sh.HW >> 2) + (size_t)((h >> 1) * (sh.W >> 1) + (w >> 1));
        return pidx[pq] == (unsigned char)((h & 1) * 2 + (w & 1)) ? dy[pq] : 0.f;
    }
}

__device__ __forceinline__ BnBwdPlane bn_bwd_plane(const float* mean_i, const float* rstd_i, const float* gamma, const float* beta,
                                                   const float* prelu_a, int prelu_span, int c) {
    BnBwdPlane p;
    p.mu = mean_i[c]; p.rs = rstd_i[c];
    p.ga = gamma ? gamma[c] : 1.f; p.be = beta ? beta[c] : 0.f;
    p.has_p = prelu_a != nullptr;
    p.a = p.has_p ? prelu_a[prelu_span > 0 ? c / prelu_span : 0] : 1.f;
    return p;
}

template <int G, bool POOL>
__global__ __launch_bounds__(256) void k_bn_bwd_partials(const float* __restrict__ dy, const unsigned char* __restrict__ pidx,
                                                         const float* __restrict__ z, const float* __restrict__ mean_i,
                                                         const float* __restrict__ rstd_i, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ prelu_a,
                                                         double* __restrict__ ws, BnShape sh, int prelu_span) {
    const int sub = threadIdx.x % G;
    const int plane = blockIdx.x * (256 / G) + threadIdx.x / G;
    const bool act = plane < sh.planes;
    const int b = act ? fastdiv(plane, sh.divCn) : 0, c = act ? plane - b * sh.Cn : 0;
    const size_t base = (size_t)b * sh.bstride + (size_t)c * sh.HW;
    const BnBwdPlane p = bn_bwd_plane(mean_i, rstd_i, gamma, beta, prelu_a, prelu_span, c);
    if (blockIdx.x == 0 && threadIdx.x == 0) *(unsigned*)(ws + BN_WS * (size_t)sh.planes) = 0u;      // k_bn_bwd_finalise's ticket counter
    double s1 = 0.0, s2 = 0.0, sb = 0.0, sg = 0.0, sa = 0.0;
    if (act) for (int i = sub; i < sh.HW; i += G) {
        float zc, nh, n, dn, dnh; bool neg;
        const float g = bn_upstream<POOL>(dy, pidx, sh, plane, base, i);
        p.visit(z[base + i], g, zc, nh, n, dn, dnh, neg);
        if (neg) sa += (double)n * (double)g;
        sb += (double)dn; sg += (double)dn * (double)nh;
        s1 += (double)dnh; s2 += (double)dnh * (double)zc;
    }
    s1 = group_sum<G>(s1); s2 = group_sum<G>(s2); sb = group_sum<G>(sb); sg = group_sum<G>(sg); sa = group_sum<G>(sa);
    if (act && sub == 0) {
        const size_t P = (size_t)sh.planes;
        ws[plane] = s1; ws[P + plane] = s2; ws[2 * P + plane] = sb; ws[3 * P + plane] = sg; ws[4 * P + plane] = sa;
    }
}

// Backward: lane k < BN_WS of a channel's wave sums value k of the staged partials in index order.  dgamma / dbeta are written from the sums, and the
// channel's s1, s2 go to the workspace slots of image 0, which is what k_bn_bwd_apply reads.  With a slope gradient the channel's slope sum goes
// there too, and the workgroup that finishes last (a ticket counter behind the workspace, zeroed by k_bn_bwd_partials) adds them up per slope: the
// lanes of its first wave stride over the slope's channels, then the butterfly of group_sum -- an order that does not depend on which came last.
__global__ __launch_bounds__(BN_FIN_NT) void k_bn_bwd_finalise(double* ws, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                               float* __restrict__ dprelu, int B, int Cn, int prelu_span) {
    __shared__ double s_v[BN_FIN_CH][BN_WS][BN_FIN_IMGS];
    __shared__ bool last;
    const int w = threadIdx.x / 64, lane = threadIdx.x % 64, c = blockIdx.x * BN_FIN_CH + w;
    const bool act = c < Cn;
    const size_t P = (size_t)B * Cn;
    double t = 0.0;                                       // lane k < BN_WS: the running sum of value k
    for (int b0 = 0; b0 < B; b0 += BN_FIN_IMGS) {
        const int nb = min(BN_FIN_IMGS, B - b0);
        __syncthreads();
        if (act) for (int i = lane; i < nb; i += 64) {
#pragma unroll
            for (int k = 0; k < BN_WS; ++k) s_v[w][k][i] = ws[k * P + (size_t)(b0 + i) * Cn + c];
        }
        __syncthreads();
        if (act && lane < BN_WS) {
#pragma unroll 8
            for (int i = 0; i < nb; ++i) t += s_v[w][lane][i];
        }
    }
    if (act && lane < BN_WS) {
        if (lane == 2 && dbeta) dbeta[c] = (float)t;
        if (lane == 3 && dgamma) dgamma[c] = (float)t;
        if (lane != 2 && lane != 3) ws[lane * P + c] = t;
    }
    if (!dprelu) return;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd((unsigned*)(ws + BN_WS * P), 1u) == gridDim.x - 1;
    __syncthreads();
    if (!last || w != 0) return;
    __threadfence();
    const int span = prelu_span > 0 ? prelu_span : Cn;
    int gs = 1;                                           // lanes per slope
    while (gs < 64 && gs < span) gs *= 2;
    const int sub = lane % gs, per_pass = 64 / gs, n_slopes = Cn / span;
    for (int s0 = 0; s0 < n_slopes; s0 += per_pass) {
        const int sl = s0 + lane / gs;
        double a = 0.0;
        if (sl < n_slopes) for (int i = sub; i < span; i += gs) a += ws[4 * P + (size_t)sl * span + i];
        for (int off = gs / 2; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
        if (sl < n_slopes && sub == 0) dprelu[sl] = (float)a;
    }
}

template <int G, bool POOL>
__global__ __launch_bounds__(256) void k_bn_bwd_apply(const float* __restrict__ dy, const unsigned char* __restrict__ pidx,
                                                      const float* __restrict__ z, const float* __restrict__ mean_i,
                                                      const float* __restrict__ rstd_i, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ prelu_a,
                                                      const double* __restrict__ ws, float* __restrict__ dz, BnShape sh, int prelu_span,
                                                      double inv_n, int stats) {
    const int sub = threadIdx.x % G;
    const int plane = blockIdx.x * (256 / G) + threadIdx.x / G;
    if (plane >= sh.planes) return;
    const int b = fastdiv(plane, sh.divCn), c = plane - b * sh.Cn;
    const size_t base = (size_t)b * sh.bstride + (size_t)c * sh.HW;
    const BnBwdPlane p = bn_bwd_plane(mean_i, rstd_i, gamma, beta, prelu_a, prelu_span, c);
    const double rs_d = (double)p.rs;
    // grad_mean and k of ATen's batch_norm_backward_cpu; with the running statistics of eval mode neither depends on z: dz = dnh rstd
    const double gm = stats ? ws[c] * inv_n : 0.0, kk = stats ? ws[(size_t)sh.planes + c] * rs_d * rs_d * inv_n : 0.0;
    for (int i = sub; i < sh.HW; i += G) {
        float zc, nh, n, dn, dnh; bool neg;
        p.visit(z[base + i], bn_upstream<POOL>(dy, pidx, sh, plane, base, i), zc, nh, n, dn, dnh, neg);
        dz[base + i] = (float)((((double)dnh - gm) - (double)zc * kk) * rs_d);
    }
}

// Lanes per plane: the power of two in [4, 64] that leaves a lane about four elements (one 2x2 window), from the plane size alone.
int bn_lanes(int HW) {
    int g = 4;
    while (g < 64 && g * 4 < HW) g *= 2;
    return g;
}

const char* bn_reject(int B, int Cn, int H, int W, long long bstride, const unsigned char* pool_idx) {
    if (B < 1 || Cn < 1 || H < 1 || W < 1) return "empty tensor";
    if ((long long)B * Cn >= (1ll << 31) || (long long)H * W >= (1ll << 29)) return "more than 2^31 planes or 2^29 pixels per plane";
    if (bstride < (long long)Cn * H * W) return "batch stride below Cn * H * W";
    if (pool_idx && ((H | W) & 1)) return "fused 2x2 max-pool needs even H and W";
    return nullptr;
}

BnShape bn_shape(int B, int Cn, int H, int W, long long bstride, bool pool) {
    BnShape sh;
    sh.planes = B * Cn; sh.Cn = Cn; sh.HW = H * W; sh.W = pool ? W : 0; sh.bstride = bstride;
    sh.divCn = make_fastdiv(Cn); sh.divW = make_fastdiv(W); sh.divW2 = make_fastdiv(W > 1 ? W / 2 : 1);
    return sh;
}

int bn_done(const char* what) { return hipGetLastError() == hipSuccess ? 0 : kan_fail_msg("%s: launch failed", what); }

}  // namespace

extern "C" {

long long kan_batchnorm_workspace_bytes(int B, int Cn) {
    return B < 1 || Cn < 1 ? 0 : ((long long)B * Cn * BN_WS + 1) * (long long)sizeof(double);      // (+ the backward's ticket counter)
}

int kan_batchnorm_prelu_fwd(const float* z, int n_slabs, long long slab_elems, float* z_out, const float* gamma, const float* beta,
                            const float* prelu_a, float* y, unsigned char* pool_idx, float* mean, float* rstd, float* running_mean,
                            float* running_var, void* workspace, int B, int Cn, int H, int W, long long bstride, float eps, double momentum,
                            int prelu_span, int training, void* stream) {
    if (!z || !z_out || !y || !mean || !rstd || !workspace || n_slabs < 1) return kan_fail_msg("kan_batchnorm_prelu_fwd: %s", "null pointer or no slab");
    if (const char* why = bn_reject(B, Cn, H, W, bstride, pool_idx)) return kan_fail_msg("kan_batchnorm_prelu_fwd: %s", why);
    if (!running_mean != !running_var) return kan_fail_msg("kan_batchnorm_prelu_fwd: %s", "running_mean and running_var come together");
    if (prelu_span < 0 || (prelu_span > 0 && Cn % prelu_span)) return kan_fail_msg("kan_batchnorm_prelu_fwd: %s", "prelu_span does not divide Cn");
    const int stats = training || !running_mean;          // torch's rule: batch statistics unless eval mode has running ones
    if (stats && training && (long long)B * H * W < 2) return kan_fail_msg("kan_batchnorm_prelu_fwd: %s", "training needs more than one value per channel");
    hipStream_t st = (hipStream_t)stream;
    const BnShape sh = bn_shape(B, Cn, H, W, bstride, pool_idx != nullptr);
    double* ws = (double*)workspace;
    pick<4, 8, 16, 32, 64>(bn_lanes(sh.HW), [&](auto g) {
        constexpr int G = decltype(g)::value;
        const dim3 grid((unsigned)((sh.planes + 256 / G - 1) / (256 / G)));
        if (stats || n_slabs > 1 || z_out != z)
            hipLaunchKernelGGL((k_bn_fwd_partials<G>), grid, dim3(256), 0, st, z, n_slabs, slab_elems, z_out, ws, sh, stats);
        hipLaunchKernelGGL(k_bn_fwd_finalise, dim3((unsigned)((Cn + BN_FIN_CH - 1) / BN_FIN_CH)), dim3(BN_FIN_NT), 0, st, (const double*)ws, mean, rstd,
                           running_mean, running_var, B, Cn, eps, momentum, stats, (int)(training && running_mean));
        if (pool_idx) hipLaunchKernelGGL((k_bn_fwd_apply<G, true>), grid, dim3(256), 0, st, (const float*)z_out, (const float*)mean, (const float*)rstd, gamma, beta, prelu_a, y, pool_idx, sh, prelu_span);
        else hipLaunchKernelGGL((k_bn_fwd_apply<G, false>), grid, dim3(256), 0, st, (const float*)z_out, (const float*)mean, (const float*)rstd, gamma, beta, prelu_a, y, pool_idx, sh, prelu_span);
    });
    return bn_done("kan_batchnorm_prelu_fwd");
}

int kan_batchnorm_prelu_bwd(const float* dy, const unsigned char* pool_idx, const float* z, const float* mean, const float* rstd,
                            const float* gamma, const float* beta, const float* prelu_a, float* dz, float* dgamma, float* dbeta, float* dprelu,
                            void* workspace, int B, int Cn, int H, int W, long long bstride, int prelu_span, int training, void* stream) {
    if (!dy || !z || !mean || !rstd || !dz || !workspace) return kan_fail_msg("kan_batchnorm_prelu_bwd: %s", "null pointer");
    if (const char* why = bn_reject(B, Cn, H, W, bstride, pool_idx)) return kan_fail_msg("kan_batchnorm_prelu_bwd: %s", why);
    if (prelu_span < 0 || (prelu_span > 0 && Cn % prelu_span)) return kan_fail_msg("kan_batchnorm_prelu_bwd: %s", "prelu_span does not divide Cn");
    if (dprelu && !prelu_a) return kan_fail_msg("kan_batchnorm_prelu_bwd: %s", "a slope gradient without a slope");
    hipStream_t st = (hipStream_t)stream;
    const BnShape sh = bn_shape(B, Cn, H, W, bstride, pool_idx != nullptr);
    double* ws = (double*)workspace;
    const double inv_n = 1.0 / ((double)B * (double)sh.HW);
    pick<4, 8, 16, 32, 64>(bn_lanes(sh.HW), [&](auto g) {
        constexpr int G = decltype(g)::value;
        const dim3 grid((unsigned)((sh.planes + 256 / G - 1) / (256 / G)));
        auto run = [&](auto pooled) {
            constexpr bool POOL = decltype(pooled)::value != 0;
            hipLaunchKernelGGL((k_bn_bwd_partials<G, POOL>), grid, dim3(256), 0, st, dy, pool_idx, z, mean, rstd, gamma, beta, prelu_a, ws, sh, prelu_span);
            hipLaunchKernelGGL(k_bn_bwd_finalise, dim3((unsigned)((Cn + BN_FIN_CH - 1) / BN_FIN_CH)), dim3(BN_FIN_NT), 0, st, ws, dgamma, dbeta, dprelu, B, Cn,
                               prelu_span);
            hipLaunchKernelGGL((k_bn_bwd_apply<G, POOL>), grid, dim3(256), 0, st, dy, pool_idx, z, mean, rstd, gamma, beta, prelu_a, (const double*)ws, dz, sh,
                               prelu_span, inv_n, training);
        };
        if (pool_idx) run(IC<1>{}); else run(IC<0>{});
    });
    return bn_done("kan_batchnorm_prelu_bwd");
}

}  // extern "C"
