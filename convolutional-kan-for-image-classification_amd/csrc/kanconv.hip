// libkanconv: conv-KAN forward / backward for MI355X (gfx950, CDNA4).  C ABI in include/kanconv.h.
//
// One implicit GEMM per direction, all on the exact-fp32 matrix pipe (v_mfma_f32_32x32x2_f32):
//
//   forward      z [o][pixel]   = sum_k  Wp[k][o]        * E[k][pixel]      k = (c, tap, plane)
//   bwd-data     G [(c,p)][pix] = sum_kd Wp[(c,tap,p)][o] * dz[o][pix(+)tap] kd = (tap, o)
//                dx[c][pix]     = sum_p  plane_p'(x) * G[(c,p)][pix]        (LDS epilogue)
//   bwd-weight   dWp[k][o]      = sum_pix E[k][pixel]    * dz[o][pixel]
//
// E is never materialised in HBM: workgroups gather x, expand it to its P planes in registers
// (kan_device.h) and write the expanded tile straight into LDS in GEMM order; out-of-image taps
// write zeros (the reference zero-pads the EXPANDED tensor, kan_layers.py:239).
//
// Accumulator orientation: MFMA C/D puts the column index on the lane, so the dimension that is
// contiguous in HBM (pixels for z / dx, o for dWp) is always the column => 128-B coalesced stores.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdint>
#include <mutex>
#include <type_traits>
#include <vector>
#include "kanconv.h"
#include "kan_device.h"

#include "kan_common.h"
#include "kan_internal.h"

namespace {


thread_local char g_err[512] = "";
int fail(const char* fmt, const char* a = "") {
    snprintf(g_err, sizeof(g_err), fmt, a);
    return -1;
}
}  // namespace
int kan_fail_msg(const char* fmt, const char* a) { return fail(fmt, a); }      // for the other translation units (kan_internal.h)

int kan_raise_lds_limit(const void* kernel, int bytes) {
    struct Raised { const void* kernel; int device, bytes; };
    static std::mutex mu;
    static std::vector<Raised> raised;                       // (kernel, device) pairs whose limit is up: a handful per process
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    std::lock_guard<std::mutex> lock(mu);
    for (const Raised& r : raised)
        if (r.kernel == kernel && r.device == dev && r.bytes >= bytes) return 0;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return -1;
    raised.push_back(Raised{kernel, dev, bytes});
    return 0;
}
namespace {

// ============================================================================ pack / unpack
// Packed forward layout: the GEMM depth axis is cut into chunks of IPC "items" (item = tap*C + c, TAP-MAJOR so that a
// whole LDS step belongs to one or two taps and can be skipped when the tap is structurally zero), each item owning
// P consecutive rows (its planes); a chunk is KC = even(IPC*P) rows, so that one LDS step of the forward kernel is
// exactly IPC whole items:   k(item, p) = (item / IPC) * KC + (item % IPC) * P + p.
// The weight-gradient kernel uses the same formula with IPC = 1, KC = P (flat, no padding).
// src_kind 0: base weights [O][C][T] -> plane 0;   src_kind 1: basis weights [O][C*nb][T] -> plane hb + q.
// A 32x32 tile goes through LDS so that both the read (along the source's contiguous (channel,tap) axis) and the
// write (along o) coalesce.
// divT / divNb / divIPC / divP: magic numbers for the per-element index divisions below.  With plain `/` the three layout
// kernels spent ~100 VALU instructions per element on integer division and were ALU-bound, not HBM-bound (0.81 ms of a
// 17.4 ms KAN-VGG11 step for 1 GB of traffic).
struct PackGeo { int O, C, T, P, hb, nb, IPC, KC, Opad, pair, cmajor; FastDiv divT, divNb, divIPC, divP;
                 int band; short tap_step[KAN_BAND_MAX_TAPS], tap_nt[KAN_BAND_MAX_TAPS]; };        // band order (kan_internal.h): IPC = channels per group

// Row of (tap, channel c, plane p) in the forward layout.  pair == 0: tap-major items as described above.  pair == 1 (the
// halo forward kernel, P = 9, C even): a step of KC = 18 rows is one tap of a channel PAIR, row 2p + (c & 1), steps
// ordered (c / 2, tap) -- so that the two k-rows of an MFMA k-pair are the same plane of two channels, a fixed LDS
// distance apart in the halo tile.
__device__ __forceinline__ int wp_row(const PackGeo& q, int tap, int c, int p) {
    if (q.band) {                                     // band kernels: step (phase, channel group, tap of the phase), row = (c % IPC) * P + p
        const int grp = fastdiv(c, q.divIPC);
        return (q.tap_step[tap] + grp * q.tap_nt[tap]) * q.KC + (c - grp * q.IPC) * q.P + p;
    }
    if (q.pair) return ((c >> 1) * q.T + tap) * q.KC + 2 * p + (c & 1);
    if (q.cmajor) return (c * q.T + tap) * q.P + p;   // flat channel-major order of the halo weight-gradient kernel
    const int item = tap * q.C + c;                   // tap-major: all channels of a tap are contiguous in the depth axis
    const int chunk = fastdiv(item, q.divIPC);
    return chunk * q.KC + (item - chunk * q.IPC) * q.P + p;
}
__device__ __forceinline__ int pack_row(const PackGeo& q, int src_kind, int j) {
    int cq = fastdiv(j, q.divT), tap = j - cq * q.T;
    int c = src_kind == 0 ? cq : fastdiv(cq, q.divNb);
    int p = src_kind == 0 ? 0 : q.hb + (cq - c * q.nb);
    return wp_row(q, tap, c, p);
}

constexpr int FP_LANES = 64;                        // words per fingerprint slot (KAN_FP_WORDS / 3 in kanconv.h)
// Content fingerprint of the reference-layout weights: two sums over the elements of bits * m(position) (mod 2^32), accumulated with
// integer atomics (order-independent, hence deterministic) into ring[cur]; ring is three slots used round-robin, and this
// launch also clears the slot of the NEXT call (nobody reads it during this one).  kan_pack_weights_cached compares
// ring[cur] with ring[cur - 1]: equal => the weights are what they were when the packed layouts were last written.
// `stride` > 1 samples every stride-th group of four elements.
// Two independent 32-bit sums: h1 = sum bits * (2 pos + 1) (odd multiplier => invertible mod 2^32: a change of any one element
// moves it) and h2 = sum rotl(bits, pos & 31).  32-bit indices and one quarter-rate multiply per element keep the kernel
// HBM-bound (with 64-bit index arithmetic and three multiplies per element it ran at 1.1 TB/s, ALU-bound).
__global__ __launch_bounds__(256) void k_fingerprint(const float* __restrict__ a, unsigned na, const float* __restrict__ b, unsigned nb,
                                                     unsigned stride, unsigned long long* __restrict__ ring, int cur) {
    __shared__ unsigned part[2][4];
    if (blockIdx.x == 0 && threadIdx.x < FP_LANES) ring[((cur + 1) % 3) * FP_LANES + threadIdx.x] = 0ull;
    unsigned h1 = 0u, h2 = 0u;
    auto fold = [&](unsigned w, unsigned p) { h1 += w * (2u * p + 1u); h2 += __builtin_rotateleft32(w, p & 31u); };
    constexpr int U = 8;                                              // independent 16-byte loads in flight per lane
    const unsigned nthreads = gridDim.x * 256u, tid0 = blockIdx.x * 256u + threadIdx.x;
    // one pass per tensor over its WHOLE groups of four; loads are unconditional on clamped indices (hipcc puts a
    // `s_waitcnt vmcnt(0)` behind every load it has to branch around, which left one load in flight: 1.2 TB/s)
    auto pass = [&](const float* __restrict__ src, unsigned n, unsigned pos_base) {
        const unsigned nfull = n / 4u, ngr = (nfull + stride - 1u) / stride;             // sampled whole groups
        for (unsigned i0 = tid0; i0 < ngr; i0 += nthreads * U) {       // (a tensor of fewer than four elements has no whole group, only a tail)
            float4 v[U]; unsigned e[U]; bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const unsigned i = i0 + u * nthreads;
                ok[u] = i < ngr;
                e[u] = (ok[u] ? i : ngr - 1u) * stride * 4u;
                v[u] = *reinterpret_cast<const float4*>(src + e[u]);   // sources are 16-byte aligned (checked on the host)
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const unsigned p = pos_base + e[u];
                if (ok[u]) { fold(__float_as_uint(v[u].x), p); fold(__float_as_uint(v[u].y), p + 1u); fold(__float_as_uint(v[u].z), p + 2u); fold(__float_as_uint(v[u].w), p + 3u); }
            }
        }
        if (tid0 == 0u) for (unsigned k = nfull * 4u; k < n; ++k) fold(__float_as_uint(src[k]), pos_base + k);     // ragged tail (< 4 elements)
    };
    if (na) pass(a, na, 0u);
    pass(b, nb, na);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { h1 += __shfl_xor(h1, off, 64); h2 += __shfl_xor(h2, off, 64); }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = h1; part[1][threadIdx.x >> 6] = h2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned s1 = part[0][0] + part[0][1] + part[0][2] + part[0][3], s2 = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        // the two sums ride in the two halves of a 64-bit word (separate 32-bit atomics: no carry between them); a slot is
        // FP_LANES words and a block adds to word blockIdx % FP_LANES (thousands of atomics on ONE address cost ~12 ns each)
        unsigned* w = reinterpret_cast<unsigned*>(ring + cur * FP_LANES + (blockIdx.x % FP_LANES));
        atomicAdd(w, s1);
        atomicAdd(w + 1, s2);
    }
}
// `fp` != NULL: the launch is a no-op when slot cur equals slot cur - 1 (weights unchanged since the layouts were written).
// Called by every thread of a workgroup (contains a barrier); the slot totals are the sums of the slot's FP_LANES words.
__device__ __forceinline__ bool fp_unchanged(const unsigned long long* fp, int cur) {
    __shared__ int same;
    if (!fp) return false;
    if (threadIdx.x < 64) {
        const int t = threadIdx.x;
        unsigned lo_c = 0, hi_c = 0, lo_p = 0, hi_p = 0;
        if (t < FP_LANES) {
            const unsigned long long c = fp[cur * FP_LANES + t], p = fp[((cur + 2) % 3) * FP_LANES + t];
            lo_c = (unsigned)c; hi_c = (unsigned)(c >> 32); lo_p = (unsigned)p; hi_p = (unsigned)(p >> 32);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            lo_c += __shfl_xor(lo_c, off, 64); hi_c += __shfl_xor(hi_c, off, 64);
            lo_p += __shfl_xor(lo_p, off, 64); hi_p += __shfl_xor(hi_p, off, 64);
        }
        if (t == 0) same = (lo_c == lo_p && hi_c == hi_p) ? 1 : 0;
    }
    __syncthreads();
    return same != 0;
}

// One launch covers both sources: tiles x < nb_base transpose the base weights (src_kind 0), the rest the basis weights.
// Grid-stride over the (x, y) tiles so that the grid stays small and an unchanged fingerprint costs microseconds.
__global__ __launch_bounds__(256) void k_pack(const float* __restrict__ src_base, const float* __restrict__ src_basis,
                                              float* __restrict__ wp, PackGeo q, int nb_base, long long wp_gstride, int tiles_x, int tiles_y,
                                              const unsigned long long* __restrict__ fp, int fp_cur) {
    __shared__ float tile[32][33];
    if (fp_unchanged(fp, fp_cur)) return;
    wp += (size_t)blockIdx.z * wp_gstride;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;           // 32 x 8
    for (int tile_id = blockIdx.x; tile_id < tiles_x * tiles_y; tile_id += gridDim.x) {
        const int by = tile_id / tiles_x, bx0 = tile_id - by * tiles_x;
        const int src_kind = bx0 < nb_base ? 0 : 1;                   // block-uniform
        const int bx = src_kind == 0 ? bx0 : bx0 - nb_base;
        const int J = src_kind == 0 ? q.C * q.T : q.C * q.nb * q.T;   // source row length
        const float* src = (src_kind == 0 ? src_base : src_basis) + (size_t)blockIdx.z * q.O * J;     // group blockIdx.z: stacked sources
        const int j0 = bx * 32, o0 = by * 32;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int o = o0 + ty + 8 * i, j = j0 + tx;
            tile[ty + 8 * i][tx] = (o < q.O && j < J) ? src[(size_t)o * J + j] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int j = j0 + ty + 8 * i, o = o0 + tx;
            if (j < J && o < q.Opad) wp[(size_t)pack_row(q, src_kind, j) * q.Opad + o] = tile[tx][ty + 8 * i];
        }
        __syncthreads();
    }
}

// Sum of the weight-gradient slabs, transposed back to the reference layout.  A tile is UNPACK_TO = 64 outputs x UNPACK_TJ = 32 source
// columns j: a thread owns one 16-byte group of four outputs in two rows (j, j + 16) of the packed slabs -- the rows are contiguous in o
// and Opad is a multiple of 64, so a tile reads whole 128-byte lines -- and the tile leaves through LDS as rows of 32 consecutive j.
// Loads are unconditional on a clamped row (pack_row once per row, not per element and slab) and all loads of a slab group are issued
// before the first add (the branchy 4-byte version kept 2 - 3 loads in flight per element); what lies outside O x J is dropped at the store.
// Per element the sum is the fixed sequence the 4-byte kernel used (and k_unpack_iod uses): eight running sums over slabs s, s + 8, ...,
// the remainder into the first, then the tree ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7)) -- the same bits.
constexpr int UNPACK_TO = 64, UNPACK_TJ = 32;
__device__ __forceinline__ float4 f4_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
// s0 (of both rows) += slabs 0 .. N - 1 at a0 / a1, in slab order; the 2 N loads go out first
template <int N>
__device__ __forceinline__ void unpack_tail(float4& r0, float4& r1, const float* a0, const float* a1, long long slab_elems) {
    float4 v0[N], v1[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        v0[i] = *reinterpret_cast<const float4*>(a0 + (size_t)i * slab_elems);
        v1[i] = *reinterpret_cast<const float4*>(a1 + (size_t)i * slab_elems);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) { r0 = f4_add(r0, v0[i]); r1 = f4_add(r1, v1[i]); }
}
__global__ __launch_bounds__(256) void k_unpack(const float* __restrict__ dwp, float* __restrict__ dst_base, float* __restrict__ dst_basis,
                                                PackGeo q, int nb_base, int n_slabs, long long slab_elems, long long dwp_gstride) {
    __shared__ float tile[UNPACK_TO][UNPACK_TJ + 1];
    const int src_kind = (int)blockIdx.x < nb_base ? 0 : 1;           // block-uniform: base gradient first, then basis
    const int bx = src_kind == 0 ? blockIdx.x : blockIdx.x - nb_base;
    const int J = src_kind == 0 ? q.C * q.T : q.C * q.nb * q.T;
    dwp += (size_t)blockIdx.z * dwp_gstride;
    float* dst = (src_kind == 0 ? dst_base : dst_basis) + (size_t)blockIdx.z * q.O * J;
    const int j0 = bx * UNPACK_TJ, o0 = blockIdx.y * UNPACK_TO;       // o0 + 64 <= Opad: no clamp along o
    const int ol = 4 * (threadIdx.x & 15), jl = threadIdx.x >> 4;     // outputs o0 + ol .. + 3 of rows j0 + jl and j0 + jl + 16
    const float* a0 = dwp + (size_t)pack_row(q, src_kind, min(j0 + jl, J - 1)) * q.Opad + o0 + ol;
    const float* a1 = dwp + (size_t)pack_row(q, src_kind, min(j0 + jl + 16, J - 1)) * q.Opad + o0 + ol;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 s[2][8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[0][i] = s[1][i] = zero;
    int sl = 0;
    for (; sl + 8 <= n_slabs; sl += 8) {                              // 16 loads in flight; fixed summation order => deterministic
        float4 v[2][8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            v[0][i] = *reinterpret_cast<const float4*>(a0 + (size_t)(sl + i) * slab_elems);
            v[1][i] = *reinterpret_cast<const float4*>(a1 + (size_t)(sl + i) * slab_elems);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) { s[0][i] = f4_add(s[0][i], v[0][i]); s[1][i] = f4_add(s[1][i], v[1][i]); }
    }
    {
        const float* b0 = a0 + (size_t)sl * slab_elems;
        const float* b1 = a1 + (size_t)sl * slab_elems;
        switch (n_slabs - sl) {                                       // (uniform) the remaining 0 - 7 slabs go into s0, in order
            case 1: unpack_tail<1>(s[0][0], s[1][0], b0, b1, slab_elems); break;
            case 2: unpack_tail<2>(s[0][0], s[1][0], b0, b1, slab_elems); break;
            case 3: unpack_tail<3>(s[0][0], s[1][0], b0, b1, slab_elems); break;
            case 4: unpack_tail<4>(s[0][0], s[1][0], b0, b1, slab_elems); break;
            case 5: unpack_tail<5>(s[0][0], s[1][0], b0, b1, slab_elems); break;
            case 6: unpack_tail<6>(s[0][0], s[1][0], b0, b1, slab_elems); break;
            case 7: unpack_tail<7>(s[0][0], s[1][0], b0, b1, slab_elems); break;
            default: break;
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const float4 t = f4_add(f4_add(f4_add(s[r][0], s[r][1]), f4_add(s[r][2], s[r][3])), f4_add(f4_add(s[r][4], s[r][5]), f4_add(s[r][6], s[r][7])));
        const int j = jl + 16 * r;
        tile[ol][j] = t.x; tile[ol + 1][j] = t.y; tile[ol + 2][j] = t.z; tile[ol + 3][j] = t.w;
    }
    __syncthreads();
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < UNPACK_TO / 8; ++i) {
        const int o = o0 + ty + 8 * i, j = j0 + tx;
        if (o < q.O && j < J) dst[(size_t)o * J + j] = tile[ty + 8 * i][tx];
    }
}

// Many-slab weight gradients (a 3-channel first layer is ONE row tile, so its pixel axis is cut ~300 ways): fold all
// slabs into slab 0 with 4 slab lanes per element and 4 partial sums per lane, then unpack a single slab.  Summation
// order is fixed (deterministic).  Block = 64 elements x 4 slab lanes.
__global__ __launch_bounds__(256) void k_fold_slabs(float* __restrict__ slabs, int n_slabs, long long slab_elems, long long n) {
    __shared__ float part[4][64];
    const int e = threadIdx.x & 63, sg = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * 64 + e;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (i < n) {
        const float* p = slabs + i;
        int sl = sg;
        for (; sl + 12 < n_slabs; sl += 16) {
            a0 += p[(size_t)sl * slab_elems]; a1 += p[(size_t)(sl + 4) * slab_elems];
            a2 += p[(size_t)(sl + 8) * slab_elems]; a3 += p[(size_t)(sl + 12) * slab_elems];
        }
        for (; sl < n_slabs; sl += 4) a0 += p[(size_t)sl * slab_elems];
    }
    part[sg][e] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (sg == 0 && i < n) slabs[i] = (part[0][e] + part[1][e]) + (part[2][e] + part[3][e]);
}

// ---------------------------------------------------------------------------- [I][O][n] coefficients of the MLP KAN heads
// The seven recurrence / Chebyshev MLP layers keep ONE parameter, coeffs[c][o][k] (input-major, basis index minor), and no base branch;
// their contraction is the conv stage on 1x1 planes with a 1x1 kernel.  The two kernels below move between that layout and the packed
// ones directly -- wp[wp_row(c, k)][o] and the flat gradient dwp[row(c, k)][o] -- so that no [O][C*n] copy of a head's weights (604 MB at
// 9216 -> 4096, degree 3) is ever made.  A tile is one input c x IOD_TO outputs: IOD_TO * n contiguous floats of coeffs on one side, n row
// segments of IOD_TO floats on the other.  LDS holds it plane-major with a pitch of IOD_TO + 4, so that the row side moves whole float4s
// (ds_read_b128 / ds_write_b128, conflict-free) and the coefficient side scatters / gathers single floats.
// `vec` bit 0: the coeffs side is 16-byte aligned per tile (base pointer aligned, O * n % 4 == 0); bit 1: the packed side is.
constexpr int IOD_TO = 256, IOD_PITCH = IOD_TO + 4;

__device__ __forceinline__ float4 iod_ld4(const float* p, bool vec) {
    return vec ? *reinterpret_cast<const float4*>(p) : make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void iod_st4(float* p, float4 v, bool vec) {
    if (vec) *reinterpret_cast<float4*>(p) = v;
    else { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
}
__device__ __forceinline__ float4 iod_add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// Tile `tile_id` -> (c, o0, live outputs no, float4 groups of the padded row segment wq).  Opad is a multiple of 32, so a group of four
// outputs is never cut by the end of a row.
struct IodTile { int c, o0, no, wq; };
__device__ __forceinline__ IodTile iod_tile(const PackGeo& q, long long tile_id, int o_tiles) {
    IodTile t;
    t.c = (int)(tile_id / o_tiles);
    t.o0 = (int)(tile_id - (long long)t.c * o_tiles) * IOD_TO;
    t.no = max(0, min(IOD_TO, q.O - t.o0));
    t.wq = min(IOD_TO, q.Opad - t.o0) >> 2;
    return t;
}

__global__ __launch_bounds__(256) void k_pack_iod(const float* __restrict__ coeffs, float* __restrict__ wp, PackGeo q, int o_tiles, long long n_tiles,
                                                  int vec) {
    __shared__ __attribute__((aligned(16))) float tile[KAN_MAX_PLANES * IOD_PITCH];
    const int n = q.nb, tid = threadIdx.x;
    for (long long tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
        const IodTile t = iod_tile(q, tile_id, o_tiles);
        const float* src = coeffs + ((size_t)t.c * q.O + t.o0) * n;
        const int cnt = t.no * n;                                   // contiguous source floats of this tile
        auto put = [&](int f, float v) { const int o = fastdiv(f, q.divNb); tile[(f - o * n) * IOD_PITCH + o] = v; };
        if (vec & 1) {                                              // (cnt is a multiple of 4 here: O * n and IOD_TO * n are)
            for (int f = 4 * tid; f < cnt; f += 1024) {
                const float4 v = *reinterpret_cast<const float4*>(src + f);
                put(f, v.x); put(f + 1, v.y); put(f + 2, v.z); put(f + 3, v.w);
            }
        } else {
            for (int f = tid; f < cnt; f += 256) put(f, src[f]);
        }
        __syncthreads();
        for (int u = tid; u < n * t.wq; u += 256) {                 // row p of the tile, outputs o .. o + 3; outputs >= O are written as zeros
            const int p = t.wq == IOD_TO / 4 ? u >> 6 : u / t.wq, o = 4 * (u - p * t.wq);
            float4 v = *reinterpret_cast<const float4*>(&tile[p * IOD_PITCH + o]);
            if (o + 3 >= t.no) { if (o >= t.no) v.x = 0.f; if (o + 1 >= t.no) v.y = 0.f; if (o + 2 >= t.no) v.z = 0.f; v.w = 0.f; }
            iod_st4(wp + (size_t)wp_row(q, 0, t.c, p) * q.Opad + t.o0 + o, v, vec & 2);
        }
        __syncthreads();
    }
}

// dcoeffs[c][o][k] = sum over the slabs of dwp[row(c, k)][o], the slabs added in the order of k_unpack (eight running sums over slabs
// s, s + 8, ..., the remainder into the first, then a fixed tree), so both unpackers return the same bits.
__global__ __launch_bounds__(256) void k_unpack_iod(const float* __restrict__ dwp, float* __restrict__ dcoeffs, PackGeo q, int o_tiles, long long n_tiles,
                                                    int n_slabs, long long slab_elems, int vec) {
    __shared__ __attribute__((aligned(16))) float tile[KAN_MAX_PLANES * IOD_PITCH];
    const int n = q.nb, tid = threadIdx.x;
    for (long long tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
        const IodTile t = iod_tile(q, tile_id, o_tiles);
        for (int u = tid; u < n * t.wq; u += 256) {
            const int p = t.wq == IOD_TO / 4 ? u >> 6 : u / t.wq, o = 4 * (u - p * t.wq);
            if (o >= t.no) continue;                                // a group of padding columns only: never read back below
            const float* a = dwp + (size_t)wp_row(q, 0, t.c, p) * q.Opad + t.o0 + o;
            const bool v2 = vec & 2;
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            float4 s0 = z, s1 = z, s2 = z, s3 = z, s4 = z, s5 = z, s6 = z, s7 = z;
            int sl = 0;
            for (; sl + 8 <= n_slabs; sl += 8) {
                const float* b = a + (size_t)sl * slab_elems;
                s0 = iod_add4(s0, iod_ld4(b, v2)); s1 = iod_add4(s1, iod_ld4(b + slab_elems, v2));
                s2 = iod_add4(s2, iod_ld4(b + 2 * slab_elems, v2)); s3 = iod_add4(s3, iod_ld4(b + 3 * slab_elems, v2));
                s4 = iod_add4(s4, iod_ld4(b + 4 * slab_elems, v2)); s5 = iod_add4(s5, iod_ld4(b + 5 * slab_elems, v2));
                s6 = iod_add4(s6, iod_ld4(b + 6 * slab_elems, v2)); s7 = iod_add4(s7, iod_ld4(b + 7 * slab_elems, v2));
            }
            for (; sl < n_slabs; ++sl) s0 = iod_add4(s0, iod_ld4(a + (size_t)sl * slab_elems, v2));
            *reinterpret_cast<float4*>(&tile[p * IOD_PITCH + o]) =
                iod_add4(iod_add4(iod_add4(s0, s1), iod_add4(s2, s3)), iod_add4(iod_add4(s4, s5), iod_add4(s6, s7)));
        }
        __syncthreads();
        float* dst = dcoeffs + ((size_t)t.c * q.O + t.o0) * n;
        const int cnt = t.no * n;
        auto get = [&](int f) { const int o = fastdiv(f, q.divNb); return tile[(f - o * n) * IOD_PITCH + o]; };
        if (vec & 1) {
            for (int f = 4 * tid; f < cnt; f += 1024) *reinterpret_cast<float4*>(dst + f) = make_float4(get(f), get(f + 1), get(f + 2), get(f + 3));
        } else {
            for (int f = tid; f < cnt; f += 256) dst[f] = get(f);
        }
        __syncthreads();
    }
}

// Backward-data weight layout, derived from the forward one by a per-tap tiled transpose:
//   wd[(tap * Opad16 + o)][ct * 128 + half * 64 + cl * P + p] = wp[k((tap*C+c), p)][o],
//   c = (ct*2 + half) * CH + cl,  CH = 64 / P whole channels per 64-column half
// i.e. the depth axis (tap, o) is the row, and the 128 columns of one channel tile are contiguous and 16-B aligned.
// Columns >= CH*P of a half and rows o >= O are zero.
__global__ __launch_bounds__(256) void k_pack_bwd_data(const float* __restrict__ wp, float* __restrict__ wd, PackGeo q,
                                                       int CH, int n_ct, int Opad32, long long wp_gstride, int tiles_x, int tiles_y,
                                                       const unsigned long long* __restrict__ fp, int fp_cur) {
    __shared__ float tile[32][33];
    if (fp_unchanged(fp, fp_cur)) return;
    const int tap = blockIdx.z;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int ncol = n_ct * 128;
    const float* const wp0 = wp; float* const wd0 = wd;
    for (int tile_id = blockIdx.x; tile_id < tiles_x * tiles_y; tile_id += gridDim.x) {      // grid-stride over the (x, y) tiles
    const int byy = tile_id / tiles_x, bxx = tile_id - byy * tiles_x;
    const int oblk = Opad32 / 32, grp = byy / oblk;                   // groups are folded into the y tiles
    const int col0 = bxx * 32, o0 = (byy - grp * oblk) * 32;          // columns of wd / rows of wd within this tap
    wp = wp0 + (size_t)grp * wp_gstride;
    wd = wd0 + (size_t)grp * q.T * Opad32 * ncol;
#pragma unroll
    for (int i = 0; i < 4; ++i) {                                   // read wp along o (contiguous)
        int col = col0 + ty + 8 * i, o = o0 + tx;
        float v = 0.f;
        if (col < ncol) {
            int hf = col >> 6, w = col & 63, cl = fastdiv(w, q.divP), p = w - cl * q.P, c = hf * CH + cl;
            if (cl < CH && c < q.C && o < q.O) {
                v = wp[(size_t)wp_row(q, tap, c, p) * q.Opad + o];
            }
        }
        tile[ty + 8 * i][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {                                   // write wd along the columns (contiguous)
        int o = o0 + ty + 8 * i, col = col0 + tx;
        if (o < Opad32 && col < ncol) wd[((size_t)tap * Opad32 + o) * ncol + col] = tile[tx][ty + 8 * i];
    }
    __syncthreads();
    }                                                               // tile loop
}

// ============================================================================ position-major copy
// dst[(c*HW + i)*B + b] = src[b*bstride + c*HW + i]: the small-plane kernels gather "one position of many images" per
// wave; in NCHW those are 4-byte reads C*HW*4 bytes apart, in this copy they are contiguous.  32x32 LDS transpose.
__global__ __launch_bounds__(256) void k_position_major(const float* __restrict__ src, float* __restrict__ dst, int B, int CHW, long long bstride) {
    __shared__ float tile[32][33];
    const int e0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = b0 + ty + 8 * i, e = e0 + tx;
        tile[ty + 8 * i][tx] = (b < B && e < CHW) ? src[(size_t)b * bstride + e] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = e0 + ty + 8 * i, b = b0 + tx;
        if (e < CHW && b < B) dst[(size_t)e * B + b] = tile[tx][ty + 8 * i];
    }
}

// ============================================================================ forward
// Workgroup tile: TO = WO*64 outputs x TP = WP*64 output pixels, one 64x64 wave tile per wave (2x2 MFMA 32x32x2).
// Pipeline per step: [expand + write step s into buffer b] barrier [issue global loads of step s+1] [MFMAs on b].
template <int KIND, int FAST, int WO, int WP, int KC>
__global__ __launch_bounds__(WO * WP * 64, (WO * WP > 4 ? 2 : 4)) void k_conv_fwd(
    const float* __restrict__ x, const float* __restrict__ xn, const float* __restrict__ wp, float* __restrict__ z,
    DevGeom g, DevBasis bs, int Opad, int IPC, int n_chunks, int chunks_per_split, long long slab_elems, unsigned x_bytes, TilePerm perm,
    int tiles_o) {
    constexpr int TO = WO * 64, TP = WP * 64, NT = WO * WP * 64, NW = WO * WP;
    constexpr int IPP = NT / TP;                          // items handled per pass over the pixels
    constexpr int UMAX = 4 / IPP;                         // units per thread (IPC <= 4)
    constexpr int RPI = 256 / TO;                         // weight rows per 1-KiB wave copy
    constexpr int NQ = (KC + RPI - 1) / RPI;              // wave copies per weight step
    static_assert(KC % 2 == 0, "KC");
    __shared__ __attribute__((aligned(16))) float sW[2 * KC * TO];
    __shared__ float sE[2 * KC * TP];
    __shared__ float sTab[KAN_MAX_TABLE];
    __shared__ float sDump[NT];                              // write-only sink for masked-off basis rows

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);           // provably wave-uniform => scalar registers
    const int w_o = wave / WP, w_p = wave % WP;
    const int HoWo = g.Ho * g.Wo, HW = g.H * g.W, T = g.kh * g.kw, P = FAST ? fast_planes(FAST) : bs.P;
    const int Mtot = g.B * HoWo, NI = g.C * T;
    const BlockId blk = xcd_block_order(!g.pix_major);
    const int grp = blk.y / tiles_o;                      // groups are folded into grid.y (scalar; 0 for ungrouped layers)
    const int px_tile0 = (perm.n ? (int)perm.idx[blk.x] : blk.x) * TP, o_tile0 = (blk.y - grp * tiles_o) * TO;
    const int pxl = (wave % (TP / 64)) * 64 + lane, il0 = wave / (TP / 64);
    {   // group grp owns channels [grp*C, (grp+1)*C) of x / xn (NCHW, or the [C*H*W][B] copy), [grp*O, ..) of z, and its own packed block
        const size_t xo = (size_t)grp * g.C * HW * (g.pix_major ? g.B : 1);
        x += xo; xn += xo;
        z += (size_t)grp * g.O * HoWo;
        wp += (size_t)grp * n_chunks * KC * Opad;
    }

    if (tid < KAN_MAX_TABLE) sTab[tid] = bs.tab[tid];
    for (int i = tid; i < 2 * KC * TP; i += NT) sE[i] = 0.f;            // pad rows stay zero for the whole kernel

    const int my_px = px_tile0 + pxl;
    const bool pv = my_px < Mtot;
    int hi0, wi0, pbase;                                     // pbase: element offset of (image, hi0, wi0); may be negative
    {
        int b, hw;
        if (g.pix_major) { hw = my_px / g.B; b = my_px - hw * g.B; }
        else { b = my_px / HoWo; hw = my_px - b * HoWo; }
        int ho = hw / g.Wo, wo = hw - ho * g.Wo;
        hi0 = ho * g.sh - g.ph; wi0 = wo * g.sw - g.pw;
        // position-major tiles read the [C*H*W][B] copy of x: element (c,hi,wi) of image b sits at (c*HW+hi*W+wi)*B + b
        pbase = g.pix_major ? (hi0 * g.W + wi0) * g.B + b : b * (int)g.xbs + hi0 * g.W + wi0;
    }
    const int estride = g.pix_major ? g.B : 1;               // element stride of the (c,hi,wi) index
    // FastKAN / LegendreKAN evaluate their basis on a second tensor, and so does any layer whose base activation the host applied
    // (x = act(input), xn = input, act = identity); the compile-time specs of the other kinds are single-input by construction
    const bool same_in = !fast_spec(FAST).xn_fwd || (x == xn);
    const kan_rsrc x_rs = make_rsrc(x, x_bytes), xn_rs = make_rsrc(same_in ? x : xn, x_bytes);
    const int wv = wave;
    const unsigned wlane = (unsigned)((lane / (TO / 4)) * Opad + (lane % (TO / 4)) * 4) * 4u;   // this lane inside a 1-KiB weight block

    float xa[UMAX], xb[UMAX]; unsigned inb_mask = 0;
    int s_ch = 0;                                            // the step whose gathers sit in xa / xb (per-channel bases decode c from it)

    // issue(ch, buf): gather the x values of step ch into registers; start the async copy of its weight rows
    // (KC rows x TO floats, a straight 2-D copy) into LDS buffer `buf`
    auto issue = [&](int ch, int buf) {
        inb_mask = 0; s_ch = ch;
#pragma unroll
        for (int u = 0; u < UMAX; ++u) {
            const int il = il0 + u * IPP;                                          // scalar
            const int item = ch * IPC + il;
            const int tap = fastdiv(item, g.divC), c = item - tap * g.C;          // tap-major depth order (scalar division)
            const int r = fastdiv(tap, g.divKw), t = tap - r * g.kw;
            const int dr = r * g.dh, dt = t * g.dw;
            const int hi = hi0 + dr, wi = wi0 + dt;
            const bool inb = il < IPC && pv && item < NI && (unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)g.W;
            const unsigned off = inb ? (unsigned)(pbase + (c * HW + dr * g.W + dt) * estride) * 4u : KAN_OOB;
            xa[u] = buf_load(x_rs, off);
            xb[u] = same_in ? xa[u] : buf_load(xn_rs, off);
            inb_mask |= (inb ? 1u : 0u) << u;
        }
        const char* wsrc = (const char*)(wp + (size_t)ch * KC * Opad + o_tile0);      // scalar
        float* dW = sW + buf * (KC * TO);
#pragma unroll
        for (int j = 0; j < (NQ + NW - 1) / NW; ++j) {
            const int q = j * NW + wv;                     // 1-KiB block index inside the weight step (wave-uniform)
            if (q < NQ) {
                if (KC % RPI == 0 || q * RPI + (int)(lane / (TO / 4)) < KC)
                    glds16((const float*)(wsrc + (size_t)q * RPI * Opad * 4 + wlane), dW + q * 256);
            }
        }
    };
    auto stage = [&](int buf) {
        float* dE = sE + buf * (KC * TP);
#pragma unroll
        for (int u = 0; u < UMAX; ++u) {
            const int il = il0 + u * IPP;
            int c = 0;
            if (KIND == KAN_BASIS_RELU) { const int item = s_ch * IPC + il; c = item - fastdiv(item, g.divC) * g.C; }
            if (il < IPC) stage_unit<KIND, FAST>(bs, sTab, (inb_mask >> u) & 1u, xa[u], xb[u], dE + (il * P) * TP + pxl, TP, sDump + tid, c);
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    int ch0 = blk.z * chunks_per_split;
    int ch1 = min(n_chunks, ch0 + chunks_per_split);
    // taps that are alive for at least one pixel position of this tile (all of them unless the tile is position-major)
    unsigned tapmask = 0xffffffffu;
    if (g.pix_major) {
        tapmask = 0;
        const int hwA = px_tile0 / g.B, hwB = min(px_tile0 + TP - 1, Mtot - 1) / g.B;
        for (int hw = hwA; hw <= hwB; ++hw)
            for (int tap = 0; tap < T; ++tap) tapmask |= (tap_alive_out(g, hw, tap) ? 1u : 0u) << tap;
        // cut this tile's split ranges over its live steps (segment = tap, starting at the step holding its first item)
        auto seg = [&](int tap) { return (tap * g.C + IPC - 1) / IPC; };
        // this tile's own split count: ~chunks_per_split live steps each; surplus workgroups only store a zero slab
        const int L = live_step_count(tapmask, T, n_chunks, seg);
        const int S = min((int)gridDim.z, max(1, (L + chunks_per_split - 1) / chunks_per_split));
        if (blk.z >= S) { ch0 = ch1 = n_chunks; }
        else {
            ch0 = blk.z == 0 ? 0 : live_step_pos(tapmask, T, n_chunks, (int)((long long)L * blk.z / S), seg);
            ch1 = blk.z == S - 1 ? n_chunks : live_step_pos(tapmask, T, n_chunks, (int)((long long)L * (blk.z + 1) / S), seg);
        }
    }
    // first step >= ch that touches a live tap (a step holds IPC consecutive items of the tap-major depth axis)
    auto next_live = [&](int ch) -> int {
        if (!g.pix_major) return ch;                       // (keeps the integer divisions below off the common path)
        while (ch < ch1) {
            const int tapA = (ch * IPC) / g.C, tapB = min(ch * IPC + IPC - 1, NI - 1) / g.C;
            if (((tapmask >> tapA) | (tapmask >> tapB)) & 1u) return ch;
            ch = max(ch + 1, ((tapB + 1) * g.C) / IPC);    // jump to the step where the next tap begins
        }
        return ch1;
    };
    int ch = next_live(ch0);
    if (ch < ch1) issue(ch, 0);
    __syncthreads();                                       // sTab + zero fill visible

    const int ao = w_o * 64 + (lane & 31), bp = w_p * 64 + (lane & 31), kh2 = lane >> 5;
    for (int cur = 0; ch < ch1; cur ^= 1) {
        stage(cur);
        // Every wave must have its own LDS-DMA weight rows landed before anyone reads them.  Waves that stage wait on
        // their gathers anyway, but a wave with no unit to stage (IPC < item lanes, or the 512-thread tile) would reach
        // the barrier with its copy in flight: the compiler does not tie global_load_lds to the barrier.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        ch = next_live(ch + 1);
        if (ch < ch1) issue(ch, cur ^ 1);
        const float* cW = sW + cur * (KC * TO);
        const float* cE = sE + cur * (KC * TP);
        // Operand fetch in explicit ISA: four ds_read_b32 per k-pair with IMMEDIATE offsets (the compiler's ds_read2 form
        // needs a v_add per address, and VALU instructions cost matrix time on this chip), and the reads of k-pair kk+1
        // are issued before the MFMAs of kk (lgkmcnt(4) = "all but the newest four have landed"; LDS returns in order),
        // so one wave alone keeps the matrix pipe fed across the LDS latency.
        const unsigned aw = lds_addr(cW + kh2 * TO + ao), ae = lds_addr(cE + kh2 * TP + bp);
        KAN_MFMA_STEP(KC / 2, aw, TO, ae, TP);
    }

    // ---- store: column (lane) = pixel => coalesced along the plane
    float* zs = z + (size_t)blk.z * slab_elems;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int px = px_tile0 + w_p * 64 + ni * 32 + (lane & 31);
        if (px >= Mtot) continue;
        int b, hw;
        if (g.pix_major) { hw = px / g.B; b = px - hw * g.B; }
        else { b = px / HoWo; hw = px - b * HoWo; }
        float* zb = zs + (size_t)b * g.ybs + hw;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = o_tile0 + w_o * 64 + mi * 32 + mfma_row(r, lane);
                if (o < g.O) zb[(size_t)o * HoWo] = acc[mi][ni][r];
            }
        }
    }
}

// ============================================================================ forward, halo variant
// The tap-major kernel above expands every input value once per TAP it is used under (9x for a 3x3 kernel), and the
// expansion is vector-ALU work that the fp32 MFMA has to share its issue slots with.  Here a workgroup expands the
// inputs its 128-pixel tile can touch ONCE per channel pair into a zero-bordered halo tile in LDS,
//     sH[channel of the pair][plane][cell],  cell = image-in-tile, row + 1, column + 1,
// and the nine taps of that pair read it through shifted addresses: the B operand of (tap, c, p) for pixel n is
// sH[c & 1][p][cell(n) + (r - 1) * (W + 2) + (t - 1)].  Weights come in the pair order of wp_row (one 18-row step = one tap
// of one channel pair), so the two k-rows of an MFMA k-pair are the same plane of the two channels.  Staging per MFMA
// drops by the tile's reuse factor (4.0 - 6.4x).  3x3, stride 1, pad 1, P = 9; tile = NIMG images x R rows x W columns.
#define LDS_READ4H(r0, r1, r2, r3, addrA, addrB0, addrB1, oA0, oA1, oB)                                                 \
    asm volatile("ds_read_b32 %0, %4 offset:%7\n\tds_read_b32 %1, %4 offset:%8\n\tds_read_b32 %2, %5 offset:%9\n\tds_read_b32 %3, %6 offset:%9" \
                 : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3) : "v"(addrA), "v"(addrB0), "v"(addrB1), "n"(oA0), "n"(oA1), "n"(oB) : "memory")

#define LDS_READ3H(r0, r1, r2, addrA, addrB, oA0, oA1, oB)                                                               \
    asm volatile("ds_read_b32 %0, %3 offset:%5\n\tds_read_b32 %1, %3 offset:%6\n\tds_read_b32 %2, %4 offset:%7"         \
                 : "=&v"(r0), "=&v"(r1), "=&v"(r2) : "v"(addrA), "v"(addrB), "n"(oA0), "n"(oA1), "n"(oB) : "memory")
#define LDS_WAIT3(r0, r1, r2, N) asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(r0), "+v"(r1), "+v"(r2) :: "memory")

template <int FAST, int WO, int W, int R, int NIMG, int QUAD = 0>
__global__ __launch_bounds__(WO * 2 * 64, ((WO > 2 && !(R * W == 16 && NIMG * W == 32)) ? 2 : 4)) void k_conv_fwd_halo(
    const float* __restrict__ x, const float* __restrict__ wp, float* __restrict__ z, DevGeom g, DevBasis bs, int Opad,
    int n_pairs, int pairs_per_split, long long slab_elems, unsigned x_bytes, int tiles_o) {
    constexpr int TO = WO * 64, TP = 128, NT = WO * 2 * 64, NW = WO * 2, P = fast_planes(FAST), KC = 2 * P, T = 9;
    constexpr int KIND = fast_kind(FAST);
    constexpr int HW_ = QUAD ? 3 : W + 2, HIMG = QUAD ? 9 : (R + 2) * HW_, HALO = (QUAD ? 32 : NIMG) * HIMG;          // cells per plane
    constexpr int RPI = 256 / TO, NQ = (KC + RPI - 1) / RPI;
    static_assert(NIMG * R * W == TP && HALO % 2 == 0, "tile shape");
    static_assert(!QUAD || (R * W == 16 && NIMG * W == 32 && WO == 4), "the quadrant order is a variant of the row-block tile");
    // Whole planes of 4 rows in a tile (4x4 planes): the tile's pixels are ordered row-major ACROSS the images, n = (row, image, column),
    // so a 32-pixel MFMA block is one output row of all 8 images -- and for the taps whose source row leaves the plane (tap row 0 under
    // output row 0, tap row 2 under the last row) the whole block multiplies the zero border: its MFMAs are skipped (exact:
    // the skipped products are all zero).  A wave owns two rows, so it skips half of its work in 3 of the 9 steps; with 8 waves the
    // pixel half is chosen by wave >> 2, which puts one wave of each half on every SIMD -- the matrix pipe of a SIMD then sees 6 instead
    // of 8 MFMAs per k-pair in 6 of 9 steps (with wave & 1 the skipping waves share two SIMDs and the others wait at the step barrier: -2 % only).
    // QUAD (the same planes, B a multiple of 32): the tile is 32 images x one 2x2 QUADRANT of the plane, pixel column n = block * 32 + image, so a
    // 32-pixel MFMA block is ONE plane position of 32 images and is wholly live or wholly dead under a tap: exactly the 25 of 36 (position, tap)
    // products that touch a real pixel are issued (5/6 = 30 of 36 with the row order).  Pixel half w_p holds the quadrant's row w_p, block q its
    // column q; wave >> 2 again puts one wave of each half on every SIMD, so every SIMD issues 25/36 of the dense MFMAs whatever the pairing --
    // and with a row per wave a lane holds two NEIGHBOURING outputs and stores them as one 8-byte word (a tile's stores are scattered over 32
    // images: with the diagonal pairing {corner, interior} / {edge, edge} and 4-byte stores the store cost ate the whole gain on 256 -> 512).
    // The halo holds the 3x3 input cells the quadrant reaches for each of the 32 images (all real inputs, no zero border; cell row / column =
    // input row / column - quadrant row / column, 288 cells per plane as before); a dead block's LDS reads may leave its image's cells by up to
    // 4 words, hence the pad of 4 words on either side.  tools/probe/quad_emul.py restates this index arithmetic in numpy.
    // The row order carries over to 8x8 planes with a HALF-plane tile, 4 images x 4 rows x 8 columns (B a multiple of 4): tile t = images 4 (t >> 1) .. + 3,
    // rows 4 (t & 1) .. + 3 -- the same B / 2 tiles as the 2-image tile -- and a 32-pixel block is one plane row of the 4 images.  Only the block of plane
    // row 0 (tap row 0) or of plane row H - 1 (tap row 2) is dead, so a tile skips one of its four blocks in three of the nine taps: 1/12 of the
    // MFMAs, every tile alike (top-half tiles skip in their pixel half 0, bottom-half tiles in half 1).
    constexpr bool ROWBLK = (NIMG * W == 32 && R == 4 && WO == 4) && !QUAD;
    constexpr bool HALFPL = ROWBLK && W == 8;               // tiles are half planes of 8 rows
    constexpr int HPAD = QUAD ? 4 : 0;
    __shared__ __attribute__((aligned(16))) float sW[2 * KC * TO];
    __shared__ float sH_[2 * P * HALO + 2 * HPAD];
    float* const sH = sH_ + HPAD;
    __shared__ float sTab[KAN_MAX_TABLE];
    __shared__ float sDump[NT];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w_o = (ROWBLK || QUAD) ? (wave & 3) : (wave >> 1), w_p = (ROWBLK || QUAD) ? (wave >> 2) : (wave & 1);
    const int HoWo = g.Ho * g.Wo, HW = g.H * g.W, Mtot = g.B * HoWo;
    const BlockId blk = xcd_block_order(true);
    const int grp = blk.y / tiles_o;
    // (QUAD) tile blk.x = 32-image group * 4 + quadrant: the four quadrants of a group are neighbours and share their input lines in L2
    const int qh = (blk.x >> 1) & 1, qw = blk.x & 1;
    const int px_tile0 = blk.x * TP, o_tile0 = (blk.y - grp * tiles_o) * TO;
    x += (size_t)grp * g.C * HW;
    z += (size_t)grp * g.O * HoWo;
    wp += (size_t)grp * n_pairs * (T * KC) * Opad;

    if (tid < KAN_MAX_TABLE) sTab[tid] = bs.tab[tid];
    for (int i = tid; i < 2 * P * HALO + 2 * HPAD; i += NT) sH_[i] = 0.f;  // borders (and out-of-image cells) stay zero for good

    // the tile: NIMG images from b0, rows [h0, h0 + R); (QUAD) 32 images from b0, input rows [qh, qh + 3), columns [qw, qw + 3)
    const int b0 = QUAD ? (blk.x >> 2) * 32 : HALFPL ? (blk.x >> 1) * NIMG : px_tile0 / HoWo;
    const int h0 = QUAD ? 0 : HALFPL ? (blk.x & 1) * R : (px_tile0 - b0 * HoWo) / W;
    // cells this thread expands every channel pair (fixed): cell -> (channel of the pair, image, halo row, halo column)
    constexpr int NCELL = 2 * HALO, CPT = (NCELL + NT - 1) / NT;
    int c_src[CPT], c_dst[CPT], c_ch[CPT]; unsigned c_ok = 0;               // x element offset (without channel) / sH offset / channel of the pair
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int idx = tid + k * NT;
        const int ch = idx / HALO, cell = idx - ch * HALO;
        const int img = cell / HIMG, rc = cell - img * HIMG, hr = rc / HW_, hc = rc - hr * HW_;
        const int b = b0 + img, h = QUAD ? qh + hr : h0 - 1 + hr, w = QUAD ? qw + hc : hc - 1;
        const bool ok = idx < NCELL && b < g.B && (unsigned)h < (unsigned)g.H && (unsigned)w < (unsigned)W;
        c_src[k] = b * (int)g.xbs + ch * HW + h * W + w;
        c_dst[k] = ch * (P * HALO) + cell;
        c_ch[k] = ch;
        c_ok |= (ok ? 1u : 0u) << k;
    }
    const kan_rsrc x_rs = make_rsrc(x, x_bytes);

    // B-operand addresses of this lane's two pixels (kh2 selects the channel of the pair)
    const int kh2 = lane >> 5;
    unsigned vb[2];
    int q_hw[2] = {0, 0}; unsigned q_live[2] = {0x1ffu, 0x1ffu};          // (QUAD, wave-uniform) plane position of the wave's two blocks, their live taps
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int n = w_p * 64 + q * 32 + (lane & 31);
        int img = n / (R * W), rem = n - img * (R * W), row = rem / W, col = rem - row * W;
        if (ROWBLK) { row = n / (NIMG * W); rem = n - row * (NIMG * W); img = rem / W; col = rem - img * W; }
        if (QUAD) {
            const int h = 2 * qh + w_p, w = 2 * qw + q;           // this wave's row of the quadrant, block q = column q
            q_hw[q] = h * 4 + w;
            unsigned m = 0;
            for (int tap = 0; tap < 9; ++tap) {
                const int r = tap / 3, t = tap - r * 3;
                m |= (((unsigned)(h + r - 1) < 4u && (unsigned)(w + t - 1) < 4u) ? 1u : 0u) << tap;
            }
            q_live[q] = m;
            vb[q] = lds_addr(sH + kh2 * (P * HALO) + (lane & 31) * HIMG + (h - qh) * HW_ + (w - qw));
            continue;
        }
        vb[q] = lds_addr(sH + kh2 * (P * HALO) + img * HIMG + (row + 1) * HW_ + (col + 1));
    }
    const int ao = w_o * 64 + (lane & 31);
    const unsigned wlane = (unsigned)((lane / (TO / 4)) * Opad + (lane % (TO / 4)) * 4) * 4u;
    const int wv = wave;

    auto issue_w = [&](int step, int buf) {                 // async copy of weight step `step` (18 rows x TO) into sW[buf]
        const char* wsrc = (const char*)(wp + (size_t)step * KC * Opad + o_tile0);
        float* dW = sW + buf * (KC * TO);
#pragma unroll
        for (int j = 0; j < (NQ + NW - 1) / NW; ++j) {
            const int q = j * NW + wv;
            if (q < NQ) {
                if (KC % RPI == 0 || q * RPI + (int)(lane / (TO / 4)) < KC)
                    glds16((const float*)(wsrc + (size_t)q * RPI * Opad * 4 + wlane), dW + q * 256);
            }
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int cp0 = blk.z * pairs_per_split, cp1 = min(n_pairs, cp0 + pairs_per_split);
    int buf = 0;
    float xv[CPT];                                           // the pair's input values, requested half a pair ahead
    auto load_pair = [&](int cp) {
#pragma unroll
        for (int k = 0; k < CPT; ++k)
            xv[k] = buf_load(x_rs, ((c_ok >> k) & 1u) ? (unsigned)(c_src[k] + 2 * cp * HW) * 4u : KAN_OOB);
    };
    if (cp0 < cp1) { issue_w(cp0 * T, 0); load_pair(cp0); }
    __syncthreads();                                         // sTab + zero fill visible
    for (int cp = cp0; cp < cp1; ++cp) {
        // ---- expand this channel pair's halo
        __syncthreads();                                     // all waves have finished reading the previous pair's halo
#pragma unroll
        for (int k = 0; k < CPT; ++k)
            if ((c_ok >> k) & 1u) stage_unit<KIND, FAST>(bs, sTab, true, xv[k], xv[k], sH + c_dst[k], HALO, sDump + tid, 2 * cp + c_ch[k]);
        // ---- nine taps: one weight step each
#pragma unroll 1
        for (int tap = 0; tap < T; ++tap) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();                                 // weights of this step landed everywhere; (tap 0) halo visible
            const int nxt = cp * T + tap + 1;
            if (nxt < cp1 * T) issue_w(nxt, buf ^ 1);
            if (tap == 4 && cp + 1 < cp1) load_pair(cp + 1);
            const int r = tap / 3, t = tap - r * 3;
            const unsigned sh = (unsigned)(((r - 1) * HW_ + (t - 1)) * 4);
            const unsigned aw = lds_addr(sW + buf * (KC * TO) + kh2 * TO + ao), ab0 = vb[0] + sh, ab1 = vb[1] + sh;
            float fa[2][2], fb[2][2];
            // (ROWBLK) this wave's rows are h0 + 2 * w_p and h0 + 2 * w_p + 1: which of its two pixel blocks this tap leaves alive
            const int dead = !ROWBLK ? -1 : (r == 0 && w_p == 0 && h0 == 0) ? 0 : (r == 2 && w_p == 1 && h0 + R == g.H) ? 1 : -1;
            // wave-uniform: scalar branches around two MFMAs each
            const bool live0 = QUAD ? ((q_live[0] >> tap) & 1u) != 0 : dead != 0, live1 = QUAD ? ((q_live[1] >> tap) & 1u) != 0 : dead != 1;
            LDS_READ4H(fa[0][0], fa[0][1], fb[0][0], fb[0][1], aw, ab0, ab1, 0, 32 * 4, 0);
#pragma unroll
            for (int kk = 0; kk < P; ++kk) {
                const int c_ = kk & 1, n_ = c_ ^ 1;
                if (kk + 1 < P) {
                    LDS_READ4H(fa[n_][0], fa[n_][1], fb[n_][0], fb[n_][1], aw, ab0, ab1, (2 * (kk + 1)) * TO * 4, (2 * (kk + 1)) * TO * 4 + 128,
                               (kk + 1) * HALO * 4);
                    LDS_WAIT4(fa[c_][0], fa[c_][1], fb[c_][0], fb[c_][1], 4);
                } else {
                    LDS_WAIT4(fa[c_][0], fa[c_][1], fb[c_][0], fb[c_][1], 0);
                }
                if (!(ROWBLK || QUAD) || live0) {
                    acc[0][0] = MFMA32(fa[c_][0], fb[c_][0], acc[0][0]);
                    acc[1][0] = MFMA32(fa[c_][1], fb[c_][0], acc[1][0]);
                }
                if (!(ROWBLK || QUAD) || live1) {
                    acc[0][1] = MFMA32(fa[c_][0], fb[c_][1], acc[0][1]);
                    acc[1][1] = MFMA32(fa[c_][1], fb[c_][1], acc[1][1]);
                }
            }
            buf ^= 1;
        }
    }

    // ---- store (as k_conv_fwd)
    float* zs = z + (size_t)blk.z * slab_elems;
    if (QUAD) {                                              // n = (block, image): the lane's two blocks are neighbours in the plane's row
        float* zb = zs + (size_t)(b0 + (lane & 31)) * g.ybs + q_hw[0];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = o_tile0 + w_o * 64 + mi * 32 + mfma_row(r, lane);
                if (o < g.O) *reinterpret_cast<float2*>(zb + (size_t)o * HoWo) = make_float2(acc[mi][0][r], acc[mi][1][r]);
            }
        }
        return;
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        int px = px_tile0 + w_p * 64 + ni * 32 + (lane & 31);
        if (ROWBLK) {                                        // n = (row, image, column) -> the plane-major pixel index
            const int l = lane & 31;
            px = (b0 + l / W) * HoWo + (h0 + w_p * 2 + ni) * W + l % W;
        }
        if (px >= Mtot) continue;
        const int b = px / HoWo, hw = px - b * HoWo;
        float* zb = zs + (size_t)b * g.ybs + hw;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = o_tile0 + w_o * 64 + mi * 32 + mfma_row(r, lane);
                if (o < g.O) zb[(size_t)o * HoWo] = acc[mi][ni][r];
            }
        }
    }
}

// Sum M per-lane values over the 64 lanes of a wave, leaving value i's total in the lanes of group i (a reduce-scatter butterfly): at every step a
// lane keeps one half of its values and receives its partner's copy of that half -- M / 2 + M / 4 + ... + 1 shuffles, then plain xor steps over the lanes
// that hold the same index (M = 16: 8 + 4 + 2 + 1 + 1 + 1 = 17 shuffles against 16 x 6 for one butterfly per value).  On return lanes with equal
// lane / (64 / M) hold `tot` = the total of value `idx`; fixed order, so the result is deterministic.
template <int M>
__device__ __forceinline__ void wave_reduce_scatter(float (&v)[M], int lane, int& idx, float& tot) {
    int base = 0;
    int m = M;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        if (m > 1) {
            const int h = m / 2;
            const bool up = (lane & off) != 0;
#pragma unroll
            for (int i = 0; i < M / 2; ++i) {
                if (i < h) {
                    const float keep = up ? v[h + i] : v[i], send = up ? v[i] : v[h + i];
                    v[i] = keep + __shfl_xor(send, off, 64);
                }
            }
            base += up ? h : 0;
            m = h;
        } else {
            v[0] += __shfl_xor(v[0], off, 64);
        }
    }
    idx = base; tot = v[0];
}

// ============================================================================ backward data
// Tile: 128 rows = two halves of 64 rows, each holding CH = 64 / P whole channels x P planes (flat cl*P + p, rest
// zero), x 128 input pixels.  Depth steps: (tap, 16 outputs); weights come from the wd layout (straight 16 x 128
// copy), dz is gathered at the output position each (input pixel, tap) pair feeds.
// Epilogue, one half at a time (32 KB of LDS): G half-tile -> LDS, then dx = sum_p plane_p'(x) * G_p.
// RB = 1 (4x4 planes, 3x3 / stride 1 / pad 1, tiles of 8 whole images): the tile's pixels are ordered (row, image, column) as in the halo
// forward, so a 32-pixel MFMA block is one input row of all 8 images; for the taps that reach it only from outside the plane (tap row 2
// for row 0, tap row 0 for row 3) the gathered dz block is all zero and its MFMAs are skipped (exact).  A wave owns two rows; so that both
// pixel halves skip the SAME amount between two barriers (a wave that skips alone just waits for the others), the depth order pairs the
// outer tap rows: a mixed step holds 8 outputs of tap (0, t) in its first four k-pairs and the same 8 outputs of tap (2, t) in the last
// four -- the waves of rows 0-1 skip a block in the second half, those of rows 2-3 in the first: 24 instead of 32 MFMAs each.  The middle
// tap row keeps plain 16-output steps.  Step index: [0, 3 n_ob) plain (t, output block), then (t, 8-output group) mixed.
// RB = 2 (the same planes, B a multiple of 32, dz given as its position-major copy dz_pm[(o * 16 + position) * B + image]): the tile is 32 images x one 2x2
// QUADRANT of the input plane, column n = block * 32 + image, tile blk.x = 32-image group * 4 + quadrant.  A 32-pixel block is one plane position and is
// wholly live or wholly dead under a tap (the forward's rule with the tap mirrored): exactly the 25 of 36 (position, tap) blocks with a source are issued.
// The four waves sit one per SIMD, so the blocks are paired diagonally -- pixel half 0 = {corner, interior}, half 1 = {edge, edge} -- and the halves hold
// 2/2 live blocks in four taps, 1/1 in four and 1/0 in one: 13/18 of dense between barriers.  Depth steps stay plain (tap, 16 outputs).  The dz tile is
// sG[block][16 outputs][32 images]: the source of (block, output) under a tap is 128 contiguous bytes of dz_pm, so wave w copies block w with two 16-byte
// LDS-DMA instructions (8 outputs each), a fixed per-lane offset and the (tap, output block) part in the scalar offset; dead blocks are not copied.
// tools/probe/quad_bwd_emul.py restates this index arithmetic in numpy.
// One step on that tile: operand B k-rows are 32 floats apart, the wave's second block 512 floats on; l0 / l1 = the wave's blocks alive (wave-uniform)
#define KAN_MFMA_STEP_QUAD(NK, addrA, LDA, addrB, l0, l1)                                                                           \
    do {                                                                                                                           \
        float fa_[2][2], fb_[2][2];                                                                                                \
        LDS_READ4(fa_[0][0], fa_[0][1], fb_[0][0], fb_[0][1], addrA, addrB, 0, 32 * 4, 0, 512 * 4);                                \
        _Pragma("unroll") for (int kk = 0; kk < (NK); ++kk) {                                                                       \
            const int c_ = kk & 1, n_ = c_ ^ 1;                                                                                    \
            if (kk + 1 < (NK)) {                                                                                                   \
                LDS_READ4(fa_[n_][0], fa_[n_][1], fb_[n_][0], fb_[n_][1], addrA, addrB, (2 * (kk + 1)) * (LDA) * 4,                \
                          (2 * (kk + 1)) * (LDA) * 4 + 128, (2 * (kk + 1)) * 32 * 4, (2 * (kk + 1)) * 32 * 4 + 512 * 4);           \
                LDS_WAIT4(fa_[c_][0], fa_[c_][1], fb_[c_][0], fb_[c_][1], 4);                                                      \
            } else {                                                                                                               \
                LDS_WAIT4(fa_[c_][0], fa_[c_][1], fb_[c_][0], fb_[c_][1], 0);                                                      \
            }                                                                                                                      \
            if (l0) {                                                                                                              \
                acc[0][0] = MFMA32(fa_[c_][0], fb_[c_][0], acc[0][0]);                                                             \
                acc[1][0] = MFMA32(fa_[c_][1], fb_[c_][0], acc[1][0]);                                                             \
            }                                                                                                                      \
            if (l1) {                                                                                                              \
                acc[0][1] = MFMA32(fa_[c_][0], fb_[c_][1], acc[0][1]);                                                             \
                acc[1][1] = MFMA32(fa_[c_][1], fb_[c_][1], acc[1][1]);                                                             \
            }                                                                                                                      \
        }                                                                                                                          \
    } while (0)

// RB = 3 (8x8 planes, 3x3 / stride 1 / pad 1, B a multiple of 32, dz given as dz_pm[(o * 64 + position) * B + image]): RB = 2 carried over with another wave
// layout.  The tile is 32 images x 4 adjacent columns of one plane row (h, w0 .. w0 + 3, w0 in {0, 4}), tile = image group * 16 + 2 h + w0 / 4 (the same B / 2
// tiles), column n = block * 32 + image, block j = position (h, w0 + j); sG[block][16 outputs][32 images] is filled as for RB = 2.  The tap rows whose source
// row h + 1 - r leaves the plane (h = 0 and h = 7: three taps each) are dead for the whole tile: their steps are skipped outright (no copies, no barrier) and
// the split ranges are cut over the live steps.  The tap columns kill block 0 of the w0 = 0 tiles (t = 2) and block 3 of the w0 = 4 tiles (t = 0): exactly 484
// of the 576 (position, tap) blocks are issued.  Each wave owns 32 ROWS x all four blocks (one A read and four B reads per k-pair; the accumulators are the
// same 64 registers, acc[j >> 1][j & 1] = block j), so between two barriers every wave skips the same block: no wave waits for another.  Epilogue: thread
// (image = tid & 31, channel = tid >> 5) contracts its channel's planes for the four positions and moves x and dx as one float4 each.  Dispatch: the 9-tap
// tiles (rows 1-6) first, then all h = 0 tiles, then all h = 7 tiles (each class walks wd in step with itself), the image group being slot % groups so that
// with 8 groups an XCD keeps one group's dz_pm and x in its L2; B / 2 tiles exceed TilePerm's 64 entries, so the order is arithmetic.  tools/probe/pos8_bwd_emul.py restates this index arithmetic in numpy.
#define LDS_READ5(ra, r0, r1, r2, r3, addrA, addrB, oA, oB)                                                                              \
    asm volatile("ds_read_b32 %0, %5 offset:%7\n\tds_read_b32 %1, %6 offset:%8\n\tds_read_b32 %2, %6 offset:%9\n\t"                    \
                 "ds_read_b32 %3, %6 offset:%10\n\tds_read_b32 %4, %6 offset:%11"                                                        \
                 : "=&v"(ra), "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3)                                                                \
                 : "v"(addrA), "v"(addrB), "n"(oA), "n"(oB), "n"((oB) + 512 * 4), "n"((oB) + 1024 * 4), "n"((oB) + 1536 * 4) : "memory")
#define LDS_WAIT5(ra, r0, r1, r2, r3, N) asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(ra), "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3) :: "memory")
// One step on that tile for a wave of 32 rows x 4 blocks: l0 / l3 = the outer blocks alive (wave-uniform, the same in every wave of the workgroup)
#define KAN_MFMA_STEP_POS8(NK, addrA, LDA, addrB, l0, l3)                                                                           \
    do {                                                                                                                           \
        float fa_[2], fb_[2][4];                                                                                                   \
        LDS_READ5(fa_[0], fb_[0][0], fb_[0][1], fb_[0][2], fb_[0][3], addrA, addrB, 0, 0);                                         \
        _Pragma("unroll") for (int kk = 0; kk < (NK); ++kk) {                                                                       \
            const int c_ = kk & 1, n_ = c_ ^ 1;                                                                                    \
            if (kk + 1 < (NK)) {                                                                                                   \
                LDS_READ5(fa_[n_], fb_[n_][0], fb_[n_][1], fb_[n_][2], fb_[n_][3], addrA, addrB, (2 * (kk + 1)) * (LDA) * 4,       \
                          (2 * (kk + 1)) * 32 * 4);                                                                                \
                LDS_WAIT5(fa_[c_], fb_[c_][0], fb_[c_][1], fb_[c_][2], fb_[c_][3], 5);                                             \
            } else {                                                                                                               \
                LDS_WAIT5(fa_[c_], fb_[c_][0], fb_[c_][1], fb_[c_][2], fb_[c_][3], 0);                                             \
            }                                                                                                                      \
            if (l0) acc[0][0] = MFMA32(fa_[c_], fb_[c_][0], acc[0][0]);                                                            \
            acc[0][1] = MFMA32(fa_[c_], fb_[c_][1], acc[0][1]);                                                                    \
            acc[1][0] = MFMA32(fa_[c_], fb_[c_][2], acc[1][0]);                                                                    \
            if (l3) acc[1][1] = MFMA32(fa_[c_], fb_[c_][3], acc[1][1]);                                                            \
        }                                                                                                                          \
    } while (0)

template <int KIND, int FAST, int RB = 0>
__global__ __launch_bounds__(256, 4) void k_conv_bwd_data(
    const float* __restrict__ dz, const float* __restrict__ x, const float* __restrict__ xn, const float* __restrict__ wd,
    float* __restrict__ dx, float* __restrict__ dxn, DevGeom g, DevBasis bs, int CH, int n_ct, int n_ob, int Opad16,
    int n_chunks, int chunks_per_split, long long slab_elems, unsigned dz_bytes, TilePerm perm, float* __restrict__ dpar) {     // grid.y = groups * n_ct
    constexpr int TP = 128, KD = 16, NT = 256;
    __shared__ __attribute__((aligned(16))) float smem[2 * 2 * KD * 128];   // 2 x (sW 16x128 + sG 16x128) = 32 KB; epilogue 64x128
    __shared__ float sTab[KAN_MAX_TABLE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);           // provably wave-uniform => scalar registers
    const int w_r = wave >> 1, w_p = wave & 1;
    const int HoWo = g.Ho * g.Wo, HW = g.H * g.W, P = bs.P;
    const int Min = g.B * HW;
    // (plain order here: an XCD then holds a few pixel tiles for ALL channel tiles, which share the dz tile; grouping by
    // split instead re-read dz once per channel tile -- measured 2.8x the fetch traffic)
    const BlockId blk = xcd_block_order(false);
    const int grp = blk.y / n_ct;                         // groups are folded into grid.y
    const int px_tile0 = (perm.n ? (int)perm.idx[blk.x] : blk.x) * TP, ct = blk.y - grp * n_ct;
    const int ncol = n_ct * 128;
    const int pxl = (wave & 1) * 64 + lane, ol0 = wave >> 1;
    // this wave's 64-row half lies wholly in the channel padding (last tile); (RB == 3) likewise its 32-row quarter of the half
    const bool idle_rows = RB == 3 ? (ct * 2 + w_r) * CH * P + w_p * 32 >= g.C * P || w_p * 32 >= CH * P : (ct * 2 + w_r) * CH >= g.C;
    // (RB == 3) the tile: dispatch slot blk.x -> tile (9-tap rows first, then the h = 0 tiles, then the h = 7 tiles), tile -> (image group, row, column half)
    int p8_tile = blk.x;
    if (RB == 3) {
        const int ng = (int)gridDim.x >> 4, nmid = 12 * ng;
        // (image group = slot % ng: with 8 groups every XCD -- workgroups are dealt to them round-robin -- keeps ONE group's dz_pm and x in its L2)
        if (blk.x < nmid) { const int k = blk.x / ng; p8_tile = (blk.x - k * ng) * 16 + 2 + k; }
        else { const int y = blk.x - nmid, cls = y >= 2 * ng ? 1 : 0, y2 = y - cls * 2 * ng, k = y2 / ng; p8_tile = (y2 - k * ng) * 16 + cls * 14 + k; }
    }
    const int p8_b0 = (p8_tile >> 4) * 32, p8_h = (p8_tile >> 1) & 7, p8_w0 = (p8_tile & 1) * 4;
    {
        const size_t xo = (size_t)grp * g.C * HW;
        x += xo; xn += xo; dx += xo; if (dxn) dxn += xo;
        dz += (size_t)grp * g.O * HoWo * ((g.pix_major || RB >= 2) ? g.B : 1);
        wd += (size_t)grp * (g.kh * g.kw) * Opad16 * ncol;
    }

    if (tid < KAN_MAX_TABLE) sTab[tid] = bs.tab[tid];
    // tile column pxl holds pixel my_px: plane-major, or (RB) column = (row, image, column) -> pixel = image * 16 + row * 4 + column
    // (RB == 2) column = (block, image): block -> plane position by the diagonal pairing (0 = the plane's corner, 1 = the interior position diagonal to
    // it, 2 / 3 = the edge positions in the corner's row / column)
    const int q_qh = (blk.x >> 1) & 1, q_qw = blk.x & 1, q_b0 = (blk.x >> 2) * 32;
    auto q_pos = [&](int bk) { return ((bk == 0 || bk == 2) ? 3 * q_qh : 1 + q_qh) * 4 + ((bk == 0 || bk == 3) ? 3 * q_qw : 1 + q_qw); };
    auto q_mask = [&](int hw) {                                // taps under which position hw has a source (an output it fed)
        unsigned m = 0;
        for (int tap = 0; tap < 9; ++tap) {
            const int r = tap / 3, t = tap - r * 3;
            m |= (((unsigned)((hw >> 2) + 1 - r) < 4u && (unsigned)((hw & 3) + 1 - t) < 4u) ? 1u : 0u) << tap;
        }
        return m;
    };
    const int my_px = RB == 2 ? (q_b0 + (pxl & 31)) * 16 + q_pos(pxl >> 5)
                              : px_tile0 + (RB == 1 ? ((pxl >> 2) & 7) * 16 + (pxl >> 5) * 4 + (pxl & 3) : pxl);
    const bool pv = my_px < Min;
    int pb, ph_, pw_;
    {
        int hw;
        if (g.pix_major) { hw = my_px / g.B; pb = my_px - hw * g.B; }
        else { pb = my_px / HW; hw = my_px - pb * HW; }
        ph_ = hw / g.W; pw_ = hw - ph_ * g.W;
    }
    // `dz` is the NCHW tensor, or (position-major tiles) its [O*Ho*Wo][B] copy: element (o,ho,wo) of image b at (o*HoWo+ho*Wo+wo)*B + b
    const kan_rsrc dz_rs = make_rsrc(dz, dz_bytes);
    const unsigned dz_img = g.pix_major ? (unsigned)pb : (unsigned)pb * (unsigned)g.ybs;
    const unsigned zstride = g.pix_major ? (unsigned)g.B : 1u;
    const int wv = wave;

    // On gfx950 the fp32 MFMA shares the vector ALU: every VALU instruction in this loop costs ~4.5 cycles of matrix
    // time (tools/probe/mfma_probe.hip), so everything that only depends on the tap is cached across the n_ob steps
    // of a tap, per-lane offsets are precomputed, and the per-step parts ride in scalar registers.
    int cur_tap = -1; unsigned base = KAN_OOB;                // gather offset of this thread's pixel for cur_tap
    const unsigned wlane = (unsigned)((lane >> 5) * ncol + (lane & 31) * 4) * 4u;      // byte offset of this lane in a 2-row weight block
    const unsigned row_bytes = (unsigned)HoWo * zstride * 4u;
    const bool o_full = (n_ob * KD == g.O);                   // no ragged last output block

    // issue(ch, buf): start the async copies of step ch into LDS buffer `buf`: the gathered dz tile (16 outputs x 128
    // pixels, 4 B per lane, masked by the buffer bounds check) and the weight rows (16 x 128, 16 B per lane)
    auto issue = [&](int ch, int buf) {
        const int tap = ch / n_ob, o0 = (ch - tap * n_ob) * KD;                       // scalar
        if (tap != cur_tap) {                                                          // uniform: once per n_ob steps
            cur_tap = tap;
            const int r = tap / g.kw, t = tap - r * g.kw;
            const int hn = ph_ + g.ph - r * g.dh, wn = pw_ + g.pw - t * g.dw;
            int ho = hn, wo = wn; bool ok = pv && hn >= 0 && wn >= 0;
            if (g.sh != 1 || g.sw != 1) {                                              // uniform; strided convs only
                ho = hn / g.sh; wo = wn / g.sw;
                ok = ok && ho * g.sh == hn && wo * g.sw == wn;
            }
            ok = ok && ho < g.Ho && wo < g.Wo;
            base = ok ? (dz_img + (unsigned)(ho * g.Wo + wo) * zstride) * 4u : KAN_OOB;
        }
        float* dW = smem + buf * (2 * KD * 128);
        float* dG = dW + KD * 128 + (wv & 1) * 64;
        const unsigned so0 = (unsigned)(o0 + ol0) * row_bytes;                         // scalar part of the offset
        if (o_full) {
#pragma unroll
            for (int n = 0; n < 8; ++n)                    // this wave's 64 pixels of row ol0 + 2n
                __builtin_amdgcn_raw_ptr_buffer_load_lds(dz_rs, (__attribute__((address_space(3))) void*)(dG + (ol0 + 2 * n) * TP), 4,
                                                         (int)base, (int)(so0 + (unsigned)(2 * n) * row_bytes), 0, 0);
        } else {
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                const int ol = ol0 + 2 * n;
                buf_load_lds4(dz_rs, o0 + ol < g.O ? base + (unsigned)(o0 + ol) * row_bytes : KAN_OOB, dG + ol * TP);
            }
        }
        const char* wsrc = (const char*)(wd + ((size_t)tap * Opad16 + o0) * ncol + ct * 128);      // scalar
#pragma unroll
        for (int j = 0; j < 2; ++j) {                      // 16 rows x 512 B = 8 wave-instructions of 1 KiB
            const int blk = j * 4 + wv;
            glds16((const float*)(wsrc + (size_t)blk * 2 * ncol * 4 + wlane), dW + blk * 256);
        }
    };

    // (RB) the paired depth order: plain steps of the middle tap row, then mixed steps (rows 0-7: tap (0,t), rows 8-15: tap (2,t))
    int rb_t = -1; unsigned baseA = KAN_OOB, baseB = KAN_OOB; bool pend_mixed = false;
    auto issue_rb = [&](int ch, int buf) {
        const int n_plain = 3 * n_ob;
        const bool mixed = ch >= n_plain;
        pend_mixed = mixed;
        int t, o0;                                                                     // scalar
        if (mixed) { const int m = ch - n_plain; t = m / (2 * n_ob); o0 = (m - t * 2 * n_ob) * 8; }
        else { t = ch / n_ob; o0 = (ch - t * n_ob) * KD; }
        const int key = mixed ? 3 + t : t;
        if (key != rb_t) {                                                             // uniform: once per tap (pair)
            rb_t = key;
            const int wn = pw_ + 1 - t;
            const bool okw = pv && wn >= 0 && wn < 4;
            const int hA = ph_ + 1 - (mixed ? 0 : 1), hB = ph_ + 1 - 2;                // source rows under tap row 0 (or 1) and 2
            baseA = (okw && hA >= 0 && hA < 4) ? (dz_img + (unsigned)(hA * 4 + wn)) * 4u : KAN_OOB;
            baseB = (okw && hB >= 0 && hB < 4) ? (dz_img + (unsigned)(hB * 4 + wn)) * 4u : KAN_OOB;
        }
        float* dW = smem + buf * (2 * KD * 128);
        float* dG = dW + KD * 128 + (wv & 1) * 64;
        // (the host takes this kernel only when O is a multiple of 16: no ragged output block, scalar row offsets)
        const unsigned soA = (unsigned)(o0 + ol0) * row_bytes;
        if (mixed) {
#pragma unroll
            for (int n = 0; n < 8; ++n)                    // row ol0 + 2n: output o0 + ((ol0 + 2n) & 7) of tap A (n < 4) or B
                __builtin_amdgcn_raw_ptr_buffer_load_lds(dz_rs, (__attribute__((address_space(3))) void*)(dG + (ol0 + 2 * n) * TP), 4,
                                                         (int)(n < 4 ? baseA : baseB), (int)(soA + (unsigned)(2 * (n & 3)) * row_bytes), 0, 0);
        } else {
#pragma unroll
            for (int n = 0; n < 8; ++n)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(dz_rs, (__attribute__((address_space(3))) void*)(dG + (ol0 + 2 * n) * TP), 4,
                                                         (int)baseA, (int)(soA + (unsigned)(2 * n) * row_bytes), 0, 0);
        }
        const int tapA = mixed ? t : 3 + t, tapB = 6 + t;
#pragma unroll
        for (int j = 0; j < 2; ++j) {                      // 16 rows x 512 B = 8 wave-instructions of 1 KiB (2 rows each)
            const int blk2 = j * 4 + wv;
            const int row = mixed ? ((blk2 < 4 ? tapA : tapB) * Opad16 + o0 + (blk2 & 3) * 2) : (tapA * Opad16 + o0 + blk2 * 2);      // scalar
            glds16((const float*)((const char*)(wd + (size_t)row * ncol + ct * 128) + wlane), dW + blk2 * 256);
        }
    };

    // (RB == 2) wave wv copies block wv: its position and live taps; the per-lane part of the source offset is fixed (lane = 8 outputs x 8 chunks of 4 images)
    const int cp_hw = q_pos(wv); const unsigned cp_live = q_mask(cp_hw);
    const unsigned q_live0 = q_mask(q_pos(2 * w_p)), q_live1 = q_mask(q_pos(2 * w_p + 1));      // the two blocks this wave multiplies
    const unsigned q_voff = (unsigned)((lane >> 3) * 16 * g.B + (lane & 7) * 4) * 4u;
    int pend_tap = 0;
    auto issue_q = [&](int ch, int buf) {
        const int tap = ch / n_ob, o0 = (ch - tap * n_ob) * KD;                       // scalar
        pend_tap = tap;
        float* dW = smem + buf * (2 * KD * 128);
        float* dG = dW + KD * 128 + wv * 512;
        if ((cp_live >> tap) & 1u) {                                                   // uniform: a dead block's copy is not issued
            const int r = tap / 3, t = tap - r * 3;
            const unsigned so = (unsigned)((o0 * 16 + cp_hw + (1 - r) * 4 + (1 - t)) * g.B + q_b0) * 4u;      // scalar part: (output block, source position, image group)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(dz_rs, (__attribute__((address_space(3))) void*)dG, 16, (int)q_voff, (int)so, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(dz_rs, (__attribute__((address_space(3))) void*)(dG + 256), 16, (int)q_voff,
                                                     (int)(so + (unsigned)(8 * 16 * g.B) * 4u), 0, 0);
        }
        const char* wsrc = (const char*)(wd + ((size_t)tap * Opad16 + o0) * ncol + ct * 128);      // scalar
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int blk2 = j * 4 + wv;
            glds16((const float*)(wsrc + (size_t)blk2 * 2 * ncol * 4 + wlane), dW + blk2 * 256);
        }
    };

    // (RB == 3) wave wv copies block wv = position (p8_h, p8_w0 + wv): dead under t = 0 in column 7, under t = 2 in column 0 (dead tap ROWS are skipped as
    // whole steps below); the same per-lane offset with 64 positions per output
    const int p8_col = p8_w0 + wv;
    const unsigned p8_voff = (unsigned)((lane >> 3) * 64 * g.B + (lane & 7) * 4) * 4u;
    auto issue_p8 = [&](int ch, int buf) {
        const int tap = ch / n_ob, o0 = (ch - tap * n_ob) * KD;                       // scalar
        pend_tap = tap;
        float* dW = smem + buf * (2 * KD * 128);
        float* dG = dW + KD * 128 + wv * 512;
        const int r = tap / 3, t = tap - r * 3;
        if ((unsigned)(p8_col + 1 - t) < 8u) {                                         // uniform: a dead block's copy is not issued
            const unsigned so = (unsigned)((o0 * 64 + (p8_h + 1 - r) * 8 + (p8_col + 1 - t)) * g.B + p8_b0) * 4u;      // scalar part: (output block, source position, image group)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(dz_rs, (__attribute__((address_space(3))) void*)dG, 16, (int)p8_voff, (int)so, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(dz_rs, (__attribute__((address_space(3))) void*)(dG + 256), 16, (int)p8_voff,
                                                     (int)(so + (unsigned)(8 * 64 * g.B) * 4u), 0, 0);
        }
        const char* wsrc = (const char*)(wd + ((size_t)tap * Opad16 + o0) * ncol + ct * 128);      // scalar
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int blk2 = j * 4 + wv;
            glds16((const float*)(wsrc + (size_t)blk2 * 2 * ncol * 4 + wlane), dW + blk2 * 256);
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    int ch0 = blk.z * chunks_per_split;
    int ch1 = min(n_chunks, ch0 + chunks_per_split);
    unsigned tapmask = 0xffffffffu;                        // taps alive for some pixel position of this tile
    const bool skip_taps = g.pix_major || RB == 3;
    if (skip_taps) {
        tapmask = 0;
        const int T = g.kh * g.kw;
        if (RB == 3) {                                     // tap rows whose source row h + 1 - r lies in the plane
            for (int r = 0; r < 3; ++r) tapmask |= ((unsigned)(p8_h + 1 - r) < 8u ? 7u : 0u) << (3 * r);
        } else {
            const int hwA = px_tile0 / g.B, hwB = min(px_tile0 + TP - 1, Min - 1) / g.B;
            for (int hw = hwA; hw <= hwB; ++hw)
                for (int tap = 0; tap < T; ++tap) tapmask |= (tap_alive_in(g, hw, tap) ? 1u : 0u) << tap;
        }
        auto seg = [&](int tap) { return tap * n_ob; };     // steps are (tap, output block)
        const int L = live_step_count(tapmask, T, n_chunks, seg);
        // ~chunks_per_split live steps each; (RB == 3) every slab of the plan an equal share of the tile's live steps
        const int S = RB == 3 ? min((int)gridDim.z, max(1, L)) : min((int)gridDim.z, max(1, (L + chunks_per_split - 1) / chunks_per_split));
        if (blk.z >= S) { ch0 = ch1 = n_chunks; }
        else {
            ch0 = blk.z == 0 ? 0 : live_step_pos(tapmask, T, n_chunks, (int)((long long)L * blk.z / S), seg);
            ch1 = blk.z == S - 1 ? n_chunks : live_step_pos(tapmask, T, n_chunks, (int)((long long)L * (blk.z + 1) / S), seg);
        }
    }
    auto next_live = [&](int ch) -> int {                  // steps are (tap, output block): skip dead taps whole
        if (!skip_taps) return ch;
        while (ch < ch1) {
            const int tap = ch / n_ob;
            if ((tapmask >> tap) & 1u) return ch;
            ch = (tap + 1) * n_ob;
        }
        return ch1;
    };
    auto issue_step = [&](int ch, int buf) {
        if (RB == 3) issue_p8(ch, buf); else if (RB == 2) issue_q(ch, buf); else if (RB) issue_rb(ch, buf); else issue(ch, buf);
    };
    int ch = next_live(ch0);
    if (ch < ch1) issue_step(ch, 0);
    const int ar = w_r * 64 + (lane & 31), bp = w_p * 64 + (lane & 31), kh2 = lane >> 5;
    for (int cur = 0; ch < ch1; cur ^= 1) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's async copies of the step have landed ...
        __syncthreads();                                   // ... and so have everyone else's; also orders the two buffers
        const bool mixed_now = pend_mixed;
        const int tap_now = pend_tap;
        ch = next_live(ch + 1);
        if (ch < ch1) issue_step(ch, cur ^ 1);
        const float* cW = smem + cur * (2 * KD * 128);
        const float* cG = cW + KD * 128;
        const unsigned aw = lds_addr(cW + kh2 * 128 + ar), ag = lds_addr(cG + kh2 * TP + bp);
        if (RB == 3) {
            // rows wave * 32 .. + 31 x the four blocks: block 0 has no source under t = 2 in the w0 = 0 tiles, block 3 none under t = 0 in the w0 = 4 tiles
            const unsigned aw8 = lds_addr(cW + kh2 * 128 + wave * 32 + (lane & 31)), ag8 = lds_addr(cG + kh2 * 32 + (lane & 31));
            const int t_now = tap_now % 3;
            const bool l0 = !(p8_w0 == 0 && t_now == 2), l3 = !(p8_w0 == 4 && t_now == 0);
            if (!idle_rows) KAN_MFMA_STEP_POS8(KD / 2, aw8, 128, ag8, l0, l3);
        } else if (RB == 2) {
            const unsigned agq = lds_addr(cG + (2 * w_p) * 512 + kh2 * 32 + (lane & 31));
            const bool l0 = ((q_live0 >> tap_now) & 1u) != 0, l1 = ((q_live1 >> tap_now) & 1u) != 0;
            if (!idle_rows) KAN_MFMA_STEP_QUAD(KD / 2, aw, 128, agq, l0, l1);
        } else if (RB) {
            // rows 2 w_p and 2 w_p + 1: row 0 has no source under tap row 2 (second half of a mixed step), row 3 none under tap row 0 (first half)
            const bool l0b = !(mixed_now && w_p == 0), l1a = !(mixed_now && w_p == 1);
            if (!idle_rows) KAN_MFMA_STEP_LIVE(KD / 2, aw, 128, ag, TP, true, l0b, l1a, true);
        } else if (!idle_rows) KAN_MFMA_STEP(KD / 2, aw, 128, ag, TP);     // (waves whose 64 rows hold no channel leave the matrix pipe to others)
    }

    // ---- epilogue: per 64-row half, G -> LDS, contract the P planes of each channel with plane'(x)
    const bool same_in = (x == xn);
    const bool split_out = (dxn != nullptr);
    float* dxs = dx + (size_t)blk.z * slab_elems;
    float* dxns = split_out ? dxn + (size_t)blk.z * slab_elems : nullptr;
    // the G rows of one half: the accumulators of its two waves -> smem[64][TP], between two barriers (the first: previous readers of smem are
    // done).  A macro: through a function the compiler no longer pairs the 64 stores into ds_write2_b32.
#define KAN_G_TO_LDS(half)                                                                                                 \
    __syncthreads();                                                                                                       \
    if (w_r == (half)) {                                                                                                   \
        _Pragma("unroll") for (int mi = 0; mi < 2; ++mi)                                                                   \
            _Pragma("unroll") for (int ni = 0; ni < 2; ++ni)                                                               \
                _Pragma("unroll") for (int r = 0; r < 16; ++r)                                                             \
                    smem[(mi * 32 + mfma_row(r, lane)) * TP + w_p * 64 + ni * 32 + (lane & 31)] = acc[mi][ni][r];          \
    }                                                                                                                      \
    __syncthreads();
    if constexpr (FAST != 0) {
        // Compile-time specs (fast_spec: FP planes, FCH = 64 / FP whole channels per half; the derivative is stage_unit_grad).  The x values
        // of this thread's (channel, pixel) pairs are requested before the LDS round trip (the generic loop below pays one dependent
        // global-load latency per channel): for both halves up front, or -- the two-tensor specs (FastKAN: x and xn in, dx and dxn out) --
        // the two inputs of one half at a time.
        constexpr FastSpec S = fast_spec(FAST);
        constexpr int FP = S.planes, FCH = 64 / FP, NIT = (FCH + 1) / 2, NPF = S.xn_bwd ? 1 : 2;      // NPF: halves prefetched at once
        if constexpr (RB == 3) {
            // thread = (image, channel): the four positions of its channel are 16 contiguous bytes of x and of dx (the host checked the alignment); a
            // wave's G rows are (wave & 1) * 32 .. + 31 of its half, all 128 columns
            constexpr int NQ = (FCH + 7) / 8;
            const int img = tid & 31, cl0 = tid >> 5;
            const size_t pix = (size_t)(p8_b0 + img) * g.xbs + (size_t)(p8_h * 8 + p8_w0);
            float4 xq[2][NQ]; unsigned okq = 0;
#pragma unroll
            for (int half = 0; half < 2; ++half)
#pragma unroll
                for (int it = 0; it < NQ; ++it) {
                    const int cl = cl0 + 8 * it, c = (ct * 2 + half) * FCH + cl;
                    const bool v = cl < FCH && c < g.C;
                    xq[half][it] = v ? *reinterpret_cast<const float4*>(x + pix + (size_t)c * HW) : make_float4(0.f, 0.f, 0.f, 0.f);
                    okq |= (v ? 1u : 0u) << (half * NQ + it);
                }
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                __syncthreads();                           // previous readers of smem are done
                if (w_r == half) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) smem[(w_p * 32 + mfma_row(r, lane)) * TP + j * 32 + (lane & 31)] = acc[j >> 1][j & 1][r];
                }
                __syncthreads();
#pragma unroll
                for (int it = 0; it < NQ; ++it) {
                    if (!((okq >> (half * NQ + it)) & 1u)) continue;
                    const int cl = cl0 + 8 * it, c = (ct * 2 + half) * FCH + cl;
                    const float4 xa = xq[half][it];
                    const float* Gc = smem + (cl * FP) * TP + img;
                    float4 d;
                    d.x = stage_unit_grad<KIND, FAST>(bs, sTab, xa.x, xa.x, Gc, TP).dx;
                    d.y = stage_unit_grad<KIND, FAST>(bs, sTab, xa.y, xa.y, Gc + 32, TP).dx;
                    d.z = stage_unit_grad<KIND, FAST>(bs, sTab, xa.z, xa.z, Gc + 64, TP).dx;
                    d.w = stage_unit_grad<KIND, FAST>(bs, sTab, xa.w, xa.w, Gc + 96, TP).dx;
                    *reinterpret_cast<float4*>(dxs + pix + (size_t)c * HW) = d;
                }
            }
            return;
        }
        float xv[NPF][NIT], nv[NIT]; unsigned ok = 0;
        // (a macro: as a by-reference lambda the same loop cost every spec ~30 instructions and, in some formulations, spills)
#define KAN_FETCH(half, slot)                                                                                              \
        _Pragma("unroll") for (int it = 0; it < NIT; ++it) {                                                                   \
            const int cl = ol0 + 2 * it, c = (ct * 2 + (half)) * FCH + cl;                                                     \
            const bool v = cl < FCH && c < g.C && pv;                                                                          \
            const size_t idx = (size_t)pb * g.xbs + (size_t)c * HW + (size_t)(ph_ * g.W + pw_);                                \
            xv[slot][it] = v ? x[idx] : 0.f;                                                                                   \
            if constexpr (S.xn_bwd) nv[it] = v ? xn[idx] : 0.f;                                                                \
            ok |= (v ? 1u : 0u) << ((slot) * NIT + it);                                                                        \
        }
        if constexpr (!S.xn_bwd) {
#pragma unroll
            for (int half = 0; half < 2; ++half) KAN_FETCH(half, half)
        }
#pragma unroll 1
        for (int half = 0; half < 2; ++half) {
            if constexpr (S.xn_bwd) { ok = 0; KAN_FETCH(half, 0) }
            KAN_G_TO_LDS(half)
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (!((ok >> ((S.xn_bwd ? 0 : half) * NIT + it)) & 1u)) continue;
                const int cl = ol0 + 2 * it, c = (ct * 2 + half) * FCH + cl;
                const float xa = (S.xn_bwd || half == 0) ? xv[0][it] : xv[NPF - 1][it];
                const InGrad d = stage_unit_grad<KIND, FAST>(bs, sTab, xa, S.xn_bwd ? nv[it] : xa, smem + (cl * FP) * TP + pxl, TP);
                const size_t idx = (size_t)pb * g.xbs + (size_t)c * HW + (size_t)(ph_ * g.W + pw_);
                dxs[idx] = d.dx;
                if constexpr (S.xn_bwd) dxns[idx] = d.dxn;
            }
        }
#undef KAN_FETCH
        return;
    }
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
        KAN_G_TO_LDS(half)
#undef KAN_G_TO_LDS
        for (int cl = ol0; cl < CH; cl += 2) {
            const int c = (ct * 2 + half) * CH + cl;
            if (c >= g.C || !pv) continue;
            const size_t idx = (size_t)pb * g.xbs + (size_t)c * HW + (size_t)(ph_ * g.W + pw_);
            const float xa = x[idx];
            const float xb = same_in ? xa : xn[idx];
            float s_base = 0.f, s_bas = 0.f;
            const float* Gc = smem + (cl * P) * TP + pxl;
            kan_planes_each<KIND, true>(bs, sTab, xa, xb, c, [&](int p, float d) {      // derivative planes streamed by run-time loops (kan_device.h)
                const float gv = Gc[p * TP];
                if (p < bs.hb) s_base += d * gv; else s_bas += d * gv;
            });
            if (split_out) { dxs[idx] = s_base; dxns[idx] = s_bas; }
            else dxs[idx] = s_base + s_bas;
        }
        if (KIND == KAN_BASIS_GRAM && dpar) {
            // GRAM-KAN: d loss / d c_{m+1} = sum over channels and pixels of sum_k act'(P_k) dP_k/dc_{m+1} G_{c,k} (gram_kan_layers.py:156-182), from
            // the same G tile.  The coefficients are layer-global, so every workgroup would hit the same few words: a thread sums over its
            // channels, the wave adds up, and lane 0 adds to one of 64 slot rows dpar[slot][n] (the host sums the rows).
            const int nb = bs.nb;
            const unsigned slot = (blockIdx.x + 7u * blockIdx.y + 13u * blockIdx.z) & 63u;
#pragma unroll 1
            for (int m = 1; m < nb - 1; ++m) {                                     // modes 1 .. nb - 2: derivative w.r.t. c_{m+1}
                DevBasis bm = bs; bm.order = m;
                float am = 0.f;
                for (int cl = ol0; cl < CH; cl += 2) {
                    const int c = (ct * 2 + half) * CH + cl;
                    if (c >= g.C || !pv) continue;
                    const float xb = (same_in ? x : xn)[(size_t)pb * g.xbs + (size_t)c * HW + (size_t)(ph_ * g.W + pw_)];      // the tensor the basis reads
                    const float* Gc = smem + (cl * P) * TP + pxl;
                    kan_planes_each<KAN_BASIS_GRAM, false>(bm, sTab, xb, xb, c, [&](int p, float v) { am += v * Gc[p * TP]; });
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) am += __shfl_xor(am, off, 64);
                if (lane == 0) atomicAdd(dpar + (size_t)slot * nb + m + 1, am);
            }
        }
        if (KIND == KAN_BASIS_RELU && dpar) {
            // Phase gradients of ReLU-KAN from the same G tile: d loss / d lo[c][j] = sum_pixels d plane_j / d lo * G_{c,j} (likewise hi) -- what two
            // more runs of the weight-gradient kernel on the parameter-derivative planes would deliver (relu_kan_layers.py:127-131).  G of a split is
            // a partial sum over its (tap, output) range and the gradient is linear in it, so every split adds its share.  Per channel: each lane
            // forms its pixel's 2 n products, the wave adds them up (xor shuffles), lane 0 adds the sums to dpar[c][2][n] (float atomics: these are
            // per-channel scalars like d gamma; the data path stays atomic-free).
            const int nb = bs.nb, hb = bs.hb;
            const float rr = bs.p0;
            for (int cl = ol0; cl < CH; cl += 2) {                                  // (wave-uniform)
                const int c = (ct * 2 + half) * CH + cl;
                if (c >= g.C) continue;
                const float xb = pv ? (same_in ? x : xn)[(size_t)pb * g.xbs + (size_t)c * HW + (size_t)(ph_ * g.W + pw_)] : 0.f;      // the tensor the basis reads
                const float* lo = bs.ctab + (size_t)c * 2 * nb;
                // The 2 n products of the channel are summed over the wave by a reduce-scatter butterfly (wave_reduce_scatter: 17 shuffles for 16 values
                // instead of 16 six-step reductions = 96), after which lane groups hold different sums and add them with ONE atomic each.
                if (2 * nb <= 16) {
                    float v[16];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float vlo = 0.f, vhi = 0.f;
                        if (j < nb) {
                            const float gv = pv ? smem[(cl * P + hb + j) * TP + pxl] : 0.f;
                            const float x1 = fmaxf(xb - lo[j], 0.f), x2 = fmaxf(lo[nb + j] - xb, 0.f);
                            const float q2 = 2.0f * (x1 * x2 * rr) * rr;
                            vlo = -(q2 * x2) * gv; vhi = (q2 * x1) * gv;
                        }
                        v[j] = vlo; v[8 + j] = vhi;
                    }
                    int idx; float tot;
                    wave_reduce_scatter<16>(v, lane, idx, tot);                    // idx < 8: lo[idx], else hi[idx - 8]
                    const int j = idx & 7;
                    if ((lane & 3) == 0 && j < nb) atomicAdd(dpar + (size_t)c * 2 * nb + (idx < 8 ? j : nb + j), tot);
                } else {
                    for (int j = 0; j < nb; ++j) {
                        const float gv = pv ? smem[(cl * P + hb + j) * TP + pxl] : 0.f;
                        const float x1 = fmaxf(xb - lo[j], 0.f), x2 = fmaxf(lo[nb + j] - xb, 0.f);
                        const float q2 = 2.0f * (x1 * x2 * rr) * rr;
                        float vlo = -(q2 * x2) * gv, vhi = (q2 * x1) * gv;
#pragma unroll
                        for (int off = 32; off > 0; off >>= 1) { vlo += __shfl_xor(vlo, off, 64); vhi += __shfl_xor(vhi, off, 64); }
                        if (lane == 0) { atomicAdd(dpar + (size_t)c * 2 * nb + j, vlo); atomicAdd(dpar + (size_t)c * 2 * nb + nb + j, vhi); }
                    }
                }
            }
        }
    }
}

// ============================================================================ backward weight
// Tile: TR = WR*64 rows of the FLAT packed K axis (row = item*P + p) x TO = WC*64 outputs; depth steps of 16 output
// pixels.  The expanded operand is written [pixel][row] (pad 1) so that both the per-pixel writes and the per-row
// MFMA reads are bank-conflict free (2-way at worst on the writes, which ds_write_b32 absorbs).
template <int KIND, int FAST, int WR, int WC>
__global__ __launch_bounds__(WR * WC * 64, (WR * WC > 4 ? 2 : 4)) void k_conv_bwd_weight(
    const float* __restrict__ dz, const float* __restrict__ x, const float* __restrict__ xn, float* __restrict__ dwp,
    DevGeom g, DevBasis bs, int Krows, int Opad, int n_chunks, int chunks_per_split, long long slab_elems,
    unsigned x_bytes, unsigned dz_bytes, int tiles_o) {
    constexpr int TR = WR * 64, TO = WC * 64, NT = WR * WC * 64, KPX = 16;
    constexpr int MRG = KAN_PMAX;                    // margin rows on both sides: units straddling the tile edge write there
    constexpr int LDE = TR + 2 * MRG + 1, LDZ = TO + 1;
    constexpr int IPP = NT / KPX;                    // items per pass (16)
    constexpr int UPF = TR / 128;                    // units per thread with register prefetch (covers P >= 8)
    constexpr int ZL = TO * KPX / NT;                // dz loads per thread
    constexpr int MAXI = TR + 2;
    __shared__ float sE[2 * KPX * LDE];
    __shared__ float sZ[2 * KPX * LDZ];
    __shared__ int sItem[MAXI];                      // c | r<<16 | t<<24, or -1
    __shared__ float sTab[KAN_MAX_TABLE];
    __shared__ float sDump[NT];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);           // provably wave-uniform => scalar registers
    const int w_r = wave / WC, w_c = wave % WC;
    const int HoWo = g.Ho * g.Wo, HW = g.H * g.W, T = g.kh * g.kw, P = FAST ? fast_planes(FAST) : bs.P;
    const int Mtot = g.B * HoWo, NI = g.C * T;
    const BlockId blk = xcd_block_order(!g.pix_major);
    const int grp = blk.y / tiles_o;                      // groups are folded into grid.y
    const int k0 = blk.x * TR, o_tile0 = (blk.y - grp * tiles_o) * TO;
    {
        const int es = g.pix_major ? g.B : 1;
        const size_t xo = (size_t)grp * g.C * HW * es;
        x += xo; xn += xo;
        dz += (size_t)grp * g.O * HoWo * es;
        dwp += (size_t)grp * Krows * Opad;
    }
    const int item_first = k0 / P;
    const int n_items = (k0 + TR - 1) / P - item_first + 1;
    const int pl = tid & (KPX - 1), il0 = tid / KPX;

    if (tid < KAN_MAX_TABLE) sTab[tid] = bs.tab[tid];
    for (int i = tid; i < n_items; i += NT) {
        int item = item_first + i, v = -1;
        if (item < NI) {
            int tap = item / g.C, c = item - tap * g.C, r = tap / g.kw, t = tap - r * g.kw;
            v = c | (r << 16) | (t << 24);
        }
        sItem[i] = v;
    }
    const bool same_in = !fast_spec(FAST).xn_fwd || (x == xn);
    __syncthreads();

    float xa[UPF], xb[UPF], zr[ZL]; unsigned inb_mask = 0;
    int s_b = 0, s_hi0 = 0, s_wi0 = 0; bool s_pv = false;    // pixel decode of the staged step (for units beyond UPF)
    const kan_rsrc x_rs = make_rsrc(x, x_bytes), xn_rs = make_rsrc(same_in ? x : xn, x_bytes), dz_rs = make_rsrc(dz, dz_bytes);
    const bool o_full = o_tile0 + TO <= g.O;                   // no ragged output tile
    const unsigned row_bytes = (unsigned)HoWo * (g.pix_major ? (unsigned)g.B : 1u) * 4u;

    auto unit_addr = [&](int it, int b, int hi0, int wi0, bool pv, unsigned& idx) -> bool {     // idx: element offset (32 bit)
        const int c = it & 0xffff, r = (it >> 16) & 0xff, t = (it >> 24) & 0xff;
        const int hi = hi0 + r * g.dh, wi = wi0 + t * g.dw;
        idx = g.pix_major ? (unsigned)((c * HW + hi * g.W + wi) * g.B + b) : (unsigned)(b * (int)g.xbs + c * HW + hi * g.W + wi);
        return pv && it >= 0 && (unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)g.W;
    };
    // The units this thread gathers with register prefetch belong to FIXED items (the K loop walks pixels, the tile's
    // rows stay): decode them once -- per step only the pixel part of the address changes.  (Was: an LDS read of the
    // item table, three integer multiplies and the unpacking, per unit per step, all of it VALU = matrix time.)
    int u_off[UPF], u_dr[UPF], u_dt[UPF], u_c[UPF]; unsigned u_ok = 0;
    const int o_row0 = (o_tile0 + il0) * HoWo;                  // first dz row of this thread (elements)
#pragma unroll
    for (int u = 0; u < UPF; ++u) {
        const int il = il0 + u * IPP;
        const int it = il < n_items ? sItem[min(il, MAXI - 1)] : -1;
        const int c = it & 0xffff, r = (it >> 16) & 0xff, t = (it >> 24) & 0xff;
        u_dr[u] = r * g.dh; u_dt[u] = t * g.dw; u_c[u] = it >= 0 ? c : 0;
        u_off[u] = (c * HW + u_dr[u] * g.W + u_dt[u]) * (g.pix_major ? g.B : 1);
        u_ok |= (it >= 0 ? 1u : 0u) << u;
    }
    auto issue = [&](int ch) {
        const int px = ch * KPX + pl;
        const bool pv = px < Mtot;
        int b, hw, ho, wo;
        if (g.pix_major) {                                     // uniform: pixel index = position * B + image
            if (g.b_shift >= 0) { hw = px >> g.b_shift; b = px & (g.B - 1); }
            else { hw = px / g.B; b = px - hw * g.B; }
            ho = hw / g.Wo; wo = hw - ho * g.Wo;
        } else if (g.howo_shift >= 0) {                        // uniform: power-of-two planes decode by shifts
            b = px >> g.howo_shift; hw = px & (HoWo - 1);
            ho = hw >> g.wo_shift; wo = hw & (g.Wo - 1);
        } else {
            b = px / HoWo; hw = px - b * HoWo;
            ho = hw / g.Wo; wo = hw - ho * g.Wo;
        }
        s_b = b; s_hi0 = ho * g.sh - g.ph; s_wi0 = wo * g.sw - g.pw; s_pv = pv;
        inb_mask = 0;
        // pixel part of the gather address: image-major b*xbs + hi0*W + wi0, position-major (hi0*W + wi0)*B + b
        const int px_off = g.pix_major ? (s_hi0 * g.W + s_wi0) * g.B + b : b * (int)g.xbs + s_hi0 * g.W + s_wi0;
#pragma unroll
        for (int u = 0; u < UPF; ++u) {
            const bool inb = pv && ((u_ok >> u) & 1u) && (unsigned)(s_hi0 + u_dr[u]) < (unsigned)g.H && (unsigned)(s_wi0 + u_dt[u]) < (unsigned)g.W;
            const unsigned off = inb ? (unsigned)(px_off + u_off[u]) * 4u : KAN_OOB;
            xa[u] = buf_load(x_rs, off);
            xb[u] = same_in ? xa[u] : buf_load(xn_rs, off);
            inb_mask |= (inb ? 1u : 0u) << u;
        }
        const unsigned zbase = !pv ? KAN_OOB
            : g.pix_major ? ((unsigned)(o_row0 + hw) * (unsigned)g.B + (unsigned)b) * 4u
                          : ((unsigned)b * (unsigned)g.ybs + (unsigned)(hw + o_row0)) * 4u;
        if (o_full) {                                          // uniform: the per-output part of the offset rides in a scalar
#pragma unroll
            for (int n = 0; n < ZL; ++n)
                zr[n] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dz_rs, (int)zbase, (int)((unsigned)(n * IPP) * row_bytes), 0));
        } else {
#pragma unroll
            for (int n = 0; n < ZL; ++n) {
                const int o = o_tile0 + il0 + n * IPP;
                zr[n] = buf_load(dz_rs, o < g.O ? zbase + (unsigned)(n * IPP) * row_bytes : KAN_OOB);
            }
        }
    };
    auto stage = [&](int buf) {
        float* dE = sE + buf * (KPX * LDE) + pl * LDE + MRG;      // row 0 of the tile sits MRG words into the line
        float* dZ = sZ + buf * (KPX * LDZ) + pl * LDZ;
#pragma unroll
        for (int u = 0; u < UPF; ++u) {
            const int il = il0 + u * IPP;
            if (il < n_items) {
                const int rbase = (item_first + il) * P - k0;
                stage_unit<KIND, FAST>(bs, sTab, (inb_mask >> u) & 1u, xa[u], xb[u], dE + rbase, 1, sDump + tid, u_c[u]);
            }
        }
#pragma unroll 1
        for (int il = il0 + UPF * IPP; il < n_items; il += IPP) {        // only for small P (many items per row tile)
            unsigned idx; float va = 0.f, vb = 0.f;
            const bool inb = unit_addr(sItem[il], s_b, s_hi0, s_wi0, s_pv, idx);
            if (inb) { va = x[idx]; vb = same_in ? va : xn[idx]; }
            const int rbase = (item_first + il) * P - k0;
            stage_unit<KIND, FAST>(bs, sTab, inb, va, vb, dE + rbase, 1, sDump + tid, sItem[il] & 0xffff);
        }
#pragma unroll
        for (int n = 0; n < ZL; ++n) dZ[il0 + n * IPP] = zr[n];
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    int ch0 = blk.z * chunks_per_split;
    int ch1 = min(n_chunks, ch0 + chunks_per_split);
    // positions whose pixels give this row tile a non-zero contribution: a row tile spans one or two taps of the
    // tap-major depth axis, and a tap is structurally zero at some output positions (position-major steps only)
    unsigned hwmask = 0xffffffffu;
    if (g.pix_major) {
        hwmask = 0;
        const int tapA = item_first / g.C, tapB = min(item_first + n_items - 1, NI - 1) / g.C;
        for (int hw = 0; hw < HoWo; ++hw)
            for (int tap = tapA; tap <= tapB; ++tap) hwmask |= (tap_alive_out(g, hw, tap) ? 1u : 0u) << hw;
        auto seg = [&](int hw) { return (hw * g.B + KPX - 1) / KPX; };   // segment = position: its first whole step
        const int L = live_step_count(hwmask, HoWo, n_chunks, seg);
        const int S = min((int)gridDim.z, max(1, (L + chunks_per_split - 1) / chunks_per_split));   // ~chunks_per_split live steps each
        if (blk.z >= S) { ch0 = ch1 = n_chunks; }
        else {
            ch0 = blk.z == 0 ? 0 : live_step_pos(hwmask, HoWo, n_chunks, (int)((long long)L * blk.z / S), seg);
            ch1 = blk.z == S - 1 ? n_chunks : live_step_pos(hwmask, HoWo, n_chunks, (int)((long long)L * (blk.z + 1) / S), seg);
        }
    }
    auto next_live = [&](int ch) -> int {
        if (!g.pix_major) return ch;
        while (ch < ch1) {
            const int hwA = (ch * KPX) / g.B, hwB = min(ch * KPX + KPX - 1, Mtot - 1) / g.B;
            if (((hwmask >> hwA) | (hwmask >> hwB)) & 1u) return ch;
            ch = max(ch + 1, ((hwB + 1) * g.B) / KPX);       // first step of the next position
        }
        return ch1;
    };
    int ch = next_live(ch0);
    if (ch < ch1) issue(ch);
    const int ar = w_r * 64 + (lane & 31), bo = w_c * 64 + (lane & 31), kh2 = lane >> 5;
    for (int cur = 0; ch < ch1; cur ^= 1) {
        stage(cur);
        __syncthreads();
        ch = next_live(ch + 1);
        if (ch < ch1) issue(ch);
        const float* cE = sE + cur * (KPX * LDE) + MRG;
        const float* cZ = sZ + cur * (KPX * LDZ);
        const unsigned ae = lds_addr(cE + kh2 * LDE + ar), az = lds_addr(cZ + kh2 * LDZ + bo);
        KAN_MFMA_STEP(KPX / 2, ae, LDE, az, LDZ);
    }

    float* out = dwp + (size_t)blk.z * slab_elems;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = k0 + w_r * 64 + mi * 32 + mfma_row(r, lane);
            if (row >= Krows) continue;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int o = o_tile0 + w_c * 64 + ni * 32 + (lane & 31);
                out[(size_t)row * Opad + o] = acc[mi][ni][r];
            }
        }
}

// ============================================================================ backward weight, halo variant
// The tap-major kernel above expands every input value once per tap it is used under and once per row tile, and stages dz
// through registers: 2.2 non-MFMA vector instructions per MFMA, and on gfx950 the fp32 MFMA shares the vector ALU.  Here
//   * rows are CHANNEL-major, row = (c*T + tap)*P + p, so a 128-row tile is 1.6 channels x all nine taps: the workgroup
//     expands the inputs of a BAND (R output rows of one image, 64 pixels = 4 MFMA steps) once per touched channel (<= 3)
//     into a zero-bordered halo tile sH[channel][plane][cell]; the nine taps of a row read the A operand through a
//     lane-constant shifted address, the pixel of a k-pair is an immediate offset (as k_conv_fwd_halo does for B);
//   * dz never passes through registers: 16 pixels x 128 outputs per step arrive by LDS-DMA (buffer_load ... lds, 4 bytes
//     per lane, 16 lanes = one 64-byte line of one output row), the per-step part of the address in a scalar register.
//     LDS-DMA places lane i at base + 4 i, so rows cannot be padded; the row [o][16 px] is XOR-swizzled instead
//     (word = px ^ ((o >> 1) & 15), chosen by the SOURCE address of each lane), which makes the B-operand reads of 32
//     consecutive outputs at one pixel hit 32 distinct banks.  The swizzle is not additive, so a lane keeps its eight
//     k-pair addresses in registers.
// Per step and wave: 32 MFMA, 32 ds_read_b32, 8 DMA instructions, ~0.3 expansions -- about 0.4 vector instructions per
// MFMA.  The weight gradient comes out in the channel-major flat order; kan_unpack_wgrad knows (the plan's HALO weight-gradient route).
#define LDS_READ4W(r0, r1, r2, r3, a0, a1, b, oA, oB0, oB1)                                                              \
    asm volatile("ds_read_b32 %0, %4 offset:%7\n\tds_read_b32 %1, %5 offset:%7\n\tds_read_b32 %2, %6 offset:%8\n\tds_read_b32 %3, %6 offset:%9" \
                 : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3) : "v"(a0), "v"(a1), "v"(b), "n"(oA), "n"(oB0), "n"(oB1) : "memory")

template <int FAST, int W, int R, int NIMG>
__global__ __launch_bounds__(256, 4) void k_conv_bwd_weight_halo(
    const float* __restrict__ dz, const float* __restrict__ x, float* __restrict__ dwp, DevGeom g, DevBasis bs, int Krows, int Opad,
    int n_bands, int bands_per_split, long long slab_elems, unsigned x_bytes, unsigned dz_bytes, int tiles_o) {
    constexpr int KIND = fast_kind(FAST);
    constexpr int P = fast_planes(FAST), T = 9, PT = P * T;
    constexpr int TR = 128, TO = 128, NT = 256, KPX = 16;
    constexpr int HWc = W + 2, HIMG = (R + 2) * HWc, CELLS = NIMG * HIMG;        // a band is NIMG images x R rows (NIMG > 1: whole images)
    constexpr int PS = W == 16 ? CELLS + 1 : W == 8 ? CELLS + 3 : W == 4 ? CELLS + 7 : CELLS + 1;   // plane stride: 2-way conflicts at worst on the A reads (brute-forced)
    constexpr int NCH = (TR + PT - 2) / PT + 1;              // channels a 128-row tile can touch
    constexpr int HB = NCH * P * PS;                         // floats per halo buffer
    constexpr int BP = NIMG * R * W, SPB = BP / KPX;         // pixels / MFMA steps per band
    constexpr int ZB = KPX * TO;                             // floats per dz buffer
    constexpr int NU = NCH * NIMG * (R + 2) * W;             // expansions per band (halo rows included, halo columns are borders)
    constexpr int SLOTS = (NU + NT - 1) / NT;
    static_assert(BP % KPX == 0 && SPB % 2 == 0 && SPB >= SLOTS + 1 && PS > CELLS && (NIMG == 1 || R == W), "band shape");
    __shared__ float sH[2 * HB];
    __shared__ __attribute__((aligned(16))) float sZ[2 * ZB];
    __shared__ float sTab[KAN_MAX_TABLE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w_r = wave >> 1, w_c = wave & 1, kh2 = lane >> 5;
    const int HoWo = g.Ho * g.Wo, HW = g.H * g.W;
    const BlockId blk = xcd_block_order(true);
    const int grp = blk.y / tiles_o;
    const int k0 = blk.x * TR, o_tile0 = (blk.y - grp * tiles_o) * TO;
    x += (size_t)grp * g.C * HW;
    dz += (size_t)grp * g.O * HoWo;
    dwp += (size_t)grp * Krows * Opad;
    const int c0 = k0 / PT;

    if (tid < KAN_MAX_TABLE) sTab[tid] = bs.tab[tid];
    for (int i = tid; i < 2 * HB; i += NT) sH[i] = 0.f;      // borders stay zero for good
    float* const dump = sH + CELLS;                           // a pad word of plane 0 that no read touches

    // ---- expansion units of this thread (fixed): unit -> (channel of the tile, halo row, column)
    int u_src[SLOTS], u_dst[SLOTS], u_hr[SLOTS], u_ch[SLOTS]; unsigned u_ok = 0;
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
        const int idx = tid + k * NT;
        constexpr int UPC = NIMG * (R + 2) * W, UPI = (R + 2) * W;        // units per channel / per image
        const int ch = idx / UPC, ri = idx - ch * UPC, img = ri / UPI, rc = ri - img * UPI, hr = rc / W, col = rc - hr * W;
        u_src[k] = (c0 + ch) * HW + img * (int)g.xbs + (hr - 1) * W + col;    // + image / band part per band
        u_dst[k] = ch * (P * PS) + img * HIMG + hr * HWc + col + 1;
        u_hr[k] = hr - 1; u_ch[k] = c0 + ch;
        u_ok |= ((idx < NU && c0 + ch < g.C) ? 1u : 0u) << k;
    }
    const kan_rsrc x_rs = make_rsrc(x, x_bytes), dz_rs = make_rsrc(dz, dz_bytes);

    // ---- A-operand addresses: this lane's two tile rows -> (channel, tap, plane) -> plane base + tap shift (+ k-half)
    unsigned aA[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        int row = k0 + w_r * 64 + mi * 32 + (lane & 31);
        if (row >= Krows) row = k0;                                         // rows past the end: any valid address (discarded at the store)
        const int c = row / PT, rem = row - c * PT, tap = rem / P, pl_ = rem - tap * P, r = tap / 3, t = tap - 3 * r;
        aA[mi] = lds_addr(sH + ((c - c0) * P + pl_) * PS + r * HWc + t + kh2);
    }
    // ---- B-operand addresses: one per k-pair (XOR swizzle), the second 32-output block and the buffer are immediates
    unsigned bB[KPX / 2];
    {
        const int ol = w_c * 64 + (lane & 31), sw = (ol >> 1) & 15;
#pragma unroll
        for (int kk = 0; kk < KPX / 2; ++kk) bB[kk] = lds_addr(sZ + ol * KPX + ((2 * kk + kh2) ^ sw));
    }
    // ---- dz DMA: wave w copies chunks m = 8 w .. 8 w + 7 (64 words = 4 output rows x 16 pixels); lane -> (row, swizzled pixel)
    unsigned zoff[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ol = 4 * (wave * 8 + j) + (lane >> 4), q = (lane & 15) ^ ((ol >> 1) & 15);
        zoff[j] = o_tile0 + ol < g.O ? (unsigned)((o_tile0 + ol) * HoWo + q) * 4u : KAN_OOB;
    }
    constexpr int BPI = NIMG > 1 ? 1 : (W * W) / BP;          // bands per image (square planes: H == W is checked on the host)
    auto issue_dz = [&](int band, int st, int zb) {
        const int gpx = band * BP + st * KPX;                  // pixel index in (image, position) order; a step never straddles images
        const int b = gpx / (W * W), px0 = gpx - b * (W * W);
        const int soff = __builtin_amdgcn_readfirstlane((b * (int)g.ybs + px0) * 4);
        float* dst = sZ + zb * ZB + wave * (8 * 64);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(dz_rs, (__attribute__((address_space(3))) void*)(dst + j * 64), 4, (int)zoff[j], soff, 0, 0);
    };
    float xv[SLOTS]; unsigned inb_mask = 0;
    auto load_band = [&](int band) {
        const int b = NIMG > 1 ? band * NIMG : band / BPI, h0 = NIMG > 1 ? 0 : (band - b * BPI) * R;
        const int sbase = b * (int)g.xbs + h0 * W;
        inb_mask = 0;
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) {
            const bool inb = ((u_ok >> k) & 1u) && (unsigned)(h0 + u_hr[k]) < (unsigned)g.H;
            xv[k] = buf_load(x_rs, inb ? (unsigned)(sbase + u_src[k]) * 4u : KAN_OOB);
            inb_mask |= (inb ? 1u : 0u) << k;
        }
    };
    auto expand = [&](int k, int hb) {
        if ((u_ok >> k) & 1u)
            stage_unit<KIND, FAST>(bs, sTab, (inb_mask >> k) & 1u, xv[k], xv[k], sH + hb * HB + u_dst[k], PS, dump, u_ch[k]);
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int nb0 = blk.z * bands_per_split, nb1 = min(n_bands, nb0 + bands_per_split);
    __syncthreads();                                          // sTab, zero fill
    if (nb0 < nb1) {
        load_band(nb0);
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) expand(k, 0);
        issue_dz(nb0, 0, 0);
    }
    int hb = 0;
    for (int band = nb0; band < nb1; ++band, hb ^= 1) {
        const unsigned hoff = (unsigned)(hb * HB * 4);
        const unsigned a0 = aA[0] + hoff, a1 = aA[1] + hoff;
#pragma unroll
        for (int st = 0; st < SPB; ++st) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this step's dz landed (own DMAs), the next band's inputs arrived
            __syncthreads();                                  // ... everybody's; halo of this band visible; previous step's reads done
            // next step's dz -> the other buffer
            if (st + 1 < SPB) issue_dz(band, st + 1, (st + 1) & 1);
            else if (band + 1 < nb1) issue_dz(band + 1, 0, 0);
            if (st == 0) { if (band + 1 < nb1) load_band(band + 1); }
            else if (st - 1 < SLOTS) { if (band + 1 < nb1) expand(st - 1, hb ^ 1); }
            // ---- 8 k-pairs of this step
            float fa[2][2], fb[2][2];
#define KAN_OFFA(kk) ((((16 * st + 2 * (kk)) / (R * W)) * HIMG + (((16 * st + 2 * (kk)) % (R * W)) / W) * HWc + ((16 * st + 2 * (kk)) % W)) * 4)
#define KAN_OFFB(kk) (((st & 1) * ZB) * 4)
            LDS_READ4W(fa[0][0], fa[0][1], fb[0][0], fb[0][1], a0, a1, bB[0], KAN_OFFA(0), KAN_OFFB(0), KAN_OFFB(0) + 32 * KPX * 4);
#pragma unroll
            for (int kk = 0; kk < KPX / 2; ++kk) {
                const int c_ = kk & 1, n_ = c_ ^ 1;
                if (kk + 1 < KPX / 2) {
                    LDS_READ4W(fa[n_][0], fa[n_][1], fb[n_][0], fb[n_][1], a0, a1, bB[kk + 1], KAN_OFFA(kk + 1), KAN_OFFB(kk + 1),
                               KAN_OFFB(kk + 1) + 32 * KPX * 4);
                    LDS_WAIT4(fa[c_][0], fa[c_][1], fb[c_][0], fb[c_][1], 4);
                } else {
                    LDS_WAIT4(fa[c_][0], fa[c_][1], fb[c_][0], fb[c_][1], 0);
                }
                acc[0][0] = MFMA32(fa[c_][0], fb[c_][0], acc[0][0]);
                acc[0][1] = MFMA32(fa[c_][0], fb[c_][1], acc[0][1]);
                acc[1][0] = MFMA32(fa[c_][1], fb[c_][0], acc[1][0]);
                acc[1][1] = MFMA32(fa[c_][1], fb[c_][1], acc[1][1]);
            }
#undef KAN_OFFA
#undef KAN_OFFB
        }
    }

    float* out = dwp + (size_t)blk.z * slab_elems;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = k0 + w_r * 64 + mi * 32 + mfma_row(r, lane);
            if (row >= Krows) continue;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int o = o_tile0 + w_c * 64 + ni * 32 + (lane & 31);
                out[(size_t)row * Opad + o] = acc[mi][ni][r];
            }
        }
}

// ============================================================================ backward weight on 8x8 planes: nine taps per wave, dead taps skipped
// The halo kernel above issues all 576 (position, tap) products of a plane although only 484 have a source inside it: its 32-row MFMA
// blocks mix three or four taps and its k-pairs are two neighbouring pixels, so no (block, k-pair) is ever wholly dead.  Here
//   * a wave owns one ROW GROUP -- 32 consecutive (c, p) pairs, index c*9 + p -- under ALL nine taps: nine 32x32 blocks (144 accumulators)
//     against 32 outputs; the four waves of a workgroup share the group and split 128 outputs.  The nine A operands of a lane are one
//     halo address plus the tap shifts r*(W+2) + t, immediates.  Row (c, tap, p) of a block lands in slab row (c*9 + tap)*9 + p as before;
//   * a band is two whole images and a k-pair is the SAME position of both, so every MFMA has one plane position and its taps are live
//     or dead at compile time (4 in the corners, 6 on the edges, 9 inside): the dead ones and their ds_read are not emitted, the same
//     for every wave.  A step is one plane row (8 positions x 2 images = 16 dz words per output); the rows come in three bodies;
//   * the halo tile sH[5 channels x 9 planes][2 images x 100 cells] is single-buffered (36 KB; two would not leave room for two
//     workgroups per CU): the next band's inputs wait in registers and are expanded behind one extra barrier per band (64 MFMA k-pairs);
//   * dz arrives as in the halo kernel (4-byte LDS-DMA, [o][16 words], word = px ^ ((o >> 1) & 15)) with px = 2*column + image.
// tools/probe/pos8_bw_emul.py restates this index arithmetic in numpy (coverage, live taps, bank sets).
#define P8_READ(dst, addr, off) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=&v"(dst) : "v"(addr), "n"(off) : "memory")
#define P8_WAIT(reg, N) asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(reg) : "n"(N) : "memory")
#define P8_TIE(reg) asm volatile("" : "+v"(reg))
constexpr int P8_W = 8, P8_HWC = P8_W + 2, P8_HIMG = P8_HWC * P8_HWC, P8_CELLS = 2 * P8_HIMG;
constexpr int P8_PS = P8_CELLS + 1;                      // plane stride: odd, so the 32 consecutive planes of a lane half hit 32 banks (the halves never conflict)
constexpr int P8_NCH = 5, P8_ZB = 16 * 128;              // channels a row group can touch; floats per dz buffer
__host__ __device__ constexpr bool pos8_col_live(int w, int t) { return w + t - 1 >= 0 && w + t - 1 < P8_W; }
__host__ __device__ constexpr int pos8_col_reads(int w, int rows) { return 1 + rows * ((w == 0 || w == P8_W - 1) ? 2 : 3); }

// One plane row: RK = 0 top (tap row 0 dead), 1 middle, 2 bottom (tap row 2 dead); ZPAR = dz buffer.  a_row = the lane's halo address of
// (plane row h, column 0) under tap (0, 0).  The operands of column w + 1 are read while the MFMAs of column w issue.
template <int RK, int ZPAR>
__device__ __forceinline__ void pos8_row(f32x16 (&acc)[9], unsigned a_row, const unsigned (&bB)[8]) {
    constexpr int R0 = RK == 0 ? 1 : 0, R1 = RK == 2 ? 1 : 2, NR = R1 - R0 + 1;
    float fa[2][9], fb[2];
#define P8_READS(w_, s_)                                                                                                          \
    do {                                                                                                                         \
        P8_READ(fb[s_], bB[w_], ZPAR * P8_ZB * 4);                                                                              \
        _Pragma("unroll") for (int r = R0; r <= R1; ++r)                                                                         \
            _Pragma("unroll") for (int t = 0; t < 3; ++t)                                                                        \
                if (pos8_col_live(w_, t)) P8_READ(fa[s_][r * 3 + t], a_row, (r * P8_HWC + t + (w_)) * 4);                        \
    } while (0)
    P8_READS(0, 0);
#pragma unroll
    for (int w = 0; w < P8_W; ++w) {
        const int c_ = w & 1, n_ = c_ ^ 1;
        if (w + 1 < P8_W) {
            P8_READS(w + 1, n_);
            P8_WAIT(fb[c_], pos8_col_reads(w + 1 < P8_W ? w + 1 : 0, NR));
        } else {
            P8_WAIT(fb[c_], 0);
        }
#pragma unroll
        for (int r = R0; r <= R1; ++r)
#pragma unroll
            for (int t = 0; t < 3; ++t)
                if (pos8_col_live(w, t)) {
                    P8_TIE(fa[c_][r * 3 + t]);
                    acc[r * 3 + t] = MFMA32(fa[c_][r * 3 + t], fb[c_], acc[r * 3 + t]);
                }
    }
#undef P8_READS
}

template <int FAST>
__global__ __launch_bounds__(256, 2) void k_conv_bwd_weight_pos8(
    const float* __restrict__ dz, const float* __restrict__ x, float* __restrict__ dwp, DevGeom g, DevBasis bs, int Krows, int Opad,
    int n_bands, int bands_per_split, long long slab_elems, unsigned x_bytes, unsigned dz_bytes, int tiles_o) {
    constexpr int KIND = fast_kind(FAST);
    constexpr int P = fast_planes(FAST), T = 9, NT = 256;
    constexpr int HB = P8_NCH * P * P8_PS;                   // floats of the halo tile
    constexpr int NU = P8_NCH * 2 * P8_W * P8_W;             // expansions per band: 5 channels x 2 images x 64 pixels (the border cells stay zero)
    constexpr int SLOTS = (NU + NT - 1) / NT;
    static_assert(P == 9, "row groups of 32 (c, p) pairs: nine planes per channel");
    __shared__ float sH[HB];
    __shared__ __attribute__((aligned(16))) float sZ[2 * P8_ZB];
    __shared__ float sTab[KAN_MAX_TABLE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kh2 = lane >> 5;
    const BlockId blk = xcd_block_order(true);
    const int grp = blk.y / tiles_o;
    const int q0 = blk.x * 32, o_tile0 = (blk.y - grp * tiles_o) * 128;      // first (c, p) pair of the row group, first output of the tile
    x += (size_t)grp * g.C * 64;
    dz += (size_t)grp * g.O * 64;
    dwp += (size_t)grp * Krows * Opad;
    const int c0 = q0 / P;

    if (tid < KAN_MAX_TABLE) sTab[tid] = bs.tab[tid];
    for (int i = tid; i < HB; i += NT) sH[i] = 0.f;          // borders (and the planes of channels past C) stay zero for good
    float* const dump = sH + P8_CELLS;                        // the pad word of plane 0, which no read touches

    // ---- expansion units of this thread (fixed): unit -> (channel of the tile, image of the band, pixel)
    int u_src[SLOTS], u_dst[SLOTS], u_ch[SLOTS]; unsigned u_ok = 0;
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
        const int idx = tid + k * NT;
        const int ch = idx >> 7, img = (idx >> 6) & 1, pos = idx & 63, h = pos >> 3, w = pos & 7;
        u_src[k] = (c0 + ch) * 64 + img * (int)g.xbs + pos;                  // + the band's first image per band
        u_dst[k] = ch * (P * P8_PS) + img * P8_HIMG + (h + 1) * P8_HWC + w + 1;
        u_ch[k] = c0 + ch;
        u_ok |= ((idx < NU && c0 + ch < g.C) ? 1u : 0u) << k;
    }
    const kan_rsrc x_rs = make_rsrc(x, x_bytes), dz_rs = make_rsrc(dz, dz_bytes);

    // ---- A-operand address: this lane's (c, p) pair -> plane of the tile (+ image of its k-half); taps, rows and columns are immediates
    const unsigned aA = lds_addr(sH + (q0 + (lane & 31) - c0 * P) * P8_PS + kh2 * P8_HIMG);
    // ---- B-operand addresses: one per k-pair = column (XOR swizzle: not additive), the buffer is an immediate
    unsigned bB[8];
    {
        const int ol = wave * 32 + (lane & 31), sw = (ol >> 1) & 15;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) bB[kk] = lds_addr(sZ + ol * 16 + ((2 * kk + kh2) ^ sw));
    }
    // ---- dz DMA: wave w copies chunks m = 8 w .. 8 w + 7 (64 words = 4 output rows x 16 words); lane -> (row, swizzled word = 2*column + image)
    unsigned zoff[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ol = 4 * (wave * 8 + j) + (lane >> 4), q = (lane & 15) ^ ((ol >> 1) & 15);
        zoff[j] = o_tile0 + ol < g.O ? (unsigned)((o_tile0 + ol) * 64 + (q >> 1) + (q & 1) * (int)g.ybs) * 4u : KAN_OOB;
    }
    auto issue_dz = [&](int band, int st, int zb) {           // plane row st of the band's two images
        const int soff = __builtin_amdgcn_readfirstlane((2 * band * (int)g.ybs + st * P8_W) * 4);
        float* dst = sZ + zb * P8_ZB + wave * (8 * 64);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(dz_rs, (__attribute__((address_space(3))) void*)(dst + j * 64), 4, (int)zoff[j], soff, 0, 0);
    };
    float xv[SLOTS];
    auto load_band = [&](int band) {
        const int sbase = 2 * band * (int)g.xbs;
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) xv[k] = buf_load(x_rs, ((u_ok >> k) & 1u) ? (unsigned)(sbase + u_src[k]) * 4u : KAN_OOB);
    };
    auto expand_band = [&]() {
#pragma unroll
        for (int k = 0; k < SLOTS; ++k)
            if ((u_ok >> k) & 1u) stage_unit<KIND, FAST>(bs, sTab, true, xv[k], xv[k], sH + u_dst[k], P8_PS, dump, u_ch[k]);
    };

    f32x16 acc[9];
#pragma unroll
    for (int a = 0; a < 9; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

    const int nb0 = blk.z * bands_per_split, nb1 = min(n_bands, nb0 + bands_per_split);
    __syncthreads();                                          // sTab, zero fill
    if (nb0 < nb1) {
        load_band(nb0);
        expand_band();
        issue_dz(nb0, 0, 0);
    }
    for (int band = nb0; band < nb1; ++band) {
        const bool more = band + 1 < nb1;
        auto step = [&](int st) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this step's dz landed (own DMAs), the next band's inputs arrived
            __syncthreads();                                  // ... everybody's; halo of this band visible; previous step's reads done
            if (st + 1 < P8_W) issue_dz(band, st + 1, (st + 1) & 1);
            else if (more) issue_dz(band + 1, 0, 0);
            if (st == 0 && more) load_band(band + 1);
        };
        step(0);
        pos8_row<0, 0>(acc, aA, bB);
#pragma unroll 1
        for (int st = 1; st < P8_W - 1; st += 2) {
            step(st);
            pos8_row<1, 1>(acc, aA + (unsigned)(st * P8_HWC * 4), bB);
            step(st + 1);
            pos8_row<1, 0>(acc, aA + (unsigned)((st + 1) * P8_HWC * 4), bB);
        }
        step(P8_W - 1);
        pos8_row<2, 1>(acc, aA + (unsigned)((P8_W - 1) * P8_HWC * 4), bB);
        if (more) {
            __syncthreads();                                  // every wave has read this band's halo
            expand_band();
        }
    }

    float* out = dwp + (size_t)blk.z * slab_elems;
    const int o = o_tile0 + wave * 32 + (lane & 31);
    if (o < Opad) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = q0 + mfma_row(r, lane);
            if (q >= g.C * P) continue;
            const int c = q / P, p = q - c * P;
#pragma unroll
            for (int tap = 0; tap < T; ++tap) out[(size_t)((c * T + tap) * P + p) * Opad + o] = acc[tap][r];
        }
    }
}

// ============================================================================ position-major, expanded: small planes
// On 4x4 / 2x2 planes a launch sees only B*16 / B*4 pixels against up to 85 MB of weights; the position-major launches of
// the tap-major kernels (which skip the taps that read padding) ran at 0.49 - 0.55 matrix-pipe busy with 2.6 - 3.2 vector
// instructions per MFMA: every (pixel, tap) pair re-expands its input value in every row tile, dz passes through registers.
// Here the EXPANDED operand is materialised once per layer call in position-major order,
//     e_pm[((c*HW + pos)*P + p)*B + b] = plane_p(x[b][c][pos])        (19 - 75 MB on the KAN-VGG layers, next to 85 MB of weights),
// and the weight-gradient kernel below is DMA + MFMA only: both operands arrive by LDS-DMA in the XOR-swizzled [row][16 px]
// layout of k_conv_bwd_weight_halo (16 images of one position are contiguous in e_pm and in dz_pm).
template <int KIND, int FAST>
__global__ __launch_bounds__(256) void k_expand_pm(const float* __restrict__ x, float* __restrict__ e_pm, DevBasis bs, int B, int CHW, int HW, int Cg,
                                                   long long bstride, float* __restrict__ dump) {
    __shared__ float tile[32][33];
    __shared__ float sTab[KAN_MAX_TABLE];
    const int e0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int P = FAST ? fast_planes(FAST) : bs.P;
    if (threadIdx.x < KAN_MAX_TABLE) sTab[threadIdx.x] = bs.tab[threadIdx.x];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = b0 + ty + 8 * i, e = e0 + tx;
        tile[ty + 8 * i][tx] = (b < B && e < CHW) ? x[(size_t)b * bstride + e] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = e0 + ty + 8 * i, b = b0 + tx;
        if (e < CHW && b < B) {
            const float v = tile[tx][ty + 8 * i];
            stage_unit<KIND, FAST>(bs, sTab, true, v, v, e_pm + (size_t)e * P * B + b, B, dump + threadIdx.x, (e / HW) % Cg);   // channel inside its group
        }
    }
}

// Forward on the expanded operand: z[o][px] = sum_k wp[k][o] e[k][px], 128 outputs x 128 images of ONE output position, a step = one tap
// of a channel pair (KC = 2 P rows: the tap-major packed layout with IPC = 2); both operands are straight LDS-DMA copies (16 B per
// lane): KC x 128 weights, and KC rows of 128 consecutive images out of e_pm.  Dead (position, tap) pairs are skipped, split
// ranges cut over live steps (as k_conv_fwd).
template <int KC>
__global__ __launch_bounds__(256, 4) void k_conv_fwd_pmdma(
    const float* __restrict__ e_pm, const float* __restrict__ wp, float* __restrict__ z, DevGeom g, int P, FastDiv divP, int Opad,
    int n_chunks, int chunks_per_split, long long slab_elems, unsigned e_bytes, unsigned w_bytes, TilePerm perm, int tiles_o, int xcd) {
    constexpr int TO = 128, TP = 128, NT = 256, NQ = KC / 2;               // NQ 1-KiB wave copies per operand and step
    __shared__ __attribute__((aligned(16))) float sW[2 * KC * TO];
    __shared__ __attribute__((aligned(16))) float sE[2 * KC * TP];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w_o = wave >> 1, w_p = wave & 1, kh2 = lane >> 5;
    const int HoWo = g.Ho * g.Wo, HW = g.H * g.W, T = g.kh * g.kw;
    const BlockId blk = xcd_block_order(xcd != 0);
    const int grp = blk.y / tiles_o;
    const int px_tile0 = (perm.n ? (int)perm.idx[blk.x] : blk.x) * TP, o_tile0 = (blk.y - grp * tiles_o) * TO;
    const int pos = px_tile0 / g.B, b0 = px_tile0 - pos * g.B;             // the tile: images b0 .. b0 + 127 of output position pos
    e_pm += (size_t)grp * g.C * HW * P * g.B;
    z += (size_t)grp * g.O * HoWo;
    wp += (size_t)grp * n_chunks * KC * Opad;
    const kan_rsrc e_rs = make_rsrc(e_pm, e_bytes), w_rs = make_rsrc(wp, w_bytes);
    const int ho = pos / g.Wo, wo = pos - ho * g.Wo;

    // per-lane parts of the DMA sources (wave w issues copies q = w, w + 4, w + 8 of each operand: two rows per copy)
    unsigned eoff[(NQ + 3) / 4];
#pragma unroll
    for (int j = 0; j < (NQ + 3) / 4; ++j) {
        const int r = 2 * (j * 4 + wave) + (lane >> 5), cl = fastdiv(min(r, KC - 1), divP), pp = min(r, KC - 1) - cl * P;
        eoff[j] = (unsigned)(((cl * HW) * P + pp) * g.B + (lane & 31) * 4) * 4u;
    }
    const unsigned woff = (unsigned)((lane >> 5) * Opad + (lane & 31) * 4) * 4u;
    auto issue = [&](int ch, int buf) {
        const int item = 2 * ch, tap = fastdiv(item, g.divC), c = item - tap * g.C;
        const int r = fastdiv(tap, g.divKw), t = tap - r * g.kw;
        const int inpos = (ho * g.sh - g.ph + r * g.dh) * g.W + (wo * g.sw - g.pw + t * g.dw);       // live steps only
        const int se = __builtin_amdgcn_readfirstlane((((c * HW + inpos) * P) * g.B + b0) * 4);
        const int sw = __builtin_amdgcn_readfirstlane((ch * KC * Opad + o_tile0) * 4);
        float* dE = sE + buf * (KC * TP);
        float* dW = sW + buf * (KC * TO);
#pragma unroll
        for (int j = 0; j < (NQ + 3) / 4; ++j) {
            const int q = j * 4 + wave;
            if (q < NQ) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(e_rs, (__attribute__((address_space(3))) void*)(dE + q * 256), 16, (int)eoff[j], se, 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (__attribute__((address_space(3))) void*)(dW + q * 256), 16, (int)woff,
                                                         sw + q * 2 * Opad * 4, 0, 0);
            }
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    unsigned tapmask = 0;
    for (int tap = 0; tap < T; ++tap) tapmask |= (tap_alive_out(g, pos, tap) ? 1u : 0u) << tap;
    auto seg = [&](int tap) { return (tap * g.C + 1) / 2; };
    int ch0, ch1;
    {
        const int L = live_step_count(tapmask, T, n_chunks, seg);
        const int S = min((int)gridDim.z, max(1, (L + chunks_per_split - 1) / chunks_per_split));
        if (blk.z >= S) { ch0 = ch1 = n_chunks; }
        else {
            ch0 = blk.z == 0 ? 0 : live_step_pos(tapmask, T, n_chunks, (int)((long long)L * blk.z / S), seg);
            ch1 = blk.z == S - 1 ? n_chunks : live_step_pos(tapmask, T, n_chunks, (int)((long long)L * (blk.z + 1) / S), seg);
        }
    }
    auto next_live = [&](int ch) -> int {
        while (ch < ch1) {
            const int tap = (2 * ch) / g.C;
            if ((tapmask >> tap) & 1u) return ch;
            ch = ((tap + 1) * g.C) / 2;
        }
        return ch1;
    };
    int ch = next_live(ch0);
    if (ch < ch1) issue(ch, 0);
    const int ao = w_o * 64 + (lane & 31), bp = w_p * 64 + (lane & 31);
    for (int cur = 0; ch < ch1; cur ^= 1) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        ch = next_live(ch + 1);
        if (ch < ch1) issue(ch, cur ^ 1);
        const unsigned aw = lds_addr(sW + cur * (KC * TO) + kh2 * TO + ao), ae = lds_addr(sE + cur * (KC * TP) + kh2 * TP + bp);
        KAN_MFMA_STEP(KC / 2, aw, TO, ae, TP);
    }

    float* zs = z + (size_t)blk.z * slab_elems;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int b = b0 + w_p * 64 + ni * 32 + (lane & 31);
        if (b >= g.B) continue;
        float* zb = zs + (size_t)b * g.ybs + pos;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = o_tile0 + w_o * 64 + mi * 32 + mfma_row(r, lane);
                if (o < g.O) zb[(size_t)o * HoWo] = acc[mi][ni][r];
            }
    }
}

// The same forward on 2x2 planes under 3x3 / stride 1 / pad 1 / dilation 1, the four output positions on the A (weight) side.  There every
// (output position q, input position p) pair is live under exactly one tap, tap(q, p) = (p_r - q_r + 1) * 3 + (p_c - q_c + 1) =
// tap(q, 0) + 3 p_r + p_c: a dense GEMM.  A tile is 32 outputs x 4 positions (128 A rows) x 128 images; a step is (input position p,
// channel pair) in (p, pair) order: B = the 18 e_pm rows of the pair at p (as above), A = sW[18][128] with column
// (o_l >> 4) * 64 + q * 16 + (o_l & 15), each 16-byte DMA chunk four consecutive outputs of step (tap(q, p), pair) of wp.  The per-lane
// part of the source is tap(q, 0)'s step, the row and the chunk; p and the pair only move the wave-uniform part, so the loop holds no
// vector address arithmetic.  For a fixed q ascending p is ascending live tap, and split z takes steps [z n / S, (z + 1) n / S) of the
// n = 4 C / 2, which is where live_step_pos cuts the kernel above: slab z holds the same partial sums, accumulated in the same order
// (bit-identical slabs).  Wave w_o owns outputs 16 w_o .. + 15 under all four q, MFMA block mi the positions 2 mi and 2 mi + 1, so by the
// 32x32 accumulator layout a lane holds the four positions of one (b, o) in acc[0][ni][r], acc[0][ni][r + 8], acc[1][ni][r],
// acc[1][ni][r + 8] (r < 8) and stores them as ONE 16-byte group z[b][o][0..3]: 16 stores per lane instead of 64, registers r & 3 and the
// lane halves completing a 128-byte line within four store instructions (the kernel above leaves each group to four workgroups).
// tools/probe/fwd_wq_emul.py restates this index arithmetic in numpy.
template <int KC>
__global__ __launch_bounds__(256, 4) void k_conv_fwd_pmdma_wq(
    const float* __restrict__ e_pm, const float* __restrict__ wp, float* __restrict__ z, DevGeom g, int Opad, int n_chunks,
    int chunks_per_split, long long slab_elems, unsigned e_bytes, unsigned w_bytes, int tiles_o, int xcd) {
    constexpr int TO = 128, TP = 128, NQ = KC / 2, P = KC / 2, HW = 4;     // NQ 1-KiB wave copies per operand and step
    __shared__ __attribute__((aligned(16))) float sW[2 * KC * TO];
    __shared__ __attribute__((aligned(16))) float sE[2 * KC * TP];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w_o = wave >> 1, w_p = wave & 1, kh2 = lane >> 5;
    const BlockId blk = xcd_block_order(xcd != 0);
    const int grp = blk.y / tiles_o, tiles_b = g.B / TP;                   // grid.x = 4 output sub-tiles x image tiles (the tile count of the kernel above)
    const int sub = blk.x / tiles_b, b0 = (blk.x - sub * tiles_b) * TP;
    const int o_tile0 = ((blk.y - grp * tiles_o) * 4 + sub) * 32;          // the tile: outputs o_tile0 .. + 31 at all four positions, images b0 .. + 127
    const int pairs = g.C >> 1;
    e_pm += (size_t)grp * g.C * HW * P * g.B;
    z += (size_t)grp * g.O * HW;
    wp += (size_t)grp * n_chunks * KC * Opad;
    const kan_rsrc e_rs = make_rsrc(e_pm, e_bytes), w_rs = make_rsrc(wp, w_bytes);

    // per-lane parts of the DMA sources (wave w issues copies w, w + 4, w + 8 of each operand: two rows per copy)
    unsigned eoff[(NQ + 3) / 4];
#pragma unroll
    for (int j = 0; j < (NQ + 3) / 4; ++j) {
        const int r = min(2 * (j * 4 + wave) + (lane >> 5), KC - 1), cl = r / P, pp = r - cl * P;
        eoff[j] = (unsigned)(((cl * HW) * P + pp) * g.B + (lane & 31) * 4) * 4u;
    }
    unsigned woff;
    {
        const int col = (lane & 31) * 4, q = (col >> 4) & 3, o_l = (col >> 6) * 16 + (col & 15);
        const int tap0 = (1 - (q >> 1)) * 3 + (1 - (q & 1));               // tap(q, p = 0)
        woff = (unsigned)((tap0 * pairs * KC + (lane >> 5)) * Opad + o_l) * 4u;
    }
    auto issue = [&](int p, int pair, int buf) {
        const int se = __builtin_amdgcn_readfirstlane((((2 * pair * HW + p) * P) * g.B + b0) * 4);
        const int sw = __builtin_amdgcn_readfirstlane(((((3 * (p >> 1) + (p & 1)) * pairs + pair) * KC) * Opad + o_tile0) * 4);
        float* dE = sE + buf * (KC * TP);
        float* dW = sW + buf * (KC * TO);
#pragma unroll
        for (int j = 0; j < (NQ + 3) / 4; ++j) {
            const int q = j * 4 + wave;
            if (q < NQ) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(e_rs, (__attribute__((address_space(3))) void*)(dE + q * 256), 16, (int)eoff[j], se, 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (__attribute__((address_space(3))) void*)(dW + q * 256), 16, (int)woff,
                                                         sw + q * 2 * Opad * 4, 0, 0);
            }
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    int ch0, ch1;                                                          // steps [ch0, ch1) of the n = 4 * pairs, all live
    {
        const int L = HW * pairs;
        const int S = min((int)gridDim.z, max(1, (L + chunks_per_split - 1) / chunks_per_split));
        if (blk.z >= S) { ch0 = ch1 = L; }
        else {
            ch0 = (int)((long long)L * blk.z / S);
            ch1 = blk.z == S - 1 ? L : (int)((long long)L * (blk.z + 1) / S);
        }
    }
    int p = ch0 / pairs, pair = ch0 - p * pairs;                           // of the step to issue next
    int ch = ch0;
    if (ch < ch1) issue(p, pair, 0);
    const int ao = w_o * 64 + (lane & 31), bp = w_p * 64 + (lane & 31);
    for (int cur = 0; ch < ch1; cur ^= 1) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        ++ch;
        if (++pair == pairs) { pair = 0; ++p; }
        if (ch < ch1) issue(p, pair, cur ^ 1);
        const unsigned aw = lds_addr(sW + cur * (KC * TO) + kh2 * TO + ao), ae = lds_addr(sE + cur * (KC * TP) + kh2 * TP + bp);
        KAN_MFMA_STEP(KC / 2, aw, TO, ae, TP);
    }

    float* zs = z + (size_t)blk.z * slab_elems;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int b = b0 + w_p * 64 + ni * 32 + (lane & 31);
        if (b >= g.B) continue;
        float* zb = zs + (size_t)b * g.ybs;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int o = o_tile0 + w_o * 16 + mfma_row(r, lane);          // rows 0 .. 15 of the block: (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
            if (o < g.O) *reinterpret_cast<float4*>(zb + (size_t)o * 4) = make_float4(acc[0][ni][r], acc[0][ni][r + 8], acc[1][ni][r], acc[1][ni][r + 8]);
        }
    }
}

// dW tile = 128 rows of the tap-major flat K axis (one tap: C*P % 128 == 0 is required) x 128 outputs; a step = 16 images of one
// output position; steps whose (position, tap) pair reads padding are skipped, split ranges are cut over live steps
// (as k_conv_bwd_weight).  No staging code at all.  Round 3: both operands are [row][16 images] with the images contiguous in HBM and in LDS,
// so they move by 16-BYTE LDS-DMA (one wave instruction = 16 rows x 64 bytes) and are read by ds_read_b128 -- a lane fetches four
// consecutive images of its row at once.  The reduction index of an MFMA k-pair is free as long as A and B agree: lanes 0 - 31 own images
// {0-3, 8-11} of the step, lanes 32 - 63 images {4-7, 12-15}; k-pair kk pairs image 4 (kk / 4) * 2 ... i.e. element (kk & 3) of each lane's
// (kk >> 2)-th fetch.  The 16-byte chunks of a row are XOR-swizzled by (row >> 2) & 3 (chosen at the DMA source), which makes the b128
// reads of 16 rows hit 64 distinct banks.  Per step and wave: 4 DMA instructions (was 16), 8 ds_read_b128 (was 32 ds_read_b32), 32 MFMA.
// Dispatch order (round 3).  A tile's live work depends on its tap (9 / 12 / 16 live positions on a 4x4 plane) and every tile is cut into
// ceil(live / target) splits, so the launch is ~2 000 workgroups of 96 - 144 steps over 1 024 slots: dispatched tap by tap, the second wave of
// workgroups started behind whatever the first happened to hold and the launch took ~300 step times for 225 steps of work per slot.  Workgroups are
// dealt in order of their linear id as slots free up, so the host sorts the (tap, split) classes by DECREASING step count (longest first: greedy
// list scheduling) and the kernel looks its (tile, split) up from a flat id; empty splits (they still write their zero slab) come last.
constexpr int PM_ORDER_MAX = 72;
struct PmOrder { int n, tiles_r_per_tap, xcd; unsigned char tap[PM_ORDER_MAX], z[PM_ORDER_MAX]; int first[PM_ORDER_MAX + 1]; };   // n == 0: plain 3-D grid

typedef float f32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256, 4) void k_conv_bwd_weight_pmdma(
    const float* __restrict__ dz_pm, const float* __restrict__ e_pm, float* __restrict__ dwp, DevGeom g, int P, FastDiv divP, int Krows, int Opad,
    int n_chunks, int chunks_per_split, long long slab_elems, unsigned e_bytes, unsigned dz_bytes, int tiles_o, int max_splits, PmOrder ord) {
    constexpr int TR = 128, TO = 128, KPX = 16, ZB = KPX * TO, AB = KPX * TR;
    __shared__ __attribute__((aligned(16))) float sA[2 * AB];
    __shared__ __attribute__((aligned(16))) float sZ[2 * ZB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w_r = wave >> 1, w_c = wave & 1, kh2 = lane >> 5;
    const int HoWo = g.Ho * g.Wo, HW = g.H * g.W, CP = g.C * P;
    BlockId blk{(int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z};
    if (ord.n) {                                              // flat grid, longest (tap, split) class first
        const int lin = (int)blockIdx.x;
        int e = 0;
        while (e + 1 < ord.n && lin >= ord.first[e + 1]) ++e;
        // Inside a class: workgroup ids go round-robin over the 8 XCDs, each with its own L2, and a (row tile, output tile) workgroup reads 128 rows of the
        // expanded operand and 128 rows of dz over its pixel range.  XCD k takes a CONTIGUOUS range of the class, ordered output tile fastest, so that the
        // workgroups sharing a row tile (its 4 output tiles) and those sharing an output tile run side by side behind ONE L2: each operand line is
        // fetched once per XCD for ~4 consumers (was: row-tile neighbours on different XCDs, the expanded operand re-fetched by every output tile).
        const int rel0 = lin - ord.first[e], per = ord.first[e + 1] - ord.first[e], ny = per / ord.tiles_r_per_tap;
        const int rel = ((per & 7) == 0 && (ord.first[e] & 7) == 0 && ord.xcd) ? (rel0 & 7) * (per >> 3) + (rel0 >> 3) : rel0;
        const int xr = rel / ny, y = rel - xr * ny;
        blk.x = (int)ord.tap[e] * ord.tiles_r_per_tap + xr; blk.y = y; blk.z = (int)ord.z[e];
    }
    const int grp = blk.y / tiles_o;
    const int k0 = blk.x * TR, o_tile0 = (blk.y - grp * tiles_o) * TO;
    e_pm += (size_t)grp * g.C * HW * P * g.B;
    dz_pm += (size_t)grp * g.O * HoWo * g.B;
    dwp += (size_t)grp * Krows * Opad;
    const int tap = k0 / CP, tr = tap / g.kw, tt = tap - tr * g.kw;          // the tile's tap (uniform)
    const kan_rsrc e_rs = make_rsrc(e_pm, e_bytes), dz_rs = make_rsrc(dz_pm, dz_bytes);

    // ---- DMA sources: wave w copies 16-row chunks m = 2 w, 2 w + 1 of each operand; lane -> (row = lane >> 2, 16-byte slot = lane & 3),
    //      the slot holds source chunk slot ^ ((row >> 2) & 3)
    unsigned aoff[2], zoff[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int rl = 16 * (wave * 2 + j) + (lane >> 2), cs = (lane & 3) ^ ((rl >> 2) & 3);
        const int row = k0 + rl, rem = min(row, Krows - 1) - tap * CP, c = fastdiv(rem, divP), pp = rem - c * P;     // (computed unconditionally: no branch)
        const unsigned va = (unsigned)(((c * HW) * P + pp) * g.B + cs * 4) * 4u, vz = (unsigned)((o_tile0 + rl) * HoWo * g.B + cs * 4) * 4u;
        aoff[j] = row < Krows ? va : KAN_OOB;
        zoff[j] = o_tile0 + rl < g.O ? vz : KAN_OOB;
    }
    // ---- operand read addresses: two 16-byte fetches per 32-row block (chunks kh2 and 2 + kh2 of the lane's row), buffer as an immediate
    unsigned aA[2][2], bB[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        const int rl = w_r * 64 + mi * 32 + (lane & 31), ol = w_c * 64 + mi * 32 + (lane & 31);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            aA[mi][h] = lds_addr(sA + rl * KPX + (((2 * h + kh2) ^ ((rl >> 2) & 3)) * 4));
            bB[mi][h] = lds_addr(sZ + ol * KPX + (((2 * h + kh2) ^ ((ol >> 2) & 3)) * 4));
        }
    }
    auto issue = [&](int ch, int buf) {
        const int px = ch * KPX, pos = px / g.B, b0 = px - pos * g.B;      // 16 images b0.. of output position pos
        const int ho = pos / g.Wo, wo = pos - ho * g.Wo;
        const int inpos = (ho * g.sh - g.ph + tr * g.dh) * g.W + (wo * g.sw - g.pw + tt * g.dw);     // live steps only: inside the image
        const int sa = __builtin_amdgcn_readfirstlane((inpos * P * g.B + b0) * 4), sz = __builtin_amdgcn_readfirstlane((pos * g.B + b0) * 4);
        float* dA = sA + buf * AB + wave * (2 * 256);
        float* dZ = sZ + buf * ZB + wave * (2 * 256);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(e_rs, (__attribute__((address_space(3))) void*)(dA + j * 256), 16, (int)aoff[j], sa, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(dz_rs, (__attribute__((address_space(3))) void*)(dZ + j * 256), 16, (int)zoff[j], sz, 0, 0);
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    // live positions of this tap, split ranges over live steps (k_conv_bwd_weight's scheme)
    unsigned hwmask = 0;
    for (int hw = 0; hw < HoWo; ++hw) hwmask |= (tap_alive_out(g, hw, tap) ? 1u : 0u) << hw;
    auto seg = [&](int hw) { return (hw * g.B + KPX - 1) / KPX; };
    int ch0, ch1;
    {
        const int L = live_step_count(hwmask, HoWo, n_chunks, seg);
        const int S = min(max_splits, max(1, (L + chunks_per_split - 1) / chunks_per_split));
        if (blk.z >= S) { ch0 = ch1 = n_chunks; }
        else {
            ch0 = blk.z == 0 ? 0 : live_step_pos(hwmask, HoWo, n_chunks, (int)((long long)L * blk.z / S), seg);
            ch1 = blk.z == S - 1 ? n_chunks : live_step_pos(hwmask, HoWo, n_chunks, (int)((long long)L * (blk.z + 1) / S), seg);
        }
    }
    auto next_live = [&](int ch) -> int {
        while (ch < ch1) {
            const int hw = (ch * KPX) / g.B;
            if ((hwmask >> hw) & 1u) return ch;
            ch = ((hw + 1) * g.B) / KPX;                        // first step of the next position
        }
        return ch1;
    };
    int ch = next_live(ch0);
    if (ch < ch1) issue(ch, 0);
    // the buffer index is a literal in each copy of the step, so that every LDS offset is an immediate
#define KAN_RD4(CUR, h_)                                                                                                    \
    asm volatile("ds_read_b128 %0, %4 offset:%8\n\tds_read_b128 %1, %5 offset:%8\n\tds_read_b128 %2, %6 offset:%8\n\tds_read_b128 %3, %7 offset:%8" \
                 : "=&v"(fa[h_][0]), "=&v"(fa[h_][1]), "=&v"(fb[h_][0]), "=&v"(fb[h_][1])                                      \
                 : "v"(aA[0][h_]), "v"(aA[1][h_]), "v"(bB[0][h_]), "v"(bB[1][h_]), "n"((CUR) * AB * 4) : "memory")
#define KAN_PM_HALF(h_)                                                                                                     \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                                          \
        acc[0][0] = MFMA32(fa[h_][0][e], fb[h_][0][e], acc[0][0]);                                                            \
        acc[0][1] = MFMA32(fa[h_][0][e], fb[h_][1][e], acc[0][1]);                                                            \
        acc[1][0] = MFMA32(fa[h_][1][e], fb[h_][0][e], acc[1][0]);                                                            \
        acc[1][1] = MFMA32(fa[h_][1][e], fb[h_][1][e], acc[1][1]);                                                            \
    }
#define KAN_PM_STEP(CUR)                                                                                     \
    do {                                                                                                     \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                     \
        __syncthreads();                                                                                     \
        ch = next_live(ch + 1);                                                                              \
        if (ch < ch1) issue(ch, (CUR) ^ 1);                                                                  \
        f32x4 fa[2][2], fb[2][2];                                                                            \
        KAN_RD4(CUR, 0);                                                                                     \
        KAN_RD4(CUR, 1);                                                                                     \
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(fa[0][0]), "+v"(fa[0][1]), "+v"(fb[0][0]), "+v"(fb[0][1]) :: "memory"); \
        KAN_PM_HALF(0)                                                                                       \
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[1][0]), "+v"(fa[1][1]), "+v"(fb[1][0]), "+v"(fb[1][1]) :: "memory"); \
        KAN_PM_HALF(1)                                                                                       \
    } while (0)
    static_assert(AB == ZB, "one immediate serves both operands");
    while (ch < ch1) {                                       // (a `break` between the two copies made hipcc spill 59 VGPRs)
        KAN_PM_STEP(0);
        if (ch < ch1) { KAN_PM_STEP(1); }
    }
#undef KAN_PM_STEP
#undef KAN_PM_HALF
#undef KAN_RD4

    float* out = dwp + (size_t)blk.z * slab_elems;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = k0 + w_r * 64 + mi * 32 + mfma_row(r, lane);
            if (row >= Krows) continue;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int o = o_tile0 + w_c * 64 + ni * 32 + (lane & 31);
                out[(size_t)row * Opad + o] = acc[mi][ni][r];
            }
        }
}

// ============================================================================ depthwise (one input channel per group)
// With C = 1 and O <= 2 per group (kan_mobilenetv2.py:253-255 replace_depthwise) the GEMM tiles above run at 1/128
// utilisation; these direct kernels do the same arithmetic per output element instead.  They are HBM / VALU bound
// (T*P multiply-adds per element), read the SAME packed weights (wp: row k(tap, p), column o, one block per group) and
// write the same slab layouts, so nothing else in the pipeline changes.  One block = 256 elements of one group.
// (DW_MAX_TP, DW_T: kan_internal.h -- the planner routes a layer here only within them)

__device__ __forceinline__ int dw_krow(int tap, int p, int IPC, int KC, int P) {   // packed row of (item = tap, plane p) when C == 1
    const int chunk = tap / IPC;
    return chunk * KC + (tap - chunk * IPC) * P + p;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_dw_fwd(const float* __restrict__ x, const float* __restrict__ xn, const float* __restrict__ wp,
                                                float* __restrict__ z, DevGeom g, DevBasis bs, int Opad, int IPC, int KC, int Kpad) {
    __shared__ float sTab[KAN_MAX_TABLE];
    __shared__ float sWt[DW_MAX_TP * 2];             // [tap*P + p][o]
    const int grp = blockIdx.y, T = g.kh * g.kw, P = bs.P, HoWo = g.Ho * g.Wo, HW = g.H * g.W;
    if (threadIdx.x < KAN_MAX_TABLE) sTab[threadIdx.x] = bs.tab[threadIdx.x];
    for (int i = threadIdx.x; i < T * P * 2; i += 256) {          // (second output slot is zero when the group has one output)
        const int o = i & 1, tp = i >> 1, tap = tp / P, p = tp - tap * P;
        sWt[i] = o < g.O ? wp[((size_t)grp * Kpad + dw_krow(tap, p, IPC, KC, P)) * Opad + o] : 0.f;
    }
    __syncthreads();
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= g.B * HoWo) return;
    const int b = e / HoWo, hw = e - b * HoWo, ho = hw / g.Wo, wo = hw - ho * g.Wo;
    const size_t xbase = (size_t)b * g.xbs + (size_t)grp * HW;
    float acc0 = 0.f, acc1 = 0.f;
    for (int tap = 0; tap < T; ++tap) {
        const int r = tap / g.kw, t = tap - r * g.kw;
        const int hi = ho * g.sh - g.ph + r * g.dh, wi = wo * g.sw - g.pw + t * g.dw;
        if ((unsigned)hi >= (unsigned)g.H || (unsigned)wi >= (unsigned)g.W) continue;      // zero padding of the expanded operand
        const float xa = x[xbase + hi * g.W + wi], xb = xn[xbase + hi * g.W + wi];
        float v[KAN_PMAX];
        kan_planes<KIND, false>(bs, sTab, xa, xb, v);
#pragma unroll
        for (int p = 0; p < KAN_PMAX; ++p)
            if (p < P) { acc0 += v[p] * sWt[(tap * P + p) * 2]; acc1 += v[p] * sWt[(tap * P + p) * 2 + 1]; }
    }
    float* zb = z + (size_t)b * g.ybs + (size_t)grp * g.O * HoWo + hw;
    zb[0] = acc0;
    if (g.O > 1) zb[HoWo] = acc1;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_dw_bwd_data(const float* __restrict__ dz, const float* __restrict__ x, const float* __restrict__ xn,
                                                     const float* __restrict__ wp, float* __restrict__ dx, float* __restrict__ dxn,
                                                     DevGeom g, DevBasis bs, int Opad, int IPC, int KC, int Kpad) {
    __shared__ float sTab[KAN_MAX_TABLE];
    __shared__ float sWt[DW_MAX_TP * 2];
    const int grp = blockIdx.y, T = g.kh * g.kw, P = bs.P, HoWo = g.Ho * g.Wo, HW = g.H * g.W;
    if (threadIdx.x < KAN_MAX_TABLE) sTab[threadIdx.x] = bs.tab[threadIdx.x];
    for (int i = threadIdx.x; i < T * P * 2; i += 256) {          // (second output slot is zero when the group has one output)
        const int o = i & 1, tp = i >> 1, tap = tp / P, p = tp - tap * P;
        sWt[i] = o < g.O ? wp[((size_t)grp * Kpad + dw_krow(tap, p, IPC, KC, P)) * Opad + o] : 0.f;
    }
    __syncthreads();
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= g.B * HW) return;
    const int b = e / HW, hw = e - b * HW, h = hw / g.W, w = hw - h * g.W;
    const size_t xi = (size_t)b * g.xbs + (size_t)grp * HW + hw;
    float G[KAN_PMAX];
#pragma unroll
    for (int p = 0; p < KAN_PMAX; ++p) G[p] = 0.f;
    for (int tap = 0; tap < T; ++tap) {
        const int r = tap / g.kw, t = tap - r * g.kw;
        const int hn = h + g.ph - r * g.dh, wn = w + g.pw - t * g.dw;
        if (hn < 0 || wn < 0) continue;
        const int ho = hn / g.sh, wo = wn / g.sw;
        if (ho * g.sh != hn || wo * g.sw != wn || ho >= g.Ho || wo >= g.Wo) continue;
        const float* zb = dz + (size_t)b * g.ybs + (size_t)grp * g.O * HoWo + ho * g.Wo + wo;
        const float d0 = zb[0], d1 = g.O > 1 ? zb[HoWo] : 0.f;
#pragma unroll
        for (int p = 0; p < KAN_PMAX; ++p)
            if (p < P) G[p] += d0 * sWt[(tap * P + p) * 2] + d1 * sWt[(tap * P + p) * 2 + 1];
    }
    float d[KAN_PMAX];
    kan_planes<KIND, true>(bs, sTab, x[xi], xn[xi], d);
    float s_base = 0.f, s_bas = 0.f;
#pragma unroll
    for (int p = 0; p < KAN_PMAX; ++p)
        if (p < P) { if (p < bs.hb) s_base += d[p] * G[p]; else s_bas += d[p] * G[p]; }
    if (dxn) { dx[xi] = s_base; dxn[xi] = s_bas; }
    else dx[xi] = s_base + s_bas;
}

// Weight gradient: block (chunk, group) walks its share of the group's B*Ho*Wo pixels with one accumulator per (tap, plane)
// in registers (statically indexed: T <= 9, planes padded to KAN_PMAX), one output of the group after the other, reduces
// them over the block in a fixed order and writes slab `chunk`.
template <int KIND>
__global__ __launch_bounds__(256) void k_dw_bwd_weight(const float* __restrict__ dz, const float* __restrict__ x, const float* __restrict__ xn,
                                                       float* __restrict__ dwp, DevGeom g, DevBasis bs, int Krows, int Opad,
                                                       long long slab_elems) {
    __shared__ float sTab[KAN_MAX_TABLE];
    __shared__ float sRed[4][DW_T * KAN_PMAX];
    const int grp = blockIdx.y, T = g.kh * g.kw, P = bs.P, HoWo = g.Ho * g.Wo, HW = g.H * g.W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < KAN_MAX_TABLE) sTab[threadIdx.x] = bs.tab[threadIdx.x];
    __syncthreads();
    float* out = dwp + (size_t)blockIdx.x * slab_elems + (size_t)grp * Krows * Opad;
    const int total = g.B * HoWo;
    for (int o = 0; o < g.O; ++o) {
        float acc[DW_T][KAN_PMAX];
#pragma unroll
        for (int a = 0; a < DW_T; ++a)
#pragma unroll
            for (int p = 0; p < KAN_PMAX; ++p) acc[a][p] = 0.f;
        for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
            const int b = e / HoWo, hw = e - b * HoWo, ho = hw / g.Wo, wo = hw - ho * g.Wo;
            const float dzv = dz[(size_t)b * g.ybs + (size_t)(grp * g.O + o) * HoWo + hw];
            const size_t xbase = (size_t)b * g.xbs + (size_t)grp * HW;
#pragma unroll
            for (int tap = 0; tap < DW_T; ++tap) {
                if (tap < T) {
                    const int r = tap / g.kw, t = tap - r * g.kw;
                    const int hi = ho * g.sh - g.ph + r * g.dh, wi = wo * g.sw - g.pw + t * g.dw;
                    if ((unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)g.W) {
                        float v[KAN_PMAX];
                        kan_planes<KIND, false>(bs, sTab, x[xbase + hi * g.W + wi], xn[xbase + hi * g.W + wi], v);
#pragma unroll
                        for (int p = 0; p < KAN_PMAX; ++p) acc[tap][p] += v[p] * dzv;      // planes >= P are zero
                    }
                }
            }
        }
        // block reduction, fixed order: lanes by xor-shuffle, then the four waves through LDS
#pragma unroll
        for (int a = 0; a < DW_T; ++a)
#pragma unroll
            for (int p = 0; p < KAN_PMAX; ++p) {
                float v = acc[a][p];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
                if (lane == 0) sRed[wave][a * KAN_PMAX + p] = v;
            }
        __syncthreads();
        for (int i = threadIdx.x; i < T * P; i += 256) {
            const int tap = i / P, p = i - tap * P, q = tap * KAN_PMAX + p;
            out[(size_t)i * Opad + o] = (sRed[0][q] + sRed[1][q]) + (sRed[2][q] + sRed[3][q]);
        }
        __syncthreads();
    }
}

// ============================================================================ slab reduce
__global__ __launch_bounds__(256) void k_slab_reduce(const float* __restrict__ slabs, int n_slabs, long long slab_elems,
                                                     float* __restrict__ out, int Cn, int HW, long long bstride, long long total) {
    const long long plane = (long long)Cn * HW;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long b = i / plane, rem = i - b * plane;
        size_t a = (size_t)b * bstride + rem;
        float s = 0.f;
        for (int sl = 0; sl < n_slabs; ++sl) s += slabs[a + (size_t)sl * slab_elems];
        out[a] = s;
    }
}

// ============================================================================ InstanceNorm + PReLU
// G lanes cooperate on one (b, channel) plane; 256/G planes per workgroup.
// Plane statistics are accumulated and combined in DOUBLE, as the reference's CPU path does (ATen's batch-norm CPU kernels
// use at::acc_type<float, false> = double for the sums, the variance, k = dotp * invstd^2 / N and the final
// (dy - mean(dy) - (x - mean) k) * invstd; kan_layers.py:242 -> F.instance_norm -> batch_norm).  It matters where the
// backward cancels: the last KAN-VGG layer receives the gradient of a spatial mean, i.e. dy CONSTANT over each 2x2 plane, so
// dy - mean(dy) is exactly zero and what survives is the small (x - mean) k term; with fp32 sums the bs-256 KAN-VGG11 weight
// gradients were 1e-2 (L2) off the fp64 result where the reference's own fp32 path is 1e-4 off.  These kernels are
// HBM-bound, the fp64 arithmetic is free.  mean / rstd are stored as fp32 (the reference's save_mean / save_invstd are too).
// (group_sum<G>: kan_common.h)

// General MaxPool2d(k, s) (no padding, floor mode: the AlexNet pattern MaxPool2d(3, 2), kan_alexnet.py:38-42) fused behind the PReLU in the generic
// norm kernels: windows overlap, so the backward of an element sums the pooled gradients of the <= ceil(k/s)^2 windows that picked it.  k == 0: not used
// (the even-plane 2x2 path below / in the register kernels).
struct PoolGeo { int k, s, Hp, Wp, nc; FastDiv divWp, divS, divK, divNc; int lds; };      // nc = ceil(k / s): window classes per axis      // lds: the plane (forward) / its pooled gradient + indices (backward) are staged in LDS

template <int G>
__global__ __launch_bounds__(256) void k_in_prelu_fwd(const float* z, int n_slabs, long long slab_elems,     // z_out may alias z (slab 0)
                                                      float* z_out, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ prelu_a,
                                                      float* __restrict__ y, float* __restrict__ mean_o, float* __restrict__ rstd_o,
                                                      int n_planes, int Cn, int HW, long long bstride, float eps, int prelu_span,
                                                      unsigned char* __restrict__ pidx, int W, FastDiv divW, PoolGeo pg) {
    const int tid = threadIdx.x, sub = tid % G;
    const int plane = blockIdx.x * (256 / G) + tid / G;
    const bool act = plane < n_planes;
    const int b = act ? plane / Cn : 0, c = act ? plane - b * Cn : 0;
    const size_t base = (size_t)b * bstride + (size_t)c * HW;
    const bool need_sum = (n_slabs > 1) || (z_out != z);
    double s = 0.0;
    if (act) for (int i = sub; i < HW; i += G) {
        // split-K slabs: four independent partial sums keep four loads in flight (a 32-slab 2x2-plane layer spent its
        // whole time in this dependent chain); fixed order => deterministic
        const float* zp = z + base + i;
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
    const double mu_d = group_sum<G>(s) / (double)HW;
    double q = 0.0;
    if (act) for (int i = sub; i < HW; i += G) { const double d = (double)z_out[base + i] - mu_d; q += d * d; }
    const double var = group_sum<G>(q) / (double)HW;
    const float mu = (float)mu_d, rs = (float)(1.0 / sqrt(var + (double)eps));
    if (!act) return;
    const float ga = gamma ? gamma[c] : 1.f, be = beta ? beta[c] : 0.f;
    const bool has_p = prelu_a != nullptr;
    const float a = has_p ? prelu_a[prelu_span > 0 ? c / prelu_span : 0] : 1.f;     // one slope per `prelu_span` channels (0: one for all)
    if (pidx && pg.k) {
        // general MaxPool2d(k, s): y and pidx are the dense pooled [B][Cn][Hp][Wp] tensors, pidx = dh * k + dw of the maximum (first maximum in
        // scan order, NaN wins: torch's max_pool2d)
        const int Q = pg.Hp * pg.Wp;
        const size_t pbase = (size_t)plane * Q;
        extern __shared__ __attribute__((aligned(16))) unsigned char pool_smem[];
        float* mine = (float*)pool_smem + (size_t)(tid / G) * HW;      // this plane's activated values (pg.lds): every element is normalised once,
        if (pg.lds) {                                                  // every window then reads LDS (was: 9 global reads + 9 normalisations per output)
            for (int i = sub; i < HW; i += G) {
                const float n = (z_out[base + i] - mu) * rs * ga + be;
                mine[i] = (has_p && !(n > 0.f)) ? a * n : n;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // a plane's G lanes sit in one wave: LDS serves a wave's accesses in order
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        for (int q = sub; q < Q; q += G) {
            const int hp = fastdiv(q, pg.divWp), wp = q - hp * pg.Wp, i0 = hp * pg.s * W + wp * pg.s;
            float best = 0.f; int arg = 0; bool first = true;
            for (int dh = 0; dh < pg.k; ++dh)
                for (int dw = 0; dw < pg.k; ++dw) {
                    float v;
                    if (pg.lds) v = mine[i0 + dh * W + dw];
                    else {
                        const float n = (z_out[base + i0 + dh * W + dw] - mu) * rs * ga + be;
                        v = (has_p && !(n > 0.f)) ? a * n : n;
                    }
                    if (first || v > best || v != v) { best = v; arg = dh * pg.k + dw; first = false; }
                }
            y[pbase + q] = best; pidx[pbase + q] = (unsigned char)arg;
        }
    } else if (pidx) {
        // fused MaxPool2d(2, 2) (the VGG pattern: kan_vgg.py:97-101 puts one right after the layer): y and pidx are the dense
        // pooled [B][Cn][H/2][W/2] tensors, pidx the position 2*dh + dw of the maximum -- first maximum in scan order, NaN wins,
        // as torch's max_pool2d picks it.  The full-size activation is never written.
        const int W2 = W >> 1, Q = HW >> 2;
        const size_t pbase = (size_t)plane * Q;
        for (int q = sub; q < Q; q += G) {
            const int h2 = fastdiv(q, divW), w2 = q - h2 * W2, i0 = 2 * h2 * W + 2 * w2;      // divW: by W / 2 here
            float best = 0.f; int arg = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float n = (z_out[base + i0 + (k >> 1) * W + (k & 1)] - mu) * rs * ga + be;
                const float v = (has_p && !(n > 0.f)) ? a * n : n;
                if (k == 0 || v > best || v != v) { best = v; arg = k; }
            }
            y[pbase + q] = best; pidx[pbase + q] = (unsigned char)arg;
        }
    } else {
        for (int i = sub; i < HW; i += G) {
            float n = (z_out[base + i] - mu) * rs * ga + be;
            y[base + i] = (has_p && !(n > 0.f)) ? a * n : n;
        }
    }
    if (sub == 0) { mean_o[plane] = mu; rstd_o[plane] = rs; }
}

constexpr int IN_BWD_HELD = 16;      // elements per lane k_in_prelu_bwd can hold in registers between its two passes (norm_route: `held`)

template <int G>
__global__ __launch_bounds__(256) void k_in_prelu_bwd(const float* __restrict__ dy, const float* __restrict__ z,
                                                      const float* __restrict__ mean_i, const float* __restrict__ rstd_i,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ prelu_a, float* __restrict__ dz,
                                                      float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dprelu,
                                                      int n_planes, int Cn, int HW, long long bstride, int prelu_span,
                                                      const unsigned char* __restrict__ pidx, int W, FastDiv divW, PoolGeo pool) {
    constexpr int EPL = IN_BWD_HELD;                // elements per lane held in registers between the two passes
    __shared__ double s_da[256 / G];
    const int tid = threadIdx.x, sub = tid % G;
    const bool has_p = prelu_a != nullptr;
    const bool in_regs = HW <= G * EPL;             // uniform
    double sa_total = 0.0;                          // PReLU-slope gradient of every plane this workgroup visits
    // grid-stride over groups of 256/G planes: the grid is capped so that the single-address atomic on dprelu
    // (one per workgroup) stays cheap -- 16 k workgroups hammering one word cost 190 us
    for (int pg = blockIdx.x; pg * (256 / G) < n_planes; pg += gridDim.x) {
    const int plane = pg * (256 / G) + tid / G;
    const bool act = plane < n_planes;
    const int b = act ? plane / Cn : 0, c = act ? plane - b * Cn : 0;
    const size_t base = (size_t)b * bstride + (size_t)c * HW;
    const float mu = act ? mean_i[plane] : 0.f, rs = act ? rstd_i[plane] : 0.f;
    const float ga = gamma ? gamma[c] : 1.f, be = beta ? beta[c] : 0.f;
    const float a = has_p ? prelu_a[prelu_span > 0 ? c / prelu_span : 0] : 1.f;
    float rc[EPL], rd[EPL];                         // centred value z - mean, d loss / d normalised value
    double s1 = 0.0, s2 = 0.0, sa = 0.0, sg = 0.0, sb = 0.0;
    extern __shared__ __attribute__((aligned(16))) unsigned char pool_smem[];
    const int poolQ = pool.k ? pool.Hp * pool.Wp : 0;
    float* gbuf = (float*)pool_smem + (size_t)(tid / G) * HW;      // pool.lds: this plane's UN-POOLED upstream gradient, built in LDS
    if (pool.k && pool.lds) {
        // Scatter of the pooled gradient without atomics and in a fixed order: windows whose (row, column) indices agree modulo nc = ceil(k / s)
        // are >= k apart and never share an element, so each of the nc^2 classes is a conflict-free pass of read-modify-writes; the classes run
        // one after the other (a plane's G lanes sit in one wave, and LDS serves a wave's accesses in order).  The passes below then read gbuf[i].
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // (the previous plane's reads of gbuf are done)
        __builtin_amdgcn_wave_barrier();
        if (act) for (int i = sub; i < HW; i += G) gbuf[i] = 0.f;
        const int nc = pool.nc;
        for (int cls = 0; cls < nc * nc; ++cls) {
            const int ch = cls / nc, cw = cls - ch * nc;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (act) for (int q = sub; q < poolQ; q += G) {
                const int hp = fastdiv(q, pool.divWp), wp = q - hp * pool.Wp;
                if (hp - fastdiv(hp, pool.divNc) * nc != ch || wp - fastdiv(wp, pool.divNc) * nc != cw) continue;
                const int arg = pidx[(size_t)plane * poolQ + q], dh = fastdiv(arg, pool.divK), dw = arg - dh * pool.k;
                gbuf[(hp * pool.s + dh) * W + wp * pool.s + dw] += dy[(size_t)plane * poolQ + q];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // upstream gradient of element i: plain, or through the fused MaxPool2d(2, 2) -- dy is then the dense pooled gradient and
    // only the element the forward marked in pidx receives it
    auto gy = [&](int i) -> float {
        if (!pidx) return dy[base + i];
        if (pool.k && pool.lds) return gbuf[i];
        const int h = fastdiv(i, divW), w = i - h * W;
        if (pool.k) {                                  // general MaxPool2d(k, s), plane too large for LDS: every window holding (h, w) whose maximum this element was
            const int k = pool.k, st = pool.s;
            const int hp1 = min(fastdiv(h, pool.divS), pool.Hp - 1), wp1 = min(fastdiv(w, pool.divS), pool.Wp - 1);
            const int hp0 = h >= k ? fastdiv(h - k + st, pool.divS) : 0, wp0 = w >= k ? fastdiv(w - k + st, pool.divS) : 0;
            float gsum = 0.f;
            for (int hp = hp0; hp <= hp1; ++hp)
                for (int wp = wp0; wp <= wp1; ++wp) {
                    const int dh = h - hp * st, dw = w - wp * st;
                    if (dh >= k || dw >= k) continue;
                    const size_t pq = (size_t)plane * poolQ + (size_t)(hp * pool.Wp + wp);
                    if (pidx[pq] == (unsigned char)(dh * k + dw)) gsum += dy[pq];
                }
            return gsum;
        }
        const size_t pq = (size_t)plane * (HW >> 2) + (size_t)((h >> 1) * (W >> 1) + (w >> 1));
        return pidx[pq] == (unsigned char)((h & 1) * 2 + (w & 1)) ? dy[pq] : 0.f;
    };
    // s1 = sum d,  s2 = sum d (z - mean)  with d = dL/d(normalised value): ATen's `sum` and `dotp`
    auto visit = [&](float zv, float g, float& zc, float& dnh) {
        zc = zv - mu;
        const float nh = zc * rs;
        const float n = nh * ga + be;
        const bool neg = has_p && !(n > 0.f);
        const float dn = neg ? a * g : g;
        if (neg) sa += (double)n * (double)g;
        sb += (double)dn; sg += (double)dn * (double)nh;
        dnh = dn * ga;
        s1 += (double)dnh; s2 += (double)dnh * (double)zc;
    };
    if (in_regs) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int i = sub + e * G;
            rc[e] = 0.f; rd[e] = 0.f;
            if (act && i < HW) visit(z[base + i], gy(i), rc[e], rd[e]);
        }
    } else if (act) {
        for (int i = sub; i < HW; i += G) { float zc, dnh; visit(z[base + i], gy(i), zc, dnh); }
    }
    s1 = group_sum<G>(s1); s2 = group_sum<G>(s2);
    sa = group_sum<G>(sa); sg = group_sum<G>(sg); sb = group_sum<G>(sb);
    const double rs_d = (double)rs;
    const double gm = s1 / (double)HW, kk = s2 * rs_d * rs_d / (double)HW;      // grad_mean and k of ATen's batch_norm_backward_cpu
    if (in_regs) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int i = sub + e * G;
            if (act && i < HW) dz[base + i] = (float)((((double)rd[e] - gm) - (double)rc[e] * kk) * rs_d);
        }
    } else if (act) {
        for (int i = sub; i < HW; i += G) {
            const float zc = z[base + i] - mu;
            const float n = zc * rs * ga + be;
            const float g = gy(i);
            const bool neg = has_p && !(n > 0.f);
            const float dnh = (neg ? a * g : g) * ga;
            dz[base + i] = (float)((((double)dnh - gm) - (double)zc * kk) * rs_d);
        }
    }
    if (act && sub == 0) {
        if (dgamma) atomicAdd(&dgamma[c], (float)sg);
        if (dbeta) atomicAdd(&dbeta[c], (float)sb);
        if (prelu_span > 0) { if (dprelu) atomicAdd(&dprelu[c / prelu_span], (float)sa); }      // per-group slopes (grouped layers)
        else sa_total += sa;
    }
    }                                               // grid-stride loop
    if (dprelu && prelu_span <= 0) {                // one atomic per workgroup
        if (sub == 0) s_da[tid / G] = sa_total;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int i = 0; i < 256 / G; ++i) t += s_da[i];
            atomicAdd(dprelu, (float)t);
        }
    }
}

// Register-resident forward for planes of <= 16 G elements: one read of the slabs, statistics and the normalised output from
// registers (k_in_prelu_fwd reads the summed plane three times and keeps one plane group in flight: 0.5 - 1 TB/s on the
// 8x8 layers).  Loads are unconditional on clamped indices, PPI plane groups per iteration.
//   POOL = false: lane `sub` of a plane holds elements sub + e G.
//   POOL = true : lane `sub` holds the 2x2 windows sub + w G (EPL = 4 windows-per-lane elements, two float2 loads per window),
//                 so that the fused MaxPool2d(2, 2) needs no neighbour exchange.  W, H even (checked on the host).
template <int G, int EPL, int PPI, bool POOL, int NT>
__global__ __launch_bounds__(NT) void k_in_prelu_fwd_regs(const float* z, int n_slabs, long long slab_elems, float* z_out,     // z_out may alias z (slab 0)
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const float* __restrict__ prelu_a, float* __restrict__ y,
                                                          float* __restrict__ mean_o, float* __restrict__ rstd_o, int n_planes, int Cn, int HW,
                                                          long long bstride, float eps, int prelu_span, unsigned char* __restrict__ pidx, int W,
                                                          FastDiv divW2) {
    constexpr int PPB = NT / G, WPL = EPL / 4;
    static_assert(!POOL || EPL % 4 == 0, "pooled variant: whole windows per lane");
    const int tid = threadIdx.x, sub = tid % G, pin = tid / G;
    const bool need_sum = (n_slabs > 1) || (z_out != z), has_p = prelu_a != nullptr;
    const int n_groups = (n_planes + PPB - 1) / PPB, W2 = W >> 1, NWIN = HW >> 2;
    for (int pg0 = blockIdx.x * PPI; pg0 < n_groups; pg0 += gridDim.x * PPI) {
        float v[PPI][EPL]; int eo[EPL]; bool eok[EPL];
        size_t base[PPI]; int ch[PPI], pln[PPI]; bool act[PPI];
        // element offsets inside a plane (the same for every plane group)
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            if (POOL) {
                const int win = sub + (e >> 2) * G, wc = win < NWIN ? win : 0, h2 = fastdiv(wc, divW2), w2 = wc - h2 * W2;
                eo[e] = (2 * h2 + ((e >> 1) & 1)) * W + 2 * w2 + (e & 1);
                eok[e] = win < NWIN;
            } else {
                const int i = sub + e * G;
                eo[e] = i < HW ? i : 0; eok[e] = i < HW;
            }
        }
#pragma unroll
        for (int q = 0; q < PPI; ++q) {
            const int plane = (pg0 + q) * PPB + pin;
            act[q] = plane < n_planes;
            pln[q] = act[q] ? plane : 0;
            const int b = pln[q] / Cn; ch[q] = pln[q] - b * Cn;
            base[q] = (size_t)b * bstride + (size_t)ch[q] * HW;
#pragma unroll
            for (int e = 0; e < EPL; ++e) v[q][e] = 0.f;
        }
        for (int sl = 0; sl < n_slabs; ++sl) {               // fixed order => deterministic
            const float* zs = z + (size_t)sl * slab_elems;
#pragma unroll
            for (int q = 0; q < PPI; ++q) {
                if (POOL) {
#pragma unroll
                    for (int e = 0; e < EPL; e += 2) {
                        const float2 t = *reinterpret_cast<const float2*>(zs + base[q] + eo[e]);
                        v[q][e] += t.x; v[q][e + 1] += t.y;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < EPL; ++e) v[q][e] += zs[base[q] + eo[e]];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < PPI; ++q) {
            double s = 0.0;
#pragma unroll
            for (int e = 0; e < EPL; ++e) s += (act[q] && eok[e]) ? (double)v[q][e] : 0.0;
            const double mu_d = group_sum<G>(s) / (double)HW;
            double qq = 0.0;
#pragma unroll
            for (int e = 0; e < EPL; ++e) { const double d = (double)v[q][e] - mu_d; qq += (act[q] && eok[e]) ? d * d : 0.0; }
            const double var = group_sum<G>(qq) / (double)HW;
            const float mu = (float)mu_d, rs = (float)(1.0 / sqrt(var + (double)eps));
            const float ga = gamma ? gamma[ch[q]] : 1.f, be = beta ? beta[ch[q]] : 0.f;
            const float a = has_p ? prelu_a[prelu_span > 0 ? ch[q] / prelu_span : 0] : 1.f;
            if (!act[q]) continue;
            if (need_sum) {
                if (POOL) {
#pragma unroll
                    for (int e = 0; e < EPL; e += 2)
                        if (eok[e]) *reinterpret_cast<float2*>(z_out + base[q] + eo[e]) = make_float2(v[q][e], v[q][e + 1]);
                } else {
#pragma unroll
                    for (int e = 0; e < EPL; ++e) if (eok[e]) z_out[base[q] + eo[e]] = v[q][e];
                }
            }
            if (POOL) {
#pragma unroll
                for (int w = 0; w < WPL; ++w) {
                    const int win = sub + w * G;
                    if (win >= NWIN) continue;
                    float best = 0.f; int arg = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {                       // scan order (0,0) (0,1) (1,0) (1,1): first maximum wins, NaN wins
                        const float n = (v[q][4 * w + k] - mu) * rs * ga + be;
                        const float val = (has_p && !(n > 0.f)) ? a * n : n;
                        if (k == 0 || val > best || val != val) { best = val; arg = k; }
                    }
                    const size_t po = (size_t)pln[q] * NWIN + win;
                    y[po] = best; pidx[po] = (unsigned char)arg;
                }
            } else {
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    if (!eok[e]) continue;
                    const float n = (v[q][e] - mu) * rs * ga + be;
                    y[base[q] + eo[e]] = (has_p && !(n > 0.f)) ? a * n : n;
                }
            }
            if (sub == 0) { mean_o[pln[q]] = mu; rstd_o[pln[q]] = rs; }
        }
    }
}

// Register-resident backward for planes of <= 16 G elements: G lanes per plane, EPL elements per lane, PPI plane groups per
// loop iteration.  Every load of an iteration is issued up front, unconditionally and on clamped indices (hipcc puts an
// `s_waitcnt vmcnt(0)` behind each load it has to branch around; the first version of this kernel, one plane group per
// iteration with guarded loads and a grid capped for the slope atomics, ran at 0.5 - 1.5 TB/s), so that a wave keeps
// PPI * EPL * 2 loads in flight.  Same arithmetic, in the same order per plane, as k_in_prelu_bwd.  NT = 1024 threads per
// workgroup where the registers allow: the PReLU-slope gradient costs one same-address atomic per workgroup (~12 ns each,
// serialised in L2 -- 2048 workgroups set a 25 us floor under the 8x8 ... 2x2 layers), so fewer, fatter workgroups.
template <int G, int EPL, int PPI, bool POOL, int NT>
__global__ __launch_bounds__(NT) void k_in_prelu_bwd_regs(const float* __restrict__ dy, const float* __restrict__ z,
                                                           const float* __restrict__ mean_i, const float* __restrict__ rstd_i,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ prelu_a, float* __restrict__ dz,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dprelu,
                                                           int n_planes, int Cn, int HW, long long bstride, int prelu_span,
                                                           const unsigned char* __restrict__ pidx, int W, FastDiv divW) {
    constexpr int PPB = NT / G;
    __shared__ double s_da[PPB];
    const int tid = threadIdx.x, sub = tid % G, pin = tid / G;
    const bool has_p = prelu_a != nullptr, affine = dgamma != nullptr || dbeta != nullptr;
    const int n_groups = (n_planes + PPB - 1) / PPB;
    double sa_total = 0.0;
    for (int pg0 = blockIdx.x * PPI; pg0 < n_groups; pg0 += gridDim.x * PPI) {
        float zr[PPI][EPL], gr[PPI][EPL], mu[PPI], rs[PPI]; unsigned char pk[PPI][EPL];
        size_t base[PPI]; int ch[PPI]; bool act[PPI];
#pragma unroll
        for (int q = 0; q < PPI; ++q) {
            const int plane = (pg0 + q) * PPB + pin;
            act[q] = plane < n_planes;
            const int pl = act[q] ? plane : 0;
            const int b = pl / Cn; ch[q] = pl - b * Cn;
            base[q] = (size_t)b * bstride + (size_t)ch[q] * HW;
            mu[q] = mean_i[pl]; rs[q] = rstd_i[pl];
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const int i = sub + e * G, ic = i < HW ? i : 0;
                zr[q][e] = z[base[q] + ic];
                if (POOL) {
                    const int h = fastdiv(ic, divW), w = ic - h * W;
                    const size_t pq = (size_t)pl * (HW >> 2) + (size_t)((h >> 1) * (W >> 1) + (w >> 1));
                    pk[q][e] = pidx[pq]; gr[q][e] = dy[pq];
                } else {
                    pk[q][e] = 0; gr[q][e] = dy[base[q] + ic];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < PPI; ++q) {
            const float ga = gamma ? gamma[ch[q]] : 1.f, be = beta ? beta[ch[q]] : 0.f;
            const float a = has_p ? prelu_a[prelu_span > 0 ? ch[q] / prelu_span : 0] : 1.f;
            float zc[EPL], dnh[EPL];
            double s1 = 0.0, s2 = 0.0, sa = 0.0, sg = 0.0, sb = 0.0;
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const int i = sub + e * G;
                const bool ok = act[q] && i < HW;
                float g = gr[q][e];
                if (POOL) {                                   // only the element the forward marked receives the pooled gradient
                    const int h = fastdiv(i < HW ? i : 0, divW), w = (i < HW ? i : 0) - h * W;
                    g = pk[q][e] == (unsigned char)((h & 1) * 2 + (w & 1)) ? g : 0.f;
                }
                g = ok ? g : 0.f;
                zc[e] = ok ? zr[q][e] - mu[q] : 0.f;
                const float nh = zc[e] * rs[q], n = nh * ga + be;
                const bool neg = has_p && !(n > 0.f);
                const float dn = neg ? a * g : g;
                if (neg) sa += (double)n * (double)g;
                if (affine) { sb += (double)dn; sg += (double)dn * (double)nh; }
                dnh[e] = dn * ga;
                s1 += (double)dnh[e]; s2 += (double)dnh[e] * (double)zc[e];
            }
            s1 = group_sum<G>(s1); s2 = group_sum<G>(s2);
            if (has_p) sa = group_sum<G>(sa);
            if (affine) { sg = group_sum<G>(sg); sb = group_sum<G>(sb); }
            const double rs_d = (double)rs[q];
            const double gm = s1 / (double)HW, kk = s2 * rs_d * rs_d / (double)HW;
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const int i = sub + e * G;
                if (act[q] && i < HW) dz[base[q] + i] = (float)((((double)dnh[e] - gm) - (double)zc[e] * kk) * rs_d);
            }
            if (act[q] && sub == 0) {
                if (dgamma) atomicAdd(&dgamma[ch[q]], (float)sg);
                if (dbeta) atomicAdd(&dbeta[ch[q]], (float)sb);
                if (prelu_span > 0) { if (dprelu) atomicAdd(&dprelu[ch[q] / prelu_span], (float)sa); }
                else sa_total += sa;
            }
        }
    }
    if (dprelu && prelu_span <= 0) {                // one atomic per workgroup
        if (sub == 0) s_da[pin] = sa_total;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int i = 0; i < PPB; ++i) t += s_da[i];
            atomicAdd(dprelu, (float)t);
        }
    }
}

// ============================================================================ host side

int launch_ok(const char* what) {
    hipError_t e = hipGetLastError();
    (void)what;
    if (e != hipSuccess) { fail("launch failed: %s", hipGetErrorString(e)); return -2; }
    return 0;
}

// Layout of the packed weights (wp, flat == false) or of the packed weight gradient (flat == true) the plan's routes read / write.
PackGeo pack_geo(const KanGeom* g, const KanBasis* b, const ConvPlan& cp, bool flat) {
    const KanPlan& pl = cp.pub;
    PackGeo q;
    q.O = g->O; q.C = g->C; q.T = g->kh * g->kw; q.P = pl.P; q.hb = b->act != KAN_ACT_NONE; q.nb = b->n_basis;
    q.IPC = flat ? 1 : pl.IPC; q.KC = flat ? pl.P : pl.KC; q.Opad = pl.Opad;
    q.pair = (!flat && cp.fwd == Route::HALO) ? 1 : 0;
    q.cmajor = (flat && cp.bwd_weight == Route::HALO) ? 1 : 0;
    q.band = (flat ? cp.bwd_weight : cp.fwd) == Route::BAND ? 1 : 0;
    if (q.band) {                                     // (the flat gradient of a band layer has the forward's rows, pad rows included)
        q.IPC = pl.IPC; q.KC = pl.KC;
        for (int i = 0; i < q.T; ++i) { q.tap_step[i] = cp.band.tap_step[i]; q.tap_nt[i] = cp.band.tap_nt[i]; }
    }
    q.divT = make_fastdiv(q.T); q.divNb = make_fastdiv(q.nb); q.divIPC = make_fastdiv(q.IPC); q.divP = make_fastdiv(q.P);
    return q;
}

// XCD-balanced order of the position-major pixel tiles, weighted by their live work
template <class Weight>
TilePerm tile_perm(int tiles_p, Weight weight) {
    TilePerm perm; perm.n = 0;
    if (tiles_p > PERM_MAX) return perm;
    int w[PERM_MAX];
    for (int t = 0; t < tiles_p; ++t) w[t] = weight(t);
    perm.n = balance_tiles(w, tiles_p, perm.idx);
    return perm;
}

// ---------------------------------------------------------------------------- InstanceNorm (+ PReLU, + max-pool): route and launchers
// Every threshold of the norm dispatch lives in the tables and in norm_route() below; the launchers take the launch shape from the route.
// Register-resident variants X(limit, G, EPL, PPI): the first row whose limit covers the plane (pixels; windows for the pooled forward).
#define KAN_IN_REGS_PLAIN(X) X(4, 4, 1, 4) X(8, 8, 1, 4) X(16, 16, 1, 4) X(32, 32, 1, 4) \
    X(64, 16, 4, 2)      /* (8x8 planes: 4 elements per lane, measured 52 -> 37 us on 256x256x8x8) */ \
    X(128, 64, 2, 2) X(256, 64, 4, 2) X(512, 64, 8, 1) X(1024, 64, 16, 1)
#define KAN_IN_REGS_POOL2(X) X(4, 4, 4, 2) X(8, 8, 4, 2) X(16, 16, 4, 2) X(32, 32, 4, 2) X(64, 64, 4, 2) X(128, 64, 8, 1) X(256, 64, 16, 1)
#define KAN_IN_GENERIC(X) X(4) X(8) X(16) X(32) X(64)
struct NormVariant { int limit, G, EPL, PPI; };
#define KAN_IN_ROW(LIM, G, EPL, PPI) {LIM, G, EPL, PPI},
constexpr NormVariant IN_REGS_PLAIN[] = {KAN_IN_REGS_PLAIN(KAN_IN_ROW)};
constexpr NormVariant IN_REGS_POOL2[] = {KAN_IN_REGS_POOL2(KAN_IN_ROW)};
#undef KAN_IN_ROW
template <int N> constexpr int last_limit(const NormVariant (&t)[N]) { return t[N - 1].limit; }
constexpr int IN_REGS_MAX_HW = last_limit(IN_REGS_PLAIN);      // the largest plane the register kernels take
static_assert(4 * last_limit(IN_REGS_POOL2) == IN_REGS_MAX_HW, "the windowed table ends at the same plane (4 pixels per window)");

// The compile-time side of the same tables: pick_*(route, f) calls f(NormPick<G, EPL, PPI>{}) for the row the route names (false: no such row).
template <int G_, int EPL_ = 0, int PPI_ = 0> struct NormPick { static constexpr int G = G_, EPL = EPL_, PPI = PPI_; };
#define KAN_IN_PICK(LIM, G_, EPL_, PPI_) if (r.G == G_ && r.EPL == EPL_ && r.PPI == PPI_) { f(NormPick<G_, EPL_, PPI_>{}); return true; }
#define KAN_IN_PICK_G(G_) if (r.G == G_) { f(NormPick<G_>{}); return true; }
template <class F> bool pick_regs_plain(const KanNormRoute& r, F&& f) { KAN_IN_REGS_PLAIN(KAN_IN_PICK) return false; }
template <class F> bool pick_regs_pool2(const KanNormRoute& r, F&& f) { KAN_IN_REGS_POOL2(KAN_IN_PICK) return false; }
template <class F> bool pick_generic(const KanNormRoute& r, F&& f) { KAN_IN_GENERIC(KAN_IN_PICK_G) return false; }
#undef KAN_IN_PICK
#undef KAN_IN_PICK_G
constexpr int IN_FWD_REGS_NT = 256, IN_FWD_REGS_CAP = 8192;
constexpr int in_bwd_regs_nt(int EPL, int PPI) { return EPL * PPI <= 8 ? 1024 : 256; }      // (<= 128 VGPRs needed for 1024 threads)
constexpr int in_bwd_regs_cap(int NT) { return 512 * (1024 / NT); }
constexpr int IN_POOL_LDS_BYTES = 48 * 1024;
constexpr int IN_POOL_PER_LANE = 12;            // generic kernels under a general pool: ~12 elements per lane, more planes per workgroup

// Lanes per (b, channel) plane.
int group_lanes(int HW) {          // (more elements per lane was measured: no gain)
    int g = 4;
    while (g < 64 && g < HW) g <<= 1;
    return g;
}

// The one decision: `pool` is a KAN_NORM_POOL_* mode, `float2_ok` what the pooled register forward needs of its pointers and strides.
KanNormRoute norm_route(bool bwd, int planes, int HW, int pool, bool float2_ok) {
    KanNormRoute r{};
    r.pool = pool;
    const bool regs = HW <= IN_REGS_MAX_HW && (bwd ? pool != KAN_NORM_POOL_K : pool == KAN_NORM_POOL_NONE || (pool == KAN_NORM_POOL_2X2 && float2_ok));
    if (regs) {
        const bool windows = !bwd && pool == KAN_NORM_POOL_2X2;       // lanes own 2x2 windows (float2 accesses)
        const NormVariant* v = windows ? IN_REGS_POOL2 : IN_REGS_PLAIN;
        const int n = windows ? HW / 4 : HW;
        while (n > v->limit) ++v;
        r.kernel = KAN_NORM_REGS; r.G = v->G; r.EPL = v->EPL; r.PPI = v->PPI;
        r.NT = bwd ? in_bwd_regs_nt(v->EPL, v->PPI) : IN_FWD_REGS_NT;
        const int cap = bwd ? in_bwd_regs_cap(r.NT) : IN_FWD_REGS_CAP;
        const int want = ceil_div(ceil_div(planes, r.NT / r.G), r.PPI);
        r.blocks = want < cap ? want : cap;
        r.strided = want > r.blocks;
        return r;
    }
    r.kernel = KAN_NORM_GENERIC; r.NT = 256;
    r.G = group_lanes(pool == KAN_NORM_POOL_K ? ceil_div(HW, IN_POOL_PER_LANE) : HW);
    const int ppb = r.NT / r.G, want = ceil_div(planes, ppb);
    r.lds = pool == KAN_NORM_POOL_K && (size_t)ppb * HW * 4 <= (size_t)IN_POOL_LDS_BYTES;
    r.blocks = want;
    if (bwd) {
        r.held = HW <= r.G * IN_BWD_HELD;
        const int cap = (long long)planes * HW < (4ll << 20) ? 512 : 2048;       // small tensors: fewer same-address atomics on dprelu
        if (r.blocks > cap) r.blocks = cap;
    }
    r.strided = want > r.blocks;
    return r;
}

template <int G>
void launch_in_fwd(hipStream_t st, const KanNormRoute& r, int planes, const float* z, int n_slabs, long long slab_elems, float* z_out,
                   const float* gamma, const float* beta, const float* a, float* y, float* mean, float* rstd, int Cn, int HW, long long bs,
                   float eps, int span, unsigned char* pidx, int W, PoolGeo pg) {
    pg.lds = r.lds;
    hipLaunchKernelGGL((k_in_prelu_fwd<G>), dim3(r.blocks), dim3(256), r.lds ? (size_t)(256 / G) * HW * 4 : 0, st, z, n_slabs, slab_elems, z_out, gamma,
                       beta, a, y, mean, rstd, planes, Cn, HW, bs, eps, span, pidx, W, make_fastdiv(W > 1 ? W / 2 : 1), pg);
}
template <int G>
void launch_in_bwd(hipStream_t st, const KanNormRoute& r, int planes, const float* dy, const float* z, const float* mean, const float* rstd,
                   const float* gamma, const float* beta, const float* a, float* dz, float* dgamma, float* dbeta, float* dprelu, int Cn, int HW,
                   long long bs, int span, const unsigned char* pidx, int W, PoolGeo pg) {
    pg.lds = r.lds;
    hipLaunchKernelGGL((k_in_prelu_bwd<G>), dim3(r.blocks), dim3(256), r.lds ? (size_t)(256 / G) * HW * 4 : 0, st, dy, z, mean, rstd, gamma, beta, a, dz,
                       dgamma, dbeta, dprelu, planes, Cn, HW, bs, span, pidx, W, make_fastdiv(W > 0 ? W : 1), pg);
}
template <int G, int EPL, int PPI, bool POOL>
void launch_in_fwd_regs(hipStream_t st, const KanNormRoute& r, int planes, const float* z, int n_slabs, long long slab_elems, float* z_out,
                        const float* gamma, const float* beta, const float* a, float* y, float* mean, float* rstd, int Cn, int HW, long long bs,
                        float eps, int span, unsigned char* pidx, int W) {
    constexpr int NT = IN_FWD_REGS_NT;
    hipLaunchKernelGGL((k_in_prelu_fwd_regs<G, EPL, PPI, POOL, NT>), dim3(r.blocks), dim3(NT), 0, st, z, n_slabs, slab_elems, z_out, gamma, beta, a, y,
                       mean, rstd, planes, Cn, HW, bs, eps, span, pidx, W, make_fastdiv(W > 1 ? W / 2 : 1));
}
template <int G, int EPL, int PPI>
void launch_in_bwd_regs(hipStream_t st, const KanNormRoute& r, int planes, const float* dy, const float* z, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, const float* a, float* dz, float* dgamma, float* dbeta, float* dprelu, int Cn,
                        int HW, long long bs, int span, const unsigned char* pidx, int W) {
    constexpr int NT = in_bwd_regs_nt(EPL, PPI);
    const FastDiv dw = make_fastdiv(W > 0 ? W : 1);
    if (pidx) hipLaunchKernelGGL((k_in_prelu_bwd_regs<G, EPL, PPI, true, NT>), dim3(r.blocks), dim3(NT), 0, st, dy, z, mean, rstd, gamma, beta, a, dz,
                                 dgamma, dbeta, dprelu, planes, Cn, HW, bs, span, pidx, W, dw);
    else hipLaunchKernelGGL((k_in_prelu_bwd_regs<G, EPL, PPI, false, NT>), dim3(r.blocks), dim3(NT), 0, st, dy, z, mean, rstd, gamma, beta, a, dz,
                            dgamma, dbeta, dprelu, planes, Cn, HW, bs, span, pidx, W, dw);
}

// ============================================================================ optimizer step
// AdamW over one flat fp32 block (generic_train.py:24 optim.AdamW(lr, weight_decay); formulas and their order as
// torch/optim/adamw.py's single-tensor path):  p *= 1 - lr wd;  m = lerp(m, g, 1 - b1);  v = v b2 + (1 - b2) g g;
// p += -(lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps)).  The lerp has ATen's two branches (one per launch): m + (g - m)(1 - b1) for a
// weight 1 - b1 < 0.5, g - (g - m) b1 from 0.5 on.  The first form alone leaves m an absolute error of one ulp of the OLD m, which at
// beta1 = 0 (m must equal g) and |g| << |m| is many times |g|.  Every scalar is formed in double on the host and rounded once; the
// bias correction multiplies by 1 / sqrt(bc2) where torch divides by sqrt(bc2).  Pure HBM traffic: 16 B read + 12 B written per
// element, so the kernel is float4 loads/stores over a grid-stride loop with correctly rounded sqrt / divide (free at this intensity).
struct AdamArgs { float decay, w1, b1, b2, w2, gscale, inv_bc2_sqrt, eps, neg_step; };

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const AdamArgs& a) {
    g *= a.gscale;
    p *= a.decay;
    const float d = g - m;
    m = a.w1 < 0.5f ? m + d * a.w1 : g - d * a.b1;
    v = v * a.b2 + a.w2 * g * g;
    const float denom = sqrtf(v) * a.inv_bc2_sqrt + a.eps;
    p += a.neg_step * (m / denom);
}

__global__ __launch_bounds__(256) void k_adamw(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, long long n, AdamArgs a) {
    const long long n4 = n >> 2;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 P = ((float4*)p)[i], G = ((const float4*)g)[i], M = ((float4*)m)[i], V = ((float4*)v)[i];
        adam1(P.x, G.x, M.x, V.x, a); adam1(P.y, G.y, M.y, V.y, a); adam1(P.z, G.z, M.z, V.z, a); adam1(P.w, G.w, M.w, V.w, a);
        ((float4*)p)[i] = P; ((float4*)m)[i] = M; ((float4*)v)[i] = V;
    }
    const long long t = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x;      // < 4 tail elements
    if (t < n) adam1(p[t], g[t], m[t], v[t], a);
}

// The same update over SEGMENTS of the flat block whose gradients live wherever autograd (or the all-reduce bucket) left
// them: workgroup b owns chunk b = elements [start, start + chunk) of segment chunk_seg[b]; a segment whose gradient
// pointer is null is skipped, as torch skips parameters without .grad.  Nothing is copied or zeroed per step.
// DEV_SCALE (the _clip entry points): grad_scale is read from scale_dev[0], the clip coefficient k_grad_norm_finish (kan_clip.hip) left in device
// memory; without it the pointer is not touched and the kernel is the one it was.
template <bool DEV_SCALE>
__global__ __launch_bounds__(256) void k_adamw_seg(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                   const unsigned long long* __restrict__ seg_grad, const long long* __restrict__ seg_off,
                                                   const int* __restrict__ seg_n, const int* __restrict__ chunk_seg,
                                                   const int* __restrict__ chunk_start, const float* __restrict__ seg_bias, int chunk,
                                                   AdamArgs a, const float* __restrict__ scale_dev) {
    const int sg = chunk_seg[blockIdx.x], start = chunk_start[blockIdx.x];
    const float* g = (const float*)seg_grad[sg];
    if (!g) return;
    if (DEV_SCALE) a.gscale = scale_dev[0];
    if (seg_bias) { a.neg_step = seg_bias[2 * sg]; a.inv_bc2_sqrt = seg_bias[2 * sg + 1]; }     // per-parameter step counts
    const int n = min(chunk, seg_n[sg] - start);
    const long long off = seg_off[sg] + start;
    p += off; m += off; v += off; g += start;
    if ((((uintptr_t)g) & 15u) == 0) {                          // p / m / v chunks are 16-byte aligned by construction
        for (int i = threadIdx.x; i < (n >> 2); i += 256) {
            float4 P = ((float4*)p)[i], G = ((const float4*)g)[i], M = ((float4*)m)[i], V = ((float4*)v)[i];
            adam1(P.x, G.x, M.x, V.x, a); adam1(P.y, G.y, M.y, V.y, a); adam1(P.z, G.z, M.z, V.z, a); adam1(P.w, G.w, M.w, V.w, a);
            ((float4*)p)[i] = P; ((float4*)m)[i] = M; ((float4*)v)[i] = V;
        }
        const int t = (n & ~3) + threadIdx.x;
        if (t < n) adam1(p[t], g[t], m[t], v[t], a);
    } else {
        for (int i = threadIdx.x; i < n; i += 256) adam1(p[i], g[i], m[i], v[i], a);
    }
}

AdamArgs adam_args(double lr, double beta1, double beta2, double eps, double weight_decay, int step, float grad_scale) {
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    AdamArgs a;
    a.decay = (float)(1.0 - lr * weight_decay);                 // hyper-parameters arrive as doubles (Python floats): 1 - beta2 formed
    a.w1 = (float)(1.0 - beta1); a.b1 = (float)beta1; a.b2 = (float)beta2; a.w2 = (float)(1.0 - beta2);      // from a float beta2 is off by 1e-5 relative
    a.gscale = grad_scale; a.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2)); a.eps = (float)eps; a.neg_step = (float)(-lr / bc1);
    return a;
}

// ---- the capturable step: lr and the step counts live in DEVICE memory, so a recorded launch (HIP graph) computes step k at its k-th replay.
// What does not change between steps -- betas, eps, weight decay, grad_scale -- stays a kernel argument (a change means re-recording).
struct AdamHyper { double beta1, beta2, eps, weight_decay; float gscale; };

// adam_args() on the device: the same expressions in double, pow(beta, (double)step), each result rounded to float once.  Device pow and
// host pow may differ in the last bit of a double, so a float of the nine can be one ulp off the host's in rare cases, never more.
__device__ __forceinline__ AdamArgs adam_args_dev(double lr, int step, const AdamHyper& h) {
    const double bc1 = 1.0 - pow(h.beta1, (double)step), bc2 = 1.0 - pow(h.beta2, (double)step);
    AdamArgs a;
    a.decay = (float)(1.0 - lr * h.weight_decay);
    a.w1 = (float)(1.0 - h.beta1); a.b1 = (float)h.beta1; a.b2 = (float)h.beta2; a.w2 = (float)(1.0 - h.beta2);
    a.gscale = h.gscale; a.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2)); a.eps = (float)h.eps; a.neg_step = (float)(-lr / bc1);
    return a;
}

// seg_step[s] += (segment s has a gradient): a segment without one does not age (torch counts steps per parameter).  One thread per segment.
__global__ __launch_bounds__(256) void k_adamw_advance(int* __restrict__ seg_step, const unsigned long long* __restrict__ seg_grad, int n_seg) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < n_seg) seg_step[s] += seg_grad[s] != 0 ? 1 : 0;
}

// k_adamw_seg with the per-step scalars read from device memory: lr_dev[0] (double) and the segment's own step count seg_step[sg] (already
// advanced, >= 1 for a segment with a gradient).  Thread 0 forms the nine floats once per workgroup; the element update is adam1, unchanged.
// DEV_SCALE: as in k_adamw_seg.
template <bool DEV_SCALE>
__global__ __launch_bounds__(256) void k_adamw_seg_dev(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                       const unsigned long long* __restrict__ seg_grad, const long long* __restrict__ seg_off,
                                                       const int* __restrict__ seg_n, const int* __restrict__ chunk_seg,
                                                       const int* __restrict__ chunk_start, const double* __restrict__ lr_dev,
                                                       const int* __restrict__ seg_step, int chunk, AdamHyper h, const float* __restrict__ scale_dev) {
    __shared__ AdamArgs sh_a;
    const int sg = chunk_seg[blockIdx.x], start = chunk_start[blockIdx.x];
    const float* g = (const float*)seg_grad[sg];
    if (!g) return;                                             // uniform over the workgroup: nobody waits at the barrier below
    if (threadIdx.x == 0) {
        if (DEV_SCALE) h.gscale = scale_dev[0];
        sh_a = adam_args_dev(lr_dev[0], seg_step[sg], h);
    }
    __syncthreads();
    const AdamArgs a = sh_a;
    const int n = min(chunk, seg_n[sg] - start);
    const long long off = seg_off[sg] + start;
    p += off; m += off; v += off; g += start;
    if ((((uintptr_t)g) & 15u) == 0) {                          // p / m / v chunks are 16-byte aligned by construction
        for (int i = threadIdx.x; i < (n >> 2); i += 256) {
            float4 P = ((float4*)p)[i], G = ((const float4*)g)[i], M = ((float4*)m)[i], V = ((float4*)v)[i];
            adam1(P.x, G.x, M.x, V.x, a); adam1(P.y, G.y, M.y, V.y, a); adam1(P.z, G.z, M.z, V.z, a); adam1(P.w, G.w, M.w, V.w, a);
            ((float4*)p)[i] = P; ((float4*)m)[i] = M; ((float4*)v)[i] = V;
        }
        const int t = (n & ~3) + threadIdx.x;
        if (t < n) adam1(p[t], g[t], m[t], v[t], a);
    } else {
        for (int i = threadIdx.x; i < n; i += 256) adam1(p[i], g[i], m[i], v[i], a);
    }
}

// The nine floats adam_args_dev forms for one (lr, step) pair held in device memory, written out in AdamArgs order (test-facing).
__global__ void k_adamw_dev_args(const double* __restrict__ lr_dev, const int* __restrict__ step_dev, AdamHyper h, float* __restrict__ out9) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const AdamArgs a = adam_args_dev(lr_dev[0], step_dev[0], h);
    out9[0] = a.decay; out9[1] = a.w1; out9[2] = a.b1; out9[3] = a.b2; out9[4] = a.w2; out9[5] = a.gscale; out9[6] = a.inv_bc2_sqrt; out9[7] = a.eps;
    out9[8] = a.neg_step;
}

// Up to 64 addresses, passed BY VALUE, into table[first .. first + n): how the gradient-address table is filled while the stream is capturing
// (the values become part of the graph node; no host memory has to outlive the capture).
struct U64x64 { unsigned long long v[64]; };
__global__ __launch_bounds__(64) void k_set_u64_table(unsigned long long* __restrict__ table, int first, int n, U64x64 vals) {
    const int t = threadIdx.x;
    if (t < n) table[first + t] = vals.v[t];
}

// ============================================================================ Wav-KAN wavelet stage (own C-ABI entry points inside)
#include "wavkan.inc"

}  // namespace

// ============================================================================ C ABI
extern "C" {

const char* kan_version(void) { return "kanconv 0.5 (gfx950, fp32 MFMA 32x32x2, halo forward, 128/256-output tiles)"; }
const char* kan_last_error(void) { return g_err; }

int kan_plan(const KanGeom* geom, const KanBasis* basis, KanPlan* plan) {
    if (!plan) return fail("null plan");
    ConvPlan cp;
    if (int rc = plan_conv(geom, basis, &cp)) return rc;
    *plan = cp.pub;
    return 0;
}

// Does packing this geometry need wp cleared first (pad rows)?  Cached packing cannot skip a clear conditionally.
static bool pack_needs_clear(const KanGeom* g, const KanPlan& pl) {
    if (pl.fwd_band) return pl.KC != pl.IPC * pl.P || g->C % pl.IPC != 0;      // pad row of an odd NG * P / channels missing from the last group
    return pl.KC != pl.IPC * pl.P || (g->C * g->kh * g->kw) % pl.IPC != 0;
}

// The [I][O][n] layout of the MLP KAN heads (k_pack_iod / k_unpack_iod): what it covers, checked before any plan or launch.
static int iod_scope(const KanGeom* g, const KanBasis* b) {
    if (!g || !b) return fail("null geometry or basis");
    if (g->kh != 1 || g->kw != 1) return fail("the [I][O][n] coefficient layout takes 1x1 kernels only");
    if (ngroups(g) != 1) return fail("the [I][O][n] coefficient layout takes one group only");
    if (b->act != KAN_ACT_NONE) return fail("the [I][O][n] coefficient layout has no base branch (act must be KAN_ACT_NONE)");
    return 0;
}
// Tile count and grid of the two [I][O][n] kernels: one tile per (input, IOD_TO outputs), a capped grid that strides over them.
struct IodLaunch { int o_tiles; long long n_tiles; unsigned blocks; };
static IodLaunch iod_launch(const KanGeom* g, const KanPlan& pl) {
    IodLaunch l;
    l.o_tiles = ceil_div(pl.Opad, IOD_TO);
    l.n_tiles = (long long)g->C * l.o_tiles;
    l.blocks = (unsigned)(l.n_tiles < 16384 ? l.n_tiles : 16384);
    return l;
}
static int iod_vec(const void* coeffs, const void* packed, const KanGeom* g, const KanBasis* b) {
    return ((((size_t)coeffs & 15) == 0 && ((long long)g->O * b->n_basis) % 4 == 0) ? 1 : 0) | ((((size_t)packed & 15) == 0) ? 2 : 0);
}

// `iod`: w_basis is the [C][O][n_basis] coefficient tensor of an MLP KAN head (kan_pack_weights_iod) instead of the conv layout; only the
// kernel that fills wp differs -- the clears before it and the bwd-data layout derived from wp are the same code.
static int pack_weights_impl(const float* w_base, const float* w_basis, float* wp, float* wd, const KanGeom* g, const KanBasis* b,
                             const unsigned long long* fp, int fp_cur, void* stream, bool iod = false) {
    ConvPlan cp;
    if (int rc = plan_conv(g, b, &cp)) return rc;
    const KanPlan& pl = cp.pub;
    const int hb = b->act != KAN_ACT_NONE;
    if ((hb && !w_base) || !w_basis || !wp) return fail("null weight pointer");
    hipStream_t st = (hipStream_t)stream;
    const int T = g->kh * g->kw, NI = g->C * T, G = ngroups(g);
    const long long wp_gs = (long long)pl.Kpad * pl.Opad;          // floats per group in wp
    PackGeo q = pack_geo(g, b, cp, false);
    if (fp && (pack_needs_clear(g, pl) || cp.fwd == Route::DW)) return fail("cached packing is not offered for this geometry (kan_pack_cacheable)");
    // rows no source element maps to must be zero: pad rows of every chunk, and the missing items of the last chunk
    if (pl.KC != pl.IPC * pl.P || (pl.fwd_band && pack_needs_clear(g, pl))) {     // (whole-buffer clear only for P that do not divide the step)
        if (hipMemsetAsync(wp, 0, (size_t)pl.packed_weight_bytes, st) != hipSuccess) return fail("memset failed");
    } else if (!pl.fwd_band && NI % pl.IPC != 0) {
        if (G > 1) {                                        // one clear instead of G small ones
            if (hipMemsetAsync(wp, 0, (size_t)pl.packed_weight_bytes, st) != hipSuccess) return fail("memset failed");
        } else {
            size_t off = (size_t)(pl.Kpad - pl.KC) * pl.Opad;
            if (hipMemsetAsync(wp + off, 0, (size_t)pl.KC * pl.Opad * 4, st) != hipSuccess) return fail("memset failed");
        }
    }
    const int nb_base = hb ? ceil_div(g->C * T, 32) : 0;
    const int tiles_x = nb_base + ceil_div(g->C * b->n_basis * T, 32), tiles_y = pl.Opad / 32;
    const long long n_tiles = (long long)tiles_x * tiles_y;
    const long long cap = fp ? 1024 : 4096;             // cached mode: the usual outcome is an early exit, keep the grid small
    dim3 grid((unsigned)(n_tiles < cap ? n_tiles : cap), 1, G);
    if (iod) {
        const IodLaunch l = iod_launch(g, pl);
        hipLaunchKernelGGL(k_pack_iod, dim3(l.blocks), dim3(256), 0, st, w_basis, wp, q, l.o_tiles, l.n_tiles, iod_vec(w_basis, wp, g, b));
    } else {
        hipLaunchKernelGGL(k_pack, grid, dim3(256), 0, st, w_base, w_basis, wp, q, nb_base, wp_gs, tiles_x, tiles_y, fp, fp_cur);
    }
    if (wd && cp.bwd_data == Route::DW) {
        if (hipMemcpyAsync(wd, wp, (size_t)pl.packed_weight_bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail("memcpy failed");
    } else if (wd) {
        const BdCfg& c = cp.bd;
        const int bx = c.tiles_c * 4, by = c.Opad32 / 32 * G;
        const long long nt = (long long)bx * by;
        const long long capd = fp ? 128 : 1024;
        dim3 gd((unsigned)(nt < capd ? nt : capd), 1, T);
        hipLaunchKernelGGL(k_pack_bwd_data, gd, dim3(256), 0, st, (const float*)wp, wd, q, c.CH, c.tiles_c, c.Opad32, wp_gs, bx, by, fp, fp_cur);
    }
    return launch_ok("pack");
}

int kan_pack_weights(const float* w_base, const float* w_basis, float* wp, float* wd, const KanGeom* g, const KanBasis* b, void* stream) {
    return pack_weights_impl(w_base, w_basis, wp, wd, g, b, nullptr, 0, stream);
}

int kan_pack_weights_iod(const float* coeffs, float* wp, float* wd, const KanGeom* g, const KanBasis* b, void* stream) {
    if (int rc = iod_scope(g, b)) return rc;
    return pack_weights_impl(nullptr, coeffs, wp, wd, g, b, nullptr, 0, stream, true);
}

int kan_tile_orders(const KanGeom* g, const KanBasis* b) {
    ConvPlan cp;
    if (plan_conv(g, b, &cp)) return 0;
    const bool halo = cp.fwd == Route::HALO;
    return (halo && cp.quad_fwd ? KAN_ORDER_QUAD_FWD : 0) | (halo && cp.rowblk8_fwd ? KAN_ORDER_ROWBLK8_FWD : 0) | (cp.quad_bd ? KAN_ORDER_QUAD_BWD_DATA : 0) |
           (cp.fwd_wq ? KAN_ORDER_FWD_WEIGHT_SIDE : 0) | (cp.pos8_bd ? KAN_ORDER_POS8_BWD_DATA : 0) |
           (cp.pos8_bw ? KAN_ORDER_POS8_BWD_WEIGHT : 0);
}

int kan_pack_cacheable(const KanGeom* g, const KanBasis* b) {
    ConvPlan cp;
    if (plan_conv(g, b, &cp)) return 0;
    if ((long long)g->O * g->C * (b->n_basis + 1) * g->kh * g->kw >= (1ll << 31)) return 0;      // 32-bit element positions in the fingerprint
    return (!pack_needs_clear(g, cp.pub) && cp.fwd != Route::DW && ngroups(g) == 1) ? 1 : 0;
}

int kan_pack_weights_cached(const float* w_base, const float* w_basis, float* wp, float* wd, const KanGeom* g, const KanBasis* b,
                            unsigned long long* ring, int cur, int force, int sample_stride, void* stream) {
    static_assert(KAN_FP_WORDS == 3 * FP_LANES, "ring size");
    if (!ring || cur < 0 || cur > 2 || sample_stride < 1) return fail("bad fingerprint ring arguments");
    if (!kan_pack_cacheable(g, b)) return fail("cached packing is not offered for this geometry (kan_pack_cacheable)");
    const int hb = b->act != KAN_ACT_NONE;
    if ((hb && !w_base) || !w_basis) return fail("null weight pointer");
    if (((size_t)w_basis & 15) || (hb && ((size_t)w_base & 15))) return fail("cached packing needs 16-byte aligned weight tensors");
    const int T = g->kh * g->kw;
    const long long na = hb ? (long long)g->O * g->C * T : 0, nbs = (long long)g->O * g->C * b->n_basis * T;
    const long long groups4 = ((na + 3) / 4 + (nbs + 3) / 4 + sample_stride - 1) / sample_stride;
    long long blocks = (groups4 + 256 * 8 - 1) / (256 * 8); if (blocks > 4096) blocks = 4096; if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_fingerprint, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, hb ? w_base : w_basis, (unsigned)na, w_basis,
                       (unsigned)nbs, (unsigned)sample_stride, ring, cur);
    if (int rc = launch_ok("fingerprint")) return rc;
    return pack_weights_impl(w_base, w_basis, wp, wd, g, b, force ? nullptr : ring, cur, stream);
}

// `iod`: dw_basis is the [C][O][n_basis] gradient of an MLP KAN head's coefficients (kan_unpack_wgrad_iod).
// `pos8`: dwp holds the slabs of kan_conv_bwd_weight_rowgroups (channel-major rows, its own slab count) instead of the plan's route's.
static int unpack_wgrad_impl(const float* dwp, float* dw_base, float* dw_basis, const KanGeom* g, const KanBasis* b, void* stream, bool iod, bool pos8 = false) {
    ConvPlan cp;
    if (int rc = plan_conv(g, b, &cp)) return rc;
    if (pos8) {
        if (!cp.pos8_bw) return fail("this geometry / basis does not offer the 8x8 tap-skipping weight gradient (kan_tile_orders)");
        cp.bwd_weight = Route::HALO;                          // the layout of its slabs: channel-major flat rows, K of them
        cp.pub.bwd_weight_band = 0;
        cp.pub.bwd_weight_splits = cp.p8.splits;
        cp.pub.bwd_weight_slab_elems = (long long)ngroups(g) * cp.pub.K * cp.pub.Opad;
    }
    const KanPlan& pl = cp.pub;
    const int hb = b->act != KAN_ACT_NONE;
    if ((hb && !dw_base) || !dw_basis || !dwp) return fail("null weight-gradient pointer");
    hipStream_t st = (hipStream_t)stream;
    const int T = g->kh * g->kw, G = ngroups(g);
    const long long dwp_gs = (long long)(pl.bwd_weight_band ? pl.Kpad : pl.K) * pl.Opad;
    PackGeo q = pack_geo(g, b, cp, true);
    int n_slabs = pl.bwd_weight_splits;
    if (n_slabs >= 32) {                                      // (dwp is the caller's scratch: slab 0 becomes the sum)
        hipLaunchKernelGGL(k_fold_slabs, dim3(ceil_div(pl.bwd_weight_slab_elems, 64)), dim3(256), 0, st, const_cast<float*>(dwp), n_slabs,
                           pl.bwd_weight_slab_elems, pl.bwd_weight_slab_elems);
        n_slabs = 1;
    }
    const int nb_base = hb ? ceil_div(g->C * T, UNPACK_TJ) : 0;
    dim3 grid(nb_base + ceil_div(g->C * b->n_basis * T, UNPACK_TJ), ceil_div(g->O, UNPACK_TO), G);
    if (iod) {
        const IodLaunch l = iod_launch(g, pl);
        hipLaunchKernelGGL(k_unpack_iod, dim3(l.blocks), dim3(256), 0, st, dwp, dw_basis, q, l.o_tiles, l.n_tiles, n_slabs, pl.bwd_weight_slab_elems,
                           iod_vec(dw_basis, dwp, g, b));
    } else {
        hipLaunchKernelGGL(k_unpack, grid, dim3(256), 0, st, dwp, dw_base, dw_basis, q, nb_base, n_slabs, pl.bwd_weight_slab_elems, dwp_gs);
    }
    return launch_ok("unpack");
}

int kan_unpack_wgrad(const float* dwp, float* dw_base, float* dw_basis, const KanGeom* g, const KanBasis* b, void* stream) {
    return unpack_wgrad_impl(dwp, dw_base, dw_basis, g, b, stream, false);
}

int kan_unpack_wgrad_rowgroups(const float* dwp, float* dw_base, float* dw_basis, const KanGeom* g, const KanBasis* b, void* stream) {
    return unpack_wgrad_impl(dwp, dw_base, dw_basis, g, b, stream, false, true);
}

int kan_unpack_wgrad_iod(const float* dwp, float* dcoeffs, const KanGeom* g, const KanBasis* b, void* stream) {
    if (int rc = iod_scope(g, b)) return rc;
    return unpack_wgrad_impl(dwp, nullptr, dcoeffs, g, b, stream, true);
}

int kan_position_major(const float* src, float* dst, int B, int Cn, int HW, long long bstride, void* stream) {
    if (!src || !dst || B < 1 || Cn < 1 || HW < 1) return fail("bad position_major arguments");
    dim3 grid(ceil_div((long long)Cn * HW, 32), ceil_div(B, 32));
    hipLaunchKernelGGL(k_position_major, grid, dim3(256), 0, (hipStream_t)stream, src, dst, B, Cn * HW, bstride);
    return launch_ok("position_major");
}

int kan_conv_fwd(const float* x, const float* xn, const float* wp, float* z, const KanGeom* g, const KanBasis* b, const float* x_pm,
                 void* stream) {
    ConvPlan cp;
    if (int rc = plan_conv(g, b, &cp)) return rc;
    const KanPlan& pl = cp.pub;
    if (!x || !xn || !wp || !z) return fail("null tensor pointer");
    if ((b->kind == KAN_BASIS_RELU || b->kind == KAN_BASIS_GRAM) && !b->chan_table) return fail("ReLU / Gram bases need their device parameter table (chan_table)");
    hipStream_t st = (hipStream_t)stream;
    if (cp.fwd == Route::DW) {
        DevGeom dgd = dev_geom(g); DevBasis dbd = dev_basis(b);
        dim3 grid(ceil_div((long long)g->B * g->Ho * g->Wo, 256), ngroups(g));
        dispatch_kind(b->kind, [&](auto kind) {
            hipLaunchKernelGGL((k_dw_fwd<decltype(kind)::value>), grid, dim3(256), 0, st, x, xn, wp, z, dgd, dbd, pl.Opad, pl.IPC, pl.KC, pl.Kpad);
        });
        return launch_ok("dw_fwd");
    }
    if (cp.fwd == Route::BAND) {
        if (x != xn && !fast_spec(cp.fast).xn_fwd) return fail("this basis / activation pair runs on single-input kernels: pass xn == x");
        return kan_band_fwd_launch(x, xn, wp, z, g, b, &cp.band, pl.fwd_splits, pl.fwd_slab_elems, stream);
    }
    const FwdCfg& c = cp.fc;
    if ((long long)c.tiles_o * ngroups(g) > 65535) return fail("groups * output tiles exceed the grid limit");
    const unsigned x_bytes = (unsigned)((long long)g->B * g->x_bstride * 4);
    if (cp.fwd == Route::HALO) {
        if (x != xn) return fail("internal: halo forward kernel needs a single input tensor");
        DevGeom dgh = dev_geom(g); DevBasis dbh = dev_basis(b);
        const int n_pairs = g->C / 2, pps = ceil_div(n_pairs, pl.fwd_splits);
        dim3 gridh(c.tiles_p, c.tiles_o * ngroups(g), pl.fwd_splits);
        dispatch_fast<ON_HALO_FWD>(cp.fast, [&](auto fv) {
            constexpr int F = decltype(fv)::value;
            auto launch = [&](auto wo, auto w, auto r, auto nimg, auto quad) {       // (output waves, plane width, rows per tile, images per tile, quadrant order)
                constexpr int WOV = decltype(wo)::value;
                hipLaunchKernelGGL((k_conv_fwd_halo<F, WOV, decltype(w)::value, decltype(r)::value, decltype(nimg)::value, decltype(quad)::value>), gridh,
                                   dim3(WOV * 128), 0, st, x, wp, z, dgh, dbh, pl.Opad, n_pairs, pps, pl.fwd_slab_elems, x_bytes, c.tiles_o);
            };
            auto planes = [&](auto wo) {
                if constexpr (decltype(wo)::value == 4) {
                    // 32 images x one quadrant (it stores 8-byte words: a z or a batch stride that is not 8-byte aligned keeps the row blocks)
                    if (g->W == 4 && cp.quad_fwd && ((uintptr_t)z & 7u) == 0 && (g->y_bstride & 1) == 0 && (pl.fwd_slab_elems & 1) == 0)
                        return launch(wo, IC<4>{}, IC<4>{}, IC<8>{}, IC<1>{});
                }
                if (g->W == 32) launch(wo, IC<32>{}, IC<4>{}, IC<1>{}, IC<0>{});
                else if (g->W == 16) launch(wo, IC<16>{}, IC<8>{}, IC<1>{}, IC<0>{});
                else if (g->W == 8) {
                    if constexpr (decltype(wo)::value == 4) {          // 4 images x half a plane, row blocks (B a multiple of 4)
                        if (cp.rowblk8_fwd) return launch(wo, IC<8>{}, IC<4>{}, IC<4>{}, IC<0>{});
                    }
                    launch(wo, IC<8>{}, IC<8>{}, IC<2>{}, IC<0>{});
                }
                else launch(wo, IC<4>{}, IC<4>{}, IC<8>{}, IC<0>{});
            };
            if constexpr (fast_has(F, ON_BIG_TILES)) {
                if (c.TO == 256) return planes(IC<4>{});
            }
            planes(IC<2>{});
        });
        return launch_ok("conv_fwd_halo");
    }
    DevGeom dg = dev_geom(g);
    dg.pix_major = (x_pm && x == xn && cp.pm_fwd) ? 1 : 0;      // (one copy serves both inputs only when they are the same)
    if (dg.pix_major) { x = x_pm; xn = x_pm; }
    DevBasis db = dev_basis(b);
    dim3 grid(c.tiles_p, c.tiles_o * ngroups(g), pl.fwd_splits);   // always the plan's slab count: the consumer sums exactly that many
    const int cps = dg.pix_major ? pl.fwd_target : ceil_div(c.chunks, pl.fwd_splits);
    TilePerm perm; perm.n = 0;
    if (dg.pix_major) perm = tile_perm(c.tiles_p, [&](int t) {     // weight of a pixel tile = its own split count (live work)
        const int hw = (int)(((long long)t * c.TP) / g->B);
        return ceil_div(live_taps_out(g, hw < g->Ho * g->Wo ? hw : 0) * ceil_div(g->C, pl.IPC), cps > 0 ? cps : 1);
    });
    if (x != xn && !fast_spec(cp.fast).xn_fwd)
        return fail("this basis / activation pair runs on single-input kernels: pass xn == x");
    auto launch = [&](auto kind, auto fast, auto wo, auto kc) {
        constexpr int WO = decltype(wo)::value;
        hipLaunchKernelGGL((k_conv_fwd<decltype(kind)::value, decltype(fast)::value, WO, 2, decltype(kc)::value>), grid, dim3(WO * 2 * 64), 0, st,
                           x, xn, wp, z, dg, db, pl.Opad, pl.IPC, c.chunks, cps, pl.fwd_slab_elems, x_bytes, perm, c.tiles_o);
    };
    const bool fast = dispatch_fast<ON_TAP_MAJOR>(cp.fast, [&](auto fv) {
        constexpr int F = decltype(fv)::value;
        if constexpr (fast_has(F, ON_BIG_TILES)) {
            if (c.TO == 256) return launch(IC<fast_kind(F)>{}, fv, IC<4>{}, IC<fast_spec(F).kc>{});
        }
        if (c.TO == 128) launch(IC<fast_kind(F)>{}, fv, IC<2>{}, IC<fast_spec(F).kc>{});
        else launch(IC<fast_kind(F)>{}, fv, IC<1>{}, IC<fast_spec(F).kc>{});
    });
    if (!fast) dispatch_kind(b->kind, [&](auto kind) {
        pick<18, 12, 16>(pl.KC, [&](auto kc) {
            if (c.TO == 128) launch(kind, IC<FAST_GENERIC>{}, IC<2>{}, kc);
            else launch(kind, IC<FAST_GENERIC>{}, IC<1>{}, kc);
        });
    });
    return launch_ok("conv_fwd");
}

static int conv_bwd_data_impl(const float* dz, const float* x, const float* xn, const float* wd, float* dx, float* dxn, float* dpar,
                              const KanGeom* g, const KanBasis* b, const float* dz_pm, void* stream);

int kan_conv_bwd_data(const float* dz, const float* x, const float* xn, const float* wd, float* dx, float* dxn,
                      const KanGeom* g, const KanBasis* b, const float* dz_pm, void* stream) {
    return conv_bwd_data_impl(dz, x, xn, wd, dx, dxn, nullptr, g, b, dz_pm, stream);
}

int kan_conv_bwd_data_params(const float* dz, const float* x, const float* xn, const float* wd, float* dx, float* dxn, float* dparams,
                             const KanGeom* g, const KanBasis* b, const float* dz_pm, void* stream) {
    if (!dparams) return fail("null dparams");
    if (b && b->kind != KAN_BASIS_RELU && b->kind != KAN_BASIS_GRAM) return fail("kan_conv_bwd_data_params: only the ReLU-KAN and GRAM bases accumulate parameter gradients in this launch");
    return conv_bwd_data_impl(dz, x, xn, wd, dx, dxn, dparams, g, b, dz_pm, stream);
}

static int conv_bwd_data_impl(const float* dz, const float* x, const float* xn, const float* wd, float* dx, float* dxn, float* dpar,
                              const KanGeom* g, const KanBasis* b, const float* dz_pm, void* stream) {
    ConvPlan cp;
    if (int rc = plan_conv(g, b, &cp)) return rc;
    const KanPlan& pl = cp.pub;
    if (dpar && cp.bwd_data == Route::DW) return fail("kan_conv_bwd_data_params: depthwise layers take the weight-gradient route");
    if (!dz || !x || !xn || !wd || !dx) return fail("null tensor pointer");
    if ((b->kind == KAN_BASIS_RELU || b->kind == KAN_BASIS_GRAM) && !b->chan_table) return fail("ReLU / Gram bases need their device parameter table (chan_table)");
    if (!dxn && x != xn) return fail("dxn is required when xn != x");
    hipStream_t st = (hipStream_t)stream;
    if (cp.bwd_data == Route::DW) {
        DevGeom dgd = dev_geom(g); DevBasis dbd = dev_basis(b);
        dim3 grid(ceil_div((long long)g->B * g->H * g->W, 256), ngroups(g));
        dispatch_kind(b->kind, [&](auto kind) {
            hipLaunchKernelGGL((k_dw_bwd_data<decltype(kind)::value>), grid, dim3(256), 0, st, dz, x, xn, wd, dx, dxn, dgd, dbd, pl.Opad, pl.IPC, pl.KC, pl.Kpad);
        });
        return launch_ok("dw_bwd_data");
    }
    const BdCfg& c = cp.bd;
    DevGeom dg = dev_geom(g);
    dg.pix_major = (dz_pm && cp.pm_bwd_data) ? 1 : 0;
    if (dg.pix_major) dz = dz_pm;
    DevBasis db = dev_basis(b);
    if ((long long)c.tiles_c * ngroups(g) > 65535) return fail("groups * channel tiles exceed the grid limit");
    dim3 grid(c.tiles_p, c.tiles_c * ngroups(g), pl.bwd_data_splits);
    const int cps = dg.pix_major ? pl.bwd_data_target : ceil_div(c.chunks, pl.bwd_data_splits);
    TilePerm perm; perm.n = 0;
    if (dg.pix_major) perm = tile_perm(c.tiles_p, [&](int t) {
        const int hw = (int)(((long long)t * 128) / g->B);
        return ceil_div(live_taps_in(g, hw < g->H * g->W ? hw : 0) * c.n_ob, cps > 0 ? cps : 1);
    });
    // compile-time epilogues: single-input specs need x == xn and one output; the two-tensor (FastKAN) specs need both tensors
    const int fast = (fast_spec(cp.fast).xn_bwd ? (x != xn && dxn) : (x == xn && !dxn)) ? cp.fast : FAST_GENERIC;
    // 4x4 planes in tiles of 8 whole images: row-ordered pixel blocks, dead (row, tap row) blocks skipped (see the kernel)
    const bool rb = !dg.pix_major && cp.rowblk_bwd_data;
    // ... with whole 32-image groups and the position-major copy of dz at hand: quadrant tiles fed from dz_pm (same tile count, splits and slabs)
    const bool quad = rb && cp.quad_bd && dz_pm && x == xn && !dxn;
    // 8x8 planes, same conditions: tiles of 32 images x 4 columns of a plane row fed from dz_pm, dead tap rows and columns skipped (the kernel's RB = 3); its
    // epilogue moves x and dx 16 bytes at a time (the planner checked the batch stride, the pointers are checked here)
    const bool pos8 = cp.pos8_bd && !dg.pix_major && dz_pm && x == xn && !dxn && !dpar && ((uintptr_t)x | (uintptr_t)dx) % 16 == 0;
    const unsigned dz_bytes = pos8 ? (unsigned)((long long)g->O * g->Ho * g->Wo * g->B * 4) : (unsigned)((long long)g->B * g->y_bstride * 4);
    auto launch = [&](auto kind, auto fast, auto rbv) {
        hipLaunchKernelGGL((k_conv_bwd_data<decltype(kind)::value, decltype(fast)::value, decltype(rbv)::value>), grid, dim3(256), 0, st,
                           decltype(rbv)::value >= 2 ? dz_pm : dz, x, xn, wd,
                           dx, dxn, dg, db, c.CH, c.tiles_c, c.n_ob, c.Opad32, c.chunks, cps, pl.bwd_data_slab_elems, dz_bytes, perm, dpar);
    };
    const bool launched = dispatch_fast<ON_TAP_MAJOR>(fast, [&](auto fv) {
        constexpr int F = decltype(fv)::value;
        if constexpr (fast_has(F, ON_ROWBLK_BWD_DATA)) {
            if (pos8) return launch(IC<fast_kind(F)>{}, fv, IC<3>{});
            if (quad) return launch(IC<fast_kind(F)>{}, fv, IC<2>{});
            if (rb) return launch(IC<fast_kind(F)>{}, fv, IC<1>{});
        }
        launch(IC<fast_kind(F)>{}, fv, IC<0>{});
    });
    if (!launched) dispatch_kind(b->kind, [&](auto kind) { launch(kind, IC<FAST_GENERIC>{}, IC<0>{}); });
    return launch_ok("conv_bwd_data");
}

int kan_conv_bwd_weight(const float* dz, const float* x, const float* xn, float* dwp, const KanGeom* g, const KanBasis* b,
                        const float* x_pm, const float* dz_pm, void* stream) {
    ConvPlan cp;
    if (int rc = plan_conv(g, b, &cp)) return rc;
    const KanPlan& pl = cp.pub;
    if (!dz || !x || !xn || !dwp) return fail("null tensor pointer");
    if ((b->kind == KAN_BASIS_RELU || b->kind == KAN_BASIS_GRAM) && !b->chan_table) return fail("ReLU / Gram bases need their device parameter table (chan_table)");
    hipStream_t st = (hipStream_t)stream;
    if (cp.bwd_weight == Route::DW) {
        DevGeom dgd = dev_geom(g); DevBasis dbd = dev_basis(b);
        dim3 grid(pl.bwd_weight_splits, ngroups(g));
        dispatch_kind(b->kind, [&](auto kind) {
            hipLaunchKernelGGL((k_dw_bwd_weight<decltype(kind)::value>), grid, dim3(256), 0, st, dz, x, xn, dwp, dgd, dbd, pl.K, pl.Opad, pl.bwd_weight_slab_elems);
        });
        return launch_ok("dw_bwd_weight");
    }
    if (cp.bwd_weight == Route::BAND) {
        if (x != xn && !fast_spec(cp.fast).xn_fwd) return fail("this basis / activation pair runs on single-input kernels: pass xn == x");
        return kan_band_bwd_weight_launch(dz, x, xn, dwp, g, b, &cp.band, pl.bwd_weight_splits, pl.bwd_weight_slab_elems, stream);
    }
    const unsigned x_bytes = (unsigned)((long long)g->B * g->x_bstride * 4), dz_bytes = (unsigned)((long long)g->B * g->y_bstride * 4);
    if (cp.bwd_weight == Route::HALO) {
        if (x != xn) return fail("internal: the channel-major weight-gradient layout needs x == xn");
        const BwHaloCfg& hc = cp.bwh;
        const DevGeom dgh = dev_geom(g); const DevBasis dbh = dev_basis(b);
        if ((long long)hc.tiles_o * ngroups(g) > 65535) return fail("groups * output tiles exceed the grid limit");
        dim3 grid(hc.tiles_r, hc.tiles_o * ngroups(g), hc.splits);
        dispatch_fast<ON_HALO_BWD_WEIGHT>(cp.fast, [&](auto fv) {
            auto launch = [&](auto w, auto r, auto nimg) {          // (plane width, rows per band, images per band)
                hipLaunchKernelGGL((k_conv_bwd_weight_halo<decltype(fv)::value, decltype(w)::value, decltype(r)::value, decltype(nimg)::value>), grid,
                                   dim3(256), 0, st, dz, x, dwp, dgh, dbh, pl.K, pl.Opad, hc.n_bands, hc.bands_per_split, pl.bwd_weight_slab_elems,
                                   x_bytes, dz_bytes, hc.tiles_o);
            };
            if (g->W == 16) launch(IC<16>{}, IC<4>{}, IC<1>{});
            else if (g->W == 8) launch(IC<8>{}, IC<8>{}, IC<1>{});
            else launch(IC<4>{}, IC<4>{}, IC<2>{});
        });
        return launch_ok("conv_bwd_weight_halo");
    }
    const BwCfg& c = cp.bw;
    DevGeom dg = dev_geom(g);
    dg.pix_major = (x_pm && dz_pm && x == xn && cp.pm_bwd_weight) ? 1 : 0;
    if (dg.pix_major) { x = x_pm; xn = x_pm; dz = dz_pm; }
    DevBasis db = dev_basis(b);
    if ((long long)c.tiles_o * ngroups(g) > 65535) return fail("groups * output tiles exceed the grid limit");
    dim3 grid(c.tiles_r, c.tiles_o * ngroups(g), pl.bwd_weight_splits);
    const int cps = dg.pix_major ? pl.bwd_weight_target : ceil_div(c.chunks, pl.bwd_weight_splits);
    if (x != xn && !fast_spec(cp.fast).xn_fwd)
        return fail("this basis / activation pair runs on single-input kernels: pass xn == x");
    auto launch = [&](auto kind, auto fast, auto wr, auto wc) {
        constexpr int WR = decltype(wr)::value, WC = decltype(wc)::value;
        hipLaunchKernelGGL((k_conv_bwd_weight<decltype(kind)::value, decltype(fast)::value, WR, WC>), grid, dim3(WR * WC * 64), 0, st, dz, x, xn, dwp,
                           dg, db, pl.K, pl.Opad, c.chunks, cps, pl.bwd_weight_slab_elems, x_bytes, dz_bytes, c.tiles_o);
    };
    auto tiles = [&](auto kind, auto fast) {                        // 128 outputs: 2 x 2 waves; 64 outputs: 4 x 1
        if (c.TO == 128) launch(kind, fast, IC<2>{}, IC<2>{});
        else launch(kind, fast, IC<4>{}, IC<1>{});
    };
    const bool fast = dispatch_fast<ON_TAP_MAJOR>(cp.fast, [&](auto fv) {
        constexpr int F = decltype(fv)::value;
        if constexpr (fast_has(F, ON_BIG_TILES)) {
            if (c.TO == 256) return launch(IC<fast_kind(F)>{}, fv, IC<2>{}, IC<4>{});
        }
        tiles(IC<fast_kind(F)>{}, fv);
    });
    if (!fast) dispatch_kind(b->kind, [&](auto kind) { tiles(kind, IC<FAST_GENERIC>{}); });
    return launch_ok("conv_bwd_weight");
}

int kan_bwd_weight_rowgroup_slabs(const KanGeom* g, const KanBasis* b) {
    ConvPlan cp;
    if (plan_conv(g, b, &cp)) return 0;
    return cp.pos8_bw ? cp.p8.splits : 0;
}

int kan_conv_bwd_weight_rowgroups(const float* dz, const float* x, float* dwp, const KanGeom* g, const KanBasis* b, void* stream) {
    ConvPlan cp;
    if (int rc = plan_conv(g, b, &cp)) return rc;
    const KanPlan& pl = cp.pub;
    if (!dz || !x || !dwp) return fail("null tensor pointer");
    if (!cp.pos8_bw) return fail("this geometry / basis does not offer the 8x8 tap-skipping weight gradient (kan_tile_orders)");
    const BwHaloCfg& hc = cp.p8;
    const DevGeom dgh = dev_geom(g); const DevBasis dbh = dev_basis(b);
    if ((long long)hc.tiles_o * ngroups(g) > 65535) return fail("groups * output tiles exceed the grid limit");
    const unsigned x_bytes = (unsigned)((long long)g->B * g->x_bstride * 4), dz_bytes = (unsigned)((long long)g->B * g->y_bstride * 4);
    const long long slab_elems = (long long)ngroups(g) * pl.K * pl.Opad;
    dim3 grid(hc.tiles_r, hc.tiles_o * ngroups(g), hc.splits);
    dispatch_fast<ON_HALO_BWD_WEIGHT>(cp.fast, [&](auto fv) {
        constexpr int F = decltype(fv)::value;
        if constexpr (fast_kind(F) == KAN_BASIS_BSPLINE)
            hipLaunchKernelGGL((k_conv_bwd_weight_pos8<F>), grid, dim3(256), 0, (hipStream_t)stream, dz, x, dwp, dgh, dbh, pl.K, pl.Opad, hc.n_bands,
                               hc.bands_per_split, slab_elems, x_bytes, dz_bytes, hc.tiles_o);
    });
    return launch_ok("conv_bwd_weight_pos8");
}

int kan_position_major_expanded(const float* x, float* e_pm, const KanGeom* g, const KanBasis* b, void* stream) {
    ConvPlan cp;
    if (int rc = plan_conv(g, b, &cp)) return rc;
    const KanPlan& pl = cp.pub;
    if (!x || !e_pm) return fail("null tensor pointer");
    if (!pl.e_pm_wanted) return fail("this geometry / basis does not use the expanded position-major copy (plan.e_pm_wanted)");
    const int G = ngroups(g), CHW = G * g->C * g->H * g->W;
    DevBasis db = dev_basis(b);
    dim3 grid(ceil_div(CHW, 32), ceil_div(g->B, 32));
    float* dump = e_pm + (pl.e_pm_elems - 256);
    if ((b->kind == KAN_BASIS_RELU || b->kind == KAN_BASIS_GRAM) && !b->chan_table) return fail("ReLU / Gram bases need their device parameter table (chan_table)");
    dispatch_fast<ON_EXPANDED>(cp.fast, [&](auto fv) {             // (ReLU-KAN: basis->order selects value / phase-derivative planes)
        constexpr int F = decltype(fv)::value;
        hipLaunchKernelGGL((k_expand_pm<fast_kind(F), F>), grid, dim3(256), 0, (hipStream_t)stream, x, e_pm, db, g->B, CHW, g->H * g->W, g->C, g->x_bstride, dump);
    });
    return launch_ok("position_major_expanded");
}

// order < 0: the planner's; 0 / KAN_ORDER_FWD_WEIGHT_SIDE: forced (kan_conv_fwd_expanded_order)
static int conv_fwd_expanded_impl(const float* e_pm, const float* wp, float* z, const KanGeom* g, const KanBasis* b, void* stream, int order) {
    ConvPlan cp;
    if (int rc = plan_conv(g, b, &cp)) return rc;
    const KanPlan& pl = cp.pub;
    if (!e_pm || !wp || !z) return fail("null tensor pointer");
    if (cp.fwd != Route::EXPANDED) return fail("the forward of this geometry / basis does not read the expanded position-major copy (plan.fwd_expanded)");
    if (order >= 0 && order != 0 && order != KAN_ORDER_FWD_WEIGHT_SIDE) return fail("order must be 0 or KAN_ORDER_FWD_WEIGHT_SIDE");
    if (order == KAN_ORDER_FWD_WEIGHT_SIDE && !cp.fwd_wq) return fail("this geometry does not offer the weight-side order (kan_tile_orders)");
    const FwdCfg& c = cp.fc;                                // (128 x 128 tiles, 18-row steps of channel pairs: the planner's pmdma shape)
    DevGeom dg = dev_geom(g);
    dg.pix_major = 1;
    if ((long long)c.tiles_o * ngroups(g) > 65535) return fail("groups * output tiles exceed the grid limit");
    if (order < 0 ? cp.fwd_wq : order != 0) {               // same grid: 4 output sub-tiles x image tiles in x
        if ((size_t)z & 15) return fail("the weight-side forward stores 16-byte groups: z must be 16-byte aligned");
        dim3 grid(c.tiles_p, c.tiles_o * ngroups(g), pl.fwd_splits);
        hipLaunchKernelGGL((k_conv_fwd_pmdma_wq<18>), grid, dim3(256), 0, (hipStream_t)stream, e_pm, wp, z, dg, pl.Opad, c.chunks, pl.fwd_target,
                           pl.fwd_slab_elems, (unsigned)(((long long)pl.e_pm_elems - 256) * 4), (unsigned)((long long)pl.Kpad * pl.Opad * 4), c.tiles_o,
                           cp.pmdma_xcd ? 1 : 0);
        return launch_ok("conv_fwd_expanded");
    }
    TilePerm perm; perm.n = 0;
    if (!cp.pmdma_xcd) {                                    // weight of a pixel tile = its live work (as kan_conv_fwd)
        const int tpp = ceil_div(g->B, c.TP), cpt = ceil_div(g->C, pl.IPC);
        perm = tile_perm(c.tiles_p, [&](int t) { return live_taps_out(g, t / tpp) * cpt; });
    }
    dim3 grid(c.tiles_p, c.tiles_o * ngroups(g), pl.fwd_splits);
    hipLaunchKernelGGL((k_conv_fwd_pmdma<18>), grid, dim3(256), 0, (hipStream_t)stream, e_pm, wp, z, dg, pl.P, make_fastdiv(pl.P), pl.Opad, c.chunks,
                       pl.fwd_target, pl.fwd_slab_elems, (unsigned)(((long long)pl.e_pm_elems - 256) * 4),
                       (unsigned)((long long)pl.Kpad * pl.Opad * 4), perm, c.tiles_o, cp.pmdma_xcd ? 1 : 0);
    return launch_ok("conv_fwd_expanded");
}

int kan_conv_fwd_expanded(const float* e_pm, const float* wp, float* z, const KanGeom* g, const KanBasis* b, void* stream) {
    return conv_fwd_expanded_impl(e_pm, wp, z, g, b, stream, -1);
}

int kan_conv_fwd_expanded_order(const float* e_pm, const float* wp, float* z, const KanGeom* g, const KanBasis* b, void* stream, int order) {
    if (order < 0) return fail("order must be 0 or KAN_ORDER_FWD_WEIGHT_SIDE");
    return conv_fwd_expanded_impl(e_pm, wp, z, g, b, stream, order);
}

int kan_conv_bwd_weight_expanded(const float* dz_pm, const float* e_pm, float* dwp, const KanGeom* g, const KanBasis* b, void* stream) {
    ConvPlan cp;
    if (int rc = plan_conv(g, b, &cp)) return rc;
    const KanPlan& pl = cp.pub;
    if (!dz_pm || !e_pm || !dwp) return fail("null tensor pointer");
    if (cp.bwd_weight != Route::EXPANDED) return fail("the weight gradient of this geometry / basis does not read the expanded position-major copy (plan.bwd_weight_expanded)");
    const BwCfg& c = cp.bw;                                 // (128 x 128 tiles: the planner's pmdma shape)
    DevGeom dg = dev_geom(g);
    dg.pix_major = 1;
    if ((long long)c.tiles_o * ngroups(g) > 65535) return fail("groups * output tiles exceed the grid limit");
    dim3 grid(c.tiles_r, c.tiles_o * ngroups(g), pl.bwd_weight_splits);
    // longest-first dispatch order over the (tap, split) classes (PmOrder): live steps of a tap = live positions x 16-image chunks, cut into
    // min(splits, ceil(live / target)) ranges exactly as the kernel cuts them
    PmOrder ord; ord.n = 0; ord.xcd = 0;
    const int T = g->kh * g->kw, S = pl.bwd_weight_splits, trpt = (g->C * pl.P) / 128;
    if (cp.pm_lpt && T * S <= PM_ORDER_MAX && T <= 255 && S <= 255 && trpt * T == c.tiles_r) {
        int steps[PM_ORDER_MAX], idx[PM_ORDER_MAX], n = 0;
        unsigned char tp[PM_ORDER_MAX], zz[PM_ORDER_MAX];
        const int per_pos = ceil_div(g->B, 16), tgt = pl.bwd_weight_target > 0 ? pl.bwd_weight_target : 1;
        for (int tap = 0; tap < T; ++tap) {
            const int L = live_positions_for_tap(g, tap) * per_pos;
            int St = ceil_div(L, tgt); St = St < 1 ? 1 : St; St = St > S ? S : St;
            for (int z = 0; z < S; ++z) {
                steps[n] = z < St ? (int)((long long)L * (z + 1) / St - (long long)L * z / St) : 0;
                tp[n] = (unsigned char)tap; zz[n] = (unsigned char)z; idx[n] = n; ++n;
            }
        }
        for (int i = 1; i < n; ++i) {                            // insertion sort by decreasing steps (stable)
            const int v = idx[i]; int j = i;
            while (j > 0 && steps[idx[j - 1]] < steps[v]) { idx[j] = idx[j - 1]; --j; }
            idx[j] = v;
        }
        const int per_entry = trpt * c.tiles_o * ngroups(g);
        ord.n = n; ord.tiles_r_per_tap = trpt; ord.xcd = cp.pm_xcd ? 1 : 0;
        for (int i = 0; i < n; ++i) { ord.tap[i] = tp[idx[i]]; ord.z[i] = zz[idx[i]]; ord.first[i] = i * per_entry; }
        ord.first[n] = n * per_entry;
        grid = dim3((unsigned)(n * per_entry), 1, 1);
    }
    hipLaunchKernelGGL(k_conv_bwd_weight_pmdma, grid, dim3(256), 0, (hipStream_t)stream, dz_pm, e_pm, dwp, dg, pl.P, make_fastdiv(pl.P), pl.K, pl.Opad, c.chunks,
                       pl.bwd_weight_target, pl.bwd_weight_slab_elems, (unsigned)(((long long)pl.e_pm_elems - 256) * 4),
                       (unsigned)((long long)g->B * g->y_bstride * 4), c.tiles_o, pl.bwd_weight_splits, ord);
    return launch_ok("conv_bwd_weight_expanded");
}

int kan_slab_reduce(const float* slabs, int n_slabs, long long slab_elems, float* out, int B, int Cn, int HW, long long bstride, void* stream) {
    if (!slabs || !out || n_slabs < 1) return fail("bad slab_reduce arguments");
    long long total = (long long)B * Cn * HW;
    int blocks = (int)((total + 255) / 256); if (blocks > 4096) blocks = 4096; if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_slab_reduce, dim3(blocks), dim3(256), 0, (hipStream_t)stream, slabs, n_slabs, slab_elems, out, Cn, HW, bstride, total);
    return launch_ok("slab_reduce");
}

static bool norm_float2_ok(const void* z, const void* z_out, long long bstride, int HW, long long slab_elems) {
    return ((bstride | HW) & 1) == 0 && (((size_t)z | (size_t)z_out) & 7) == 0 && (slab_elems & 1) == 0;
}
static int norm_pool_mode(const void* pidx, const PoolGeo& pg) { return !pidx ? KAN_NORM_POOL_NONE : pg.k ? KAN_NORM_POOL_K : KAN_NORM_POOL_2X2; }

static int instnorm_fwd_any(const float* z, int n_slabs, long long slab_elems, float* z_out, const float* gamma, const float* beta,
                            const float* prelu_a, float* y, float* mean, float* rstd, int B, int Cn, int HW, long long bstride, float eps,
                            int prelu_span, unsigned char* pidx, int W, void* stream, PoolGeo pg = PoolGeo{}) {
    if (!z || !z_out || !y || !mean || !rstd || n_slabs < 1 || B < 1 || Cn < 1 || HW < 1) return fail("bad instnorm_fwd arguments");
    hipStream_t st = (hipStream_t)stream;
    int planes = B * Cn;
    const KanNormRoute r = norm_route(false, planes, HW, norm_pool_mode(pidx, pg), norm_float2_ok(z, z_out, bstride, HW, slab_elems));
    bool ok;
    if (r.kernel == KAN_NORM_REGS && r.pool)                  // lanes own 2x2 windows (float2 accesses)
        ok = pick_regs_pool2(r, [&](auto v) { launch_in_fwd_regs<decltype(v)::G, decltype(v)::EPL, decltype(v)::PPI, true>(st, r, planes, z, n_slabs, slab_elems, z_out, gamma, beta, prelu_a, y, mean, rstd, Cn, HW, bstride, eps, prelu_span, pidx, W); });
    else if (r.kernel == KAN_NORM_REGS)
        ok = pick_regs_plain(r, [&](auto v) { launch_in_fwd_regs<decltype(v)::G, decltype(v)::EPL, decltype(v)::PPI, false>(st, r, planes, z, n_slabs, slab_elems, z_out, gamma, beta, prelu_a, y, mean, rstd, Cn, HW, bstride, eps, prelu_span, pidx, W); });
    else
        ok = pick_generic(r, [&](auto v) { launch_in_fwd<decltype(v)::G>(st, r, planes, z, n_slabs, slab_elems, z_out, gamma, beta, prelu_a, y, mean, rstd, Cn, HW, bstride, eps, prelu_span, pidx, W, pg); });
    if (!ok) return fail("instnorm_fwd: no kernel for the route");
    return launch_ok("instnorm_fwd");
}

int kan_instnorm_prelu_fwd(const float* z, int n_slabs, long long slab_elems, float* z_out, const float* gamma, const float* beta,
                           const float* prelu_a, float* y, float* mean, float* rstd, int B, int Cn, int HW, long long bstride, float eps,
                           int prelu_span, void* stream) {
    return instnorm_fwd_any(z, n_slabs, slab_elems, z_out, gamma, beta, prelu_a, y, mean, rstd, B, Cn, HW, bstride, eps, prelu_span, nullptr, 0,
                            stream);
}

int kan_instnorm_prelu_pool_fwd(const float* z, int n_slabs, long long slab_elems, float* z_out, const float* gamma, const float* beta,
                                const float* prelu_a, float* y_pooled, unsigned char* pool_idx, float* mean, float* rstd, int B, int Cn,
                                int H, int W, long long bstride, float eps, int prelu_span, void* stream) {
    if (!pool_idx || H < 2 || W < 2 || (H & 1) || (W & 1)) return fail("fused 2x2 max-pool needs even H and W and an index buffer");
    return instnorm_fwd_any(z, n_slabs, slab_elems, z_out, gamma, beta, prelu_a, y_pooled, mean, rstd, B, Cn, H * W, bstride, eps, prelu_span,
                            pool_idx, W, stream);
}

static int instnorm_bwd_any(const float* dy, const float* z, const float* mean, const float* rstd, const float* gamma, const float* beta,
                            const float* prelu_a, float* dz, float* dgamma, float* dbeta, float* dprelu, int B, int Cn, int HW,
                            long long bstride, int prelu_span, const unsigned char* pidx, int W, void* stream, PoolGeo pg = PoolGeo{}) {
    if (!dy || !z || !mean || !rstd || !dz || B < 1 || Cn < 1 || HW < 1) return fail("bad instnorm_bwd arguments");
    hipStream_t st = (hipStream_t)stream;
    int planes = B * Cn;
    const KanNormRoute r = norm_route(true, planes, HW, norm_pool_mode(pidx, pg), true);
    bool ok;
    if (r.kernel == KAN_NORM_REGS)                            // register-resident variants: G lanes x EPL elements cover the plane
        ok = pick_regs_plain(r, [&](auto v) { launch_in_bwd_regs<decltype(v)::G, decltype(v)::EPL, decltype(v)::PPI>(st, r, planes, dy, z, mean, rstd, gamma, beta, prelu_a, dz, dgamma, dbeta, dprelu, Cn, HW, bstride, prelu_span, pidx, W); });
    else
        ok = pick_generic(r, [&](auto v) { launch_in_bwd<decltype(v)::G>(st, r, planes, dy, z, mean, rstd, gamma, beta, prelu_a, dz, dgamma, dbeta, dprelu, Cn, HW, bstride, prelu_span, pidx, W, pg); });
    if (!ok) return fail("instnorm_bwd: no kernel for the route");
    return launch_ok("instnorm_bwd");
}

int kan_instnorm_prelu_bwd(const float* dy, const float* z, const float* mean, const float* rstd, const float* gamma, const float* beta,
                           const float* prelu_a, float* dz, float* dgamma, float* dbeta, float* dprelu, int B, int Cn, int HW,
                           long long bstride, int prelu_span, void* stream) {
    return instnorm_bwd_any(dy, z, mean, rstd, gamma, beta, prelu_a, dz, dgamma, dbeta, dprelu, B, Cn, HW, bstride, prelu_span, nullptr, 0, stream);
}

int kan_instnorm_prelu_pool_bwd(const float* dy_pooled, const unsigned char* pool_idx, const float* z, const float* mean, const float* rstd,
                                const float* gamma, const float* beta, const float* prelu_a, float* dz, float* dgamma, float* dbeta,
                                float* dprelu, int B, int Cn, int H, int W, long long bstride, int prelu_span, void* stream) {
    if (!pool_idx || H < 2 || W < 2 || (H & 1) || (W & 1)) return fail("fused 2x2 max-pool needs even H and W and the forward's index buffer");
    return instnorm_bwd_any(dy_pooled, z, mean, rstd, gamma, beta, prelu_a, dz, dgamma, dbeta, dprelu, B, Cn, H * W, bstride, prelu_span,
                            pool_idx, W, stream);
}

static int pool_geo(int H, int W, int k, int st, PoolGeo* pg) {
    if (k < 2 || k > 15 || st < 1 || st > k || H < k || W < k) return fail("fused max-pool: need 2 <= kernel <= 15, 1 <= stride <= kernel, plane >= kernel");
    pg->k = k; pg->s = st; pg->Hp = (H - k) / st + 1; pg->Wp = (W - k) / st + 1;
    pg->divWp = make_fastdiv(pg->Wp); pg->divS = make_fastdiv(st); pg->divK = make_fastdiv(k); pg->nc = (k + st - 1) / st; pg->divNc = make_fastdiv(pg->nc); pg->lds = 0;
    return 0;
}

int kan_instnorm_prelu_poolk_fwd(const float* z, int n_slabs, long long slab_elems, float* z_out, const float* gamma, const float* beta,
                                 const float* prelu_a, float* y_pooled, unsigned char* pool_idx, float* mean, float* rstd, int B, int Cn,
                                 int H, int W, long long bstride, float eps, int prelu_span, int pool_k, int pool_s, void* stream) {
    PoolGeo pg;
    if (!pool_idx) return fail("fused max-pool needs an index buffer");
    if (pool_geo(H, W, pool_k, pool_s, &pg)) return -1;
    return instnorm_fwd_any(z, n_slabs, slab_elems, z_out, gamma, beta, prelu_a, y_pooled, mean, rstd, B, Cn, H * W, bstride, eps, prelu_span,
                            pool_idx, W, stream, pg);
}

int kan_instnorm_prelu_poolk_bwd(const float* dy_pooled, const unsigned char* pool_idx, const float* z, const float* mean, const float* rstd,
                                 const float* gamma, const float* beta, const float* prelu_a, float* dz, float* dgamma, float* dbeta,
                                 float* dprelu, int B, int Cn, int H, int W, long long bstride, int prelu_span, int pool_k, int pool_s,
                                 void* stream) {
    PoolGeo pg;
    if (!pool_idx) return fail("fused max-pool needs the forward's index buffer");
    if (pool_geo(H, W, pool_k, pool_s, &pg)) return -1;
    return instnorm_bwd_any(dy_pooled, z, mean, rstd, gamma, beta, prelu_a, dz, dgamma, dbeta, dprelu, B, Cn, H * W, bstride, prelu_span,
                            pool_idx, W, stream, pg);
}

int kan_norm_route(int backward, int B, int Cn, int H, int W, long long bstride, int n_slabs, long long slab_elems, int pool2x2, int pool_k,
                   int pool_s, int aligned8, KanNormRoute* route) {
    if (!route || n_slabs < 1 || B < 1 || Cn < 1 || H < 1 || W < 1) return fail("bad norm_route arguments");
    if (pool2x2 && (pool_k || H < 2 || W < 2 || (H & 1) || (W & 1))) return fail("fused 2x2 max-pool needs even H and W");
    PoolGeo pg{};
    if (pool_k && pool_geo(H, W, pool_k, pool_s, &pg)) return -1;
    const int HW = H * W;
    *route = norm_route(backward != 0, B * Cn, HW, pool_k ? KAN_NORM_POOL_K : pool2x2 ? KAN_NORM_POOL_2X2 : KAN_NORM_POOL_NONE,
                        aligned8 && norm_float2_ok(nullptr, nullptr, bstride, HW, slab_elems));
    return 0;
}

int kan_adamw_step(float* p, const float* g, float* m, float* v, long long n, double lr, double beta1, double beta2, double eps,
                   double weight_decay, int step, float grad_scale, void* stream) {
    if (!p || !g || !m || !v) return fail("null tensor pointer");
    if (n < 0 || step < 1) return fail("adamw: n must be >= 0 and step >= 1");
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15u) return fail("adamw: blocks must be 16-byte aligned");
    if (n == 0) return 0;
    const AdamArgs a = adam_args(lr, beta1, beta2, eps, weight_decay, step, grad_scale);
    long long blocks = ((n >> 2) + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;                  // 16 workgroups per CU, grid-stride beyond
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_adamw, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, a);
    return launch_ok("adamw");
}

int kan_adamw_step_segments(float* p, float* m, float* v, const unsigned long long* seg_grad, const long long* seg_off, const int* seg_n,
                            const int* chunk_seg, const int* chunk_start, const float* seg_bias, int n_chunks, int chunk_elems, double lr,
                            double beta1, double beta2, double eps, double weight_decay, int step, float grad_scale, void* stream) {
    if (!p || !m || !v || !seg_grad || !seg_off || !seg_n || !chunk_seg || !chunk_start) return fail("null tensor pointer");
    if (n_chunks < 0 || step < 1 || chunk_elems < 4 || (chunk_elems & 3)) return fail("adamw: bad chunk table or step");
    if (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15u) return fail("adamw: blocks must be 16-byte aligned");
    if (n_chunks == 0) return 0;
    const AdamArgs a = adam_args(lr, beta1, beta2, eps, weight_decay, step, grad_scale);
    hipLaunchKernelGGL(k_adamw_seg<false>, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, p, m, v, seg_grad, seg_off, seg_n, chunk_seg,
                       chunk_start, seg_bias, chunk_elems, a, (const float*)nullptr);
    return launch_ok("adamw_seg");
}

int kan_adamw_step_segments_clip(float* p, float* m, float* v, const unsigned long long* seg_grad, const long long* seg_off, const int* seg_n,
                                 const int* chunk_seg, const int* chunk_start, const float* seg_bias, int n_chunks, int chunk_elems, double lr,
                                 double beta1, double beta2, double eps, double weight_decay, int step, const float* scale_dev, void* stream) {
    if (!p || !m || !v || !seg_grad || !seg_off || !seg_n || !chunk_seg || !chunk_start || !scale_dev) return fail("null tensor pointer");
    if (n_chunks <= 0 || step < 1 || chunk_elems < 4 || (chunk_elems & 3)) return fail("adamw_clip: bad chunk table or step");
    if (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15u) return fail("adamw: blocks must be 16-byte aligned");
    if ((uintptr_t)scale_dev & 3u) return fail("adamw_clip: scale_dev must be 4-byte aligned");
    const AdamArgs a = adam_args(lr, beta1, beta2, eps, weight_decay, step, 1.0f);
    hipLaunchKernelGGL(k_adamw_seg<true>, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, p, m, v, seg_grad, seg_off, seg_n, chunk_seg,
                       chunk_start, seg_bias, chunk_elems, a, scale_dev);
    return launch_ok("adamw_seg_clip");
}

static bool adam_hyper(double beta1, double beta2, double eps, double weight_decay, float grad_scale, AdamHyper* h) {
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0)) return false;
    h->beta1 = beta1; h->beta2 = beta2; h->eps = eps; h->weight_decay = weight_decay; h->gscale = grad_scale;
    return true;
}

int kan_adamw_advance(int* seg_step, const unsigned long long* seg_grad, int n_seg, void* stream) {
    if (!seg_step || !seg_grad) return fail("null tensor pointer");
    if (n_seg < 0) return fail("adamw_advance: n_seg must be >= 0");
    if (n_seg == 0) return 0;
    hipLaunchKernelGGL(k_adamw_advance, dim3((unsigned)((n_seg + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seg_step, seg_grad, n_seg);
    return launch_ok("adamw_advance");
}

int kan_adamw_step_segments_dev(float* p, float* m, float* v, const unsigned long long* seg_grad, const long long* seg_off, const int* seg_n,
                                const int* chunk_seg, const int* chunk_start, const double* lr_dev, const int* seg_step, int n_chunks,
                                int chunk_elems, double beta1, double beta2, double eps, double weight_decay, float grad_scale, void* stream) {
    if (!p || !m || !v || !seg_grad || !seg_off || !seg_n || !chunk_seg || !chunk_start || !lr_dev || !seg_step) return fail("null tensor pointer");
    if (n_chunks < 0 || chunk_elems < 4 || (chunk_elems & 3)) return fail("adamw: bad chunk table");
    if (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15u) return fail("adamw: blocks must be 16-byte aligned");
    if (((uintptr_t)lr_dev & 7u) || ((uintptr_t)seg_step & 3u)) return fail("adamw: lr_dev must be 8-byte and seg_step 4-byte aligned");
    AdamHyper h;
    if (!adam_hyper(beta1, beta2, eps, weight_decay, grad_scale, &h)) return fail("adamw: invalid hyper-parameters");
    if (n_chunks == 0) return 0;
    hipLaunchKernelGGL(k_adamw_seg_dev<false>, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, p, m, v, seg_grad, seg_off, seg_n,
                       chunk_seg, chunk_start, lr_dev, seg_step, chunk_elems, h, (const float*)nullptr);
    return launch_ok("adamw_seg_dev");
}

int kan_adamw_step_segments_dev_clip(float* p, float* m, float* v, const unsigned long long* seg_grad, const long long* seg_off, const int* seg_n,
                                     const int* chunk_seg, const int* chunk_start, const double* lr_dev, const int* seg_step, int n_chunks,
                                     int chunk_elems, double beta1, double beta2, double eps, double weight_decay, const float* scale_dev,
                                     void* stream) {
    if (!p || !m || !v || !seg_grad || !seg_off || !seg_n || !chunk_seg || !chunk_start || !lr_dev || !seg_step || !scale_dev)
        return fail("null tensor pointer");
    if (n_chunks <= 0 || chunk_elems < 4 || (chunk_elems & 3)) return fail("adamw_clip: bad chunk table");
    if (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15u) return fail("adamw: blocks must be 16-byte aligned");
    if (((uintptr_t)lr_dev & 7u) || (((uintptr_t)seg_step | (uintptr_t)scale_dev) & 3u))
        return fail("adamw_clip: lr_dev must be 8-byte, seg_step and scale_dev 4-byte aligned");
    AdamHyper h;
    if (!adam_hyper(beta1, beta2, eps, weight_decay, 1.0f, &h)) return fail("adamw: invalid hyper-parameters");
    hipLaunchKernelGGL(k_adamw_seg_dev<true>, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, p, m, v, seg_grad, seg_off, seg_n,
                       chunk_seg, chunk_start, lr_dev, seg_step, chunk_elems, h, scale_dev);
    return launch_ok("adamw_seg_dev_clip");
}

int kan_adamw_dev_args(const double* lr_dev, const int* step_dev, double beta1, double beta2, double eps, double weight_decay, float grad_scale,
                       float* out9, void* stream) {
    if (!lr_dev || !step_dev || !out9) return fail("null tensor pointer");
    if (((uintptr_t)lr_dev & 7u) || ((uintptr_t)step_dev & 3u) || ((uintptr_t)out9 & 3u)) return fail("adamw_dev_args: misaligned pointer");
    AdamHyper h;
    if (!adam_hyper(beta1, beta2, eps, weight_decay, grad_scale, &h)) return fail("adamw: invalid hyper-parameters");
    hipLaunchKernelGGL(k_adamw_dev_args, dim3(1), dim3(64), 0, (hipStream_t)stream, lr_dev, step_dev, h, out9);
    return launch_ok("adamw_dev_args");
}

int kan_set_u64_table(unsigned long long* table, int first, const unsigned long long* values, int n, void* stream) {
    if (!table || !values) return fail("null pointer");
    if (first < 0 || n < 0 || n > 64) return fail("set_u64_table: first must be >= 0 and n in 0..64");
    if ((uintptr_t)table & 7u) return fail("set_u64_table: the table must be 8-byte aligned");
    if (n == 0) return 0;
    U64x64 vals;
    for (int i = 0; i < 64; ++i) vals.v[i] = i < n ? values[i] : 0ull;           // read NOW, on the host: the node carries the values
    hipLaunchKernelGGL(k_set_u64_table, dim3(1), dim3(64), 0, (hipStream_t)stream, table, first, n, vals);
    return launch_ok("set_u64_table");
}

}  // extern "C"
