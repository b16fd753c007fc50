// Batch preparation from a device-resident uint8 dataset: the per-sample transforms of the reference's loader (utils/dataloader.py:56-90, the
// non-ImageNet branch: RandomCrop(S, padding=p) + RandomHorizontalFlip + ToTensor + Normalize, or ToTensor + Normalize alone) and the batching
// of its DataLoader (:111-112), one launch per batch instead of PIL transforms per sample in worker processes and an fp32 copy to the device.
//
//   k_feed_batch   one workgroup of 256 threads per (batch row, block of output rows).  Batch row b reads table[b] = (index, top, left, flip) and produces
//                      data[b][c][y][x] = norm_c(src[index][c][top + y][left + (flip ? Wo - 1 - x : x)]),   target[b] = labels[index]
//                  with src = 0 (the raw byte) outside [0, H) x [0, W): torchvision pads the uint8 image, crops, flips, then converts, so a
//                  padded pixel comes out as (0 - mean[c]) / std[c].  top / left are in unpadded source coordinates and may be negative.
//                  norm_c(v) = (float(v) / 255.0f - mean[c]) / std[c]: three correctly rounded fp32 operations in ToTensor's and Normalize's
//                  order (div, sub_, div_), taken from a C x 256 table the workgroup builds in LDS with exactly these operations -- no
//                  reciprocal, no contraction.  The kernel proper is a byte gather plus a table read:
//                    1. the source rows the block's output rows touch are staged into LDS, 16 bytes per load where the image stride and the
//                       base pointer allow it (the staged range is widened to 16-byte boundaries, which stay inside the image because the
//                       image itself starts and ends on one), byte loads otherwise;
//                    2. every thread gathers 4 consecutive output pixels from the staged bytes and stores one float4 (Wo % 4 == 0 and a
//                       16-byte aligned output), or one pixel and one float otherwise.
// An index outside [0, N) is compared against the range before it addresses anything: the row's image is all zeros (0.0f, not the padding
// value) and its target -1, which kan_xent_fwd leaves out of the loss and counts in bad_target.
// Plain C++ throughout: no inline assembly, no atomics, no floating-point reduction; every output element is written by exactly one thread from
// values that depend on its own row of the table alone, so two launches on the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include "kanconv.h"
#include "kan_internal.h"

namespace {

constexpr int FD_NT = 256;                              // threads of a workgroup (= entries per channel of the value table)
constexpr int FD_MAX_C = 4;                             // channels (the by-value mean / std argument)
constexpr int FD_MAX_IMAGE_BYTES = 65536;               // H * W * C of one image
constexpr int FD_BLOCK_BYTES = 16384;                   // source bytes a workgroup stages, when more than one source row fits
constexpr int FD_SLACK = 32;                            // per staged segment: up to 15 bytes before and after it, from widening to 16-byte boundaries

struct FeedNorm { float mean[FD_MAX_C], std[FD_MAX_C]; };

// staged LDS bytes of one segment (channels_last: the one segment of all channels; CHW: one segment per channel) holding `rows` source rows
constexpr int feed_seg_stride(int rows, int row_bytes) { return ((rows * row_bytes + 15) & ~15) + FD_SLACK; }

// RB output rows per workgroup; VEC_IN: 16-byte staging loads; VEC_OUT: float4 stores; CL: channels_last source
template <bool CL, bool VEC_IN, bool VEC_OUT>
__global__ __launch_bounds__(FD_NT) void k_feed_batch(const unsigned char* __restrict__ images, const long long* __restrict__ labels,
                                                      const int* __restrict__ table, FeedNorm norm, long long N, int Cn, int H, int W, int Ho,
                                                      int Wo, int RB, int n_blk, int seg_stride, float* __restrict__ data, long long* __restrict__ target) {
    extern __shared__ __align__(16) unsigned char s_raw[];
    float* s_val = reinterpret_cast<float*>(s_raw);                      // [Cn][256]: byte -> normalised value
    unsigned char* s_src = s_raw + (size_t)Cn * 256 * sizeof(float);     // staged source rows, seg_stride bytes per segment
    const int b = blockIdx.x / n_blk, blk = blockIdx.x - b * n_blk, y0 = blk * RB, tid = threadIdx.x;
    const int rows = min(RB, Ho - y0);                                   // output rows of this block
    const int* row = table + 4 * (size_t)b;
    const long long index = row[0];
    const bool ok = index >= 0 && index < N;                             // before it addresses anything; uniform over the workgroup
    const size_t plane = (size_t)Ho * Wo;
    float* out = data + (size_t)b * Cn * plane;
    if (target && blk == 0 && tid == 0) target[b] = ok ? labels[index] : -1ll;
    if (!ok) {
        if (VEC_OUT) {
            const int qpr = Wo >> 2, quads = Cn * rows * qpr;
            for (int q = tid; q < quads; q += FD_NT) {
                const int c = q / (rows * qpr), r = q - c * rows * qpr;
                *reinterpret_cast<float4*>(out + c * plane + (size_t)y0 * Wo + 4 * (size_t)r) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else {
            const int n = Cn * rows * Wo;
            for (int e = tid; e < n; e += FD_NT) {
                const int c = e / (rows * Wo), r = e - c * rows * Wo;
                out[c * plane + (size_t)y0 * Wo + r] = 0.f;
            }
        }
        return;
    }
    // any top <= -Ho (left <= -Wo) or >= H (W) reads padding only: clamping keeps every sum below inside int
    const int top = max(-Ho, min(row[1], H)), left = max(-Wo, min(row[2], W));
    const bool flip = row[3] != 0;

    {   // the value table, in ToTensor's and Normalize's operation order
#pragma clang fp contract(off)
        const float t = (float)tid / 255.0f;
        for (int c = 0; c < Cn; ++c) s_val[c * 256 + tid] = (t - norm.mean[c]) / norm.std[c];
    }

    // source rows [r0, r1) of the image serve output rows [y0, y0 + rows)
    const int r0 = max(0, min(top + y0, H)), r1 = max(0, min(top + y0 + rows, H));
    const int row_bytes = CL ? W * Cn : W, n_seg = CL ? 1 : Cn;
    const size_t image = (size_t)index * H * W * Cn;                     // byte offset of the image
    const int len = (r1 - r0) * row_bytes;
    if (len > 0) {
        for (int s = 0; s < n_seg; ++s) {
            const size_t g0 = image + (size_t)s * H * W + (size_t)r0 * row_bytes;       // s = 0 for channels_last
            unsigned char* dst = s_src + (size_t)s * seg_stride;
            if (VEC_IN) {
                const size_t a0 = g0 & ~(size_t)15, a1 = (g0 + len + 15) & ~(size_t)15;   // inside the image: it starts and ends on a 16-byte boundary
                const int n16 = (int)((a1 - a0) >> 4);
                const uint4* src = reinterpret_cast<const uint4*>(images + a0);
                for (int i = tid; i < n16; i += FD_NT) reinterpret_cast<uint4*>(dst)[i] = src[i];
            } else {
                for (int i = tid; i < len; i += FD_NT) dst[i] = images[g0 + i];
            }
        }
    }
    __syncthreads();

    // byte of source pixel (c, sy, sx); the lead of a segment is the distance of its first byte from the 16-byte boundary below it
    auto value = [&](int c, int sy, int sx) -> float {
        unsigned v = 0;
        if (sy >= r0 && sy < r1 && sx >= 0 && sx < W) {
            int at;
            if (CL) {
                at = (VEC_IN ? (int)((image + (size_t)r0 * row_bytes) & 15) : 0) + ((sy - r0) * W + sx) * Cn + c;
            } else {
                at = c * seg_stride + (VEC_IN ? (int)((image + (size_t)c * H * W + (size_t)r0 * row_bytes) & 15) : 0) + (sy - r0) * W + sx;
            }
            v = s_src[at];
        }
        return s_val[c * 256 + v];
    };
    if (VEC_OUT) {
        const int qpr = Wo >> 2, quads = Cn * rows * qpr;
        for (int q = tid; q < quads; q += FD_NT) {
            const int c = q / (rows * qpr), r = q - c * rows * qpr, y = y0 + r / qpr, x = 4 * (r % qpr);
            const int sy = top + y, sx = left + (flip ? Wo - 1 - x : x), dx = flip ? -1 : 1;
            float4 o;
            o.x = value(c, sy, sx);
            o.y = value(c, sy, sx + dx);
            o.z = value(c, sy, sx + 2 * dx);
            o.w = value(c, sy, sx + 3 * dx);
            *reinterpret_cast<float4*>(out + c * plane + (size_t)y * Wo + x) = o;
        }
    } else {
        const int n = Cn * rows * Wo;
        for (int e = tid; e < n; e += FD_NT) {
            const int c = e / (rows * Wo), r = e - c * rows * Wo, y = y0 + r / Wo, x = r % Wo;
            out[c * plane + (size_t)y * Wo + x] = value(c, top + y, left + (flip ? Wo - 1 - x : x));
        }
    }
}

}  // namespace

extern "C" {

long long kan_feed_max_image_bytes(void) { return FD_MAX_IMAGE_BYTES; }

int kan_feed_batch(const unsigned char* images, const long long* labels, const int* table, long long N, int B, int C, int H, int W, int Ho,
                   int Wo, int channels_last, const float* mean, const float* std, float* data, long long* target, void* stream) {
    if (!images || !table || !mean || !std || !data) return kan_fail_msg("kan_feed_batch: %s", "null pointer");
    if (!labels != !target) return kan_fail_msg("kan_feed_batch: %s", "labels and target are given together or not at all");
    if (N < 1 || B < 1 || C < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1) return kan_fail_msg("kan_feed_batch: %s", "N, B, C, H, W, Ho, Wo must be at least 1");
    if (C > FD_MAX_C) return kan_fail_msg("kan_feed_batch: %s", "at most 4 channels");
    if ((long long)H * W * C > FD_MAX_IMAGE_BYTES) return kan_fail_msg("kan_feed_batch: %s", "an image may hold at most 65536 bytes (H * W * C)");
    if ((long long)C * Ho * Wo > (1ll << 24) || (long long)Ho * Wo > (1ll << 24)) return kan_fail_msg("kan_feed_batch: %s", "an output image may hold at most 2^24 elements");
    FeedNorm norm;
    for (int c = 0; c < FD_MAX_C; ++c) { norm.mean[c] = c < C ? mean[c] : 0.f; norm.std[c] = c < C ? std[c] : 1.f; }
    const int image_bytes = H * W * C, src_row = W * C;
    // output rows per workgroup: the whole image while its source fits a block, else as many rows as source rows fit (at least one)
    int RB = Ho;
    if (image_bytes > FD_BLOCK_BYTES) RB = FD_BLOCK_BYTES / src_row > 0 ? FD_BLOCK_BYTES / src_row : 1;
    if (RB > Ho) RB = Ho;
    const int src_rows = RB < H ? RB : H;
    const int seg_stride = feed_seg_stride(src_rows, channels_last ? W * C : W);
    const int lds = C * 256 * (int)sizeof(float) + (channels_last ? 1 : C) * seg_stride;
    const bool vec_in = image_bytes % 16 == 0 && (reinterpret_cast<size_t>(images) & 15) == 0;
    const bool vec_out = Wo % 4 == 0 && (reinterpret_cast<size_t>(data) & 15) == 0;
    const int n_blk = (Ho + RB - 1) / RB;
    if ((long long)B * n_blk > 0x7fffffffll) return kan_fail_msg("kan_feed_batch: %s", "too many workgroups for one launch");
    const dim3 grid((unsigned)((long long)B * n_blk));
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = 0;
    auto launch = [&](auto cl, auto vi, auto vo) {
        auto k = k_feed_batch<decltype(cl)::value != 0, decltype(vi)::value != 0, decltype(vo)::value != 0>;
        if (lds > 64 * 1024 && kan_raise_lds_limit((const void*)k, 80 * 1024)) { rc = kan_fail_msg("kan_feed_batch: cannot reserve %s of LDS", "80 KB"); return; }
        hipLaunchKernelGGL(k, grid, dim3(FD_NT), (size_t)lds, st, images, labels, table, norm, N, C, H, W, Ho, Wo, RB, n_blk, seg_stride, data, target);
    };
    pick<1, 0>(channels_last ? 1 : 0, [&](auto cl) {
        pick<1, 0>(vec_in ? 1 : 0, [&](auto vi) { pick<1, 0>(vec_out ? 1 : 0, [&](auto vo) { launch(cl, vi, vo); }); });
    });
    if (rc) return rc;
    return hipGetLastError() == hipSuccess ? 0 : kan_fail_msg("%s: launch failed", "kan_feed_batch");
}

}  // extern "C"
