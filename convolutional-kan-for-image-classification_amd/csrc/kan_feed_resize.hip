// Batch preparation with PIL's 8-bit bilinear resampling: the per-sample transforms of the reference loader's ImageNet branch
// (utils/dataloader.py:26-54: Resize + RandomResizedCrop / CenterCrop + RandomHorizontalFlip, or Resize + Grayscale(3), then ToTensor +
// Normalize) for a uint8 dataset that lives on the device, one launch per batch.
//
// PIL's 8-bit resampling is integer arithmetic once its coefficients are known, and the coefficients depend on lengths alone, so the HOST
// computes them in float64 (data.resample_coeffs) and the kernel does none of that work: device bytes equal PIL's bytes by construction.
// One pass from n to m samples reads, per output xx, one coefficient row (xmin, count, k[0 .. ksize)):
//       out[xx] = clip((2^21 + sum_{t < count} in[xmin + t] * k[t]) >> 22, 0, 255)                 (int32: 255 * (2^22 + ksize) + 2^21 < 2^31)
// and a resize is the horizontal pass into a uint8 image, then the vertical pass over that.  Per sample, in torchvision's order on PIL images:
//       stage 1  resize the whole H x W source to Rh x Rw               (tables k1x: Rw rows, k1y: Rh rows)
//       crop     the box (top, left, h, w) of the stage-1 image
//       stage 2  resize the h x w box to Ho x Wo                         (tables k2x / k2y: one block of Wo / Ho rows per source length 1 .. Rw / Rh)
//       flip, optional replication of one channel to three, ToTensor and Normalize through the C x 256 value table of k_feed_batch.
// Four uint8 roundings precede the float conversion.
//
//   k_feed_resize_batch   one workgroup of 256 threads per (batch row, block of RB output rows).  Only what the block's rows depend on is computed:
//       the stage-2 vertical windows of the block's rows name nv box rows, their stage-1 vertical windows name ns source rows, and
//         1. those source rows are staged in LDS (16-byte loads under k_feed_batch's rule), with the coefficient rows the passes below read;
//         A. stage-1 horizontal pass of the ns source rows, box columns only          -> uint8 tile [C][ns][w]
//         B. stage-1 vertical pass                                                    -> uint8 tile [C][nv][w]     (4 columns per thread)
//         C. stage-2 horizontal pass                                                  -> uint8 tile [C][nv][Wo]
//         D. stage-2 vertical pass of the block's rows, flip, value table, float4 stores (Wo % 4 == 0 and a 16-byte aligned output).
// Coefficient rows are trusted for values, never for addresses: every window is clamped into the tile it reads, and a block whose windows
// span more rows than its tiles hold (impossible for tables from data.resize_tables) writes zeros.  A row of the batch table is compared before
// it addresses anything: an index outside [0, N), or a box not inside the stage-1 image with h, w >= 1, gives an all-zero image and target -1.
// Plain C++: no inline assembly, no atomics; every output element has one writer and depends on its own table row alone.
#include <hip/hip_runtime.h>
#include "kanconv.h"
#include "kan_internal.h"

namespace {

constexpr int FR_NT = 256;                              // threads of a workgroup (= entries per channel of the value table)
constexpr int FR_MAX_C = 4;                             // channels (the by-value mean / std argument)
constexpr int FR_MAX_IMAGE_BYTES = 65536;               // H * W * C of one source image
constexpr int FR_MAX_KSIZE = 9;                         // taps of one coefficient row: downscaling by up to 4 in one pass
constexpr int FR_MAX_EDGE = 4096;                       // Rh, Rw, Ho, Wo
constexpr int FR_MAX_RB = 16;                           // output rows per workgroup
constexpr int FR_SLACK = 32;                            // per staged segment: up to 15 bytes before and after it, from widening to 16-byte boundaries
constexpr int FR_LDS_SOFT = 64 * 1024;                  // the row block shrinks until the workgroup fits this
constexpr int FR_LDS_HARD = 160 * 1024;                 // what a gfx950 CU has

struct ResizeNorm { float mean[FR_MAX_C], std[FR_MAX_C]; };

struct ResizeGeom {
    long long N;
    int Cn, OC, H, W, Rh, Rw, Ho, Wo, RB, n_blk, seg_stride, ns_max, nv_max;
    int st1x, st1y, st2x, st2y;                          // ints per coefficient row: ksize + 2
    int off_k1x, off_k1y, off_k2x, off_k2y, off_src, off_a, off_b, off_c;   // LDS byte offsets, each a multiple of 16
};

constexpr int align16(int v) { return (v + 15) & ~15; }
// the most inputs `outs` consecutive outputs of a pass from n <= n_max inputs to m outputs can touch: the windows of outputs y0 <= y1 span less than
// (y1 - y0) * scale + 2 * support + 1 with scale = n / m, support = max(scale, 1), both largest at n = n_max
int span_bound(int outs, int n_max, int m) {
    const long long v = ((long long)(outs - 1) * n_max + m - 1) / m + 2 * (long long)((n_max + m - 1) / m > 1 ? (n_max + m - 1) / m : 1) + 2;
    return v < n_max ? (int)v : n_max;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
// clip(acc >> 22, 0, 255) as a test of the sign and an unsigned shift and minimum.  Written as clamp(acc >> 22, 0, 255), two of these packed into
// one word select gfx950's v_ashr_pk_u8_i32, whose result the compiler then ORs with the other bytes as if its upper half were zero; on the
// MI355X bytes 2 and 3 of the words pass B packed came out wrong wherever that register had held a nonzero partial sum before.
__device__ __forceinline__ unsigned to_byte(int acc) { return acc < 0 ? 0u : min((unsigned)acc >> 22, 255u); }

template <bool VEC_OUT>
__device__ void zero_rows(float* out, int OC, size_t plane, int y0, int rows, int Wo, int tid) {
    if (VEC_OUT) {
        const int qpr = Wo >> 2, quads = OC * rows * qpr;
        for (int q = tid; q < quads; q += FR_NT) {
            const int c = q / (rows * qpr), r = q - c * rows * qpr;
            *reinterpret_cast<float4*>(out + c * plane + (size_t)y0 * Wo + 4 * (size_t)r) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
        const int n = OC * rows * Wo;
        for (int e = tid; e < n; e += FR_NT) {
            const int c = e / (rows * Wo), r = e - c * rows * Wo;
            out[c * plane + (size_t)y0 * Wo + r] = 0.f;
        }
    }
}

// VEC_IN: 16-byte staging loads; VEC_OUT: float4 stores; CL: channels_last source
template <bool CL, bool VEC_IN, bool VEC_OUT>
__global__ __launch_bounds__(FR_NT) void k_feed_resize_batch(const unsigned char* __restrict__ images, const long long* __restrict__ labels,
                                                             const int* __restrict__ table, const int* __restrict__ k1x,
                                                             const int* __restrict__ k1y, const int* __restrict__ k2x,
                                                             const int* __restrict__ k2y, ResizeNorm norm, ResizeGeom g,
                                                             float* __restrict__ data, long long* __restrict__ target) {
    extern __shared__ __align__(16) unsigned char s_raw[];
    float* s_val = reinterpret_cast<float*>(s_raw);                      // [OC][256]: byte -> normalised value
    int* s_k1x = reinterpret_cast<int*>(s_raw + g.off_k1x);              // rows left .. left + w of k1x
    int* s_k1y = reinterpret_cast<int*>(s_raw + g.off_k1y);              // rows top + v_lo .. of k1y, nv of them
    int* s_k2x = reinterpret_cast<int*>(s_raw + g.off_k2x);              // the Wo rows of k2x for source length w
    int* s_k2y = reinterpret_cast<int*>(s_raw + g.off_k2y);              // rows y0 .. of k2y for source length h
    unsigned char* s_src = s_raw + g.off_src;                            // staged source rows, seg_stride bytes per segment
    unsigned char* s_a = s_raw + g.off_a;                                // [Cn][ns][wp]
    unsigned char* s_b = s_raw + g.off_b;                                // [Cn][nv][wp]
    unsigned char* s_c = s_raw + g.off_c;                                // [Cn][nv][Wop]
    const int Cn = g.Cn, OC = g.OC, H = g.H, W = g.W, Ho = g.Ho, Wo = g.Wo;
    const int b = blockIdx.x / g.n_blk, blk = blockIdx.x - b * g.n_blk, y0 = blk * g.RB, tid = threadIdx.x;
    const int rows = min(g.RB, Ho - y0);                                 // output rows of this block
    const int* row = table + 6 * (size_t)b;
    const long long index = row[0];
    const int top = row[1], left = row[2], h = row[3], w = row[4];
    const bool flip = row[5] != 0;
    // before it addresses anything; uniform over the workgroup
    const bool row_ok = index >= 0 && index < g.N && h >= 1 && w >= 1 && h <= g.Rh && w <= g.Rw && top >= 0 && left >= 0 && top <= g.Rh - h &&
                        left <= g.Rw - w;
    const size_t plane = (size_t)Ho * Wo;
    float* out = data + (size_t)b * OC * plane;
    if (target && blk == 0 && tid == 0) target[b] = row_ok ? labels[index] : -1ll;

    // box rows [v_lo, v_lo + nv) serve the block's output rows; source rows [s_lo, s_lo + ns) serve those (windows move monotonically)
    const int* k2y_rows = k2y;
    int v_lo = 0, nv = 0, s_lo = 0, ns = 0;
    bool ok = row_ok;
    if (ok) {
        k2y_rows = k2y + ((size_t)(h - 1) * Ho + y0) * g.st2y;
        const int* last = k2y_rows + (size_t)(rows - 1) * g.st2y;
        v_lo = clampi(k2y_rows[0], 0, h - 1);
        nv = clampi(clampi(last[0], 0, h) + clampi(last[1], 0, h), v_lo + 1, h) - v_lo;
        const int* a0 = k1y + (size_t)(top + v_lo) * g.st1y;
        const int* a1 = k1y + (size_t)(top + v_lo + nv - 1) * g.st1y;
        s_lo = clampi(a0[0], 0, H - 1);
        ns = clampi(clampi(a1[0], 0, H) + clampi(a1[1], 0, H), s_lo + 1, H) - s_lo;
        ok = nv <= g.nv_max && ns <= g.ns_max;
    }
    if (!ok) {
        zero_rows<VEC_OUT>(out, OC, plane, y0, rows, Wo, tid);
        return;
    }

    {   // the value table, in ToTensor's and Normalize's operation order
#pragma clang fp contract(off)
        const float t = (float)tid / 255.0f;
        for (int c = 0; c < OC; ++c) s_val[c * 256 + tid] = (t - norm.mean[c]) / norm.std[c];
    }
    for (int i = tid; i < w * g.st1x; i += FR_NT) s_k1x[i] = k1x[(size_t)left * g.st1x + i];
    for (int i = tid; i < nv * g.st1y; i += FR_NT) s_k1y[i] = k1y[(size_t)(top + v_lo) * g.st1y + i];
    for (int i = tid; i < Wo * g.st2x; i += FR_NT) s_k2x[i] = k2x[(size_t)(w - 1) * Wo * g.st2x + i];
    for (int i = tid; i < rows * g.st2y; i += FR_NT) s_k2y[i] = k2y_rows[i];

    const int row_bytes = CL ? W * Cn : W, n_seg = CL ? 1 : Cn;
    const size_t image = (size_t)index * H * W * Cn;                     // byte offset of the image
    {
        const int len = ns * row_bytes;
        for (int s = 0; s < n_seg; ++s) {
            const size_t g0 = image + (size_t)s * H * W + (size_t)s_lo * row_bytes;     // s = 0 for channels_last
            unsigned char* dst = s_src + (size_t)s * g.seg_stride;
            if (VEC_IN) {
                const size_t a0 = g0 & ~(size_t)15, a1 = (g0 + len + 15) & ~(size_t)15;   // inside the image: it starts and ends on a 16-byte boundary
                const int n16 = (int)((a1 - a0) >> 4);
                const uint4* src = reinterpret_cast<const uint4*>(images + a0);
                for (int i = tid; i < n16; i += FR_NT) reinterpret_cast<uint4*>(dst)[i] = src[i];
            } else {
                for (int i = tid; i < len; i += FR_NT) dst[i] = images[g0 + i];
            }
        }
    }
    __syncthreads();

    const int wp = (w + 3) & ~3, Wop = (Wo + 3) & ~3;                    // tile row strides: whole 4-byte words

    // A: stage-1 horizontal pass of staged source row r at stage-1 column left + j
    {
        const int ksz = g.st1x - 2, n = Cn * ns * w;
        for (int e = tid; e < n; e += FR_NT) {
            const int c = e / (ns * w), r = (e - c * ns * w) / w, j = e - (c * ns + r) * w;
            const int* kr = s_k1x + j * g.st1x;
            const int lo = clampi(kr[0], 0, W - 1), cnt = clampi(kr[1], 0, min(ksz, W - lo));
            // the lead of a segment is the distance of its first byte from the 16-byte boundary below it
            const unsigned char* px;
            if (CL) px = s_src + (VEC_IN ? (int)((image + (size_t)s_lo * row_bytes) & 15) : 0) + (r * W + lo) * Cn + c;
            else px = s_src + c * g.seg_stride + (VEC_IN ? (int)((image + (size_t)c * H * W + (size_t)s_lo * row_bytes) & 15) : 0) + r * W + lo;
            int acc = 1 << 21;
            for (int t = 0; t < cnt; ++t) acc += (int)px[CL ? t * Cn : t] * kr[2 + t];
            s_a[(c * ns + r) * wp + j] = (unsigned char)to_byte(acc);
        }
    }
    __syncthreads();

    // B: stage-1 vertical pass, four columns per thread (the columns past w of a row hold nothing that is read as a pixel)
    {
        const int ksz = g.st1y - 2, qn = wp >> 2, n = Cn * nv * qn;
        for (int e = tid; e < n; e += FR_NT) {
            const int c = e / (nv * qn), v = (e - c * nv * qn) / qn, q = e - (c * nv + v) * qn;
            const int* kr = s_k1y + v * g.st1y;
            const int lo = clampi(clampi(kr[0], 0, H) - s_lo, 0, ns - 1), cnt = clampi(kr[1], 0, min(ksz, ns - lo));
            const unsigned char* px = s_a + (c * ns + lo) * wp + 4 * q;
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
            for (int t = 0; t < cnt; ++t) {
                const unsigned u = *reinterpret_cast<const unsigned*>(px + t * wp);
                const int k = kr[2 + t];
                a0 += (int)(u & 255u) * k;
                a1 += (int)((u >> 8) & 255u) * k;
                a2 += (int)((u >> 16) & 255u) * k;
                a3 += (int)(u >> 24) * k;
            }
            *reinterpret_cast<unsigned*>(s_b + (c * nv + v) * wp + 4 * q) = to_byte(a0) | (to_byte(a1) << 8) | (to_byte(a2) << 16) | (to_byte(a3) << 24);
        }
    }
    __syncthreads();

    // C: stage-2 horizontal pass of box row v_lo + v, box columns [0, w)
    {
        const int ksz = g.st2x - 2, n = Cn * nv * Wo;
        for (int e = tid; e < n; e += FR_NT) {
            const int cv = e / Wo, x = e - cv * Wo;
            const int* kr = s_k2x + x * g.st2x;
            const int lo = clampi(kr[0], 0, w - 1), cnt = clampi(kr[1], 0, min(ksz, w - lo));
            const unsigned char* px = s_b + cv * wp + lo;
            int acc = 1 << 21;
            for (int t = 0; t < cnt; ++t) acc += (int)px[t] * kr[2 + t];
            s_c[cv * Wop + x] = (unsigned char)to_byte(acc);
        }
    }
    __syncthreads();

    // D: stage-2 vertical pass of the block's rows, flip, replication, value table, store
    const int ksz = g.st2y - 2;
    const bool replicate = OC != Cn;                                      // one source channel to OC outputs
    if (VEC_OUT) {
        const int qpr = Wo >> 2, quads = Cn * rows * qpr;
        for (int q = tid; q < quads; q += FR_NT) {
            const int c = q / (rows * qpr), r = (q - c * rows * qpr) / qpr, x = 4 * (q - (c * rows + r) * qpr);
            const int* kr = s_k2y + r * g.st2y;
            const int lo = clampi(clampi(kr[0], 0, h) - v_lo, 0, nv - 1), cnt = clampi(kr[1], 0, min(ksz, nv - lo));
            const unsigned char* px = s_c + (c * nv + lo) * Wop + (flip ? Wo - 4 - x : x);
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
            for (int t = 0; t < cnt; ++t) {
                const unsigned u = *reinterpret_cast<const unsigned*>(px + t * Wop);
                const int k = kr[2 + t];
                a0 += (int)(u & 255u) * k;
                a1 += (int)((u >> 8) & 255u) * k;
                a2 += (int)((u >> 16) & 255u) * k;
                a3 += (int)(u >> 24) * k;
            }
            const unsigned b0 = to_byte(flip ? a3 : a0), b1 = to_byte(flip ? a2 : a1), b2 = to_byte(flip ? a1 : a2), b3 = to_byte(flip ? a0 : a3);
            for (int oc = replicate ? 0 : c; oc < (replicate ? OC : c + 1); ++oc) {
                const float* val = s_val + oc * 256;
                *reinterpret_cast<float4*>(out + oc * plane + (size_t)(y0 + r) * Wo + x) = make_float4(val[b0], val[b1], val[b2], val[b3]);
            }
        }
    } else {
        const int n = Cn * rows * Wo;
        for (int e = tid; e < n; e += FR_NT) {
            const int c = e / (rows * Wo), r = (e - c * rows * Wo) / Wo, x = e - (c * rows + r) * Wo;
            const int* kr = s_k2y + r * g.st2y;
            const int lo = clampi(clampi(kr[0], 0, h) - v_lo, 0, nv - 1), cnt = clampi(kr[1], 0, min(ksz, nv - lo));
            const unsigned char* px = s_c + (c * nv + lo) * Wop + (flip ? Wo - 1 - x : x);
            int acc = 1 << 21;
            for (int t = 0; t < cnt; ++t) acc += (int)px[t * Wop] * kr[2 + t];
            const unsigned v = to_byte(acc);
            for (int oc = replicate ? 0 : c; oc < (replicate ? OC : c + 1); ++oc) out[oc * plane + (size_t)(y0 + r) * Wo + x] = s_val[oc * 256 + v];
        }
    }
}

}  // namespace

extern "C" {

int kan_feed_resize_max_ksize(void) { return FR_MAX_KSIZE; }

int kan_feed_resize_batch(const unsigned char* images, const long long* labels, const int* table, long long N, int B, int C, int H, int W, int Rh,
                          int Rw, int Ho, int Wo, int channels_last, int out_channels, const int* k1x, int ksize1x, const int* k1y, int ksize1y,
                          const int* k2x, int ksize2x, const int* k2y, int ksize2y, const float* mean, const float* std, float* data,
                          long long* target, void* stream) {
    const char* name = "kan_feed_resize_batch: %s";
    if (!images || !table || !k1x || !k1y || !k2x || !k2y || !mean || !std || !data) return kan_fail_msg(name, "null pointer");
    if (!labels != !target) return kan_fail_msg(name, "labels and target are given together or not at all");
    if (N < 1 || B < 1 || C < 1 || H < 1 || W < 1 || Rh < 1 || Rw < 1 || Ho < 1 || Wo < 1 || ksize1x < 1 || ksize1y < 1 || ksize2x < 1 || ksize2y < 1)
        return kan_fail_msg(name, "N, B, C, H, W, Rh, Rw, Ho, Wo and every ksize must be at least 1");
    if (C > FR_MAX_C) return kan_fail_msg(name, "at most 4 channels");
    if (out_channels != C && !(out_channels == 3 && C == 1)) return kan_fail_msg(name, "out_channels is C, or 3 with C == 1");
    if ((long long)H * W * C > FR_MAX_IMAGE_BYTES) return kan_fail_msg(name, "an image may hold at most 65536 bytes (H * W * C)");
    if (ksize1x > FR_MAX_KSIZE || ksize1y > FR_MAX_KSIZE || ksize2x > FR_MAX_KSIZE || ksize2y > FR_MAX_KSIZE)
        return kan_fail_msg(name, "a ksize above 9 (one pass downscales by at most 4)");
    if (Rh > FR_MAX_EDGE || Rw > FR_MAX_EDGE || Ho > FR_MAX_EDGE || Wo > FR_MAX_EDGE) return kan_fail_msg(name, "Rh, Rw, Ho, Wo may be at most 4096");
    ResizeNorm norm;
    for (int c = 0; c < FR_MAX_C; ++c) { norm.mean[c] = c < out_channels ? mean[c] : 0.f; norm.std[c] = c < out_channels ? std[c] : 1.f; }
    ResizeGeom g;
    g.N = N; g.Cn = C; g.OC = out_channels; g.H = H; g.W = W; g.Rh = Rh; g.Rw = Rw; g.Ho = Ho; g.Wo = Wo;
    g.st1x = ksize1x + 2; g.st1y = ksize1y + 2; g.st2x = ksize2x + 2; g.st2y = ksize2y + 2;
    const int Rwp = (Rw + 3) & ~3, Wop = (Wo + 3) & ~3;
    // LDS of a workgroup of RB output rows, every tile at its largest (a box as large as the stage-1 image)
    auto layout = [&](int RB) {
        g.RB = RB;
        g.nv_max = span_bound(RB, Rh, Ho);
        g.ns_max = span_bound(g.nv_max, H, Rh);
        g.seg_stride = align16(g.ns_max * (channels_last ? W * C : W)) + FR_SLACK;
        int at = out_channels * 256 * (int)sizeof(float);
        auto take = [&](int bytes) { const int o = at; at += align16(bytes); return o; };
        g.off_k1x = take(Rw * g.st1x * 4);
        g.off_k1y = take(g.nv_max * g.st1y * 4);
        g.off_k2x = take(Wo * g.st2x * 4);
        g.off_k2y = take(RB * g.st2y * 4);
        g.off_src = take((channels_last ? 1 : C) * g.seg_stride);
        g.off_a = take(C * g.ns_max * Rwp);
        g.off_b = take(C * g.nv_max * Rwp);
        g.off_c = take(C * g.nv_max * Wop);
        return at;
    };
    int RB = Ho < FR_MAX_RB ? Ho : FR_MAX_RB;
    int lds = layout(RB);
    while (lds > FR_LDS_SOFT && RB > 1) lds = layout(RB = (RB + 1) / 2);
    if (lds > FR_LDS_HARD) return kan_fail_msg(name, "one output row needs more than the 160 KB of LDS of a compute unit");
    g.n_blk = (Ho + RB - 1) / RB;
    const bool vec_in = (long long)H * W * C % 16 == 0 && (reinterpret_cast<size_t>(images) & 15) == 0;
    const bool vec_out = Wo % 4 == 0 && (reinterpret_cast<size_t>(data) & 15) == 0;
    if ((long long)B * g.n_blk > 0x7fffffffll) return kan_fail_msg(name, "too many workgroups for one launch");
    const dim3 grid((unsigned)((long long)B * g.n_blk));
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = 0;
    auto launch = [&](auto cl, auto vi, auto vo) {
        auto k = k_feed_resize_batch<decltype(cl)::value != 0, decltype(vi)::value != 0, decltype(vo)::value != 0>;
        if (lds > 64 * 1024 && kan_raise_lds_limit((const void*)k, FR_LDS_HARD)) { rc = kan_fail_msg("kan_feed_resize_batch: cannot reserve %s of LDS", "160 KB"); return; }
        hipLaunchKernelGGL(k, grid, dim3(FR_NT), (size_t)lds, st, images, labels, table, k1x, k1y, k2x, k2y, norm, g, data, target);
    };
    pick<1, 0>(channels_last ? 1 : 0, [&](auto cl) {
        pick<1, 0>(vec_in ? 1 : 0, [&](auto vi) { pick<1, 0>(vec_out ? 1 : 0, [&](auto vo) { launch(cl, vi, vo); }); });
    });
    if (rc) return rc;
    return hipGetLastError() == hipSuccess ? 0 : kan_fail_msg("%s: launch failed", "kan_feed_resize_batch");
}

}  // extern "C"
