// libkanconv, OPT-IN split-precision forward (round 3), input gradient (k_split_bwd_data, further down) and weight gradient (k_split_bwd_weight, after it).  NOT on any default path: `dtype` f32 stays exact; this mode is reached only
// through its own entry points (kan_split_*), carries its own tolerance in the tests and is reported under `other_workloads` by bench.py.
//
// Every fp32 operand (expanded plane value, weight) is cut into three bf16 pieces hi + mid + lo (24 mantissa bits); each 16-deep k-block runs six
// v_mfma_f32_32x32x16_bf16 products (lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi) into the fp32 accumulator.  Scope of this first kernel: the default
// B-spline spec (grid 5, order 3, SiLU base branch: P = 9 planes) on 8x8 or 16x16 planes, 3x3 / stride 1 / pad 1, one group, C % 8 == 0, O % 128 == 0 (even
// batch on 8x8) -- KAN-VGG11's 64 -> 128 @ 16x16, 128 -> 256 and 256 -> 256 @ 8x8 layers.  Replaces, for such a layer, kan_layers.py:199-200, 203-239 (as kan_conv_fwd does).
//
// Kernel design (k_split_fwd), following the halo forward of the library:
//   tile    128 outputs x 128 pixels (two whole 8x8 images, or eight rows of one 16x16 image) per workgroup, one workgroup per CU at the VGG shapes; 512 threads = 4 MFMA waves (wave tile
//           64 x 64, 2 x 2 blocks of 32 x 32) + 4 PRODUCER waves, one of each per SIMD;
//   B side  per group of 8 input channels the producers expand the 2 x 64 input values once (SiLU + 8 B-spline planes, fp32 vector ALU), cut each
//           plane into 3 bf16 pieces (v_cvt_pk_bf16_f32 on channel pairs) and write a zero-bordered halo tile per image into LDS, plane-major inside a
//           cell: the 8 channels of one plane are 16 contiguous bytes = one lane's share of a 16-deep MFMA operand (k = 8 (lane >> 5) + j), so every tap
//           reads the SAME tile through a shifted address with one ds_read_b128 per piece and block.  Cell = 9 chunks of 16 B (odd: 8 consecutive pixels
//           hit 8 different 16-byte slots), rows of 88 chunks (= 8 mod 16: the four lane groups of ds_read_b128 each cover all 16 slots; the right border
//           cell of a row overlaps the left border cell of the next -- both zero, never written).  The next group's pieces are computed into registers
//           WHILE the current group is contracted and written in the last step of the group (the MFMA waves hold that step's operands in registers);
//   depth   per channel group 81 (tap, plane) k-groups of 8 (+ 3 zero groups = 42 steps of 16); lanes 0-31 and 32-63 of a step read DIFFERENT
//           k-groups (own shift each, a compile-time constant per step: the 21 step pairs of a group are unrolled);
//   A side  weights pre-cut (kan_split_pack_weights) into [step][piece][k-half][output][8 bf16] and streamed by 16-byte LDS-DMA into a ring of six
//           one-step buffers (12 KB per step) by the PRODUCER waves, six steps ahead; one barrier per TWO steps (48 MFMAs per wave), entered by the
//           producers under a counted s_waitcnt vmcnt(6) and issued as a bare s_barrier (__syncthreads() drains vmcnt to 0: the L2 latency of the
//           newest copies then sits on the critical path at any ring depth);
//   loop    explicit ISA: the 24 MFMAs of a step with the 12 ds_read_b128 of the NEXT step placed one per MFMA gap.
// tools/probe/split_bf16_conv.hip is the stand-alone A/B harness this kernel was developed in (cycles per step of every design step: its header).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdint>
#include "kanconv.h"
#include "kan_device.h"
#include "kan_common.h"
#include "kan_internal.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16s __attribute__((ext_vector_type(16)));
typedef float f32x4s __attribute__((ext_vector_type(4)));
#define f32x16 f32x16s
#define f32x4 f32x4s
#define BF(v) __builtin_bit_cast(bf16x8, v)
#define BAR_PLAIN() asm volatile("s_barrier" ::: "memory")
#define BAR_LDS() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

constexpr int NP = 9, CG = 8, NGRP = 84, NSTEP = NGRP / 2;
constexpr int CELLC = 9;                                             // chunks (16 B) per cell
// Pixel tile = 128 pixels: two whole 8x8 images (PW = 8: 2 x 10 halo rows of 10 cells) or eight rows of one 16x16 image (PW = 16: 10 halo rows of 18
// cells, the outer two real data or image border depending on the half).  Row pitch in chunks: the right border cell of a row overlaps the left border
// cell of the next (both zero, never written); 88 = 8 mod 16 for 8-pixel rows and 160 = 0 mod 16 for 16-pixel rows make the four lane groups of a
// ds_read_b128 (two / one image rows of a 32-pixel block each) cover all sixteen 16-byte slots.
template <int PW> struct SplitGeo {
    static constexpr int ROWC = PW == 8 ? 88 : 160, ROWS = PW == 8 ? 20 : 10, HWP = PW * PW;
    static constexpr int SPLITB = (ROWS * ROWC + 2) * 16, HALOB = 3 * SPLITB;      // bytes per piece (+ the overhang of the last border cell), per halo tile
};
constexpr int WSLOT = 3 * 2 * 128 * 16, NBUF = 6;                    // one step of one 128-output tile in LDS
template <int PW> constexpr int lds_bytes() { return SplitGeo<PW>::HALOB + NBUF * WSLOT + NGRP * 4 + 64; }

template <int ROWC> __device__ constexpr int off_of(int gi) { return gi < 81 ? (((gi / 9) / 3 - 1) * ROWC + ((gi / 9) % 3 - 1) * CELLC + gi % 9) * 16 : 0; }
__device__ inline int split_mfma_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }
#define mfma_row split_mfma_row

__device__ inline void split3(float v, __bf16& h, __bf16& m, __bf16& l) {
    h = (__bf16)v; const float r1 = v - (float)h;
    m = (__bf16)r1; const float r2 = r1 - (float)m;
    l = (__bf16)r2;
}

// two values -> three packed bf16 pairs (v_cvt_pk_bf16_f32 rounds to nearest even; a bf16 widens to fp32 by a shift / mask)
__device__ __forceinline__ void split_pair(float v0, float v1, unsigned& h, unsigned& m, unsigned& l) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    auto pk = [](float a, float b) { f32x2 f = {a, b}; return __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2)); };
    h = pk(v0, v1);
    const float r0 = v0 - __builtin_bit_cast(float, h << 16), r1 = v1 - __builtin_bit_cast(float, h & 0xffff0000u);
    m = pk(r0, r1);
    l = pk(r0 - __builtin_bit_cast(float, m << 16), r1 - __builtin_bit_cast(float, m & 0xffff0000u));
}

// ---- weights: reference layout (base [O][C][3][3], spline [O][C*8][3][3], channel c*8+k) -> wc[cg][step][piece][k-half][o][8 bf16]
__global__ void k_cut_weights(const float* __restrict__ wb, const float* __restrict__ ws, __bf16* __restrict__ wc, int NC, int NO) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;             // (cg, step, kh, o)
    if (idx >= (NC / CG) * NSTEP * 2 * NO) return;
    const int o = idx % NO, kh = (idx / NO) & 1, st = (idx / (2 * NO)) % NSTEP, cg = idx / (2 * NO * NSTEP);
    const int gi = 2 * st + kh;
    bf16x8 h, m, l;
    for (int j = 0; j < 8; ++j) {
        float v = 0.f;
        if (gi < 81) {
            const int tap = gi / 9, p = gi % 9, c = cg * CG + j;
            v = p == 0 ? wb[((size_t)o * NC + c) * 9 + tap] : ws[((size_t)o * NC * 8 + c * 8 + (p - 1)) * 9 + tap];
        }
        __bf16 a, b, d; split3(v, a, b, d); h[j] = a; m[j] = b; l[j] = d;
    }
    const size_t step = (size_t)cg * NSTEP + st;
    bf16x8* dst = (bf16x8*)wc;
    dst[((step * 3 + 0) * 2 + kh) * NO + o] = h;
    dst[((step * 3 + 1) * 2 + kh) * NO + o] = m;
    dst[((step * 3 + 2) * 2 + kh) * NO + o] = l;
}

// ---- the forward
template <int PW>
__global__ __launch_bounds__(512, 1) void k_split_fwd(const float* __restrict__ x, const __bf16* __restrict__ wc, float* __restrict__ z, DevBasis bs, int NC, int NO, int o_tiles) {
    const int NCG = NC / CG, TOTAL_STEPS = NCG * NSTEP, WSTEP_G = 3 * 2 * NO * 16;        // channel groups, 16-deep steps, bytes of one step of the cut weights
    constexpr int ROWC = SplitGeo<PW>::ROWC, SPLITB = SplitGeo<PW>::SPLITB, HALOB = SplitGeo<PW>::HALOB, HW = SplitGeo<PW>::HWP;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sH = smem;
    unsigned char* sW = smem + HALOB;
    int* sOff = (int*)(smem + HALOB + NBUF * WSLOT);
    float* sTab = (float*)(sOff + NGRP);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w_o = wave & 1, w_p = wave >> 1, kh = lane >> 5, m = lane & 31;
    const int ot = blockIdx.x % o_tiles, ptile = blockIdx.x / o_tiles;
    const int b0 = PW == 8 ? ptile * 2 : ptile >> 1, half_img = PW == 8 ? 0 : (ptile & 1);      // PW = 16: image b0, rows [8 half_img, 8 half_img + 8)

    for (int i = tid; i < HALOB / 16; i += 512) ((uint4*)sH)[i] = uint4{0u, 0u, 0u, 0u};
    if (tid < NGRP) {
        int off = 0;
        if (tid < 81) { const int tap = tid / 9, p = tid % 9, dr = tap / 3 - 1, dc = tap % 3 - 1; off = (dr * ROWC + dc * CELLC + p) * 16; }
        sOff[tid] = off;
    }
    if (tid < 16) sTab[tid] = bs.tab[tid];

    // weight stream: 3 chunks of 16 B per thread and step
    const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(wc), 0, (int)((long long)TOTAL_STEPS * WSTEP_G), 0x00020000);
    unsigned voff[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { const int q = (tid & 255) + 256 * j, sk = q >> 7, o = q & 127; voff[j] = (unsigned)((sk * NO + ot * 128 + o) * 16); }
    auto issue2 = [&](int t, int slot) {
        unsigned char* dst = sW + (slot % NBUF) * WSLOT + (wave & 3) * 1024;
        const int so = __builtin_amdgcn_readfirstlane(t * WSTEP_G);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (__attribute__((address_space(3))) void*)(dst + j * 4096), 16, (int)voff[j], so, 0, 0);
    };

    // operand addresses (bytes from smem)
    unsigned bBase[2];
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
        const int lp = bj * 32 + m;
        const int hrow = PW == 8 ? w_p * 10 + (lp >> 3) + 1 : w_p * 4 + (lp >> 4) + 1, c = PW == 8 ? (lp & 7) : (lp & 15);      // halo row, column
        bBase[bj] = (unsigned)((hrow * ROWC + (c + 1) * CELLC) * 16);
    }
    const unsigned aLane = (unsigned)(HALOB + (kh * 128 + w_o * 64 + m) * 16);

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    // expansion: thread = (pixel q of the 128, half hh of the channel group)
    const int q = tid & 127, hh = (tid >> 7) & 1, qi = q >> 6, lp = q & 63;
    const unsigned cellB = PW == 8 ? (unsigned)(((qi * 10 + (lp >> 3) + 1) * ROWC + ((lp & 7) + 1) * CELLC) * 16 + hh * 8)
                                   : (unsigned)((((q >> 4) + 1) * ROWC + ((q & 15) + 1) * CELLC) * 16 + hh * 8);
    const float* xq = PW == 8 ? x + ((size_t)(b0 + qi) * NC + hh * 4) * HW + lp : x + ((size_t)b0 * NC + hh * 4) * HW + half_img * 128 + q;
    // PW = 16: the ninth real row of the tile (image row 8 below the upper half, row 7 above the lower half) -- 16 pixels x 2 channel halves, lanes q < 16
    const bool extra = PW == 16 && q < 16;
    const unsigned cellX = (unsigned)(((half_img ? 0 : 9) * ROWC + (q + 1) * CELLC) * 16 + hh * 8);
    const float* xqx = x + ((size_t)b0 * NC + hh * 4) * HW + (half_img ? 7 : 8) * 16 + (q & 15);

    // PRODUCER waves (4 .. 7, one per SIMD next to an MFMA wave): the hardware issues their vector work in the MFMA waves' gaps.  They compute the
    // next channel group's pieces into registers while the current group is contracted, and write them once the halo tile is free.
    struct Pieces { uint2 h[NP], m[NP], l[NP]; };          // per plane: the 4 channels' pieces, packed bf16 pairs (ch0 ch1 | ch2 ch3)
    auto compute = [&](int cg, Pieces& pc, const float* xsrc) {
        float v[4][NP];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xv = xsrc[(size_t)(cg * CG + j) * HW];
            v[j][0] = xv * kan_rcp(1.0f + kan_exp2k(xv, -1.44269504088896340736f));      // SiLU through hardware exp2 / rcp, as the library's fast specs
            int j0 = 0; float N[4];
            const bool ok = bspline_uniform<false>(3, xv, sTab, 12, bs.inv_h, j0, N);
            const int e = ok ? -j0 : 64;                     // plane p holds basis p - 1: N[p - 1 + e] where that index is 0..3, else zero
            bool mk[11];
#pragma unroll
            for (int k = 0; k < 11; ++k) mk[k] = e == k - 7;
#pragma unroll
            for (int p = 1; p < NP; ++p) {
                float val = 0.f;
                val = mk[8 - p] ? N[0] : val; val = mk[9 - p] ? N[1] : val; val = mk[10 - p] ? N[2] : val;
                if (11 - p <= 10) val = mk[11 - p] ? N[3] : val;
                v[j][p] = val;
            }
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            split_pair(v[0][p], v[1][p], pc.h[p].x, pc.m[p].x, pc.l[p].x);
            split_pair(v[2][p], v[3][p], pc.h[p].y, pc.m[p].y, pc.l[p].y);
        }
    };
    auto write = [&](const Pieces& pc, unsigned cellB) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            *(uint2*)(sH + cellB + p * 16) = pc.h[p];
            *(uint2*)(sH + SPLITB + cellB + p * 16) = pc.m[p];
            *(uint2*)(sH + 2 * SPLITB + cellB + p * 16) = pc.l[p];
        }
    };
    if (tid >= 256) {
        // producers also stream the weights (the MFMA waves issue no vector-memory instruction at all in the main loop): steps t+6, t+7 go out at the
        // barrier of pair t, and that barrier is entered only when all but the six newest copies (steps t+4, t+5) have landed
        Pieces pc, px;                                     // px: the extra halo row of a 16x16 tile (lanes q < 16)
        for (int i = 0; i < NBUF; ++i) issue2(i, i);
        __syncthreads();                                   // B1: zero fill, tables
        compute(0, pc, xq); write(pc, cellB);
        if (extra) { compute(0, px, xqx); write(px, cellX); }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                   // B2
        int t = 0;
#pragma unroll 1
        for (int cg = 0; cg < NCG; ++cg) {
            const bool more = cg + 1 < NCG;
            if (more) { compute(cg + 1, pc, xq); if (extra) compute(cg + 1, px, xqx); }
#pragma unroll
            for (int pr = 0; pr < NSTEP / 2; ++pr) {
                if (t + 4 < TOTAL_STEPS) asm volatile("s_waitcnt vmcnt(6)\n\ts_barrier" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
                if (t + 6 < TOTAL_STEPS) { issue2(t + 6, 2 * pr); issue2(t + 7, 2 * pr + 1); }
                t += 2;
            }
            if (more) { write(pc, cellB); if (extra) write(px, cellX); BAR_LDS(); }
        }
        return;
    }
    // Operand fetch in explicit ISA (as the library's kernels): the 12 ds_read_b128 of step t+1 are issued BEFORE the 24 MFMAs of step t, so the
    // LDS phase of the four waves (one per SIMD) hides behind the matrix phase instead of alternating with it.
    struct Frag { f32x4 a[3][2], b[3][2]; };
#define DSR(d, addr, imm) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(d) : "v"(addr), "n"(imm) : "memory")
#define FRAG_REGS(f) "+v"(f.a[0][0]), "+v"(f.a[0][1]), "+v"(f.a[1][0]), "+v"(f.a[1][1]), "+v"(f.a[2][0]), "+v"(f.a[2][1]), \
                     "+v"(f.b[0][0]), "+v"(f.b[0][1]), "+v"(f.b[1][0]), "+v"(f.b[1][1]), "+v"(f.b[2][0]), "+v"(f.b[2][1])
    auto loadF = [&](Frag& f, int tt, int st) {
        const unsigned ao = aLane + (unsigned)((tt % NBUF) * WSLOT);
        const unsigned off = (unsigned)(kh ? off_of<ROWC>(2 * st + 1) : off_of<ROWC>(2 * st));
        const unsigned p0 = bBase[0] + off, p1 = bBase[1] + off, q0 = p0 + 2 * SPLITB, q1 = p1 + 2 * SPLITB;
        DSR(f.a[0][0], ao, 0);    DSR(f.a[0][1], ao, 512);
        DSR(f.b[0][0], p0, 0);    DSR(f.b[0][1], p1, 0);
        DSR(f.a[1][0], ao, 4096); DSR(f.a[1][1], ao, 4608);
        DSR(f.b[1][0], p0, SPLITB); DSR(f.b[1][1], p1, SPLITB);
        DSR(f.a[2][0], ao, 8192); DSR(f.a[2][1], ao, 8704);
        DSR(f.b[2][0], q0, 0);    DSR(f.b[2][1], q1, 0);
    };
    // One 16-deep step in explicit ISA: 24 MFMAs (product-major, smallest products first: every accumulator sees lo*hi, hi*lo, mid*mid, mid*hi, hi*mid,
    // hi*hi in that order), with the 12 operand reads of the NEXT step and the weight DMA of a later pair placed one per MFMA gap.
#define MF(i, j, A, Bv) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc[i][j]) : "v"(A), "v"(Bv) : "memory")
#define MF4(A0, A1, B0, B1) MF(0, 0, A0, B0); G(); MF(0, 1, A0, B1); G(); MF(1, 0, A1, B0); G(); MF(1, 1, A1, B1); G()
    auto step = [&](Frag& c, Frag& n, bool load_next, int tt_next, int st_next, int dma_t, int dma_slot) {
        unsigned ao = 0, p0 = 0, p1 = 0, q0 = 0, q1 = 0;
        if (load_next) {
            ao = aLane + (unsigned)((tt_next % NBUF) * WSLOT);
            const unsigned off = (unsigned)(kh ? off_of<ROWC>(2 * st_next + 1) : off_of<ROWC>(2 * st_next));
            p0 = bBase[0] + off; p1 = bBase[1] + off; q0 = p0 + 2 * SPLITB; q1 = p1 + 2 * SPLITB;
        }
        int gap = 0;
        auto G = [&]() {
            if (load_next) {
                switch (gap) {
                    case 0: DSR(n.a[0][0], ao, 0); break;        case 1: DSR(n.a[0][1], ao, 512); break;
                    case 2: DSR(n.b[0][0], p0, 0); break;        case 3: DSR(n.b[0][1], p1, 0); break;
                    case 4: DSR(n.a[1][0], ao, 4096); break;     case 5: DSR(n.a[1][1], ao, 4608); break;
                    case 6: DSR(n.b[1][0], p0, SPLITB); break;   case 7: DSR(n.b[1][1], p1, SPLITB); break;
                    case 8: DSR(n.a[2][0], ao, 8192); break;     case 9: DSR(n.a[2][1], ao, 8704); break;
                    case 10: DSR(n.b[2][0], q0, 0); break;       case 11: DSR(n.b[2][1], q1, 0); break;
                    default: break;
                }
            }
            if (dma_t >= 0 && dma_t < TOTAL_STEPS) { if (gap == 13) issue2(dma_t, dma_slot); if (gap == 17) issue2(dma_t + 1, dma_slot + 1); }
            ++gap;
        };
        asm volatile("s_waitcnt lgkmcnt(0)" : FRAG_REGS(c) :: "memory");
        MF4(c.a[2][0], c.a[2][1], c.b[0][0], c.b[0][1]);
        MF4(c.a[0][0], c.a[0][1], c.b[2][0], c.b[2][1]);
        MF4(c.a[1][0], c.a[1][1], c.b[1][0], c.b[1][1]);
        MF4(c.a[1][0], c.a[1][1], c.b[0][0], c.b[0][1]);
        MF4(c.a[0][0], c.a[0][1], c.b[1][0], c.b[1][1]);
        MF4(c.a[0][0], c.a[0][1], c.b[0][0], c.b[0][1]);
    };
    __builtin_amdgcn_s_setprio(3);                         // the MFMA wave wins the issue arbitration of its SIMD; the producer fills what is left
    Frag F0, F1;
    static_assert(NSTEP % NBUF == 0, "buffer slots repeat per channel group");
    __syncthreads();                                       // B1
    __syncthreads();                                       // B2: halo tile of group 0 written, steps 0..5 landed
    loadF(F0, 0, 0);
    int t = 0;
#pragma unroll 1
    for (int cg = 0; cg < NCG; ++cg) {
#pragma unroll
        for (int pr = 0; pr < NSTEP / 2; ++pr) {
            const bool last = pr == NSTEP / 2 - 1;
            step(F0, F1, true, 2 * pr + 1, 2 * pr + 1, -1, 0);
            asm volatile("s_waitcnt lgkmcnt(0)" : FRAG_REGS(F1) :: "memory");
            // all but the six newest copies (steps t+4, t+5) done: steps t+2, t+3 have landed ... for every thread after the barrier; every MFMA wave
            // holds steps t, t+1 in registers: their buffers are free.  (A bare s_barrier: __syncthreads() makes the compiler drain vmcnt to 0,
            // which puts the whole L2 latency of the newest copies on the critical path whatever the ring depth.)
            BAR_PLAIN();
            step(F1, F0, !last, 2 * pr + 2, 2 * pr + 2, -1, 0);  // (last pair: the producers write the next group's halo tile meanwhile)
            if (last && cg + 1 < NCG) { BAR_PLAIN(); loadF(F0, 0, 0); }
            t += 2;
        }
    }
    // ---- store: column (lane) = pixel
    float* zi = PW == 8 ? z + ((size_t)(b0 + w_p) * NO + ot * 128 + w_o * 64) * HW
                        : z + ((size_t)b0 * NO + ot * 128 + w_o * 64) * HW + half_img * 128 + w_p * 64;      // (16-pixel rows: a block's 32 pixels are contiguous)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) zi[(size_t)(i * 32 + mfma_row(r, lane)) * HW + j * 32 + m] = acc[i][j][r];
}

// ---- the input gradient (k_split_bwd_data): what kan_conv_bwd_data computes for a layer in scope, G = dgrad(dz, W_p) per plane, dx = sum_p plane_p'(x) G_p,
// into ONE slab, every element written once.  The forward's loop turned round:
//   tile    128 rows x 128 pixels per workgroup, 512 threads = 4 MFMA waves (64 x 64 each) + 4 producer waves.  Rows = two 64-row halves of 7 channels x 9
//           planes (+ one zero row): the `wd` tile of the exact kernel, each MFMA wave row owns whole channels for the epilogue.  Pixels: as the forward (two
//           8x8 images or eight rows of a 16x16 image), but ordered so that 16 consecutive columns are ONE lane group of a ds_read_b128: on 8x8 planes column
//           n = 16 row + 8 image + col (the same row of both images), on 16x16 planes one image row;
//   depth   per group of 16 output channels 9 steps of 16: step = tap, k-half = o-octet.  No zero padding; both k-halves of a step share the tap shift;
//   B side  raw dz: the producers load the group's 16 x 128 fp32 values (8 per thread), cut them (split_pair) and write a zero-bordered halo tile per piece and
//           o-octet, ONE 16-byte chunk per cell (the 8 consecutive o of a lane's operand share).  Every tap reads the same tile through a shifted address,
//           shift = -(r - 1) rows - (t - 1) cells (the forward's with the sign turned).  Row pitch: 16x16 planes 17 chunks (the 16 cells of a lane group are
//           consecutive: all sixteen 16-byte slots; the right border cell overlaps the next row's left one); 8x8 planes 9 chunks per image with the second
//           image 104 = 8 mod 16 chunks behind the first (its 8 cells take the other 8 slots).  The tile is small (16 / 18 KB for all six planes), so there
//           are TWO: group g + 1 is written while group g is contracted, and no step waits for a halo write;
//   A side  weights pre-cut (kan_split_pack_weights_bwd_data) into wcd[row tile][step][piece][k-half][row][8 bf16 of consecutive o], streamed by 16-byte
//           LDS-DMA into the forward's ring of six one-step buffers, under the same counted waits; one barrier per two steps.  18 steps (two groups) are
//           unrolled, so ring slot, halo buffer and tap shift of every step are compile-time;
//   loop    the forward's explicit-ISA step: 24 MFMAs, smallest products first, the 12 ds_read_b128 of the next step one per MFMA gap;
//   end     accumulators -> LDS (the ring's space), all 512 threads contract the 9 planes of their (channel, pixel) pairs with stage_unit_grad (the exact
//           kernel's derivative values) and store dx; the x values are requested before the LDS round trip.  Rows of padding channels are never stored.
constexpr int BD_CH = 7, BD_TCH = 2 * BD_CH, BD_TP = 132;            // channels per 64-row half / per row tile; pitch (floats) of the G tile in the epilogue
template <int PW> struct BwdGeo {
    static constexpr int PITCH = PW == 8 ? 9 : 17, IMG1 = 104;       // chunks per halo row; PW = 8: chunk offset of the second image
    static constexpr int TILEC = PW == 8 ? 196 : 172;                // chunks of one (piece, o-octet) tile: 10 halo rows (+ the overhang of the last border cell)
    static constexpr int TILEB = TILEC * 16, HALOB = 6 * TILEB, HWP = PW * PW;
    __device__ static constexpr int cell(int n) {                    // chunk of tile column n (0..127)
        return PW == 8 ? ((n >> 3) & 1) * IMG1 + ((n >> 4) + 1) * PITCH + (n & 7) + 1 : ((n >> 4) + 1) * PITCH + (n & 15) + 1;
    }
};
template <int PW> constexpr int lds_bytes_bwd() { return NBUF * WSLOT + 2 * BwdGeo<PW>::HALOB + 64; }
static_assert(128 * BD_TP * 4 <= NBUF * WSLOT, "the G tile of the epilogue fits the weight ring");
inline int bwd_row_tiles(int C) { return (C + BD_TCH - 1) / BD_TCH; }

// ---- weights: reference layout -> wcd[row tile][step = (o / 16) * 9 + tap][piece][k-half][row][8 bf16: o = 16 (o / 16) + 8 k-half + j];
// row = 64 half + 9 channel + plane, channel c = 14 tile + 7 half + channel; rows 63 / 127 and rows of channels >= C are zero
__global__ void k_cut_weights_bwd_data(const float* __restrict__ wb, const float* __restrict__ ws, __bf16* __restrict__ wcd, int NC, int NO, int c_tiles) {
    const int steps = (NO / 16) * 9;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;             // (row tile, step, kh, row)
    if (idx >= c_tiles * steps * 2 * 128) return;
    const int row = idx & 127, kh = (idx >> 7) & 1, st = (idx >> 8) % steps, ct = (idx >> 8) / steps;
    const int tap = st % 9, o0 = (st / 9) * 16 + kh * 8, rr = row & 63, c = ct * BD_TCH + (row >> 6) * BD_CH + rr / NP, p = rr % NP;
    bf16x8 h, m, l;
    for (int j = 0; j < 8; ++j) {
        float v = 0.f;
        if (rr < BD_CH * NP && c < NC) {
            const int o = o0 + j;
            v = p == 0 ? wb[((size_t)o * NC + c) * 9 + tap] : ws[((size_t)o * NC * 8 + c * 8 + (p - 1)) * 9 + tap];
        }
        __bf16 a, b, d; split3(v, a, b, d); h[j] = a; m[j] = b; l[j] = d;
    }
    const size_t step = (size_t)ct * steps + st;
    bf16x8* dst = (bf16x8*)wcd;
    dst[((step * 3 + 0) * 2 + kh) * 128 + row] = h;
    dst[((step * 3 + 1) * 2 + kh) * 128 + row] = m;
    dst[((step * 3 + 2) * 2 + kh) * 128 + row] = l;
}

template <int PW>
__global__ __launch_bounds__(512, 1) void k_split_bwd_data(const float* __restrict__ dz, const float* __restrict__ x, const __bf16* __restrict__ wcd, float* __restrict__ dx, DevBasis bs, int NC, int NO, int c_tiles) {
    using Gm = BwdGeo<PW>;
    constexpr int PITCH = Gm::PITCH, TILEB = Gm::TILEB, HALOB = Gm::HALOB, HW = Gm::HWP, RINGB = NBUF * WSLOT;
    const int NOG = NO / 16, TOTAL_STEPS = NOG * 9;                        // groups of 16 output channels (even: O % 128 == 0), 16-deep steps
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sW = smem;                                              // weight ring; the G tile of the epilogue afterwards
    unsigned char* sH = smem + RINGB;                                      // two halo buffers of [piece][o-octet] tiles
    float* sTab = (float*)(smem + RINGB + 2 * HALOB);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w_o = wave & 1, w_p = (wave >> 1) & 1, kh = lane >> 5, m = lane & 31;
    const int ct = blockIdx.x % c_tiles, ptile = blockIdx.x / c_tiles;
    const int b0 = PW == 8 ? ptile * 2 : ptile >> 1, half_img = PW == 8 ? 0 : (ptile & 1);      // PW = 16: image b0, rows [8 half_img, 8 half_img + 8)

    for (int i = tid; i < 2 * HALOB / 16; i += 512) ((uint4*)sH)[i] = uint4{0u, 0u, 0u, 0u};
    if (tid < 16) sTab[tid] = bs.tab[tid];

    // weight stream: 3 chunks of 16 B per producer thread and step (a step of a row tile is 12 KB contiguous)
    const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(wcd), 0, (int)((long long)c_tiles * TOTAL_STEPS * WSLOT), 0x00020000);
    auto issue2 = [&](int t, int slot) {
        unsigned char* dst = sW + (slot % NBUF) * WSLOT + (wave & 3) * 1024;
        const int so = __builtin_amdgcn_readfirstlane((ct * TOTAL_STEPS + t) * WSLOT);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (__attribute__((address_space(3))) void*)(dst + j * 4096), 16, (int)(((tid & 255) + 256 * j) * 16), so, 0, 0);
    };

    // epilogue units: thread = (tile column en, channel slot tid >> 7 of four), channels slot, slot + 4, ...
    const int en = tid & 127;
    const size_t epix = PW == 8 ? (size_t)(b0 + ((en >> 3) & 1)) * NC * HW + (en >> 4) * 8 + (en & 7) : (size_t)b0 * NC * HW + half_img * 128 + en;

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    if (tid >= 256) {
        // PRODUCER waves: thread = (tile column q, o-octet hh); per group 8 dz values -> three 16-byte chunks.  They also stream the weights, exactly as
        // the forward's: steps t+6, t+7 go out after the barrier of pair t, which is entered only when all but the six newest copies have landed.  The dz
        // loads of a group are issued BEFORE the copies of their pair, so the counted wait of the next barrier covers them too.
        const int q = en, hh = (tid >> 7) & 1;
        const unsigned cellB = (unsigned)(hh * TILEB + Gm::cell(q) * 16);
        const float* dzq = PW == 8 ? dz + ((size_t)(b0 + ((q >> 3) & 1)) * NO + hh * 8) * HW + (q >> 4) * 8 + (q & 7) : dz + ((size_t)b0 * NO + hh * 8) * HW + half_img * 128 + q;
        // PW = 16: the ninth real row of the tile (image row 8 below the upper half: halo row 9; row 7 above the lower half: halo row 0), lanes q < 16
        const bool extra = PW == 16 && q < 16;
        const unsigned cellX = (unsigned)(hh * TILEB + ((half_img ? 0 : 9) * PITCH + (q & 15) + 1) * 16);
        const float* dzx = dz + ((size_t)b0 * NO + hh * 8) * HW + (half_img ? 7 : 8) * 16 + (q & 15);
        auto load = [&](int og, float (&v)[8], const float* src) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = src[(size_t)(og * 16 + j) * HW];
        };
        auto cutwrite = [&](const float (&v)[8], int buf, unsigned cellb) {
            uint4 h, md, l;
            split_pair(v[0], v[1], h.x, md.x, l.x); split_pair(v[2], v[3], h.y, md.y, l.y);
            split_pair(v[4], v[5], h.z, md.z, l.z); split_pair(v[6], v[7], h.w, md.w, l.w);
            unsigned char* d = sH + buf * HALOB + cellb;
            *(uint4*)d = h; *(uint4*)(d + 2 * TILEB) = md; *(uint4*)(d + 4 * TILEB) = l;
        };
        float dv[8], dxv[8];
        for (int i = 0; i < NBUF; ++i) issue2(i, i);
        __syncthreads();                                   // B1: zero fill, tables
        load(0, dv, dzq); cutwrite(dv, 0, cellB);
        if (extra) { load(0, dxv, dzx); cutwrite(dxv, 0, cellX); }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                   // B2
        int t = 0;
#pragma unroll 1
        for (int gg = 0; gg < NOG / 2; ++gg) {             // groups 2 gg (halo buffer 0) and 2 gg + 1 (buffer 1)
            const bool more = gg + 1 < NOG / 2;
#pragma unroll
            for (int pr = 0; pr < 9; ++pr) {
                if (t + 4 < TOTAL_STEPS) asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)\n\ts_barrier" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
                // buffer 1 is read from the step before barrier 4 on and free since barrier 8 of the previous round; buffer 0 is read until barrier 4
                // and again after barrier 8: written after barriers 1 and 6, complete (lgkmcnt(0) above) at barriers 2 and 7
                if (pr == 1) { cutwrite(dv, 1, cellB); if (extra) cutwrite(dxv, 1, cellX); }
                if (pr == 6 && more) { cutwrite(dv, 0, cellB); if (extra) cutwrite(dxv, 0, cellX); }
                if (pr == 0) { load(2 * gg + 1, dv, dzq); if (extra) load(2 * gg + 1, dxv, dzx); }
                if (pr == 5 && more) { load(2 * gg + 2, dv, dzq); if (extra) load(2 * gg + 2, dxv, dzx); }
                if (t + 6 < TOTAL_STEPS) { issue2(t + 6, 2 * pr); issue2(t + 7, 2 * pr + 1); }
                t += 2;
            }
        }
    } else {
        // operand addresses (bytes from smem): the tap shift and the halo buffer are added per step (compile-time)
        unsigned bBase[2];
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) bBase[bj] = (unsigned)(RINGB + kh * TILEB + Gm::cell(w_p * 64 + bj * 32 + m) * 16);
        const unsigned aLane = (unsigned)((kh * 128 + w_o * 64 + m) * 16);
        struct Frag { f32x4 a[3][2], b[3][2]; };
        // step s of the 18 of a round: ring slot s % 6, halo buffer s / 9, tap s % 9
        auto b_off = [](int s) { const int tap = s % 9; return (s / 9) * HALOB - ((tap / 3 - 1) * PITCH + (tap % 3 - 1)) * 16; };
        auto loadF = [&](Frag& f, int s) {
            const unsigned ao = aLane + (unsigned)((s % NBUF) * WSLOT);
            const unsigned p0 = bBase[0] + (unsigned)b_off(s), p1 = bBase[1] + (unsigned)b_off(s);
            DSR(f.a[0][0], ao, 0);    DSR(f.a[0][1], ao, 512);
            DSR(f.b[0][0], p0, 0);    DSR(f.b[0][1], p1, 0);
            DSR(f.a[1][0], ao, 4096); DSR(f.a[1][1], ao, 4608);
            DSR(f.b[1][0], p0, 2 * TILEB); DSR(f.b[1][1], p1, 2 * TILEB);
            DSR(f.a[2][0], ao, 8192); DSR(f.a[2][1], ao, 8704);
            DSR(f.b[2][0], p0, 4 * TILEB); DSR(f.b[2][1], p1, 4 * TILEB);
        };
        // the 24 MFMAs of the step held in c, the 12 operand reads of step s_next into n, one per MFMA gap
        auto step = [&](Frag& c, Frag& n, int s_next) {
            const unsigned ao = aLane + (unsigned)((s_next % NBUF) * WSLOT);
            const unsigned p0 = bBase[0] + (unsigned)b_off(s_next), p1 = bBase[1] + (unsigned)b_off(s_next);
            int gap = 0;
            auto G = [&]() {
                switch (gap) {
                    case 0: DSR(n.a[0][0], ao, 0); break;            case 1: DSR(n.a[0][1], ao, 512); break;
                    case 2: DSR(n.b[0][0], p0, 0); break;            case 3: DSR(n.b[0][1], p1, 0); break;
                    case 4: DSR(n.a[1][0], ao, 4096); break;         case 5: DSR(n.a[1][1], ao, 4608); break;
                    case 6: DSR(n.b[1][0], p0, 2 * TILEB); break;    case 7: DSR(n.b[1][1], p1, 2 * TILEB); break;
                    case 8: DSR(n.a[2][0], ao, 8192); break;         case 9: DSR(n.a[2][1], ao, 8704); break;
                    case 10: DSR(n.b[2][0], p0, 4 * TILEB); break;   case 11: DSR(n.b[2][1], p1, 4 * TILEB); break;
                    default: break;
                }
                ++gap;
            };
            asm volatile("s_waitcnt lgkmcnt(0)" : FRAG_REGS(c) :: "memory");
            MF4(c.a[2][0], c.a[2][1], c.b[0][0], c.b[0][1]);
            MF4(c.a[0][0], c.a[0][1], c.b[2][0], c.b[2][1]);
            MF4(c.a[1][0], c.a[1][1], c.b[1][0], c.b[1][1]);
            MF4(c.a[1][0], c.a[1][1], c.b[0][0], c.b[0][1]);
            MF4(c.a[0][0], c.a[0][1], c.b[1][0], c.b[1][1]);
            MF4(c.a[0][0], c.a[0][1], c.b[0][0], c.b[0][1]);
        };
        __builtin_amdgcn_s_setprio(3);
        Frag F0, F1;
        __syncthreads();                                   // B1
        __syncthreads();                                   // B2: halo tile of group 0 written, steps 0..5 landed
        loadF(F0, 0);
#pragma unroll 1
        for (int gg = 0; gg < NOG / 2; ++gg) {
#pragma unroll
            for (int pr = 0; pr < 9; ++pr) {
                step(F0, F1, 2 * pr + 1);
                asm volatile("s_waitcnt lgkmcnt(0)" : FRAG_REGS(F1) :: "memory");
                BAR_PLAIN();                               // steps t+2, t+3 have landed; every MFMA wave holds steps t, t+1 in registers: their ring slots are free
                step(F1, F0, (2 * pr + 2) % 18);           // (after the last step of all: a read of stale, in-bounds LDS that nobody uses)
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" : FRAG_REGS(F0) :: "memory");
        __builtin_amdgcn_s_setprio(0);
    }

    // ---- epilogue: G -> LDS, contract the 9 planes of each channel with plane'(x)
    float xv[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int cl = (tid >> 7) + 4 * it, c = ct * BD_TCH + cl;
        xv[it] = (cl < BD_TCH && c < NC) ? x[epix + (size_t)c * HW] : 0.f;
    }
    float* sG = (float*)sW;
    __syncthreads();                                       // every wave is done with the ring
    if (tid < 256) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) sG[(w_o * 64 + i * 32 + mfma_row(r, lane)) * BD_TP + w_p * 64 + j * 32 + m] = acc[i][j][r];
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int cl = (tid >> 7) + 4 * it, c = ct * BD_TCH + cl;
        if (cl >= BD_TCH || c >= NC) continue;
        const int row0 = (cl / BD_CH) * 64 + (cl % BD_CH) * NP;
        dx[epix + (size_t)c * HW] = stage_unit_grad<KAN_BASIS_BSPLINE, FAST_BSPLINE_SILU>(bs, sTab, xv[it], xv[it], sG + row0 * BD_TP + en, BD_TP).dx;
    }
}


const char* split_reject(const KanGeom* g, const KanBasis* b) {
    if (!g || !b) return "null geometry / basis";
    if (b->kind != KAN_BASIS_BSPLINE || b->n_basis != 8 || b->order != 3 || b->act != KAN_ACT_SILU) return "split-precision forward: default B-spline spec only (grid 5, order 3, SiLU)";
    if (!((g->H == 8 && g->W == 8) || (g->H == 16 && g->W == 16)) || g->Ho != g->H || g->Wo != g->W || g->kh != 3 || g->kw != 3 || g->sh != 1 || g->sw != 1 || g->ph != 1 || g->pw != 1 || g->dh != 1 || g->dw != 1)
        return "split-precision forward: 8x8 or 16x16 planes, 3x3 / stride 1 / pad 1 only";
    if (g->groups > 1 || g->C % CG || g->O % 128 || (g->H == 8 && g->B % 2) || g->C < CG) return "split-precision forward: one group, C % 8 == 0, O % 128 == 0, even batch on 8x8 planes";
    if (g->x_bstride != (long long)g->C * g->H * g->W || g->y_bstride != (long long)g->O * g->H * g->W) return "split-precision forward: dense NCHW tensors";
    if ((long long)(g->C / CG) * NSTEP * 3 * 2 * g->O * 16 >= (1ll << 31)) return "split-precision forward: cut weights must stay under 2 GiB";
    return nullptr;
}

// the bwd-data launch: the scope of split_reject, and its own cut-weight buffer under 2 GiB
const char* split_bwd_reject(const KanGeom* g, const KanBasis* b) {
    if (const char* why = split_reject(g, b)) return why;
    if ((long long)bwd_row_tiles(g->C) * (g->O / 16) * 9 * WSLOT >= (1ll << 31)) return "split-precision bwd-data: cut weights must stay under 2 GiB";
    return nullptr;
}

// ---- the weight gradient (k_split_bwd_weight): what kan_conv_bwd_weight + kan_unpack_wgrad compute for a layer in scope,
//   dW[o][c][plane][tap] = sum_{b,h,w} dz[b,o,h,w] * plane(x[b,c,h+r-1,w+t-1]),   tap = 3 r + t,
// straight into the reference layouts.  The GEMM depth is now the pixel axis (b, h, w); a lane of the 32x32x16 MFMA wants 8 depth-consecutive bf16 values
// in one 16-byte fragment, and a tap's column shift of one pixel would misalign a pixel-contiguous chunk by 2 bytes.  Way out taken here: IMAGES are the
// inner depth index.  A 16-byte chunk holds the 8 images of an octet at the same (channel, plane, cell), so every tap is a whole-cell shift of one
// zero-bordered halo tile, read with ds_read_b128 exactly as the forward reads its tile; nothing is transposed, EXEC stays full, and a batch tail is just
// zero images.  (The hardware-transposed reads, ds_read_b64_tr_b16 on a cell-major tile, would keep the forward's tile but need two reads per fragment under
// their alignment rules and give nothing back: the expansion is per (image, pixel) either way.)  The price is paid at small batches only: an octet with
// fewer than 8 images multiplies zeros.
//   tile    128 outputs x 96 columns per workgroup: the 81 (plane, tap) columns of ONE input channel (column n = 9 plane + tap: the reference order of both
//           gradient tensors) + 15 padding columns that are computed and never stored.  512 threads = 8 waves, two per SIMD: wave = (32-output block,
//           depth half), each 32 outputs x 96 columns (3 blocks) over its half of every block's steps -- one wave's operand reads hide behind the other's
//           MFMAs; the halves are added through LDS at the end, in a fixed order;
//   depth   units of 64 pixels x 8 images: an octet of whole 8x8 images, or four image rows of an octet of 16x16 images.  A step of 16 = two neighbouring
//           pixels of a row (the k-halves) x 8 images; a unit is 8 blocks of 8 pixels (4 steps).  The units of a layer are dealt to KS workgroups per
//           (channel, output tile) in contiguous runs; every workgroup stores its 128 x 81 partial sums once and k_wgrad_reduce adds the KS partials in
//           ascending order into dw_base / dw_basis (every element written once, no atomics: two runs are bit-identical);
//   B side  per unit all threads expand the channel's values (stage_unit, the exact kernels' own plane values: SiLU + 8 B-spline planes), cut image PAIRS with split_pair and
//           write 4 bytes per (plane, piece) into the halo tile [piece][cell][plane][8 images]; rows outside the image and images past the batch are
//           written as zeros, the left / right border cells are zeroed once.  The x values of a unit are fetched one unit ahead.  The expanded tensor
//           never exists in HBM;
//   A side  dz is cut once per call (k_cut_dz) into dzc[octet][pixel][piece][o][8 images] in the caller's workspace and streamed by 16-byte LDS-DMA, one
//           8-pixel block (48 KB) ahead of the block being contracted (across units too), two buffers, s_waitcnt vmcnt(0) + barrier per block (36 MFMAs per wave);
//   loop    18 MFMAs per step and wave (3 column blocks x the six products, smallest first), operands of 3 + 9 ds_read_b128, through the MFMA builtin: the
//           compiler's schedule (it sinks the block's barrier between a wave's two steps, so the two waves of a SIMD drift half a block apart) measured
//           1.42 - 1.48 x the exact kernels; pinning MFMAs and barrier in source order with volatile asm measured 7 % slower on all three shapes.
// First version: one role for every wave, not the producer / MFMA wave split, the counted vmcnt + bare s_barrier ring and the explicit-ISA step of the two
// kernels above.  The producer split itself was NOT tried here: the only alternative measured is the pinned order above.  The rate of issued bf16 products
// (~1.3 PFLOP/s at 256 -> 256) is in the range of the forward's; what this kernel gives away against the 1.7 - 1.9 x of the other two launches is the 15
// padding columns of 96, the expansion and the dz copy wait sitting on every wave's critical path, and the pre-pass and reduce launches.
constexpr int WG_NB = 3, WG_COLS = NP * 9;                           // column blocks of 32; live columns
constexpr int WG_PXB = 3 * 128 * 16, WG_DZBUF = 8 * WG_PXB;          // bytes of one pixel / one 8-pixel block of a 128-output tile of dzc
template <int PW> struct WgGeo {
    static constexpr int TR = PW == 8 ? 8 : 4, UPO = PW / TR;        // image rows per unit; units per image octet
    static constexpr int PITCH = PW + 2, CELLS = (TR + 2) * PITCH, PIECEB = CELLS * CELLC * 16, EB = 3 * PIECEB, HWP = PW * PW;
    static constexpr int NROWS = PW == 8 ? TR : TR + 2, HR0 = PW == 8 ? 1 : 0;     // halo rows a unit writes (8x8: the outer two are always outside the image)
};
template <int PW> constexpr int lds_bytes_wg() { return WgGeo<PW>::EB + 2 * WG_DZBUF + 64; }

inline int wg_octets(const KanGeom* g) { return (g->B + 7) / 8; }
inline int wg_units(const KanGeom* g) { return wg_octets(g) * (g->H == 8 ? 1 : 4); }
// depth splits: enough workgroups for two rounds of 256 CUs, at most 32 and at most one per unit -- a function of the geometry alone
inline int wg_ksplit(const KanGeom* g) {
    const int tiles = g->C * (g->O / 128), units = wg_units(g);
    int ks = (512 + tiles - 1) / tiles;
    ks = ks > 32 ? 32 : ks;
    return ks > units ? units : ks;
}
inline long long wg_dz_bytes(const KanGeom* g) { return (long long)wg_octets(g) * g->H * g->W * 3 * g->O * 16; }
inline long long wg_part_bytes(const KanGeom* g) { return (long long)wg_ksplit(g) * g->O * g->C * WG_COLS * 4; }

const char* split_bww_reject(const KanGeom* g, const KanBasis* b) {
    if (const char* why = split_reject(g, b)) return why;
    if (wg_dz_bytes(g) >= (1ll << 31)) return "split-precision bwd-weight: cut dz must stay under 2 GiB";
    return nullptr;
}

// ---- dz [B][O][HW] -> dzc[octet][pixel][piece][o][8 bf16: images 8 octet .. 8 octet + 7, zero past the batch].  A workgroup cuts a tile of 16 outputs x 16
// pixels of one octet: it reads pixel-fastest (64 contiguous bytes per output and image), turns the tile round in LDS (pitch 17 chunks: conflict-free both
// ways) and stores output-fastest (256 contiguous bytes per pixel and piece)
__global__ __launch_bounds__(256) void k_cut_dz(const float* __restrict__ dz, __bf16* __restrict__ dzc, int NB, int NO, int HW) {
    __shared__ uint4 sT[3 * 16 * 17];
    const int t = threadIdx.x, o_tiles = NO / 16, p_tiles = HW / 16;
    const int o0 = (blockIdx.x % o_tiles) * 16, px0 = ((blockIdx.x / o_tiles) % p_tiles) * 16, q = blockIdx.x / (o_tiles * p_tiles);
    {
        const int ol = t >> 4, pl = t & 15;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { const int b = q * 8 + i; v[i] = b < NB ? dz[((size_t)b * NO + o0 + ol) * HW + px0 + pl] : 0.f; }
        uint4 h, md, l;
        split_pair(v[0], v[1], h.x, md.x, l.x); split_pair(v[2], v[3], h.y, md.y, l.y);
        split_pair(v[4], v[5], h.z, md.z, l.z); split_pair(v[6], v[7], h.w, md.w, l.w);
        sT[pl * 17 + ol] = h; sT[272 + pl * 17 + ol] = md; sT[544 + pl * 17 + ol] = l;
    }
    __syncthreads();
    const int pl = t >> 4, ol = t & 15;
    uint4* dst = (uint4*)dzc + ((size_t)(q * HW + px0 + pl) * 3) * NO + o0 + ol;
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) dst[(size_t)pc * NO] = sT[pc * 272 + pl * 17 + ol];
}

template <int PW>
__global__ __launch_bounds__(512, 1) void k_split_bwd_weight(const float* __restrict__ x, const __bf16* __restrict__ dzc, float* __restrict__ part, DevBasis bs,
                                                             int NB, int NC, int NO, int o_tiles, int KS, int dzc_bytes) {
    using Gm = WgGeo<PW>;
    constexpr int PITCH = Gm::PITCH, PIECEB = Gm::PIECEB, EB = Gm::EB, HW = Gm::HWP, TR = Gm::TR, UPO = Gm::UPO, NCELL = Gm::NROWS * PW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sE = smem;                                              // halo tile of the expanded channel
    unsigned char* sD = smem + EB;                                         // two 8-pixel blocks of cut dz
    float* sTab = (float*)(smem + EB + 2 * WG_DZBUF);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), kh = lane >> 5, m = lane & 31;
    const int wo = wave & 3, dh = wave >> 2;                               // 32-output block; depth half: steps 2 dh, 2 dh + 1 of every block
    const int c = blockIdx.x % NC, ot = (blockIdx.x / NC) % o_tiles, ks = blockIdx.x / (NC * o_tiles);
    const int units = ((NB + 7) / 8) * UPO, u0 = (int)((long long)ks * units / KS), u1 = (int)((long long)(ks + 1) * units / KS);

    for (int i = tid; i < EB / 16; i += 512) ((uint4*)sE)[i] = uint4{0u, 0u, 0u, 0u};
    if (tid < 16) sTab[tid] = bs.tab[tid];

    // dz stream: 6 chunks of 16 B per thread and block; chunk (pixel, piece, o) of the block at ((pixel * 3 + piece) * 128 + o) * 16
    const __amdgpu_buffer_rsrc_t d_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(dzc), 0, dzc_bytes, 0x00020000);
    const int voff0 = ((tid >> 7) * NO + ot * 128 + (tid & 127)) * 16;
    auto issue = [&](int q, int px0, int buf) {
        unsigned char* dst = sD + buf * WG_DZBUF + wave * 1024;
        const int so = __builtin_amdgcn_readfirstlane((q * HW + px0) * 3 * NO * 16);
#pragma unroll
        for (int j = 0; j < 6; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(d_rs, (__attribute__((address_space(3))) void*)(dst + j * 8192), 16, voff0 + j * 4 * NO * 16, so, 0, 0);
    };
    // first pixel of block blk of the unit whose first image row is r0
    auto block_px = [&](int r0, int blk) { return PW == 8 ? blk * 8 : (r0 + (blk >> 1)) * 16 + (blk & 1) * 8; };

    // operand addresses (bytes): A = dz rows of this wave, B = the lane's column (plane, tap) of each block, both at the k-half's pixel
    const unsigned aLane = (unsigned)(EB + (4 * dh + kh) * WG_PXB + (wo * 32 + m) * 16);
    unsigned bLane[WG_NB];
#pragma unroll
    for (int j = 0; j < WG_NB; ++j) {
        const int n = j * 32 + m, p = n < WG_COLS ? n / 9 : 0, tap = n < WG_COLS ? n % 9 : 4;      // padding columns: centre tap of plane 0 (never stored)
        bLane[j] = (unsigned)((((tap / 3 - 1) * PITCH + (tap % 3 - 1) + 4 * dh + kh) * CELLC + p) * 16);
    }

    f32x16 acc[WG_NB];
#pragma unroll
    for (int j = 0; j < WG_NB; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    // expansion item of this thread: (cell, image pair); NCELL * 4 <= 512 items, one per thread.  Its two x values are fetched one unit ahead.
    static_assert(NCELL * 4 <= 512, "one expansion item per thread");
    const bool has_item = tid < NCELL * 4;
    const int pair = tid / NCELL, cl = tid % NCELL, hr = Gm::HR0 + cl / PW, col = cl % PW;
    auto fetch = [&](int u, float (&xr)[2]) {
        const int q = u / UPO, row = (u % UPO) * TR + hr - 1;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int b = q * 8 + pair * 2 + i;
            xr[i] = (has_item && row >= 0 && row < PW && b < NB) ? x[((size_t)b * NC + c) * HW + row * PW + col] : 0.f;
        }
    };
    float xr[2];
    fetch(u0, xr);
    __syncthreads();
    issue(u0 / UPO, block_px((u0 % UPO) * TR, 0), 0);
#pragma unroll 1
    for (int u = u0; u < u1; ++u) {
        const int q = u / UPO, r0 = (u % UPO) * TR;
        // (every wave is past the barrier of the previous unit's last block: the tile and dz buffer 1 are free; block 0 of this unit is on its way to buffer 0)
        if (has_item) {
            float* colS = (float*)(sD + WG_DZBUF) + tid;                   // this thread's stage_unit column (+ dump slot), pitch 512, in dz buffer 1
            const int row = r0 + hr - 1;
            float v[2][NP];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const bool inb = row >= 0 && row < PW && q * 8 + pair * 2 + i < NB;      // outside: all nine planes zero
                stage_unit<KAN_BASIS_BSPLINE, FAST_BSPLINE_SILU>(bs, sTab, inb, xr[i], xr[i], colS, 512, colS + NP * 512);
#pragma unroll
                for (int p = 0; p < NP; ++p) v[i][p] = colS[p * 512];
            }
            unsigned char* d = sE + ((hr * PITCH + col + 1) * CELLC) * 16 + pair * 4;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                unsigned h, md, l;
                split_pair(v[0][p], v[1][p], h, md, l);
                *(unsigned*)(d + p * 16) = h; *(unsigned*)(d + PIECEB + p * 16) = md; *(unsigned*)(d + 2 * PIECEB + p * 16) = l;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const bool more = u + 1 < u1;
        if (more) fetch(u + 1, xr);                                         // lands behind block 0's MFMAs
#pragma unroll 1
        for (int blk = 0; blk < 8; ++blk) {
            if (blk + 1 < 8) issue(q, block_px(r0, blk + 1), (blk + 1) & 1);
            else if (more) issue((u + 1) / UPO, block_px(((u + 1) % UPO) * TR, 0), 0);      // the next unit's block 0: buffer 0 is free since block 6's barrier
            const int lrow = PW == 8 ? blk : (blk >> 1), col0 = PW == 8 ? 0 : (blk & 1) * 8;
            const unsigned char* pa = smem + aLane + (blk & 1) * WG_DZBUF;
            const unsigned char* pb = sE + ((lrow + 1) * PITCH + col0 + 1) * CELLC * 16;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                bf16x8 a[3], b[WG_NB][3];
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) {
                    a[pc] = *(const bf16x8*)(pa + s * 2 * WG_PXB + pc * 2048);
#pragma unroll
                    for (int j = 0; j < WG_NB; ++j) b[j][pc] = *(const bf16x8*)(pb + s * 2 * CELLC * 16 + bLane[j] + pc * PIECEB);
                }
                // smallest products first: lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi (A = dz, B = plane value)
#pragma unroll
                for (int j = 0; j < WG_NB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[j][0], acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < WG_NB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[j][2], acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < WG_NB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[j][1], acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < WG_NB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[j][0], acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < WG_NB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[j][1], acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < WG_NB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[j][0], acc[j], 0, 0, 0);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }
    // ---- the two depth halves meet in LDS (the dz buffers are free after the last barrier), added in a fixed order; then the partial sums:
    // part[ks][o][c][n], live columns only
    float* sR = (float*)sD;
    if (dh) {
#pragma unroll
        for (int j = 0; j < WG_NB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) sR[((wo * WG_NB + j) * 16 + r) * 64 + lane] = acc[j][r];
    }
    __syncthreads();
    if (dh) return;
    float* po = part + ((size_t)ks * NO + ot * 128 + wo * 32) * NC * WG_COLS + (size_t)c * WG_COLS;
#pragma unroll
    for (int j = 0; j < WG_NB; ++j) {
        const int n = j * 32 + m;
        if (n >= WG_COLS) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) po[(size_t)mfma_row(r, lane) * NC * WG_COLS + n] = acc[j][r] + sR[((wo * WG_NB + j) * 16 + r) * 64 + lane];
    }
}

// ---- part[KS][O][C][81] -> dw_base[O][C][9], dw_basis[O][C * 8][9], the KS partials added in ascending order
__global__ void k_wgrad_reduce(const float* __restrict__ part, float* __restrict__ dwb, float* __restrict__ dws, int n_oc, int KS) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;             // (o, c, column)
    if (idx >= n_oc * WG_COLS) return;
    float s = part[idx];
    for (int k = 1; k < KS; ++k) s += part[(size_t)k * n_oc * WG_COLS + idx];
    const int oc = idx / WG_COLS, n = idx % WG_COLS;
    if (n < 9) dwb[(size_t)oc * 9 + n] = s;
    else dws[(size_t)oc * 72 + (n - 9)] = s;
}

}  // namespace

extern "C" {

int kan_split_supported(const KanGeom* g, const KanBasis* b) { return split_reject(g, b) == nullptr ? 1 : 0; }

long long kan_split_weight_bytes(const KanGeom* g, const KanBasis* b) {
    if (split_reject(g, b)) return 0;
    return (long long)(g->C / CG) * NSTEP * 3 * 2 * g->O * 16;
}

int kan_split_pack_weights(const float* w_base, const float* w_basis, void* wc, const KanGeom* g, const KanBasis* b, void* stream) {
    const char* why = split_reject(g, b);
    if (why) return kan_fail_msg("%s", why);
    if (!w_base || !w_basis || !wc) return kan_fail_msg("kan_split_pack_weights: null pointer%s", "");
    const int n = (g->C / CG) * NSTEP * 2 * g->O;
    hipLaunchKernelGGL(k_cut_weights, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, w_base, w_basis, (__bf16*)wc, g->C, g->O);
    return hipGetLastError() == hipSuccess ? 0 : kan_fail_msg("kan_split_pack_weights: launch failed%s", "");
}

int kan_conv_fwd_split(const float* x, const void* wc, float* z, const KanGeom* g, const KanBasis* b, void* stream) {
    const char* why = split_reject(g, b);
    if (why) return kan_fail_msg("%s", why);
    if (!x || !wc || !z) return kan_fail_msg("kan_conv_fwd_split: null pointer%s", "");
    if (kan_raise_lds_limit((const void*)k_split_fwd<8>, lds_bytes<8>()) || kan_raise_lds_limit((const void*)k_split_fwd<16>, lds_bytes<16>()))
        return kan_fail_msg("kan_conv_fwd_split: cannot reserve %s of LDS", "158 KB");
    const DevBasis db = dev_basis(b);
    const int o_tiles = g->O / 128;
    if (g->H == 8)
        hipLaunchKernelGGL(k_split_fwd<8>, dim3((unsigned)((g->B / 2) * o_tiles)), dim3(512), lds_bytes<8>(), (hipStream_t)stream, x, (const __bf16*)wc, z, db, g->C, g->O, o_tiles);
    else
        hipLaunchKernelGGL(k_split_fwd<16>, dim3((unsigned)(g->B * 2 * o_tiles)), dim3(512), lds_bytes<16>(), (hipStream_t)stream, x, (const __bf16*)wc, z, db, g->C, g->O, o_tiles);
    return hipGetLastError() == hipSuccess ? 0 : kan_fail_msg("kan_conv_fwd_split: launch failed%s", "");
}

long long kan_split_bwd_data_weight_bytes(const KanGeom* g, const KanBasis* b) {
    if (split_bwd_reject(g, b)) return 0;
    return (long long)bwd_row_tiles(g->C) * (g->O / 16) * 9 * WSLOT;
}

int kan_split_pack_weights_bwd_data(const float* w_base, const float* w_basis, void* wcd, const KanGeom* g, const KanBasis* b, void* stream) {
    const char* why = split_bwd_reject(g, b);
    if (why) return kan_fail_msg("%s", why);
    if (!w_base || !w_basis || !wcd) return kan_fail_msg("kan_split_pack_weights_bwd_data: null pointer%s", "");
    const int c_tiles = bwd_row_tiles(g->C), n = c_tiles * (g->O / 16) * 9 * 2 * 128;
    hipLaunchKernelGGL(k_cut_weights_bwd_data, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, w_base, w_basis, (__bf16*)wcd, g->C, g->O, c_tiles);
    return hipGetLastError() == hipSuccess ? 0 : kan_fail_msg("kan_split_pack_weights_bwd_data: launch failed%s", "");
}

int kan_conv_bwd_data_split(const float* dz, const float* x, const void* wcd, float* dx, const KanGeom* g, const KanBasis* b, void* stream) {
    const char* why = split_bwd_reject(g, b);
    if (why) return kan_fail_msg("%s", why);
    if (!dz || !x || !wcd || !dx) return kan_fail_msg("kan_conv_bwd_data_split: null pointer%s", "");
    if (kan_raise_lds_limit((const void*)k_split_bwd_data<8>, lds_bytes_bwd<8>()) || kan_raise_lds_limit((const void*)k_split_bwd_data<16>, lds_bytes_bwd<16>()))
        return kan_fail_msg("kan_conv_bwd_data_split: cannot reserve %s of LDS", "109 KB");
    const DevBasis db = dev_basis(b);
    const int c_tiles = bwd_row_tiles(g->C);
    if (g->H == 8)
        hipLaunchKernelGGL(k_split_bwd_data<8>, dim3((unsigned)((g->B / 2) * c_tiles)), dim3(512), lds_bytes_bwd<8>(), (hipStream_t)stream, dz, x, (const __bf16*)wcd, dx, db, g->C, g->O, c_tiles);
    else
        hipLaunchKernelGGL(k_split_bwd_data<16>, dim3((unsigned)(g->B * 2 * c_tiles)), dim3(512), lds_bytes_bwd<16>(), (hipStream_t)stream, dz, x, (const __bf16*)wcd, dx, db, g->C, g->O, c_tiles);
    return hipGetLastError() == hipSuccess ? 0 : kan_fail_msg("kan_conv_bwd_data_split: launch failed%s", "");
}

long long kan_split_bwd_weight_workspace_bytes(const KanGeom* g, const KanBasis* b) {
    if (split_bww_reject(g, b)) return 0;
    return wg_dz_bytes(g) + wg_part_bytes(g);
}

int kan_conv_bwd_weight_split(const float* dz, const float* x, float* dw_base, float* dw_basis, void* workspace, const KanGeom* g, const KanBasis* b, void* stream) {
    const char* why = split_bww_reject(g, b);
    if (why) return kan_fail_msg("%s", why);
    if (!dz || !x || !dw_base || !dw_basis || !workspace) return kan_fail_msg("kan_conv_bwd_weight_split: null pointer%s", "");
    if ((uintptr_t)workspace & 15) return kan_fail_msg("kan_conv_bwd_weight_split: workspace must be 16-byte aligned%s", "");
    if (kan_raise_lds_limit((const void*)k_split_bwd_weight<8>, lds_bytes_wg<8>()) || kan_raise_lds_limit((const void*)k_split_bwd_weight<16>, lds_bytes_wg<16>()))
        return kan_fail_msg("kan_conv_bwd_weight_split: cannot reserve %s of LDS", "142 KB");
    const DevBasis db = dev_basis(b);
    const hipStream_t st = (hipStream_t)stream;
    const int o_tiles = g->O / 128, KS = wg_ksplit(g), HW = g->H * g->W, n_cut = wg_octets(g) * (HW / 16) * (g->O / 16), n_oc = g->O * g->C;
    __bf16* dzc = (__bf16*)workspace;
    float* part = (float*)((char*)workspace + wg_dz_bytes(g));
    hipLaunchKernelGGL(k_cut_dz, dim3((unsigned)n_cut), dim3(256), 0, st, dz, dzc, g->B, g->O, HW);      // one workgroup per (octet, 16 pixels, 16 outputs)
    const dim3 grid((unsigned)(g->C * o_tiles * KS));
    if (g->H == 8)
        hipLaunchKernelGGL(k_split_bwd_weight<8>, grid, dim3(512), lds_bytes_wg<8>(), st, x, (const __bf16*)dzc, part, db, g->B, g->C, g->O, o_tiles, KS, (int)wg_dz_bytes(g));
    else
        hipLaunchKernelGGL(k_split_bwd_weight<16>, grid, dim3(512), lds_bytes_wg<16>(), st, x, (const __bf16*)dzc, part, db, g->B, g->C, g->O, o_tiles, KS, (int)wg_dz_bytes(g));
    hipLaunchKernelGGL(k_wgrad_reduce, dim3((n_oc * WG_COLS + 255) / 256), dim3(256), 0, st, (const float*)part, dw_base, dw_basis, n_oc, KS);
    return hipGetLastError() == hipSuccess ? 0 : kan_fail_msg("kan_conv_bwd_weight_split: launch failed%s", "");
}

}  // extern "C"
