// Host-side interfaces between the translation units of libkanconv (not part of the C ABI; nothing here is exported).
//   kanconv.hip     C-ABI entry points, the tap-major / halo / position-major GEMM kernels and their launchers, layout and norm kernels
//   kan_plan.hip    host only: argument checks and the planner (plan_conv) -- the one place that picks a route and a tile for each stage
//   kan_direct.hip  band kernels: layers of few input channels (first layers: 3 -> 64) and layers whose output count fills no 128-wide
//                   tile (64 -> 192), any kernel size / stride / dilation / padding
//   kan_split.hip   opt-in split-precision forward
//   kan_loss.hip    cross-entropy loss, its gradient and the counters of the test metrics
//   kan_feed.hip    batches from a device-resident uint8 dataset: gather, crop, flip, convert, normalise
#pragma once
#include <type_traits>
#include "kanconv.h"

// sets the thread-local message behind kan_last_error() and returns -1 (defined in kanconv.hip)
int kan_fail_msg(const char* fmt, const char* a);
// Raises `kernel`'s dynamic-LDS limit to `bytes` once per (kernel, device) -- the only mutable global state of the library (a mutex-guarded
// list); later calls on the same device return at once, so a launch stays a plain launch (and graph capture sees nothing new).  0 or -1.
int kan_raise_lds_limit(const void* kernel, int bytes);

// ---------------------------------------------------------------------------------------------------------------- compile-time basis specs
// A fast variant is a basis (kind, planes, activation) with compile-time kernels (template parameter FAST; 0 = the generic kernels);
// its facts are its row of fast_spec below.  The values are part of the kernel names: never renumber.
enum : int {
    FAST_GENERIC = 0,
    FAST_BSPLINE_SILU = 1,    // B-spline grid 5 order 3, SiLU base
    FAST_BSPLINE_GELU = 2,    // B-spline grid 5 order 3, GELU base
    FAST_RBF8 = 3,            // FastKAN, 8 centres, SiLU base
    FAST_CHEBY5 = 4,          // ChebyKAN degree 4
    FAST_CHEBY4 = 5,          // ChebyKAN degree 3
    FAST_POLY4 = 6,           // recurrence families degree 3, with base
    FAST_POLY3 = 7,           // recurrence families degree 2, with base
    FAST_RBF5 = 8,            // FastKAN, 5 centres (kan_vgg.py's grid_size 5), SiLU base
    FAST_RELU8 = 9,           // ReLU-KAN g + k = 8, SiLU base (halo and expanded kernels only)
    FAST_GRAM4 = 10,          // GRAM-KAN degree 3, SiLU base (halo and expanded kernels only)
    FAST_POLY1 = 11,          // recurrence families degree 0, with base
    FAST_LAST = 11
};
// The kernel families instantiated for a fast variant (FastSpec::routes: the planner asks it which routes a basis may take, the
// launchers instantiate exactly these kernels).
enum : unsigned {
    ON_TAP_MAJOR = 1u << 0,          // k_conv_fwd / k_conv_bwd_data / k_conv_bwd_weight with FAST = F
    ON_BIG_TILES = 1u << 1,          // 256-output tiles of the tap-major and halo kernels
    ON_HALO_FWD = 1u << 2,           // k_conv_fwd_halo
    ON_HALO_BWD_WEIGHT = 1u << 3,    // k_conv_bwd_weight_halo
    ON_BAND_FWD = 1u << 4,           // k_band_fwd
    ON_BAND_BWD_WEIGHT = 1u << 5,    // k_band_bwd_weight
    ON_EXPANDED_FWD = 1u << 6,       // k_conv_fwd_pmdma on the expanded copy
    ON_EXPANDED = 1u << 7,           // k_expand_pm + k_conv_bwd_weight_pmdma
    ON_ROWBLK_BWD_DATA = 1u << 8,    // k_conv_bwd_data with row-ordered pixel blocks (RB = 1)
};
// THE definition of a fast variant: kernels, launchers and the planner read these facts and restate none of them.
struct FastSpec {
    int kind, planes;        // KAN_BASIS_*, planes per channel P (base plane included)
    bool base;               // plane 0 is the base branch act(x)
    bool xn_fwd, xn_bwd;     // the basis reads a second tensor xn != x in the forward / weight gradient; also in bwd-data (which then writes dx and dxn)
    int kc;                  // tap-major LDS step (rows)
    unsigned routes;         // kernel families instantiated (ON_*)
};
constexpr FastSpec fast_spec(int f) {
    constexpr unsigned bspline = ON_TAP_MAJOR | ON_BIG_TILES | ON_HALO_FWD | ON_HALO_BWD_WEIGHT | ON_BAND_FWD | ON_BAND_BWD_WEIGHT |
                                 ON_EXPANDED_FWD | ON_EXPANDED | ON_ROWBLK_BWD_DATA;
    switch (f) {
        case FAST_BSPLINE_SILU: case FAST_BSPLINE_GELU: return {KAN_BASIS_BSPLINE, 9, true, false, false, 18, bspline};
        case FAST_RBF8: return {KAN_BASIS_RBF, 9, true, true, true, 18, ON_TAP_MAJOR | ON_BAND_FWD | ON_BAND_BWD_WEIGHT};
        case FAST_RBF5: return {KAN_BASIS_RBF, 6, true, true, true, 18, ON_TAP_MAJOR};
        case FAST_CHEBY5: return {KAN_BASIS_CHEBY, 5, false, false, false, 16, ON_TAP_MAJOR | ON_BIG_TILES | ON_BAND_FWD | ON_BAND_BWD_WEIGHT};
        case FAST_CHEBY4: return {KAN_BASIS_CHEBY, 4, false, false, false, 16, ON_TAP_MAJOR | ON_HALO_FWD | ON_BAND_FWD};
        case FAST_POLY4: return {KAN_BASIS_POLY, 5, true, true, false, 16, ON_TAP_MAJOR | ON_BIG_TILES | ON_HALO_FWD | ON_BAND_FWD};
        case FAST_POLY3: return {KAN_BASIS_POLY, 4, true, true, false, 16, ON_TAP_MAJOR};
        case FAST_POLY1: return {KAN_BASIS_POLY, 2, true, true, false, 16, ON_TAP_MAJOR};
        case FAST_RELU8: return {KAN_BASIS_RELU, 9, true, false, false, 16, ON_HALO_FWD | ON_HALO_BWD_WEIGHT | ON_EXPANDED_FWD | ON_EXPANDED};
        case FAST_GRAM4: return {KAN_BASIS_GRAM, 5, true, false, false, 16, ON_HALO_FWD | ON_HALO_BWD_WEIGHT | ON_EXPANDED};
        default: return {-1, 0, false, true, true, 0, 0};          // FAST_GENERIC: the generic kernels read both tensors, the rest is DevBasis at run time
    }
}
constexpr int fast_kind(int f) { return fast_spec(f).kind; }
constexpr int fast_planes(int f) { return fast_spec(f).planes; }
constexpr bool fast_has(int f, unsigned routes) { return (fast_spec(f).routes & routes) == routes && f != FAST_GENERIC; }

// ---------------------------------------------------------------------------------------------------------------- dispatch helpers
template <int V> using IC = std::integral_constant<int, V>;
// fn(IC<F>) for the variant F == f if F has every bit of ROUTES; false (nothing called) otherwise.  Instantiates fn for those F only.
template <unsigned ROUTES, int F = 1, class Fn>
bool dispatch_fast(int f, Fn&& fn) {
    if constexpr (F > FAST_LAST) {
        return false;
    } else {
        if constexpr (fast_has(F, ROUTES)) {
            if (f == F) { fn(IC<F>{}); return true; }
        }
        return dispatch_fast<ROUTES, F + 1>(f, fn);
    }
}
// fn(IC<V>) for the first listed V equal to v, else for the last one.
template <int V, int... REST, class Fn>
void pick(int v, Fn&& fn) {
    if constexpr (sizeof...(REST) == 0) fn(IC<V>{});
    else if (v == V) fn(IC<V>{});
    else pick<REST...>(v, fn);
}
// fn(IC<kind>) over the basis kinds of the generic kernels (anything else runs as ChebyKAN, as the kernels read it)
template <class Fn>
void dispatch_kind(int kind, Fn&& fn) {
    pick<KAN_BASIS_BSPLINE, KAN_BASIS_RBF, KAN_BASIS_POLY, KAN_BASIS_FOURIER, KAN_BASIS_RELU, KAN_BASIS_GRAM, KAN_BASIS_CHEBY>(kind, fn);
}

// ---------------------------------------------------------------------------------------------------------------- band kernels
// The tap-major kernels expand every input value once per TAP it is used under (9x for 3x3, 121x for 11x11) -- vector-ALU work the fp32
// MFMA shares its issue slots with; with 3 input channels the GEMM depth is so short (243 rows) that this staging IS the kernel (0.34 -
// 0.40 matrix-pipe busy).  The band kernels expand the inputs a pixel tile can touch ONCE per channel group into an LDS halo tile and let
// every tap read it through a shifted address (the idea of k_conv_fwd_halo), for any geometry:
//   * strided taps by PHASE: input row = sh*ho - ph + dh*r = sh*(ho + off_r) + a_r, so the taps of one (row phase a, column phase b)
//     read the sub-image x[sh*i + a][sw*j + b] at (i, j) = (ho + off_r, wo + off_t): a stride-1 pattern.  A stride-s layer is
//     s*s phases of stride-1 sub-convolutions over the same output tile;
//   * a pixel tile is TP CONSECUTIVE output pixels in (image, row, column) order (no row-band restriction, so 27- or 55-wide planes fill
//     their 128-pixel tiles); its halo holds one "virtual row" per touched output row plus span_r extra rows PER IMAGE, so that rows of
//     different images never alias:  cell(pixel) = vrow * HC + wo,  B operand of tap (r, t) = cell + (off_r - OR0) * HC + (off_t - OC0);
//   * the halo is plane-minor, sH[cell][NPS] with NPS odd: the planes of a k-pair are an IMMEDIATE offset apart (no address arithmetic in
//     the MFMA loop) and 32 consecutive pixels hit 32 banks;
//   * depth order: step = (phase, channel group, tap of the phase), NPLE = even(NG * P) rows per step (row = ch * P + p, a zero pad row
//     when NG * P is odd); weights are packed in that order (kan_pack_weights follows the plan) and arrive by LDS-DMA.
// tools/probe/band_emul.py is the numpy restatement of this index arithmetic, checked against conv2d on random geometries.
#define KAN_BAND_MAX_TAPS 128
#define KAN_BAND_MAX_PHASES 16
typedef struct KanBandCfg {
    int ok;                       /* 0: this geometry / basis does not take the band kernels */
    int fast, P, NG, NPLE, NPS;   /* compile-time spec, planes per channel, channels per group, rows per step, halo words per cell */
    int NGR;                      /* channel groups (ceil(C / NG)) */
    int WO, MO, WP, TO, TP, NT;   /* waves along outputs, 32-output MFMA blocks per wave, waves along pixels; tile TO = 32 MO WO x TP = 64 WP; threads */
    int tiles_o, tiles_p;
    int n_phase, n_taps, n_steps; /* n_steps = NGR * n_taps weight steps of NPLE rows */
    int HC, span_r, OR0, OC0;     /* halo row length in cells, extra rows per image, smallest row / column offset of any tap */
    int cells;                    /* halo cells allocated per tile (largest tile) */
    int img_max;                  /* most images any one pixel tile touches (informational: kan_band_route) */
    int slots;                    /* expansion units per thread: ceil(NG * cells / NT) */
    int TS;                       /* taps per barrier step of the forward (2 where one tap is under ~36 MFMAs per wave) */
    int lds_bytes, wgs_per_cu;
    int fwd_splits;               /* split-K over the (phase, group) list */
    /* weight gradient (k_band_bwd_weight): row tiles of TR = 32 WR rows inside one (phase, channel group), all TO = 32 NI outputs per wave */
    int bw_ok, bw_WR, bw_NI, bw_NT, bw_tiles_o, bw_row_tiles, bw_TPI, bw_ptiles, bw_cells, bw_slots, bw_lds_bytes, bw_splits;
    unsigned short bw_ph_rt0[KAN_BAND_MAX_PHASES + 1];                      /* first row tile of each phase (NGR * ceil(nt * NPLE / TR) tiles per phase) */
    unsigned char ph_a[KAN_BAND_MAX_PHASES], ph_b[KAN_BAND_MAX_PHASES];     /* row / column phase of phase i */
    short ph_tap0[KAN_BAND_MAX_PHASES + 1];                                 /* first entry of phase i in the tap lists below */
    unsigned short tap_shift[KAN_BAND_MAX_TAPS];                            /* phase-ordered: halo shift of the tap, in cells */
    unsigned short tap_rt[KAN_BAND_MAX_TAPS];                               /* phase-ordered: r << 8 | t */
    short tap_step[KAN_BAND_MAX_TAPS], tap_nt[KAN_BAND_MAX_TAPS];           /* natural tap r*kw + t -> step of (group 0, this tap), taps in its phase:
                                                                               step(c, tap) = tap_step[tap] + (c / NG) * tap_nt[tap] */
} KanBandCfg;

/* Fill cfg for (geom, basis); `fast` = the compile-time spec of the basis (0: none -> cfg->ok = 0).  Pure host arithmetic (the planner's). */
void kan_band_cfg(const KanGeom* g, const KanBasis* b, int fast, KanBandCfg* cfg);
/* The band launchers take the plan's configuration and slab count; the planner picked the band route, so cfg->ok (and bw_ok) hold. */
/* dwp: bw_splits slabs of G * Kpad * Opad floats in band order (rows as the packed forward weights: kan_unpack_wgrad follows the plan). */
int kan_band_bwd_weight_launch(const float* dz, const float* x, const float* xn, float* dwp, const KanGeom* g, const KanBasis* b,
                               const KanBandCfg* cfg, int splits, long long slab_elems, void* stream);
/* z slabs [fwd_splits][B][O_total][Ho][Wo] as kan_conv_fwd; wp in band order. */
int kan_band_fwd_launch(const float* x, const float* xn, const float* wp, float* z, const KanGeom* g, const KanBasis* b,
                        const KanBandCfg* cfg, int splits, long long slab_elems, void* stream);

// ---------------------------------------------------------------------------------------------------------------- the plan
// Direct depthwise kernels (kanconv.hip): taps and taps * planes they hold
constexpr int DW_T = 9;
constexpr int DW_MAX_TP = 96;                      // taps * planes held in registers by the weight-gradient kernel

// Route of one stage.  EXPANDED: the stage has its own entry on the expanded position-major copy (kan_conv_fwd_expanded /
// kan_conv_bwd_weight_expanded); kan_conv_fwd / kan_conv_bwd_weight then run the tap-major kernel.
enum class Route { TAP_MAJOR, DW, BAND, HALO, EXPANDED };

struct FwdCfg { int TO, TP, tiles_o, tiles_p, chunks, splits, slots; };
struct BdCfg { int CH, tiles_c, tiles_p, n_ob, Opad32, chunks, splits; };   // Opad32: rows per tap of wd (multiple of 32)
struct BwCfg { int TR, TO, tiles_r, tiles_o, chunks, splits, slots; };
struct BwHaloCfg { int R, nimg, spb, n_bands, tiles_r, tiles_o, splits, bands_per_split; };

// Everything a launcher needs to know about (geom, basis): plan_conv fills it, every entry point reads it and decides nothing else
// (except what depends on the pointers the caller passed: position-major copies, x != xn, dxn).
struct ConvPlan {
    KanPlan pub;                          // the public plan (kan_plan)
    int fast;                             // compile-time spec (FAST_*)
    Route fwd, bwd_data, bwd_weight;
    bool pm_fwd, pm_bwd_data, pm_bwd_weight;     // position-major launches offered (taken when the caller passes the copies)
    bool rowblk_bwd_data;                 // 4x4 planes: row-ordered pixel blocks in the image-major bwd-data launch
    bool quad_fwd;                        // ... B a multiple of 32: the halo forward takes quadrant tiles instead (exact tap skipping)
    bool quad_bd;                         // ... and bwd-data takes quadrant tiles when the caller passes dz_pm (single-tensor specs)
    bool pos8_bd;                         // 8x8 planes, B a multiple of 32: bwd-data takes tiles of 32 images x 4 columns of a plane row when the caller passes dz_pm (484/576 issued)
    bool pos8_bw;                         // 8x8 planes, even B: kan_conv_bwd_weight_rowgroups is offered -- image-pair bands, nine taps per wave, 484/576 issued; its tiles and slabs are p8
    bool rowblk8_fwd;                     // 8x8 planes, 256-output tiles, B a multiple of 4: the halo forward takes half-plane tiles in row order (1/12 skipped)
    bool fwd_wq;                          // 2x2 planes, 3x3 / s1 / p1 / d1: the expanded forward keeps the four output positions on the weight side of a tile
    bool pmdma_xcd, pm_lpt, pm_xcd;       // expanded launches: XCD order of the forward, longest-first and XCD order of the weight gradient
    FwdCfg fc;                            // tap-major / halo / expanded forward tiles
    BdCfg bd;                             // bwd-data tiles
    BwCfg bw;                             // tap-major / expanded weight-gradient tiles
    BwHaloCfg bwh;                        // halo weight-gradient bands (Route::HALO)
    BwHaloCfg p8;                         // kan_conv_bwd_weight_rowgroups (pos8_bw): row groups, 128-output tiles, image-pair bands, its own slab count
    KanBandCfg band;                      // band kernels (fwd or bwd_weight Route::BAND)
};
int plan_conv(const KanGeom* g, const KanBasis* b, ConvPlan* cp);       // 0, or the checks' error (message set)

// live work of position-major tiles (kan_plan.hip)
int live_taps_out(const KanGeom* g, int hw);
int live_taps_in(const KanGeom* g, int hw);
int live_positions_for_tap(const KanGeom* g, int tap);
// XCD-balanced dispatch order of n <= PERM_MAX pixel tiles of the given weights into idx; returns n, or 0 (identity order)
int balance_tiles(const int* weight, int n, unsigned short* idx);
