// Planner of the conv-KAN launches (host only: no kernels in this unit).  plan_conv is the one place that checks a geometry, reads the
// tuning knobs and decides, for each stage, the route (which kernel family), its tiles and its split count; the C-ABI entry points in
// kanconv.hip and kan_direct.hip launch what the ConvPlan says.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "kanconv.h"
#include "kan_device.h"
#include "kan_common.h"
#include "kan_internal.h"

namespace {

int fail(const char* msg) { return kan_fail_msg("%s", msg); }

int check(const KanGeom* g, const KanBasis* b) {
    if (!g || !b) return fail("null geometry/basis");
    if (g->groups < 0 || g->groups > 65535) return fail("groups out of range");
    if (g->B <= 0 || g->C <= 0 || g->O <= 0 || g->H <= 0 || g->W <= 0 || g->Ho <= 0 || g->Wo <= 0) return fail("non-positive dimension");
    if (g->kh <= 0 || g->kw <= 0 || g->sh <= 0 || g->sw <= 0 || g->dh <= 0 || g->dw <= 0 || g->ph < 0 || g->pw < 0) return fail("bad conv parameters");
    if (g->kh > 255 || g->kw > 255 || g->C > 65535) return fail("kernel size / channel count out of supported range");
    if ((g->H + 2 * g->ph - g->dh * (g->kh - 1) - 1) / g->sh + 1 != g->Ho || (g->W + 2 * g->pw - g->dw * (g->kw - 1) - 1) / g->sw + 1 != g->Wo)
        return fail("Ho/Wo inconsistent with H/W, kernel, stride, padding, dilation");
    if ((long long)g->B * g->Ho * g->Wo >= (1ll << 31) || (long long)g->B * g->H * g->W >= (1ll << 31)) return fail("pixel count exceeds int32");
    if ((long long)g->B * g->x_bstride * 4 >= (1ll << 31) || (long long)g->B * g->y_bstride * 4 >= (1ll << 31))
        return fail("activation tensors must be smaller than 2 GiB (32-bit buffer offsets)");
    if (g->x_bstride < (long long)ngroups(g) * g->C * g->H * g->W || g->y_bstride < (long long)ngroups(g) * g->O * g->Ho * g->Wo)
        return fail("batch stride smaller than groups * channels * plane");
    if (b->kind < 0 || b->kind > KAN_BASIS_GRAM) return fail("unknown basis kind");
    const int first = KAN_ORDER_FIRST(b->order), mode = KAN_ORDER_MODE(b->order);      // plane windows (kanconv.h): order = mode | first << 8
    if (first < 0) return fail("negative first-plane offset");
    if (first != 0 && b->kind != KAN_BASIS_POLY && b->kind != KAN_BASIS_CHEBY && b->kind != KAN_BASIS_FOURIER)
        return fail("a first-plane offset (upper bits of order) is taken by the Poly, Cheby and Fourier bases only");
    if (b->kind == KAN_BASIS_GRAM && (b->order < 0 || b->order >= b->n_basis || b->n_basis < 2 || b->act == KAN_ACT_NONE))
        return fail("Gram basis needs degree >= 1, an activation, and a mode (order) in 0..degree-1");
    if (b->kind == KAN_BASIS_RELU && (b->order < 0 || b->order > 2)) return fail("ReLU basis mode (order) must be 0, 1 or 2");
    if (b->kind == KAN_BASIS_FOURIER && (b->n_basis & 1)) return fail("Fourier basis needs an even plane count (cos and sin per frequency)");
    if (b->kind == KAN_BASIS_POLY && (mode < 0 || mode > 1)) return fail("bad recurrence-basis parameters");
    if (b->kind == KAN_BASIS_POLY && first + b->n_basis > 11 && !b->chan_table)
        return fail("a recurrence basis of first + n_basis > 11 planes needs its coefficients as a device table (chan_table)");
    if (b->act < KAN_ACT_NONE || b->act > KAN_ACT_GELU_TANH) return fail("unknown activation");
    int P = b->n_basis + (b->act != KAN_ACT_NONE);
    if (b->n_basis < 1 || P > KAN_MAX_PLANES) return fail("planes per channel exceed KAN_MAX_PLANES");
    if ((long long)g->C * g->kh * g->kw * P >= (1ll << 30)) return fail("GEMM depth too large");
    if (b->kind == KAN_BASIS_BSPLINE) {
        if (b->order < 0 || b->order > 3) return fail("spline_order must be in 0..3");
        const int nk = b->n_basis + b->order + 1;
        if (nk > KAN_MAX_TABLE) return fail("too many knots");
        if (b->n_basis - b->order < 1) return fail("grid_size must be >= 1");
        const float h = (b->table[nk - 1] - b->table[0]) / (float)(nk - 1);
        if (!(h > 0.f)) return fail("knots must be increasing");
        for (int i = 0; i < nk; ++i) {          // the closed-form basis assumes torch.linspace knots (kan_layers.py:184-190)
            float d = b->table[i] - (b->table[0] + h * (float)i);
            if (d < 0) d = -d;
            if (d > 1e-4f * h) return fail("knots must be uniform (torch.linspace), as the reference always builds them");
        }
    }
    if (b->kind == KAN_BASIS_RBF && (b->n_basis > KAN_MAX_TABLE || !(b->p0 != 0.f))) return fail("bad RBF parameters");
    return 0;
}

// Compile-time specialisation available?  (FAST_* in kan_internal.h)
int fast_variant(const KanBasis* b) {
    // a plane window (first != 0) or a device coefficient table is what the compile-time specs do not know: a tail window of 4 planes is no degree-3 layer
    if (KAN_ORDER_FIRST(b->order) != 0 || (b->kind == KAN_BASIS_POLY && b->chan_table)) return FAST_GENERIC;
    if (b->kind == KAN_BASIS_BSPLINE && b->n_basis == 8 && b->order == 3)
        return b->act == KAN_ACT_SILU ? FAST_BSPLINE_SILU : b->act == KAN_ACT_GELU ? FAST_BSPLINE_GELU : FAST_GENERIC;
    if (b->kind == KAN_BASIS_RBF && b->act == KAN_ACT_SILU && (b->n_basis == 8 || b->n_basis == 5)) return b->n_basis == 8 ? FAST_RBF8 : FAST_RBF5;
    if (b->kind == KAN_BASIS_CHEBY && b->act == KAN_ACT_NONE) return b->n_basis == 5 ? FAST_CHEBY5 : b->n_basis == 4 ? FAST_CHEBY4 : FAST_GENERIC;
    if (b->kind == KAN_BASIS_POLY && b->act != KAN_ACT_NONE)
        return b->n_basis == 4 ? FAST_POLY4 : b->n_basis == 3 ? FAST_POLY3 : b->n_basis == 1 ? FAST_POLY1 : FAST_GENERIC;
    if (b->kind == KAN_BASIS_RELU && b->act == KAN_ACT_SILU && b->n_basis == 8) return FAST_RELU8;
    if (b->kind == KAN_BASIS_GRAM && b->act == KAN_ACT_SILU && b->n_basis == 4) return FAST_GRAM4;
    return FAST_GENERIC;
}

// A/B switches for kernel experiments (NAME=0 turns a code path off).  The shipped library has none: it reads no
// environment variable (include/kanconv.h).  Build with -DKAN_TUNING_KNOBS to get them.
bool tuning_off(const char* name) {
#ifdef KAN_TUNING_KNOBS
    const char* e = getenv(name);
    return e && atoi(e) == 0;
#else
    (void)name;
    return false;
#endif
}
bool tuning_on(const char* name) {              // opt-in experiments (NAME=1), same build flag
#ifdef KAN_TUNING_KNOBS
    const char* e = getenv(name);
    return e && atoi(e) != 0;
#else
    (void)name;
    return false;
#endif
}

// Position-major pixel order (and with it tap skipping) is offered on small padded planes (<= 16 positions: 31 % of
// the products are dead on 4x4, 56 % on 2x2).  Lanes then walk images, so the kernels must be given the [C*H*W][B]
// copies of their gathered inputs (kan_position_major); without a copy they stay on the image-major path (on NCHW the
// strided 4-byte gathers cost more than 4x4 skipping saves).  Masks are 32-bit.  Not for FastKAN (second input tensor).
// Measured on KAN-VGG11 (bs 256): the weight-gradient kernel gains 27 % on 4x4 planes and 65 % on 2x2; forward and
// bwd-data gain 40-60 % on 2x2 but nothing on 4x4 (their step latency, not the step count, sets the time there), so
// they take the position-major path only up to 4 positions.
enum { PM_FWD = 0, PM_BWD_DATA = 1, PM_BWD_WEIGHT = 2 };
// The DMA-only forward on the expanded position-major operand (k_conv_fwd_pmdma): default B-spline specs (P = 9: 18-row steps),
// channel pairs, 128-image and 128-output tiles.  Measured on 4x4 planes it LOSES to the dense halo forward (256->512: 0.76 vs 0.63 ms,
// 512->512: 1.36 vs 1.24 -- 16 positions x 2 image tiles walk the 85 MB weight stream out of step), so the forward's position-major
// limit stays at 4 positions (2x2 planes: 0.247 -> 0.211 ms); -DKAN_TUNING_KNOBS + KAN_PMDMA_FWD16=1 re-runs the experiment.
bool pmdma_fwd_shape(const KanGeom* g, int f) {
    return !tuning_off("KAN_PMDMA_FWD") && fast_has(f, ON_EXPANDED_FWD) && g->C % 2 == 0 && g->B % 128 == 0 && ((g->O + 63) / 64 * 64) % 128 == 0 &&
           (long long)g->C * g->H * g->W * 9 * g->B * 4 < (1ll << 31);
}
bool want_pix_major(const KanGeom* g, const KanBasis* b, int which, bool pmdma_shape) {
    const int plane = which == PM_BWD_DATA ? g->H * g->W : g->Ho * g->Wo;
    const int limit = which == PM_BWD_WEIGHT ? 16 : (which == PM_FWD && pmdma_shape && tuning_on("KAN_PMDMA_FWD16")) ? 16 : 4;
    return b->kind != KAN_BASIS_RBF && plane <= limit && g->kh * g->kw <= 32 && (g->ph > 0 || g->pw > 0) && g->B >= 16;
}

// Split-K factor.  The conv kernels keep 4 workgroups per CU resident (1024 on the chip), so a grid of W workgroups
// runs in ceil(W/1024) rounds and wastes the empty part of the last one (1184 workgroups = 58 % efficiency).  Model the
// time of s splits as rounds(s) * (steps per workgroup + a fixed per-workgroup cost of ~6 steps for prologue, tile
// store and the extra slab) and take the cheapest s with at least min_chunks steps per split and no empty split.
// One slab costs its consumer a pass over `slab_bytes` (~4 TB/s => bytes/4e6 step-units of ~1 us) and never less
// than ~1/6 of a step (latency of the serial slab loop on tiny outputs).
double slab_cost_steps(double slab_bytes) { const double bw = slab_bytes / 4.0e6; return bw > 1.0 / 6.0 ? bw : 1.0 / 6.0; }

int pick_splits(long long tiles, int chunks, int min_chunks, double slab_bytes, long long SLOTS = 1024) {
    int cap = chunks / min_chunks; if (cap < 1) cap = 1;
    if (cap > 1024) cap = 1024;
    int best = 1; double best_cost = -1;
    for (int s = 1; s <= cap; ++s) {
        const int cps = ceil_div(chunks, s);
        if (ceil_div(chunks, cps) != s) continue;            // would leave an empty split
        const long long rounds = (tiles * s + SLOTS - 1) / SLOTS;
        // + the consumer's serial pass over the s slabs (measured: 1024 slabs of a 62 KB tile cost the reducer 170 us,
        // i.e. ~1/6 of a step each) -- only matters for tiny outputs split hundreds of ways (layer 0's weight gradient)
        const double cost = (double)(rounds * (cps + 6)) + s * slab_cost_steps(slab_bytes);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = s; }
    }
    return best;
}

// 256-output tiles (512 threads, 2 workgroups per CU): every expanded input value then feeds 256 outputs instead of 128,
// which halves the staging work (basis evaluation + LDS writes: ~13 % of the forward kernel's time, measured by
// ablation) per MFMA.  Offered where the compile-time basis specs exist and O is a multiple of 256.
bool big_tiles(int f, const KanPlan& pl) {
    const bool off = tuning_off("KAN_BIG");
    return !off && pl.Opad % 256 == 0 && fast_has(f, ON_BIG_TILES);
}
// Halo forward kernel (k_conv_fwd_halo): 3x3 / stride 1 / pad 1 layers of the default B-spline specs whose 128-pixel
// tiles are whole row blocks of one image or whole images (the KAN-VGG shapes 32x32, 16x16, 8x8, 4x4).
bool halo_fwd(const KanGeom* g, const KanBasis* b, int f, bool pm_fwd) {
    const bool off = tuning_off("KAN_HALO");
    if (off || !fast_has(f, ON_HALO_FWD)) return false;     // B-spline defaults, ChebyKAN degree 3, recurrence families degree 3, ReLU-KAN / GRAM-KAN defaults
    if (b->kind == KAN_BASIS_POLY && b->order == 0) return false;          // order 0 = basis on a second, pre-normalised tensor (LegendreKAN): tap-major kernel
    if (g->kh != 3 || g->kw != 3 || g->sh != 1 || g->sw != 1 || g->dh != 1 || g->dw != 1 || g->ph != 1 || g->pw != 1) return false;
    if ((g->C & 1) || g->O % 128 != 0) return false;
    if (pm_fwd) return false;
    const int W = g->W, H = g->H;
    return (W == 32 && H % 4 == 0) || (W == 16 && H % 8 == 0) || (W == 8 && H == 8) || (W == 4 && H == 4);
}
// Band forward kernel (kan_direct.hip): the layers that would otherwise run the tap-major kernel on 64-output tiles -- few input channels
// (a model's first layer: the whole GEMM depth is a few hundred rows and re-expanding the input once per tap is most of the kernel) or an
// output count that fills no 128-wide tile (64 -> 192) -- with a compile-time basis spec.  Any kernel size, stride, dilation, padding.
bool band_fwd(const KanGeom* g, const KanBasis* b, int f, bool dw, bool pm_fwd, bool halo, KanBandCfg* out) {
    if (tuning_off("KAN_BAND") || !fast_has(f, ON_BAND_FWD)) return false;
    if (b->kind == KAN_BASIS_POLY && b->order == 0) return false;            // (LegendreKAN: second input tensor; keep it on the tap-major kernel for now)
    if (dw || pm_fwd || halo) return false;
    // ... and (round 3, measured on the 13x13 ChebyKAN-AlexNet layers) every other layer of >= 4 taps that the halo kernel's plane list does not cover:
    // one expansion per channel group instead of one per tap
    if (!(g->C <= 3 || round_up(g->O, 64) % 128 != 0 || (g->kh * g->kw >= 4 && g->C % 2 == 0 && !tuning_off("KAN_BAND_WIDE")))) return false;
    kan_band_cfg(g, b, f, out);
    return out->ok != 0;
}
FwdCfg fwd_cfg(const KanGeom* g, const KanPlan& pl, bool big, bool pm_fwd, bool halo) {
    FwdCfg c;
    c.TO = (big && !pm_fwd) ? 256 : (pl.Opad % 128 == 0) ? 128 : 64;   // (2x2 planes: -17 % with 256)
    c.slots = c.TO == 256 ? 512 : 1024;
    c.TP = 128;
    c.tiles_o = pl.Opad / c.TO;
    c.tiles_p = ceil_div((long long)g->B * g->Ho * g->Wo, c.TP);
    c.chunks = pl.Kpad / pl.KC;
    c.splits = pick_splits((long long)c.tiles_o * c.tiles_p * ngroups(g), c.chunks, 8, 4.0 * g->B * g->O * g->Ho * g->Wo * ngroups(g), c.slots);
    if (halo) {                                      // the halo kernel splits the depth axis between channel pairs (9 steps each)
        const int n_pairs = g->C / 2, pps = ceil_div(n_pairs, c.splits < n_pairs ? c.splits : n_pairs);
        c.splits = ceil_div(n_pairs, pps);
    }
    return c;
}
// Row-ordered pixel blocks on 4x4 planes (k_conv_fwd_halo ROWBLK, k_conv_bwd_data RB): 1/6 of the MFMA blocks multiply the zero border and are skipped
bool rowblk_bwd_data(const KanGeom* g, int f, bool pm_bwd_data) {
    return !tuning_off("KAN_BD_ROWBLK") && fast_has(f, ON_ROWBLK_BWD_DATA) && !pm_bwd_data && g->H == 4 && g->W == 4 && g->Ho == 4 && g->Wo == 4 &&
           g->kh == 3 && g->kw == 3 && g->sh == 1 && g->sw == 1 && g->ph == 1 && g->pw == 1 && g->dh == 1 && g->dw == 1 && g->B % 8 == 0 && g->O % 16 == 0;
}
// With dead-tap skipping the tiles of one launch carry 4/9 ... 9/9 of the nominal work depending on their pixel
// position (or tap, for the weight gradient).  Each tile therefore gets its own split count ceil(live steps / target)
// so that every workgroup runs ~`target` live steps, and the target is chosen on the host by the same round model as
// pick_splits, evaluated on the true per-class workgroup counts (a 1088-workgroup grid would run two rounds).
// (Oversubscribing 4x with small equal splits instead was measured 15-40 % slower.)
struct LiveClass { long long tiles; int live_steps; };           // tiles sharing one live-step count

int pick_target_steps(const LiveClass* cls, int ncls, int min_steps, double slab_bytes, int* max_splits, long long SLOTS = 1024) {
    int hi = 1;
    for (int i = 0; i < ncls; ++i) if (cls[i].live_steps > hi) hi = cls[i].live_steps;
    int best = hi; double best_cost = -1; int best_ms = 1;
    for (int t = min_steps < hi ? min_steps : hi; t <= hi; ++t) {
        long long wgs = 0; int ms = 1;
        for (int i = 0; i < ncls; ++i) {
            const int sp = cls[i].live_steps > 0 ? ceil_div(cls[i].live_steps, t) : 1;
            wgs += cls[i].tiles * sp;
            if (sp > ms) ms = sp;
        }
        const long long rounds = (wgs + SLOTS - 1) / SLOTS;
        const double cost = (double)(rounds * (t + 6)) + ms * slab_cost_steps(slab_bytes);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = t; best_ms = ms; }
    }
    *max_splits = best_ms;
    return best;
}
BdCfg bd_cfg(const KanGeom* g, const KanPlan& pl) {
    BdCfg c;
    c.CH = 64 / pl.P;
    c.tiles_c = ceil_div(g->C, 2 * c.CH);
    c.tiles_p = ceil_div((long long)g->B * g->H * g->W, 128);
    c.n_ob = ceil_div(g->O, 16);
    c.Opad32 = round_up(g->O, 32);
    c.chunks = g->kh * g->kw * c.n_ob;
    c.splits = pick_splits((long long)c.tiles_c * c.tiles_p * ngroups(g), c.chunks, 8, 4.0 * g->B * g->C * g->H * g->W * ngroups(g));
    return c;
}
// Halo weight-gradient kernel (k_conv_bwd_weight_halo): 3x3 / stride 1 / pad 1 layers of the default B-spline specs on square
// 16x16 and 8x8 planes (KAN-VGG layers 1-3), whole 128-output tiles, single input tensor.  Its packed gradient is
// CHANNEL-major: row = (c*T + tap)*P + p (kan_unpack_wgrad follows).
// DMA-only position-major weight gradient on the expanded operand (k_conv_bwd_weight_pmdma): default B-spline specs, whole
// 128-row tiles inside one tap, 16-image steps, 128-output tiles.
bool pmdma_bwd_weight(const KanGeom* g, const KanBasis* b, int f, bool want_pm_bw) {
    if (tuning_off("KAN_PMDMA") || !fast_has(f, ON_EXPANDED)) return false;      // B-spline, ReLU-KAN, GRAM-KAN default specs
    if (!want_pm_bw) return false;
    const int P = b->n_basis + (b->act != KAN_ACT_NONE);
    return (g->C * P) % 128 == 0 && g->B % 16 == 0 && round_up(g->O, 64) % 128 == 0 &&
           (long long)g->C * g->H * g->W * P * g->B * 4 < (1ll << 31);
}
bool halo_bwd_weight(const KanGeom* g, int f, bool pmdma_bw) {
    if (tuning_off("KAN_HALO_BW") || !fast_has(f, ON_HALO_BWD_WEIGHT)) return false;
    if (g->kh != 3 || g->kw != 3 || g->sh != 1 || g->sw != 1 || g->dh != 1 || g->dw != 1 || g->ph != 1 || g->pw != 1) return false;
    if (round_up(g->O, 64) % 128 != 0 || g->C > 65535 / 81) return false;      // (row index = (c*9 + tap)*P + p stays far below 2^31)
    if (g->H != g->W) return false;
    // 4x4 planes: two images per band, dense (31 % of the products multiply padding).  The position-major tap-skipping launch
    // wins where it has enough row tiles to balance its unequal taps (measured: 512 -> 512 142 TFLOP/s dense-equivalent against
    // 134 here; 256 -> 512 118 against 134), so it keeps the wide layers.
    if (g->W == 4) return !pmdma_bw && g->B % 2 == 0 && g->C <= 256;
    return g->W == 16 || g->W == 8;
}
BwHaloCfg bw_halo_cfg(const KanGeom* g, const KanPlan& pl) {
    BwHaloCfg c;
    c.R = g->W == 16 ? 4 : g->W;
    c.nimg = g->W == 4 ? 2 : 1;
    c.spb = c.nimg * c.R * g->W / 16;
    c.n_bands = g->B * (g->H / c.R) / c.nimg;
    c.tiles_r = ceil_div(pl.K, 128);
    c.tiles_o = pl.Opad / 128;
    const long long tiles = (long long)c.tiles_r * c.tiles_o * ngroups(g);
    const double slab_bytes = 4.0 * pl.K * pl.Opad * ngroups(g);
    int best = 1; double best_cost = -1;
    for (int sp = 1; sp <= c.n_bands && sp <= 1024; ++sp) {            // the round model of pick_splits, in bands of spb steps
        const int bps = ceil_div(c.n_bands, sp);
        if (ceil_div(c.n_bands, bps) != sp) continue;
        const long long rounds = (tiles * sp + 1023) / 1024;
        const double cost = (double)(rounds * (bps * c.spb + 6)) + sp * slab_cost_steps(slab_bytes);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = sp; }
    }
    c.splits = best;
    c.bands_per_split = ceil_div(c.n_bands, best);
    return c;
}
// Weight gradient on 8x8 planes with exact tap skipping (k_conv_bwd_weight_pos8): default B-spline specs, 3x3 / stride 1 / pad 1 / dilation 1,
// even B (a band is an image pair), any C and O.  A workgroup is one row group (32 (c, p) pairs under all nine taps) x 128 outputs; 144
// accumulators leave two workgroups per CU, so the round model fills 512 slots, not 1024.  A step here is one plane row of an image pair:
// ~60 MFMAs per wave against the 32 of a halo step, counted as two.  Every split takes at least two bands where there are two.
// Kept out: launches of more than 8 bands that fill under one workgroup per CU at their split count -- the plan's own route cuts those
// finer (16 -> 128 at B = 32: 352 workgroups on the halo kernel's one-image bands, 40 here).
bool pos8_bw_cfg(const KanGeom* g, int f, bool dw, BwHaloCfg* out) {
    if (tuning_off("KAN_POS8_BW") || !fast_has(f, ON_HALO_BWD_WEIGHT) || fast_kind(f) != KAN_BASIS_BSPLINE || dw) return false;
    if (g->H != 8 || g->W != 8 || g->Ho != 8 || g->Wo != 8 || g->kh != 3 || g->kw != 3 || g->sh != 1 || g->sw != 1 || g->ph != 1 || g->pw != 1 ||
        g->dh != 1 || g->dw != 1) return false;
    if (g->B % 2 != 0 || g->C > 65535 / 81) return false;
    if ((long long)g->B * g->x_bstride * 4 >= (1ll << 31) || (long long)g->B * g->y_bstride * 4 >= (1ll << 31)) return false;
    BwHaloCfg c;
    const int P = fast_planes(f), Opad = round_up(g->O, 64);
    c.R = 8; c.nimg = 2; c.spb = 8;
    c.n_bands = g->B / 2;
    c.tiles_r = ceil_div(g->C * P, 32);
    c.tiles_o = ceil_div(Opad, 128);
    const long long tiles = (long long)c.tiles_r * c.tiles_o * ngroups(g);
    const double slab_bytes = 4.0 * g->C * 9 * P * Opad * ngroups(g);
    int best = 1; double best_cost = -1;
    for (int sp = 1; sp <= c.n_bands && sp <= 1024; ++sp) {
        const int bps = ceil_div(c.n_bands, sp);
        if (ceil_div(c.n_bands, bps) != sp || (bps < 2 && c.n_bands >= 2)) continue;
        const long long rounds = (tiles * sp + 511) / 512;
        const double cost = (double)(rounds * (bps * c.spb * 2 + 6)) + sp * slab_cost_steps(slab_bytes);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = sp; }
    }
    c.splits = best;
    c.bands_per_split = ceil_div(c.n_bands, best);
    if (c.n_bands > 8 && tiles * c.splits < 256) return false;
    *out = c;
    return true;
}
BwCfg bw_cfg(const KanGeom* g, const KanPlan& pl, bool big, bool pm_bw) {
    BwCfg c;
    c.TO = (big && !pm_bw) ? 256 : (pl.Opad % 128 == 0) ? 128 : 64;
    c.slots = c.TO == 256 ? 512 : 1024;
    c.TR = c.TO == 64 ? 256 : 128;
    c.tiles_r = ceil_div(pl.K, c.TR);
    c.tiles_o = pl.Opad / c.TO;
    c.chunks = ceil_div((long long)g->B * g->Ho * g->Wo, 16);
    c.splits = pick_splits((long long)c.tiles_r * c.tiles_o * ngroups(g), c.chunks, 16, 4.0 * pl.K * pl.Opad * ngroups(g), c.slots);
    return c;
}

// Depthwise groups (one input channel, <= 2 outputs per group, <= 9 taps): direct kernels instead of GEMM tiles.
bool dw_direct(const KanGeom* g, const KanBasis* b) {
    const bool off = tuning_off("KAN_DW");
    const int T = g->kh * g->kw, P = b->n_basis + (b->act != KAN_ACT_NONE);
    return !off && g->C == 1 && g->O <= 2 && T <= DW_T && T * P <= DW_MAX_TP;
}
int dw_weight_chunks(const KanGeom* g) {           // slabs of the depthwise weight gradient: ~2048 blocks over all groups
    const long long total = (long long)g->B * g->Ho * g->Wo;
    int s = ceil_div(2048, ngroups(g));
    const int most = ceil_div(total, 256);
    if (s > most) s = most;
    if (s > 64) s = 64;
    return s < 1 ? 1 : s;
}

}  // namespace

int live_taps_out(const KanGeom* g, int hw) {
    int n = 0;
    for (int tap = 0; tap < g->kh * g->kw; ++tap) {
        const int r = tap / g->kw, t = tap % g->kw, ho = hw / g->Wo, wo = hw % g->Wo;
        const int hi = ho * g->sh - g->ph + r * g->dh, wi = wo * g->sw - g->pw + t * g->dw;
        n += (hi >= 0 && hi < g->H && wi >= 0 && wi < g->W);
    }
    return n;
}
int live_taps_in(const KanGeom* g, int hw) {
    int n = 0;
    for (int tap = 0; tap < g->kh * g->kw; ++tap) {
        const int r = tap / g->kw, t = tap % g->kw, h = hw / g->W, w = hw % g->W;
        const int hn = h + g->ph - r * g->dh, wn = w + g->pw - t * g->dw;
        n += (hn >= 0 && wn >= 0 && hn % g->sh == 0 && wn % g->sw == 0 && hn / g->sh < g->Ho && wn / g->sw < g->Wo);
    }
    return n;
}
int live_positions_for_tap(const KanGeom* g, int tap) {
    int n = 0;
    for (int hw = 0; hw < g->Ho * g->Wo; ++hw) {
        const int r = tap / g->kw, t = tap % g->kw, ho = hw / g->Wo, wo = hw % g->Wo;
        const int hi = ho * g->sh - g->ph + r * g->dh, wi = wo * g->sw - g->pw + t * g->dw;
        n += (hi >= 0 && hi < g->H && wi >= 0 && wi < g->W);
    }
    return n;
}

// Workgroups are dealt to the 8 XCDs round-robin by linear block id and never migrate.  Position-major pixel tiles are
// ordered by position, so without care XCD k would get only the tiles of positions k, k+8, ... -- all light (corner)
// or all heavy (centre) ones (measured: half the chip idle).  The host therefore deals the pixel tiles to 8 bins in
// snake order of decreasing live work and hands the kernel the resulting order.
int balance_tiles(const int* weight, int n, unsigned short* idx) {
    if (n < 2 || n > PERM_MAX) return 0;
    int order[PERM_MAX];
    for (int i = 0; i < n; ++i) order[i] = i;
    for (int i = 1; i < n; ++i) {                                   // insertion sort, heaviest first (stable)
        int v = order[i], j = i;
        while (j > 0 && weight[order[j - 1]] < weight[v]) { order[j] = order[j - 1]; --j; }
        order[j] = v;
    }
    // rank r goes to slot (bin = snake(r), depth = r / 8); slot s = depth*8 + bin is dispatched s-th => XCD = bin
    for (int r = 0; r < n; ++r) {
        const int depth = r / 8, k = r % 8, bin = (depth & 1) ? 7 - k : k;
        int slot = depth * 8 + bin;
        if (slot >= n) slot = r;                                    // ragged last row: keep it simple
        idx[slot] = (unsigned short)order[r];
    }
    // the ragged fallback can collide; verify it is a permutation, else identity
    bool seen[PERM_MAX] = {false};
    for (int i = 0; i < n; ++i) { if (idx[i] >= n || seen[idx[i]]) return 0; seen[idx[i]] = true; }
    return n;
}

int plan_conv(const KanGeom* g, const KanBasis* b, ConvPlan* cp) {
    if (int rc = check(g, b)) return rc;
    ConvPlan& c = *cp;
    KanPlan* pl = &c.pub;
    const int T = g->kh * g->kw, G = ngroups(g), f = fast_variant(b);
    c.fast = f;
    // ---- every predicate, once
    const bool pm_shape = pmdma_fwd_shape(g, f);
    c.pm_fwd = want_pix_major(g, b, PM_FWD, pm_shape);
    c.pm_bwd_data = want_pix_major(g, b, PM_BWD_DATA, false);
    const bool want_pm_bw = want_pix_major(g, b, PM_BWD_WEIGHT, false);
    const bool dw = dw_direct(g, b);
    const bool halo = halo_fwd(g, b, f, c.pm_fwd);
    c.band.ok = c.band.bw_ok = 0;
    const bool band = band_fwd(g, b, f, dw, c.pm_fwd, halo, &c.band);
    const bool pmdma_fwd = pm_shape && c.pm_fwd;
    const bool pmdma_bw = pmdma_bwd_weight(g, b, f, want_pm_bw);
    const bool halo_bw = halo_bwd_weight(g, f, pmdma_bw);
    c.pm_bwd_weight = want_pm_bw && !halo_bw;
    const bool band_bw = band && c.band.bw_ok && !want_pm_bw && !tuning_off("KAN_BAND_BW");
    // the weight gradient's own entry on 8x8 planes (kan_conv_bwd_weight_rowgroups): offered beside the plan's route, with its own slab count, so that
    // nothing in KanPlan moves (kan_tile_orders reports it)
    c.pos8_bw = pos8_bw_cfg(g, f, dw, &c.p8);
    c.rowblk_bwd_data = rowblk_bwd_data(g, f, c.pm_bwd_data);
    c.pmdma_xcd = tuning_on("KAN_PMDMA_XCD");
    c.pm_lpt = !tuning_off("KAN_PM_LPT");
    c.pm_xcd = !tuning_off("KAN_PM_XCD");
    c.fwd = dw ? Route::DW : band ? Route::BAND : halo ? Route::HALO : pmdma_fwd ? Route::EXPANDED : Route::TAP_MAJOR;
    c.bwd_data = dw ? Route::DW : Route::TAP_MAJOR;
    c.bwd_weight = dw ? Route::DW : band_bw ? Route::BAND : halo_bw ? Route::HALO : pmdma_bw ? Route::EXPANDED : Route::TAP_MAJOR;
    // ---- packing and sizes
    pl->P = b->n_basis + (b->act != KAN_ACT_NONE);
    pl->K = g->C * T * pl->P;
    {   // LDS step of the forward kernel: KC in {16, 18} rows holding IPC <= 4 whole items; take the one wasting fewer rows
        int i18 = 18 / pl->P, i16 = 16 / pl->P;
        if (i18 > 4) i18 = 4;
        if (i16 > 4) i16 = 4;
        const bool use18 = (long long)i18 * pl->P * 16 > (long long)i16 * pl->P * 18;   // i18*P/18 > i16*P/16
        pl->KC = use18 ? 18 : 16;
        pl->IPC = use18 ? i18 : i16;
        // 10 - 12 planes (FourierKAN grid 5: P = 11) hold ONE item in either step and leave 31 - 44 % of the rows -- of the MFMA work -- as zero padding:
        // a 12-row step wastes 0 - 17 % (round 3; the generic forward is the only kernel that pays for pad rows)
        if (pl->P >= 10 && pl->P <= 12) { pl->KC = 12; pl->IPC = 1; }
        if (halo) { pl->KC = 2 * pl->P; pl->IPC = 2; }      // pair order: one step = one tap of a channel pair, no pad rows
    }
    pl->Kpad = ceil_div(g->C * T, pl->IPC) * pl->KC;
    if (band) { pl->KC = c.band.NPLE; pl->IPC = c.band.NG; pl->Kpad = c.band.n_steps * c.band.NPLE; }      // band order: steps of even(NG * P) rows
    pl->Opad = round_up(g->O, 64);
    pl->packed_weight_bytes = (long long)G * pl->Kpad * pl->Opad * 4;
    c.bd = bd_cfg(g, *pl);
    pl->bwd_data_weight_bytes = (long long)G * T * c.bd.Opad32 * c.bd.tiles_c * 128 * 4;
    pl->fwd_slab_elems = (long long)g->B * g->y_bstride;
    pl->bwd_data_slab_elems = (long long)g->B * g->x_bstride;
    pl->bwd_weight_slab_elems = (long long)G * pl->K * pl->Opad;
    // ---- tiles and splits
    const bool big = big_tiles(f, *pl);
    c.fc = fwd_cfg(g, *pl, big, c.pm_fwd, halo);
    c.bw = bw_cfg(g, *pl, big, c.pm_bwd_weight);
    if (halo_bw) c.bwh = bw_halo_cfg(g, *pl);
    pl->fwd_splits = band ? c.band.fwd_splits : c.fc.splits;
    pl->bwd_data_splits = c.bd.splits;
    pl->bwd_weight_splits = halo_bw ? c.bwh.splits : c.bw.splits;
    if (band_bw) {
        pl->bwd_weight_splits = c.band.bw_splits;
        pl->bwd_weight_slab_elems = (long long)G * pl->Kpad * pl->Opad;      // rows as the packed forward weights (pad rows included)
    }
    pl->fwd_target = pl->bwd_data_target = pl->bwd_weight_target = 0;
    const bool rowblk_fwd = halo && g->H == 4 && g->W == 4 && c.fc.TO == 256;
    // quadrant tiles (32 images x a 2x2 quadrant) where the row-block order is taken and whole 32-image groups exist: same tile count (B / 8),
    // same splits and slabs -- an internal choice of pixel order, invisible in KanPlan
    c.quad_fwd = rowblk_fwd && g->B % 32 == 0 && !tuning_off("KAN_QUAD_FWD");
    // bwd-data on the same tile, its dz copies fed from the position-major copy the caller passes for the expanded weight gradient (128 contiguous bytes per
    // (output, position) and 32 images); without dz_pm the launcher keeps the row blocks
    c.quad_bd = c.rowblk_bwd_data && g->B % 32 == 0 && !tuning_off("KAN_QUAD_BD");
    // 8x8 planes: row blocks on half-plane tiles of 4 images (k_conv_fwd_halo<4, 8, 4, 4>) instead of whole planes of 2: the same B / 2 tiles, splits
    // and slabs, again invisible in KanPlan (row_blocks stays 0 for these geometries)
    c.rowblk8_fwd = halo && g->H == 8 && g->W == 8 && c.fc.TO == 256 && g->B % 4 == 0 && !tuning_off("KAN_ROWBLK8_FWD");
    // 8x8 planes, bwd-data: tiles of 32 images x 4 adjacent columns of one plane row, fed from dz_pm when the caller passes it (the plan does not ask for the
    // copy: dz_pm_wanted stays 0; ops builds it where kan_tile_orders reports this bit).  The same B / 2 tiles, splits and slabs; exactly the 484 of 576
    // (position, tap) blocks with a source are issued.  The epilogue moves x and dx 16 bytes at a time.
    c.pos8_bd = !tuning_off("KAN_POS8_BD") && fast_has(f, ON_ROWBLK_BWD_DATA) && !c.pm_bwd_data && !dw && g->H == 8 && g->W == 8 && g->Ho == 8 && g->Wo == 8 &&
                g->kh == 3 && g->kw == 3 && g->sh == 1 && g->sw == 1 && g->ph == 1 && g->pw == 1 && g->dh == 1 && g->dw == 1 && g->B % 32 == 0 &&
                g->O % 16 == 0 && g->x_bstride % 4 == 0 && (long long)g->O * 64 * g->B * 4 < (1ll << 31);
    // 2x2 planes under 3x3 / s1 / p1 / d1: the expanded forward puts the four output positions on the weight side of its tiles (32 outputs x 4
    // positions x 128 images: the same 32 tiles per split) and stores whole 16-byte groups z[b][o][0..3]; same steps per split, same slabs
    // bit for bit (0.212 -> 0.153 ms per launch on 512 -> 512); -DKAN_TUNING_KNOBS + KAN_PMDMA_FWD_WQ=0 runs the other order
    c.fwd_wq = c.fwd == Route::EXPANDED && g->H == 2 && g->W == 2 && g->Ho == 2 && g->Wo == 2 && g->kh == 3 && g->kw == 3 && g->sh == 1 && g->sw == 1 &&
               g->ph == 1 && g->pw == 1 && g->dh == 1 && g->dw == 1 && pl->P == 9 && pl->KC == 18 && g->y_bstride % 4 == 0 && !tuning_off("KAN_PMDMA_FWD_WQ");
    if (dw) {                                   // direct depthwise kernels: no split-K on the data path, no position-major copies
        pl->fwd_splits = pl->bwd_data_splits = 1;
        pl->bwd_weight_splits = dw_weight_chunks(g);
        pl->bwd_data_weight_bytes = pl->packed_weight_bytes;      // the direct bwd-data kernel reads the forward layout: wd = copy of wp
        c.pm_fwd = c.pm_bwd_data = c.pm_bwd_weight = false;
    }
    if (c.pm_fwd) {                             // forward: one class per output position; a tap holds C/IPC steps
        LiveClass cls[16]; const int plane = g->Ho * g->Wo;
        const long long tiles_per_pos = (long long)ceil_div(g->B, c.fc.TP) * c.fc.tiles_o * G;
        for (int hw = 0; hw < plane; ++hw) cls[hw] = LiveClass{tiles_per_pos, live_taps_out(g, hw) * ceil_div(g->C, pl->IPC)};
        pl->fwd_target = pick_target_steps(cls, plane, 8, 4.0 * g->B * g->O * g->Ho * g->Wo * G, &pl->fwd_splits, c.fc.slots);
    }
    if (c.pm_bwd_weight) {                      // bwd-weight: one class per tap; a live position holds B/16 steps
        LiveClass cw[32];
        const long long tiles_per_tap = (long long)ceil_div((long long)g->C * pl->P, c.bw.TR) * c.bw.tiles_o * G;
        for (int tap = 0; tap < T; ++tap) cw[tap] = LiveClass{tiles_per_tap, live_positions_for_tap(g, tap) * ceil_div(g->B, 16)};
        pl->bwd_weight_target = pick_target_steps(cw, T, 16, 4.0 * pl->K * pl->Opad * G, &pl->bwd_weight_splits, c.bw.slots);
    }
    if (c.pm_bwd_data) {                        // bwd-data: one class per input position; a tap holds n_ob steps
        LiveClass cls[16]; const int plane = g->H * g->W;
        const long long tiles_per_pos = (long long)ceil_div(g->B, 128) * c.bd.tiles_c * G;
        for (int hw = 0; hw < plane; ++hw) cls[hw] = LiveClass{tiles_per_pos, live_taps_in(g, hw) * c.bd.n_ob};
        pl->bwd_data_target = pick_target_steps(cls, plane, 8, 4.0 * g->B * g->C * g->H * g->W * G, &pl->bwd_data_splits);
    }
    // ---- the informational flags, from the routes
    pl->fwd_halo = c.fwd == Route::HALO;
    pl->fwd_band = c.fwd == Route::BAND;
    pl->fwd_expanded = c.fwd == Route::EXPANDED;
    pl->bwd_weight_halo = c.bwd_weight == Route::HALO;
    pl->bwd_weight_band = c.bwd_weight == Route::BAND;
    pl->bwd_weight_expanded = c.bwd_weight == Route::EXPANDED;
    pl->x_pm_wanted = (c.pm_fwd && c.fwd != Route::EXPANDED) || (c.pm_bwd_weight && c.bwd_weight != Route::EXPANDED);
    pl->dz_pm_wanted = c.pm_bwd_data || c.pm_bwd_weight;
    pl->e_pm_wanted = pl->fwd_expanded || pl->bwd_weight_expanded;
    pl->e_pm_elems = pl->e_pm_wanted ? (long long)G * g->C * g->H * g->W * pl->P * g->B + 256 : 0;      // + a pad the expansion kernel may scribble on
    pl->row_blocks = (rowblk_fwd ? 1 : 0) | (c.rowblk_bwd_data ? 2 : 0);
    return 0;
}

// What the band launchers will run for (geom, basis): a copy out of the KanBandCfg they read, nothing decided here.
int kan_band_route(const KanGeom* g, const KanBasis* b, KanBandRoute* r) {
    static_assert(KAN_BAND_ROUTE_PHASES == KAN_BAND_MAX_PHASES, "phase_taps holds one entry per band phase");
    if (!r) return fail("null route in kan_band_route");
    memset(r, 0, sizeof(*r));
    ConvPlan cp;
    if (int rc = plan_conv(g, b, &cp)) return rc;
    const KanBandCfg& c = cp.band;
    if (cp.fwd == Route::BAND) {
        r->fwd_band = 1;
        r->fast = c.fast; r->P = c.P; r->NG = c.NG; r->NPLE = c.NPLE; r->NGR = c.NGR;
        r->MO = c.MO; r->WP = c.WP; r->TO = c.TO; r->TP = c.TP; r->NT = c.NT; r->tiles_o = c.tiles_o; r->tiles_p = c.tiles_p;
        r->n_phase = c.n_phase; r->empty_phase = c.n_phase < g->sh * g->sw ? 1 : 0; r->n_steps = c.n_steps;
        for (int ph = 0; ph < c.n_phase; ++ph) r->phase_taps[ph] = c.ph_tap0[ph + 1] - c.ph_tap0[ph];
        r->HC = c.HC; r->span_r = c.span_r; r->cells = c.cells; r->slots = c.slots; r->lds_bytes = c.lds_bytes;
        r->fwd_splits = c.fwd_splits; r->max_images = c.img_max;
    }
    if (cp.bwd_weight == Route::BAND) {
        r->bw_band = 1;
        r->bw_WR = c.bw_WR; r->bw_NI = c.bw_NI; r->bw_slots = c.bw_slots; r->bw_TPI = c.bw_TPI; r->bw_ptiles = c.bw_ptiles;
        r->bw_row_tiles = c.bw_row_tiles; r->bw_cells = c.bw_cells; r->bw_lds_bytes = c.bw_lds_bytes; r->bw_splits = c.bw_splits;
    }
    return 0;
}
