/*
 * kanconv.h -- C ABI of libkanconv.so: MI355X (gfx950) kernels for the conv-KAN hot path.
 *
 * The reference (GadGadGad/Convolutional-KAN-for-Image-Classification) has NO native
 * interface for this path: it is ~60 eager ATen ops per layer call.  The entry points
 * below are what a ctypes/cffi binding placed inside the reference's layer classes would
 * call instead of those op sequences.  Each declaration cites the
 * reference lines it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless stated otherwise;
 *   - the caller owns every buffer, including workspaces; the library never allocates,
 *     frees or synchronises the device; all work is enqueued on `stream`
 *     (a hipStream_t passed as void*);
 *   - return value: 0 on success, <0 on error; message via kan_last_error() (thread-local);
 *   - no C++ exception crosses the boundary; no mutable global state, except one: a mutex-guarded
 *     record of the (kernel, device) pairs whose dynamic-LDS limit the library has raised (once each).
 *
 * Tensor layouts: activations NCHW.  KanGeom describes ONE group of the reference layer
 * (kan_layers.py:249-258 loops over groups in Python); `groups` = G > 1 runs G such groups in
 * the same launches: group j reads channels [j*C, (j+1)*C) of x and writes channels
 * [j*O, (j+1)*O) of z, x / z point at group 0's first channel and the batch strides
 * (`x_bstride`, `y_bstride`) are those of the FULL tensors.  Per-group weights are stacked on a
 * leading axis; every packed / workspace layout is G per-group blocks back to back.
 */
#ifndef KANCONV_H
#define KANCONV_H

#ifdef __cplusplus
extern "C" {
#endif

#define KAN_MAX_PLANES 16   /* basis planes per input channel incl. the base-activation plane */
#define KAN_MAX_TABLE  32   /* knots (B-spline) or centres (RBF) */
#define KAN_FP_WORDS   192  /* 64-bit words of the fingerprint ring of kan_pack_weights_cached (3 slots x 64) */

/* basis families */
enum { KAN_BASIS_BSPLINE = 0, KAN_BASIS_RBF = 1, KAN_BASIS_CHEBY = 2, KAN_BASIS_POLY = 3, KAN_BASIS_FOURIER = 4, KAN_BASIS_RELU = 5, KAN_BASIS_GRAM = 6 };
/* base-branch activations; KAN_ACT_NONE = layer has no base branch (ChebyKAN) */
enum { KAN_ACT_NONE = -1, KAN_ACT_IDENTITY = 0, KAN_ACT_GELU = 1, KAN_ACT_SILU = 2, KAN_ACT_RELU = 3,
       KAN_ACT_TANH = 4, KAN_ACT_SIGMOID = 5, KAN_ACT_GELU_TANH = 6 };

/* Geometry of ONE group's convolution (all fields in elements, not bytes). */
typedef struct KanGeom {
    int B, C, H, W;              /* input block: batch, channels of this group, height, width */
    int O, Ho, Wo;               /* output block of this group */
    int kh, kw, sh, sw, ph, pw, dh, dw;
    int groups;                  /* G groups handled by one call (0 is read as 1); C and O stay PER GROUP */
    long long x_bstride;         /* distance between images in x / dx  (C_total*H*W)   */
    long long y_bstride;         /* distance between images in z / dz  (O_total*Ho*Wo) */
} KanGeom;

/* Basis description.
 *   B-spline : n_basis = grid_size + spline_order, order = spline_order,
 *              table[0 .. n_basis+order] = the fp32 knots of torch.linspace
 *              (layers/kan_layers.py:184-190); must be uniform, as the reference always
 *              builds them (non-uniform knots are rejected)
 *   RBF      : n_basis = grid_size, table[0..n_basis-1] = centres, p0 = denominator
 *              (utils/utils.py:28-30)
 *   Chebyshev: n_basis = degree + 1, p0 / p1 = clamp bounds (-1+1e-7, 1-1e-7 as fp32)
 *              (layers/cheby_kan_layers.py:93-96)
 *   Poly     : three-term-recurrence families (Bessel, Fibonacci, Gegenbauer, Hermite, Laguerre, Lucas, Taylor, Jacobi:
 *              layers/<family>_kan_layers.py compute_*_basis).  n_basis planes T_0..T_{n-1} of t = tanh(x) (order = 1)
 *              or t = x (order = 0):  T_0 = table[0], T_1 = table[1]*t + table[2],
 *              T_k = (table[3k-3]*t + table[3k-2]) * T_{k-1} + table[3k-1] * T_{k-2} for k >= 2.  `table` holds 11 planes;
 *              a longer basis (or a plane window, below) passes the same coefficients as a device table: chan_table =
 *              [c0, a1, b1, A_2, B_2, C_2, ...], 3 * (first + n_basis) floats, read instead of `table` when non-NULL
 *   Fourier  : n_basis = 2*grid_size planes cos(k x), k = 1..grid_size, then sin(k x)
 *              (layers/fourier_kan_layers.py:163-187)
 *   ReLU     : n_basis = g + k planes  (r * relu(x - lo[c][j]) * relu(hi[c][j] - x))^2, p0 = r = 4 g^2 / (k+1)^2
 *              (layers/relu_kan_layers.py:118-136).  The phases are PER CHANNEL and trainable, so they live in device
 *              memory: chan_table[c][0][j] = phase_low, chan_table[c][1][j] = phase_high, c = channel inside its group
 *              (the reference shares one phase tensor between the groups).  `order` selects what the non-derivative
 *              planes hold: 0 the basis; 1 / 2 its derivative w.r.t. phase_low / phase_high (base plane zero), so
 *              that kan_conv_bwd_weight yields the factor of the phase gradient,
 *              d phase[c][j] = sum_{o,tap} W[o][c*n+j][tap] * dW_mode[o][c*n+j][tap].
 *   Gram     : n_basis = degree + 1 planes act(P_k(tanh x)), P_0 = 1, P_1 = t, P_k = t P_{k-1} - c_k P_{k-2}, the planes
 *              passed through the layer's activation `act` (layers/gram_kan_layers.py:150-182).  The c_k derive from the
 *              trainable `beta_weights`, so they are read from device memory: chan_table[k] = c_k, k = 2..degree (entries 0, 1
 *              unused; one row for the whole layer).  `order` = 0: the basis; m >= 1: its derivative w.r.t. c_{m+1}
 *              (base plane zero), for the coefficient gradient through kan_conv_bwd_weight as for ReLU.
 * `act` is the base-branch activation (KAN_ACT_NONE: no base branch, no base weight).
 * Planes per channel P = n_basis + (act != KAN_ACT_NONE); P <= KAN_MAX_PLANES.
 *
 * Plane windows.  The conv stage is linear in the planes, so a layer of more planes than one launch holds runs one launch set per
 * window of <= KAN_MAX_PLANES planes and sums the results.  Poly, Cheby and Fourier planes depend on the planes below them, so their
 * launches take a first-plane offset in the upper bits of `order`:
 *     order = KAN_ORDER_PACK(mode, first)       mode = the `order` value described above (low 8 bits), first >= 0
 * The launch emits the family's planes first .. first + n_basis - 1 (Poly: T_first ..; Cheby: T_first ..; Fourier: `first` counts
 * skipped FREQUENCIES -- n_basis = 2m planes cos(k x), k = first+1 .. first+m, then sin(k x) for the same k), bit for bit the planes
 * the same indices get in a launch that starts at 0.  Poly needs chan_table as soon as first + n_basis > 11.  The other kinds take
 * first = 0 only (a B-spline / RBF / ReLU window is a slice of the knots / centres / phases).  Windowed launches run the generic kernels. */
#define KAN_ORDER_PACK(mode, first) ((int)(mode) | ((int)(first) << 8))
#define KAN_ORDER_MODE(order) ((int)(order) & 0xff)
#define KAN_ORDER_FIRST(order) ((int)(order) >> 8)
typedef struct KanBasis {
    int kind, n_basis, order, act;
    float p0, p1;
    float table[KAN_MAX_TABLE];
    const float* chan_table;      /* device pointer: KAN_BASIS_RELU [C][2][n_basis] floats, KAN_BASIS_GRAM [n_basis] floats,
                                     KAN_BASIS_POLY NULL or the coefficient table [3 * (first + n_basis)] floats; else NULL */
} KanBasis;

/* Launch plan for one geometry: split counts and workspace sizes (bytes). */
typedef struct KanPlan {
    int P;                        /* planes per channel */
    int K;                        /* GEMM depth of the forward conv: C*kh*kw*P (= rows of the packed weight gradient) */
    int IPC, KC;                  /* forward packing: IPC (c,tap) items per LDS step of KC = even(IPC*P) rows */
    int Kpad, Opad;               /* dims of the packed weight matrix [Kpad][Opad], Kpad = ceil(C*kh*kw / IPC) * KC */
    int fwd_splits;               /* z is written as fwd_splits partial slabs */
    int bwd_data_splits;          /* dx is written as bwd_data_splits partial slabs */
    int bwd_weight_splits;        /* packed dW is written as bwd_weight_splits partial slabs */
    int fwd_target, bwd_data_target, bwd_weight_target;   /* position-major launches: live steps per split (0 = n/a) */
    int x_pm_wanted, dz_pm_wanted;/* small padded planes: pass position-major copies (kan_position_major) of x / dz to
                                     unlock structural-zero tap skipping; optional, NULL keeps the image-major path */
    int bwd_weight_expanded;      /* the weight gradient reads the expanded copy (kan_conv_bwd_weight_expanded) */
    int row_blocks;               /* informational: bit 0 / bit 1 = the forward / bwd-data launch orders 4x4 planes in row blocks and skips
                                     the 1/6 of its MFMA work that multiplies the zero border; with B a multiple of 32 the forward orders
                                     them in quadrant tiles instead (32 images x a 2x2 quadrant) and skips exactly the dead 11/36 */
    int e_pm_wanted, fwd_expanded;/* small padded planes: the weight gradient (and, with fwd_expanded, the forward) reads the EXPANDED
                                     position-major copy: build it with kan_position_major_expanded (e_pm_elems floats) and call
                                     kan_conv_bwd_weight_expanded / kan_conv_fwd_expanded */
    int fwd_halo, bwd_weight_halo;/* informational: the forward / weight-gradient launch of this geometry uses the halo-tile kernel
                                     (k_conv_fwd_halo / k_conv_bwd_weight_halo) -- profiling tools name their samples by it */
    int fwd_band, bwd_weight_band;/* informational: the forward / weight-gradient launch uses the band kernels (few input channels, or an
                                     output count that fills no 128-wide tile: k_band_fwd / k_band_bwd_weight); wp is then in band order */
    long long packed_weight_bytes;    /* G*Kpad*Opad*4    : all groups, group j at j*Kpad*Opad floats */
    long long bwd_data_weight_bytes;  /* size of the bwd-data weight layout `wd`, all groups (equal blocks) */
    long long fwd_slab_elems;         /* B*y_bstride      : stride between z slabs  */
    long long bwd_data_slab_elems;    /* B*x_bstride      : stride between dx slabs */
    long long bwd_weight_slab_elems;  /* G*K*Opad         : stride between dW slabs, group j at j*K*Opad inside a slab */
    long long e_pm_elems;             /* floats of the expanded position-major copy (0 unless e_pm_wanted) */
} KanPlan;

const char* kan_version(void);
const char* kan_last_error(void);

/* Fill `plan` for (geom, basis).  Pure host arithmetic, no device work. */
int kan_plan(const KanGeom* geom, const KanBasis* basis, KanPlan* plan);

/* Informational, for profiling tools and tests: the pixel order inside the tiles of this geometry's launches, which the launchers choose
 * among orders of the same tile count, splits and slabs (so nothing in KanPlan moves with it).  Bits:
 *   KAN_ORDER_QUAD_FWD     4x4 planes, B % 32 == 0: the halo forward runs quadrant tiles (exactly the live 25/36 of the MFMA blocks issued)
 *   KAN_ORDER_ROWBLK8_FWD  8x8 planes, 256-output tiles, B % 4 == 0: the halo forward runs half-plane tiles of 4 images in row order and skips
 *                          the block of the plane's first / last row under the tap row that leaves the plane (11/12 issued)
 *   KAN_ORDER_QUAD_BWD_DATA 4x4 planes, B % 32 == 0, O % 16 == 0: bwd-data runs quadrant tiles (25/36 issued) when it is given dz_pm and one input tensor;
 *                          otherwise it keeps the row blocks of KanPlan.row_blocks bit 1
 *   KAN_ORDER_FWD_WEIGHT_SIDE 2x2 planes, 3x3 / stride 1 / pad 1 / dilation 1, y_bstride % 4 == 0: the expanded forward (plan.fwd_expanded) runs tiles of
 *                          32 outputs x the 4 output positions x 128 images instead of 128 outputs x 1 position x 128 images and stores z[b][o][0..3] as one
 *                          16-byte group; the slabs are bit for bit those of the other order
 *   KAN_ORDER_POS8_BWD_DATA 8x8 planes, 3x3 / stride 1 / pad 1 / dilation 1, B % 32 == 0, O % 16 == 0, x_bstride % 4 == 0: bwd-data runs tiles of 32 images x
 *                          4 adjacent columns of one plane row and issues exactly the 484 of 576 (position, tap) blocks with a source, when it is given dz_pm
 *                          (which KanPlan.dz_pm_wanted does not ask for on these planes: build it where this bit is set), one input tensor and 16-byte
 *                          aligned x and dx; otherwise it runs the plane-major tiles
 *   KAN_ORDER_POS8_BWD_WEIGHT 8x8 planes, 3x3 / stride 1 / pad 1 / dilation 1, default B-spline specs, even B: the weight gradient has an entry of its own,
 *                          kan_conv_bwd_weight_rowgroups (below), which issues exactly the 484 of 576 (position, tap) blocks with a source; kan_conv_bwd_weight
 *                          keeps running the plan's route and nothing in KanPlan moves
 * 0 for a geometry the planner rejects. */
#define KAN_ORDER_QUAD_FWD 1
#define KAN_ORDER_ROWBLK8_FWD 2
#define KAN_ORDER_QUAD_BWD_DATA 4
#define KAN_ORDER_FWD_WEIGHT_SIDE 8
#define KAN_ORDER_POS8_BWD_DATA 16
#define KAN_ORDER_POS8_BWD_WEIGHT 32
int kan_tile_orders(const KanGeom* geom, const KanBasis* basis);

/* Informational, for tests and profiling tools: what the band kernels (plan.fwd_band / plan.bwd_weight_band) run for this geometry -- the kernel
 * instantiation and the run-time switches of a launch, copied from the configuration kan_conv_fwd and kan_conv_bwd_weight launch from.  Pure host
 * arithmetic, no device work (like kan_norm_route and kan_wav_route).
 *   forward (fwd_band = 1; all forward fields 0 otherwise)
 *     fast: compile-time basis spec (1 B-spline SiLU, 2 B-spline GELU, 3 FastKAN 8 centres, 4 ChebyKAN degree 4, 5 ChebyKAN degree 3, 6 recurrence
 *     families degree 3);  P planes per channel;  NG channels per group (k_band_fwd<.., NG, 2, MO, WP, ..>), NPLE = even(NG P) rows per step, NGR
 *     channel groups;  MO 32-output MFMA blocks per wave, WP waves along the pixels: tile TO = 64 MO outputs x TP = 64 WP pixels, NT threads,
 *     tiles_o x tiles_p tiles;  n_phase stride phases that hold a tap, phase_taps[i] taps in phase i, empty_phase = 1 when some of the sh sw phases
 *     hold none (stride > kernel);  n_steps = NGR taps weight steps;  HC cells per halo row, span_r extra halo rows per image, cells per tile;
 *     slots: live expansion units per thread (1 .. 6);  lds_bytes of dynamic LDS (above 65536: the raised limit);  fwd_splits slabs;  max_images:
 *     the most images any one pixel tile covers (tiles are TP consecutive pixels in (image, row, column) order)
 *   weight gradient (bw_band = 1; all bw_ fields 0 otherwise)
 *     k_band_bwd_weight<.., NG, bw_WR, bw_NI, bw_slots>: bw_WR waves of 32 rows, bw_NI 32-output blocks per wave, 3 or 6 expansion slots;  bw_TPI
 *     128-pixel tiles per image, bw_ptiles of them in all;  bw_row_tiles row tiles of 32 bw_WR rows;  bw_cells halo cells per tile;  bw_lds_bytes;
 *     bw_splits slabs
 * Returns 0 with every field 0 where the plan takes neither band route, and kan_plan's error for a geometry the planner rejects. */
#define KAN_BAND_ROUTE_PHASES 16
typedef struct KanBandRoute {
    int fwd_band, fast, P, NG, NPLE, NGR, MO, WP, TO, TP, NT, tiles_o, tiles_p, n_phase, empty_phase, n_steps, HC, span_r, cells, slots, lds_bytes,
        fwd_splits, max_images;
    int phase_taps[KAN_BAND_ROUTE_PHASES];
    int bw_band, bw_WR, bw_NI, bw_slots, bw_TPI, bw_ptiles, bw_row_tiles, bw_cells, bw_lds_bytes, bw_splits;
} KanBandRoute;
int kan_band_route(const KanGeom* geom, const KanBasis* basis, KanBandRoute* route);

/* Pack the reference-layout weights of one group into the GEMM layouts of the kernels:
 *   wp (forward):   wp[k(item,p)][o],  item = tap*C + c (tap-major), T = kh*kw,
 *                   k = (item / IPC)*KC + (item % IPC)*P + p;  plane p = 0 is the base branch
 *                   (if any), planes hb.. are basis k = p - hb;  plan.packed_weight_bytes.
 *                   (3x3 / stride 1 / pad 1 layers of the default B-spline, ChebyKAN degree-3 and one-input recurrence
 *                   degree-3 specs on 32x32, 16x16, 8x8, 4x4 planes use the pair order of the halo forward kernel instead:
 *                   k = ((c/2)*T + tap)*2P + 2p + (c&1).  Poly specs with order = 0 -- basis on a second tensor xn != x,
 *                   LegendreKAN -- never do.  Layers served by the band kernels -- plan.fwd_band -- use
 *                   k = ((phase, channel group, tap of the phase) step) * KC + (c % IPC) * P + p with KC = even(IPC * P).
 *                   wp is opaque to the caller either way: it is only ever passed back to kan_conv_fwd of the same geometry and basis.)
 *   wd (bwd-data):  optional (NULL to skip), plan.bwd_data_weight_bytes (for depthwise groups -- C = 1, O <= 2, <= 9 taps,
 *                   which run on direct kernels -- it is a plain copy of wp):
 *                   wd[tap*Opad32 + o][ct*128 + cl*P + p],  c = ct*(128/P) + cl.
 * Replaces nothing in the reference (layout only); sources are  base_conv[g].weight [O,C,kh,kw]  (kan_layers.py:159-166) and
 * spline_conv[g].weight / poly_conv[g].weight [O,C*n_basis,kh,kw], channel c*n_basis+k
 * (kan_layers.py:170-177,237; fast_kan_layers.py:68-75,107; cheby_kan_layers.py:77-84,95).
 * `w_base` may be NULL iff basis->act == KAN_ACT_NONE.  With geom->groups = G the sources are the per-group weights
 * stacked on a leading axis, [G,O,C,kh,kw] and [G,O,C*n_basis,kh,kw]. */
int kan_pack_weights(const float* w_base, const float* w_basis, float* wp, float* wd,
                     const KanGeom* geom, const KanBasis* basis, void* stream);

/* kan_pack_weights for the MLP KAN heads whose one parameter is stored input-major: coeffs[C][O][n_basis] -- the `cheby_coeffs` /
 * `bessel_coeffs` / `fib_coeffs` / `gegenbauer_coeffs` / `hermite_coeffs` / `laguerre_coeffs` / `lucas_coeffs` parameter that the layer's
 * einsum('bid,iod->bo', basis, coeffs) contracts (cheby_kan_layers.py:16,34-36; bessel_kan_layers.py:19,35; fibonacci_kan_layers.py:16,37;
 * gegenbauer_kan_layers.py:16,32; hermite_kan_layers.py:15,27; laguerre_kan_layers.py:15,35; lucas_kan_layers.py:16,37).  That contraction is
 * the conv stage on [B, C, 1, 1] with a 1x1 kernel, and this call fills wp and wd (NULL to skip) with exactly what kan_pack_weights writes
 * for the tensor permuted to [O][C*n_basis][1][1] -- padding included, so the conv launchers cannot tell which packer ran -- without that
 * permuted copy ever existing.  Scope: kh = kw = 1, one group, act == KAN_ACT_NONE, any basis the planner accepts; anything else fails
 * before a launch.  Replaces nothing in the reference (layout only). */
int kan_pack_weights_iod(const float* coeffs, float* wp, float* wd, const KanGeom* geom, const KanBasis* basis, void* stream);

/* The same with the packed layouts kept by the caller between calls (single-group geometries for which kan_pack_cacheable
 * returns 1; 16-byte aligned weight tensors).  Every call fingerprints the reference-layout weights on the device -- the two 32-bit sums
 * sum_i bits_i * (2 i + 1) and sum_i rotl(bits_i, i mod 32), over all elements or over every sample_stride-th group of
 * four when sample_stride > 1 -- into slot `cur` of `ring`, and the pack kernels return
 * at once when slot cur equals slot (cur + 2) % 3, i.e. when the weights are bit-for-bit what they were at the previous call: no
 * host round trip, and writes that bypass the framework's version counters are still seen.  `ring` is KAN_FP_WORDS device words (three slots), zero
 * before the first call; the caller passes cur = 0, 1, 2, 0, ... on successive calls (the call also clears slot cur + 1).
 * force != 0 packs unconditionally (first call, new buffers, a weight change the host already knows of).  wd may be NULL (no
 * bwd-data layout wanted): a later call that wants it must pass force. */
int kan_pack_cacheable(const KanGeom* geom, const KanBasis* basis);
int kan_pack_weights_cached(const float* w_base, const float* w_basis, float* wp, float* wd,
                            const KanGeom* geom, const KanBasis* basis, unsigned long long* ring, int cur, int force,
                            int sample_stride, void* stream);

/* Fused forward:  z = act(x) (*) W_base + sum_k basis_k(xn) (*) W_basis[:, c*n+k]
 * with zero padding applied to the EXPANDED operand.  Replaces
 *   kan_layers.py:199-200, 203-239   (B-spline: activation, knot broadcast, indicator,
 *                                     Cox-de Boor, moveaxis/flatten, two convs, add)
 *   fast_kan_layers.py:103, 106-109  (RBF; xn = normalised input, x = raw input)
 *   cheby_kan_layers.py:93-97        (Chebyshev; no base branch)
 * `xn` is the tensor the basis is evaluated on (== x except for FastKAN / LegendreKAN, and for a host-applied base
 * activation: x = act(input), xn = input, act = KAN_ACT_IDENTITY).  The compile-time specs of the single-input kinds
 * (default B-spline with SiLU/GELU, ChebyKAN, ReLU-KAN, GRAM) reject xn != x.
 * z holds plan.fwd_splits slabs of plan.fwd_slab_elems elements; their sum is the result
 * (kan_instnorm_prelu_fwd / kan_slab_reduce consume slabs directly). */
int kan_conv_fwd(const float* x, const float* xn, const float* wp, float* z,
                 const KanGeom* geom, const KanBasis* basis, const float* x_pm, void* stream);

/* dst[(c*HW + i)*B + b] = src[b*bstride + c*HW + i]  (B images, Cn channels of HW pixels; Cn = G*C or G*O of a grouped
 * call): the position-major copy the conv kernels read on small padded planes, where whole taps are structurally zero for a given output position
 * (the reference multiplies those zeros: kan_layers.py:239 zero-pads the expanded tensor). */
int kan_position_major(const float* src, float* dst, int B, int Cn, int HW, long long bstride, void* stream);

/* Gradient w.r.t. the input (autograd of the sites listed at kan_conv_fwd):
 *   dx  = act'(x) * dgrad(dz, W_base)              (base branch)
 *   dxn = sum_k basis_k'(xn) * dgrad(dz, W_basis)_k
 * If dxn == NULL the two are summed into dx (valid when xn == x).  Both are written as
 * plan.bwd_data_splits slabs of plan.bwd_data_slab_elems elements. */
int kan_conv_bwd_data(const float* dz, const float* x, const float* xn, const float* wd,
                      float* dx, float* dxn,
                      const KanGeom* geom, const KanBasis* basis, const float* dz_pm, void* stream);

/* kan_conv_bwd_data that also accumulates the gradient of the basis' trainable device-memory parameters from the same launch.  ReLU-KAN
 * (relu_kan_layers.py:127-131): dparams[C][2][n_basis] (d phase_low, d phase_high per channel of a group; groups share the table and add up).
 * GRAM-KAN (gram_kan_layers.py:156-182): dparams[64][n_basis], 64 slot rows of partial sums of d c_k (entries k < 2 stay 0) that the caller
 * adds up.  The caller zeroes dparams beforehand; every split adds its share with float atomics (scalars; dx stays atomic-free).  Replaces
 * the runs of the weight-gradient kernel on the parameter-derivative planes (two for ReLU-KAN, n_basis - 2 for GRAM). */
int kan_conv_bwd_data_params(const float* dz, const float* x, const float* xn, const float* wd, float* dx, float* dxn, float* dparams,
                             const KanGeom* geom, const KanBasis* basis, const float* dz_pm, void* stream);

/* Gradient w.r.t. the weights in the FLAT packed layout dwp[(tap*C+c)*P + p][o]
 * = sum_pixels expanded[k][pixel] * dz[o][pixel], written as plan.bwd_weight_splits slabs of plan.bwd_weight_slab_elems elements. */
int kan_conv_bwd_weight(const float* dz, const float* x, const float* xn, float* dwp,
                        const KanGeom* geom, const KanBasis* basis, const float* x_pm, const float* dz_pm, void* stream);

/* Small padded planes (plan.e_pm_wanted): the expanded operand in position-major order,
 *   e_pm[((c*HW + pos)*P + p)*B + b] = plane_p(x[b][c][pos])        (c over all G*C channels; plan.e_pm_elems floats),
 * materialised once per layer call -- on 4x4 / 2x2 planes it is 19 - 75 MB next to 85 MB of weights -- and the weight gradient on it:
 * a DMA + MFMA kernel (both operands by LDS-DMA, the (position, tap) pairs that read padding skipped), same dwp layout and slab
 * count as kan_conv_bwd_weight.  dz_pm = kan_position_major(dz).  Replaces the same reference lines as kan_conv_bwd_weight. */
int kan_position_major_expanded(const float* x, float* e_pm, const KanGeom* geom, const KanBasis* basis, void* stream);
int kan_conv_fwd_expanded(const float* e_pm, const float* wp, float* z, const KanGeom* geom, const KanBasis* basis, void* stream);   /* plan.fwd_expanded; z slabs as kan_conv_fwd */
/* The same launch with the tile order forced, for A/B tests and profiling tools: order = 0 (one output position per tile) or KAN_ORDER_FWD_WEIGHT_SIDE
 * (only where kan_tile_orders reports it; z 16-byte aligned).  Both orders write the same bits. */
int kan_conv_fwd_expanded_order(const float* e_pm, const float* wp, float* z, const KanGeom* geom, const KanBasis* basis, void* stream, int order);
int kan_conv_bwd_weight_expanded(const float* dz_pm, const float* e_pm, float* dwp,
                                 const KanGeom* geom, const KanBasis* basis, void* stream);

/* The weight gradient on 8x8 planes with exact tap skipping, where kan_tile_orders reports KAN_ORDER_POS8_BWD_WEIGHT (an error elsewhere): computes what
 * kan_conv_bwd_weight computes from the image-major x and dz (one input tensor), in another order of summation -- row groups of 32 (channel, plane) pairs
 * under all nine taps, bands of two images, a k-pair = one plane position of both images.  dwp receives kan_bwd_weight_rowgroup_slabs() partial slabs of
 * groups * plan.K * plan.Opad floats each (rows (c * taps + tap) * P + p: not the plan's slab count, and not its layout where the plan's route is the
 * band kernel); kan_unpack_wgrad_rowgroups sums and scatters them as kan_unpack_wgrad does for the plan's route.  kan_bwd_weight_rowgroup_slabs is 0 where the
 * entry is not offered. */
int kan_bwd_weight_rowgroup_slabs(const KanGeom* geom, const KanBasis* basis);
int kan_conv_bwd_weight_rowgroups(const float* dz, const float* x, float* dwp, const KanGeom* geom, const KanBasis* basis, void* stream);
int kan_unpack_wgrad_rowgroups(const float* dwp, float* dw_base, float* dw_basis, const KanGeom* geom, const KanBasis* basis, void* stream);

/* Sum the dwp slabs and scatter back to the reference layouts (inverse of kan_pack_weights; stacked [G,...] when
 * geom->groups = G).  dw_base may be NULL iff there is no base branch.  dwp is scratch: with >= 32 slabs the sum is
 * first folded into slab 0 in place. */
int kan_unpack_wgrad(const float* dwp, float* dw_base, float* dw_basis,
                     const KanGeom* geom, const KanBasis* basis, void* stream);

/* kan_unpack_wgrad for the same heads: dcoeffs[C][O][n_basis], the gradient of the `..._coeffs` parameter through the einsum lines listed at
 * kan_pack_weights_iod (autograd of cheby_kan_layers.py:34-36 and its six siblings), bit for bit the permuted result of kan_unpack_wgrad:
 * the plan.bwd_weight_splits slabs are added in the same order (dwp is scratch in the same way).  Same scope as kan_pack_weights_iod. */
int kan_unpack_wgrad_iod(const float* dwp, float* dcoeffs, const KanGeom* geom, const KanBasis* basis, void* stream);

/* out = sum_s slabs[s]  over an NCHW block (B, Cn channels, HW pixels, batch stride bstride). */
int kan_slab_reduce(const float* slabs, int n_slabs, long long slab_elems, float* out,
                    int B, int Cn, int HW, long long bstride, void* stream);

/* InstanceNorm2d (eps, biased variance, per (b,channel) plane, optional affine gamma/beta)
 * followed by an optional scalar-slope PReLU; replaces kan_layers.py:241-243
 * (layer_norm -> prelus), cheby_kan_layers.py:98 and fast_kan_layers.py:106 (norm only:
 * pass prelu_a = NULL).  `z` holds n_slabs partial slabs (their sum is normalised); the
 * summed pre-norm value is written to z_out (may alias slab 0), which the backward needs.
 * mean / rstd: [B*Cn] outputs saved for the backward.
 * prelu_span: 0 = one slope prelu_a[0] for every channel (nn.PReLU()); k > 0 = channel c uses prelu_a[c / k] -- the
 * per-group slopes prelus[g] of a grouped layer (kan_layers.py:182,243) concatenated, k = channels per group. */
int kan_instnorm_prelu_fwd(const float* z, int n_slabs, long long slab_elems, float* z_out,
                           const float* gamma, const float* beta, const float* prelu_a,
                           float* y, float* mean, float* rstd,
                           int B, int Cn, int HW, long long bstride, float eps, int prelu_span, void* stream);

/* Backward of the above.  dz <- gradient w.r.t. the summed pre-norm value.
 * dgamma/dbeta ([Cn]) and dprelu ([1], or [Cn / prelu_span]) are ACCUMULATED with atomics: zero them first.
 * Any of gamma/prelu_a/dgamma/dbeta/dprelu may be NULL when that feature is off. */
int kan_instnorm_prelu_bwd(const float* dy, const float* z, const float* mean, const float* rstd,
                           const float* gamma, const float* beta, const float* prelu_a,
                           float* dz, float* dgamma, float* dbeta, float* dprelu,
                           int B, int Cn, int HW, long long bstride, int prelu_span, void* stream);

/* The same pair with MaxPool2d(kernel 2, stride 2) fused behind the PReLU -- the VGG pattern (models/kan_vgg.py:97-101: a
 * "M" entry right after the layer).  y_pooled / dy_pooled are dense [B][Cn][H/2][W/2]; pool_idx (same shape, bytes) holds the
 * position 2*dh + dw of each window's maximum (first maximum in scan order, NaN wins: torch's max_pool2d rule) and carries
 * the routing to the backward.  The full-size activation and its gradient never touch HBM.  H and W must be even. */
int kan_instnorm_prelu_pool_fwd(const float* z, int n_slabs, long long slab_elems, float* z_out,
                                const float* gamma, const float* beta, const float* prelu_a,
                                float* y_pooled, unsigned char* pool_idx, float* mean, float* rstd,
                                int B, int Cn, int H, int W, long long bstride, float eps, int prelu_span, void* stream);
int kan_instnorm_prelu_pool_bwd(const float* dy_pooled, const unsigned char* pool_idx, const float* z, const float* mean, const float* rstd,
                                const float* gamma, const float* beta, const float* prelu_a,
                                float* dz, float* dgamma, float* dbeta, float* dprelu,
                                int B, int Cn, int H, int W, long long bstride, int prelu_span, void* stream);

/* The same with a general MaxPool2d(pool_k, pool_s) (no padding, floor mode; 2 <= pool_k <= 15, 1 <= pool_s <= pool_k) -- the AlexNet pattern
 * MaxPool2d(kernel_size=3, stride=2) right after a layer (models/kan_alexnet.py:120-126 `features`).  y_pooled / dy_pooled / pool_idx are dense
 * [B][Cn][Hp][Wp], Hp = (H - pool_k) / pool_s + 1; pool_idx = dh * pool_k + dw of the window's maximum (torch's rule, as above).  Windows overlap:
 * the backward of an element sums the pooled gradients of every window that picked it, as torch's max_pool2d backward does. */
int kan_instnorm_prelu_poolk_fwd(const float* z, int n_slabs, long long slab_elems, float* z_out,
                                 const float* gamma, const float* beta, const float* prelu_a,
                                 float* y_pooled, unsigned char* pool_idx, float* mean, float* rstd,
                                 int B, int Cn, int H, int W, long long bstride, float eps, int prelu_span, int pool_k, int pool_s, void* stream);
int kan_instnorm_prelu_poolk_bwd(const float* dy_pooled, const unsigned char* pool_idx, const float* z, const float* mean, const float* rstd,
                                 const float* gamma, const float* beta, const float* prelu_a,
                                 float* dz, float* dgamma, float* dbeta, float* dprelu,
                                 int B, int Cn, int H, int W, long long bstride, int prelu_span, int pool_k, int pool_s, void* stream);

/* Which kernel variant the six kan_instnorm_prelu* entry points launch for a tensor, and with what launch shape.  Pure host arithmetic, no
 * device work (like kan_plan); the entry points dispatch from this struct and from nothing else.
 *   kernel  KAN_NORM_GENERIC: k_in_prelu_fwd / _bwd <G>, 256 threads;  KAN_NORM_REGS: k_in_prelu_fwd_regs / _bwd_regs <G, EPL, PPI, pool, NT>
 *   G       lanes per (b, channel) plane;  EPL, PPI: elements per lane, plane groups per loop iteration (register kernels; 0 otherwise)
 *   pool    KAN_NORM_POOL_NONE / _2X2 (even planes, windows never overlap) / _K (general MaxPool2d(pool_k, pool_s))
 *   lds     general pool: the plane (forward) / its un-pooled gradient (backward) is staged in LDS
 *   held    generic backward: the plane stays in registers between the two passes (otherwise it is read again)
 *   blocks  workgroups launched;  strided: the grid is capped and some workgroup runs its grid-stride loop more than once */
enum { KAN_NORM_GENERIC = 0, KAN_NORM_REGS = 1 };
enum { KAN_NORM_POOL_NONE = 0, KAN_NORM_POOL_2X2 = 1, KAN_NORM_POOL_K = 2 };
typedef struct KanNormRoute {
    int kernel, G, EPL, PPI, NT, pool, lds, held, blocks, strided;
} KanNormRoute;

/* Fill `route` for the forward (backward = 0) or backward launch over B x Cn planes of H x W pixels.  pool2x2 != 0: the fused MaxPool2d(2, 2)
 * entry points (H, W even); pool_k != 0: the general ones (pool2x2 must be 0; same limits as kan_instnorm_prelu_poolk_fwd); both 0: no pool.
 * aligned8: z and z_out are 8-byte aligned (what the forward tests on its pointers before it takes the float2 kernels; ignored otherwise). */
int kan_norm_route(int backward, int B, int Cn, int H, int W, long long bstride, int n_slabs, long long slab_elems,
                   int pool2x2, int pool_k, int pool_s, int aligned8, KanNormRoute* route);

/* BatchNorm2d with per-rank batch statistics [+ scalar-slope PReLU] [+ MaxPool2d(2, 2)] behind the conv stage: replaces kan_layers.py:241-243
 * (layer_norm -> prelus) of a layer built with norm_layer=BatchNorm2d, which train.py:67-68 makes the default of the reference's training
 * script (--norm_layer / --kan_norm_layer), and cheby_kan_layers.py:98 / fast_kan_layers.py:106 (norm only: prelu_a = NULL).
 * Three launches per direction (per-plane partials, a per-channel finalise, the apply pass) around `workspace`, a caller-owned device
 * buffer of kan_batchnorm_workspace_bytes bytes that the backward may share with the forward once the forward has run.  No allocation, no
 * synchronisation; every sum has a fixed order and no value goes through an atomic, so reruns are bit-identical, parameter gradients too.
 *   z, n_slabs, slab_elems, z_out, gamma, beta, prelu_a, prelu_span, bstride: as in kan_instnorm_prelu_fwd.
 *   mean / rstd: [Cn] outputs saved for the backward (rstd = 1 / sqrt(biased variance + eps)).
 *   pool_idx: NULL = y is [B][Cn][H][W]; else (H, W even) y and pool_idx are the dense pooled [B][Cn][H/2][W/2] tensors, pool_idx the
 *             position 2*dh + dw of each window's maximum, as in kan_instnorm_prelu_pool_fwd; the full-size activation is never written.
 *   running_mean / running_var: [Cn], both or neither (NULL: track_running_stats=False).
 *   training != 0: batch statistics; the running buffers, when given, move by `momentum` (the variance by its unbiased estimate N / (N - 1),
 *             as ATen does), which needs more than one value per channel.
 *   training == 0: mean = running_mean, rstd = 1 / sqrt(running_var + eps), nothing is updated; without running buffers batch statistics. */
long long kan_batchnorm_workspace_bytes(int B, int Cn);
int kan_batchnorm_prelu_fwd(const float* z, int n_slabs, long long slab_elems, float* z_out,
                            const float* gamma, const float* beta, const float* prelu_a,
                            float* y, unsigned char* pool_idx, float* mean, float* rstd,
                            float* running_mean, float* running_var, void* workspace,
                            int B, int Cn, int H, int W, long long bstride, float eps, double momentum,
                            int prelu_span, int training, void* stream);

/* Backward of the above (the same reference lines: kan_layers.py:241-243 with norm_layer=BatchNorm2d, train.py:67-68).  dy is the gradient of
 * y: pooled and routed through pool_idx when that is given.  dz <- gradient of the summed pre-norm value; dgamma / dbeta ([Cn]) and dprelu
 * ([1], or [Cn / prelu_span]) are WRITTEN, not accumulated.  training != 0: mean / rstd were the batch's (also what an eval-mode forward
 * without running buffers used); 0: they were the running statistics, dz = (gradient of the normalised value) * rstd.
 * Any of pool_idx, gamma, beta, prelu_a, dgamma, dbeta, dprelu may be NULL when that feature is off. */
int kan_batchnorm_prelu_bwd(const float* dy, const unsigned char* pool_idx, const float* z, const float* mean, const float* rstd,
                            const float* gamma, const float* beta, const float* prelu_a,
                            float* dz, float* dgamma, float* dbeta, float* dprelu, void* workspace,
                            int B, int Cn, int H, int W, long long bstride, int prelu_span, int training, void* stream);

/* OPT-IN split-precision forward: NOT reached from kan_conv_fwd, never the default.  Every fp32 operand is cut into three bf16
 * pieces (hi + mid + lo = 24 mantissa bits) and six bf16 MFMA products per 16-deep block are accumulated in fp32: the fp32 result to ~4e-6 of its
 * largest element at K = 20 736 (one fp32 accumulation chain; the exact path sits at ~1e-6), at ~1.7x the speed of the exact fp32 MFMA kernel.
 * Scope: the default B-spline spec (n_basis 8, order 3, SiLU) on 8x8 or 16x16 planes, 3x3 / stride 1 / pad 1, one group, C % 8 == 0, O % 128 == 0, even B on 8x8
 * planes, dense NCHW -- KAN-VGG11's 64 -> 128 @ 16x16, 128 -> 256 and 256 -> 256 @ 8x8 layers.  Computes what kan_conv_fwd computes for such a layer (kan_layers.py:199-200, 203-239) into ONE slab.
 *   kan_split_supported      1 if (geom, basis) is in scope
 *   kan_split_weight_bytes   size of the cut-weight buffer `wc` (0 if out of scope)
 *   kan_split_pack_weights   reference-layout weights (as kan_pack_weights takes them) -> wc; once per weight update
 *   kan_conv_fwd_split       z[B][O][H][W] = the conv stage */
int kan_split_supported(const KanGeom* geom, const KanBasis* basis);
long long kan_split_weight_bytes(const KanGeom* geom, const KanBasis* basis);
int kan_split_pack_weights(const float* w_base, const float* w_basis, void* wc, const KanGeom* geom, const KanBasis* basis, void* stream);
int kan_conv_fwd_split(const float* x, const void* wc, float* z, const KanGeom* geom, const KanBasis* basis, void* stream);

/* OPT-IN split-precision input gradient: NOT reached from kan_conv_bwd_data, never the default.  The arithmetic and the scope of the
 * split forward above (kan_split_supported serves both directions): dz and the weights are cut into three bf16 pieces, six bf16 MFMA products per 16-deep
 * block, fp32 accumulation; the derivative planes of the epilogue are the exact kernel's.  Computes what kan_conv_bwd_data computes for such a layer -- the
 * autograd of kan_layers.py:199-200, 203-239 w.r.t. the layer input -- into ONE slab dx[B][C][H][W], every element written exactly once (no atomics, no
 * slab reduce).
 *   kan_split_bwd_data_weight_bytes   size of the cut-weight buffer `wcd` (0 if out of scope):
 *                                     wcd[ceil(C / 14) row tiles][(O / 16) * 9 steps][3 pieces][2 k-halves][128 rows][8 bf16 of consecutive o]
 *   kan_split_pack_weights_bwd_data   reference-layout weights (as kan_split_pack_weights takes them: kan_layers.py:159-166, 170-177) -> wcd; once per weight update
 *   kan_conv_bwd_data_split           dx = sum_p plane_p'(x) * dgrad(dz, W_p)
 * Out-of-scope geometry and null pointers are refused by host arithmetic before any launch. */
long long kan_split_bwd_data_weight_bytes(const KanGeom* geom, const KanBasis* basis);
int kan_split_pack_weights_bwd_data(const float* w_base, const float* w_basis, void* wcd, const KanGeom* geom, const KanBasis* basis, void* stream);
int kan_conv_bwd_data_split(const float* dz, const float* x, const void* wcd, float* dx, const KanGeom* geom, const KanBasis* basis, void* stream);

/* OPT-IN split-precision weight gradient: NOT reached from kan_conv_bwd_weight, never the default.  The arithmetic and the scope of
 * the two split launches above (kan_split_supported serves all three): the expanded plane values (the exact kernels' own) and dz are cut into three bf16
 * pieces, six bf16 MFMA products per 16-deep block, fp32 accumulation.  Computes what kan_conv_bwd_weight + kan_unpack_wgrad compute for such a layer -- the
 * autograd of kan_layers.py:199-200, 203-239 w.r.t. the base_conv / spline_conv weights -- straight into the reference layouts dw_base[O][C][3][3] and
 * dw_basis[O][C * 8][3][3] (channel c * 8 + k), every element written exactly once, nothing else written, no float atomics: two calls give the same bits.
 * Any batch the scope admits, batch tails included (images are the inner depth index, in octets; missing images are zeros).
 *   kan_split_bwd_weight_workspace_bytes   size of `workspace` (0 = out of scope; in scope always > 0): the cut dz, then the depth-split partial sums,
 *                                          dzc [ceil(B / 8) octets][H * W pixels][3 pieces][O][8 bf16 of consecutive images]
 *                                          part[KS][O][C][81 floats: 9 planes x 9 taps],   KS = min(32, ceil(512 / (C * O / 128)), units),
 *                                          units = ceil(B / 8) on 8x8 planes, 4 ceil(B / 8) on 16x16 planes (depth units of 64 pixels x 8 images)
 *   kan_conv_bwd_weight_split              cuts dz, contracts, adds the KS partials in ascending order; `workspace` is scratch (16-byte aligned)
 * Out-of-scope geometry, null pointers and a workspace that is not 16-byte aligned are refused by host arithmetic before any launch. */
long long kan_split_bwd_weight_workspace_bytes(const KanGeom* geom, const KanBasis* basis);
int kan_conv_bwd_weight_split(const float* dz, const float* x, float* dw_base, float* dw_basis, void* workspace,
                              const KanGeom* geom, const KanBasis* basis, void* stream);

/* One AdamW step over a flat fp32 block of n elements, in place (p, m = exp_avg, v = exp_avg_sq; g is read only and
 * multiplied by grad_scale first).  Replaces the per-tensor update loop of torch.optim.AdamW as the reference builds it
 * (generic_train.py:24 `optim.AdamW(model.parameters(), lr, weight_decay)`, stepped once per batch: evaluations.py train()),
 * the same formulas in the same order, amsgrad / maximize off:
 *   p *= 1 - lr*weight_decay;  m = lerp(m, g, 1 - beta1);  v = v*beta2 + (1 - beta2) g^2;
 *   p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * with ATen's two-branch lerp (m + (g - m)(1 - beta1) below a weight of 0.5, g - (g - m) beta1 from 0.5 on).  Not the same roundings: every
 * scalar is formed in double and rounded to fp32 once, the bias correction multiplies by 1 / sqrt(1 - beta2^step), and the compiler may fuse
 * a multiply with the add behind it; tests/test_gpu_adamw_matrix.py bounds the difference against an fp64 reference.
 * `step` counts from 1.  The four blocks must be 16-byte aligned.  HBM-bound: 28 bytes per element. */
int kan_adamw_step(float* p, const float* g, float* m, float* v, long long n, double lr, double beta1, double beta2, double eps,
                   double weight_decay, int step, float grad_scale, void* stream);

/* The same step with the gradients left where autograd (or an all-reduce bucket) wrote them.  p / m / v are flat blocks
 * holding n_seg segments (one per parameter); segment s covers elements [seg_off[s], seg_off[s] + seg_n[s]) and reads its
 * gradient from the device address seg_grad[s] (0 = no gradient this step: the segment is skipped, as torch skips it).
 * Workgroup b updates elements [chunk_start[b], chunk_start[b] + chunk_elems) of segment chunk_seg[b]; the caller builds
 * the chunk table once per layout (seg_off and chunk_start multiples of 4 elements, chunk_elems a multiple of 4).  All
 * tables are DEVICE arrays; only seg_grad changes between steps.  torch counts steps PER PARAMETER (one that had no
 * gradient for a while is bias-corrected with its own count): seg_bias, if not NULL, holds per segment
 * { -lr / (1 - beta1^step_s), 1 / sqrt(1 - beta2^step_s) } and overrides the values derived from `step`. */
int kan_adamw_step_segments(float* p, float* m, float* v, const unsigned long long* seg_grad, const long long* seg_off, const int* seg_n,
                            const int* chunk_seg, const int* chunk_start, const float* seg_bias, int n_chunks, int chunk_elems, double lr,
                            double beta1, double beta2, double eps, double weight_decay, int step, float grad_scale, void* stream);

/* ---- The capturable step: the same update with the scalars that change between steps held in DEVICE memory, so that a launch recorded into
 * a HIP graph computes step k at its k-th replay.  Stands in, like the two entry points above, for generic_train.py:24-25 (`optim.AdamW` +
 * `ExponentialLR`: the scheduler changes lr between epochs, the step count grows every batch) in torch's single-tensor AdamW order (above).
 * The caller owns every buffer; everything runs on `stream`; nothing allocates, synchronises or copies; all of it may be stream-captured.
 *
 * Adds 1 to seg_step[s] (int32, DEVICE) for every segment s in [0, n_seg) whose seg_grad[s] is not 0: a segment without a gradient does not
 * age, as torch's per-parameter `step` (the `state[p]["step"] += 1` of its single-tensor AdamW) does not.  Launch it in front of the dev step
 * below, once per step. */
int kan_adamw_advance(int* seg_step, const unsigned long long* seg_grad, int n_seg, void* stream);

/* The segment step above with lr read from lr_dev[0] (a DEVICE double) and each segment's step count from seg_step[s] (DEVICE int32, already
 * advanced: >= 1 wherever seg_grad[s] != 0).  decay = 1 - lr*weight_decay, -lr / (1 - beta1^step) and 1 / sqrt(1 - beta2^step) are formed on
 * the device per segment, in double with pow(beta, (double)step), each rounded to float once -- the expressions of the host path, so where
 * the floats agree bit for bit (device and host pow can differ in the last bit of a double: rarely one float ulp, never more) the results are
 * those of the segment step above bit for bit.  There is no seg_bias: per-segment step counts are native.  betas, eps, weight_decay and
 * grad_scale are kernel arguments: they are frozen into a recorded launch, and changing one means recording again. */
int kan_adamw_step_segments_dev(float* p, float* m, float* v, const unsigned long long* seg_grad, const long long* seg_off, const int* seg_n,
                                const int* chunk_seg, const int* chunk_start, const double* lr_dev, const int* seg_step, int n_chunks,
                                int chunk_elems, double beta1, double beta2, double eps, double weight_decay, float grad_scale, void* stream);

/* Test-facing: the nine floats the dev step forms for ONE (lr_dev[0], step_dev[0]) pair, by the same device function -- the scalars torch's
 * single-tensor AdamW derives from `lr`, `weight_decay`, the betas and `step` (generic_train.py:24-25) --, written to the DEVICE
 * array out9 in the order decay, 1 - beta1, beta1, beta2, 1 - beta2, grad_scale, 1 / sqrt(1 - beta2^step), eps, -lr / (1 - beta1^step). */
int kan_adamw_dev_args(const double* lr_dev, const int* step_dev, double beta1, double beta2, double eps, double weight_decay, float grad_scale,
                       float* out9, void* stream);

/* Writes values[0 .. n) (HOST memory, read before the call returns; n <= 64) into the DEVICE array table[first .. first + n) with one small
 * launch that carries the values as its argument: the way to fill seg_grad while `stream` is capturing, where a host-to-device copy is not
 * allowed (outside capture the table is re-uploaded with a copy).  Stands in for nothing in the reference: torch's AdamW (generic_train.py:24-25) walks
 * `p.grad` on the host every step; this is what replaces that walk inside a recorded step.  The values become part of the graph node; `values` need
 * not outlive the call. */
int kan_set_u64_table(unsigned long long* table, int first, const unsigned long long* values, int n, void* stream);

/* ---- Global-norm gradient clipping inside the step.  The reference asks for it at evaluations.py:33
 * (`clip_grad_norm_(model.parameters(), max_norm=1.0)  # Prevent exploding gradients`, called there before any gradient exists, so it does
 * nothing) and for per-parameter gradient norms in the commented-out `GRAD NORM` print of evaluations.py:66-71.  torch walks the parameter list on
 * the host, launches a norm per tensor and rescales every gradient in place; here two launches leave the norm and the clip coefficient in DEVICE
 * memory and the segment step multiplies by the coefficient as it reads the gradient -- the gradients themselves are not modified.
 * All four entry points run on `stream`, allocate nothing, read no host memory after they return and may be stream-captured; null pointers,
 * n_chunks <= 0 (n_seg <= 0) and a chunk_elems that is not a positive multiple of 4 are refused before any launch (kan_last_error()).
 *
 * Sum of squares per chunk, over the chunk table of kan_adamw_step_segments (evaluations.py:33, the inner `torch.linalg.vector_norm` per
 * parameter): workgroup b reads elements [chunk_start[b], chunk_start[b] + chunk_elems) of the gradient at seg_grad[chunk_seg[b]] and writes ONE
 * double, partial[b]; exactly 0.0 where the address is 0.  Each square is (double)g * (double)g; every sum is in double in a fixed order (thread,
 * wave, workgroup), without atomics: two launches give the same bits.  Nothing else is written.  One launch per parameter group, each at its own
 * offset into `partial`. */
int kan_grad_sqnorm_chunks(const unsigned long long* seg_grad, const int* seg_n, const int* chunk_seg, const int* chunk_start, int n_chunks,
                           int chunk_elems, double* partial, void* stream);

/* The global norm and the clip coefficient (evaluations.py:33: `total_norm` over ALL parameters, `clip_coef = max_norm / (total_norm + 1e-6)`
 * clamped to 1; evaluations.py:66-71: the norm per parameter).  One workgroup; segment s owns partial[seg_first_chunk[s] .. seg_first_chunk[s + 1])
 * -- the tables span all parameter groups.  Writes seg_sq[s] (double, the squared norm of parameter s) for every s in [0, n_seg), sums them in
 * ascending order, and writes out[0] = (float)sqrt(total) and out[1] = (float)min(1.0, (double)max_norm_dev[0] / (sqrt(total) + 1e-6)), formed in
 * double and rounded once.  Non-finite values propagate as in torch: an inf or NaN gradient gives a non-finite norm and the coefficient that
 * expression gives for it, and a NaN quotient stays NaN (torch.clamp's rule), so the step after it poisons the parameters as torch's would. */
int kan_grad_norm_finish(const double* partial, const int* seg_first_chunk, int n_seg, const float* max_norm_dev, double* seg_sq, float* out,
                         void* stream);

/* kan_adamw_step_segments and kan_adamw_step_segments_dev (generic_train.py:24-25) with grad_scale read from scale_dev[0] (DEVICE float: out + 1
 * of kan_grad_norm_finish) instead of passed by value: the clipped step of evaluations.py:33 without the in-place rescaling pass.  The element
 * update is the same function, and the two plain entry points are the same kernels instantiated without the pointer.  scale_dev is
 * read at run time, so a recorded launch clips by whatever the recorded finish launch in front of it computes at replay. */
int kan_adamw_step_segments_clip(float* p, float* m, float* v, const unsigned long long* seg_grad, const long long* seg_off, const int* seg_n,
                                 const int* chunk_seg, const int* chunk_start, const float* seg_bias, int n_chunks, int chunk_elems, double lr,
                                 double beta1, double beta2, double eps, double weight_decay, int step, const float* scale_dev, void* stream);
int kan_adamw_step_segments_dev_clip(float* p, float* m, float* v, const unsigned long long* seg_grad, const long long* seg_off, const int* seg_n,
                                     const int* chunk_seg, const int* chunk_start, const double* lr_dev, const int* seg_step, int n_chunks,
                                     int chunk_elems, double beta1, double beta2, double eps, double weight_decay, const float* scale_dev,
                                     void* stream);

/* ---- Device-side anomaly mode (OPT-IN; with neither entry point in use the step and the layers launch what they launched before).
 * The reference never trains without a watchdog: train.py:431 calls `torch.autograd.set_detect_anomaly(True)` unconditionally, which names the op
 * that first produced a NaN, and evaluations.py:33 is commented "Prevent exploding gradients".  In a recorded training loop the host looks at
 * nothing per step, so both halves live on the device: a probe that counts, and a guard that lets the optimizer step leave everything alone.
 *
 * The probe (train.py:431): counts the non-finite elements -- NaN, +inf, -inf: exponent bits all ones, decided on the bit pattern -- of the dense
 * fp32 buffer x[0 .. n) and adds the count to record[0]; record is three int64 words in DEVICE memory, [elements, first_tick, last_tick], zeroed by
 * the caller.  tick[0] (DEVICE int64, read at run time: a recorded launch sees the tick of its replay) is written to first_tick by the one launch
 * that finds the record at zero elements and something to add, and to last_tick by every launch that finds something; a launch that finds nothing
 * writes nothing.  Integer atomics only, at most three per workgroup that found something: the record is exact whatever the order.  HBM-bound:
 * 4 bytes read per element, float4 loads where x is 16-byte aligned.  Runs on `stream`, allocates nothing, may be stream-captured.  Null pointers,
 * n < 0, a tick or record that is not 8-byte aligned and an x that is not 4-byte aligned are refused before any launch; n == 0 launches nothing. */
int kan_nonfinite_count(const float* x, long long n, const long long* tick, long long* record, void* stream);

/* The guard of the optimizer step (evaluations.py:33, "Prevent exploding gradients"; torch's counterpart is the found_inf skip of
 * torch.optim.AdamW under a GradScaler): ONE decision per step over all parameter groups, taken on the device, so replay k decides for step k.
 * Launch it behind kan_grad_norm_finish.  seg_sq[0 .. n_seg) are that launch's exact double sums of squares per parameter -- finite fp32 squares
 * cannot overflow a double, so seg_sq[s] is non-finite exactly when gradient s holds a non-finite element; the double's exponent bits are tested.
 * groups[g] = { address of group g's seg_grad table, address of its masked copy, number of segments } (DEVICE, 3 x n_groups 8-byte words): the
 * masked copy receives the addresses on a clean step and zeros on a skipped one, and is what kan_adamw_advance and the dev step are then handed --
 * both skip a segment whose address is 0, so a skipped step touches no parameter, no moment and no step count.
 * counters (int64, DEVICE, zeroed by the caller): [0] guarded steps, [1] skipped steps, [2] / [3] the ordinal (counting guarded steps from 1) of the
 * first / last skipped step, [4] 1 if this step was skipped, else 0.  flags[s] (int64) is set to 1 / 0 for every s by a SKIPPED step -- 1 where
 * gradient s was non-finite -- and left alone by a clean one.  One workgroup; no atomics.  Null pointers, n_seg < 1, n_groups < 1 and pointers that
 * are not 8-byte aligned are refused before any launch. */
int kan_adamw_guard(const double* seg_sq, int n_seg, const unsigned long long* groups, int n_groups, long long* counters, long long* flags,
                    void* stream);

/* ---- Gradient accumulation decided on the device (OPT-IN: FusedAdamW.accumulate_steps = k > 1; with k == 1 neither entry point is launched).
 * The loop these extend is evaluations.py:44-72 -- one `optimizer.zero_grad()` / `loss.backward()` / `optimizer.step()` per batch.  The reference
 * has NO accumulation: its effective batch is its loader's batch.  A window of k micro-steps here computes what k data-parallel ranks compute: the
 * mean of the k shard gradients (the reducer's AVG), then ONE AdamW step.  Both entry points run on `stream`, allocate nothing, read no host memory
 * after they return and may be stream-captured.
 *
 * One micro-step of one parameter group, on the grid and chunk tables of kan_adamw_step_segments (n_chunks workgroups of 256 threads; seg_grad,
 * seg_off, seg_n, chunk_seg, chunk_start as there).  acc is a flat fp32 row with the layout of the optimizer's flat block (segment s at
 * [seg_off[s], seg_off[s] + seg_n[s]); the alignment padding between segments is never read or written).  m, the index of this micro-step within
 * the window of k, is micro_dev[0] (DEVICE int32, read at run time: a recorded launch sees the m of its replay) or, with micro_dev == NULL, the
 * argument m in [0, k):
 *   m == 0          acc = g              a copy: the bits survive (-0.0 stays -0.0) and what the previous window left is never read; a segment whose
 *                                        seg_grad[s] is 0 is zero-filled
 *   0 < m < k - 1   acc = acc + g        one fp32 add per element; a segment whose address is 0 is left alone
 *   m == k - 1      acc = (acc + g) * s  s = (float)(1.0 / k): acc then holds the mean, to be read as an ordinary gradient; a segment whose address is
 *                                        0 in this call becomes acc * s (it may have had a gradient earlier in the window)
 * With k == 1 every call is the first row.  float4 accesses where the gradient address is 16-byte aligned, scalar ones otherwise (bucket views, odd
 * offsets).  seen[s] (int32, DEVICE) is set to 1 for every segment whose address is not 0; nothing clears it here.  HBM-bound: 12 bytes per
 * element, 8 at m == 0.  Null pointers (micro_dev excepted), n_chunks < 1, a chunk_elems that is not a positive multiple of 4, k < 1, an m outside
 * [0, k) when micro_dev is NULL, an acc that is not 16-byte aligned and tables that are not aligned to their element size are refused before any
 * launch. */
int kan_grad_accumulate(float* acc, const unsigned long long* seg_grad, const long long* seg_off, const int* seg_n, const int* chunk_seg,
                        const int* chunk_start, int n_chunks, int chunk_elems, const int* micro_dev /* nullable */, int m, int k, int* seen,
                        void* stream);

/* The gate: ONE launch per optimizer call (evaluations.py:72 `optimizer.step()`, which the reference reaches on every batch), behind the
 * accumulate launches of all groups and in front of any statistics launch.  groups[g] = { address of group g's table of accumulator addresses
 * (acc + seg_off[s], 8-byte words), address of its GATED table, address of its seen flags (int32), number of segments } (DEVICE, 4 x n_groups 8-byte
 * words); micro is the window's counter (DEVICE int32, one per optimizer).
 *   micro[0] + 1 == k   gated[s] = seen[s] ? accumulator address : 0 for every segment of every group; seen is cleared; micro[0] = 0
 *   otherwise           gated[s] = 0 everywhere; micro[0] += 1
 * kan_grad_sqnorm_chunks, kan_adamw_guard (as the source it masks), kan_adamw_advance and the dev step are handed the gated table where they are
 * handed seg_grad otherwise: off the boundary they see no gradient and change nothing -- the norm reads 0, the coefficient 1.  guard_counters: NULL, or
 * the counters of the kan_adamw_guard launch that follows in the same call; that launch counts one guarded step, so off the boundary the gate
 * subtracts one from guard_counters[0] in advance and the guard's ordinals count windows.  One workgroup, ordinary stores, no atomics.  Null groups
 * or micro, n_groups < 1, k < 1, groups or guard_counters not 8-byte aligned and a micro that is not 4-byte aligned are refused before any launch. */
int kan_accum_gate(const unsigned long long* groups, int n_groups, int* micro, int k, long long* guard_counters /* nullable */, void* stream);

/* ---------------------------------------------------------------------------------------------- cross-entropy loss and test metrics
 * The criterion of the training script (generic_train.py:26 `nn.CrossEntropyLoss()`, called at evaluations.py:61 and :131: mean reduction, no
 * class weights, no ignore_index, no label smoothing) and what the evaluation loop collects per batch (evaluations.py:131-136: the batch loss,
 * torch.max's prediction, the correct count; :139-140, :146-151: every target and prediction, for scikit-learn's macro precision / recall / F1)
 * -- without the reference's host reads per batch.  logits: fp32 [B][C] row-major;  target: int64 [B].
 *   forward    loss[0] = mean_b (lse[b] - logits[b][target[b]]),  lse[b] = log sum_c exp(logits[b][c]) (kept for the backward).  The batch mean is
 *              summed in double in an order that depends on B alone, and a row's lse on that row alone: the same inputs give the same bits.
 *   metrics    NULL, or a zero-initialised buffer of 8-byte words that every forward call adds to:
 *                [0] correct  [1] samples  [2] batches  [3] bad_target (rows with a target outside [0, C); sticky)  [4] loss_sum, a DOUBLE: the sum
 *                of the batch-mean losses (evaluations.py:132, :150 average batch means)  [5..7] unused
 *                [8 ..) tp[C], pred[C], true[C]: per class, the rows predicted and labelled c / predicted c / labelled c
 *              The prediction of a row is the LOWEST index among its maxima (torch.max).  Integer counters: exact whatever the order.
 *   bad rows   a target outside [0, C) never indexes anything: the row adds 0 to the loss (the mean still divides by B), counts in no counter
 *              but bad_target, and gets a zero gradient row.  The caller reads bad_target when it reads the counters, not per batch.
 *   backward   dlogits[b][c] = grad_loss[0] * (exp(logits[b][c] - lse[b]) - [c == target[b]]) / B;  grad_loss is a DEVICE scalar.
 *   workspace  scratch of the forward (the row losses and row states), 4-byte aligned.
 * Null pointers (metrics excepted), B < 1 and C < 1 are refused by host arithmetic before any launch; the two size functions return 0 for them. */
long long kan_xent_workspace_bytes(int B);
long long kan_xent_metrics_bytes(int C);
int kan_xent_fwd(const float* logits, const long long* target, int B, int C, float* loss, float* lse, void* metrics /* nullable */,
                 void* workspace, void* stream);
int kan_xent_bwd(const float* logits, const long long* target, const float* lse, const float* grad_loss /* device */, float* dlogits,
                 int B, int C, void* stream);

/* ---------------------------------------------------------------------------------------------- batches from a device-resident uint8 dataset
 * The per-sample transforms of the loader's non-ImageNet branch (utils/dataloader.py:56-90: `RandomCrop(S, padding=p)`, `RandomHorizontalFlip`,
 * `ToTensor`, `Normalize`, or the last two alone) and the batching of its DataLoader (:111-112), for a dataset that lives on the device as uint8:
 * one launch per batch, no host read.  Reading dataset files, Resize / RandomResizedCrop / Grayscale (:26-54) and the random draws themselves
 * (the caller makes the table) are not here.
 *   images   uint8, N images of H x W x C: [N][H][W][C] (channels_last != 0; CIFAR) or [N][C][H][W] (channels_last == 0; SVHN, MNIST with C = 1)
 *   labels   int64 [N], or NULL together with target
 *   table    DEVICE int32 [B][4], one row (index, top, left, flip) per batch row
 *   mean/std HOST float [C], C <= 4 (they travel as kernel arguments)
 *   data     fp32 [B][C][Ho][Wo] contiguous:  data[b][c][y][x] = (float(v) / 255.0f - mean[c]) / std[c]  -- three correctly rounded fp32 operations in
 *            that order, ToTensor's div and Normalize's sub_ and div_ -- with v the byte at (c, top + y, left + (flip ? Wo - 1 - x : x)) of image
 *            `index`, and v = 0 outside [0, H) x [0, W).  top and left are in UNPADDED source coordinates and may be negative: torchvision pads the
 *            uint8 image with 0, crops, flips, then converts, so a padded pixel is (0 - mean[c]) / std[c], not 0.  RandomCrop(32, padding=4) on
 *            32 x 32 is top, left in [-4, 4]; a centre crop is top = (H - Ho) / 2; no crop is 0.
 *   target   int64 [B]:  labels[index]
 *   bad rows an index outside [0, N) is compared against the range before it addresses anything: the row's image is all 0.0f and its target -1,
 *            which the loss kernels leave out and count in bad_target.
 * Every output element has one writer and depends on its own table row alone: the same inputs give the same bits.  Null pointers (labels and
 * target excepted, as a pair), N, B, C, H, W, Ho, Wo < 1, C > 4 and H * W * C above the size helper's value are refused by host arithmetic
 * before any launch. */
long long kan_feed_max_image_bytes(void);
int kan_feed_batch(const unsigned char* images, const long long* labels /* nullable */, const int* table, long long N, int B, int C, int H, int W,
                   int Ho, int Wo, int channels_last, const float* mean /* host */, const float* std /* host */, float* data,
                   long long* target /* nullable with labels */, void* stream);

/* The loader's ImageNet branch (utils/dataloader.py:26-54: Resize + RandomResizedCrop / CenterCrop + RandomHorizontalFlip, or Resize +
 * Grayscale(3); then ToTensor + Normalize) on the same device-resident uint8 dataset, one launch per batch, with PIL's 8-bit BILINEAR
 * resampling reproduced byte for byte.  Per sample, torchvision's order on PIL images: stage 1 resizes the whole H x W source to Rh x Rw; the
 * box (top, left, h, w) of that image is cropped; stage 2 resizes the box to Ho x Wo; flip; one channel may be replicated to three; then the
 * value arithmetic of kan_feed_batch.  A resize is a horizontal pass into a uint8 image, then a vertical pass over it, so four uint8 roundings
 * precede the float conversion.  One pass from n to m samples is integer arithmetic over HOST-computed coefficient rows
 * (data.resample_coeffs: PIL's float64 operations in PIL's order; the kernel does no floating-point coefficient work):
 *       out[xx] = clip((2^21 + sum_{t < count} in[xmin + t] * k[t]) >> 22, 0, 255),   a row = (xmin, count, k[0 .. ksize)) of ksize + 2 int32,
 * k zero past count.
 *   images, labels, mean / std, target, channels_last   as kan_feed_batch; mean / std hold out_channels values
 *   table    DEVICE int32 [B][6], one row (index, top, left, h, w, flip) per batch row; the box is in stage-1 coordinates
 *   k1x, k1y DEVICE stage-1 coefficient rows: [Rw] rows of ksize1x + 2 for W -> Rw, [Rh] rows of ksize1y + 2 for H -> Rh
 *   k2x, k2y DEVICE stage-2 coefficient rows for EVERY source length: [Rw][Wo] rows of ksize2x + 2 (block w - 1 is the pass w -> Wo), and
 *            [Rh][Ho] rows of ksize2y + 2; a block whose own ksize is smaller is zero-padded to the common one
 *   out_channels   C, or 3 with C == 1 (Grayscale(num_output_channels=3) on a one-channel image: a plain copy)
 *   data     fp32 [B][out_channels][Ho][Wo] contiguous
 *   bad rows an index outside [0, N), or a box not inside [0, Rh) x [0, Rw) with h, w >= 1, is compared before it addresses anything: an
 *            all-zero image and target -1.  Coefficient rows are used for values only: every window is clamped into the tile it reads.
 * One writer per output element; the same inputs give the same bits.  Refused by host arithmetic before any launch: null pointers (labels and
 * target excepted, as a pair), a size or ksize below 1, C > 4, out_channels other than the above, H * W * C above kan_feed_max_image_bytes(),
 * a ksize above kan_feed_resize_max_ksize() (9: one pass downscales by at most 4 -- the kernel's tiles are sized for that), Rh, Rw, Ho or Wo
 * above 4096, and a geometry of which one output row does not fit the 160 KB of LDS of a compute unit. */
int kan_feed_resize_max_ksize(void);
int kan_feed_resize_batch(const unsigned char* images, const long long* labels /* nullable */, const int* table, long long N, int B, int C, int H,
                          int W, int Rh, int Rw, int Ho, int Wo, int channels_last, int out_channels, const int* k1x, int ksize1x, const int* k1y,
                          int ksize1y, const int* k2x, int ksize2x, const int* k2y, int ksize2y, const float* mean /* host */,
                          const float* std /* host */, float* data, long long* target /* nullable with labels */, void* stream);

/* ---------------------------------------------------------------------------------------------- Wav-KAN wavelet stage
 * u[b, o, ho, wo] = sum_{c, r, t} w[o, c, r, t] * psi((x[b, c, hi, wi] - trans[o, c]) / scale[o, c]),  zero padding applied to the
 * wavelet values.  Replaces WaveletConvND / WaveletConvNDFast / WaveletConvNDFastPlusOne .forward up to (not including) the 1x1
 * `wavelet_out` conv (wav_kan_layers.py:186-217, 257-276, 318-338): the three versions are this arithmetic over differently shaped
 * weight tensors.  One group per call (pre-offset x / u by the group's first channel; x_bstride / u_bstride = elements between
 * images).  scale, trans: [O][C]; w: [O][C][kh][kw] (the 'fast' layout; 'base' and 'fast_plus_one' reshape to it).  fp32, direct
 * vector-ALU kernels (every (o, c) pair has its own wavelet: nothing to share through a GEMM). */
enum { KAN_WAV_MEXICAN_HAT = 0, KAN_WAV_MORLET = 1, KAN_WAV_DOG = 2, KAN_WAV_MEYER = 3, KAN_WAV_SHANNON = 4 };
typedef struct {
    int B, C, H, W, O, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw;
    int wavelet;                      /* KAN_WAV_* */
    long long x_bstride, u_bstride;
} KanWavGeom;
int kan_wav_fwd(const float* x, const float* scale, const float* trans, const float* w, float* u, const KanWavGeom* geom, void* stream);
/* dx = d loss / d x through the wavelets (autograd of the same lines); du: [B][O][Ho][Wo] with u_bstride */
int kan_wav_bwd_input(const float* du, const float* x, const float* scale, const float* trans, const float* w, float* dx,
                      const KanWavGeom* geom, void* stream);
/* dw [O][C][kh][kw], dscale / dtrans [O][C]; workspace: kan_wav_param_workspace(geom) floats of scratch (partial sums, added in a fixed order) */
long long kan_wav_param_workspace(const KanWavGeom* geom);
int kan_wav_bwd_params(const float* du, const float* x, const float* scale, const float* trans, const float* w, float* dw, float* dscale,
                       float* dtrans, float* workspace, const KanWavGeom* geom, void* stream);

/* Which kernels the four entry points above launch for a geometry, and with what launch shapes.  Pure host arithmetic, no device work (like
 * kan_norm_route); kan_wav_fwd, kan_wav_bwd_input, kan_wav_bwd_params and kan_wav_param_workspace take their decisions from this struct and
 * from nothing else.
 *   forward     block = NIMG images x TH x TW output pixels (<= 256) x 4 outputs; RH x RW: the tile's input region (NIMG RH RW <= 1792 cells
 *               unless a single pixel's region is larger);  tiles_h x tiles_w tiles per image;  fwd_shrunk: TH / TW were halved to get a tile's
 *               region under 1792 cells;  fwd_nimg_cut: the same cap lowered NIMG below min(256 / (TH TW), B);  fwd_lds_bytes: dynamic LDS;
 *               fwd_fits = 0: above 64 KB, kan_wav_fwd refuses;  fwd_blocks: tiles x image groups (x ceil(O / 4) in grid y)
 *   bwd-input   TAPS9: k_wav_bwd_input9 (kh kw <= 9);  STRIDE1 / STRIDED: k_wav_bwd_input<true / false>;  bwd_input_blocks: ceil(B H W / 256)
 *               (x ceil(C / 4) in grid y)
 *   bwd-params  TILED: k_wav_bwd_params_tiled, one launch per pass -- work item = NI images x a band of BH input rows, `bands` bands per
 *               image, `items` items, items_per_chunk of them per workgroup, RU x CU cells of du per output (row pitches XP / UP floats),
 *               lds_bytes of dynamic LDS;  PIXEL (the band does not fit 56 KB): k_wav_bwd_params, all passes inside one launch, px_per_chunk
 *               of the B H W input pixels per workgroup.  passes = ceil(kh kw / 9);  chunks: partial-sum slabs = grid z = what
 *               kan_wav_param_workspace counts.  The fields of the kernel not taken are 0.
 * Block counts that do not fit an int are reported as INT_MAX (the entry points refuse such a launch). */
enum { KAN_WAV_BI_TAPS9 = 0, KAN_WAV_BI_STRIDE1 = 1, KAN_WAV_BI_STRIDED = 2 };
enum { KAN_WAV_PAR_TILED = 0, KAN_WAV_PAR_PIXEL = 1 };
typedef struct KanWavRoute {
    int TH, TW, NIMG, RH, RW, tiles_h, tiles_w, fwd_shrunk, fwd_nimg_cut, fwd_lds_bytes, fwd_fits, fwd_blocks;
    int bwd_input_kernel, bwd_input_blocks;
    int params_kernel, passes, chunks, BH, NI, RU, CU, XP, UP, bands, items, items_per_chunk, lds_bytes, px_per_chunk;
} KanWavRoute;
int kan_wav_route(const KanWavGeom* geom, KanWavRoute* route);

#ifdef __cplusplus
}
#endif
#endif /* KANCONV_H */
