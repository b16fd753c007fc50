// Wav-KAN wavelet stage (wav_kan_layers.py:113-338: WaveletConvND / ...Fast / ...FastPlusOne -- the three versions are the same
// arithmetic over differently shaped weights):
//     u[b, o, ho, wo] = sum_{c, r, t} Wk[o, c, r, t] * psi((x[b, c, hi, wi] - trans[o, c]) / scale[o, c]),   hi = ho*sh - ph + r*dh, ...
// with zero padding applied to the WAVELET values.  Every (output, input) pair has its own wavelet, so there is no expanded operand
// shared between outputs and no GEMM: these are direct vector-ALU kernels (one wavelet evaluation per (o, c, input pixel), kh*kw
// multiply-adds per (o, c, output pixel)).  Included by kanconv.hip (same translation unit: fail(), launch_ok()).
//
// Wavelets (wav_kan_layers.py:145-190), u = (x - trans) / scale:
//   0 mexican_hat  K (u^2 - 1) exp(-u^2/2),  K = 2 / (sqrt(3) pi^(1/4))
//   1 morlet       exp(-u^2/2) cos(5 u)
//   2 dog          -u exp(-u^2/2)
//   3 meyer        sin(pi |u|) aux(|u|),  aux(v) = 1 (v <= 1/2), 0 (v >= 1), cos(pi/2 nu(2v - 1)) between,  nu(t) = t^4 (35 - 84 t + 70 t^2 - 20 t^3)
//   4 shannon      sinc(u / pi) * hamming(C)[c] = sin(u) / u * (0.54 - 0.46 cos(2 pi c / (C - 1)))   (window over the CHANNEL axis: x.size(2))

struct WavDev {
    int B, C, H, W, O, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw;
    long long xbs, ubs;          // elements between consecutive images of x / u
};

template <int WT>
__device__ __forceinline__ void wav_eval(float u, float& psi, float& dpsi) {
    if (WT == KAN_WAV_MEXICAN_HAT) {
        constexpr float K = 0.86732507058407751832f;
        const float u2 = u * u, e = kan_exp2k(u2, -0.72134752044448170368f);
        psi = K * (u2 - 1.0f) * e;
        dpsi = K * u * (3.0f - u2) * e;
    } else if (WT == KAN_WAV_MORLET) {
        const float e = kan_exp2k(u * u, -0.72134752044448170368f);
        float s, c;
        sincosf(5.0f * u, &s, &c);
        psi = e * c;
        dpsi = -e * (u * c + 5.0f * s);
    } else if (WT == KAN_WAV_DOG) {
        const float u2 = u * u, e = kan_exp2k(u2, -0.72134752044448170368f);
        psi = -u * e;
        dpsi = (u2 - 1.0f) * e;
    } else if (WT == KAN_WAV_MEYER) {
        constexpr float PI = 3.14159265358979323846f;
        const float v = fabsf(u), sg = u > 0.f ? 1.f : (u < 0.f ? -1.f : 0.f);       // torch.abs has gradient sign(u) (0 at 0)
        float s, c;
        sincosf(PI * v, &s, &c);
        float aux = 1.f, daux = 0.f;
        if (v >= 1.0f) { aux = 0.f; }
        else if (v > 0.5f) {
            const float t = 2.f * v - 1.f, t2 = t * t, t3 = t2 * t;
            const float nu = t2 * t2 * (35.f - 84.f * t + 70.f * t2 - 20.f * t3);
            const float dnu = t3 * (140.f - 420.f * t + 420.f * t2 - 140.f * t3);          // d nu / dt
            float sn, cn;
            sincosf(0.5f * PI * nu, &sn, &cn);
            aux = cn;
            daux = -sn * (0.5f * PI) * dnu * 2.f;                                           // d aux / dv
        }
        psi = s * aux;
        dpsi = sg * (PI * c * aux + s * daux);
    } else {                                                                                // shannon, without the window
        // (cos u - sin(u)/u) / u cancels catastrophically near 0 (absolute error ~ eps / |u|, in torch's fp32 formula too): series below 0.3
        if (fabsf(u) < 0.3f) {
            const float u2 = u * u;
            psi = 1.f + u2 * (-1.f / 6.f + u2 * (1.f / 120.f + u2 * (-1.f / 5040.f + u2 * (1.f / 362880.f))));
            dpsi = u * (-1.f / 3.f + u2 * (1.f / 30.f + u2 * (-1.f / 840.f + u2 * (1.f / 45360.f))));
        } else {
            float s, c;
            sincosf(u, &s, &c);
            const float r = 1.0f / u;
            psi = s * r;
            dpsi = (c - psi) * r;
        }
    }
}

__device__ __forceinline__ float wav_window(int wt, int c, int C) {       // hamming_window(C, periodic=False)[c]; 1 for the other wavelets
    if (wt != KAN_WAV_SHANNON || C <= 1) return 1.f;
    return 0.54f - 0.46f * cosf(6.28318530717958647692f * (float)c / (float)(C - 1));
}

// ---------------------------------------------------------------- forward
// Block: 256 threads = one tile of NIMG images x TH x TW output pixels, WAV_OB outputs.  Per input channel the threads evaluate the
// wavelets of the tile's input region ONCE into LDS (zero outside the image: the padding is applied to the wavelet values), then every
// pixel thread accumulates its kh*kw taps from there.
constexpr int WAV_OB = 4;
struct WavTile { int TH, TW, NIMG, RH, RW, tiles_h, tiles_w; };

template <int WT>
__global__ __launch_bounds__(256) void k_wav_fwd(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ trans,
                                                  const float* __restrict__ w, float* __restrict__ u, WavDev g, WavTile tl) {
    extern __shared__ float s_psi[];                       // [WAV_OB][NIMG * RH * RW]
    const int tid = threadIdx.x;
    int bx = blockIdx.x;
    const int twi = bx % tl.tiles_w; bx /= tl.tiles_w;
    const int thi = bx % tl.tiles_h; bx /= tl.tiles_h;
    const int b0 = bx * tl.NIMG, o0 = blockIdx.y * WAV_OB;
    const int ho0 = thi * tl.TH, wo0 = twi * tl.TW;
    const int hin0 = ho0 * g.sh - g.ph, win0 = wo0 * g.sw - g.pw;          // input coordinates of region cell (0, 0)
    const int region = tl.RH * tl.RW, cells = tl.NIMG * region, T = g.kh * g.kw, HW = g.H * g.W;
    // the output pixel this thread owns
    const int npx = tl.TH * tl.TW;
    const int img = tid / npx, rem = tid - img * npx, th = rem / tl.TW, tw = rem - th * tl.TW;
    const int b = b0 + img, ho = ho0 + th, wo = wo0 + tw;
    const bool own = tid < tl.NIMG * npx && b < g.B && ho < g.Ho && wo < g.Wo;
    const int cell0 = img * region + (th * g.sh) * tl.RW + tw * g.sw;
    float acc[WAV_OB];
#pragma unroll
    for (int j = 0; j < WAV_OB; ++j) acc[j] = 0.f;
    // the region's cells outside the image are the zero padding of the wavelet values: written once; per channel only the in-image
    // sub-rectangle [h_lo, h_hi) x [w_lo, w_hi) of every image is evaluated.  What a thread needs per channel is staged in LDS so that the
    // channel loop has no integer division and no dependent scalar load: s_cell / s_src = (LDS cell, x offset inside a channel plane) of the
    // in-image cells (they do not depend on the channel), s_w = this channel's taps as [tap][WAV_OB] (one 16-byte broadcast read per tap),
    // s_par = translation and 1 / scale of the WAV_OB outputs.
    float* s_w0 = s_psi + WAV_OB * cells;                  // 2 x [T][WAV_OB]   (double-buffered: channel c + 1 is staged while slower threads still
    float* s_par0 = s_w0 + 2 * WAV_OB * T;                 // 2 x [2][WAV_OB]    read channel c's taps; the two barriers of an iteration order the rest)
    int* s_cell = (int*)(s_par0 + 4 * WAV_OB);             // [n_in]
    long long* s_src = (long long*)(s_cell + ((cells + 1) & ~1));     // [n_in] (8-byte aligned: the float counts before it are even)
    for (int idx = tid; idx < WAV_OB * cells; idx += 256) s_psi[idx] = 0.f;
    const int h_lo = max(0, -hin0), h_hi = min(tl.RH, g.H - hin0), w_lo = max(0, -win0), w_hi = min(tl.RW, g.W - win0);
    const int nh = max(0, h_hi - h_lo), nw = max(0, w_hi - w_lo), n_img = min(tl.NIMG, g.B - b0), n_in = n_img * nh * nw;
    for (int idx = tid; idx < n_in; idx += 256) {
        const int im = idx / (nh * nw), rc = idx - im * (nh * nw), rh = h_lo + rc / nw, rw = w_lo + rc % nw;
        s_cell[idx] = im * region + rh * tl.RW + rw;
        s_src[idx] = (long long)(b0 + im) * g.xbs + (hin0 + rh) * g.W + (win0 + rw);
    }
    __syncthreads();

    for (int c = 0; c < g.C; ++c) {
        const float win = wav_window(WT, c, g.C);
        float* s_w = s_w0 + (c & 1) * (WAV_OB * T);
        float* s_par = s_par0 + (c & 1) * (2 * WAV_OB);
        for (int i = tid; i < WAV_OB * T; i += 256) {
            const int tap = i / WAV_OB, j = i - tap * WAV_OB;
            s_w[i] = w[((size_t)min(o0 + j, g.O - 1) * g.C + c) * T + tap];
        }
        if (tid < 2 * WAV_OB) {
            const int j = tid & (WAV_OB - 1), o = min(o0 + j, g.O - 1);
            s_par[tid] = tid < WAV_OB ? trans[o * g.C + c] : 1.0f / scale[o * g.C + c];
        }
        __syncthreads();                                    // taps and parameters of this channel staged (and the previous channel's reads are done)
        const float* xc = x + (size_t)c * HW;
        for (int idx = tid; idx < n_in; idx += 256) {
            const float xv = xc[s_src[idx]];
            const int cell = s_cell[idx];
#pragma unroll
            for (int j = 0; j < WAV_OB; ++j) {
                float p, dp;
                wav_eval<WT>((xv - s_par[j]) * s_par[WAV_OB + j], p, dp);
                s_psi[j * cells + cell] = p * win;
            }
        }
        __syncthreads();
        if (own) {
            for (int r = 0; r < g.kh; ++r)
                for (int t = 0; t < g.kw; ++t) {
                    const int cell = cell0 + (r * g.dh) * tl.RW + t * g.dw;
                    const float4 wv = *reinterpret_cast<const float4*>(s_w + (r * g.kw + t) * WAV_OB);
                    acc[0] += wv.x * s_psi[cell];
                    acc[1] += wv.y * s_psi[cells + cell];
                    acc[2] += wv.z * s_psi[2 * cells + cell];
                    acc[3] += wv.w * s_psi[3 * cells + cell];
                }
        }
    }
    if (own) {
#pragma unroll
        for (int j = 0; j < WAV_OB; ++j)
            if (o0 + j < g.O) u[(size_t)b * g.ubs + (size_t)(o0 + j) * (g.Ho * g.Wo) + ho * g.Wo + wo] = acc[j];
    }
}

// ---------------------------------------------------------------- backward: input
// dx[b, c, hi, wi] = sum_o psi'(u_oc) / scale[o, c] * G_o,   G_o = sum_{r, t} Wk[o, c, r, t] du[b, o, ho, wo]  over the taps that read this pixel.
// Thread = one input pixel x WAV_CB channels; the du values of a tap are shared by the channels.
constexpr int WAV_CB = 4;
template <int WT, bool S1>                                  // S1: stride 1 in both axes (no divisibility tests, no divisions)
__global__ __launch_bounds__(256) void k_wav_bwd_input(const float* __restrict__ du, const float* __restrict__ x, const float* __restrict__ scale,
                                                        const float* __restrict__ trans, const float* __restrict__ w, float* __restrict__ dx, WavDev g) {
    const int HW = g.H * g.W, HoWo = g.Ho * g.Wo, T = g.kh * g.kw;
    const long long px = (long long)blockIdx.x * 256 + threadIdx.x;
    if (px >= (long long)g.B * HW) return;
    const int b = (int)(px / HW), hw = (int)(px - (long long)b * HW), hi = hw / g.W, wi = hw - hi * g.W;
    const int c0 = blockIdx.y * WAV_CB;
    float xv[WAV_CB], acc[WAV_CB], win[WAV_CB];
#pragma unroll
    for (int j = 0; j < WAV_CB; ++j) {
        const int c = min(c0 + j, g.C - 1);
        xv[j] = x[(size_t)b * g.xbs + (size_t)c * HW + hw];
        win[j] = wav_window(WT, c, g.C);
        acc[j] = 0.f;
    }
    // the (tap -> output pixel) table of this input pixel does not depend on o
    const float* dub = du + (size_t)b * g.ubs;
    for (int o = 0; o < g.O; ++o) {
        float G[WAV_CB];
#pragma unroll
        for (int j = 0; j < WAV_CB; ++j) G[j] = 0.f;
        for (int r = 0; r < g.kh; ++r) {
            const int hn = hi + g.ph - r * g.dh;
            if (hn < 0 || (!S1 && hn % g.sh)) continue;
            const int ho = S1 ? hn : hn / g.sh;
            if (ho >= g.Ho) continue;
            for (int t = 0; t < g.kw; ++t) {
                const int wn = wi + g.pw - t * g.dw;
                if (wn < 0 || (!S1 && wn % g.sw)) continue;
                const int wo = S1 ? wn : wn / g.sw;
                if (wo >= g.Wo) continue;
                const float d = dub[(size_t)o * HoWo + ho * g.Wo + wo];
#pragma unroll
                for (int j = 0; j < WAV_CB; ++j) {
                    const int c = min(c0 + j, g.C - 1);
                    G[j] += w[((size_t)o * g.C + c) * T + r * g.kw + t] * d;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < WAV_CB; ++j) {
            const int c = min(c0 + j, g.C - 1);
            const float is = 1.0f / scale[o * g.C + c];
            float p, dp;
            wav_eval<WT>((xv[j] - trans[o * g.C + c]) * is, p, dp);
            acc[j] += dp * is * win[j] * G[j];
        }
    }
#pragma unroll
    for (int j = 0; j < WAV_CB; ++j)
        if (c0 + j < g.C) dx[(size_t)b * g.xbs + (size_t)(c0 + j) * HW + hw] = acc[j];
}

// The same for kernels of at most 9 taps (3x3, 1x3, ...): the (tap -> output pixel) table of the thread's input pixel sits in registers (it does not
// depend on o: clamped offsets + 0/1 masks, unconditional loads), and the taps / translation / 1/scale of 8 outputs x WAV_CB channels are staged in
// LDS per barrier pair instead of being fetched by dependent scalar loads inside the loop.
template <int WT>
__global__ __launch_bounds__(256) void k_wav_bwd_input9(const float* __restrict__ du, const float* __restrict__ x, const float* __restrict__ scale,
                                                         const float* __restrict__ trans, const float* __restrict__ w, float* __restrict__ dx, WavDev g) {
    constexpr int TK = 9, OBI = 8, REC = TK + 2;                          // per (output, channel) record: 9 taps, translation, 1 / scale
    __shared__ float s_rec[OBI][WAV_CB][REC];
    const int HW = g.H * g.W, HoWo = g.Ho * g.Wo, T = g.kh * g.kw, tid = threadIdx.x;
    const long long pxl = (long long)blockIdx.x * 256 + tid, total = (long long)g.B * HW;
    const long long px = pxl < total ? pxl : total - 1;                     // (threads past the end work on the last pixel and do not store)
    const int b = (int)(px / HW), hw = (int)(px - (long long)b * HW), hi = hw / g.W, wi = hw - hi * g.W;
    const int c0 = blockIdx.y * WAV_CB;
    float xv[WAV_CB], acc[WAV_CB];
#pragma unroll
    for (int j = 0; j < WAV_CB; ++j) {
        xv[j] = x[(size_t)b * g.xbs + (size_t)min(c0 + j, g.C - 1) * HW + hw];
        acc[j] = 0.f;
    }
    int off[TK]; unsigned msk = 0u;                      // bit k: tap k reaches an output element (select, not multiply: 0 * Inf would be NaN)
#pragma unroll
    for (int k = 0; k < TK; ++k) {
        const int tap = min(k, T - 1), r = tap / g.kw, t = tap - r * g.kw;
        const int hn = hi + g.ph - r * g.dh, wn = wi + g.pw - t * g.dw;
        const int ho = hn / g.sh, wo = wn / g.sw;
        const bool ok = k < T && hn >= 0 && wn >= 0 && ho * g.sh == hn && wo * g.sw == wn && ho < g.Ho && wo < g.Wo;
        off[k] = ok ? ho * g.Wo + wo : 0;
        msk |= (ok ? 1u : 0u) << k;
    }
    const float* dub = du + (size_t)b * g.ubs;
    for (int o0 = 0; o0 < g.O; o0 += OBI) {
        __syncthreads();
        for (int i = tid; i < OBI * WAV_CB * REC; i += 256) {
            const int ob = i / (WAV_CB * REC), rem = i - ob * (WAV_CB * REC), j = rem / REC, f = rem - j * REC;
            const int o = min(o0 + ob, g.O - 1), c = min(c0 + j, g.C - 1);
            s_rec[ob][j][f] = f < TK ? (f < T ? w[((size_t)o * g.C + c) * T + f] : 0.f) : f == TK ? trans[o * g.C + c] : 1.0f / scale[o * g.C + c];
        }
        __syncthreads();
        const int nob = min(OBI, g.O - o0);
        for (int ob = 0; ob < nob; ++ob) {
            const float* dpl = dub + (size_t)(o0 + ob) * HoWo;
            float G[WAV_CB];
#pragma unroll
            for (int j = 0; j < WAV_CB; ++j) G[j] = 0.f;
#pragma unroll
            for (int k = 0; k < TK; ++k) {
                const float d = ((msk >> k) & 1u) ? dpl[off[k]] : 0.f;      // unconditional load on the clamped offset, v_cndmask on the value
#pragma unroll
                for (int j = 0; j < WAV_CB; ++j) G[j] += s_rec[ob][j][k] * d;
            }
#pragma unroll
            for (int j = 0; j < WAV_CB; ++j) {
                const float is = s_rec[ob][j][TK + 1];
                float p, dp;
                wav_eval<WT>((xv[j] - s_rec[ob][j][TK]) * is, p, dp);
                acc[j] += dp * is * G[j];
            }
        }
    }
    if (pxl < total) {
#pragma unroll
        for (int j = 0; j < WAV_CB; ++j)
            if (c0 + j < g.C) dx[(size_t)b * g.xbs + (size_t)(c0 + j) * HW + hw] = acc[j] * wav_window(WT, c0 + j, g.C);
    }
}

// ---------------------------------------------------------------- backward: parameters
// Block = one (o, c) pair and one chunk of the B*H*W input pixels.  Per input pixel: psi and psi' once, then for every tap that reads the pixel
//   dW[o, c, r, t] += psi * du(tap),   G += W[r, t] * du(tap);    dtrans -= psi' G / s,   dscale -= psi' G u / s.
// The T + 2 sums are reduced over the block in a fixed order and written to partial slab `chunk` ([chunks][O*C*(T+2)], summed by
// kan_slab_reduce-style addition on the host side): deterministic, no atomics.
template <int WT>
__global__ __launch_bounds__(256) void k_wav_bwd_params(const float* __restrict__ du, const float* __restrict__ x, const float* __restrict__ scale,
                                                         const float* __restrict__ trans, const float* __restrict__ w, float* __restrict__ part,
                                                         WavDev g, int px_per_chunk) {
    constexpr int TMAX = 9;                                                      // taps kept in registers per pass
    __shared__ float s_red[4][TMAX + 2];
    const int c = blockIdx.x, o = blockIdx.y, chunk = blockIdx.z;
    const int HW = g.H * g.W, HoWo = g.Ho * g.Wo, T = g.kh * g.kw;
    const long long total = (long long)g.B * HW;
    const long long p0 = (long long)chunk * px_per_chunk, p1 = min(total, p0 + px_per_chunk);
    const float is = 1.0f / scale[o * g.C + c], tr = trans[o * g.C + c], win = wav_window(WT, c, g.C);
    const float* wk = w + ((size_t)o * g.C + c) * T;
    float* out = part + ((size_t)chunk * g.O * g.C + (size_t)o * g.C + c) * (T + 2);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t0 = 0; t0 < T; t0 += TMAX) {                                       // (kernels above 9 taps take several passes; every pass adds its share of dtrans / dscale)
        const int nt = min(TMAX, T - t0);
        float sw_[TMAX], st = 0.f, ss = 0.f;
#pragma unroll
        for (int k = 0; k < TMAX; ++k) sw_[k] = 0.f;
        for (long long px = p0 + tid; px < p1; px += 256) {
            const int b = (int)(px / HW), hw = (int)(px - (long long)b * HW), hi = hw / g.W, wi = hw - hi * g.W;
            const float xv = x[(size_t)b * g.xbs + (size_t)c * HW + hw];
            const float uu = (xv - tr) * is;
            float p, dp;
            wav_eval<WT>(uu, p, dp);
            p *= win; dp *= win;
            const float* dub = du + (size_t)b * g.ubs + (size_t)o * HoWo;
            float G = 0.f;
#pragma unroll
            for (int k = 0; k < TMAX; ++k) {                                       // (branch-free body: stays fully unrolled, sums in registers)
                const int tap = min(t0 + k, T - 1), r = tap / g.kw, t = tap - r * g.kw;
                const int hn = hi + g.ph - r * g.dh, wn = wi + g.pw - t * g.dw;
                const int ho = hn / g.sh, wo = wn / g.sw;
                const bool ok = k < nt && hn >= 0 && wn >= 0 && ho * g.sh == hn && wo * g.sw == wn && ho < g.Ho && wo < g.Wo;
                const float d = ok ? dub[ho * g.Wo + wo] : 0.f;
                sw_[k] += p * d;
                G += wk[tap] * d;
            }
            st -= dp * is * G;
            ss -= dp * is * uu * G;
        }
        // block reduction in a fixed order: lanes by shuffles, the four waves through LDS
#pragma unroll
        for (int k = 0; k < TMAX + 2; ++k) {
            float v = k < TMAX ? sw_[k < TMAX ? k : 0] : (k == TMAX ? st : ss);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) s_red[wave][k] = v;
        }
        __syncthreads();
        if (tid < TMAX + 2) {
            const float v = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
            if (tid < nt) out[t0 + tid] = v;
            else if (tid == TMAX) out[T] = (t0 == 0 ? v : out[T] + v);               // (G is partial per pass: the passes add up)
            else if (tid == TMAX + 1) out[T + 1] = (t0 == 0 ? v : out[T + 1] + v);
        }
        __syncthreads();
    }
}

// The same sums with one THREAD per (o, c) pair (block = 16 outputs x 16 channels) and no reduction: per work item -- NI images x one band
// of BH input rows -- the block stages the x band of its 16 channels and the du values of its 16 outputs in LDS, the latter scattered onto
// the grid of hn = hi + ph - r*dh (zeros where no output pixel sits: stride holes, borders), so that tap (r, t) of input pixel (hi, wi) is
// the LDS cell at a fixed scalar offset from the pixel's own and needs no bounds or divisibility test.  The pixel loop is uniform over the
// block (scalar index arithmetic); a wave reads 16 distinct x cells and 4 distinct du cells per step (LDS broadcast).  Up to 9 taps per pass.
constexpr int WAV_PO = 16, WAV_PC = 16;
struct WavBand { int BH, NI, RU, CU, XP, UP, bands, items, items_per_chunk; };

template <int WT>
__global__ __launch_bounds__(256) void k_wav_bwd_params_tiled(const float* __restrict__ du, const float* __restrict__ x, const float* __restrict__ scale,
                                                               const float* __restrict__ trans, const float* __restrict__ w, float* __restrict__ part,
                                                               WavDev g, WavBand wb, int t0) {
    constexpr int TMAX = 9;
    extern __shared__ float s_wp[];
    float* sx = s_wp;                                           // [NI][16][XP]
    float* su = s_wp + wb.NI * WAV_PC * wb.XP;                  // [NI][16][UP]
    const int tid = threadIdx.x, c_l = tid & 15, o_l = tid >> 4;
    const int c0 = blockIdx.x * WAV_PC, o0 = blockIdx.y * WAV_PO, chunk = blockIdx.z;
    const int c = min(c0 + c_l, g.C - 1), o = min(o0 + o_l, g.O - 1);
    const bool valid = c0 + c_l < g.C && o0 + o_l < g.O;
    const int HW = g.H * g.W, HoWo = g.Ho * g.Wo, T = g.kh * g.kw, nt = min(TMAX, T - t0);
    const float is = 1.0f / scale[o * g.C + c], tr = trans[o * g.C + c], win = wav_window(WT, c, g.C);
    float wk[TMAX]; int toff[TMAX];
#pragma unroll
    for (int k = 0; k < TMAX; ++k) {
        const int tap = min(t0 + k, T - 1), r = tap / g.kw, t = tap - r * g.kw;
        wk[k] = k < nt ? w[((size_t)o * g.C + c) * T + tap] : 0.f;
        toff[k] = r * g.dh * wb.CU + t * g.dw;                                   // scalar
    }
    float sw_[TMAX], st = 0.f, ss = 0.f;
#pragma unroll
    for (int k = 0; k < TMAX; ++k) sw_[k] = 0.f;
    const int wnmin = g.pw - (g.kw - 1) * g.dw;
    const int item0 = chunk * wb.items_per_chunk, item1 = min(wb.items, item0 + wb.items_per_chunk);
    for (int item = item0; item < item1; ++item) {
        const int ig = item / wb.bands, band = item - ig * wb.bands;
        const int b0 = ig * wb.NI, h0 = band * wb.BH, bh = min(wb.BH, g.H - h0);
        const int hnmin = h0 + g.ph - (g.kh - 1) * g.dh;
        __syncthreads();                                                          // the previous item's reads are done
        const int nx = wb.NI * WAV_PC * wb.BH * g.W;
        for (int idx = tid; idx < nx; idx += 256) {
            const int wc = idx % g.W; int q = idx / g.W;
            const int r = q % wb.BH; q /= wb.BH;
            const int cc = q % WAV_PC, im = q / WAV_PC;
            const int b = b0 + im, ch = c0 + cc, hi = h0 + r;
            const bool ok = b < g.B && ch < g.C && hi < g.H;
            sx[(im * WAV_PC + cc) * wb.XP + r * g.W + wc] = ok ? x[(size_t)b * g.xbs + (size_t)ch * HW + hi * g.W + wc] : 0.f;
        }
        const int nu = wb.NI * WAV_PO * wb.RU * wb.CU;
        for (int idx = tid; idx < nu; idx += 256) {
            const int cu = idx % wb.CU; int q = idx / wb.CU;
            const int ru = q % wb.RU; q /= wb.RU;
            const int oo = q % WAV_PO, im = q / WAV_PO;
            const int b = b0 + im, oc = o0 + oo, hn = hnmin + ru, wn = wnmin + cu;
            const int ho = hn / g.sh, wo = wn / g.sw;
            const bool ok = b < g.B && oc < g.O && hn >= 0 && wn >= 0 && ho * g.sh == hn && wo * g.sw == wn && ho < g.Ho && wo < g.Wo;
            su[(im * WAV_PO + oo) * wb.UP + ru * wb.CU + cu] = ok ? du[(size_t)b * g.ubs + (size_t)oc * HoWo + ho * g.Wo + wo] : 0.f;
        }
        __syncthreads();
        for (int im = 0; im < wb.NI; ++im) {
            const float* px_x = sx + (im * WAV_PC + c_l) * wb.XP;
            const float* px_u = su + (im * WAV_PO + o_l) * wb.UP + (g.kh - 1) * g.dh * wb.CU + (g.kw - 1) * g.dw;
            for (int r = 0; r < bh; ++r)
                for (int wc = 0; wc < g.W; ++wc) {
                    const float xv = px_x[r * g.W + wc];
                    const float uu = (xv - tr) * is;
                    float p, dp;
                    wav_eval<WT>(uu, p, dp);
                    const float* cell = px_u + r * wb.CU + wc;
                    float G = 0.f;
#pragma unroll
                    for (int k = 0; k < TMAX; ++k) {
                        const float d = cell[-toff[k]];
                        sw_[k] += p * d;
                        G += wk[k] * d;
                    }
                    st -= dp * G;
                    ss -= dp * uu * G;
                }
        }
    }
    if (valid) {
        float* out = part + ((size_t)chunk * g.O * g.C + (size_t)o * g.C + c) * (T + 2);
#pragma unroll
        for (int k = 0; k < TMAX; ++k)
            if (k < nt) out[t0 + k] = sw_[k] * win;
        if (t0 == 0) { out[T] = st * is * win; out[T + 1] = ss * is * win; }
        else { out[T] += st * is * win; out[T + 1] += ss * is * win; }
    }
}

__global__ void k_wav_sum_parts(const float* __restrict__ part, int chunks, long long n, int T, float* __restrict__ dw, float* __restrict__ dscale,
                                float* __restrict__ dtrans) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;       // over O*C*(T+2)
    if (i >= n) return;
    float v = 0.f;
    for (int s = 0; s < chunks; ++s) v += part[(size_t)s * n + i];
    const long long oc = i / (T + 2); const int k = (int)(i - oc * (T + 2));
    if (k < T) dw[oc * T + k] = v;
    else if (k == T) dtrans[oc] = v;
    else dscale[oc] = v;
}

static WavDev wav_dev(const KanWavGeom* g) {
    WavDev d;
    d.B = g->B; d.C = g->C; d.H = g->H; d.W = g->W; d.O = g->O; d.Ho = g->Ho; d.Wo = g->Wo; d.kh = g->kh; d.kw = g->kw;
    d.sh = g->sh; d.sw = g->sw; d.ph = g->ph; d.pw = g->pw; d.dh = g->dh; d.dw = g->dw; d.xbs = g->x_bstride; d.ubs = g->u_bstride;
    return d;
}

static int wav_check(const KanWavGeom* g) {
    if (!g) return fail("null wavelet geometry");
    if (g->B < 1 || g->C < 1 || g->O < 1 || g->H < 1 || g->W < 1 || g->kh < 1 || g->kw < 1 || g->sh < 1 || g->sw < 1 || g->dh < 1 || g->dw < 1 ||
        g->ph < 0 || g->pw < 0)
        return fail("bad wavelet geometry");
    if (g->Ho != (g->H + 2 * g->ph - g->dh * (g->kh - 1) - 1) / g->sh + 1 || g->Wo != (g->W + 2 * g->pw - g->dw * (g->kw - 1) - 1) / g->sw + 1 || g->Ho < 1 || g->Wo < 1)
        return fail("wavelet geometry: Ho / Wo do not match the convolution arithmetic");
    if (g->wavelet < 0 || g->wavelet > KAN_WAV_SHANNON) return fail("unknown wavelet type");
    if ((long long)g->O * g->C * (g->kh * g->kw + 2) >= (1ll << 31)) return fail("wavelet weight tensor too large");
    return 0;
}

// Every launch decision of the wavelet stage (kan_wav_route exports it; the four entry points dispatch from it and from nothing else).
//   forward: a tile of up to 256 output pixels (whole small planes of several images, or a TH x TW patch), input region <= 1792 cells (LDS: 4
//   wavelet planes + the cell tables);  bwd-input: the register-table kernel up to 9 taps, else the generic one (stride 1 or not);  bwd-params:
//   the tiled kernel while NI images x a band of BH rows (x and the scattered du, 16 channels / outputs each) fit 56 KB of LDS, else (very wide
//   rows / large dilated kernels) the per-pixel kernel.
constexpr int WAV_TAPS = 9;                       // taps per pass of the parameter kernels; the register table of k_wav_bwd_input9
constexpr long long WAV_REGION_CELLS = 1792;
constexpr size_t WAV_FWD_LDS = 64 * 1024, WAV_BAND_LDS = 56 * 1024;

static int wav_sat(long long v) { return v > 2147483647ll ? 2147483647 : (int)v; }

static void wav_plan(const KanWavGeom* g, KanWavRoute& r, long long& fwd_blocks, long long& bi_blocks, size_t& fwd_smem, size_t& par_smem) {
    r = KanWavRoute{};
    const int T = g->kh * g->kw;
    // ---- forward
    r.TW = g->Wo < 16 ? g->Wo : 16;
    r.TH = g->Ho < 256 / r.TW ? g->Ho : 256 / r.TW;
    auto region = [&](int th, int tw, int& rh, int& rw) { rh = (th - 1) * g->sh + (g->kh - 1) * g->dh + 1; rw = (tw - 1) * g->sw + (g->kw - 1) * g->dw + 1; };
    region(r.TH, r.TW, r.RH, r.RW);
    while ((long long)r.RH * r.RW > WAV_REGION_CELLS && (r.TH > 1 || r.TW > 1)) {
        if (r.TH >= r.TW && r.TH > 1) r.TH = (r.TH + 1) / 2; else r.TW = (r.TW + 1) / 2;
        region(r.TH, r.TW, r.RH, r.RW);
        r.fwd_shrunk = 1;
    }
    r.NIMG = 256 / (r.TH * r.TW);
    if (r.NIMG < 1) r.NIMG = 1;
    const int nimg_free = r.NIMG < g->B ? r.NIMG : g->B;
    while (r.NIMG > 1 && (long long)r.NIMG * r.RH * r.RW > WAV_REGION_CELLS) --r.NIMG;
    if (r.NIMG > g->B) r.NIMG = g->B;
    r.fwd_nimg_cut = r.NIMG < nimg_free;
    r.tiles_h = (g->Ho + r.TH - 1) / r.TH; r.tiles_w = (g->Wo + r.TW - 1) / r.TW;
    fwd_blocks = (long long)((g->B + r.NIMG - 1) / r.NIMG) * r.tiles_h * r.tiles_w;
    const size_t n_cells = (size_t)r.NIMG * r.RH * r.RW;
    fwd_smem = ((size_t)WAV_OB * (n_cells + 2 * T + 4) + ((n_cells + 1) & ~(size_t)1)) * sizeof(float) + n_cells * sizeof(long long);
    r.fwd_fits = fwd_smem <= WAV_FWD_LDS;
    r.fwd_lds_bytes = wav_sat((long long)fwd_smem);
    r.fwd_blocks = wav_sat(fwd_blocks);
    // ---- bwd-input
    r.bwd_input_kernel = T <= WAV_TAPS ? KAN_WAV_BI_TAPS9 : (g->sh == 1 && g->sw == 1 ? KAN_WAV_BI_STRIDE1 : KAN_WAV_BI_STRIDED);
    const long long total = (long long)g->B * g->H * g->W;
    bi_blocks = (total + 255) / 256;
    r.bwd_input_blocks = wav_sat(bi_blocks);
    // ---- bwd-params
    r.passes = (T + WAV_TAPS - 1) / WAV_TAPS;
    const int BH = g->W >= 256 ? 1 : (256 / g->W < g->H ? 256 / g->W : g->H);
    const int RU = BH + (g->kh - 1) * g->dh, CU = g->W + (g->kw - 1) * g->dw;
    const int XP = (BH * g->W) | 1, UP = (RU * CU) | 1;
    int NI = 256 / (BH * g->W); if (NI < 1) NI = 1; if (NI > g->B) NI = g->B;
    auto bytes = [&](int ni) { return (size_t)ni * 16 * ((size_t)XP + UP) * sizeof(float); };
    while (NI > 1 && bytes(NI) > WAV_BAND_LDS) --NI;
    par_smem = bytes(NI);
    long long chunks;
    if (par_smem <= WAV_BAND_LDS) {
        r.params_kernel = KAN_WAV_PAR_TILED;
        r.BH = BH; r.NI = NI; r.RU = RU; r.CU = CU; r.XP = XP; r.UP = UP;
        r.lds_bytes = (int)par_smem;
        r.bands = (g->H + BH - 1) / BH;
        r.items = ((g->B + NI - 1) / NI) * r.bands;
        const long long pairs = (long long)((g->C + 15) / 16) * ((g->O + 15) / 16);
        chunks = (2048 + pairs - 1) / pairs;
        if (chunks > r.items) chunks = r.items;
        if (chunks > 65535) chunks = 65535;
        r.items_per_chunk = (int)((r.items + chunks - 1) / chunks);
        chunks = (r.items + r.items_per_chunk - 1) / r.items_per_chunk;
    } else {
        r.params_kernel = KAN_WAV_PAR_PIXEL;
        par_smem = 0;
        const long long pairs = (long long)g->O * g->C;
        chunks = (4096 + pairs - 1) / pairs;                             // enough blocks to fill the chip, >= 256 pixels each
        if (chunks > (total + 255) / 256) chunks = (total + 255) / 256;
        if (chunks < 1) chunks = 1;
        if (chunks > 65535) chunks = 65535;
        r.px_per_chunk = (int)((total + chunks - 1) / chunks);
    }
    r.chunks = (int)chunks;
}

#define KAN_WAV_DISPATCH(CALL)                                  \
    switch (g->wavelet) {                                        \
        case KAN_WAV_MEXICAN_HAT: CALL(KAN_WAV_MEXICAN_HAT); break; \
        case KAN_WAV_MORLET: CALL(KAN_WAV_MORLET); break;           \
        case KAN_WAV_DOG: CALL(KAN_WAV_DOG); break;                 \
        case KAN_WAV_MEYER: CALL(KAN_WAV_MEYER); break;             \
        default: CALL(KAN_WAV_SHANNON); break;                      \
    }

}  // namespace

extern "C" {

int kan_wav_route(const KanWavGeom* g, KanWavRoute* route) {
    if (int rc = wav_check(g)) return rc;
    if (!route) return fail("null route in kan_wav_route");
    long long fwd_blocks, bi_blocks; size_t fwd_smem, par_smem;
    wav_plan(g, *route, fwd_blocks, bi_blocks, fwd_smem, par_smem);
    return 0;
}

int kan_wav_fwd(const float* x, const float* scale, const float* trans, const float* w, float* u, const KanWavGeom* g, void* stream) {
    if (int rc = wav_check(g)) return rc;
    if (!x || !scale || !trans || !w || !u) return fail("null pointer in kan_wav_fwd");
    KanWavRoute r; long long blocks, bi_blocks; size_t smem, par_smem;
    wav_plan(g, r, blocks, bi_blocks, smem, par_smem);
    const WavTile tl = {r.TH, r.TW, r.NIMG, r.RH, r.RW, r.tiles_h, r.tiles_w};
    const WavDev d = wav_dev(g);
    const int oblocks = (g->O + WAV_OB - 1) / WAV_OB;
    if (blocks >= (1ll << 31) || oblocks > 65535) return fail("wavelet forward grid too large");
    static_assert(WAV_OB == 4, "k_wav_fwd reads its taps as float4");
    if (!r.fwd_fits) return fail("wavelet forward tile does not fit in LDS (kernel / stride / dilation too large)");
#define KAN_WAV_F(WT) hipLaunchKernelGGL((k_wav_fwd<WT>), dim3((unsigned)blocks, oblocks), dim3(256), smem, (hipStream_t)stream, x, scale, trans, w, u, d, tl)
    KAN_WAV_DISPATCH(KAN_WAV_F)
#undef KAN_WAV_F
    return launch_ok("wav_fwd");
}

int kan_wav_bwd_input(const float* du, const float* x, const float* scale, const float* trans, const float* w, float* dx, const KanWavGeom* g,
                      void* stream) {
    if (int rc = wav_check(g)) return rc;
    if (!du || !x || !scale || !trans || !w || !dx) return fail("null pointer in kan_wav_bwd_input");
    KanWavRoute r; long long fwd_blocks, blocks; size_t fwd_smem, par_smem;
    wav_plan(g, r, fwd_blocks, blocks, fwd_smem, par_smem);
    const WavDev d = wav_dev(g);
    const int cblocks = (g->C + WAV_CB - 1) / WAV_CB;
    if (blocks >= (1ll << 31) || cblocks > 65535) return fail("wavelet bwd-input grid too large");
#define KAN_WAV_I(WT) hipLaunchKernelGGL((k_wav_bwd_input<WT, true>), dim3((unsigned)blocks, cblocks), dim3(256), 0, (hipStream_t)stream, du, x, scale, trans, w, dx, d)
#define KAN_WAV_IS(WT) hipLaunchKernelGGL((k_wav_bwd_input<WT, false>), dim3((unsigned)blocks, cblocks), dim3(256), 0, (hipStream_t)stream, du, x, scale, trans, w, dx, d)
#define KAN_WAV_I9(WT) hipLaunchKernelGGL((k_wav_bwd_input9<WT>), dim3((unsigned)blocks, cblocks), dim3(256), 0, (hipStream_t)stream, du, x, scale, trans, w, dx, d)
    static_assert(WAV_TAPS == 9, "k_wav_bwd_input9 holds a table of 9 taps");
    if (r.bwd_input_kernel == KAN_WAV_BI_TAPS9) { KAN_WAV_DISPATCH(KAN_WAV_I9) }
    else if (r.bwd_input_kernel == KAN_WAV_BI_STRIDE1) { KAN_WAV_DISPATCH(KAN_WAV_I) } else { KAN_WAV_DISPATCH(KAN_WAV_IS) }
#undef KAN_WAV_I9
#undef KAN_WAV_IS
#undef KAN_WAV_I
    return launch_ok("wav_bwd_input");
}

long long kan_wav_param_workspace(const KanWavGeom* g) {
    if (wav_check(g)) return -1;
    KanWavRoute r; long long fwd_blocks, bi_blocks; size_t fwd_smem, par_smem;
    wav_plan(g, r, fwd_blocks, bi_blocks, fwd_smem, par_smem);
    return r.chunks * (long long)g->O * g->C * (g->kh * g->kw + 2);
}

int kan_wav_bwd_params(const float* du, const float* x, const float* scale, const float* trans, const float* w, float* dw, float* dscale, float* dtrans,
                       float* workspace, const KanWavGeom* g, void* stream) {
    if (int rc = wav_check(g)) return rc;
    if (!du || !x || !scale || !trans || !w || !dw || !dscale || !dtrans || !workspace) return fail("null pointer in kan_wav_bwd_params");
    if (g->O > 65535 * 16) return fail("wavelet bwd-params grid too large");
    KanWavRoute r; long long fwd_blocks, bi_blocks; size_t fwd_smem, smem;
    wav_plan(g, r, fwd_blocks, bi_blocks, fwd_smem, smem);
    const WavDev d = wav_dev(g);
    const int T = g->kh * g->kw, chunks = r.chunks;
    const long long n = (long long)g->O * g->C * (T + 2);
    static_assert(WAV_TAPS == 9, "the parameter kernels keep 9 taps in registers per pass (TMAX)");
    if (r.params_kernel == KAN_WAV_PAR_TILED) {
        const WavBand wb = {r.BH, r.NI, r.RU, r.CU, r.XP, r.UP, r.bands, r.items, r.items_per_chunk};
        const dim3 grid((g->C + 15) / 16, (g->O + 15) / 16, chunks);
        for (int pass = 0; pass < r.passes; ++pass) {                    // 9 taps per pass (dtrans / dscale add up over the passes)
            const int t0 = pass * WAV_TAPS;
#define KAN_WAV_PT(WT) hipLaunchKernelGGL((k_wav_bwd_params_tiled<WT>), grid, dim3(256), smem, (hipStream_t)stream, du, x, scale, trans, w, workspace, d, wb, t0)
            KAN_WAV_DISPATCH(KAN_WAV_PT)
#undef KAN_WAV_PT
            if (int rc = launch_ok("wav_bwd_params_tiled")) return rc;
        }
    } else {
        if (g->O > 65535) return fail("wavelet bwd-params grid too large");
        const int ppc = r.px_per_chunk;
#define KAN_WAV_P(WT) hipLaunchKernelGGL((k_wav_bwd_params<WT>), dim3(g->C, g->O, chunks), dim3(256), 0, (hipStream_t)stream, du, x, scale, trans, w, workspace, d, ppc)
        KAN_WAV_DISPATCH(KAN_WAV_P)
#undef KAN_WAV_P
        if (int rc = launch_ok("wav_bwd_params")) return rc;
    }
    hipLaunchKernelGGL(k_wav_sum_parts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, workspace, chunks, n, T, dw, dscale, dtrans);
    return launch_ok("wav_sum_parts");
}

}  // extern "C"

namespace {
