// Rhythm on the onset envelope (rhythm.py: tempogram, tempo, beat_track; the definitions of librosa.feature.tempogram,
// librosa.feature.tempo and librosa.beat.beat_track).
//
// ap_tempogram_wave_kernel (W <= 512: one wave per frame on the N = 1024 transform, described at the kernel) and
// ap_tempogram_kernel (any W up to 8192: the fallback and the cross-check).  For an envelope e (n) of one clip, a window
// w (W), h = W / 2:
//   center: p = e between two linear ramps of h values, p[i] = e[0] i / h on the left, e[n-1] (h - 1 - j) / h on the right
//           (np.pad(e, h, mode="linear_ramp", end_values=0)), T = n;  else p = e, T = n - W + 1
//   x_t[i]   = w[i] p[t + i]
//   ac[k, t] = sum_{i < W - k} x_t[i] x_t[i + k]                        (i ascending)
//   tg[k, t] = ac[k, t] / m_t, m_t = max_k |ac[k, t]| (left alone where m_t < FLT_MIN);  norm off: tg = ac
//   General kernel: a 256-thread workgroup owns 64 frames of one clip; lane = frame, wave v owns the lags v, v + 4, ...  The slice
//   p[t0 .. t0 + 63 + W - 1] (the ramps are computed as it is loaded: no padded copy exists) and the window are staged in
//   LDS, a wave reads 64 consecutive floats of the slice per instruction and stores 64 consecutive frames of a lag.  With
//   the norm every sum is formed twice, once for m_t and once for the store: direct sums in a fixed order, accumulated
//   in float64 (sequential float32 sums of 512 terms miss the tolerance the float32 FFT route sets); any W up to 8192.
//   Aggregate mode (agg != NULL): the tile's sum_t tg[k, t] goes to agg[clip][tile][k]; a wave stages 16 of its lags as
//   [lag][frame] and lane c adds the 64 frames of lag c in frame order.  ap_tempo_pick_kernel joins the tiles in tile
//   order: no atomics, and a clip's bits do not depend on its place in the batch.
//
// ap_tempo_pick_kernel.  Per column: g[k] = (sum_r G[k, r]) / div, the first k maximising log1p(1e6 g[k]) + prior[k],
//   as int32.  One workgroup per column, the threads over k.
//
// ap_beat_track_kernel.  One workgroup per row (T <= 16384, period 2 .. 2048), the row in LDS; the stages are those of
//   the definition in include/audioprims.h.  The dynamic programme runs in blocks of h = rint(P / 2) frames: C[i] reads
//   C[<= i - h] only, so the frames of a block are independent; g threads share a frame's candidates d = 2P .. h and
//   the frame's first thread joins their maxima (the smaller candidate index, i.e. the larger d, on a tie).  C is
//   written over L in place, the links over o'; the trim recomputes L at the beats from the row in memory with the
//   same operations (contraction is off, so the bits are the same).
#pragma once
#include "ap_launch.h"
#include "kernels_wave.h"
#include "kernels_wave512.h"

extern __shared__ __attribute__((aligned(16))) char ap_smem[];

#define APTG_WAVES 4            // waves per workgroup; wave v owns the lags v, v + 4, ...
#define APTG_TT 64              // frames per tile: the lanes of a wave
#define APTG_WMAX 8192
#define APTG_AC 16              // lags a wave stages at a time for the aggregate
#define APTG_FLT_MIN 1.17549435e-38f
#define APTP_BLOCK 256
#define APBT_BLOCK 256
#define APBT_TMAX 16384
#define APBT_PMAX 2048

static inline bool ap_rhythm_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

// ---- tempogram -------------------------------------------------------------------------------------------------
struct ApTempogramParams {
    const float *env, *win;     // (B, rs), (W)
    const ap_float2 *tw;        // (1024) twiddles: the wave kernel; NULL: the general kernel
    float *out, *agg;           // (B, W, T) or NULL, (B, n_tt, W) or NULL
    int64_t B, rs, n_tiles;
    int n, W, h, T, center, norm, n_tt;
    int off_win, off_part, off_stage, lds_bytes;
    int off_tw2, off_tw1, off_slice, slice_floats, off_tile, tile_floats;      // wave kernel
};

#define APTW_WMAX 512           // the wave kernel: W windowed values, zero-padded to the N = 1024 transform, lags 0 .. W - 1
#define APTW_G 8                // frames a wave stages before their lags leave as runs along T
static inline bool ap_tempogram_wave_shape(int W) { return W >= 1 && W <= APTW_WMAX; }

static inline int64_t ap_tempogram_frames(int64_t n, int W, int center) { return center ? n : n - W + 1; }

static inline int ap_prepare_tempogram(ApTempogramParams &P, const float *env, int64_t B, int64_t n, int64_t rs,
                                       const float *win, int W, int center, int norm, const float *tw, float *out,
                                       float *agg) {
    if (!env || !win || (!out && !agg)) AP_FAIL(AP_ERR_INVALID, "tempogram: NULL buffer");
    if (B <= 0 || n <= 0) AP_FAIL(AP_ERR_INVALID, "tempogram: the envelope must be non-empty, got (%lld, %lld)", (long long)B, (long long)n);
    if (W < 1) AP_FAIL(AP_ERR_INVALID, "win_length must be a positive integer, got %d", W);
    if (W > APTG_WMAX) AP_FAIL(AP_ERR_UNSUPPORTED, "tempogram: win_length beyond %d is not supported, got %d", APTG_WMAX, W);
    if (rs < n) AP_FAIL(AP_ERR_INVALID, "tempogram: row stride (%lld) must be >= n = %lld", (long long)rs, (long long)n);
    if (n > (1 << 28)) AP_FAIL(AP_ERR_UNSUPPORTED, "tempogram: n must be <= 2^28");
    if (B > ((int64_t)1 << 40) || rs > ((int64_t)1 << 40)) AP_FAIL(AP_ERR_UNSUPPORTED, "tempogram: extents too large");
    const int64_t T = ap_tempogram_frames(n, W, center);
    if (T <= 0) AP_FAIL(AP_ERR_INVALID, "tempogram: the envelope (%lld frames) is shorter than win_length (%d)", (long long)n, W);
    if ((double)B * (double)W * (double)T * 4.0 > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "tempogram: more than 2^63 bytes");
    const int64_t n_tt = (T + APTG_TT - 1) / APTG_TT;
    if ((double)B * (double)n_tt > (double)kApMaxGrid) AP_FAIL(AP_ERR_UNSUPPORTED, "tempogram: more than 2^31 - 1 tiles");
    const int64_t in_bytes = ((B - 1) * rs + n) * 4;
    if ((out && ap_rhythm_overlap(env, in_bytes, out, B * W * T * 4)) || (agg && ap_rhythm_overlap(env, in_bytes, agg, B * n_tt * W * 4)))
        AP_FAIL(AP_ERR_INVALID, "tempogram: an output overlaps the envelope");
    P.env = env; P.win = win; P.out = out; P.agg = agg;
    P.B = B; P.rs = rs; P.n_tiles = B * n_tt;
    P.n = (int)n; P.W = W; P.h = W / 2; P.T = (int)T; P.center = center ? 1 : 0; P.norm = norm ? 1 : 0; P.n_tt = (int)n_tt;
    int off = ap_align16((APTG_TT + W - 1) * 4);
    P.off_win = off; off += ap_align16(W * 4);
    P.off_part = off; off += APTG_WAVES * APTG_TT * 4;
    P.off_stage = off; off += agg ? APTG_WAVES * APTG_AC * (APTG_TT + 1) * 4 : 0;
    P.lds_bytes = off;
    P.tw = reinterpret_cast<const ap_float2 *>(tw);
    if (tw) {
        // wave kernel: exchange buffers, the two twiddle tables, the window, a slice and a [lag][8 frames] tile per wave
        if (!ap_tempogram_wave_shape(W)) AP_FAIL(AP_ERR_UNSUPPORTED, "tempogram: the wave kernel serves win_length <= %d, got %d", APTW_WMAX, W);
        off = APTG_WAVES * APH_X_COMPLEX * (int)sizeof(ap_float2);
        P.off_tw2 = off; off += APW_TW2_COMPLEX * (int)sizeof(ap_float2);
        P.off_tw1 = off; off += 8 * 64 * (int)sizeof(ap_float2);
        P.off_win = off; off += ap_align16(W * 4);
        P.slice_floats = (APTG_TT + W - 1 + 3) & ~3;
        P.off_slice = off; off += APTG_WAVES * P.slice_floats * 4;
        P.tile_floats = out ? (APTW_G * W + W / 2 + 4) & ~3 : 0;
        P.off_tile = off; off += APTG_WAVES * P.tile_floats * 4;
        P.lds_bytes = off;
    }
    return AP_OK;
}

static inline int ap_tempogram_grid(const ApTempogramParams &P) { return (int)(P.n_tiles < (1 << 20) ? P.n_tiles : (1 << 20)); }

// p[q] of the (virtually) padded envelope, 0 beyond it
AP_DEV float aptg_padded(const ApTempogramParams &P, const float *e, int q) {
    if (!P.center) return q < P.n ? e[q] : 0.0f;
    const int i = q - P.h;
    if (i < 0) return e[0] * (float)q / (float)P.h;
    if (i < P.n) return e[i];
    const int j = i - P.n;
    return j < P.h ? e[P.n - 1] * (float)(P.h - 1 - j) / (float)P.h : 0.0f;
}

__global__ void __launch_bounds__(64 * APTG_WAVES) ap_tempogram_kernel(ApTempogramParams P) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int W = P.W;
    float *ps = reinterpret_cast<float *>(ap_smem);
    float *ws = reinterpret_cast<float *>(ap_smem + P.off_win);
    float *part = reinterpret_cast<float *>(ap_smem + P.off_part);
    float *stage = reinterpret_cast<float *>(ap_smem + P.off_stage) + wave * APTG_AC * (APTG_TT + 1);
    for (int i = tid; i < W; i += 64 * APTG_WAVES) ws[i] = P.win[i];
    const float *xs = ps + lane;
    auto ac = [&](int k) -> float {
        double acc = 0.0;                                       // x_t in float32, its products exact, one rounding at the end
        for (int i = 0; i < W - k; ++i) acc += (double)(ws[i] * xs[i]) * (double)(ws[i + k] * xs[i + k]);
        return (float)acc;
    };
    for (int64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
        const int64_t b = tile / P.n_tt;
        const int tt = (int)(tile - b * P.n_tt);
        const int t0 = tt * APTG_TT;
        const int t = t0 + lane;
        const float *e = P.env + b * P.rs;
        for (int j = tid; j < APTG_TT + W - 1; j += 64 * APTG_WAVES) ps[j] = aptg_padded(P, e, t0 + j);
        AP_LDS_BARRIER();
        float m = 0.0f;
        if (P.norm) {
            for (int k = wave; k < W; k += APTG_WAVES) m = fmaxf(m, fabsf(ac(k)));
            part[wave * APTG_TT + lane] = m;
            AP_LDS_BARRIER();
            m = fmaxf(fmaxf(part[lane], part[APTG_TT + lane]), fmaxf(part[2 * APTG_TT + lane], part[3 * APTG_TT + lane]));
        }
        const bool scale = P.norm && m >= APTG_FLT_MIN;
        float *dst = P.out ? P.out + (b * W) * (int64_t)P.T + t : nullptr;
        for (int k0 = wave; k0 < W; k0 += APTG_WAVES * APTG_AC) {
            for (int c = 0; c < APTG_AC; ++c) {
                const int k = k0 + APTG_WAVES * c;
                if (k >= W) break;                              // (uniform over the wave)
                float v = ac(k);
                if (scale) v = v / m;
                if (dst && t < P.T) dst[(int64_t)k * P.T] = v;
                if (P.agg) stage[c * (APTG_TT + 1) + lane] = t < P.T ? v : 0.0f;
            }
            if (P.agg) {
                AP_WAVE_SYNC();
                const int k = k0 + APTG_WAVES * lane;
                if (lane < APTG_AC && k < W) {
                    float s = 0.0f;
                    for (int j = 0; j < APTG_TT; ++j) s += stage[lane * (APTG_TT + 1) + j];
                    P.agg[(b * P.n_tt + tt) * (int64_t)W + k] = s;
                }
                AP_WAVE_SYNC();
            }
        }
        AP_LDS_BARRIER();                       // the next tile overwrites the slice and the maxima
    }
}

// persistent grid of the wave kernel: a wave owns whole 64-frame tiles (the aggregate's unit)
static inline int ap_tempogram_wave_grid(const ApTempogramParams &P) {
    int64_t g = (P.n_tiles + APTG_WAVES - 1) / APTG_WAVES;
    if (g > 256 * 2) g = 256 * 2;
    return (int)(g < 1 ? 1 : g);
}

#ifdef AP_HOST_EMU
AP_DEV float aptg_lane_get(float x, int src) { return emu_lane_perm(x, src); }
#else
AP_DEV float aptg_lane_get(float x, int src) { return __shfl(x, src & 63, 64); }
#endif
AP_DEV float aptg_wave_max(float v, int lane) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmaxf(v, aptg_lane_get(v, lane ^ m));
    return v;
}

// W <= 512: one wave per frame on the N = 1024 transform of kernels_wave512.h.  x_t (W values, the rest zero) as 512
// packed pairs -> forward real transform -> |A|^2 on the paired bins k and 512 - k -> Hermitian merge and the same
// transform on conjugated data -> ac(0 .. 1023), of which the lags below W are free of wrap-around (W <= 512): two
// transforms per frame.  Lane l holds the lags 2 (l + 64 e), 2 (l + 64 e) + 1, e < 4; m_t is a wave max-reduction; the
// values of 8 consecutive frames are staged in a wave-private LDS tile [lag][8] (one pad float per 2 lags: a lane's
// stride is 17 floats) and leave as runs along T; the aggregate is 8 registers per lane, added in frame order.
__global__ void __launch_bounds__(64 * APTG_WAVES) ap_tempogram_wave_kernel(ApTempogramParams P) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = AP_UNIFORM(tid >> 6);
    const int W = P.W;
    ap_float2 *X = reinterpret_cast<ap_float2 *>(ap_smem) + wave * APH_X_COMPLEX;
    const ap_float2 *TW2 = reinterpret_cast<const ap_float2 *>(ap_smem + P.off_tw2);
    const ap_float2 *TW1 = reinterpret_cast<const ap_float2 *>(ap_smem + P.off_tw1);
    float *ws = reinterpret_cast<float *>(ap_smem + P.off_win);
    float *SL = reinterpret_cast<float *>(ap_smem + P.off_slice) + wave * P.slice_floats;
    float *TL = reinterpret_cast<float *>(ap_smem + P.off_tile) + wave * P.tile_floats;
    {
        ap_float2 *tw2 = reinterpret_cast<ap_float2 *>(ap_smem + P.off_tw2);
        ap_float2 *tw1 = reinterpret_cast<ap_float2 *>(ap_smem + P.off_tw1);
        for (int i = tid; i < 8 * 64; i += 64 * APTG_WAVES) tw1[i] = P.tw[(2 * (i & 63) * (i >> 6)) & 1023];     // as in ap_yin_wave_kernel
        if (tid < 64) tw2[tid] = P.tw[16 * (tid >> 3) * (tid & 7)];
        for (int i = tid; i < W; i += 64 * APTG_WAVES) ws[i] = P.win[i];
    }
    AP_LDS_BARRIER();                       // the only workgroup barrier
    const ApwLane lc = apw_lane_init(lane, TW2, P.tw);       // (tws0h, half, halfc of it)
    const int64_t worker = (int64_t)blockIdx.x * APTG_WAVES + wave;
    const int64_t n_workers = (int64_t)gridDim.x * APTG_WAVES;
    const float scale = 2.0f / 1024.0f;
    for (int64_t tile = worker; tile < P.n_tiles; tile += n_workers) {
        const int64_t b = tile / P.n_tt;
        const int tt = (int)(tile - b * P.n_tt);
        const int t0 = tt * APTG_TT;
        const float *e = P.env + b * P.rs;
        for (int j = lane; j < APTG_TT + W - 1; j += 64) SL[j] = aptg_padded(P, e, t0 + j);
        AP_WAVE_SYNC();
        const int nfr = P.T - t0 < APTG_TT ? P.T - t0 : APTG_TT;
        float sum[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) sum[i] = 0.0f;
        for (int f = 0; f < nfr; ++f) {
            ap_float2 v[8], ak[4], am[4], azh;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i0 = 2 * (lane + 64 * j);
                const float x0 = (j < 4 && i0 < W) ? ws[i0] * SL[f + i0] : 0.0f;
                const float x1 = (j < 4 && i0 + 1 < W) ? ws[i0 + 1] * SL[f + i0 + 1] : 0.0f;
                v[j] = ap_mk(x0, x1);
            }
            aph_forward(v, X, TW1, TW2, lane);
            aph_split<true>(v, X, lc.tws0h, lane, ak, am, azh);
            // |A|^2, Hermitian merge and the inverse transform as in ap_yin_wave_kernel (B = A)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const ap_float2 a_k = ap_mk(ak[r].x * ak[r].x + ((r == 0 && lane == 0) ? 0.0f : ak[r].y * ak[r].y), 0.0f);
                const ap_float2 a_m = ap_mk(am[r].x * am[r].x + ((r == 0 && lane == 0) ? 0.0f : am[r].y * am[r].y), 0.0f);
                const ap_float2 a = ap_add_conj(a_k, a_m);
                const ap_float2 d = ap_sub_conj(a_k, a_m);
                const ap_float2 w = r == 0 ? lc.tws0h : ap_mul_bw_c(lc.tws0h, APH_C16(r), APH_S16(r));
                const ap_float2 o = ap_mul_bw(d, w);
                v[r] = ap_fma_sub_swap(a, lc.halfc, o);
                const int km = (512 - (lane + 64 * r)) & 511;
                if (!(r == 0 && lane == 0)) X[km - 256] = ap_fma_add_mi(a, lc.half, o);
            }
            if (lane == 0) X[0] = ap_mk(azh.x * azh.x + azh.y * azh.y, 0.0f);      // the middle bin
            AP_WAVE_SYNC();
#pragma unroll
            for (int j = 4; j < 8; ++j) v[j] = X[lane + 64 * (j - 4)];
            AP_WAVE_SYNC();
            aph_forward(v, X, TW1, TW2, lane);
            float r8[8];
            float m = 0.0f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {               // lags 2 (lane + 64 q) and the next
                const int k = 2 * (lane + 64 * q);
                r8[2 * q] = k < W ? v[q].x * scale : 0.0f;
                r8[2 * q + 1] = k + 1 < W ? -v[q].y * scale : 0.0f;
                m = fmaxf(m, fmaxf(fabsf(r8[2 * q]), fabsf(r8[2 * q + 1])));
            }
            if (P.norm) {
                m = aptg_wave_max(m, lane);
                if (m >= APTG_FLT_MIN) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) r8[i] = r8[i] / m;
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) sum[i] += r8[i];
            if (P.out) {                                // (uniform)
                const int slot = f & (APTW_G - 1);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int k = 2 * (lane + 64 * (i >> 1)) + (i & 1);
                    if (k < W) TL[APTW_G * k + (k >> 1) + slot] = r8[i];
                }
                if (slot == APTW_G - 1 || f == nfr - 1) {
                    AP_WAVE_SYNC();
                    float *dst = P.out + (b * W) * (int64_t)P.T + (t0 + f - slot);
                    for (int idx = lane; idx < APTW_G * W; idx += 64) {
                        const int k = idx / APTW_G, col = idx & (APTW_G - 1);
                        if (col <= slot) dst[(int64_t)k * P.T + col] = TL[APTW_G * k + (k >> 1) + col];
                    }
                    AP_WAVE_SYNC();
                }
            }
        }
        if (P.agg) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = 2 * (lane + 64 * (i >> 1)) + (i & 1);
                if (k < W) P.agg[(b * P.n_tt + tt) * (int64_t)W + k] = sum[i];
            }
        }
        AP_WAVE_SYNC();                     // the next tile overwrites the slice
    }
}

// ---- tempo: the pick ---------------------------------------------------------------------------------------------
struct ApTempoPickParams {
    const float *g, *prior;     // values (see the strides), (W)
    int *idx;                   // (B, n_col)
    int64_t B, n_col, sb, sk, sc, n_red, sr;
    int W;
    float div;
    int lds_bytes;
};

static inline int ap_prepare_tempo_pick(ApTempoPickParams &P, const float *g, int64_t B, int64_t n_col, int W, int64_t sb,
                                        int64_t sk, int64_t sc, int64_t n_red, int64_t sr, float div, const float *prior,
                                        int *idx) {
    if (!g || !prior || !idx) AP_FAIL(AP_ERR_INVALID, "tempo: NULL buffer");
    if (B <= 0 || n_col <= 0 || n_red <= 0) AP_FAIL(AP_ERR_INVALID, "tempo: nothing to pick from, got (%lld, %lld, %lld)", (long long)B, (long long)n_col, (long long)n_red);
    if (W < 1) AP_FAIL(AP_ERR_INVALID, "tempo: the tempogram must have at least one lag, got %d", W);
    if (sb < 0 || sk < 0 || sc < 0 || sr < 0) AP_FAIL(AP_ERR_INVALID, "tempo: negative stride");
    if (!(div > 0.0f)) AP_FAIL(AP_ERR_INVALID, "tempo: the divisor must be positive");
    if ((double)B * (double)n_col > (double)kApMaxGrid) AP_FAIL(AP_ERR_UNSUPPORTED, "tempo: more than 2^31 - 1 columns");
    P.g = g; P.prior = prior; P.idx = idx;
    P.B = B; P.n_col = n_col; P.sb = sb; P.sk = sk; P.sc = sc; P.n_red = n_red; P.sr = sr;
    P.W = W; P.div = div;
    P.lds_bytes = 2 * APTP_BLOCK * 4;
    return AP_OK;
}

static inline int ap_tempo_pick_grid(const ApTempoPickParams &P) {
    const int64_t n = P.B * P.n_col;
    return (int)(n < (1 << 20) ? n : (1 << 20));
}

__global__ void __launch_bounds__(APTP_BLOCK) ap_tempo_pick_kernel(ApTempoPickParams P) {
    const int tid = threadIdx.x;
    float *rv = reinterpret_cast<float *>(ap_smem);
    int *rk = reinterpret_cast<int *>(rv + APTP_BLOCK);
    const int64_t n = P.B * P.n_col;
    for (int64_t col = blockIdx.x; col < n; col += gridDim.x) {
        const int64_t b = col / P.n_col;
        const float *base = P.g + b * P.sb + (col - b * P.n_col) * P.sc;
        float best = 0.0f;
        int bk = -1;
        for (int k = tid; k < P.W; k += APTP_BLOCK) {
            const float *gk = base + (int64_t)k * P.sk;
            float s = 0.0f;
            for (int64_t r = 0; r < P.n_red; ++r) s += gk[r * P.sr];
            const float v = log1pf(1.0e6f * (s / P.div)) + P.prior[k];
            if (bk < 0 || v > best) { best = v; bk = k; }
        }
        rv[tid] = best; rk[tid] = bk;
        AP_LDS_BARRIER();
        if (tid == 0) {                                         // the first k of the largest value
            const int nt = P.W < APTP_BLOCK ? P.W : APTP_BLOCK;
            for (int j = 1; j < nt; ++j) {
                const float v = rv[j];
                if (v > best || (v == best && rk[j] < bk)) { best = v; bk = rk[j]; }
            }
            P.idx[col] = bk;
        }
        AP_LDS_BARRIER();                       // the next column overwrites the records
    }
}

// ---- beat tracking -----------------------------------------------------------------------------------------------
struct ApBeatParams {
    const float *env;           // (B, rs)
    const int *period;          // (B)
    unsigned char *mask;        // (B, T)
    int *count;                 // (B): beats of the row, -1 for a period outside 2 .. APBT_PMAX
    float *L, *C;               // (B, T) or NULL
    int *link;                  // (B, T) or NULL
    int64_t B, rs;
    int T, trim;
    float tightness;
    int off_z, off_tab, off_bits, off_red, lds_bytes;
};

static inline int ap_prepare_beat_track(ApBeatParams &P, const float *env, int64_t B, int64_t T, int64_t rs, const int *period,
                                        float tightness, int trim, unsigned char *mask, int *count, float *L, float *C,
                                        int *link) {
    if (!env || !period || !mask || !count) AP_FAIL(AP_ERR_INVALID, "beat_track: NULL buffer");
    if (B <= 0 || T <= 0) AP_FAIL(AP_ERR_INVALID, "beat_track: the envelope must be non-empty, got (%lld, %lld)", (long long)B, (long long)T);
    if (T > APBT_TMAX) AP_FAIL(AP_ERR_UNSUPPORTED, "beat_track: rows of more than %d frames are not supported, got %lld", APBT_TMAX, (long long)T);
    if (rs < T) AP_FAIL(AP_ERR_INVALID, "beat_track: row stride (%lld) must be >= T = %lld", (long long)rs, (long long)T);
    if (!(tightness > 0.0f)) AP_FAIL(AP_ERR_INVALID, "tightness must be strictly positive");
    if (B > ((int64_t)1 << 40) || rs > ((int64_t)1 << 40)) AP_FAIL(AP_ERR_UNSUPPORTED, "beat_track: extents too large");
    if (ap_rhythm_overlap(env, ((B - 1) * rs + T) * 4, mask, B * T)) AP_FAIL(AP_ERR_INVALID, "beat_track: the mask overlaps the envelope");
    const int t = (int)T;
    P.env = env; P.period = period; P.mask = mask; P.count = count; P.L = L; P.C = C; P.link = link;
    P.B = B; P.rs = rs; P.T = t; P.trim = trim ? 1 : 0; P.tightness = tightness;
    int off = ap_align16(t * 4);
    P.off_z = off; off += ap_align16(t * 4);
    P.off_tab = off; off += ap_align16((2 * APBT_PMAX + 1) * 4);
    P.off_bits = off; off += ap_align16(((t + 63) / 64) * 8);
    P.off_red = off; off += (2 * APBT_BLOCK + 32) * 8 + 64;
    P.lds_bytes = off;
    return AP_OK;
}

static inline int ap_beat_track_grid(const ApBeatParams &P) { return (int)(P.B < (1 << 16) ? P.B : (1 << 16)); }

// rint(P / 2), halves to even
AP_DEV int apbt_half(int P) { return (P & 1) ? (P >> 1) + ((P >> 1) & 1) : P >> 1; }

// tap k (-P .. P) of the local-score window and the transition cost of a step of d frames, rounded once from float64
AP_DEV float apbt_tap(int k, int P) {
    const double x = 32.0 * (double)k / (double)P;
    return (float)exp(-0.5 * x * x);
}
AP_DEV float apbt_cost(int d, int P, float tightness) {
    const double l = log((double)d / (double)P);
    return (float)(-(double)tightness * l * l);
}

__global__ void __launch_bounds__(APBT_BLOCK) ap_beat_track_kernel(ApBeatParams Q) {
#ifndef AP_HOST_EMU
#pragma clang fp contract(off)   // L at the beats is formed twice (stage 2 and the trim) and must have the same bits
#endif
    const int tid = threadIdx.x;
    const int T = Q.T;
    const int nw = (T + 63) >> 6;
    float *Y = reinterpret_cast<float *>(ap_smem);                      // L, then C in place, then the beats (int)
    float *Z = reinterpret_cast<float *>(ap_smem + Q.off_z);            // o', then the links (int), then L at the beats
    int *LK = reinterpret_cast<int *>(Z);
    int *BT = reinterpret_cast<int *>(Y);
    float *tab = reinterpret_cast<float *>(ap_smem + Q.off_tab);        // the taps, then the transition costs
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(ap_smem + Q.off_bits);
    double *rd = reinterpret_cast<double *>(ap_smem + Q.off_red);       // [2][256] reduction records
    float *rv = reinterpret_cast<float *>(rd);                          // the same bytes as the DP's (value, candidate)
    int *ri = reinterpret_cast<int *>(rv + APBT_BLOCK);
    double *qd = rd + 2 * APBT_BLOCK;                                   // [32]
    int *sh = reinterpret_cast<int *>(qd + 32);                         // [16] row scalars
    float *shf = reinterpret_cast<float *>(sh + 8);

    // sum / maximum of one double per thread in a fixed order: 16 groups of 16, then the 16 partial results
    auto bsum = [&](double x) -> double {
        rd[tid] = x;
        AP_LDS_BARRIER();
        if (tid < 16) {
            double s = 0.0;
            for (int i = 0; i < 16; ++i) s += rd[tid * 16 + i];
            qd[tid] = s;
        }
        AP_LDS_BARRIER();
        double s = 0.0;
        for (int i = 0; i < 16; ++i) s += qd[i];
        AP_LDS_BARRIER();
        return s;
    };
    auto bmax = [&](double x) -> double {
        rd[tid] = x;
        AP_LDS_BARRIER();
        if (tid < 16) {
            double s = rd[tid * 16];
            for (int i = 1; i < 16; ++i) s = fmax(s, rd[tid * 16 + i]);
            qd[tid] = s;
        }
        AP_LDS_BARRIER();
        double s = qd[0];
        for (int i = 1; i < 16; ++i) s = fmax(s, qd[i]);
        AP_LDS_BARRIER();
        return s;
    };

    for (int64_t b = blockIdx.x; b < Q.B; b += gridDim.x) {
        const float *ob = Q.env + b * Q.rs;
        const int P = Q.period[b];
        // ---- 1: finiteness / any, mean, two-pass deviation (ddof = 1) -------------------------------------------
        double s = 0.0, nbad = 0.0, nany = 0.0;
        for (int n = tid; n < T; n += APBT_BLOCK) {
            const float v = ob[n];
            Z[n] = v;
            s += (double)v;
            if (!(fabsf(v) <= 3.4028234664e38f)) nbad += 1.0;
            if (v != 0.0f) nany += 1.0;
        }
        nbad = bsum(nbad);
        nany = bsum(nany);
        const bool bad_period = P < 2 || P > APBT_PMAX;
        bool empty = T < 2 || nbad > 0.0 || nany == 0.0 || bad_period;
        float stdf = 0.0f;
        if (!empty) {                                                   // (uniform)
            const double mean = bsum(s) / (double)T;
            double dv = 0.0;
            for (int n = tid; n < T; n += APBT_BLOCK) {
                const double d = (double)Z[n] - mean;
                dv += d * d;
            }
            stdf = (float)sqrt(bsum(dv) / (double)(T - 1));
            empty = !(stdf > 0.0f) || !(stdf <= 3.4028234664e38f);
        }
        if (empty) {
            for (int n = tid; n < T; n += APBT_BLOCK) {
                Q.mask[b * T + n] = 0;
                if (Q.L) Q.L[b * T + n] = 0.0f;
                if (Q.C) Q.C[b * T + n] = 0.0f;
                if (Q.link) Q.link[b * T + n] = -1;
            }
            if (tid == 0) Q.count[b] = bad_period ? -1 : 0;
            AP_LDS_BARRIER();
            continue;
        }
        const int h = apbt_half(P);
        const int nd = 2 * P - h + 1;                                   // candidates d = 2P - c, c = 0 .. nd - 1
        // ---- 2: o' and the local score, every frame on its own ---------------------------------------------------
        for (int n = tid; n < T; n += APBT_BLOCK) Z[n] = Z[n] / stdf;   // the values this thread stored
        for (int k = tid; k <= 2 * P; k += APBT_BLOCK) tab[k] = apbt_tap(k - P, P);
        AP_LDS_BARRIER();
        double lmax = -INFINITY;
        for (int i = tid; i < T; i += APBT_BLOCK) {
            const int k_lo = i - (T - 1) > -P ? i - (T - 1) : -P, k_hi = i < P ? i : P;
            float acc = 0.0f;
            for (int k = k_lo; k <= k_hi; ++k) acc += tab[k + P] * Z[i - k];
            Y[i] = acc;
            lmax = fmax(lmax, (double)acc);
            if (Q.L) Q.L[b * T + i] = acc;
        }
        // ---- 3: max(L) and the first frame at or above 1 % of it ------------------------------------------------
        const float thr1 = 0.01f * (float)bmax(lmax);
        double fst = -(double)T;
        for (int i = tid; i < T; i += APBT_BLOCK)
            if (Y[i] >= thr1) { fst = -(double)i; break; }
        const int first = (int)(-bmax(fst));
        for (int c = tid; c < nd; c += APBT_BLOCK) tab[c] = apbt_cost(2 * P - c, P, Q.tightness);
        AP_LDS_BARRIER();
        // ---- 4: the dynamic programme in blocks of h frames ------------------------------------------------------
        int g = APBT_BLOCK;                                             // threads per frame
        while (g > 1 && (g / 2 >= nd || (g / 2) * h >= APBT_BLOCK)) g >>= 1;
        const int slots = APBT_BLOCK / g, slot = tid / g, sub = tid - slot * g;
        for (int i0 = 0; i0 < T; i0 += h) {
            const int nf = T - i0 < h ? T - i0 : h;
            for (int f0 = 0; f0 < nf; f0 += slots) {
                const int f = f0 + slot;
                const int i = i0 + f;
                float best = -INFINITY;
                int bc = nd;
                if (f < nf) {
                    for (int c = sub; c < nd; c += g) {
                        const int j = i - (2 * P - c);
                        const float v = tab[c] + (j >= 0 ? Y[j] : 0.0f);
                        if (v > best) { best = v; bc = c; }
                    }
                }
                if (g > 1) {                                            // (uniform)
                    rv[tid] = best; ri[tid] = bc;
                    AP_LDS_BARRIER();
                    if (sub == 0 && f < nf) {
                        for (int e = 1; e < g; ++e) {
                            const float v = rv[tid + e];
                            const int c = ri[tid + e];
                            if (v > best || (v == best && c < bc)) { best = v; bc = c; }
                        }
                    }
                }
                if (sub == 0 && f < nf) {                               // frames of this block are read by later blocks only
                    Y[i] = Y[i] + best;
                    LK[i] = i < first ? -1 : i - (2 * P - bc);
                }
                AP_LDS_BARRIER();
            }
        }
        if (Q.C || Q.link) {
            for (int i = tid; i < T; i += APBT_BLOCK) {
                if (Q.C) Q.C[b * T + i] = Y[i];
                if (Q.link) Q.link[b * T + i] = LK[i];
            }
        }
        // ---- 5: local maxima of C and the median of their values by rank counting -------------------------------
        double cnt = 0.0;
        for (int w = tid; w < nw; w += APBT_BLOCK) {
            unsigned long long m = 0;
            const int n1 = T - w * 64 < 64 ? T - w * 64 : 64;
            for (int j = 0; j < n1; ++j) {
                const int i = w * 64 + j;
                const bool up = i > 0 && Y[i] > Y[i - 1];
                const bool pk = up && (i == T - 1 || Y[i] >= Y[i + 1]);
                m |= (unsigned long long)(pk ? 1 : 0) << j;
            }
            bits[w] = m;
            cnt += (double)__builtin_popcountll(m);
        }
        const int n_pk = (int)bsum(cnt);                                // (its barriers publish the bits)
        if (n_pk > 0) {
            for (int w = tid; w < nw; w += APBT_BLOCK) {
                unsigned long long mine = bits[w];
                while (mine) {
                    const int i = w * 64 + __builtin_ctzll(mine);
                    mine &= mine - 1;
                    const float v = Y[i];
                    int rank = 0;
                    for (int u = 0; u < nw; ++u) {
                        unsigned long long other = bits[u];
                        while (other) {
                            const int j = u * 64 + __builtin_ctzll(other);
                            other &= other - 1;
                            const float x = Y[j];
                            rank += (x < v || (x == v && j < i)) ? 1 : 0;
                        }
                    }
                    if (rank == (n_pk - 1) / 2) shf[0] = v;
                    if (rank == n_pk / 2) shf[1] = v;
                }
            }
        }
        AP_LDS_BARRIER();
        // ---- 6: the tail and the backtrack, by one thread ------------------------------------------------------------
        if (tid == 0) {
            int nb = 0;
            if (n_pk > 0) {
                const float med = 0.5f * (shf[0] + shf[1]);
                int tail = -1;
                for (int w = nw - 1; w >= 0 && tail < 0; --w) {
                    unsigned long long m = bits[w];
                    while (m) {
                        const int j = 63 - __builtin_clzll(m);
                        m &= ~(1ull << j);
                        if (2.0f * Y[w * 64 + j] > med) { tail = w * 64 + j; break; }
                    }
                }
                for (int cur = tail; cur >= 0 && nb < T; cur = LK[cur]) BT[nb++] = cur;     // C is dead from here on
            }
            sh[0] = nb;
        }
        AP_LDS_BARRIER();
        const int nb = sh[0];                                           // beat j is BT[nb - 1 - j]
        // ---- 7: the trim: L at the beats again, from the row in memory ---------------------------------------------
        for (int j = tid; j < nb; j += APBT_BLOCK) {                    // (the links are dead: Z takes the values)
            const int i = BT[nb - 1 - j];
            const int k_lo = i - (T - 1) > -P ? i - (T - 1) : -P, k_hi = i < P ? i : P;
            float acc = 0.0f;
            for (int k = k_lo; k <= k_hi; ++k) acc += apbt_tap(k, P) * (ob[i - k] / stdf);
            Z[j] = acc;
        }
        AP_LDS_BARRIER();
        auto smooth = [&](int j) -> float {                             // hann(5), 'same'
            const float a = j > 0 ? Z[j - 1] : 0.0f, c = j + 1 < nb ? Z[j + 1] : 0.0f;
            return (0.5f * a + Z[j]) + 0.5f * c;
        };
        double ss = 0.0;
        for (int j = tid; j < nb; j += APBT_BLOCK) {
            const double v = (double)smooth(j);
            ss += v * v;
        }
        ss = bsum(ss);
        const float thr = (Q.trim && nb > 0) ? 0.5f * (float)sqrt(ss / (double)nb) : 0.0f;
        double jlo = -(double)nb, jhi = -1.0;
        for (int j = tid; j < nb; j += APBT_BLOCK) {
            if (smooth(j) > thr) {
                if (jlo == -(double)nb) jlo = -(double)j;
                jhi = (double)j;
            }
        }
        const int lo = (int)(-bmax(jlo)), hi = (int)bmax(jhi);         // lo = nb, hi = -1: nothing above the threshold
        // ---- 8: the mask and the count ---------------------------------------------------------------------------
        for (int w = tid; w < nw; w += APBT_BLOCK) bits[w] = 0;
        AP_LDS_BARRIER();
        if (tid == 0) {
            for (int j = lo; j <= hi; ++j) {
                const int i = BT[nb - 1 - j];
                bits[i >> 6] |= 1ull << (i & 63);
            }
            Q.count[b] = hi >= lo ? hi - lo + 1 : 0;
        }
        AP_LDS_BARRIER();
        for (int n = tid; n < T; n += APBT_BLOCK) Q.mask[b * T + n] = (unsigned char)((bits[n >> 6] >> (n & 63)) & 1);
        AP_LDS_BARRIER();                       // the next row overwrites everything
    }
}
