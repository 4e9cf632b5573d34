// YIN fundamental-frequency tracker (de Cheveigne & Kawahara 2002): yin / yin_cmnd of pitch.py.
//
// For a frame x[0 .. n), W = n / 2 and the lags tau = 0 .. hi (hi <= n - W - 1, so j + tau never leaves the frame):
//   d(tau)  = sum_{j<W} (x[j] - x[j + tau])^2 = e(0) + e(tau) - 2 r(tau)
//   e(tau)  = sum_{j=tau}^{tau+W-1} x[j]^2,   r(tau) = sum_{j<W} x[j] x[j + tau]
//   d'(0)   = 1,  d'(tau) = d(tau) tau / sum_{k=1..tau} d(k)   (1 where that sum is 0)
// and on d'(lo .. hi): the first local minimum below the threshold, else the first global minimum; a parabola
// through its neighbours refines the lag; f0 = sr / lag.  There is no absolute floor anywhere: d' does not
// change when the clip is scaled.
//
// Two kernels:
//
//   ap_yin_wave_kernel (frame_length 2048 and 1024): persistent workgroups, every wave64 owns a contiguous stretch of
//   the flattened (clip, frame) stream and keeps a frame in its registers and its wave-private exchange buffer
//   (no workgroup barrier in the frame loop).  Bounds-checked sample loads (constant padding for free) ->
//   prefix sums of x^2 in a fixed order (e as differences of that one array) -> the packed n / 2-point transform
//   of the frame and of its first half (zero-padded; a subset of the same registers) -> A conj(B) on the paired
//   bins k and n / 2 - k the real split hands out -> Hermitian merge and the same transform on conjugated data ->
//   r(0 .. n / 2 - 1) -> d, running sum (second scan), d' -> pick by wave reductions -> one lane stores f0 and d'.
//   Three transforms per frame; the audio is read once and 4 (or 8) bytes per frame are written.  With CURVE
//   the same kernel stores d'(lo .. hi) instead, staged over a few frames in an LDS tile so that it leaves as
//   runs along T.
//
//   ap_yin_general_kernel (any even frame_length 4 .. 8192): one workgroup per frame, the frame in LDS, d by
//   direct sums (threads over tau), block scan, the same pick.  Slow by design and free of cancellation: the
//   fallback, and the cross-check of the wave kernel.
#pragma once
#include "ap_launch.h"
#include "kernels_wave.h"
#include "kernels_wave512.h"

#define APY_WAVES 4            // waves per workgroup of the wave kernels, one per SIMD
#ifndef APY_MIN_WAVES
#define APY_MIN_WAVES 2         // waves per SIMD the register allocation aims at = workgroups per CU (n = 2048)
#endif
#ifndef APY_MIN_WAVES_1024
#define APY_MIN_WAVES_1024 3    // the same for n = 1024
#endif
#define APY_BIG 3.0e38f

struct ApYinParams {
    const float *y;            // (B, L)
    const ap_float2 *tw;       // (n) twiddles, wave kernel only
    float *f0;                 // (B, T) or NULL
    float *aper;               // (B, T) or NULL: d' at the chosen lag
    float *curve;              // (B, hi - lo + 1, T) or NULL: d'(lo .. hi)
    int64_t L, T, n_clips;
    int n, hop, pad, lo, hi;
    float sr, thr;
    int off_tw2, off_tw1, lds_bytes;     // wave kernel
    // wave kernel, curve output: every wave stages the curves of 2^tile_gs consecutive frames in an LDS tile of
    // tile_floats floats and stores them as runs along T (tile_gs = 0: no tile, every lane stores its own values)
    int off_tile, tile_floats, tile_gs;
    int off_d, off_tot, off_pick;        // general kernel
};

static inline bool ap_yin_wave_shape(int frame_length, int hop, int64_t L) {
    // even hop: the centred frames start at even samples (pair loads, ap_clip_loads_ok); 32-bit sample offsets
    return (frame_length == 2048 || frame_length == 1024) && hop > 0 && hop % 2 == 0 && L > 0 && L <= (1 << 28);
}

static inline int ap_prepare_yin(ApYinParams &P, const float *y, int64_t B, int64_t L, int frame_length, int hop,
                                 int center, int lo, int hi, float sr, float thr, const float *tw, float *f0,
                                 float *aper, float *curve) {
    if (!y || (!f0 && !curve)) AP_FAIL(AP_ERR_INVALID, "yin: NULL buffer");
    if (frame_length < 4 || frame_length > 8192 || frame_length % 2)
        AP_FAIL(AP_ERR_INVALID, "frame_length must be even and in 4 .. 8192, got %d", frame_length);
    if (hop <= 0) AP_FAIL(AP_ERR_INVALID, "hop_length must be positive, got %d", hop);
    if (!(sr > 0.0f)) AP_FAIL(AP_ERR_INVALID, "sr must be positive");
    if (B <= 0 || L <= 0) AP_FAIL(AP_ERR_INVALID, "yin: signal must be non-empty");
    const int64_t T = ap_n_frames(L, frame_length, hop, center);
    if (T <= 0)
        AP_FAIL(AP_ERR_INVALID, "Signal length (%lld) must be >= frame_length (%d). Consider padding the signal.",
                (long long)(L + (center ? 2 * (frame_length / 2) : 0)), frame_length);
    if (lo < 1 || lo >= hi || hi > frame_length - frame_length / 2 - 1)
        AP_FAIL(AP_ERR_INVALID, "yin: lag range [%d, %d] must satisfy 1 <= lo < hi <= frame_length / 2 - 1 = %d", lo,
                hi, frame_length - frame_length / 2 - 1);
    if (B * T > kApMaxGrid) AP_FAIL(AP_ERR_UNSUPPORTED, "yin: more than 2^31 - 1 frames");
    P.y = y;
    P.tw = reinterpret_cast<const ap_float2 *>(tw);
    P.f0 = f0;
    P.aper = aper;
    P.curve = curve;
    P.L = L;
    P.T = T;
    P.n_clips = B;
    P.n = frame_length;
    P.hop = hop;
    P.pad = center ? frame_length / 2 : 0;
    P.lo = lo;
    P.hi = hi;
    P.sr = sr;
    P.thr = thr;
    // wave kernel: exchange buffers, then the two twiddle tables
    int off = APY_WAVES * (frame_length == 2048 ? APW_X_COMPLEX : APH_X_COMPLEX) * (int)sizeof(ap_float2);
    P.off_tw2 = off; off += APW_TW2_COMPLEX * (int)sizeof(ap_float2);
    P.off_tw1 = off; off += (frame_length == 2048 ? 16 : 8) * 64 * (int)sizeof(ap_float2);
    P.off_tile = off;
    P.tile_floats = 0;
    P.tile_gs = 0;
    if (tw && curve) {
        // the largest tile that leaves the workgroups per CU the register allocation allows (2 / 3) their LDS
        const int nl = hi - lo + 1;
        const int budget = AP_LDS_MAX / (frame_length == 2048 ? APY_MIN_WAVES : APY_MIN_WAVES_1024) - off;
        for (int gs = 3; gs >= 1; --gs) {
            const int fl = ((nl << gs) + (nl >> 4) + 4) & ~3;
            if (APY_WAVES * fl * 4 <= budget) { P.tile_gs = gs; P.tile_floats = fl; off += APY_WAVES * fl * 4; break; }
        }
    }
    P.lds_bytes = off;
    // general kernel: frame, d / d' (hi + 1 floats), chunk totals, per-thread pick records (3 floats)
    off = frame_length * 4;
    P.off_d = off; off += ap_align16((hi + 1) * 4);
    P.off_tot = off; off += AP_BLOCK * 4;
    P.off_pick = off; off += 3 * AP_BLOCK * 4;
    if (!tw) P.lds_bytes = off;
    return AP_OK;
}

// persistent grid of the wave kernel: >= 2 frames per wave, as many workgroups per CU as the register
// allocation lets run at once (one wave of each per SIMD)
static inline int ap_yin_wave_grid(const ApYinParams &P) {
    const int64_t n_frames = P.n_clips * P.T;
    const int per_cu = P.n == 2048 ? APY_MIN_WAVES : APY_MIN_WAVES_1024;
    int64_t g = (n_frames + 2 * APY_WAVES - 1) / (2 * APY_WAVES);
    if (g > 256 * per_cu) g = 256 * per_cu;
    if (g < 1) g = 1;
    return (int)g;
}
static inline int ap_yin_general_grid(const ApYinParams &P) {
    const int64_t n_frames = P.n_clips * P.T;
    return (int)(n_frames < 256 * 32 ? n_frames : 256 * 32);
}

#ifdef AP_HOST_EMU
AP_DEV float apy_lane_get(float x, int src) { return emu_lane_perm(x, src); }
#else
AP_DEV float apy_lane_get(float x, int src) { return __shfl(x, src & 63, 64); }
#endif

// exclusive prefix sum over the lanes of a wave, in one fixed order (Hillis-Steele): the result does not depend
// on which wave or workgroup runs it
AP_DEV float apy_wave_excl_scan(float v, int lane) {
    float s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = apy_lane_get(s, lane - d);
        if (lane >= d) s += o;
    }
    const float e = apy_lane_get(s, lane - 1);
    return lane ? e : 0.0f;
}
AP_DEV float apy_wave_min(float v, int lane) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fminf(v, apy_lane_get(v, lane ^ m));
    return v;
}

// lag refinement and the stores of one frame; cm / cp: d' at chosen -+ 1 (unused at the ends of the range)
AP_DEV void apy_store_pick(const ApYinParams &P, int64_t f, int chosen, float cm, float c0, float cp) {
    float shift = 0.0f;
    if (chosen > P.lo && chosen < P.hi) {
        const float a = (cm + cp - 2.0f * c0) * 0.5f;
        const float b = (cp - cm) * 0.5f;
        if (fabsf(b) < fabsf(a)) shift = -b / (2.0f * a);
    }
    P.f0[f] = P.sr / ((float)chosen + shift);
    if (P.aper) P.aper[f] = c0;
}

// N = 2048: the 16 x 16 x 4 transform of kernels_wave.h (16 sample pairs and 16 lags per lane);
// N = 1024: the 8 x 8 x 8 transform of kernels_wave512.h (8 and 8).
template <int N, bool CURVE>
__global__ void __launch_bounds__(64 * APY_WAVES, (N == 2048 ? APY_MIN_WAVES : APY_MIN_WAVES_1024))
ap_yin_wave_kernel(ApYinParams P) {
    constexpr int NP = N / 128;             // sample pairs per lane = lags per lane
    constexpr int SH = N == 2048 ? 4 : 3;   // padded arrays: element q lives in float slot q + (q >> SH)
    constexpr int W = N / 2;
    constexpr int XC = N == 2048 ? APW_X_COMPLEX : APH_X_COMPLEX;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = AP_UNIFORM(tid >> 6);
    ap_float2 *X = reinterpret_cast<ap_float2 *>(ap_smem) + wave * XC;
    float *XF = reinterpret_cast<float *>(X);
    const ap_float2 *TW2 = reinterpret_cast<const ap_float2 *>(ap_smem + P.off_tw2);
    const ap_float2 *TW1 = reinterpret_cast<const ap_float2 *>(ap_smem + P.off_tw1);
    {
        ap_float2 *tw2 = reinterpret_cast<ap_float2 *>(ap_smem + P.off_tw2);
        ap_float2 *tw1 = reinterpret_cast<ap_float2 *>(ap_smem + P.off_tw1);
        if (N == 2048) {
            if (tid < 64)       // signs of the quad stage folded in, as in apw_fill_tables
                tw2[(tid >> 4) * 17 + (tid & 15)] = ap_scale(P.tw[32 * (tid >> 4) * (tid & 15)], ((tid >> 4) == 1 || (tid >> 4) == 2) ? -1.0f : 1.0f);
            for (int i = tid; i < 16 * 64; i += 64 * APY_WAVES) tw1[i] = P.tw[2 * (i & 63) * (i >> 6)];
        } else {                // as in ap_istft1024_wave_kernel
            for (int i = tid; i < 8 * 64; i += 64 * APY_WAVES) tw1[i] = P.tw[(2 * (i & 63) * (i >> 6)) & 1023];
            if (tid < 64) tw2[tid] = P.tw[16 * (tid >> 3) * (tid & 7)];
        }
    }
    const ApwLane lc = apw_lane_init(lane, TW2, P.tw);       // (N = 1024 uses tws0h, half, halfc of it)
    AP_LDS_BARRIER();                       // the only workgroup barrier

    const int64_t worker = (int64_t)blockIdx.x * APY_WAVES + wave;
    const int64_t n_workers = (int64_t)gridDim.x * APY_WAVES;
    const int64_t n_frames = P.n_clips * P.T;
    const int64_t f_lo = n_frames * worker / n_workers, f_hi = n_frames * (worker + 1) / n_workers;
    const int nl = P.hi - P.lo + 1;
    const int tau0 = NP * lane;             // this lane's lags: tau0 .. tau0 + NP - 1
    const int row = (NP + 1) * lane;        // float (or complex) slot of element NP * lane in the padded arrays

    // v[j] = packed samples lane + 64 j -> bins k = lane + 64 r (xk) and N / 2 - k (xm), zh = Z[N / 4]
    auto rfft_bins = [&](ap_float2 (&v)[NP], ap_float2 (&xk)[NP / 2], ap_float2 (&xm)[NP / 2], ap_float2 &zh) {
        if constexpr (N == 2048) {
            apw_forward<true, true>(v, X, TW1, lc);
            apw_split<true>(X, lc, xk, xm, zh);
        } else {
            aph_forward(v, X, TW1, TW2, lane);
            aph_split<true>(v, X, lc.tws0h, lane, xk, xm, zh);
        }
    };

    for (int64_t f = f_lo; f < f_hi; ++f) {
        const int64_t b = f / P.T;
        const int64_t t = f - b * P.T;
        const ApClip clip = ap_clip_make(P.y + b * P.L, P.L);
        const int64_t base = t * (int64_t)P.hop - P.pad;              // wave-uniform, even
        ap_float2 raw[NP];                                            // samples 2 p, 2 p + 1 of pair p = lane + 64 j
#pragma unroll
        for (int j = 0; j < NP; ++j) raw[j] = ap_clip_load2(clip, (int)(base + 2 * (lane + 64 * j)));

        // ---- e(0) + e(tau): prefix sums c[q] = sum_{i<q} x[i]^2, every lane 2 NP consecutive samples --------
        float ee[NP];
        {
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const int p = lane + 64 * j;
                X[p + (p >> SH)] = ap_mul2(raw[j], raw[j]);
            }
            AP_WAVE_SYNC();
            float run[2 * NP];
            float acc = 0.0f;
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const ap_float2 s = X[row + i];
                acc += s.x; run[2 * i] = acc;
                acc += s.y; run[2 * i + 1] = acc;
            }
            const float off = apy_wave_excl_scan(acc, lane);
            AP_WAVE_SYNC();
            if (lane == 0) XF[0] = 0.0f;
#pragma unroll
            for (int i = 0; i < 2 * NP; ++i) {
                const int q = 2 * NP * lane + 1 + i;
                XF[q + (q >> SH)] = off + run[i];
            }
            AP_WAVE_SYNC();
            const float e0 = XF[W + (W >> SH)];
#pragma unroll
            for (int i = 0; i < NP; ++i) ee[i] = e0 + (XF[W + (W >> SH) + row + i] - XF[row + i]);
            AP_WAVE_SYNC();
        }

        // ---- A = rfft(x), B = rfft(first half of x, zero-padded): bins lane + 64 r and N / 2 - (lane + 64 r) -
        ap_float2 v[NP], ak[NP / 2], am[NP / 2], bk[NP / 2], bm[NP / 2], azh, bzh;
#pragma unroll
        for (int j = 0; j < NP; ++j) v[j] = raw[j];
        rfft_bins(v, ak, am, azh);
#pragma unroll
        for (int j = 0; j < NP; ++j) v[j] = j < NP / 2 ? raw[j] : ap_mk(0.0f, 0.0f);
        rfft_bins(v, bk, bm, bzh);

        // ---- P = A conj(B), Hermitian merge and the inverse transform as in the irfft / ISTFT wave kernels ---
#pragma unroll
        for (int r = 0; r < NP / 2; ++r) {
            ap_float2 a_k = ap_mul_fw(ak[r], bk[r]), a_m = ap_mul_fw(am[r], bm[r]);
            if (r == 0 && lane == 0) { a_k.y = 0.0f; a_m.y = 0.0f; }      // DC and Nyquist are real
            const ap_float2 a = ap_add_conj(a_k, a_m);
            const ap_float2 d = ap_sub_conj(a_k, a_m);
            const ap_float2 w = r == 0 ? lc.tws0h
                                       : (N == 2048 ? ap_mul_bw_c(lc.tws0h, APW_C32(r), APW_S32(r))
                                                    : ap_mul_bw_c(lc.tws0h, APH_C16(r), APH_S16(r)));
            const ap_float2 o = ap_mul_bw(d, w);
            v[r] = ap_fma_sub_swap(a, lc.halfc, o);
            const int km = (N / 2 - (lane + 64 * r)) & (N / 2 - 1);
            if (!(r == 0 && lane == 0)) X[N == 2048 ? apw_zidx(km) : km - 256] = ap_fma_add_mi(a, lc.half, o);
        }
        if (lane == 0) {                    // the middle bin: A = conj(azh), B = conj(bzh)
            const ap_float2 ph = ap_mul_fw(azh, bzh);
            X[N == 2048 ? apw_zidx(APW_NC / 2) : 0] = ap_mk(ph.x, -ph.y);
        }
        AP_WAVE_SYNC();
#pragma unroll
        for (int j = NP / 2; j < NP; ++j) v[j] = X[N == 2048 ? apw_zidx(lane + 64 * j) : lane + 64 * (j - NP / 2)];
        AP_WAVE_SYNC();
        // r(2 m), r(2 m + 1) = conj(v) / (N / 2) for the sample pair m a register holds; lags below N / 2 only
        const float scale = 2.0f / (float)N;
        if constexpr (N == 2048) {
            apw_forward<false, true>(v, X, TW1, lc);
            AP_WAVE_SYNC();
            if (lc.qd < 2) {                // m = k1p + 16 cc + 256 qd
#pragma unroll
                for (int cc = 0; cc < 16; ++cc) {
                    const int q = 2 * (lc.k1p + 16 * cc + 256 * lc.qd);
                    XF[q + (q >> SH)] = v[cc].x * scale;
                    XF[q + (q >> SH) + 1] = -v[cc].y * scale;
                }
            }
        } else {
            aph_forward(v, X, TW1, TW2, lane);
            AP_WAVE_SYNC();
#pragma unroll
            for (int e = 0; e < NP / 2; ++e) {   // m = lane + 64 e
                const int q = 2 * (lane + 64 * e);
                XF[q + (q >> SH)] = v[e].x * scale;
                XF[q + (q >> SH) + 1] = -v[e].y * scale;
            }
        }
        AP_WAVE_SYNC();

        // ---- d, running sum, d' ---------------------------------------------------------------------------
        float dp[NP];
        {
            float run[NP];
            float acc = 0.0f;
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const int tau = tau0 + i;
                float d = fmaxf(ee[i] - 2.0f * XF[row + i], 0.0f);
                if (tau == 0 || tau > P.hi) d = 0.0f;
                dp[i] = d;
                acc += d;
                run[i] = acc;
            }
            AP_WAVE_SYNC();                 // the next frame's x^2 overwrite r
            const float off = apy_wave_excl_scan(acc, lane);
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const float s = off + run[i];
                const int tau = tau0 + i;
                dp[i] = (tau > 0 && s > 0.0f) ? dp[i] * (float)tau / s : 1.0f;
            }
        }
        if (CURVE) {
            const int gs = P.tile_gs;
            if (gs == 0) {                  // no room for a tile: every lane stores its own values
                float *dst = P.curve + b * (int64_t)nl * P.T + t;
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    const int tau = tau0 + i;
                    if (tau >= P.lo && tau <= P.hi) dst[(int64_t)(tau - P.lo) * P.T] = dp[i];
                }
                continue;
            }
            // tile [lag][frame mod G] (one pad float per 16 lags: the lanes' 16-lag blocks fall into different
            // banks); a run of frames of one clip leaves as G consecutive floats per lag, adjacent lanes adjacent
            // addresses
            float *TL = reinterpret_cast<float *>(ap_smem + P.off_tile) + wave * P.tile_floats;
            const int G = 1 << gs;
            const int slot = (int)t & (G - 1);
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const int r = tau0 + i - P.lo;
                if (r >= 0 && r < nl) TL[(r << gs) + (r >> 4) + slot] = dp[i];
            }
            if (slot == G - 1 || t == P.T - 1 || f == f_hi - 1) {
                // the columns this wave filled: back to the start of the group or of its own stretch
                const int c0 = slot - (int)(f - f_lo < slot ? f - f_lo : slot);
                AP_WAVE_SYNC();
                float *dst = P.curve + b * (int64_t)nl * P.T + (t - slot);
                for (int idx = lane; idx < (nl << gs); idx += 64) {
                    const int r = idx >> gs, col = idx & (G - 1);
                    if (col >= c0 && col <= slot) dst[(int64_t)r * P.T + col] = TL[(r << gs) + (r >> 4) + col];
                }
                AP_WAVE_SYNC();
            }
            continue;
        }

        // ---- pick: first trough below the threshold, else the first global minimum -------------------------
        const float prev = apy_lane_get(dp[NP - 1], lane - 1), next = apy_lane_get(dp[0], lane + 1);
        float cand = APY_BIG, mval = APY_BIG, mtau = APY_BIG;
#pragma unroll
        for (int i = NP - 1; i >= 0; --i) {   // downwards: the lowest lag wins, ties of the minimum included
            const int tau = tau0 + i;
            const float c = dp[i];
            const float left = tau > P.lo ? (i ? dp[i ? i - 1 : 0] : prev) : APY_BIG;
            const float right = tau < P.hi ? (i < NP - 1 ? dp[i < NP - 1 ? i + 1 : NP - 1] : next) : APY_BIG;
            const bool in = tau >= P.lo && tau <= P.hi;
            if (in && c < P.thr && c < left && c <= right) cand = (float)tau;
            if (in && c <= mval) { mval = c; mtau = (float)tau; }
        }
        float chosen_f = apy_wave_min(cand, lane);
        const float gmin = apy_wave_min(mval, lane);
        const float gtau = apy_wave_min(mval == gmin ? mtau : APY_BIG, lane);
        if (!(chosen_f < APY_BIG)) chosen_f = gtau;
        const int chosen = (int)chosen_f;
        if (chosen / NP == lane) {
            float cm = 0.0f, c0 = 0.0f, cp = 0.0f;
#pragma unroll
            for (int i = 0; i < NP; ++i)
                if (chosen % NP == i) {
                    cm = i ? dp[i ? i - 1 : 0] : prev;
                    c0 = dp[i];
                    cp = i < NP - 1 ? dp[i < NP - 1 ? i + 1 : NP - 1] : next;
                }
            apy_store_pick(P, f, chosen, cm, c0, cp);
        }
    }
}

// One workgroup per frame (grid-stride): the frame in LDS, d(tau) by direct sums, block scan, the same pick.
template <bool CURVE>
__global__ void __launch_bounds__(AP_BLOCK) ap_yin_general_kernel(ApYinParams P) {
    const int tid = threadIdx.x;
    float *xs = reinterpret_cast<float *>(ap_smem);                    // [n]
    float *ds = reinterpret_cast<float *>(ap_smem + P.off_d);          // [hi + 1]: d, then d'
    float *tot = reinterpret_cast<float *>(ap_smem + P.off_tot);       // [AP_BLOCK]
    float *pk = reinterpret_cast<float *>(ap_smem + P.off_pick);       // [AP_BLOCK][3]: trough lag, min, its lag
    const int n = P.n, W = P.n / 2, nt = P.hi + 1, nl = P.hi - P.lo + 1;
    const int chunk = (nt + AP_BLOCK - 1) / AP_BLOCK;                  // consecutive lags per thread
    const int c_lo = tid * chunk < nt ? tid * chunk : nt;
    const int c_hi = c_lo + chunk < nt ? c_lo + chunk : nt;
    const int64_t n_frames = P.n_clips * P.T;
    for (int64_t f = blockIdx.x; f < n_frames; f += gridDim.x) {
        const int64_t b = f / P.T;
        const int64_t t = f - b * P.T;
        const float *yb = P.y + b * P.L;
        const int64_t base = t * (int64_t)P.hop - P.pad;
        for (int i = tid; i < n; i += AP_BLOCK) {
            const int64_t p = base + i;
            xs[i] = (p >= 0 && p < P.L) ? yb[p] : 0.0f;                // constant padding
        }
        AP_LDS_BARRIER();
        for (int tau = tid; tau < nt; tau += AP_BLOCK) {
            float acc = 0.0f;
            for (int j = 0; j < W; ++j) {
                const float df = xs[j] - xs[j + tau];
                acc += df * df;
            }
            ds[tau] = acc;                                             // d(0) = 0 exactly
        }
        AP_LDS_BARRIER();
        {
            float acc = 0.0f;
            for (int tau = c_lo; tau < c_hi; ++tau) acc += ds[tau];
            tot[tid] = acc;
        }
        AP_LDS_BARRIER();
        if (tid == 0) {                                                // exclusive scan of the chunk totals
            float acc = 0.0f;
            for (int i = 0; i < AP_BLOCK; ++i) { const float v = tot[i]; tot[i] = acc; acc += v; }
        }
        AP_LDS_BARRIER();
        {
            float acc = tot[tid];
            for (int tau = c_lo; tau < c_hi; ++tau) {
                const float d = ds[tau];
                acc += d;
                ds[tau] = (tau > 0 && acc > 0.0f) ? d * (float)tau / acc : 1.0f;
            }
        }
        AP_LDS_BARRIER();
        if (CURVE) {
            float *dst = P.curve + b * (int64_t)nl * P.T + t;
            for (int i = tid; i < nl; i += AP_BLOCK) dst[(int64_t)i * P.T] = ds[P.lo + i];
        } else {
            float cand = APY_BIG, mval = APY_BIG, mtau = APY_BIG;
            for (int tau = c_hi - 1; tau >= c_lo; --tau) {
                if (tau < P.lo || tau > P.hi) continue;
                const float c = ds[tau];
                const float left = tau > P.lo ? ds[tau - 1] : APY_BIG;
                const float right = tau < P.hi ? ds[tau + 1] : APY_BIG;
                if (c < P.thr && c < left && c <= right) cand = (float)tau;
                if (c <= mval) { mval = c; mtau = (float)tau; }
            }
            pk[3 * tid] = cand; pk[3 * tid + 1] = mval; pk[3 * tid + 2] = mtau;
            AP_LDS_BARRIER();
            if (tid == 0) {
                float ch = APY_BIG, gm = APY_BIG, gt = APY_BIG;
                for (int i = 0; i < AP_BLOCK; ++i) {                   // chunks are in lag order: the first wins
                    if (!(ch < APY_BIG) && pk[3 * i] < APY_BIG) ch = pk[3 * i];
                    if (pk[3 * i + 1] < gm) { gm = pk[3 * i + 1]; gt = pk[3 * i + 2]; }
                }
                const int chosen = (int)(ch < APY_BIG ? ch : gt);
                apy_store_pick(P, f, chosen, ds[chosen - 1], ds[chosen], chosen < P.hi ? ds[chosen + 1] : 0.0f);
            }
        }
        AP_LDS_BARRIER();                                              // ds / xs are rewritten by the next frame
    }
}
