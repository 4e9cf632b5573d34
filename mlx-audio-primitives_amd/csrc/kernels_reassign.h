// reassigned_spectrogram (reassign.py; the definition of librosa 0.10, restated in DESIGN.md 9.15 and tests/reassign_ref.py).
//
// Three STFTs of the same frames, with the window h, its cyclic central difference dh and its time-weighted copy th:
//   mags  = |S_h|
//   freqs = k sr / n - Im(S_dh / S_h) sr / (2 pi)
//   times = (t hop + (center ? 0 : n / 2)) / sr + Re(S_th / S_h) / sr
// then NaN where mags < sqrt(ref_power) or S_h = 0, the optional fill (bin frequency / frame time) and the optional clip
// (freqs to [0, sr / 2], times to [0, L / sr]; NaN stays NaN).  The three spectra never reach HBM: a frame's samples are
// read once, transformed once per requested window on chip, and only the float planes are written (12 bytes per bin).
//
// The quotients are S_x conj(S_h) / |S_h|^2 with one reciprocal per bin; the affine step that turns a quotient into Hz or
// seconds runs in float64 (17 operations per lane and plane, nothing next to a transform) and is rounded to float32
// once, so a value carries the error of its quotient plus half an ulp.  |S_h|^2 = 0 (S_h = 0, or so small that its
// square underflows float32: |S_h| < 1e-22) counts as "no energy": NaN, where NumPy gives an infinity for x / 0.
//
// ap_reassign2048_wave_kernel (n_fft = 2048).  The workgroup shape of ap_stft2048_wave_kernel: 8 waves take the 8
//   consecutive frames of a group, one each; a workgroup walks a contiguous stretch of the (clip, group) stream.  A wave
//   loads its frame's 32 samples per lane once (bounds-checked buffer loads; PADGEN = 1: index-remapped loads for the
//   frames that overlap a clip boundary) and keeps them in registers across up to three apw_forward / apw_split runs:
//   the split bins of S_h (17 complex per lane) and their reciprocals stay in registers while S_dh and S_th are formed
//   and reduced to one float per bin each.  A plane that is not requested costs no transform (RF / RT are template
//   arguments).  The next group's samples are fetched under the store phase (PADGEN = 0).
//   Store granularity: a group is 8 frames, so a row segment is a 32-byte run.  Gathering 16 frames before a store
//   needs the first 8 frames' results (3 x 1025 x 8 floats = 98 KB) parked while the exchange buffers (82 KB) and the
//   tables (33 KB) are in use: over the 160 KB of a CU; parking them in registers is 51 VGPRs per lane across a whole
//   transform in a kernel that already uses all 256.  So the runs stay at 32 bytes, the sector size of the memory system,
//   and the stretch order lets the two runs of a 64-byte sector meet in L2 (the same CU writes them back to back).
//   The transposition goes through the exchange buffers, which are idle once the last split has read them: two
//   staging buffers of 1025 rows x 9 floats (36.9 KB each, 9 = 8 frames + 1 pad: conflict-free writes) live on top of
//   them, plane after plane, one LDS-only barrier per plane.  No LDS beyond the STFT kernel's but the two extra windows.
//
// ap_reassign_tile_kernel (every other n_fft the FFT plan serves, even or odd).  A workgroup of 256 threads owns one clip
//   and G consecutive frames: it stages n_win G rows (n_win = 1 + requested planes; row w G + g = frame g times window
//   w) from ONE read of the samples, runs ap_fft_tile once over all rows, and an epilogue thread takes bin k of frame g
//   (frame index fastest: adjacent lanes write adjacent frames of one row), splits the rows of that frame
//   (ap_rfft_split for even n) and does the arithmetic above.  G comes from the LDS budget (ap_prepare_reassign).
//
// Fixed order of operations, no atomics: the same bits on every run, and for a clip alone or inside a batch.
#pragma once
#include <cmath>

#include "ap_launch.h"
#include "kernels_wave.h"

#define AP_REASSIGN_FREQ 1      // flags of ap_reassign_f32 (include/audioprims.h)
#define AP_REASSIGN_TIME 2
#define AP_REASSIGN_FILL 4
#define AP_REASSIGN_CLIP 8

#define APR_ROW 9                                  // floats per staging row: 8 frames + 1 pad
#define APR_STAGE_FLOATS (1028 * APR_ROW)          // one staging buffer: 1025 rows, rounded to 16 bytes
#define APR_TILE_BUDGET (80 * 1024)                // tile kernel: two workgroups per CU
static_assert(2 * APR_STAGE_FLOATS * 4 <= APS_WAVES * APW_X_COMPLEX * 8, "both staging buffers fit over the exchange buffers");

struct ApReassignParams {
    const float *y;                  // (B, L)
    const float *win_h, *win_dh, *win_th;   // (n_fft) each; dh / th NULL when their plane is off
    const ap_float2 *tw;             // (n_fft)
    float *freqs, *times, *mags;     // (B, F, out_rs); freqs / times NULL when their plane is off
    int64_t L, T, B, out_rs, groups_per_clip, n_groups;
    double bin_hz, f_scale, inv_sr, t_off;   // sr / n, sr / (2 pi), 1 / sr, center ? 0 : n / 2
    float thr, f_max, t_max;         // sqrt(ref_power), sr / 2, L / sr
    int hop, pad, pad_mode, flags, n_bins;
    int wave, padgen;                // 1: the n_fft = 2048 wave kernel (padgen: its index-remapped loader)
    int n_win, G, fstride, lds_bytes;
    int off_tw2, off_tw1, off_win;   // wave kernel: LDS carve-up; the three windows follow each other at off_win
    ApFftPlan plan;
};

// Validation and launch geometry of ap_reassign_f32.
static inline int ap_prepare_reassign(ApReassignParams &P, const float *y, int64_t B, int64_t L, int n_fft, int hop, const float *win_h,
                                      const float *win_dh, const float *win_th, const float *tw, int center, int pad_mode, int64_t T,
                                      double sr, double ref_power, int flags, float *freqs, float *times, float *mags, int64_t out_rs) {
    const bool rf = (flags & AP_REASSIGN_FREQ) != 0, rt = (flags & AP_REASSIGN_TIME) != 0;
    if (flags & ~15) AP_FAIL(AP_ERR_INVALID, "reassign: unknown flags %d", flags);
    if (!rf && !rt) AP_FAIL(AP_ERR_INVALID, "reassign_frequencies or reassign_times must be True");
    if (!y || !win_h || !tw || !mags) AP_FAIL(AP_ERR_INVALID, "reassign: NULL buffer");
    if (rf != (freqs != nullptr) || rf != (win_dh != nullptr)) AP_FAIL(AP_ERR_INVALID, "reassign: freqs and win_dh go with the frequency flag");
    if (rt != (times != nullptr) || rt != (win_th != nullptr)) AP_FAIL(AP_ERR_INVALID, "reassign: times and win_th go with the time flag");
    if (n_fft <= 0) AP_FAIL(AP_ERR_INVALID, "n_fft must be positive, got %d", n_fft);
    if (hop <= 0) AP_FAIL(AP_ERR_INVALID, "hop_length must be positive, got %d", hop);
    if (B <= 0 || L <= 0) AP_FAIL(AP_ERR_INVALID, "reassign: signal must be non-empty");
    if (!(sr > 0.0) || !std::isfinite(sr)) AP_FAIL(AP_ERR_INVALID, "sr must be positive, got %g", sr);
    if (!(ref_power >= 0.0) || !std::isfinite(ref_power)) AP_FAIL(AP_ERR_INVALID, "ref_power must be non-negative, got %g", ref_power);
    if (pad_mode < AP_PAD_CONSTANT || pad_mode > AP_PAD_REFLECT) AP_FAIL(AP_ERR_INVALID, "Unknown pad_mode. Supported: reflect, constant, edge");
    const int pad = center ? n_fft / 2 : 0;
    if (center && pad_mode == AP_PAD_REFLECT && pad > L - 1) AP_FAIL(AP_ERR_INVALID, "reflect padding requires n_fft//2 <= signal_length - 1");
    const int64_t Texp = ap_n_frames(L, n_fft, hop, center);
    if (Texp <= 0)
        AP_FAIL(AP_ERR_INVALID, "Signal length (%lld) must be >= frame_length (%d). Consider padding the signal.", (long long)(L + 2 * pad), n_fft);
    if (T != Texp) AP_FAIL(AP_ERR_INVALID, "reassign: n_frames mismatch (got %lld, expected %lld)", (long long)T, (long long)Texp);
    if (out_rs < T) AP_FAIL(AP_ERR_INVALID, "reassign: out_row_stride (%lld) must be >= T = %lld", (long long)out_rs, (long long)T);
    if (ap_make_plan(n_fft, &P.plan) != 0) AP_FAIL(AP_ERR_UNSUPPORTED, "n_fft=%d: cannot build FFT plan", n_fft);
    P.n_bins = n_fft / 2 + 1;
    if ((double)B * (double)P.n_bins * (double)out_rs * 4.0 > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "reassign: more than 2^63 bytes");
    if ((double)T * (double)hop > 9.0e15) AP_FAIL(AP_ERR_UNSUPPORTED, "reassign: clip too long");
    P.y = y; P.win_h = win_h; P.win_dh = win_dh; P.win_th = win_th; P.tw = reinterpret_cast<const ap_float2 *>(tw);
    P.freqs = freqs; P.times = times; P.mags = mags;
    P.L = L; P.T = T; P.B = B; P.out_rs = out_rs;
    P.bin_hz = sr / (double)n_fft;
    P.f_scale = sr / 6.283185307179586476925;
    P.inv_sr = 1.0 / sr;
    P.t_off = center ? 0.0 : (double)(n_fft / 2);
    P.thr = (float)std::sqrt(ref_power);
    P.f_max = (float)(0.5 * sr);
    P.t_max = (float)((double)L / sr);
    P.hop = hop; P.pad = pad; P.pad_mode = pad_mode; P.flags = flags;
    P.n_win = 1 + (rf ? 1 : 0) + (rt ? 1 : 0);
    P.wave = 0; P.padgen = 0; P.G = 0; P.fstride = 0; P.off_tw2 = P.off_tw1 = P.off_win = 0;
    if (n_fft == 2 * APW_NC && L <= (1 << 28)) {         // 32-bit sample offsets in the bounds-checked loads
        P.wave = 1;
        P.padgen = ap_clip_loads_ok(P) ? 0 : 1;
        P.groups_per_clip = (T + APS_WAVES - 1) / APS_WAVES;
        if ((double)P.groups_per_clip * (double)B > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "reassign: too many groups");
        P.n_groups = P.groups_per_clip * B;
        int off = APS_WAVES * APW_X_COMPLEX * (int)sizeof(ap_float2);
        P.off_tw2 = off; off += APW_TW2_COMPLEX * (int)sizeof(ap_float2);
        P.off_tw1 = off; off += 16 * 64 * (int)sizeof(ap_float2);
        P.off_win = off; off += 3 * APW_NC * (int)sizeof(ap_float2);
        P.lds_bytes = off;
        return AP_OK;
    }
    P.fstride = P.plan.nc + 1;
    const int64_t per_frame = (int64_t)P.n_win * 2 * P.fstride * (int64_t)sizeof(ap_float2);     // both ping-pong buffers, every window
    if (per_frame > AP_LDS_MAX)
        AP_FAIL(AP_ERR_UNSUPPORTED, "n_fft=%d: %d windowed frames do not fit the %d KiB LDS of one CU", n_fft, P.n_win, AP_LDS_MAX / 1024);
    int64_t G = APR_TILE_BUDGET / per_frame;
    if (G < 1) G = 1;
    if (G > AP_MAX_G) G = AP_MAX_G;
    if (G > T) G = T;
    P.G = (int)G;
    P.lds_bytes = (int)(per_frame * G);
    P.groups_per_clip = (T + G - 1) / G;
    if ((double)P.groups_per_clip * (double)B > (double)kApMaxGrid) AP_FAIL(AP_ERR_UNSUPPORTED, "reassign: grid too large");
    P.n_groups = P.groups_per_clip * B;
    return AP_OK;
}

static inline int ap_reassign_wave_grid(const ApReassignParams &P) { return (int)(P.n_groups < 256 ? P.n_groups : 256); }   // one workgroup per CU

// ---- the arithmetic both kernels share ---------------------------------------------------------------------------
AP_DEV float apr_power(ap_float2 h) { return fmaf(h.y, h.y, h.x * h.x); }
// Im and Re of x conj(h) / |h|^2, inv = 1 / |h|^2
AP_DEV float apr_quot_im(ap_float2 x, ap_float2 h, float inv) { return fmaf(x.y, h.x, -(x.x * h.y)) * inv; }
AP_DEV float apr_quot_re(ap_float2 x, ap_float2 h, float inv) { return fmaf(x.x, h.x, x.y * h.y) * inv; }

// quotient -> Hz / seconds: `centre` is the bin frequency (the frame time), q the quotient already scaled to the unit
AP_DEV float apr_finish(double centre, double q, bool bad, bool fill, bool clip, float hi) {
    float v = (float)(centre + q);
    if (bad) v = fill ? (float)centre : __builtin_nanf("");
    if (clip) v = v < 0.0f ? 0.0f : (v > hi ? hi : v);          // comparisons with NaN are false: NaN stays
    return v;
}

template <int PADGEN, bool RF, bool RT>
__global__ void __launch_bounds__(64 * APS_WAVES, 2) ap_reassign2048_wave_kernel(ApReassignParams P) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = AP_UNIFORM(tid >> 6);
    ap_float2 *X = reinterpret_cast<ap_float2 *>(ap_smem) + wave * APW_X_COMPLEX;
    const ap_float2 *TW2 = reinterpret_cast<const ap_float2 *>(ap_smem + P.off_tw2);
    const ap_float2 *TW1 = reinterpret_cast<const ap_float2 *>(ap_smem + P.off_tw1);
    const ap_float2 *WINH = reinterpret_cast<const ap_float2 *>(ap_smem + P.off_win);          // 1024 sample pairs each
    const ap_float2 *WINDH = WINH + APW_NC, *WINTH = WINH + 2 * APW_NC;
    float *stage0 = reinterpret_cast<float *>(ap_smem), *stage1 = stage0 + APR_STAGE_FLOATS;   // over the exchange buffers
    {
        ap_float2 *win = reinterpret_cast<ap_float2 *>(ap_smem + P.off_win);
        apw_fill_tables(reinterpret_cast<ap_float2 *>(ap_smem + P.off_tw2), reinterpret_cast<ap_float2 *>(ap_smem + P.off_tw1),
                        win, P.tw, P.win_h, tid, 64 * APS_WAVES);
        for (int i = tid; i < APW_NC; i += 64 * APS_WAVES) {
            if (RF) win[APW_NC + i] = reinterpret_cast<const ap_float2 *>(P.win_dh)[i];
            if (RT) win[2 * APW_NC + i] = reinterpret_cast<const ap_float2 *>(P.win_th)[i];
        }
    }
    const ApwLane lc = apw_lane_init(lane, TW2, P.tw);
    AP_LDS_BARRIER();

    const int F = APW_NC + 1;
    const bool fill = (P.flags & AP_REASSIGN_FILL) != 0, clip = (P.flags & AP_REASSIGN_CLIP) != 0;
    ap_float2 raw[16];
    auto load_frame = [&](int64_t group) {
        const int64_t b = group / P.groups_per_clip;
        const int64_t t = (group - b * P.groups_per_clip) * APS_WAVES + wave;
        const float *yb = P.y + b * P.L;
        const ApClip cl = ap_clip_make(yb, P.L);
        const int64_t base = t * (int64_t)P.hop - P.pad;          // wave-uniform
        // frames beyond T read past the clip: zeros (never stored).  Edge / reflect padding only touches the frames
        // that overlap a clip boundary.
        const bool inside = !PADGEN || t >= P.T || (base >= 0 && base + 2 * APW_NC <= P.L);
        if (inside) {
#pragma unroll
            for (int j = 0; j < 16; ++j) raw[j] = ap_clip_load2(cl, (int)(base + 2 * (lane + 64 * j)));
        } else {
            int lane_p = lane;
            AP_PIN(lane_p);              // 64-bit sample offsets made here, not carried through the group loop
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int64_t p = base + 2 * (lane_p + 64 * j);
                raw[j] = ap_mk(ap_load_padded(yb, P.L, p, P.pad_mode), ap_load_padded(yb, P.L, p + 1, P.pad_mode));
            }
        }
    };
    // one windowed transform of the frame in `raw`: bins lane + 64 r in xk, 1024 - lane - 64 r in xm, bin 512 in xh
    auto transform = [&](const ap_float2 *WIN, ap_float2 (&xk)[8], ap_float2 (&xm)[8], ap_float2 &xh) {
        ap_float2 v[16];
        {
            ap_float2 w[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) w[j] = WIN[lane + 64 * j];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = ap_mul2(raw[j], w[j]);
        }
        AP_SCHED_FENCE();
        apw_forward<true, true>(v, X, TW1, lc);
        ap_float2 zh;
        apw_split<true>(X, lc, xk, xm, zh);
        xh = ap_mk(zh.x, -zh.y);                                  // X[512] = conj Z[512]
        AP_SCHED_FENCE();
    };
    // a plane of the group, transposed through LDS: every wave leaves its frame as a column, then 8 adjacent lanes
    // write the 8 frames of one row
    auto stage = [&](float *buf, const float (&val)[17]) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            buf[(lane + 64 * r) * APR_ROW + wave] = val[r];
            buf[(APW_NC - lane - 64 * r) * APR_ROW + wave] = val[8 + r];
        }
        if (lane == 0) buf[(APW_NC / 2) * APR_ROW + wave] = val[16];
    };
    auto flush = [&](const float *buf, float *ob, int trem) {
        for (int e = tid; e < F * APS_WAVES; e += 64 * APS_WAVES) {
            const int row = e >> 3, f = e & 7;
            if (f < trem) ob[(int64_t)row * P.out_rs + f] = buf[row * APR_ROW + f];
        }
    };

    // every workgroup owns a contiguous stretch of the (clip, group) stream: the 32-byte runs of consecutive groups are
    // written back to back by the same CU
    const int64_t g_lo = P.n_groups * (int64_t)blockIdx.x / gridDim.x;
    const int64_t g_hi = P.n_groups * ((int64_t)blockIdx.x + 1) / gridDim.x;
    // the edge / reflect instantiation does not prefetch: with both loaders live across the store phase it spills
    if (!PADGEN && g_lo < g_hi) load_frame(g_lo);
    for (int64_t group = g_lo; group < g_hi; ++group) {
        if (PADGEN) load_frame(group);
        const int64_t b = group / P.groups_per_clip;
        const int64_t t0 = (group - b * P.groups_per_clip) * APS_WAVES;
        const int trem = (int)(P.T - t0 < APS_WAVES ? P.T - t0 : APS_WAVES);
        const int64_t obase = b * (int64_t)F * P.out_rs + t0;

        ap_float2 hk[8], hm[8], hh;
        float inv[17], fq[17], tq[17];
        transform(WINH, hk, hm, hh);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            inv[r] = 1.0f / apr_power(hk[r]);
            inv[8 + r] = 1.0f / apr_power(hm[r]);
        }
        inv[16] = 1.0f / apr_power(hh);
        if (RF) {
            ap_float2 xk[8], xm[8], xh;
            transform(WINDH, xk, xm, xh);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                fq[r] = apr_quot_im(xk[r], hk[r], inv[r]);
                fq[8 + r] = apr_quot_im(xm[r], hm[r], inv[8 + r]);
            }
            fq[16] = apr_quot_im(xh, hh, inv[16]);
        }
        if (RT) {
            ap_float2 xk[8], xm[8], xh;
            transform(WINTH, xk, xm, xh);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                tq[r] = apr_quot_re(xk[r], hk[r], inv[r]);
                tq[8 + r] = apr_quot_re(xm[r], hm[r], inv[8 + r]);
            }
            tq[16] = apr_quot_re(xh, hh, inv[16]);
        }
        // ---- threshold, fill, clip: the lane's 17 bins of frame t0 + wave ----
        float mg[17];
        int lane_k = lane;
        AP_PIN(lane_k);                  // the bin frequencies are computed here, every time: hoisted out of the group loop
                                         // they would hold 34 registers across the transforms
        const double frame_pos = (double)((t0 + wave) * (int64_t)P.hop) + P.t_off;
#pragma unroll
        for (int s = 0; s < 17; ++s) {
            const int k = s < 8 ? lane_k + 64 * s : (s < 16 ? APW_NC - lane_k - 64 * (s - 8) : APW_NC / 2);
            const ap_float2 h = s < 8 ? hk[s] : (s < 16 ? hm[s - 8] : hh);
            mg[s] = sqrtf(apr_power(h));
            const bool bad = !(mg[s] > 0.0f) || mg[s] < P.thr;
            if (RF) fq[s] = apr_finish((double)k * P.bin_hz, -(double)fq[s] * P.f_scale, bad, fill, clip, P.f_max);
            if (RT) tq[s] = apr_finish(frame_pos * P.inv_sr, (double)tq[s] * P.inv_sr, bad, fill, clip, P.t_max);
        }
        AP_SCHED_FENCE();
        if (!PADGEN && group + 1 < g_hi) load_frame(group + 1);   // the next group's samples, in flight during the stores
        AP_SCHED_FENCE();
        AP_LDS_BARRIER();                                          // every wave is done with its exchange buffer
        stage(stage0, mg);
        AP_LDS_BARRIER();
        flush(stage0, P.mags + obase, trem);
        if (RF) {
            stage(stage1, fq);
            AP_LDS_BARRIER();
            flush(stage1, P.freqs + obase, trem);
        }
        if (RT) {
            float *buf = RF ? stage0 : stage1;                     // RF: everyone left stage0 before the barrier above
            stage(buf, tq);
            AP_LDS_BARRIER();
            flush(buf, P.times + obase, trem);
        }
        AP_LDS_BARRIER();                                          // the staging buffers become exchange buffers again
    }
}

AP_KERNEL void __launch_bounds__(AP_BLOCK) ap_reassign_tile_kernel(ApReassignParams P) {
    const ApFftPlan &pl = P.plan;
    const int G = P.G, fstride = P.fstride, nc = pl.nc, NW = P.n_win, rows = NW * G;
    ap_float2 *bufA = reinterpret_cast<ap_float2 *>(ap_smem);
    ap_float2 *bufB = bufA + (size_t)rows * fstride;
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int64_t b = blockIdx.x / P.groups_per_clip;
    const int64_t t0 = (blockIdx.x - b * P.groups_per_clip) * G;
    const int Gt = (int)((P.T - t0) < G ? (P.T - t0) : G);
    const float *yb = P.y + b * P.L;
    const bool rf = (P.flags & AP_REASSIGN_FREQ) != 0, rt = (P.flags & AP_REASSIGN_TIME) != 0;
    const bool fill = (P.flags & AP_REASSIGN_FILL) != 0, clip = (P.flags & AP_REASSIGN_CLIP) != 0;
    const float *win[3] = {P.win_h, rf ? P.win_dh : P.win_th, P.win_th};     // row block w uses win[w]

    // ---- load: virtual pad + frame, one read of the samples for every window; row w G + g ----
    for (int item = tid; item < G * nc; item += nthreads) {
        const int g = item / nc;
        const int c = item - g * nc;
        float s0 = 0.0f, s1 = 0.0f;
        const int i0 = pl.even ? 2 * c : c;
        if (g < Gt) {
            const int64_t base = (t0 + g) * (int64_t)P.hop - P.pad;
            s0 = ap_load_padded(yb, P.L, base + i0, P.pad_mode);
            if (pl.even) s1 = ap_load_padded(yb, P.L, base + i0 + 1, P.pad_mode);
        }
        for (int w = 0; w < NW; ++w)
            bufA[(w * G + g) * fstride + c] = ap_mk(win[w][i0] * s0, pl.even ? win[w][i0 + 1] * s1 : 0.0f);
    }
    AP_LDS_BARRIER();

    const ap_float2 *Z = ap_fft_tile(bufA, bufB, pl, P.tw, rows, fstride, tid, nthreads);
    const int F = P.n_bins;
    for (int item = tid; item < F * G; item += nthreads) {
        const int k = item / G;
        const int g = item - k * G;
        if (g >= Gt) continue;
        auto bin = [&](int w) {
            const ap_float2 *Zr = Z + (w * G + g) * fstride;
            return pl.even ? ap_rfft_split(Zr, nc, k, P.tw) : Zr[k];
        };
        const ap_float2 h = bin(0);
        const float inv = 1.0f / apr_power(h), mag = sqrtf(apr_power(h));
        const bool bad = !(mag > 0.0f) || mag < P.thr;
        const int64_t o = (b * F + k) * P.out_rs + t0 + g;
        P.mags[o] = mag;
        if (rf) {
            const float q = apr_quot_im(bin(1), h, inv);
            P.freqs[o] = apr_finish((double)k * P.bin_hz, -(double)q * P.f_scale, bad, fill, clip, P.f_max);
        }
        if (rt) {
            const float q = apr_quot_re(bin(NW - 1), h, inv);
            const double frame_pos = (double)((t0 + g) * (int64_t)P.hop) + P.t_off;
            P.times[o] = apr_finish(frame_pos * P.inv_sr, (double)q * P.inv_sr, bad, fill, clip, P.t_max);
        }
    }
}
