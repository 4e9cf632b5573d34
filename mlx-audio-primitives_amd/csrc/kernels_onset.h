// Onset strength (spectral flux) and peak picking (onset.py: onset_strength, peak_pick, onset_detect; the definitions
// of librosa.onset.onset_strength, librosa.util.peak_pick and librosa.onset.onset_detect).
//
// ap_onset_strength_kernel.  For a log-power spectrogram S (M, T) of one clip, lag >= 1 and 1 <= max_size <= 255:
//   R[m,t]  = ref[m,t] when a reference is given, else max S[r(j, M), t] over j in [m - max_size/2, m + (max_size-1)/2]
//             (r: SciPy's mode="reflect", d c b a | a b c d | d c b a: scipy.ndimage.maximum_filter1d along m;
//             max_size = 1: S itself)
//   flux[u] = (1 / M) sum_m max(0, S[m, u + lag] - R[m, u]),  0 <= u < T - lag
//   out[t]  = flux[t - shift] for shift <= t < T, 0 for t < shift    (shift >= lag: every read stays inside the row)
// DB = true: S holds power and every value is converted on load, max(coef log10(max(s, amin) / ref), floor) with the
// helpers ap_to_db_kernel uses (ap_db.h), so the dB array never exists in memory and the result has the
// bits of the two-step route.  A reference array is taken as it is in both modes.
//
//   A 256-thread workgroup owns 64 OUTPUT frames of one clip; lane = frame, so a wave reads 64 consecutive floats of a
//   row per instruction and the same launch writes the `shift` leading zeros.  Wave w owns the rows w, w + 4, ... and
//   adds their terms in ascending order; the four partial sums go through LDS and are added as ((p0 + p1) + p2) + p3,
//   then divided by M once: no atomics, and a result depends on its clip's values and t only.
//   max_size == 1 or a reference: nothing is staged, both operands come straight from memory (the second read of a
//   line hits the cache).  max_size > 1: the rows are walked in chunks of 64; a chunk's 64 + max_size - 1 reflected
//   rows of the R column are staged in LDS (dB applied once), the window maximum is max_size conflict-free LDS reads.
//
// ap_peak_pick_kernel.  One workgroup per row x (T <= 16384), everything in one launch:
//   row minimum / maximum / finiteness; x = (x - min) / (max - min + FLT_MIN) when `normalize`; candidates
//     x[n] == max x[max(0, n - pre_max) : min(n + post_max, T)]  and
//     x[n] >= mean x[max(0, n - pre_avg) : min(n + post_avg, T)] + delta     (float32 sum in index order / count)
//   (a NaN anywhere in a window makes the frame no candidate, as NumPy's max and mean do); the candidates as one bit
//   mask per 64 frames; the greedy pass (a candidate is kept iff it lies more than `wait` frames after the last kept
//   one) by one thread over the set bits only; `backtrack`: every kept frame n moves to the largest k <= n that is 0
//   or has e[k] <= e[k-1] and e[k] < e[k+1], 1 <= k <= T - 2 (e = `energy`, or the values the candidates saw);
//   the mask (bytes) and its population count per row.  `guard` (onset_detect): a row that is all zero or holds a
//   non-finite value yields no frame.
#pragma once
#include "ap_db.h"
#include "ap_launch.h"
#include "fft_lds.h"

extern __shared__ __attribute__((aligned(16))) char ap_smem[];

#define APON_WAVES 4            // waves per workgroup; wave w owns the rows w, w + 4, ...
#define APON_TT 64              // output frames per tile: the lanes of a wave
#define APON_MC 64              // rows per staged chunk (a multiple of APON_WAVES: a row's wave does not depend on the chunk)
#define APON_KMAX 255
#define APPK_BLOCK 256
#define APPK_TMAX 16384
#define APPK_FLT_MIN 1.17549435e-38f

struct ApOnsetParams {
    const float *S, *ref;       // (B, M, rs_in), (B, M, rs_ref) or NULL
    float *out;                 // (B, rs_out)
    int64_t B, rs_in, rs_ref, rs_out, n_tiles;
    int M, T, lag, max_size, shift, db, staged, n_tt;
    int off_part, lds_bytes;
    ApDbParams D;
};

static inline bool ap_onset_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

// Validation and launch geometry of ap_onset_strength_f32 (and of its emulator twin).
static inline int ap_prepare_onset_strength(ApOnsetParams &P, const float *S, int64_t B, int64_t M, int64_t T, int64_t rs_in,
                                            const float *ref, int64_t rs_ref, int lag, int max_size, int shift, int db_mode,
                                            float db_coef, float db_amin, float db_ref, float db_top_db,
                                            const unsigned *smax_key, float *out, int64_t rs_out) {
    if (!S || !out) AP_FAIL(AP_ERR_INVALID, "onset_strength: NULL buffer");
    if (B <= 0 || M <= 0 || T <= 0) AP_FAIL(AP_ERR_INVALID, "onset_strength: S must be non-empty, got (%lld, %lld, %lld)", (long long)B, (long long)M, (long long)T);
    if (lag < 1) AP_FAIL(AP_ERR_INVALID, "lag must be a positive integer, got %d", lag);
    if (max_size < 1 || max_size > APON_KMAX) AP_FAIL(AP_ERR_INVALID, "max_size must be an integer in 1 .. 255, got %d", max_size);
    if (shift < lag) AP_FAIL(AP_ERR_INVALID, "onset_strength: shift (%d) must be >= lag (%d)", shift, lag);
    if (rs_in < T || rs_out < T || (ref && rs_ref < T))
        AP_FAIL(AP_ERR_INVALID, "onset_strength: row strides (%lld, %lld, %lld) must be >= T = %lld", (long long)rs_in, (long long)rs_ref, (long long)rs_out, (long long)T);
    if (db_mode && db_top_db >= 0.0f && !smax_key) AP_FAIL(AP_ERR_INVALID, "onset_strength: top_db needs the key of max(S)");
    // 32-bit (m, t) and reflect arithmetic; element offsets are 64-bit
    if (M > (1 << 28) || T > (1 << 28)) AP_FAIL(AP_ERR_UNSUPPORTED, "onset_strength: M and T must be <= 2^28");
    if (lag > (1 << 29) || shift > (1 << 29)) AP_FAIL(AP_ERR_UNSUPPORTED, "onset_strength: lag and shift must be <= 2^29");
    if (rs_in > ((int64_t)1 << 40) || rs_ref > ((int64_t)1 << 40) || rs_out > ((int64_t)1 << 40) || B > ((int64_t)1 << 40))
        AP_FAIL(AP_ERR_UNSUPPORTED, "onset_strength: extents too large");
    if ((double)B * (double)M * (double)(rs_in > rs_ref ? rs_in : rs_ref) * 4.0 > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "onset_strength: more than 2^63 bytes");
    // exact extents: the padding behind the last row belongs to nobody
    const int64_t out_bytes = ((B - 1) * rs_out + T) * 4;
    if (ap_onset_overlap(S, ((B * M - 1) * rs_in + T) * 4, out, out_bytes) ||
        (ref && ap_onset_overlap(ref, ((B * M - 1) * rs_ref + T) * 4, out, out_bytes)))
        AP_FAIL(AP_ERR_INVALID, "onset_strength: the output overlaps an input");
    P.S = S; P.ref = ref; P.out = out;
    P.B = B; P.rs_in = rs_in; P.rs_ref = ref ? rs_ref : 0; P.rs_out = rs_out;
    P.M = (int)M; P.T = (int)T; P.lag = lag; P.max_size = max_size; P.shift = shift; P.db = db_mode ? 1 : 0;
    P.D.coef = db_coef; P.D.amin = db_amin; P.D.ref_value = db_ref; P.D.top_db = db_top_db >= 0.0f ? db_top_db : -1.0f;
    P.D.ref_key = nullptr; P.D.smax_key = smax_key;
    P.staged = (!ref && max_size > 1) ? 1 : 0;
    P.off_part = P.staged ? (APON_MC + max_size - 1) * APON_TT * 4 : 0;
    P.lds_bytes = P.off_part + APON_WAVES * APON_TT * 4;
    P.n_tt = (int)((T + APON_TT - 1) / APON_TT);
    if ((double)B * (double)P.n_tt > (double)kApMaxGrid) AP_FAIL(AP_ERR_UNSUPPORTED, "onset_strength: more than 2^31 - 1 tiles");
    P.n_tiles = B * (int64_t)P.n_tt;
    return AP_OK;
}

static inline int ap_onset_grid(const ApOnsetParams &P) { return (int)(P.n_tiles < (1 << 20) ? P.n_tiles : (1 << 20)); }

// SciPy's mode="reflect" index for any i
AP_DEV int apon_reflect(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// max(0, d) that keeps a NaN, as NumPy's maximum does (fmaxf would turn it into 0)
AP_DEV float apon_rectify(float d) { return d < 0.0f ? 0.0f : d; }

template <bool DB>
__global__ void __launch_bounds__(64 * APON_WAVES) ap_onset_strength_kernel(ApOnsetParams P) {
#ifndef AP_HOST_EMU
#pragma clang fp contract(off)   // coef log10(.) is rounded before the difference, as it is when the dB array is stored
#endif
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    float *L = reinterpret_cast<float *>(ap_smem);
    float *part = reinterpret_cast<float *>(ap_smem + P.off_part);
    float dref = 1.0f, dfloor = 0.0f;
    if (DB) { dref = ap_db_ref(P.D); dfloor = ap_db_floor(P.D, dref); }
    auto level = [&](float s) -> float { return DB ? fmaxf(ap_db_value(P.D, dref, s), dfloor) : s; };
    const int lo = P.max_size / 2;
    for (int64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
        const int64_t b = tile / P.n_tt;
        const int t = (int)(tile - b * P.n_tt) * APON_TT + lane;
        const int u = t - P.shift;
        const bool live = t < P.T && u >= 0;              // then 0 <= u and u + lag <= t < T
        const float *Sb = P.S + b * P.M * P.rs_in;
        const float *cur = Sb + (live ? u + P.lag : 0);
        float acc = 0.0f;
        if (!P.staged) {
            const float *Rb = P.ref ? P.ref + b * P.M * P.rs_ref : Sb;
            const int64_t rs_r = P.ref ? P.rs_ref : P.rs_in;
            const bool rdb = DB && !P.ref;
            if (live) {
#pragma unroll 4
                for (int m = wave; m < P.M; m += APON_WAVES) {
                    const float c = level(cur[(int64_t)m * P.rs_in]);
                    const float r0 = Rb[(int64_t)m * rs_r + u];
                    const float r = rdb ? level(r0) : r0;
                    acc += apon_rectify(c - r);
                }
            }
        } else {
            for (int m0 = 0; m0 < P.M; m0 += APON_MC) {
                const int mc = P.M - m0 < APON_MC ? P.M - m0 : APON_MC;
                const int rows = mc + P.max_size - 1;
                if (live) {
                    for (int r = wave; r < rows; r += APON_WAVES) {
                        const int m = apon_reflect(m0 - lo + r, P.M);
                        L[r * APON_TT + lane] = level(Sb[(int64_t)m * P.rs_in + u]);
                    }
                }
                AP_LDS_BARRIER();
                if (live) {
                    for (int ml = wave; ml < mc; ml += APON_WAVES) {
                        const float *w = L + ml * APON_TT + lane;       // rows m - lo .. m + (max_size - 1) / 2
                        float r = w[0];
                        for (int j = 1; j < P.max_size; ++j) {
                            const float v = w[j * APON_TT];
                            r = (v > r || v != v) ? v : r;          // a NaN stays (fmaxf would drop it)
                        }
                        const float c = level(cur[(int64_t)(m0 + ml) * P.rs_in]);
                        acc += apon_rectify(c - r);
                    }
                }
                AP_LDS_BARRIER();               // the next chunk overwrites the rows
            }
        }
        part[wave * APON_TT + lane] = acc;
        AP_LDS_BARRIER();
        if (wave == 0 && t < P.T) {
            const float s = ((part[lane] + part[APON_TT + lane]) + part[2 * APON_TT + lane]) + part[3 * APON_TT + lane];
            P.out[b * P.rs_out + t] = live ? s / (float)P.M : 0.0f;
        }
        AP_LDS_BARRIER();                       // the next tile overwrites the partial sums
    }
}

// ---- peak picking ----------------------------------------------------------------------------------------------
struct ApPeakPickParams {
    const float *x, *energy;    // (B, rs_x), (B, rs_e) or NULL
    unsigned char *mask;        // (B, T)
    int *count;                 // (B) or NULL
    int64_t B, rs_x, rs_e;
    int T, pre_max, post_max, pre_avg, post_avg, wait, normalize, guard, backtrack;
    float delta;
    int off_flag, off_cand, off_kept, off_red, lds_bytes;
};

static inline int ap_prepare_peak_pick(ApPeakPickParams &P, const float *x, int64_t B, int64_t T, int64_t rs_x, int pre_max,
                                       int post_max, int pre_avg, int post_avg, float delta, int wait, int normalize,
                                       int guard, int backtrack, const float *energy, int64_t rs_e,
                                       unsigned char *mask, int *count) {
    if (!x || !mask) AP_FAIL(AP_ERR_INVALID, "peak_pick: NULL buffer");
    if (B <= 0 || T <= 0) AP_FAIL(AP_ERR_INVALID, "peak_pick: x must be non-empty, got (%lld, %lld)", (long long)B, (long long)T);
    if (pre_max < 0 || pre_avg < 0) AP_FAIL(AP_ERR_INVALID, "pre_max and pre_avg must be non-negative integers, got (%d, %d)", pre_max, pre_avg);
    if (post_max < 1 || post_avg < 1) AP_FAIL(AP_ERR_INVALID, "post_max and post_avg must be positive integers, got (%d, %d)", post_max, post_avg);
    if (wait < 0) AP_FAIL(AP_ERR_INVALID, "wait must be a non-negative integer, got %d", wait);
    if (T > APPK_TMAX) AP_FAIL(AP_ERR_UNSUPPORTED, "peak_pick: rows of more than %d frames are not supported, got %lld", APPK_TMAX, (long long)T);
    if (rs_x < T || (energy && rs_e < T)) AP_FAIL(AP_ERR_INVALID, "peak_pick: row strides (%lld, %lld) must be >= T = %lld", (long long)rs_x, (long long)rs_e, (long long)T);
    if (B > ((int64_t)1 << 40) || rs_x > ((int64_t)1 << 40) || rs_e > ((int64_t)1 << 40)) AP_FAIL(AP_ERR_UNSUPPORTED, "peak_pick: extents too large");
    if (ap_onset_overlap(x, ((B - 1) * rs_x + T) * 4, mask, B * T) || (energy && ap_onset_overlap(energy, ((B - 1) * rs_e + T) * 4, mask, B * T)))
        AP_FAIL(AP_ERR_INVALID, "peak_pick: the mask overlaps an input");
    const int t = (int)T;
    P.x = x; P.energy = energy; P.mask = mask; P.count = count;
    P.B = B; P.rs_x = rs_x; P.rs_e = energy ? rs_e : 0;
    P.T = t;
    // a window never reaches further than the row
    P.pre_max = pre_max < t ? pre_max : t; P.post_max = post_max < t ? post_max : t;
    P.pre_avg = pre_avg < t ? pre_avg : t; P.post_avg = post_avg < t ? post_avg : t;
    P.wait = wait < t ? wait : t;
    P.normalize = normalize ? 1 : 0; P.guard = guard ? 1 : 0; P.backtrack = backtrack ? 1 : 0;
    P.delta = delta;
    const int nw = (t + 63) / 64;
    int off = ap_align16(t * 4);
    P.off_flag = off; off += ap_align16(t);
    P.off_cand = off; off += ap_align16(nw * 8);
    P.off_kept = off; off += ap_align16(nw * 8);
    P.off_red = off; off += (3 * APPK_BLOCK + 3 * 16) * 4;
    P.lds_bytes = off;
    return AP_OK;
}

static inline int ap_peak_pick_grid(const ApPeakPickParams &P) { return (int)(P.B < (1 << 16) ? P.B : (1 << 16)); }

__global__ void __launch_bounds__(APPK_BLOCK) ap_peak_pick_kernel(ApPeakPickParams P) {
    const int tid = threadIdx.x;
    const int T = P.T;
    const int nw = (T + 63) >> 6;
    float *xs = reinterpret_cast<float *>(ap_smem);
    unsigned char *flag = reinterpret_cast<unsigned char *>(ap_smem + P.off_flag);
    unsigned long long *cand = reinterpret_cast<unsigned long long *>(ap_smem + P.off_cand);
    unsigned long long *kept = reinterpret_cast<unsigned long long *>(ap_smem + P.off_kept);
    float *rmin = reinterpret_cast<float *>(ap_smem + P.off_red);
    float *rmax = rmin + APPK_BLOCK;
    int *rint = reinterpret_cast<int *>(rmax + APPK_BLOCK);
    float *qmin = reinterpret_cast<float *>(rint + APPK_BLOCK);
    float *qmax = qmin + 16;
    int *qint = reinterpret_cast<int *>(qmax + 16);
    for (int64_t b = blockIdx.x; b < P.B; b += gridDim.x) {
        const float *xb = P.x + b * P.rs_x;
        // the row, its minimum and maximum (NaN ignored) and whether every value is finite: two levels of 16
        float mn = INFINITY, mx = -INFINITY;
        int bad = 0;
        for (int n = tid; n < T; n += APPK_BLOCK) {
            const float v = xb[n];
            xs[n] = v;
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
            bad |= fabsf(v) <= 3.4028234664e38f ? 0 : 1;
        }
        rmin[tid] = mn; rmax[tid] = mx; rint[tid] = bad;
        AP_LDS_BARRIER();
        if (tid < 16) {
            for (int i = 0; i < 16; ++i) {
                mn = fminf(mn, rmin[tid * 16 + i]);
                mx = fmaxf(mx, rmax[tid * 16 + i]);
                bad |= rint[tid * 16 + i];
            }
            qmin[tid] = mn; qmax[tid] = mx; qint[tid] = bad;
        }
        AP_LDS_BARRIER();
        mn = qmin[0]; mx = qmax[0]; bad = qint[0];
        for (int i = 1; i < 16; ++i) {
            mn = fminf(mn, qmin[i]);
            mx = fmaxf(mx, qmax[i]);
            bad |= qint[i];
        }
        const bool empty = P.guard && (bad || (mn == 0.0f && mx == 0.0f));
        if (P.normalize) {
            const float den = (mx - mn) + APPK_FLT_MIN;
            for (int n = tid; n < T; n += APPK_BLOCK) xs[n] = (xs[n] - mn) / den;     // the values this thread stored
        }
        AP_LDS_BARRIER();
        // candidates: every frame on its own
        for (int n = tid; n < T; n += APPK_BLOCK) {
            const float v = xs[n];
            int a = n - P.pre_max > 0 ? n - P.pre_max : 0;
            int e = n + P.post_max < T ? n + P.post_max : T;
            float m = xs[a];
            for (int i = a + 1; i < e; ++i) {
                const float w = xs[i];
                m = (w > m || w != w) ? w : m;              // a NaN stays
            }
            a = n - P.pre_avg > 0 ? n - P.pre_avg : 0;
            e = n + P.post_avg < T ? n + P.post_avg : T;
            float sum = 0.0f;
            for (int i = a; i < e; ++i) sum += xs[i];
            const float mean = sum / (float)(e - a);
            flag[n] = (!empty && v == m && v >= mean + P.delta) ? 1 : 0;
        }
        AP_LDS_BARRIER();
        for (int w = tid; w < nw; w += APPK_BLOCK) {
            unsigned long long bits = 0;
            const int n1 = T - w * 64 < 64 ? T - w * 64 : 64;
            for (int j = 0; j < n1; ++j) bits |= (unsigned long long)flag[w * 64 + j] << j;
            cand[w] = bits;
        }
        AP_LDS_BARRIER();
        // the greedy pass, over the candidates only; the flags become the final mask meanwhile
        if (tid == 0) {
            int last = -(P.wait + 1);
            for (int w = 0; w < nw; ++w) {
                unsigned long long bits = cand[w], keep = 0;
                while (bits) {
                    const int j = __builtin_ctzll(bits);
                    bits &= bits - 1;
                    const int n = w * 64 + j;
                    if (n > last + P.wait) { keep |= 1ull << j; last = n; }
                }
                kept[w] = keep;
            }
        }
        for (int n = tid; n < T; n += APPK_BLOCK) flag[n] = 0;
        AP_LDS_BARRIER();
        const float *en = P.energy ? P.energy + b * P.rs_e : xs;
        for (int w = tid; w < nw; w += APPK_BLOCK) {
            unsigned long long bits = kept[w];
            while (bits) {
                int k = w * 64 + __builtin_ctzll(bits);
                bits &= bits - 1;
                if (P.backtrack)
                    while (k > 0 && !(k <= T - 2 && en[k] <= en[k - 1] && en[k] < en[k + 1])) --k;
                flag[k] = 1;                                  // coinciding ones merge
            }
        }
        AP_LDS_BARRIER();
        int cnt = 0;
        for (int n = tid; n < T; n += APPK_BLOCK) {
            const unsigned char f = flag[n];
            P.mask[b * T + n] = f;
            cnt += f;
        }
        if (P.count) {                                         // (uniform)
            rint[tid] = cnt;
            AP_LDS_BARRIER();
            if (tid < 16) {
                int s = 0;
                for (int i = 0; i < 16; ++i) s += rint[tid * 16 + i];
                qint[tid] = s;
            }
            AP_LDS_BARRIER();
            if (tid == 0) {
                int s = 0;
                for (int i = 0; i < 16; ++i) s += qint[i];
                P.count[b] = s;
            }
        }
        AP_LDS_BARRIER();                       // the next row overwrites everything
    }
}
