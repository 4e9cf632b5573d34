// Chroma features (chroma.py: chroma_stft, chroma_cqt, chroma_cens, tonnetz; the definitions of librosa 0.10).
//
// ap_chroma_fold_kernel.  For a spectrum x (B, K, T), a matrix w (n_out, K) and every frame (b, t):
//   v_k = x (real), |z| or |z|^2 (complex)                      in_kind 0 / 1 / 2
//   a_c = sum_k w[c,k] v_k                                      (w NULL: the identity, K = n_out)
//   pre_l1:     p = sum_k |v_k|, p < FLT_MIN -> 1, a_c = a_c / p
//   threshold:  a_c < threshold -> 0
//   norm:       n = max |a|, sum |a| or sqrt(sum a^2), n < FLT_MIN -> 1, out_c = a_c / n
// One read of x, one write of out.
//
//   A workgroup (4 waves) owns one clip and a tile of APCH_TT = 64 frames: lane = frame, so every read of x and
//   every write of out is one row segment of 64 consecutive frames.  The bins are dealt to the waves in runs of
//   APCH_U = 4: wave q takes k = 16 j + 4 q + u.  A lane keeps the n_out sums of its frame in registers (NACC of
//   them, the next of 6, 12, 24, 36, 48 at or above n_out: the rows past n_out repeat row n_out - 1 and are never
//   joined); w[c,k] is the same for every lane of a wave.  The four values of a run are loaded before they are used.
//   Waves 1 to 3 hand their sums over through LDS and wave 0 joins them in wave order, ((s0 + s1) + s2) + s3,
//   then normalises its frame and writes it.
//
//   Every product is an fmaf, every sum has a fixed order, sqrtf and / are IEEE: a frame's bits depend on nothing
//   but its own column of x.  The longest chain of dependent additions is d = APCH_U ceil(K / 16) + 3.
//
// ap_chroma_cens_kernel.  For chroma (B, n, T):
//   v = chroma / max(sum_c |chroma|, -> 1 below FLT_MIN);  q = 0.25 ([v > .4] + [v > .2] + [v > .1] + [v > .05])
//   s[c,t] = sum_j taps[j] q[c, t + (n_taps - 1) / 2 - j], q = 0 outside [0, T)          (n_taps = 0: s = q)
//   out = s / norm(s) as above.
//   A workgroup owns one clip and APCN_TT = 64 frames.  One thread per frame of the tile and its halo
//   (64 + n_taps - 1 <= 192 frames) quantises its frame into LDS; thread (f, g) = (tid & 63, tid >> 6) then sums the
//   taps in ascending j for the channels c = g, g + 4, .. into a second LDS plane, and after a barrier walks all n
//   channels of frame f in ascending c for the norm and writes its own channels.  Nothing but out reaches memory.
#pragma once
#include <cfloat>
#include <cmath>

#include "ap_launch.h"
#include "fft_lds.h"

extern __shared__ __attribute__((aligned(16))) char ap_smem[];

#define APCH_WAVES 4            // waves per workgroup of the fold
#define APCH_TT 64              // frames per tile: lane = frame
#define APCH_U 4                // consecutive bins a wave takes per step
#define APCH_MAX_OUT 48         // cap on n_out (and on n of the CENS kernel)
#define APCN_TT 64              // output frames per tile of the CENS kernel
#define APCN_MAX_SMOOTH 129     // cap on n_taps
#define APCN_THREADS 256

static_assert(APCH_TT == 64, "lane = frame");
static_assert(APCN_TT + APCN_MAX_SMOOTH - 1 <= APCN_THREADS, "one thread quantises one frame of tile + halo");
static_assert(APCH_MAX_OUT * (2 * APCN_TT + APCN_MAX_SMOOTH - 1) * 4 <= 48 * 1024, "the CENS planes fit without the opt-in");
static_assert((APCH_WAVES - 1) * (APCH_MAX_OUT + 1) * 64 * 4 <= 48 * 1024, "the fold's hand-over fits without the opt-in");

struct ApChromaFoldParams {
    const float *x;             // (B, K, in_rs) float, or complex as (re, im)
    const float *w;             // (n_out, K) or NULL
    float *out;                 // (B, n_out, out_rs)
    int64_t B, T, in_rs, out_rs, n_tt, n_tiles;
    int K, n_out, in_kind, pre_l1, use_threshold, norm, nacc, lds_bytes;
    float threshold;
};

struct ApChromaCensParams {
    const float *x;             // (B, n, in_rs)
    const float *taps;          // (n_taps) or NULL
    float *out;                 // (B, n, out_rs)
    int64_t B, T, in_rs, out_rs, n_tt, n_tiles;
    int n, n_taps, norm, halo, lds_bytes;
};

static inline int ap_chroma_nacc(int n_out) { return n_out <= 6 ? 6 : n_out <= 12 ? 12 : n_out <= 24 ? 24 : n_out <= 36 ? 36 : 48; }

// Validation and the launch geometry of ap_chroma_fold_f32 (and of its emulator twin).
static inline int ap_prepare_chroma_fold(ApChromaFoldParams &P, const float *x, int in_kind, int64_t B, int K, int64_t T,
                                         int64_t in_rs, const float *w, int n_out, int pre_l1, int use_threshold,
                                         float threshold, int norm, float *out, int64_t out_rs) {
    if (!x || !out) AP_FAIL(AP_ERR_INVALID, "chroma_fold: NULL buffer");
    if (B <= 0 || K <= 0 || T <= 0)
        AP_FAIL(AP_ERR_INVALID, "chroma_fold: the spectrum must be non-empty, got (%lld, %d, %lld)", (long long)B, K, (long long)T);
    if (n_out < 1 || n_out > APCH_MAX_OUT) AP_FAIL(AP_ERR_INVALID, "chroma_fold: n_out must lie in [1, %d], got %d", APCH_MAX_OUT, n_out);
    if (in_kind < 0 || in_kind > 2) AP_FAIL(AP_ERR_INVALID, "chroma_fold: unknown in_kind %d (0 real, 1 |z|, 2 |z|^2)", in_kind);
    if (norm < 0 || norm > 3) AP_FAIL(AP_ERR_INVALID, "chroma_fold: unknown norm %d (0 none, 1, 2, 3 = inf)", norm);
    if (in_rs < T) AP_FAIL(AP_ERR_INVALID, "chroma_fold: in_row_stride (%lld) must be >= T = %lld", (long long)in_rs, (long long)T);
    if (out_rs < T) AP_FAIL(AP_ERR_INVALID, "chroma_fold: out_row_stride (%lld) must be >= T = %lld", (long long)out_rs, (long long)T);
    if (!w && K != n_out) AP_FAIL(AP_ERR_INVALID, "chroma_fold: w = NULL is the identity and needs K == n_out, got %d and %d", K, n_out);
    if ((double)B * (double)K * (double)in_rs * 8.0 > 9.0e18 || (double)B * (double)n_out * (double)out_rs * 4.0 > 9.0e18)
        AP_FAIL(AP_ERR_UNSUPPORTED, "chroma_fold: more than 2^63 bytes");
    P.x = x; P.w = w; P.out = out;
    P.B = B; P.T = T; P.in_rs = in_rs; P.out_rs = out_rs;
    P.K = K; P.n_out = n_out; P.in_kind = in_kind; P.pre_l1 = pre_l1 ? 1 : 0; P.use_threshold = use_threshold ? 1 : 0;
    P.norm = norm; P.threshold = threshold;
    P.nacc = ap_chroma_nacc(n_out);
    P.n_tt = (T + APCH_TT - 1) / APCH_TT;
    if ((double)B * (double)P.n_tt > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "chroma_fold: too many tiles");
    P.n_tiles = B * P.n_tt;
    P.lds_bytes = (APCH_WAVES - 1) * (P.nacc + 1) * 64 * 4;
    return AP_OK;
}

static inline int ap_prepare_chroma_cens(ApChromaCensParams &P, const float *x, int64_t B, int n, int64_t T, int64_t in_rs,
                                         const float *taps, int n_taps, int norm, float *out, int64_t out_rs) {
    if (!x || !out) AP_FAIL(AP_ERR_INVALID, "chroma_cens: NULL buffer");
    if (B <= 0 || T <= 0) AP_FAIL(AP_ERR_INVALID, "chroma_cens: chroma must be non-empty, got (%lld, %d, %lld)", (long long)B, n, (long long)T);
    if (n < 1 || n > APCH_MAX_OUT) AP_FAIL(AP_ERR_INVALID, "chroma_cens: n must lie in [1, %d], got %d", APCH_MAX_OUT, n);
    if (n_taps < 0 || n_taps > APCN_MAX_SMOOTH) AP_FAIL(AP_ERR_INVALID, "chroma_cens: n_taps must lie in [0, %d], got %d", APCN_MAX_SMOOTH, n_taps);
    if (n_taps > 0 && !taps) AP_FAIL(AP_ERR_INVALID, "chroma_cens: NULL taps");
    if (norm < 0 || norm > 3) AP_FAIL(AP_ERR_INVALID, "chroma_cens: unknown norm %d (0 none, 1, 2, 3 = inf)", norm);
    if (in_rs < T) AP_FAIL(AP_ERR_INVALID, "chroma_cens: in_row_stride (%lld) must be >= T = %lld", (long long)in_rs, (long long)T);
    if (out_rs < T) AP_FAIL(AP_ERR_INVALID, "chroma_cens: out_row_stride (%lld) must be >= T = %lld", (long long)out_rs, (long long)T);
    if ((double)B * (double)n * (double)in_rs * 4.0 > 9.0e18 || (double)B * (double)n * (double)out_rs * 4.0 > 9.0e18)
        AP_FAIL(AP_ERR_UNSUPPORTED, "chroma_cens: more than 2^63 bytes");
    P.x = x; P.taps = taps; P.out = out;
    P.B = B; P.T = T; P.in_rs = in_rs; P.out_rs = out_rs;
    P.n = n; P.n_taps = n_taps; P.norm = norm;
    P.halo = n_taps > 0 ? n_taps - 1 : 0;
    P.n_tt = (T + APCN_TT - 1) / APCN_TT;
    if ((double)B * (double)P.n_tt > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "chroma_cens: too many tiles");
    P.n_tiles = B * P.n_tt;
    P.lds_bytes = n * (2 * APCN_TT + P.halo) * 4;
    return AP_OK;
}

static inline int ap_chroma_grid(int64_t n_tiles) { return (int)(n_tiles < (1 << 24) ? n_tiles : (1 << 24)); }

// w is read-only for the whole launch and its index is the same for every lane of a wave: on the device it is read
// through the constant address space, which makes the loads scalar
#ifdef AP_HOST_EMU
#define APCH_CONST
AP_DEV int apch_uniform(int x) { return x; }
#else
#define APCH_CONST __attribute__((address_space(4)))
AP_DEV int apch_uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }
#endif

// v_k of one frame, `e` pointing at the frame's element of row k: x as it is, |z| or |z|^2.  IEEE sqrtf; explicit fmaf.
template <int KIND>
AP_DEV float apch_value(const float *e) {
    if (KIND == 0) return e[0];
    const float re = e[0], im = e[1];
    const float m2 = fmaf(im, im, re * re);
    return KIND == 1 ? sqrtf(m2) : m2;
}

// One wave's share of the sums of a frame: the runs k = 16 j + 4 wave + u in ascending k.  xl points at the lane's
// frame in row 0, rows `rs` floats apart.  IDENT: w is the identity.  Rows c >= n_out repeat row n_out - 1.
template <int NACC, int KIND, bool IDENT>
AP_DEV void apch_accumulate(const ApChromaFoldParams &P, const float *xl, int64_t rs, int wave, float (&acc)[NACC], float &p) {
    const int K = P.K, n_out = P.n_out;
    const APCH_CONST float *w = (const APCH_CONST float *)P.w;
    int k0 = APCH_U * wave;
    for (; k0 + APCH_U <= K; k0 += APCH_U * APCH_WAVES) {
        float v[APCH_U];
#pragma unroll
        for (int u = 0; u < APCH_U; ++u) v[u] = apch_value<KIND>(xl + (int64_t)(k0 + u) * rs);
#pragma unroll
        for (int u = 0; u < APCH_U; ++u) {
            p += fabsf(v[u]);
#pragma unroll
            for (int c = 0; c < NACC; ++c) {
                const int cc = c < n_out ? c : n_out - 1;
                const float wv = IDENT ? (cc == k0 + u ? 1.0f : 0.0f) : w[(int64_t)cc * K + (k0 + u)];
                acc[c] = fmaf(wv, v[u], acc[c]);
            }
        }
    }
    for (int k = k0; k < K; ++k) {                              // the last, short run
        const float v = apch_value<KIND>(xl + (int64_t)k * rs);
        p += fabsf(v);
#pragma unroll
        for (int c = 0; c < NACC; ++c) {
            const int cc = c < n_out ? c : n_out - 1;
            const float wv = IDENT ? (cc == k ? 1.0f : 0.0f) : w[(int64_t)cc * K + k];
            acc[c] = fmaf(wv, v, acc[c]);
        }
    }
}

// max that keeps a NaN once it has one
AP_DEV float apch_nanmax(float n, float a) { return (a > n || a != a) ? a : n; }

// a_c -> out_c over the n channels of one frame read through `get(c)`: the norm in ascending c
template <class Get>
AP_DEV float apch_norm(int norm, int n, Get get) {
    float s = 0.0f;
    if (norm == 3) {
        for (int c = 0; c < n; ++c) s = apch_nanmax(s, fabsf(get(c)));
    } else if (norm == 1) {
        for (int c = 0; c < n; ++c) s += fabsf(get(c));
    } else {
        for (int c = 0; c < n; ++c) { const float a = get(c); s = fmaf(a, a, s); }
        s = sqrtf(s);
    }
    return s < FLT_MIN ? 1.0f : s;
}

template <int NACC, int KIND>
__global__ void __launch_bounds__(64 * APCH_WAVES) ap_chroma_fold_kernel(ApChromaFoldParams P) {
    float *hand = reinterpret_cast<float *>(ap_smem);          // [APCH_WAVES - 1][NACC + 1][64]
    const int lane = threadIdx.x & 63;
    const int wave = apch_uniform((int)(threadIdx.x >> 6));
    const int K = P.K, n_out = P.n_out;
    const int64_t esz = KIND == 0 ? 1 : 2;
    for (int64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
        const int64_t b = tile / P.n_tt;
        const int64_t t0 = (tile - b * P.n_tt) * APCH_TT;
        const int64_t t = t0 + lane;
        const bool live = t < P.T;
        // a lane beyond the clip's end reads the last frame again and stores nothing
        const float *xl = P.x + (b * K * P.in_rs + (live ? t : P.T - 1)) * esz;

        float acc[NACC];
#pragma unroll
        for (int c = 0; c < NACC; ++c) acc[c] = 0.0f;
        float p = 0.0f;
        if (P.w) apch_accumulate<NACC, KIND, false>(P, xl, P.in_rs * esz, wave, acc, p);
        else apch_accumulate<NACC, KIND, true>(P, xl, P.in_rs * esz, wave, acc, p);

        // waves 1 .. 3 hand their sums over, wave 0 joins them in wave order
        if (wave > 0) {
            float *h = hand + (wave - 1) * (NACC + 1) * 64;
#pragma unroll
            for (int c = 0; c < NACC; ++c) h[c * 64 + lane] = acc[c];
            h[NACC * 64 + lane] = p;
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int q = 0; q < APCH_WAVES - 1; ++q) {
                const float *h = hand + q * (NACC + 1) * 64;
#pragma unroll
                for (int c = 0; c < NACC; ++c) acc[c] += h[c * 64 + lane];
                p += h[NACC * 64 + lane];
            }
            if (P.pre_l1) {
                if (p < FLT_MIN) p = 1.0f;
#pragma unroll
                for (int c = 0; c < NACC; ++c) acc[c] = acc[c] / p;
            }
            if (P.use_threshold) {
#pragma unroll
                for (int c = 0; c < NACC; ++c)
                    if (acc[c] < P.threshold) acc[c] = 0.0f;
            }
            if (P.norm) {
                // the rows past n_out repeat row n_out - 1: they change no maximum, and the sums stop at n_out
                float s = 0.0f;
                if (P.norm == 3) {
#pragma unroll
                    for (int c = 0; c < NACC; ++c) s = apch_nanmax(s, fabsf(acc[c]));
                } else if (P.norm == 1) {
#pragma unroll
                    for (int c = 0; c < NACC; ++c)
                        if (c < n_out) s += fabsf(acc[c]);
                } else {
#pragma unroll
                    for (int c = 0; c < NACC; ++c)
                        if (c < n_out) s = fmaf(acc[c], acc[c], s);
                    s = sqrtf(s);
                }
                if (s < FLT_MIN) s = 1.0f;
#pragma unroll
                for (int c = 0; c < NACC; ++c) acc[c] = acc[c] / s;
            }
            if (live) {
                float *ob = P.out + b * n_out * P.out_rs + t;
#pragma unroll
                for (int c = 0; c < NACC; ++c)
                    if (c < n_out) ob[(int64_t)c * P.out_rs] = acc[c];
            }
        }
        __syncthreads();                                    // the hand-over buffer is free for the next tile
    }
}

__global__ void __launch_bounds__(APCN_THREADS) ap_chroma_cens_kernel(ApChromaCensParams P) {
    const int n = P.n, n_taps = P.n_taps, halo = P.halo;
    const int W = APCN_TT + halo;                              // frames of the tile and its halo
    float *q = reinterpret_cast<float *>(ap_smem);             // [n][W]
    float *sm = q + n * W;                                     // [n][APCN_TT]
    const int tid = threadIdx.x;
    const int h = n_taps > 0 ? (n_taps - 1) / 2 : 0;
    for (int64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
        const int64_t b = tile / P.n_tt;
        const int64_t t0 = (tile - b * P.n_tt) * APCN_TT;
        const float *xb = P.x + b * n * P.in_rs;
        // local frame i of the tile is frame t0 + h - halo + i of the clip
        if (tid < W) {
            const int64_t g = t0 + h - halo + tid;
            if (g >= 0 && g < P.T) {
                float p = 0.0f;
                for (int c = 0; c < n; ++c) p += fabsf(xb[(int64_t)c * P.in_rs + g]);
                if (p < FLT_MIN) p = 1.0f;
                for (int c = 0; c < n; ++c) {
                    const float v = xb[(int64_t)c * P.in_rs + g] / p;
                    q[c * W + tid] = 0.25f * ((v > 0.4f ? 1.0f : 0.0f) + (v > 0.2f ? 1.0f : 0.0f) + (v > 0.1f ? 1.0f : 0.0f) +
                                              (v > 0.05f ? 1.0f : 0.0f));
                }
            } else {
                for (int c = 0; c < n; ++c) q[c * W + tid] = 0.0f;
            }
        }
        __syncthreads();
        const int f = tid & (APCN_TT - 1), grp = tid >> 6;
        for (int c = grp; c < n; c += APCN_THREADS / APCN_TT) {
            float s;
            if (n_taps > 0) {
                s = 0.0f;
                const float *qc = q + c * W + f + halo;        // tap j meets local frame f + halo - j
                for (int j = 0; j < n_taps; ++j) s = fmaf(P.taps[j], qc[-j], s);
            } else {
                s = q[c * W + f];
            }
            sm[c * APCN_TT + f] = s;
        }
        __syncthreads();
        const int64_t t = t0 + f;
        if (t < P.T) {
            float nrm = 1.0f;
            if (P.norm) nrm = apch_norm(P.norm, n, [&](int c) { return sm[c * APCN_TT + f]; });
            float *ob = P.out + b * n * P.out_rs + t;
            for (int c = grp; c < n; c += APCN_THREADS / APCN_TT) {
                const float s = sm[c * APCN_TT + f];
                ob[(int64_t)c * P.out_rs] = P.norm ? s / nrm : s;
            }
        }
        __syncthreads();                                    // the planes are free for the next tile
    }
}
