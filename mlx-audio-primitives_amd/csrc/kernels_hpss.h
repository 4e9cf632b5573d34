// Harmonic / percussive source separation by median filtering (Fitzgerald 2010; decompose.py: hpss, hpss_medians,
// hpss_audio, harmonic, percussive).
//
// For M = |S| (or S itself when real) of one clip, (F, T), and window sizes kh, kp in 1 .. 255:
//   harm[f,t] = element of rank kh / 2 (0-based, ascending) of M[f, r(t - kh/2 + j, T)], j = 0 .. kh - 1
//   perc[f,t] = element of rank kp / 2 of M[r(f - kp/2 + j, F), t],                      j = 0 .. kp - 1
//   r(i, n)   = i mod 2n, mirrored as 2n - 1 - i when that is >= n  (SciPy's mode="reflect": d c b a | a b c d | d c b a,
//               repeated as often as the window needs when it is longer than the axis)
// = scipy.ndimage.median_filter(M, size=(1, kh) / (kp, 1), mode="reflect"), bit for bit: a median is one of its
// inputs.  Then librosa's softmask in float32,
//   mask_h = softmask(harm, perc * margin_h),  mask_p = softmask(perc, harm * margin_p),
//   softmask(X, R): Z = max(X, R); Z < FLT_MIN -> 0.5 if split else 0; else a = (X/Z)^power, r = (R/Z)^power, a / (a + r);
//   power = inf: X > R as 0 / 1;   split = (margin_h == 1 and margin_p == 1)
// and the components S * mask_h, S * mask_p (real and imaginary part each times the mask).
//
// One kernel body, two instantiations of the median:
//
//   FUSED (kh = kp = 31): a 256-thread workgroup owns f_tile x 64 outputs of one clip and stages the
//   (f_tile + 30) x 94 magnitudes around them in LDS (reflect indices and |.| applied on load).  Lanes run along T:
//   the 31 reads of the time window (one row, columns lane + j) and the 31 reads of the frequency window (column
//   lane + 15, rows fl + j) are both 64 consecutive dwords per instruction, so a 32-lane half touches 32 different
//   banks whatever the row pitch is; the pitch is the region's width, which also keeps the staging stores (one row
//   segment per instruction) consecutive.  The median is a comparator network on 31 registers: Batcher's odd-even
//   merge sort for 32 inputs, the comparators of the +inf input dropped and the rest pruned backwards to what output
//   15 depends on (built at compile time by aph_make_net; APHP_NET_OPS min / max per median).
//
//   general (any kh, kp in 1 .. 255): the same staging into two regions (the rows of the tile with kh - 1 halo columns,
//   the columns of the tile with kp - 1 halo rows), and the median by rank counting straight from LDS: the candidate v
//   with #(w < v) <= rank < #(w <= v).  The fallback, and the cross-check of the network (identical bits on (31, 31)).
//
// Every output depends on its clip's values and (f, t) only: tiles, workgroups and batch position do not enter.
#pragma once
#include <utility>

#include "ap_launch.h"
#include "fft_lds.h"

extern __shared__ __attribute__((aligned(16))) char ap_smem[];

#define APHP_WAVES 4            // waves per workgroup; wave w owns the tile rows w, w + 4, ...
#define APHP_TT 64              // tile width along T: the lanes of a wave
#define APHP_K 31               // the window the network serves
#define APHP_FT 32              // default tile height along F
#define APHP_FT_MAX 64
#define APHP_KMAX 255
#define APHP_LDS_GENERAL (96 * 1024)    // the general kernel lowers its tile height until both regions fit in this
#define APHP_FLT_MIN 1.17549435e-38f

enum { APHP_POW_ANY = 0, APHP_POW_1 = 1, APHP_POW_2 = 2, APHP_POW_HARD = 3 };

struct ApHpssParams {
    const float *S;             // (B, F, rs_in) real, or complex pairs
    float *out_h, *out_p;       // (B, F, rs_out) real (complex pairs: components of a complex input), either may be NULL
    int64_t B, rs_in, rs_out, n_tiles;
    int F, T, kh, kp, mode, is_complex, split, pow_kind, fused;
    float margin_h, margin_p, power;
    int f_tile, n_ft, n_tt;
    int rows_a, cols_a, rows_b, cols_b, off_b, lds_bytes;    // LDS regions (fused: region a only)
};

static inline bool ap_hpss_network_sizes(int kh, int kp) { return kh == APHP_K && kp == APHP_K; }

static inline bool ap_hpss_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

// Validation and launch geometry of ap_hpss_f32 (and of its emulator twin).  f_tile: 0 = the default tile height.
static inline int ap_prepare_hpss(ApHpssParams &P, const float *S, int is_complex, int64_t B, int64_t F, int64_t T,
                                  int64_t rs_in, int kh, int kp, float margin_h, float margin_p, float power, int mode,
                                  int general, float *out_h, float *out_p, int64_t rs_out, int f_tile) {
    if (!S || (!out_h && !out_p)) AP_FAIL(AP_ERR_INVALID, "hpss: NULL buffer");
    if (B <= 0 || F <= 0 || T <= 0) AP_FAIL(AP_ERR_INVALID, "hpss: S must be non-empty, got (%lld, %lld, %lld)", (long long)B, (long long)F, (long long)T);
    if (kh < 1 || kh > APHP_KMAX || kp < 1 || kp > APHP_KMAX)
        AP_FAIL(AP_ERR_INVALID, "kernel_size must be an integer in 1 .. 255, got (%d, %d)", kh, kp);
    if (mode < 0 || mode > 2) AP_FAIL(AP_ERR_INVALID, "hpss: mode must be 0 (components), 1 (masks) or 2 (medians), got %d", mode);
    if (!(margin_h >= 1.0f) || !(margin_p >= 1.0f)) AP_FAIL(AP_ERR_INVALID, "Margins must be >= 1.0. A typical range is between 1 and 10.");
    if (!(power > 0.0f)) AP_FAIL(AP_ERR_INVALID, "power must be strictly positive");
    if (rs_in < T || rs_out < T) AP_FAIL(AP_ERR_INVALID, "hpss: row strides (%lld, %lld) must be >= T = %lld", (long long)rs_in, (long long)rs_out, (long long)T);
    if (f_tile < 0 || f_tile > APHP_FT_MAX) AP_FAIL(AP_ERR_INVALID, "hpss: tile height must be in 1 .. %d", APHP_FT_MAX);
    // 32-bit (f, t) and reflect arithmetic (2 n and t0 + halo stay below 2^31); element offsets are 64-bit
    if (F > (1 << 28) || T > (1 << 28)) AP_FAIL(AP_ERR_UNSUPPORTED, "hpss: F and T must be <= 2^28");
    if (rs_in > ((int64_t)1 << 40) || rs_out > ((int64_t)1 << 40) || B > ((int64_t)1 << 40)) AP_FAIL(AP_ERR_UNSUPPORTED, "hpss: extents too large");
    if ((double)B * (double)F * (double)(rs_in > rs_out ? rs_in : rs_out) * 8.0 > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "hpss: more than 2^63 bytes");
    const int64_t in_bytes = B * F * rs_in * (is_complex ? 8 : 4);
    const int64_t out_bytes = B * F * rs_out * ((is_complex && mode == 0) ? 8 : 4);
    if ((out_h && ap_hpss_overlap(S, in_bytes, out_h, out_bytes)) || (out_p && ap_hpss_overlap(S, in_bytes, out_p, out_bytes)))
        AP_FAIL(AP_ERR_INVALID, "hpss: an output overlaps S");
    if (out_h && out_p && ap_hpss_overlap(out_h, out_bytes, out_p, out_bytes)) AP_FAIL(AP_ERR_INVALID, "hpss: the outputs overlap");
    P.S = S; P.out_h = out_h; P.out_p = out_p;
    P.B = B; P.rs_in = rs_in; P.rs_out = rs_out;
    P.F = (int)F; P.T = (int)T; P.kh = kh; P.kp = kp; P.mode = mode; P.is_complex = is_complex ? 1 : 0;
    P.margin_h = margin_h; P.margin_p = margin_p; P.power = power;
    P.split = (margin_h == 1.0f && margin_p == 1.0f) ? 1 : 0;
    P.pow_kind = power == 1.0f ? APHP_POW_1 : power == 2.0f ? APHP_POW_2 : (power > 3.0e38f ? APHP_POW_HARD : APHP_POW_ANY);
    P.fused = (!general && ap_hpss_network_sizes(kh, kp)) ? 1 : 0;
    int ft = f_tile ? f_tile : APHP_FT;
    if (P.fused) {
        P.rows_a = ft + APHP_K - 1; P.cols_a = APHP_TT + APHP_K - 1;
        P.rows_b = 0; P.cols_b = 0;
        P.off_b = P.rows_a * P.cols_a * 4;
        P.lds_bytes = P.off_b;
    } else {
        for (;; ft >>= 1) {
            P.rows_a = ft; P.cols_a = APHP_TT + kh - 1;
            P.rows_b = ft + kp - 1; P.cols_b = APHP_TT;
            P.off_b = ap_align16(P.rows_a * P.cols_a * 4);
            P.lds_bytes = P.off_b + P.rows_b * P.cols_b * 4;
            if (P.lds_bytes <= APHP_LDS_GENERAL || ft == 1) break;
        }
    }
    if (P.lds_bytes > AP_LDS_MAX) AP_FAIL(AP_ERR_UNSUPPORTED, "hpss: the tile does not fit the LDS");
    P.f_tile = ft;
    P.n_ft = (int)((F + ft - 1) / ft);
    P.n_tt = (int)((T + APHP_TT - 1) / APHP_TT);
    P.n_tiles = B * P.n_ft * (int64_t)P.n_tt;
    if ((double)B * P.n_ft * (double)P.n_tt > (double)kApMaxGrid) AP_FAIL(AP_ERR_UNSUPPORTED, "hpss: more than 2^31 - 1 tiles");
    return AP_OK;
}

static inline int ap_hpss_grid(const ApHpssParams &P) { return (int)(P.n_tiles < (1 << 20) ? P.n_tiles : (1 << 20)); }

// ---- the comparator network -----------------------------------------------------------------------------------
// Batcher's odd-even merge sort on 32 wires (191 comparators, min to the lower wire).  Wire 31 carries +inf and is never
// the lower wire, so it keeps +inf and its comparators do nothing: dropped.  Walking the rest backwards from output
// 15 = the median of the 31 values keeps only what that output depends on, and of a comparator only the half (min or max)
// that is read afterwards.
struct ApHpssNet {
    int n, ops;
    unsigned char a[192], b[192], kind[192];       // kind: 1 = the min is used, 2 = the max, 3 = both
};
constexpr ApHpssNet aph_make_net() {
    ApHpssNet net{};
    unsigned char ca[192] = {}, cb[192] = {}, ck[192] = {};
    int n = 0;
    for (int p = 1; p < 32; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j <= 31 - k; j += 2 * k)
                for (int i = 0; i <= (k - 1 < 31 - j - k ? k - 1 : 31 - j - k); ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p) && i + j + k != 31) {
                        ca[n] = (unsigned char)(i + j);
                        cb[n] = (unsigned char)(i + j + k);
                        ++n;
                    }
    bool live[32] = {};
    live[(APHP_K + 1) / 2 - 1] = true;
    for (int c = n - 1; c >= 0; --c) {
        const bool la = live[ca[c]], lb = live[cb[c]];
        ck[c] = (unsigned char)((la ? 1 : 0) | (lb ? 2 : 0));
        if (la || lb) live[ca[c]] = live[cb[c]] = true;
    }
    for (int c = 0; c < n; ++c)
        if (ck[c]) {
            net.a[net.n] = ca[c]; net.b[net.n] = cb[c]; net.kind[net.n] = ck[c];
            ++net.n;
            net.ops += ck[c] == 3 ? 2 : 1;
        }
    return net;
}
#define APHP_NET_N (aph_make_net().n)          // comparators kept
#define APHP_NET_OPS (aph_make_net().ops)      // min / max operations per median

template <int I>
AP_DEV void aph_net_step(float (&v)[APHP_K]) {
    constexpr ApHpssNet net = aph_make_net();
    constexpr int a = net.a[I], b = net.b[I], kind = net.kind[I];
    const float lo = fminf(v[a], v[b]), hi = fmaxf(v[a], v[b]);
    if (kind & 1) v[a] = lo;
    if (kind & 2) v[b] = hi;
}
template <int... I>
AP_DEV float aph_net_run(float (&v)[APHP_K], std::integer_sequence<int, I...>) {
    (aph_net_step<I>(v), ...);
    return v[(APHP_K + 1) / 2 - 1];
}
// median of 31 values in registers (v is consumed); every index is a compile-time constant
AP_DEV float aph_median31(float (&v)[APHP_K]) { return aph_net_run(v, std::make_integer_sequence<int, APHP_NET_N>()); }

// the element of rank k / 2 among w[0], w[stride], ..., w[(k - 1) stride] (LDS) by rank counting
AP_DEV float aph_rank_select(const float *w, int stride, int k) {
    const int rank = k >> 1;
    float res = w[0];
    for (int i = 0; i < k; ++i) {
        const float vi = w[i * stride];
        int less = 0, leq = 0;
        for (int j = 0; j < k; ++j) {
            const float vj = w[j * stride];
            less += vj < vi ? 1 : 0;
            leq += vj <= vi ? 1 : 0;
        }
        if (less <= rank && rank < leq) { res = vi; break; }
    }
    return res;
}

// SciPy's mode="reflect" index for any i
AP_DEV int aph_reflect(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

AP_DEV float aph_softmask(float X, float R, int pow_kind, float power, int split) {
#ifndef AP_HOST_EMU
#pragma clang fp contract(off)   // a a + r r as NumPy rounds it: products, then the sum
#endif
    if (pow_kind == APHP_POW_HARD) return X > R ? 1.0f : 0.0f;
    const float Z = fmaxf(X, R);
    if (Z < APHP_FLT_MIN) return split ? 0.5f : 0.0f;
    float a = X / Z, r = R / Z;
    if (pow_kind == APHP_POW_2) { a = a * a; r = r * r; }
    else if (pow_kind == APHP_POW_ANY) { a = powf(a, power); r = powf(r, power); }
    return a / (a + r);
}

// magnitudes of rows f_org .. f_org + rows - 1, columns t_org .. t_org + cols - 1 of one clip (reflected) into L[rows][cols]:
// a wave stores one row segment of 64 consecutive floats per instruction
template <bool CPLX>
AP_DEV void aph_stage(const ApHpssParams &P, const float *Sb, float *L, int rows, int cols, int f_org, int t_org,
                      int wave, int lane) {
    for (int c = lane; c < cols; c += APHP_TT) {
        const int t = aph_reflect(t_org + c, P.T);
        for (int r = wave; r < rows; r += APHP_WAVES) {
            const int f = aph_reflect(f_org + r, P.F);
            const int64_t e = (int64_t)f * P.rs_in + t;
            L[r * cols + c] = CPLX ? ap_complex_abs(reinterpret_cast<const ap_float2 *>(Sb)[e]) : Sb[e];
        }
    }
}

template <bool CPLX, bool FUSED>
__global__ void __launch_bounds__(64 * APHP_WAVES) ap_hpss_kernel(ApHpssParams P) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    float *LA = reinterpret_cast<float *>(ap_smem);
    float *LB = reinterpret_cast<float *>(ap_smem + P.off_b);
    const int64_t per_clip = (int64_t)P.n_ft * P.n_tt;
    const bool want_h = P.out_h != nullptr, want_p = P.out_p != nullptr;
    // mode 2 needs only the medians that are stored; a mask needs both
    const bool need_h = P.mode != 2 || want_h, need_p = P.mode != 2 || want_p;
    const bool cplx_out = CPLX && P.mode == 0;
    for (int64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
        const int64_t b = tile / per_clip;
        const int rem = (int)(tile - b * per_clip);
        const int f0 = (rem / P.n_tt) * P.f_tile, t0 = (rem % P.n_tt) * APHP_TT;     // T fastest: neighbours share halo columns
        const float *Sb = P.S + b * P.F * P.rs_in * (CPLX ? 2 : 1);
        if (FUSED) {
            aph_stage<CPLX>(P, Sb, LA, P.rows_a, P.cols_a, f0 - APHP_K / 2, t0 - APHP_K / 2, wave, lane);
        } else {
            if (need_h || P.mode == 0) aph_stage<CPLX>(P, Sb, LA, P.rows_a, P.cols_a, f0, t0 - P.kh / 2, wave, lane);
            if (need_p) aph_stage<CPLX>(P, Sb, LB, P.rows_b, P.cols_b, f0 - P.kp / 2, t0, wave, lane);
        }
        AP_LDS_BARRIER();
        const int t = t0 + lane;
        if (t < P.T) {
            for (int fl = wave; fl < P.f_tile && f0 + fl < P.F; fl += APHP_WAVES) {
                float h = 0.0f, p = 0.0f, m;
                if (FUSED) {
                    constexpr int C = APHP_TT + APHP_K - 1;
                    const float *row = LA + (fl + APHP_K / 2) * C + lane;
                    const float *col = LA + fl * C + lane + APHP_K / 2;
                    float v[APHP_K];
                    m = row[APHP_K / 2];
                    if (need_h) {
#pragma unroll
                        for (int j = 0; j < APHP_K; ++j) v[j] = row[j];
                        h = aph_median31(v);
                    }
                    if (need_p) {
#pragma unroll
                        for (int j = 0; j < APHP_K; ++j) v[j] = col[j * C];
                        p = aph_median31(v);
                    }
                } else {
                    m = (P.mode == 0 && !CPLX) ? LA[fl * P.cols_a + lane + P.kh / 2] : 0.0f;
                    if (need_h) h = aph_rank_select(LA + fl * P.cols_a + lane, 1, P.kh);
                    if (need_p) p = aph_rank_select(LB + fl * P.cols_b + lane, P.cols_b, P.kp);
                }
                const int f = f0 + fl;
                const int64_t o = (b * P.F + f) * P.rs_out + t;
                if (P.mode == 2) {
                    if (want_h) P.out_h[o] = h;
                    if (want_p) P.out_p[o] = p;
                    continue;
                }
                float mh = 0.0f, mp = 0.0f;
                if (want_h) mh = aph_softmask(h, p * P.margin_h, P.pow_kind, P.power, P.split);
                if (want_p) mp = aph_softmask(p, h * P.margin_p, P.pow_kind, P.power, P.split);
                if (P.mode == 1) {
                    if (want_h) P.out_h[o] = mh;
                    if (want_p) P.out_p[o] = mp;
                } else if (cplx_out) {
                    const ap_float2 s = reinterpret_cast<const ap_float2 *>(Sb)[(int64_t)f * P.rs_in + t];
                    if (want_h) reinterpret_cast<ap_float2 *>(P.out_h)[o] = ap_mk(s.x * mh, s.y * mh);
                    if (want_p) reinterpret_cast<ap_float2 *>(P.out_p)[o] = ap_mk(s.x * mp, s.y * mp);
                } else {
                    if (want_h) P.out_h[o] = m * mh;
                    if (want_p) P.out_p[o] = m * mp;
                }
            }
        }
        AP_LDS_BARRIER();               // the next tile overwrites the regions
    }
}
