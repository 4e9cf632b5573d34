// piptrack / estimate_tuning / pitch_tuning (pitch.py; the definitions of librosa 0.10, restated in DESIGN.md 9.10 and
// tests/piptrack_ref.py).
//
// ap_piptrack_kernel.  For a magnitude spectrum S (B, F, T), real or complex (|z| = sqrtf(fmaf(im, im, re re)) on load), and
// every frame (b, t), with a, b, c = S[k-1], S[k], S[k+1]:
//   avg = 0.5 (c - a);  den = (2 b - c) - a;  shift = avg / (den + (|den| < FLT_MIN ? 1 : 0));  avg = shift = 0 at k = F - 1
//   dskew = (0.5 avg) shift;  ref_value = threshold max_k S[k], or |ref|;  X[k] = S[k] > ref_value ? S[k] : 0
//   peak(k) = X[k] > X[k-1] and X[k] >= X[min(k+1, F-1)] and max(k_lo, 1) <= k < k_hi
//   pitch = peak ? ((float)k + shift) bin_hz : 0;  magnitude = peak ? S[k] + dskew : 0
// Every operation is rounded on its own (contraction is off for the whole header); max is exact in any order: a
// frame's bits depend on nothing but its own column.
//
//   A workgroup (4 waves) owns one clip and a tile of APPT_TT = 64 frames: lane = frame, so every read of S and every
//   write is one row segment of 64 consecutive frames.  Wave q owns the bins [q ceil(F / 4), (q + 1) ceil(F / 4)).
//   The column is read twice: once for the frame's maximum (joined over the waves through 1 KB of LDS; skipped when
//   ref is given), once for the peaks, where a lane slides (a, b, c) down its bins and loads four rows ahead.
//   DENSE: pitches and magnitudes are written for every bin (zeros where there is no peak).
//   COMPACT: nothing dense is written.  A wave stages the (magnitude, pitch) records of its peaks with pitch > 0 in its own
//   4 KB of LDS (the slot from a ballot and a lane-prefix count: no atomic), and when fewer than 64 slots are left, and
//   at the end of the tile, takes n slots of its group's record buffer with ONE integer atomicAdd on the group's
//   counter and copies the records out in rows of 64.  The counter keeps counting past the capacity; records beyond
//   it are dropped and the host runs again with the exact size.  A group is the batch, or one clip (per_clip).
//
// ap_piptrack_tuning_kernel.  One workgroup of 1024 threads per group over its n = counter records:
//   the order statistics (n - 1) / 2 and n / 2 of the magnitudes by a radix select on the order-preserving key of the
//   float bits (4 passes of 8 bits, a 256-bin LDS histogram each; for even n the upper one is the lower one again when
//   equal keys reach past it, else the smallest key above it: one more pass with an integer atomicMin);
//   thr = odd n ? m : (m_lo + m_hi) 0.5f;  then the histogram of the residuals of the records with magnitude >= thr.
// ap_pitch_hist_kernel.  The same histogram over a dense array of frequencies, f <= 0 (and NaN) skipped.
//   r = fmod(bpo log2((double)f / 27.5), 1), + 1 when negative, - 1 when >= 0.5, all in float64; the bin is the i with
//   edges[i] <= r < edges[i+1] (numpy.histogram with explicit edges), found from a guess and corrected against the edges.
//   Counts are integers (LDS atomics per workgroup, then global): no floating-point atomic anywhere.
#pragma once
#include <cfloat>
#include <cmath>

#include "ap_launch.h"
#include "fft_lds.h"

// one rounding per operation, here and in whatever these functions are inlined into
#pragma clang fp contract(off)

extern __shared__ __attribute__((aligned(16))) char ap_smem[];

#define APPT_WAVES 4            // waves per workgroup of the peak kernel
#define APPT_TT 64              // frames per tile: lane = frame
#define APPT_U 4                // rows a lane loads ahead
#define APPT_WCAP 512           // records a wave stages in LDS
#define APPT_SEL_THREADS 1024   // one workgroup per group
#define APPT_HIST_THREADS 256
#define APPT_MAX_BINS 8192      // cap on the bins of the residual histogram
#define APPT_MAX_RECORDS 2147483647LL   // cap on the records of one group (32-bit LDS counters)

static_assert(APPT_TT == 64, "lane = frame");
static_assert(APPT_WCAP >= 128, "a wave adds at most 64 records between two checks");
static_assert((256 + 8 + APPT_MAX_BINS) * 4 <= 48 * 1024, "the select kernel's LDS fits without the opt-in");

typedef unsigned long long ap_u64;

struct ApPiptrackParams {
    const float *S;             // (B, F, in_rs) float, or complex as (re, im)
    const float *ref;           // (B, T) or NULL
    float *pitches, *mags;      // (B, F, out_rs), dense mode
    float *records;             // (G, capacity, 2), compact mode
    ap_u64 *counters;           // (G)
    int64_t B, T, in_rs, out_rs, n_tt, n_tiles, capacity;
    int F, k_lo, k_hi, kind, ref_mode, compact, per_clip, lds_bytes;
    float threshold, ref_value, bin_hz;
};

struct ApTuningParams {
    const float *records;       // (G, capacity, 2)
    const ap_u64 *counters;     // (G)
    const double *edges;        // (n_bins + 1)
    float *thr_out;             // (G)
    ap_u64 *counts;             // (G, n_bins)
    int64_t G, capacity;
    double bpo;
    int n_bins, lds_bytes;
};

struct ApPitchHistParams {
    const float *f;             // (n)
    const double *edges;        // (n_bins + 1)
    ap_u64 *counts;             // (n_bins), zero before the launch
    int64_t n;
    double bpo;
    int n_bins, lds_bytes;
};

// Validation and the launch geometry of ap_piptrack_f32 / ap_piptrack_records_f32 (and of their emulator twins).
static inline int ap_prepare_piptrack(ApPiptrackParams &P, const float *S, int in_kind, int64_t B, int F, int64_t T, int64_t in_rs,
                                      int k_lo, int k_hi, float threshold, int ref_mode, float ref_value, const float *ref,
                                      float bin_hz, int compact, float *pitches, float *mags, int64_t out_rs, int per_clip,
                                      float *records, int64_t capacity, ap_u64 *counters) {
    if (!S) AP_FAIL(AP_ERR_INVALID, "piptrack: NULL S");
    if (B <= 0 || T <= 0) AP_FAIL(AP_ERR_INVALID, "piptrack: S must be non-empty, got (%lld, %d, %lld)", (long long)B, F, (long long)T);
    if (F < 2) AP_FAIL(AP_ERR_INVALID, "piptrack: S must hold at least 2 frequency bins, got %d", F);
    if (in_kind < 0 || in_kind > 1) AP_FAIL(AP_ERR_INVALID, "piptrack: unknown in_kind %d (0 real, 1 complex)", in_kind);
    if (in_rs < T) AP_FAIL(AP_ERR_INVALID, "piptrack: in_row_stride (%lld) must be >= T = %lld", (long long)in_rs, (long long)T);
    if (k_lo < 0 || k_hi > F || k_lo > k_hi) AP_FAIL(AP_ERR_INVALID, "piptrack: need 0 <= k_lo <= k_hi <= F, got %d, %d, F = %d", k_lo, k_hi, F);
    if (ref_mode < 0 || ref_mode > 2) AP_FAIL(AP_ERR_INVALID, "piptrack: unknown ref_mode %d (0 threshold * max, 1 a scalar, 2 an array)", ref_mode);
    if (ref_mode == 0 && !(threshold >= 0.0f)) AP_FAIL(AP_ERR_INVALID, "piptrack: threshold must be non-negative, got %g", (double)threshold);
    if (ref_mode == 2 && !ref) AP_FAIL(AP_ERR_INVALID, "piptrack: ref_mode 2 needs ref");
    if ((double)B * (double)F * (double)in_rs * 8.0 > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "piptrack: more than 2^63 bytes");
    if (compact) {
        if (!records || !counters) AP_FAIL(AP_ERR_INVALID, "piptrack_records: NULL buffer");
        if (capacity < 1) AP_FAIL(AP_ERR_INVALID, "piptrack_records: capacity must be positive, got %lld", (long long)capacity);
        if (capacity > APPT_MAX_RECORDS)
            AP_FAIL(AP_ERR_UNSUPPORTED, "piptrack_records: capacity %lld is above the cap of %lld records per group", (long long)capacity, APPT_MAX_RECORDS);
        if ((double)(per_clip ? B : 1) * (double)capacity * 8.0 > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "piptrack_records: more than 2^63 bytes");
    } else {
        if (!pitches || !mags) AP_FAIL(AP_ERR_INVALID, "piptrack: NULL output");
        if (out_rs < T) AP_FAIL(AP_ERR_INVALID, "piptrack: out_row_stride (%lld) must be >= T = %lld", (long long)out_rs, (long long)T);
        if ((double)B * (double)F * (double)out_rs * 4.0 > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "piptrack: more than 2^63 bytes");
    }
    P.S = S; P.ref = ref; P.pitches = pitches; P.mags = mags; P.records = records; P.counters = counters;
    P.B = B; P.T = T; P.in_rs = in_rs; P.out_rs = out_rs; P.capacity = capacity;
    P.F = F; P.k_lo = k_lo; P.k_hi = k_hi; P.kind = in_kind; P.ref_mode = ref_mode; P.compact = compact ? 1 : 0;
    P.per_clip = per_clip ? 1 : 0;
    P.threshold = threshold; P.ref_value = ref_value; P.bin_hz = bin_hz;
    P.n_tt = (T + APPT_TT - 1) / APPT_TT;
    if ((double)B * (double)P.n_tt > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "piptrack: too many tiles");
    P.n_tiles = B * P.n_tt;
    P.lds_bytes = APPT_WAVES * 64 * 4 + (compact ? APPT_WAVES * APPT_WCAP * 8 : 0);
    return AP_OK;
}

static inline int ap_prepare_tuning_bins(const char *who, double bpo, const double *edges, int n_bins) {
    if (!edges) AP_FAIL(AP_ERR_INVALID, "%s: NULL edges", who);
    if (n_bins < 1) AP_FAIL(AP_ERR_INVALID, "%s: n_bins must be positive, got %d", who, n_bins);
    if (n_bins > APPT_MAX_BINS) AP_FAIL(AP_ERR_UNSUPPORTED, "%s: n_bins = %d is above the cap of %d (resolution too fine)", who, n_bins, APPT_MAX_BINS);
    if (!(bpo >= 1.0)) AP_FAIL(AP_ERR_INVALID, "%s: bins_per_octave must be >= 1, got %g", who, bpo);
    return AP_OK;
}

static inline int ap_prepare_piptrack_tuning(ApTuningParams &Q, const float *records, const ap_u64 *counters, int64_t G,
                                             int64_t capacity, double bpo, const double *edges, int n_bins, float *thr_out,
                                             ap_u64 *counts) {
    if (!records || !counters || !thr_out || !counts) AP_FAIL(AP_ERR_INVALID, "piptrack_tuning: NULL buffer");
    if (G <= 0 || capacity < 1) AP_FAIL(AP_ERR_INVALID, "piptrack_tuning: need G >= 1 and capacity >= 1, got %lld, %lld", (long long)G, (long long)capacity);
    if (capacity > APPT_MAX_RECORDS)
        AP_FAIL(AP_ERR_UNSUPPORTED, "piptrack_tuning: capacity %lld is above the cap of %lld records per group", (long long)capacity, APPT_MAX_RECORDS);
    if (G > (1 << 24)) AP_FAIL(AP_ERR_UNSUPPORTED, "piptrack_tuning: more than 2^24 groups");
    int rc = ap_prepare_tuning_bins("piptrack_tuning", bpo, edges, n_bins);
    if (rc != AP_OK) return rc;
    Q.records = records; Q.counters = counters; Q.edges = edges; Q.thr_out = thr_out; Q.counts = counts;
    Q.G = G; Q.capacity = capacity; Q.bpo = bpo; Q.n_bins = n_bins;
    Q.lds_bytes = (256 + 8 + n_bins) * 4;
    return AP_OK;
}

static inline int ap_prepare_pitch_hist(ApPitchHistParams &H, const float *f, int64_t n, double bpo, const double *edges, int n_bins,
                                        ap_u64 *counts) {
    if (!f || !counts) AP_FAIL(AP_ERR_INVALID, "pitch_hist: NULL buffer");
    if (n <= 0) AP_FAIL(AP_ERR_INVALID, "pitch_hist: frequencies must be non-empty, got %lld", (long long)n);
    if (n > (1LL << 42)) AP_FAIL(AP_ERR_UNSUPPORTED, "pitch_hist: more than 2^42 frequencies");
    int rc = ap_prepare_tuning_bins("pitch_hist", bpo, edges, n_bins);
    if (rc != AP_OK) return rc;
    H.f = f; H.n = n; H.bpo = bpo; H.edges = edges; H.n_bins = n_bins; H.counts = counts;
    H.lds_bytes = n_bins * 4;
    return AP_OK;
}

static inline int ap_piptrack_grid(int64_t n_tiles) { return (int)(n_tiles < (1 << 24) ? n_tiles : (1 << 24)); }
static inline int ap_pitch_hist_grid(int64_t n) { return ap_grid_1d(n, APPT_HIST_THREADS, kApStreamGrid); }

// Wave-level helpers.  The emulator's twins (emu_ballot64, emu_first_u64, atomicAdd, atomicMin) are defined by the
// translation unit that includes this header for the CPU.
#ifdef AP_HOST_EMU
#define APPT_WAVE_SYNC() emu_wave_sync()
AP_DEV ap_u64 appt_ballot(bool p) { return emu_ballot64(p); }
AP_DEV ap_u64 appt_first(ap_u64 v) { return emu_first_u64(v); }
AP_DEV int appt_prefix(ap_u64 m, int lane) { return __builtin_popcountll(m & ((1ull << lane) - 1ull)); }
AP_DEV int appt_popc(ap_u64 m) { return __builtin_popcountll(m); }
AP_DEV int appt_uniform(int x) { return x; }
#else
#define APPT_WAVE_SYNC()                                        \
    do {                                                        \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
        __builtin_amdgcn_wave_barrier();                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
    } while (0)
AP_DEV ap_u64 appt_ballot(bool p) { return __ballot(p); }
AP_DEV ap_u64 appt_first(ap_u64 v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return ((ap_u64)hi << 32) | lo;
}
AP_DEV int appt_prefix(ap_u64 m, int) { return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); }
AP_DEV int appt_popc(ap_u64 m) { return __popcll(m); }
AP_DEV int appt_uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }
#endif

// S[k] of one frame, `e` pointing at the frame's element of row k: the same expression as apch_value<1>
template <int KIND>
AP_DEV float appt_value(const float *e) {
    if (KIND == 0) return e[0];
    const float re = e[0], im = e[1];
    return sqrtf(fmaf(im, im, re * re));
}

// A wave hands its n staged records to its group's buffer: one atomic, then rows of 64 records.
AP_DEV void appt_flush(const ApPiptrackParams &P, int64_t g, const float *stage, int n, int lane) {
    APPT_WAVE_SYNC();
    ap_u64 base = 0;
    if (lane == 0) base = atomicAdd(P.counters + g, (ap_u64)n);
    base = appt_first(base);
    float *rec = P.records + g * P.capacity * 2;
    for (int i = lane; i < n; i += 64) {
        const ap_u64 slot = base + (ap_u64)i;
        if (slot < (ap_u64)P.capacity) {
            rec[slot * 2] = stage[2 * i];
            rec[slot * 2 + 1] = stage[2 * i + 1];
        }
    }
    APPT_WAVE_SYNC();                                       // the stage is free again
}

template <int KIND, bool COMPACT>
__global__ void __launch_bounds__(64 * APPT_WAVES) ap_piptrack_kernel(ApPiptrackParams P) {
    float *red = reinterpret_cast<float *>(ap_smem);           // [APPT_WAVES][64]
    const int lane = threadIdx.x & 63;
    const int wave = appt_uniform((int)(threadIdx.x >> 6));
    float *stage = red + APPT_WAVES * 64 + wave * (APPT_WCAP * 2);   // [APPT_WCAP][2] of this wave (COMPACT)
    const int F = P.F;
    const int64_t esz = KIND == 0 ? 1 : 2;
    const int64_t rs = P.in_rs * esz;
    const int nk = (F + APPT_WAVES - 1) / APPT_WAVES;
    const int k_beg = wave * nk;
    const int k_end = k_beg + nk < F ? k_beg + nk : F;         // may lie below k_beg: this wave has no bin
    for (int64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
        const int64_t b = tile / P.n_tt;
        const int64_t t0 = (tile - b * P.n_tt) * APPT_TT;
        const int64_t t = t0 + lane;
        const bool live = t < P.T;
        const int64_t tt = live ? t : P.T - 1;                 // a lane beyond the clip's end reads the last frame again
        const float *xl = P.S + (b * F * P.in_rs + tt) * esz;

        float rv;
        if (P.ref_mode == 0) {
            float m = -INFINITY;
            int k = k_beg;
            for (; k + APPT_U <= k_end; k += APPT_U) {
                float v[APPT_U];
#pragma unroll
                for (int u = 0; u < APPT_U; ++u) v[u] = appt_value<KIND>(xl + (int64_t)(k + u) * rs);
#pragma unroll
                for (int u = 0; u < APPT_U; ++u) m = v[u] > m ? v[u] : m;
            }
            for (; k < k_end; ++k) {
                const float v = appt_value<KIND>(xl + (int64_t)k * rs);
                m = v > m ? v : m;
            }
            red[wave * 64 + lane] = m;
            __syncthreads();
            m = red[lane];
#pragma unroll
            for (int q = 1; q < APPT_WAVES; ++q) { const float o = red[q * 64 + lane]; m = o > m ? o : m; }
            rv = P.threshold * m;
        } else if (P.ref_mode == 1) {
            rv = P.ref_value;
        } else {
            rv = fabsf(P.ref[b * P.T + tt]);
        }

        const int64_t g = P.per_clip ? b : 0;
        int n_w = 0;                                           // records staged by this wave: the same in every lane
        if (!COMPACT && wave == 0 && live) {
            const int64_t o = b * F * P.out_rs + t;
            P.pitches[o] = 0.0f;
            P.mags[o] = 0.0f;
        }
        const int ks = k_beg > 1 ? k_beg : 1;                  // bin 0 is never a peak: the walk starts at bin 1
        if (ks < k_end) {
            float a = appt_value<KIND>(xl + (int64_t)(ks - 1) * rs);
            float bv = appt_value<KIND>(xl + (int64_t)ks * rs);
            for (int k0 = ks; k0 < k_end; k0 += APPT_U) {
                float cv[APPT_U];
#pragma unroll
                for (int u = 0; u < APPT_U; ++u) {
                    const int kk = k0 + 1 + u < F ? k0 + 1 + u : F - 1;
                    cv[u] = appt_value<KIND>(xl + (int64_t)kk * rs);
                }
#pragma unroll
                for (int u = 0; u < APPT_U; ++u) {
                    const int k = k0 + u;
                    if (k < k_end) {
                        const float c = cv[u];                 // at k = F - 1 this is S[F - 1] again: X[k] >= X[k] holds
                        const float xa = a > rv ? a : 0.0f, xb = bv > rv ? bv : 0.0f, xc = c > rv ? c : 0.0f;
                        float avg = 0.0f, shift = 0.0f;
                        if (k + 1 < F) {
                            avg = 0.5f * (c - a);
                            float den = (2.0f * bv - c) - a;
                            den = den + (fabsf(den) < FLT_MIN ? 1.0f : 0.0f);
                            shift = avg / den;
                        }
                        const float dskew = (0.5f * avg) * shift;
                        const bool peak = xb > xa && xb >= xc && k >= P.k_lo && k < P.k_hi && live;
                        const float pitch = peak ? ((float)k + shift) * P.bin_hz : 0.0f;
                        const float mag = peak ? bv + dskew : 0.0f;
                        if (COMPACT) {
                            const bool keep = peak && pitch > 0.0f;
                            const ap_u64 mask = appt_ballot(keep);
                            if (mask) {
                                if (keep) {
                                    const int pos = n_w + appt_prefix(mask, lane);
                                    stage[2 * pos] = mag;
                                    stage[2 * pos + 1] = pitch;
                                }
                                n_w += appt_popc(mask);
                                if (n_w > APPT_WCAP - 64) {
                                    appt_flush(P, g, stage, n_w, lane);
                                    n_w = 0;
                                }
                            }
                        } else if (live) {
                            const int64_t o = (b * F + k) * P.out_rs + t;
                            P.pitches[o] = pitch;
                            P.mags[o] = mag;
                        }
                        a = bv;
                        bv = c;
                    }
                }
            }
        }
        if (COMPACT && n_w > 0) appt_flush(P, g, stage, n_w, lane);
        if (P.ref_mode == 0) __syncthreads();                  // the maxima are free for the next tile
    }
}

// The bin of numpy.histogram(r, edges) for the residual of frequency f, or -1 when f has none (f <= 0, NaN, inf).
AP_DEV int appt_residual_bin(float f, double bpo, const double *edges, int n_bins) {
    if (!(f > 0.0f)) return -1;
    const double x = bpo * log2((double)f / 27.5);
    double r = fmod(x, 1.0);
    if (r < 0.0) r += 1.0;
    if (r >= 0.5) r -= 1.0;
    if (!(r >= -0.5 && r <= 0.5)) return -1;
    int i = (int)((r + 0.5) * (double)n_bins);
    i = i < 0 ? 0 : i > n_bins - 1 ? n_bins - 1 : i;
    while (i > 0 && r < edges[i]) --i;
    while (i < n_bins - 1 && r >= edges[i + 1]) ++i;
    return i;
}

__global__ void __launch_bounds__(APPT_SEL_THREADS) ap_piptrack_tuning_kernel(ApTuningParams Q) {
    unsigned *hist = reinterpret_cast<unsigned *>(ap_smem);    // [256]
    unsigned *st = hist + 256;                                 // [8]: prefix, rank, equal keys at the rank, smallest key above
    unsigned *cnt = st + 8;                                    // [n_bins]
    const int tid = threadIdx.x;
    const int n_bins = Q.n_bins;
    for (int64_t g = blockIdx.x; g < Q.G; g += gridDim.x) {
        const ap_u64 n_all = Q.counters[g];
        if (n_all > (ap_u64)Q.capacity) continue;              // the buffer was too small: the host runs again
        const int64_t n = (int64_t)n_all;
        const float *rec = Q.records + g * Q.capacity * 2;
        for (int j = tid; j < n_bins; j += APPT_SEL_THREADS) cnt[j] = 0u;
        float thr = 0.0f;
        if (n > 0) {
            const int64_t r_lo = (n - 1) / 2, r_hi = n / 2;
            if (tid == 0) { st[0] = 0u; st[1] = (unsigned)r_lo; st[2] = 0u; st[3] = 0xFFFFFFFFu; }
            for (int pass = 3; pass >= 0; --pass) {
                const int sh = 8 * pass;
                for (int j = tid; j < 256; j += APPT_SEL_THREADS) hist[j] = 0u;
                __syncthreads();
                const unsigned prefix = st[0];
                for (int64_t i = tid; i < n; i += APPT_SEL_THREADS) {
                    const unsigned key = ap_fkey(rec[2 * i]);
                    if (pass == 3 || (key >> (sh + 8)) == (prefix >> (sh + 8))) atomicAdd(&hist[(key >> sh) & 255u], 1u);
                }
                __syncthreads();
                if (tid == 0) {
                    unsigned rank = st[1], cum = 0u;
                    int d = 0;
                    for (; d < 255; ++d) {
                        if (cum + hist[d] > rank) break;
                        cum += hist[d];
                    }
                    st[0] = prefix | ((unsigned)d << sh);
                    st[1] = rank - cum;
                    st[2] = hist[d];
                }
                __syncthreads();
            }
            const unsigned key_lo = st[0];
            unsigned key_hi = key_lo;
            if (r_hi != r_lo && st[1] + 1u >= st[2]) {         // the equal keys end at r_lo: the next larger key
                for (int64_t i = tid; i < n; i += APPT_SEL_THREADS) {
                    const unsigned key = ap_fkey(rec[2 * i]);
                    if (key > key_lo) atomicMin(&st[3], key);
                }
                __syncthreads();
                key_hi = st[3];
            }
            const float m_lo = ap_fkey_inv(key_lo), m_hi = ap_fkey_inv(key_hi);
            thr = r_hi == r_lo ? m_lo : (m_lo + m_hi) * 0.5f;
            for (int64_t i = tid; i < n; i += APPT_SEL_THREADS) {
                if (rec[2 * i] >= thr) {
                    const int j = appt_residual_bin(rec[2 * i + 1], Q.bpo, Q.edges, n_bins);
                    if (j >= 0) atomicAdd(&cnt[j], 1u);
                }
            }
        }
        __syncthreads();
        for (int j = tid; j < n_bins; j += APPT_SEL_THREADS) Q.counts[g * n_bins + j] = (ap_u64)cnt[j];
        if (tid == 0) Q.thr_out[g] = thr;
        __syncthreads();                                    // the histograms are free for the next group
    }
}

__global__ void __launch_bounds__(APPT_HIST_THREADS) ap_pitch_hist_kernel(ApPitchHistParams H) {
    unsigned *cnt = reinterpret_cast<unsigned *>(ap_smem);     // [n_bins]
    const int tid = threadIdx.x;
    for (int j = tid; j < H.n_bins; j += APPT_HIST_THREADS) cnt[j] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * APPT_HIST_THREADS + tid; i < H.n; i += (int64_t)gridDim.x * APPT_HIST_THREADS) {
        const int j = appt_residual_bin(H.f[i], H.bpo, H.edges, H.n_bins);
        if (j >= 0) atomicAdd(&cnt[j], 1u);
    }
    __syncthreads();
    for (int j = tid; j < H.n_bins; j += APPT_HIST_THREADS)
        if (cnt[j]) atomicAdd(H.counts + j, (ap_u64)cnt[j]);
}
