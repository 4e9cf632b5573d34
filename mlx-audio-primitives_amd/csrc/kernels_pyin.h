// Probabilistic YIN (pitch.py: pyin; the definition of DESIGN.md 9.17, stated in numpy by tests/pyin_ref.py).
//
// ap_pyin_observe_kernel.  The cumulative-mean-normalised difference curve d (B, n_lags, T) of yin_cmnd -> time-major log
//   emissions E (B, T, n_bins + 1) and voiced_prob (B, T).  A workgroup of four waves owns one clip and `ft` consecutive
//   frames: the (n_lags x ft) tile is read as segments of ft frames and turned in LDS (odd pitch), then a wave takes a
//   frame at a time.  Per frame, all in the wave's own LDS slice:
//     1  troughs: lanes over lags, ballot + prefix count compact the lags into tx[] in lag order, the heights into pp[];
//     2  lanes over thresholds: N_c = number of troughs below thr[c] (broadcast reads of the heights),
//        wc[c] = beta[c] nz[N_c] in float64;
//     3  lanes over troughs, 64 at a time in lag order, a serial loop over the thresholds: the ballot of "passes c" gives
//        every lane its rank among the passing troughs (prefix count + the count of the chunks before, base[c]) and
//        p += wc[c] ea[rank].  The sum runs over c ascending in float64 and is rounded once: a float32 product
//        beta nz ea underflows (e^-2k is below the smallest float32 from k = 52) and "p > 0", which decides whether a
//        trough is a candidate at all, must not depend on that;
//     4  the first lowest trough takes no_trough_prob times the beta mass of the thresholds it misses;
//     5  candidates (p > 0): parabolic shift, f0 and the bin in float64; owner[bin] = max trough index through an LDS
//        atomic max (the larger lag wins, nothing is summed, no order dependence);
//     6  lanes over bins: p of the owner (float32), the float32 sum of a lane's bins and one butterfly give
//        voiced_prob; E = logf(p + FLT_MIN), the last column logf((1 - voiced_prob) / n_bins + FLT_MIN).
//   Nothing a frame computes depends on the wave, the workgroup or the batch position it lands on.
//
// ap_pyin_decode_kernel.  One workgroup per sequence, one lane per pitch bin j (both voicing blocks).  Per step:
//     x[a,i] = (v[a,i] - m) - lz[i] as float2 (x[0,i], x[1,i]) in LDS, -inf in a margin of h bins on either side;  barrier
//     c[a,j] = max_i x[a,i] + lw[j - i] over i = j - h .. j + h ascending, first maximum: one 8-byte LDS read per two
//       candidates, lw at an address that depends on the loop counter alone (the same in every lane);
//     v'[b,j] = E + max(c[0,j] + ls[0][b], c[1,j] + ls[1][b]) (block 1 only when greater), pointer a n_bins + k[a,j]
//       as uint16; the wave maxima of v' go to LDS;  barrier
//   Two LDS-only barriers per step, the emissions of step t + 1 loaded during step t, back-pointer stores never waited
//   for before the backtrack, which stages APP_CHUNK rows in LDS as the dense decode does and writes states, f0 and the
//   voiced flag.  No multiplication in the recursion: the outputs equal the sequential float32 model in every bit.
#pragma once
#include <cfloat>
#include <climits>
#include <cmath>

#include "ap_launch.h"
#include "fft_lds.h"

extern __shared__ __attribute__((aligned(16))) char ap_smem[];

#define APP_MAX_BINS 1024        // pitch bins (2048 states: uint16 pointers, one lane per bin)
#define APP_MAX_HALF 512         // half-width h of the transition band (W <= 1025)
#define APP_MAX_STEPS (1 << 20)  // the cap of the sequence decoders
#define APP_MAX_LAGS 4096
#define APP_OBS_WAVES 4
#define APP_OBS_THREADS (64 * APP_OBS_WAVES)
#define APP_CHUNK 16             // rows of back-pointers staged per backtrack chunk

struct ApPyinObsParams {
    const float *d;              // (B, n_lags, T)
    const float *thr, *beta;     // (n)
    const float *ea, *nz;        // (kmax + 1): ea[rank], nz[N]
    float *E;                    // (B, T, n_bins + 1)
    float *vp;                   // (B, T)
    double sr, fmin, bin_scale;
    int64_t B, T, n_tt, n_items;
    float no_trough;
    int n_lags, lo, n, n_bins, kmax, ft, pitch;
    int off_thr, off_beta, off_ea, off_nz, off_wave, wave_bytes, off_pp, off_owner, off_wc, off_base, lds_bytes;
};

struct ApPyinDecParams {
    const float *E;              // (B, T, nb + 1)
    const float *lw;             // (2 h + 1): lw[d + h]
    const float *lz;             // (nb)
    const float *ls;             // (4): [a][b]
    const float *freq;           // (nb)
    uint16_t *ptr;               // (B, T, 2 nb)
    int32_t *states;             // (B, T)
    float *f0;                   // (B, T)
    uint8_t *voiced;             // (B, T)
    double *logp;                // (B)
    int64_t B, T;
    float li, fill;
    int use_fill, nb, h, threads, off_v, off_wmax, off_stage, off_chunk, lds_bytes;
};

static inline int ap_prepare_pyin_observe(ApPyinObsParams &P, const float *d, int64_t B, int n_lags, int64_t T, int lo, double sr,
                                          double fmin, int bins_per_semitone, int n_bins, const float *thr, const float *beta, int n,
                                          const float *ea, const float *nz, int n_tab, float no_trough, float *E, float *vp) {
    if (!d || !thr || !beta || !ea || !nz || !E || !vp) AP_FAIL(AP_ERR_INVALID, "pyin_observe: NULL buffer");
    if (B <= 0 || T <= 0 || n_lags < 2 || lo < 1)
        AP_FAIL(AP_ERR_INVALID, "pyin_observe: needs B, T >= 1, n_lags >= 2, lo >= 1, got (%lld, %lld, %d, %d)", (long long)B, (long long)T, n_lags, lo);
    if (!(sr > 0.0) || !(fmin > 0.0) || bins_per_semitone < 1 || n_bins < 1 || n < 1 || !(no_trough >= 0.0f))
        AP_FAIL(AP_ERR_INVALID, "pyin_observe: sr, fmin, bins_per_semitone, n_bins, n_thresholds must be positive, no_trough_prob >= 0");
    if (n_lags > APP_MAX_LAGS) AP_FAIL(AP_ERR_UNSUPPORTED, "pyin_observe: n_lags must not exceed %d, got %d", APP_MAX_LAGS, n_lags);
    if (n_bins > APP_MAX_BINS) AP_FAIL(AP_ERR_UNSUPPORTED, "pyin_observe: n_bins must not exceed %d, got %d", APP_MAX_BINS, n_bins);
    if (T > APP_MAX_STEPS) AP_FAIL(AP_ERR_UNSUPPORTED, "pyin_observe: T must not exceed %d, got %lld", APP_MAX_STEPS, (long long)T);
    if ((double)B * (double)T * ((double)n_lags + n_bins + 1) * 4.0 > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "pyin_observe: more than 2^63 bytes");
    const int kmax = (n_lags + 1) / 2;                          // troughs are at least two lags apart
    if (n_tab < kmax + 1) AP_FAIL(AP_ERR_INVALID, "pyin_observe: the Boltzmann tables need %d entries, got %d", kmax + 1, n_tab);
    P.d = d; P.thr = thr; P.beta = beta; P.ea = ea; P.nz = nz; P.E = E; P.vp = vp;
    P.sr = sr; P.fmin = fmin; P.bin_scale = 12.0 * bins_per_semitone;
    P.B = B; P.T = T; P.no_trough = no_trough;
    P.n_lags = n_lags; P.lo = lo; P.n = n; P.n_bins = n_bins; P.kmax = kmax;
    P.pitch = (n_lags + 2) | 1;
    // a wave's slice: tx uint16 [kmax], pp double [kmax], owner int [n_bins], wc double [n], base int [n]
    P.off_pp = ap_align16(kmax * 2);
    P.off_owner = P.off_pp + ap_align16(kmax * 8);
    P.off_wc = P.off_owner + ap_align16(n_bins * 4);
    P.off_base = P.off_wc + ap_align16(n * 8);
    P.wave_bytes = P.off_base + ap_align16(n * 4);
    const int64_t tables = 2 * (int64_t)ap_align16(n * 4) + 2 * (int64_t)ap_align16((kmax + 1) * 4) + (int64_t)APP_OBS_WAVES * P.wave_bytes;
    // 16 frames per tile (64-byte segments of d) where the workgroup then stays within 64 KB, fewer for long curves
    int ft = 16;
    while (ft > 1 && tables + ap_align16(ft * P.pitch * 4) > (ft > 4 ? 64 * 1024 : AP_LDS_MAX)) ft >>= 1;
    if (tables + ap_align16(ft * P.pitch * 4) > AP_LDS_MAX)
        AP_FAIL(AP_ERR_UNSUPPORTED, "pyin_observe: n_lags = %d with %d thresholds does not fit the %d KiB of LDS", n_lags, n, AP_LDS_MAX / 1024);
    P.ft = ft;
    P.off_thr = ap_align16(ft * P.pitch * 4);
    P.off_beta = P.off_thr + ap_align16(n * 4);
    P.off_ea = P.off_beta + ap_align16(n * 4);
    P.off_nz = P.off_ea + ap_align16((kmax + 1) * 4);
    P.off_wave = P.off_nz + ap_align16((kmax + 1) * 4);
    P.lds_bytes = P.off_wave + APP_OBS_WAVES * P.wave_bytes;
    P.n_tt = (T + ft - 1) / ft;
    P.n_items = B * P.n_tt;
    return AP_OK;
}

static inline int ap_prepare_pyin_decode(ApPyinDecParams &P, const float *E, int64_t B, int nb, int64_t T, const float *lw, int h,
                                         const float *lz, const float *ls, float li, const float *freq, int use_fill, float fill,
                                         uint16_t *ptr, int32_t *states, float *f0, uint8_t *voiced, double *logp) {
    if (!E || !lw || !lz || !ls || !freq || !ptr || !states || !f0 || !voiced || !logp) AP_FAIL(AP_ERR_INVALID, "pyin_decode: NULL buffer");
    if (B <= 0 || nb <= 0 || T <= 0 || h < 0)
        AP_FAIL(AP_ERR_INVALID, "pyin_decode: the emissions must be non-empty and the half-width >= 0, got (%lld, %lld, %d, %d)", (long long)B,
                (long long)T, nb, h);
    if (nb > APP_MAX_BINS) AP_FAIL(AP_ERR_UNSUPPORTED, "pyin_decode: n_bins must not exceed %d, got %d", APP_MAX_BINS, nb);
    if (h > APP_MAX_HALF) AP_FAIL(AP_ERR_UNSUPPORTED, "pyin_decode: the half-width must not exceed %d, got %d", APP_MAX_HALF, h);
    if (T > APP_MAX_STEPS) AP_FAIL(AP_ERR_UNSUPPORTED, "pyin_decode: T must not exceed %d, got %lld", APP_MAX_STEPS, (long long)T);
    if ((double)B * (double)T * (double)(nb + 1) * 4.0 > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "pyin_decode: more than 2^63 bytes");
    P.E = E; P.lw = lw; P.lz = lz; P.ls = ls; P.freq = freq; P.ptr = ptr; P.states = states; P.f0 = f0; P.voiced = voiced; P.logp = logp;
    P.B = B; P.T = T; P.li = li; P.fill = fill; P.use_fill = use_fill ? 1 : 0; P.nb = nb; P.h = h;
    P.threads = (nb + 63) & ~63;
    // x float2 [nb + 2 h], the final v [2 nb], the wave maxima [16], the staged states [APP_CHUNK] and the carried one,
    // a chunk of back-pointers [APP_CHUNK][2 nb] uint16
    P.off_v = ap_align16((nb + 2 * h) * 8);
    P.off_wmax = P.off_v + ap_align16(2 * nb * 4);
    P.off_stage = P.off_wmax + 16 * 4;
    P.off_chunk = P.off_stage + ap_align16((APP_CHUNK + 1) * 4);
    P.lds_bytes = P.off_chunk + ap_align16(APP_CHUNK * 2 * nb * 2);
    return AP_OK;
}

static inline int ap_pyin_grid(int64_t n, int64_t cap) {
    if (cap <= 0 || cap > (1 << 20)) cap = 1 << 20;
    return (int)(n < cap ? n : cap);
}

#define APP_WAVE_SYNC()                                         \
    do {                                                        \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
        __builtin_amdgcn_wave_barrier();                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
    } while (0)

AP_DEV int app_prefix(unsigned long long m) { return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); }
AP_DEV float app_max(float a, float b) { return b > a ? b : a; }
AP_DEV float app_wave_max(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = app_max(x, __shfl_xor(x, o, 64));
    return x;
}

// ---------------------------------------------------------------------------------------------------------------------
// observations
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(APP_OBS_THREADS) ap_pyin_observe_kernel(ApPyinObsParams P) {
    float *tile = reinterpret_cast<float *>(ap_smem);                           // [ft][pitch]
    float *thr = reinterpret_cast<float *>(ap_smem + P.off_thr);
    float *beta = reinterpret_cast<float *>(ap_smem + P.off_beta);
    float *ea = reinterpret_cast<float *>(ap_smem + P.off_ea);
    float *nz = reinterpret_cast<float *>(ap_smem + P.off_nz);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    char *mine = ap_smem + P.off_wave + wave * P.wave_bytes;
    uint16_t *tx = reinterpret_cast<uint16_t *>(mine);                          // [kmax] trough lags, in lag order
    double *pp = reinterpret_cast<double *>(mine + P.off_pp);                   // [kmax] heights, then probabilities
    int *owner = reinterpret_cast<int *>(mine + P.off_owner);                   // [n_bins] trough that holds the bin, -1: none
    double *wc = reinterpret_cast<double *>(mine + P.off_wc);                   // [n] beta[c] nz[N_c]
    int *base = reinterpret_cast<int *>(mine + P.off_base);                     // [n] passing troughs in the chunks before
    const int n = P.n, n_lags = P.n_lags, n_bins = P.n_bins, ft = P.ft, pitch = P.pitch;
    for (int c = tid; c < n; c += APP_OBS_THREADS) { thr[c] = P.thr[c]; beta[c] = P.beta[c]; }
    for (int k = tid; k <= P.kmax; k += APP_OBS_THREADS) { ea[k] = P.ea[k]; nz[k] = P.nz[k]; }
    for (int64_t item = blockIdx.x; item < P.n_items; item += gridDim.x) {
        const int64_t b = item / P.n_tt, t0 = (item - b * P.n_tt) * ft;
        const float *db = P.d + b * n_lags * P.T;
        __syncthreads();                                        // the tables are there; the tile is free
        for (int idx = tid; idx < ft * n_lags; idx += APP_OBS_THREADS) {
            const int f = idx & (ft - 1), x = idx / ft;
            if (t0 + f < P.T) tile[f * pitch + x] = db[(int64_t)x * P.T + t0 + f];
        }
        __syncthreads();
        for (int f = wave; f < ft && t0 + f < P.T; f += APP_OBS_WAVES) {
            const float *row = tile + f * pitch;
            const int64_t t = t0 + f;
            // 1  troughs, compacted in lag order
            int K = 0;
            for (int x0 = 0; x0 < n_lags; x0 += 64) {
                const int x = x0 + lane;
                bool tr = false;
                if (x < n_lags) {
                    const float c = row[x];
                    if (x == 0) tr = c < row[1];
                    else if (x == n_lags - 1) tr = c < row[x - 1];
                    else tr = c < row[x - 1] && c <= row[x + 1];
                }
                const unsigned long long m = __ballot(tr);
                if (tr) {
                    const int k = K + app_prefix(m);
                    tx[k] = (uint16_t)x;
                    pp[k] = (double)row[x];
                }
                K += __popcll(m);
            }
            APP_WAVE_SYNC();
            // 2  how many troughs pass each threshold
            for (int c = lane; c < n; c += 64) {
                const float th = thr[c];
                int N = 0;
                for (int k = 0; k < K; ++k) N += (float)pp[k] < th ? 1 : 0;
                wc[c] = (double)beta[c] * (double)nz[N];
                base[c] = 0;
            }
            APP_WAVE_SYNC();
            // 3  the probability of every trough; the first lowest trough on the way
            float bh = INFINITY;
            int bk = 0;
            for (int k0 = 0; k0 < K; k0 += 64) {
                const int k = k0 + lane;
                const bool act = k < K;
                const float hgt = act ? (float)pp[k] : INFINITY;
                const bool more = k0 + 64 < K;
                double p = 0.0;
                for (int c = 0; c < n; ++c) {
                    const bool pass = hgt < thr[c];
                    const unsigned long long m = __ballot(pass);
                    const int bs = base[c];
                    if (pass) p += wc[c] * (double)ea[bs + app_prefix(m)];
                    if (more && lane == 0) base[c] = bs + __popcll(m);
                }
                if (act) pp[k] = p;
                if (act && hgt < bh) { bh = hgt; bk = k; }
                APP_WAVE_SYNC();
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float oh = __shfl_xor(bh, o, 64);
                const int ok = __shfl_xor(bk, o, 64);
                if (oh < bh || (oh == bh && ok < bk)) { bh = oh; bk = ok; }
            }
            // 4  the mass of the thresholds that the lowest trough misses
            if (K > 0) {
                double s = 0.0;
                for (int c = lane; c < n; c += 64) s += bh < thr[c] ? 0.0 : (double)beta[c];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
                if (lane == 0) pp[bk] = pp[bk] + (double)P.no_trough * s;
            }
            for (int j = lane; j < n_bins; j += 64) owner[j] = -1;
            APP_WAVE_SYNC();
            // 5  candidates to bins
            for (int k = lane; k < K; k += 64) {
                if (pp[k] > 0.0) {
                    const int x = tx[k];
                    double shift = 0.0;
                    if (x > 0 && x < n_lags - 1) {
                        const double dm = (double)row[x - 1], d0 = (double)row[x], dp = (double)row[x + 1];
                        const double a = dp + dm - 2.0 * d0, bb = (dp - dm) / 2.0;
                        if (fabs(bb) < fabs(a)) shift = -bb / a;
                    }
                    const double f0 = P.sr / ((double)(P.lo + x) + shift);
                    double r = rint(P.bin_scale * log2(f0 / P.fmin));
                    r = r < 0.0 ? 0.0 : (r > (double)n_bins ? (double)n_bins : r);
                    const int bin = (int)r;
                    if (bin < n_bins) atomicMax(owner + bin, k);
                }
            }
            APP_WAVE_SYNC();
            // 6  voiced probability and emissions
            float *Er = P.E + (b * P.T + t) * (n_bins + 1);
            float s = 0.0f;
            for (int j = lane; j < n_bins; j += 64) {
                const int o = owner[j];
                const float p = o >= 0 ? (float)pp[o] : 0.0f;
                s += p;
                Er[j] = logf(p + FLT_MIN);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            const float v = fminf(fmaxf(s, 0.0f), 1.0f);
            if (lane == 0) {
                P.vp[b * P.T + t] = v;
                Er[n_bins] = logf((1.0f - v) / (float)n_bins + FLT_MIN);
            }
            APP_WAVE_SYNC();                                    // the slice is free for the wave's next frame
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// banded two-block decode
// ---------------------------------------------------------------------------------------------------------------------
// state s of frame o: the state itself, the voiced flag and the frequency of its bin (unvoiced: `fill` when asked for)
AP_DEV void app_emit_state(const ApPyinDecParams &P, int64_t o, int s) {
    const bool unv = s >= P.nb;
    P.states[o] = s;
    P.voiced[o] = unv ? 0 : 1;
    P.f0[o] = (unv && P.use_fill) ? P.fill : P.freq[unv ? s - P.nb : s];
}

__global__ void __launch_bounds__(1024) ap_pyin_decode_kernel(ApPyinDecParams P) {
    const int nb = P.nb, h = P.h, S = 2 * nb, W = 2 * h + 1;
    float2 *xs = reinterpret_cast<float2 *>(ap_smem);                           // [nb + 2 h]: bin i at h + i
    float *vfin = reinterpret_cast<float *>(ap_smem + P.off_v);                 // [2 nb] the final v
    float *wmax = reinterpret_cast<float *>(ap_smem + P.off_wmax);              // [16]
    int *stage = reinterpret_cast<int *>(ap_smem + P.off_stage);                // [APP_CHUNK] states, [APP_CHUNK]: the carried one
    uint32_t *chunk = reinterpret_cast<uint32_t *>(ap_smem + P.off_chunk);      // [APP_CHUNK][2 nb] uint16
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
    const bool ok = tid < nb;
    const int j = ok ? tid : nb - 1;                            // idle lanes compute the last bin again and store nothing
    const float ninf = -INFINITY;
    for (int i = tid; i < h; i += blockDim.x) {
        xs[i] = make_float2(ninf, ninf);
        xs[h + nb + i] = make_float2(ninf, ninf);
    }
    const float lzj = P.lz[j];
    const float ls00 = P.ls[0], ls01 = P.ls[1], ls10 = P.ls[2], ls11 = P.ls[3];
    const float *__restrict__ lw = P.lw;
    const int q_first = h - j > 0 ? h - j : 0;                  // the first in-band source, as an offset from j - h
    for (int64_t b = blockIdx.x; b < P.B; b += gridDim.x) {
        const float *Eb = P.E + b * P.T * (nb + 1);
        uint16_t *Pb = P.ptr + b * P.T * S;
        // step 0
        float v0 = Eb[j] + P.li, v1 = Eb[nb] + P.li;
        if (ok) { Pb[j] = 0; Pb[nb + j] = 0; }
        float lm = app_wave_max(ok ? app_max(v0, v1) : ninf);
        if (lane == 0) wmax[wave] = lm;
        AP_LDS_BARRIER();
        double acc = 0.0;
        float e_next = P.T > 1 ? Eb[(nb + 1) + j] : 0.0f, u_next = P.T > 1 ? Eb[(nb + 1) + nb] : 0.0f;
        for (int64_t t = 1; t < P.T; ++t) {
            float m = wmax[0];
            for (int w = 1; w < n_waves; ++w) m = app_max(m, wmax[w]);
            if (tid == 0) acc += (double)m;
            if (ok) xs[h + j] = make_float2((v0 - m) - lzj, (v1 - m) - lzj);
            const float e = e_next, u = u_next;
            const int64_t tn = t + 1 < P.T ? t + 1 : t;         // (the last step loads its own row again)
            e_next = Eb[tn * (nb + 1) + j];
            u_next = Eb[tn * (nb + 1) + nb];
            AP_LDS_BARRIER();                                   // x is complete; the maxima have been read
            const float2 *xw = xs + j;                          // source i = j - h + q sits at xw[q]
            float c0 = ninf, c1 = ninf;
            int q0 = q_first, q1 = q_first;
            int q = 0;
            for (; q + 4 <= W; q += 4) {
                float2 x[4];
                float l[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { x[r] = xw[q + r]; l[r] = lw[2 * h - q - r]; }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float a0 = x[r].x + l[r], a1 = x[r].y + l[r];
                    const bool w0 = a0 > c0, w1 = a1 > c1;
                    c0 = w0 ? a0 : c0; q0 = w0 ? q + r : q0;
                    c1 = w1 ? a1 : c1; q1 = w1 ? q + r : q1;
                }
            }
            for (; q < W; ++q) {
                const float2 x = xw[q];
                const float l = lw[2 * h - q];
                const float a0 = x.x + l, a1 = x.y + l;
                if (a0 > c0) { c0 = a0; q0 = q; }
                if (a1 > c1) { c1 = a1; q1 = q; }
            }
            const int k0 = j - h + q0, k1 = nb + j - h + q1;
            const float a00 = c0 + ls00, a10 = c1 + ls10, a01 = c0 + ls01, a11 = c1 + ls11;
            const bool s0 = a10 > a00, s1 = a11 > a01;
            v0 = e + (s0 ? a10 : a00);
            v1 = u + (s1 ? a11 : a01);
            if (ok) {
                Pb[t * S + j] = (uint16_t)(s0 ? k1 : k0);
                Pb[t * S + nb + j] = (uint16_t)(s1 ? k1 : k0);
            }
            lm = app_wave_max(ok ? app_max(v0, v1) : ninf);
            if (lane == 0) wmax[wave] = lm;
            AP_LDS_BARRIER();                                   // the maxima are complete; x has been read
        }
        if (ok) { vfin[j] = v0; vfin[nb + j] = v1; }
        __syncthreads();                                        // the final v and every back-pointer of the sequence are written
        if (tid == 0) {
            float m = wmax[0];
            for (int w = 1; w < n_waves; ++w) m = app_max(m, wmax[w]);
            acc += (double)m;
            float bv = vfin[0];
            int bs = 0;
            for (int s = 1; s < S; ++s) {
                const float x = vfin[s];
                if (x > bv) { bv = x; bs = s; }
            }
            P.logp[b] = acc + (double)(bv - m);
            app_emit_state(P, b * P.T + (P.T - 1), bs);
            stage[APP_CHUNK] = bs;
        }
        // the backtrack: rows (lo, hi] of back-pointers give the states lo .. hi - 1
        for (int64_t hi = P.T - 1; hi > 0; hi -= APP_CHUNK) {
            const int64_t lo = hi - APP_CHUNK < 0 ? 0 : hi - APP_CHUNK;
            const int n = (int)(hi - lo);
            const uint32_t *rows = reinterpret_cast<const uint32_t *>(Pb + (lo + 1) * S);     // (S is even: whole words)
            for (int idx = tid; idx < n * nb; idx += blockDim.x) chunk[idx] = rows[idx];
            __syncthreads();
            if (tid == 0) {
                const uint16_t *ch = reinterpret_cast<const uint16_t *>(chunk);
                int s = stage[APP_CHUNK];
                for (int r = n - 1; r >= 0; --r) {
                    s = ch[r * S + s];
                    stage[r] = s;
                }
                stage[APP_CHUNK] = s;
            }
            __syncthreads();
            if (tid < n) app_emit_state(P, b * P.T + lo + tid, stage[tid]);
        }
        __syncthreads();                                        // x, the maxima and the stage are free for the next sequence
    }
}
