// Hidden-Markov sequence decoding (sequence.py: viterbi, viterbi_discriminative, viterbi_binary; the definition of
// DESIGN.md 9.12, stated in numpy by tests/viterbi_ref.py).
//
// ap_viterbi_emission_kernel.  prob (B, S, T), rows rs apart -> time-major log emissions, tiny = FLT_MIN:
//   mode 0   E[b,t,j]   = logf(p + tiny)
//   mode 1   E[b,t,j]   = logf(p + tiny) - lps[j]
//   mode 2   E[b,t,l,1] = logf(p + tiny) - lps[l,1],   E[b,t,l,0] = logf((1 - p) + tiny) - lps[l,0]
//   A workgroup owns one sequence and 64 steps and walks the states in tiles of 64: a tile is read as row segments of
//   64 steps, turned in LDS (pitch 65: both sides free of bank conflicts) and leaves as segments of 64 states.  The
//   flag word of the sequence takes bit 0 when a value is NaN or outside [0, 1] and, in mode 1, bit 1 when a column
//   sum (float64, ascending states per quarter, the quarters in order) is not within 1e-8 + 1e-5 of 1 (numpy's
//   allclose, librosa's test).  The only logf of the decoders is taken here.
//
// ap_viterbi_decode_kernel.  One workgroup per sequence, v double-buffered in LDS.  At step t every destination state j
//   takes the first maximum over i of (v[i] - m) + lt[i,j], m the maximum of the step before (the renormalisation is
//   applied where v is read: the same bits as a stored v - m, one pass less); lt is read row-wise, lanes running over j,
//   v[i] is a broadcast read.  With S below the block G lanes share a state (lane g takes i = g, g + G, ...) and meet
//   in a (value, index) reduction through LDS that keeps the smallest index on ties.  A lane loads APV_UNROLL rows of lt
//   for all its (up to 4: NP) states before it uses the first, and a whole block of rows is taken with straight-line
//   selects.  v'[j] = E[t,j] + best, E[t] loaded during step t - 1; the block maximum of v' goes through one wave
//   reduction and four LDS words.  One LDS-only barrier per step (two with G > 1): the back-pointer stores are never
//   waited for until the backtrack.  LT_LDS: lt lives in LDS (S <= the threshold the host passes).  The backtrack
//   stages APV_CHUNK rows of back-pointers in LDS, one lane walks them and the states leave as one segment per chunk.
//   m is summed in time order in float64 by lane 0.
//
// ap_viterbi_binary_kernel.  One lane per (sequence, label) chain of two states, lanes over labels (the time-major
//   reads are segments), 16 steps of emissions in flight.  Two pointer bits per step, 16 steps to a word of the scratch
//   (B, ceil(T / 16), S); the same lane walks its words back, 64 steps of 64 labels are turned in LDS and leave as rows.
//
// No multiplication anywhere in the recursions: nothing for a compiler to contract, every + and - is one rounded
// float32 operation and the outputs equal the sequential float32 model in every bit.
#pragma once
#include <cfloat>
#include <climits>
#include <cmath>

#include "ap_launch.h"
#include "fft_lds.h"

extern __shared__ __attribute__((aligned(16))) char ap_smem[];

#define APV_THREADS 256          // the decode and the emission workgroup
#define APV_WAVES (APV_THREADS / 64)
#define APV_MAX_STATES 1024      // cap on S of the dense decode (back-pointers are uint16, v and a chunk fit 48 KB)
#define APV_MAX_STEPS (1 << 20)  // cap on T
#define APV_MAX_G 16             // lanes that share a destination state, at most
#define APV_UNROLL 16            // rows of lt in flight per lane and pass
#define APV_CHUNK 16             // rows of back-pointers staged per backtrack chunk
#define APV_LT_LDS_MAX 176       // lt may live in LDS up to this S (121 KB of the CU's 160)
#define APVE_TILE 64             // the emission tile: 64 states x 64 steps
#define APVE_PITCH 65
#define APVB_WORD 16             // steps per packed word of the binary decode
#define APVB_TILE 64             // labels of a wave = steps per output tile
#define APVB_PITCH 65
#define APV_FLAG_RANGE 1
#define APV_FLAG_COLSUM 2

static_assert(APV_MAX_STATES <= 65536, "back-pointers are uint16");
static_assert(APV_MAX_STATES <= 4 * APV_THREADS, "the decode kernel is instantiated for up to 4 passes");
static_assert(APV_LT_LDS_MAX < APV_THREADS, "lt in LDS is the one-pass kernel");
static_assert(APV_LT_LDS_MAX * APV_LT_LDS_MAX * 4 + (APV_CHUNK + 4) * APV_LT_LDS_MAX * 2 + 4096 <= AP_LDS_MAX, "lt, v and a chunk fit the LDS");
static_assert(APVB_TILE % APVB_WORD == 0, "whole words per output tile");

struct ApViterbiEmisParams {
    const float *prob;          // (B, S, rs)
    const float *lps;           // NULL, (S) or (S, 2)
    float *E;                   // (B, T, S) or (B, T, S, 2)
    int32_t *flags;             // (B)
    int64_t B, S, T, rs, n_tt, n_items;
    int mode, lds_bytes;
};

struct ApViterbiDecParams {
    const float *E;             // (B, T, S)
    const float *lt;            // (S, S)
    const float *li;            // (S)
    uint16_t *ptr;              // (B, T, S)
    int32_t *states;            // (B, T)
    double *logp;               // (B)
    int64_t B, T;
    int S, nj, G, n_pass, lt_lds, off_chunk, off_lt, lds_bytes;
};

struct ApViterbiBinParams {
    const float *E;             // (B, T, S, 2)
    const float *lt;            // (4) or (S, 4): [i][j] of every label
    const float *li;            // (S, 2)
    uint32_t *bits;             // (B, n_words, S)
    int32_t *states;            // (B, S, T)
    double *logp;               // (B, S)
    int64_t B, S, T, n_words, n_lt, n_items;
    int per_label, lds_bytes;
};

static inline int ap_prepare_viterbi_emission(ApViterbiEmisParams &P, const float *prob, int64_t B, int64_t S, int64_t T, int64_t rs,
                                              int mode, const float *lps, float *E, int32_t *flags) {
    if (!prob || !E || !flags) AP_FAIL(AP_ERR_INVALID, "viterbi_emission: NULL buffer");
    if (B <= 0 || S <= 0 || T <= 0)
        AP_FAIL(AP_ERR_INVALID, "viterbi_emission: prob must be non-empty, got (%lld, %lld, %lld)", (long long)B, (long long)S, (long long)T);
    if (mode < 0 || mode > 2) AP_FAIL(AP_ERR_INVALID, "viterbi_emission: unknown mode %d (0 viterbi, 1 discriminative, 2 binary)", mode);
    if (mode != 0 && !lps) AP_FAIL(AP_ERR_INVALID, "viterbi_emission: mode %d needs the log state priors", mode);
    if (rs < T) AP_FAIL(AP_ERR_INVALID, "viterbi_emission: row_stride (%lld) must be >= T = %lld", (long long)rs, (long long)T);
    if (T > APV_MAX_STEPS) AP_FAIL(AP_ERR_UNSUPPORTED, "viterbi_emission: T must not exceed %d", APV_MAX_STEPS);
    if ((double)B * (double)S * (double)rs * 4.0 > 9.0e18 || (double)B * (double)S * (double)T * 8.0 > 9.0e18)
        AP_FAIL(AP_ERR_UNSUPPORTED, "viterbi_emission: more than 2^63 bytes");
    P.prob = prob; P.lps = lps; P.E = E; P.flags = flags;
    P.B = B; P.S = S; P.T = T; P.rs = rs; P.mode = mode;
    P.n_tt = (T + APVE_TILE - 1) / APVE_TILE;
    P.n_items = B * P.n_tt;
    P.lds_bytes = 2 * APVE_TILE * APVE_PITCH * 4 + APV_WAVES * APVE_TILE * 8;
    return AP_OK;
}

// lt_lds_max: lt is kept in LDS when S does not exceed it (0: never; at most APV_LT_LDS_MAX)
static inline int ap_prepare_viterbi_decode(ApViterbiDecParams &P, const float *E, int64_t B, int64_t S, int64_t T, const float *lt,
                                            const float *li, uint16_t *ptr, int32_t *states, double *logp, int lt_lds_max) {
    if (!E || !lt || !li || !ptr || !states || !logp) AP_FAIL(AP_ERR_INVALID, "viterbi_decode: NULL buffer");
    if (B <= 0 || S <= 0 || T <= 0)
        AP_FAIL(AP_ERR_INVALID, "viterbi_decode: the emissions must be non-empty, got (%lld, %lld, %lld)", (long long)B, (long long)T, (long long)S);
    if (S > APV_MAX_STATES) AP_FAIL(AP_ERR_UNSUPPORTED, "viterbi_decode: S must not exceed %d, got %lld", APV_MAX_STATES, (long long)S);
    if (T > APV_MAX_STEPS) AP_FAIL(AP_ERR_UNSUPPORTED, "viterbi_decode: T must not exceed %d, got %lld", APV_MAX_STEPS, (long long)T);
    if ((double)B * (double)T * (double)S * 4.0 > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "viterbi_decode: more than 2^63 bytes");
    P.E = E; P.lt = lt; P.li = li; P.ptr = ptr; P.states = states; P.logp = logp;
    P.B = B; P.T = T; P.S = (int)S;
    P.nj = P.S < APV_THREADS ? P.S : APV_THREADS;
    P.G = APV_THREADS / P.nj;
    if (P.G > P.S) P.G = P.S;
    if (P.G > APV_MAX_G) P.G = APV_MAX_G;
    P.n_pass = (P.S + APV_THREADS - 1) / APV_THREADS;
    if (lt_lds_max > APV_LT_LDS_MAX) lt_lds_max = APV_LT_LDS_MAX;
    P.lt_lds = P.S <= lt_lds_max ? 1 : 0;
    // v [2][S], the wave maxima [2][APV_WAVES], the reduction (value, index) [APV_THREADS] each, the staged states
    // [APV_CHUNK] and the carried state, then the chunk [APV_CHUNK][S] uint16 and lt [S][S]
    P.off_chunk = ap_align16(2 * P.S * 4 + 2 * APV_WAVES * 4 + 2 * APV_THREADS * 4 + (APV_CHUNK + 1) * 4);
    P.off_lt = P.off_chunk + ap_align16(APV_CHUNK * P.S * 2);
    P.lds_bytes = P.off_lt + (P.lt_lds ? P.S * P.S * 4 : 0);
    return AP_OK;
}

static inline int ap_prepare_viterbi_binary(ApViterbiBinParams &P, const float *E, int64_t B, int64_t S, int64_t T, const float *lt,
                                            int per_label, const float *li, uint32_t *bits, int32_t *states, double *logp) {
    if (!E || !lt || !li || !bits || !states || !logp) AP_FAIL(AP_ERR_INVALID, "viterbi_binary: NULL buffer");
    if (B <= 0 || S <= 0 || T <= 0)
        AP_FAIL(AP_ERR_INVALID, "viterbi_binary: the emissions must be non-empty, got (%lld, %lld, %lld)", (long long)B, (long long)T, (long long)S);
    if (T > APV_MAX_STEPS) AP_FAIL(AP_ERR_UNSUPPORTED, "viterbi_binary: T must not exceed %d, got %lld", APV_MAX_STEPS, (long long)T);
    if ((double)B * (double)T * (double)S * 8.0 > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "viterbi_binary: more than 2^63 bytes");
    P.E = E; P.lt = lt; P.li = li; P.bits = bits; P.states = states; P.logp = logp;
    P.B = B; P.S = S; P.T = T; P.per_label = per_label ? 1 : 0;
    P.n_words = (T + APVB_WORD - 1) / APVB_WORD;
    P.n_lt = (S + APVB_TILE - 1) / APVB_TILE;
    if ((double)B * (double)P.n_lt > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "viterbi_binary: too many chains");
    P.n_items = B * P.n_lt;
    P.lds_bytes = APVB_TILE * APVB_PITCH * 4;
    return AP_OK;
}

static inline int ap_viterbi_grid(int64_t n) { return (int)(n < (1 << 20) ? n : (1 << 20)); }

// The larger of two values, the first on a tie (and whenever the second is a NaN); the maximum of a wave; an integer
// flag raised from any thread.
AP_DEV float apv_max(float a, float b) { return b > a ? b : a; }
#ifdef AP_HOST_EMU
AP_DEV float apv_wave_max(float x) {
    emu_xchg[threadIdx.x] = x;
    emu_wave_sync();
    const unsigned base = threadIdx.x & ~63u;
    float m = emu_xchg[base];
    for (int q = 1; q < 64; ++q) m = apv_max(m, emu_xchg[base + q]);
    emu_wave_sync();
    return m;
}
AP_DEV void apv_flag_or(int32_t *p, int32_t bits) { __atomic_fetch_or(p, bits, __ATOMIC_RELAXED); }
#else
AP_DEV float apv_wave_max(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = apv_max(x, __shfl_xor(x, o, 64));
    return x;
}
AP_DEV void apv_flag_or(int32_t *p, int32_t bits) { atomicOr(p, bits); }
#endif

// ---------------------------------------------------------------------------------------------------------------------
// emission
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(APV_THREADS) ap_viterbi_emission_kernel(ApViterbiEmisParams P) {
    float *tile0 = reinterpret_cast<float *>(ap_smem);                          // [64 states][APVE_PITCH]
    float *tile1 = tile0 + APVE_TILE * APVE_PITCH;                              // state 1 of the binary mode
    double *cs = reinterpret_cast<double *>(tile1 + APVE_TILE * APVE_PITCH);    // [APV_WAVES][64 steps]
    const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
    const float tiny = FLT_MIN;
    for (int64_t item = blockIdx.x; item < P.n_items; item += gridDim.x) {
        const int64_t b = item / P.n_tt, t0 = (item - b * P.n_tt) * APVE_TILE;
        const float *Pb = P.prob + b * P.S * P.rs;
        double colsum = 0.0;
        bool bad = false;
        for (int64_t s0 = 0; s0 < P.S; s0 += APVE_TILE) {
            // lane = step: a row of the tile is one segment of prob
#pragma unroll 4
            for (int k = 0; k < APVE_TILE / APV_WAVES; ++k) {
                const int r = q + APV_WAVES * k;
                const int64_t s = s0 + r, t = t0 + c;
                if (s < P.S && t < P.T) {
                    const float p = Pb[s * P.rs + t];
                    bad = bad || !(p >= 0.0f && p <= 1.0f);
                    colsum += (double)p;
                    float e = logf(p + tiny);
                    if (P.mode == 1) e = e - P.lps[s];
                    if (P.mode == 2) {
                        e = e - P.lps[2 * s + 1];
                        tile0[r * APVE_PITCH + c] = logf((1.0f - p) + tiny) - P.lps[2 * s];
                        tile1[r * APVE_PITCH + c] = e;
                    } else {
                        tile0[r * APVE_PITCH + c] = e;
                    }
                }
            }
            __syncthreads();
            // lane = state: a row of the output is one segment of E
#pragma unroll 4
            for (int k = 0; k < APVE_TILE / APV_WAVES; ++k) {
                const int r = q + APV_WAVES * k;
                const int64_t s = s0 + c, t = t0 + r;
                if (s < P.S && t < P.T) {
                    const int64_t o = (b * P.T + t) * P.S + s;
                    if (P.mode == 2) {
                        P.E[2 * o] = tile0[c * APVE_PITCH + r];
                        P.E[2 * o + 1] = tile1[c * APVE_PITCH + r];
                    } else {
                        P.E[o] = tile0[c * APVE_PITCH + r];
                    }
                }
            }
            __syncthreads();                                    // the tile is free for the next one
        }
        if (bad) apv_flag_or(P.flags + b, APV_FLAG_RANGE);
        if (P.mode == 1) {
            cs[q * 64 + c] = colsum;
            __syncthreads();
            if (q == 0 && t0 + c < P.T) {
                const double sum = ((cs[c] + cs[64 + c]) + cs[128 + c]) + cs[192 + c];
                if (!(fabs(sum - 1.0) <= 1e-8 + 1e-5)) apv_flag_or(P.flags + b, APV_FLAG_COLSUM);
            }
            __syncthreads();                                    // the sums are free for the next item
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// dense decode
// ---------------------------------------------------------------------------------------------------------------------
template <bool LT_LDS, int NP>
__global__ void __launch_bounds__(APV_THREADS) ap_viterbi_decode_kernel(ApViterbiDecParams P) {
    const int S = P.S, nj = P.nj, G = P.G;
    float *v = reinterpret_cast<float *>(ap_smem);              // [2][S]
    float *wmax = v + 2 * S;                                    // [2][APV_WAVES]
    float *redv = wmax + 2 * APV_WAVES;                         // [APV_THREADS]
    int *redi = reinterpret_cast<int *>(redv + APV_THREADS);    // [APV_THREADS]
    int *stage = redi + APV_THREADS;                            // [APV_CHUNK] states of a chunk, [APV_CHUNK]: the carried state
    uint16_t *chunk = reinterpret_cast<uint16_t *>(ap_smem + P.off_chunk);     // [APV_CHUNK][S]
    const float *lts = reinterpret_cast<const float *>(ap_smem + P.off_lt);    // [S][S]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int jl = tid % nj, g = tid / nj;
    const bool part = g < G;                                    // the lane takes candidates
    const bool owner = g == 0;                                  // the lane finishes its states
    if (LT_LDS) {
        float *w = reinterpret_cast<float *>(ap_smem + P.off_lt);
        for (int idx = tid; idx < S * S; idx += APV_THREADS) w[idx] = P.lt[idx];
        __syncthreads();
    }
    const float *LT = LT_LDS ? lts : P.lt;
    for (int64_t b = blockIdx.x; b < P.B; b += gridDim.x) {
        const float *Eb = P.E + b * P.T * S;
        uint16_t *Pb = P.ptr + b * P.T * S;
        // step 0
        float lm = -INFINITY;
        for (int j = tid; j < S; j += APV_THREADS) {
            const float x = Eb[j] + P.li[j];
            v[j] = x;
            Pb[j] = 0;
            lm = apv_max(lm, x);
        }
        lm = apv_wave_max(lm);
        if (lane == 0) wmax[wave] = lm;
        AP_LDS_BARRIER();
        double acc = 0.0;
        // the emissions of a step are loaded one step ahead: their latency would otherwise be most of a step of a small model
        float e[NP], e_next[NP];
        int jc[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int j = jl + p * APV_THREADS;
            jc[p] = j < S ? j : 0;
            e_next[p] = (owner && P.T > 1) ? Eb[S + jc[p]] : 0.0f;
        }
        for (int64_t t = 1; t < P.T; ++t) {
            const int cur = (int)((t - 1) & 1);
            const float *vp = v + cur * S;
            float *vn = v + (cur ^ 1) * S;
            const float *wm = wmax + cur * APV_WAVES;
            const float m = apv_max(apv_max(wm[0], wm[1]), apv_max(wm[2], wm[3]));
            if (tid == 0) acc += (double)m;
            lm = -INFINITY;
            float best[NP];
            int bi[NP];
            const int64_t tn = t + 1 < P.T ? t + 1 : t;         // (the last step loads its own row again)
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                e[p] = e_next[p];
                e_next[p] = owner ? Eb[tn * S + jc[p]] : 0.0f;
                best[p] = -INFINITY;
                bi[p] = g < S ? g : 0;
            }
            if (part) {
                // APV_UNROLL rows of lt at a time: NP x APV_UNROLL independent loads are in flight before the first is used
                for (int i0 = g; i0 < S; i0 += G * APV_UNROLL) {
                    float l[NP][APV_UNROLL];
#pragma unroll
                    for (int u = 0; u < APV_UNROLL; ++u) {
                        const int i = i0 + u * G;
                        const int row = (i < S ? i : g) * S;
#pragma unroll
                        for (int p = 0; p < NP; ++p) l[p][u] = LT[row + jc[p]];
                    }
                    if (i0 + (APV_UNROLL - 1) * G < S) {        // a whole block: straight-line selects
#pragma unroll
                        for (int u = 0; u < APV_UNROLL; ++u) {
                            const int i = i0 + u * G;
                            const float x = vp[i] - m;
#pragma unroll
                            for (int p = 0; p < NP; ++p) {
                                const float cand = x + l[p][u];
                                const bool win = cand > best[p];
                                best[p] = win ? cand : best[p];
                                bi[p] = win ? i : bi[p];
                            }
                        }
                    } else {
#pragma unroll
                        for (int u = 0; u < APV_UNROLL; ++u) {
                            const int i = i0 + u * G;
                            if (i < S) {
                                const float x = vp[i] - m;
#pragma unroll
                                for (int p = 0; p < NP; ++p) {
                                    const float cand = x + l[p][u];
                                    if (cand > best[p]) { best[p] = cand; bi[p] = i; }
                                }
                            }
                        }
                    }
                }
            }
            if (G > 1) {                                        // (G > 1 means S < APV_THREADS: one pass)
                if (part) { redv[g * nj + jl] = best[0]; redi[g * nj + jl] = bi[0]; }
                AP_LDS_BARRIER();
                if (owner) {
                    for (int k = 1; k < G; ++k) {
                        const float cand = redv[k * nj + jl];
                        const int ci = redi[k * nj + jl];
                        if (cand > best[0] || (cand == best[0] && ci < bi[0])) { best[0] = cand; bi[0] = ci; }
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int j = jl + p * APV_THREADS;
                if (owner && j < S) {
                    const float x = e[p] + best[p];
                    vn[j] = x;
                    Pb[t * S + j] = (uint16_t)bi[p];
                    lm = apv_max(lm, x);
                }
            }
            lm = apv_wave_max(lm);
            if (lane == 0) wmax[(cur ^ 1) * APV_WAVES + wave] = lm;
            AP_LDS_BARRIER();
        }
        // the last state: the first maximum of the final v; logp
        {
            const int cur = (int)((P.T - 1) & 1);
            if (tid == 0) {
                const float *vf = v + cur * S;
                const float *wm = wmax + cur * APV_WAVES;
                const float m = apv_max(apv_max(wm[0], wm[1]), apv_max(wm[2], wm[3]));
                acc += (double)m;
                float bv = vf[0];
                int bs = 0;
                for (int j = 1; j < S; ++j) {
                    const float x = vf[j];
                    if (x > bv) { bv = x; bs = j; }
                }
                P.logp[b] = acc + (double)(bv - m);
                P.states[b * P.T + (P.T - 1)] = bs;
                stage[APV_CHUNK] = bs;
            }
        }
        __syncthreads();                                        // every back-pointer of the sequence is written
        // the backtrack: rows (lo, hi] of back-pointers give the states lo .. hi - 1
        for (int64_t hi = P.T - 1; hi > 0; hi -= APV_CHUNK) {
            const int64_t lo = hi - APV_CHUNK < 0 ? 0 : hi - APV_CHUNK;
            const int n = (int)(hi - lo);
            const uint16_t *rows = Pb + (lo + 1) * S;
            for (int idx = tid; idx < n * S; idx += APV_THREADS) chunk[idx] = rows[idx];
            __syncthreads();
            if (tid == 0) {
                int s = stage[APV_CHUNK];
                for (int r = n - 1; r >= 0; --r) {
                    s = chunk[r * S + s];
                    stage[r] = s;
                }
                stage[APV_CHUNK] = s;
            }
            __syncthreads();
            if (tid < n) P.states[b * P.T + lo + tid] = stage[tid];
        }
        __syncthreads();                                        // v, the maxima and the stage are free for the next sequence
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// binary decode
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) ap_viterbi_binary_kernel(ApViterbiBinParams P) {
    int *tile = reinterpret_cast<int *>(ap_smem);               // [64 labels][APVB_PITCH]
    const int lane = threadIdx.x & 63;
    const int64_t S = P.S, T = P.T;
    for (int64_t item = blockIdx.x; item < P.n_items; item += gridDim.x) {
        const int64_t b = item / P.n_lt, l0 = (item - b * P.n_lt) * APVB_TILE;
        const int64_t l = l0 + lane;
        const bool ok = l < S;
        const int64_t lc = ok ? l : S - 1;                      // idle lanes compute the last label again and store nothing
        const float *ltp = P.lt + (P.per_label ? lc * 4 : 0);
        const float t00 = ltp[0], t01 = ltp[1], t10 = ltp[2], t11 = ltp[3];
        const float *Eb = P.E + (b * T * S + lc) * 2;            // a step is 2 S floats further
        uint32_t *Wb = P.bits + b * P.n_words * S + lc;         // a word is S words further
        float v0 = Eb[0] + P.li[2 * lc], v1 = Eb[1] + P.li[2 * lc + 1];
        float m = apv_max(v0, v1);
        v0 -= m; v1 -= m;
        double acc = (double)m;
        for (int64_t w = 0; w < P.n_words; ++w) {
            float e0[APVB_WORD], e1[APVB_WORD];
#pragma unroll
            for (int u = 0; u < APVB_WORD; ++u) {
                const int64_t t = w * APVB_WORD + u;
                const int64_t tc = t < T ? t : T - 1;
                e0[u] = Eb[tc * S * 2];
                e1[u] = Eb[tc * S * 2 + 1];
            }
            uint32_t word = 0;
#pragma unroll
            for (int u = 0; u < APVB_WORD; ++u) {
                const int64_t t = w * APVB_WORD + u;
                if (t >= 1 && t < T) {
                    const float c00 = v0 + t00, c10 = v1 + t10, c01 = v0 + t01, c11 = v1 + t11;
                    const uint32_t p0 = c10 > c00 ? 1u : 0u, p1 = c11 > c01 ? 1u : 0u;
                    const float n0 = e0[u] + (p0 ? c10 : c00), n1 = e1[u] + (p1 ? c11 : c01);
                    m = apv_max(n0, n1);
                    v0 = n0 - m; v1 = n1 - m;
                    acc += (double)m;
                    word |= (p0 | (p1 << 1)) << (2 * u);
                }
            }
            if (ok) Wb[w * S] = word;
        }
        int s = v1 > v0 ? 1 : 0;
        if (ok) P.logp[b * S + l] = acc + (double)(s ? v1 : v0);
        // the backtrack: 64 steps at a time, from the end
        for (int64_t t0 = ((T - 1) / APVB_TILE) * APVB_TILE; t0 >= 0; t0 -= APVB_TILE) {
            uint32_t wd[APVB_TILE / APVB_WORD];
#pragma unroll
            for (int k = 0; k < APVB_TILE / APVB_WORD; ++k) {
                const int64_t w = t0 / APVB_WORD + k;
                wd[k] = Wb[(w < P.n_words ? w : P.n_words - 1) * S];      // the lane's own stores
            }
#pragma unroll
            for (int k = APVB_TILE / APVB_WORD - 1; k >= 0; --k) {
#pragma unroll
                for (int u = APVB_WORD - 1; u >= 0; --u) {
                    const int64_t t = t0 + k * APVB_WORD + u;
                    if (t < T) {
                        tile[lane * APVB_PITCH + k * APVB_WORD + u] = s;
                        if (t >= 1) s = (int)((wd[k] >> (2 * u + s)) & 1u);
                    }
                }
            }
            __syncthreads();
            for (int r = 0; r < APVB_TILE; ++r) {
                const int64_t lab = l0 + r, t = t0 + lane;
                if (lab < S && t < T) P.states[(b * S + lab) * T + t] = tile[r * APVB_PITCH + lane];
            }
            __syncthreads();                                    // the tile is free for the next one
        }
    }
}
