// Phase vocoder (effects.py: phase_vocoder, time_stretch, pitch_shift; the definition of librosa 0.10's phase_vocoder).
//
// ap_pv_kernel.  For one row D[0 .. T-1] of complex64 (columns T and T + 1 read as zero), rate > 0 and
// k = 0 .. T_out - 1, T_out = ceil(T / rate) in float64 (len(np.arange(0, T, rate))):
//   pos_k = (double)k rate,  i_k = floor(pos_k),  a_k = pos_k - i_k
//   mag_k = (1 - a_k) |D[i_k]| + a_k |D[i_k + 1]|
//   out_k = mag_k P_k,  P_0 = u[0],  P_k = P_(k-1) u[i_(k-1) + 1] conj(u[i_(k-1)]),  u[c] = D[c] / |D[c]| (1 where D[c] = 0)
// librosa accumulates angles, acc += phi + wrap(angle(D[i+1]) - angle(D[i]) - phi); wrap removes multiples of 2 pi only,
// so exp(j acc) is the running product above and phi (with it hop_length and n_fft) drops out.  The product needs no
// atan2 / sin / cos and is an associative scan: q_0 = u[0], q_k = u[i_(k-1) + 1] conj(u[i_(k-1)]), P_k = q_0 q_1 .. q_k.
//
//   Lanes run along time: a chunk is 64 output steps of one row, one coalesced 512-byte store.  For a chunk the wave
//   loads the input columns [i_(k0-1), i_(k0+63) + 1] once, coalesced, computes (|D|, u) once per column and parks them
//   in LDS (APPV_SPAN columns at a time; a faster rate takes several sub-spans); each lane then picks its columns
//   i_(k-1), i_(k-1) + 1, i_k, i_k + 1.  q goes through a six-level inclusive complex product across the wave and
//   is multiplied by the carry, one unit phasor kept in registers and renormalised once per chunk so that its length
//   does not drift with T_out.
//   W = 1: a workgroup's APPV_WAVES waves own whole rows and share nothing.  W > 1 (few long rows): the W waves of a
//   workgroup own one row and take W consecutive chunks at a time; the chunk totals go through LDS (double-buffered, one
//   barrier per W chunks) and every wave multiplies the carry by the totals before its own, in the same order, so all
//   waves hold the same carry.  The bits depend on W, never on the run, the row's place or the batch.
//   u is formed on (re, im) scaled by the power of two of max(|re|, |im|): re^2 + im^2 neither underflows nor overflows.
//   -0.0 + 0j has magnitude zero and gets u = 1 like +0.0 (NumPy's angle is pi there).
#pragma once
#include <cmath>

#include "ap_launch.h"
#include "fft_lds.h"

#define APPV_WAVES 4            // W = 1: waves per workgroup, each owns whole rows
#define APPV_SPAN 128           // input columns staged in LDS per wave at a time
#define APPV_WMAX 16
#define APPV_ROWS_FULL 4096     // rows from which one wave per row fills the chip

struct ApPvParams {
    const ap_float2 *D;         // (rows, rs_in)
    ap_float2 *out;             // (rows, rs_out)
    int64_t rows, rs_in, rs_out;
    int T, T_out, W;
    double rate;
};

// len(np.arange(0, T, rate)): ceil(T / rate) in float64; 0 for T <= 0, -1 when rate is not a positive finite number or
// the length does not fit 2^62
static inline int64_t ap_pv_frames(int64_t T, double rate) {
    if (!(rate > 0.0) || !std::isfinite(rate)) return -1;
    if (T <= 0) return 0;
    const double n = std::ceil((double)T / rate);
    if (!(n < 4.0e18)) return -1;
    return (int64_t)n;
}

// Waves per row from the row count and the row's own chunk count: more waves only while rows alone leave the chip
// idle and every wave still gets at least two chunks.
static inline int ap_pv_waves(int64_t rows, int64_t T_out) {
    // AP_PV_WAVES = 1 / 4 / 16 in the environment overrides the rule (tools/pv_bench.py times the variants with it)
    static const int force = std::getenv("AP_PV_WAVES") ? std::atoi(std::getenv("AP_PV_WAVES")) : 0;
    if (force == 1 || force == 4 || force == 16) return force;
    const int64_t chunks = (T_out + 63) / 64;
    const int64_t want = (APPV_ROWS_FULL + rows - 1) / rows;
    if (want > 4 && chunks >= 2 * 16) return 16;
    if (want > 1 && chunks >= 2 * 4) return 4;
    return 1;
}

// Validation and launch geometry of ap_phase_vocoder_f32.
static inline int ap_prepare_pv(ApPvParams &P, const float *D, int64_t rows, int64_t T, int64_t rs_in, double rate, int64_t T_out,
                                float *out, int64_t rs_out) {
    if (!D || !out) AP_FAIL(AP_ERR_INVALID, "phase_vocoder: NULL buffer");
    if (!(rate > 0.0) || !std::isfinite(rate)) AP_FAIL(AP_ERR_INVALID, "rate must be a positive number");
    if (rows <= 0 || T <= 0) AP_FAIL(AP_ERR_INVALID, "phase_vocoder: D must be non-empty, got (%lld, %lld)", (long long)rows, (long long)T);
    const int64_t want = ap_pv_frames(T, rate);
    if (T_out != want) AP_FAIL(AP_ERR_INVALID, "phase_vocoder: T_out mismatch (got %lld, expected %lld)", (long long)T_out, (long long)want);
    if (rs_in < T || rs_out < T_out)
        AP_FAIL(AP_ERR_INVALID, "phase_vocoder: row strides (%lld, %lld) must be >= (T, T_out) = (%lld, %lld)", (long long)rs_in,
                (long long)rs_out, (long long)T, (long long)T_out);
    // 32-bit column and step arithmetic; element offsets are 64-bit
    if (T > (1 << 28) || T_out > (1 << 28)) AP_FAIL(AP_ERR_UNSUPPORTED, "phase_vocoder: T and T_out must be <= 2^28");
    if (rs_in > ((int64_t)1 << 40) || rs_out > ((int64_t)1 << 40) || rows > ((int64_t)1 << 40))
        AP_FAIL(AP_ERR_UNSUPPORTED, "phase_vocoder: extents too large");
    if ((double)rows * (double)(rs_in > rs_out ? rs_in : rs_out) * 8.0 > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "phase_vocoder: more than 2^63 bytes");
    const uintptr_t pi = reinterpret_cast<uintptr_t>(D), po = reinterpret_cast<uintptr_t>(out);
    const uintptr_t ni = (uintptr_t)(((rows - 1) * rs_in + T) * 8), no = (uintptr_t)(((rows - 1) * rs_out + T_out) * 8);
    if (pi < po + no && po < pi + ni) AP_FAIL(AP_ERR_INVALID, "phase_vocoder: the output overlaps the input");
    P.D = reinterpret_cast<const ap_float2 *>(D);
    P.out = reinterpret_cast<ap_float2 *>(out);
    P.rows = rows; P.rs_in = rs_in; P.rs_out = rs_out;
    P.T = (int)T; P.T_out = (int)T_out; P.rate = rate;
    P.W = ap_pv_waves(rows, T_out);
    return AP_OK;
}

static inline int ap_pv_grid(const ApPvParams &P) {
    const int64_t g = P.W == 1 ? (P.rows + APPV_WAVES - 1) / APPV_WAVES : P.rows;
    return (int)(g < (1 << 20) ? g : (1 << 20));
}

#ifndef AP_HOST_EMU
// LDS traffic inside one wave: program order is enough for the hardware, the fences are for the compiler
#define APPV_WAVE_SYNC()                                        \
    do {                                                        \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
        __builtin_amdgcn_wave_barrier();                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
    } while (0)

AP_DEV ap_float2 appv_mul(ap_float2 a, ap_float2 b) {
    ap_float2 r;
    r.x = a.x * b.x - a.y * b.y;
    r.y = a.x * b.y + a.y * b.x;
    return r;
}

AP_DEV ap_float2 appv_mul_conj(ap_float2 a, ap_float2 b) {      // a conj(b)
    ap_float2 r;
    r.x = a.x * b.x + a.y * b.y;
    r.y = a.y * b.x - a.x * b.y;
    return r;
}

// (|d|, d / |d|); (0, 1) for a zero of either sign.  The pair is scaled by 2^-e, e the exponent of max(|re|, |im|), so
// that the larger part lies in [0.5, 1) and the squared length in [0.25, 2).
AP_DEV void appv_polar(ap_float2 d, float &mag, ap_float2 &u) {
    const float s = fmaxf(fabsf(d.x), fabsf(d.y));
    mag = 0.0f;
    u.x = 1.0f; u.y = 0.0f;
    if (s > 0.0f) {
        int e;
        (void)frexpf(s, &e);
        const float x = ldexpf(d.x, -e), y = ldexpf(d.y, -e);
        const float r = sqrtf(x * x + y * y);
        u.x = x / r; u.y = y / r;
        mag = ldexpf(r, e);
    }
}

AP_DEV ap_float2 appv_unit(ap_float2 p) {                      // |p| is 1 to a few roundings
    const float inv = 1.0f / sqrtf(p.x * p.x + p.y * p.y);
    p.x *= inv; p.y *= inv;
    return p;
}

template <int W>
__global__ void __launch_bounds__(64 * (W == 1 ? APPV_WAVES : W)) ap_pv_kernel(ApPvParams P) {
    constexpr int NW = W == 1 ? APPV_WAVES : W;
    constexpr int TEAMS = NW / W;                               // rows in flight per workgroup
    __shared__ float s_mag[NW][APPV_SPAN];
    __shared__ ap_float2 s_u[NW][APPV_SPAN];
    __shared__ ap_float2 s_tot[2][NW];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int w = wave % W;                                     // place in the row's team
    float *lm = s_mag[wave];
    ap_float2 *lu = s_u[wave];
    const int n_chunks = (P.T_out + 63) >> 6;
    const int n_steps = (n_chunks + W - 1) / W;                 // W chunks per step
    for (int64_t row = (int64_t)blockIdx.x * TEAMS + wave / W; row < P.rows; row += (int64_t)gridDim.x * TEAMS) {
        const ap_float2 *Dr = P.D + row * P.rs_in;
        ap_float2 *Or = P.out + row * P.rs_out;
        ap_float2 carry;
        carry.x = 1.0f; carry.y = 0.0f;
        for (int step = 0; step < n_steps; ++step) {
            const int k0 = (step * W + w) << 6;
            const int k = k0 + lane;
            const bool live = k < P.T_out;
            // columns: ca = i_(k-1) (-1 in front of the row: u = 1), cb = i_k; a dead lane multiplies by 1
            const double pos = (double)k * P.rate;
            const int cb = live ? (int)floor(pos) : -4;
            const float a = live ? (float)(pos - floor(pos)) : 0.0f;
            const int ca = (live && k > 0) ? (int)floor((double)(k - 1) * P.rate) : (live ? -1 : -4);
            float m0 = 0.0f, m1 = 0.0f;
            ap_float2 ua, ub;
            ua.x = 1.0f; ua.y = 0.0f; ub = ua;
            if (k0 < P.T_out) {                                 // wave-uniform
                const int kl = min(k0 + 63, P.T_out - 1);
                const int lo = k0 > 0 ? (int)floor((double)(k0 - 1) * P.rate) : 0;
                int hi = (int)floor((double)kl * P.rate) + 1;
                if (hi > P.T - 1) hi = P.T - 1;                 // the columns behind the row are zero: (0, 1), as initialised
                for (int base = lo; base <= hi; base += APPV_SPAN) {
                    const int n = min(APPV_SPAN, hi - base + 1);
                    APPV_WAVE_SYNC();                           // the sub-span before has been read
                    for (int j = lane; j < n; j += 64) {
                        float mg;
                        ap_float2 uu;
                        appv_polar(Dr[base + j], mg, uu);       // base + j <= hi <= T - 1
                        lm[j] = mg;
                        lu[j] = uu;
                    }
                    APPV_WAVE_SYNC();
                    int j = ca - base;
                    if (j >= 0 && j < n) ua = lu[j];
                    j = ca + 1 - base;
                    if (ca >= -1 && j >= 0 && j < n) ub = lu[j];
                    j = cb - base;
                    if (j >= 0 && j < n) m0 = lm[j];
                    j = cb + 1 - base;
                    if (cb >= 0 && j >= 0 && j < n) m1 = lm[j];
                }
            }
            ap_float2 p = appv_mul_conj(ub, ua);                // q_k
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                ap_float2 up;
                up.x = __shfl_up(p.x, s, 64);
                up.y = __shfl_up(p.y, s, 64);
                if (lane >= s) p = appv_mul(up, p);
            }
            ap_float2 tot;
            tot.x = __shfl(p.x, 63, 64);
            tot.y = __shfl(p.y, 63, 64);
            ap_float2 before = carry;                           // the product in front of this wave's chunk
            if (W > 1) {
                if (lane == 0) s_tot[step & 1][w] = tot;
                __syncthreads();
                ap_float2 run = carry;
#pragma unroll
                for (int v = 0; v < W; ++v) {
                    if (v == w) before = run;
                    run = appv_mul(run, s_tot[step & 1][v]);
                }
                carry = appv_unit(run);
            } else {
                carry = appv_unit(appv_mul(carry, tot));
            }
            if (live) {
                p = appv_mul(before, p);
                const float mag = (1.0f - a) * m0 + a * m1;
                ap_float2 o;
                o.x = mag * p.x; o.y = mag * p.y;
                Or[k] = o;
            }
        }
        if (W > 1) __syncthreads();                             // the next row's first totals reuse s_tot[0]
    }
}
#endif  // AP_HOST_EMU
