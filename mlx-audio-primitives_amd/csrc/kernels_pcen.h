// Per-channel energy normalisation (pcen.py: pcen, streaming.py: StreamingPCEN; the definition of librosa.pcen,
// Wang et al. 2017).
//
// ap_pcen_kernel.  For S (B, M, T) >= 0, b in [0, 1], a = 1 - b, 1 <= max_size <= 255:
//   R[m,t]   = ref[m,t] when a reference is given, else max S[r(j, M), t] over j in [m - max_size/2, m + (max_size-1)/2]
//              (r: SciPy's mode="reflect"; scipy.ndimage.maximum_filter1d along m; max_size = 1: S itself)
//   Msm[t]   = b R[t] + a Msm[t-1],  a Msm[-1] = zi          (scipy.signal.lfilter([b], [1, b - 1], R, zi=zi))
//   smooth   = (eps + Msm)^-gain
//   out      = (S smooth + bias)^power - bias^power  as  bias^power expm1(power log1p(S smooth / bias))   APPC_GENERAL
//            = log1p(S smooth)                                                                            APPC_LOG   (power = 0)
//            = (S smooth)^power                                                                           APPC_POWER (bias = 0)
//   zf       = a Msm[T-1]
//
//   One wave per (clip, band) row, lane = frame: a tile of 64 frames is one coalesced 256-byte load and one store, the
//   smoother never reaches memory.  Inside a tile v = b R goes through an inclusive Hillis-Steele scan,
//   v += a^(2^j) lane_up(v, 2^j) for j = 0 .. 5, then the frames before the tile come in as one term:
//   Msm = v + a^lane zi in the first tile, v + a^(lane+1) Msm[last frame of the tile before] in the others.  The powers
//   a^0 .. a^64 are float32 roundings of float64 powers built on the host (ApPcenParams::apow), not float32 products,
//   so a term that is n frames old carries O(log n) roundings inside a tile plus three per tile crossed instead of n.
//   The waves of a workgroup share nothing: no LDS, no barrier.  max_size > 1 reads the window's rows at the lane's
//   frame, coalesced like the row itself; the neighbouring rows are in the cache, their own waves read them too.
//   A NaN in S reaches the frames from its own on, in the rows whose window holds it, and nothing else.
#pragma once
#include <cmath>

#include "ap_launch.h"
#include "fft_lds.h"

#define APPC_WAVES 4            // waves per workgroup; every wave owns whole rows
#define APPC_TT 64              // frames per tile: the lanes of a wave
#define APPC_KMAX 255
#define APPC_GENERAL 0
#define APPC_LOG 1
#define APPC_POWER 2

struct ApPcenParams {
    const float *S, *ref, *zi;  // (rows, rs_in), (rows, rs_ref) or NULL, (rows) or NULL
    float *out, *zf;            // (rows, rs_out), (rows) or NULL
    int64_t rows, rs_in, rs_ref, rs_out;
    int M, T, max_size, n_tt, chain;
    float b, a, gain, inv_bias, power, eps, scale, zi0;     // scale = bias^power, zi0 = 1 - b (the state without zi)
    float apow[APPC_TT + 1];    // a^k, 0 <= k <= 64, each rounded from the float64 power
};

static inline bool ap_pcen_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

// Validation, the power table and the launch geometry of ap_pcen_f32 (and of its emulator twin).
static inline int ap_prepare_pcen(ApPcenParams &P, const float *S, int64_t B, int64_t M, int64_t T, int64_t rs_in, const float *ref,
                                  int64_t rs_ref, int max_size, double b, float gain, float bias, float power, float eps,
                                  const float *zi, float *out, int64_t rs_out, float *zf) {
    if (!S || !out) AP_FAIL(AP_ERR_INVALID, "pcen: NULL buffer");
    if (B <= 0 || M <= 0 || T <= 0) AP_FAIL(AP_ERR_INVALID, "pcen: S must be non-empty, got (%lld, %lld, %lld)", (long long)B, (long long)M, (long long)T);
    if (!(b >= 0.0 && b <= 1.0)) AP_FAIL(AP_ERR_INVALID, "b must lie in [0, 1], got %g", b);
    if (b == 0.0 && !zi) AP_FAIL(AP_ERR_INVALID, "b = 0 needs zi: the steady state of the smoother is undefined");
    if (!(gain >= 0.0f)) AP_FAIL(AP_ERR_INVALID, "gain must be non-negative, got %g", (double)gain);
    if (!(bias >= 0.0f)) AP_FAIL(AP_ERR_INVALID, "bias must be non-negative, got %g", (double)bias);
    if (!(power >= 0.0f)) AP_FAIL(AP_ERR_INVALID, "power must be non-negative, got %g", (double)power);
    if (!(eps >= 1.17549435e-38f)) AP_FAIL(AP_ERR_INVALID, "eps must be a positive normal float32 (>= 1.1755e-38), got %g", (double)eps);
    if (max_size < 1 || max_size > APPC_KMAX) AP_FAIL(AP_ERR_INVALID, "max_size must be an integer in 1 .. 255, got %d", max_size);
    if (rs_in < T || rs_out < T || (ref && rs_ref < T))
        AP_FAIL(AP_ERR_INVALID, "pcen: row strides (%lld, %lld, %lld) must be >= T = %lld", (long long)rs_in, (long long)rs_ref, (long long)rs_out, (long long)T);
    // 32-bit (m, t) and reflect arithmetic; element offsets are 64-bit
    if (M > (1 << 28) || T > (1 << 28)) AP_FAIL(AP_ERR_UNSUPPORTED, "pcen: M and T must be <= 2^28");
    if (rs_in > ((int64_t)1 << 40) || rs_ref > ((int64_t)1 << 40) || rs_out > ((int64_t)1 << 40) || B > ((int64_t)1 << 32))
        AP_FAIL(AP_ERR_UNSUPPORTED, "pcen: extents too large");
    int64_t rs_max = rs_in > rs_out ? rs_in : rs_out;
    if (rs_ref > rs_max) rs_max = rs_ref;
    if ((double)B * (double)M * (double)rs_max * 4.0 > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "pcen: more than 2^63 bytes");
    const int64_t rows = B * M;
    // exact extents: the padding behind the last row belongs to nobody
    const int64_t out_bytes = ((rows - 1) * rs_out + T) * 4;
    if (ap_pcen_overlap(S, ((rows - 1) * rs_in + T) * 4, out, out_bytes) ||
        (ref && ap_pcen_overlap(ref, ((rows - 1) * rs_ref + T) * 4, out, out_bytes)))
        AP_FAIL(AP_ERR_INVALID, "pcen: the output overlaps an input");
    if (zf && (ap_pcen_overlap(zf, rows * 4, out, out_bytes) || ap_pcen_overlap(zf, rows * 4, S, ((rows - 1) * rs_in + T) * 4) ||
               (zi && ap_pcen_overlap(zf, rows * 4, zi, rows * 4))))
        AP_FAIL(AP_ERR_INVALID, "pcen: zf overlaps another buffer");
    P.S = S; P.ref = ref; P.zi = zi; P.out = out; P.zf = zf;
    P.rows = rows; P.rs_in = rs_in; P.rs_ref = ref ? rs_ref : 0; P.rs_out = rs_out;
    P.M = (int)M; P.T = (int)T; P.max_size = max_size;
    P.n_tt = (int)((T + APPC_TT - 1) / APPC_TT);
    P.chain = power == 0.0f ? APPC_LOG : (bias == 0.0f ? APPC_POWER : APPC_GENERAL);
    const double a = 1.0 - b;
    P.b = (float)b; P.a = (float)a; P.zi0 = (float)a;
    P.gain = gain; P.power = power; P.eps = eps;
    P.inv_bias = bias > 0.0f ? (float)(1.0 / (double)bias) : 0.0f;
    P.scale = (float)std::pow((double)bias, (double)power);
    for (int k = 0; k <= APPC_TT; ++k) P.apow[k] = (float)std::pow(a, (double)k);      // pow(0, 0) = 1
    return AP_OK;
}

static inline int ap_pcen_grid(const ApPcenParams &P) {
    const int64_t g = (P.rows + APPC_WAVES - 1) / APPC_WAVES;
    return (int)(g < (1 << 20) ? g : (1 << 20));
}

#ifdef AP_HOST_EMU
AP_DEV float appc_lane_get(float x, int src) { return emu_lane_perm(x, src); }
#else
AP_DEV float appc_lane_get(float x, int src) { return __shfl(x, src & 63, 64); }
#endif

// SciPy's mode="reflect" index for any i
AP_DEV int appc_reflect(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// The transcendentals of the chain are the hardware's own: v_log_f32 (log2), v_exp_f32 (2^x), v_rcp_f32, a quarter-rate
// instruction each, where the library's logf / expf / log1pf / expm1f cost the kernel twice its time.
// They take and give normal float32 values only: eps is a normal float32 (ap_prepare_pcen) and every argument below is
// eps + Msm >= eps, 1 + u >= 1 or 2^q >= 1; a result below FLT_MIN may come out as 0.
#ifdef AP_HOST_EMU
AP_DEV float appc_log2(float x) { return log2f(x); }
AP_DEV float appc_exp2(float x) { return exp2f(x); }
AP_DEV float appc_rcp(float x) { return 1.0f / x; }
#else
AP_DEV float appc_log2(float x) { return __builtin_amdgcn_logf(x); }
AP_DEV float appc_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
AP_DEV float appc_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
#endif
#define APPC_LN2 0.6931471805599453f
#define APPC_LOG2E 1.4426950408889634f

// log1p(u), u >= 0, as ln(w) u / (w - 1) with w = fl(1 + u) (Kahan): w - 1 is the increment ln(w) really saw, so the
// rounding of 1 + u cancels and a quiet u keeps its relative precision; w = 1: log1p(u) = u to half a unit roundoff.
AP_DEV float appc_log1p(float u) {
    const float w = 1.0f + u;
    return w == 1.0f ? u : (appc_log2(w) * APPC_LN2) * (u * appc_rcp(w - 1.0f));
}

// expm1(q), q >= 0, as (e - 1) q / ln(e) with e = fl(2^(q log2 e)): the same cancellation of e's own error.
AP_DEV float appc_expm1(float q) {
    const float e = appc_exp2(q * APPC_LOG2E);
    return e == 1.0f ? q : (e - 1.0f) * (q * appc_rcp(appc_log2(e) * APPC_LN2));
}

// The pointwise chain on x = S smooth >= 0.  No form subtracts two rounded values of like size: a quiet x / bias goes
// through log1p and expm1 with its relative precision intact.
template <int CHAIN>
AP_DEV float appc_compress(const ApPcenParams &P, float x) {
    if (CHAIN == APPC_LOG) return appc_log1p(x);
    if (CHAIN == APPC_POWER) return appc_exp2(P.power * appc_log2(x));     // x = 0: 2^-inf = 0
    return P.scale * appc_expm1(P.power * appc_log1p(x * P.inv_bias));
}

template <int CHAIN>
__global__ void __launch_bounds__(64 * APPC_WAVES) ap_pcen_kernel(ApPcenParams P) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const float pl = P.apow[lane], pl1 = P.apow[lane + 1];
    const bool windowed = !P.ref && P.max_size > 1;
    const int lo = P.max_size / 2;
    const int last_lane = (P.T - 1) & (APPC_TT - 1);
    for (int64_t row = (int64_t)blockIdx.x * APPC_WAVES + wave; row < P.rows; row += (int64_t)gridDim.x * APPC_WAVES) {
        const float *Sr = P.S + row * P.rs_in;
        const float *Rr = P.ref ? P.ref + row * P.rs_ref : Sr;
        float *Or = P.out + row * P.rs_out;
        const int m = (int)(row % P.M);
        const float *Sb = Sr - (int64_t)m * P.rs_in;           // row 0 of the clip
        float carry = P.zi ? P.zi[row] : P.zi0;                 // a Msm[-1]; from the second tile on Msm[64 tt - 1]
        for (int tt = 0; tt < P.n_tt; ++tt) {
            const int t = tt * APPC_TT + lane;
            const bool live = t < P.T;
            float s = 0.0f, r = 0.0f;
            if (live) {
                s = Sr[t];
                r = P.ref ? Rr[t] : s;
                if (windowed) {
                    r = Sb[(int64_t)appc_reflect(m - lo, P.M) * P.rs_in + t];
                    for (int j = 1; j < P.max_size; ++j) {
                        const float w = Sb[(int64_t)appc_reflect(m - lo + j, P.M) * P.rs_in + t];
                        r = (w > r || w != w) ? w : r;          // a NaN stays (fmaxf would drop it)
                    }
                }
            }
            float v = P.b * r;                                  // 0 behind the row's end
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const float up = appc_lane_get(v, lane - (1 << j));
                if (lane >= (1 << j)) v += P.apow[1 << j] * up;
            }
            v += (tt == 0 ? pl : pl1) * carry;                  // Msm
            carry = appc_lane_get(v, APPC_TT - 1);
            if (P.zf && tt == P.n_tt - 1 && lane == last_lane) P.zf[row] = P.a * v;
            if (live) {
                float x = s;
                if (P.gain != 0.0f) x = s * appc_exp2(-P.gain * appc_log2(P.eps + v));      // (eps + Msm)^-gain
                Or[t] = appc_compress<CHAIN>(P, x);
            }
        }
    }
}
