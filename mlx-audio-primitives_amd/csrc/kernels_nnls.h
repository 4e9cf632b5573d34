// Non-negative least squares per frame, min_x ||A x - s||^2 with x >= 0, by accelerated projected gradient (FISTA) with
// a fixed step and a fixed number of iterations (inverse.py: mel_to_stft; DESIGN.md 9.14, stated in numpy by
// tests/nnls_ref.py).  s (B, M, T) >= 0 with a row stride, A the non-negative (M, F) bank as the plan of
// ap_nnls_plan_host (ap_common.h: the band of every row, the row range of every bin, the weights of both packed),
// P (F, M) the initial-solution matrix, out (B, F, T) with a row stride.
//
//   x0 = max(P s, 0); z = x0; repeat n_iter times: r = A z - s; x' = max(z - step A^T r, 0);
//   z = x' + momentum[it] (x' - x); x = x';    out = x^(1 / power)
//
// One launch.  A workgroup of 1024 threads (16 waves, four per SIMD) owns APQ_TT = 16 consecutive frames of one clip:
// thread = (frame f = tid % 16, group g = tid / 16), 64 groups.  LDS holds z and x as [F][16], s and r as [M][16], the
// frame fastest: the 16 lanes of a group read 16 consecutive words and the four groups of a wave four such runs, so a
// ds_read_b32 of state at (k + j) 16 + f has conflicts only where two groups of a half-wave meet in k mod 2, and the
// weights are uniform over a group (one address per 16 lanes, served by the vector L1: a CU touches the 2 x nnz packed
// weights and 3 (M + F) descriptor words of the plan, about 30 KB for the 128 x 1025 mel bank, over and over).
// (2 F + 2 M) 64 bytes of LDS (147 584 at 1025 x 128) allow one workgroup per CU, which is why it is as large as a
// workgroup gets.  Between the load of the s tile and the store of the x tile no state leaves the CU.
//
//   init      x0 = max(P s, 0) on v_mfma_f32_16x16x4_f32: the tile is 16 frames wide, the N of that instruction; wave w
//             takes the 16-bin blocks w, w + 16, .., walks M in steps of 4 with P from HBM (lane l: P[bin0 + l % 16]
//             [m0 + l / 16]) and s from LDS (s[m0 + l / 16][l % 16], 64 consecutive words)
//   A z       group g takes the rows g, 127 - g, 128 + g, .. (every other pass of 64 mirrored: the bands of a mel bank
//             grow with the row, so a group gets a short and a long one), the band in column order, fmaf
//   A^T r     group g takes the bins g, g + 64, ..: the bin's row range in row order, fmaf, then the projection and the
//             momentum step on the element the same thread owns in every iteration
// Every sum has one order, fixed by the shape alone: the same bits on every run, alone or in a batch.
#pragma once
#include <cmath>

#include "ap_launch.h"
#include "fft_lds.h"

extern __shared__ __attribute__((aligned(16))) char ap_smem[];

#define APQ_THREADS 1024
#define APQ_TT 16                                   // frames per tile
#define APQ_GROUPS (APQ_THREADS / APQ_TT)           // 64
#define APQ_WAVES (APQ_THREADS / 64)                // 16

struct ApNnlsParams {
    const float *s;             // (B, M, rs)
    const int32_t *plan;        // ap_nnls_plan_host
    const float *P;             // (F, M)
    const float *mom;           // (n_iter)
    float *out;                 // (B, F, ors)
    int64_t T, rs, ors, tiles;  // tiles of APQ_TT frames per clip
    int M, F, n_iter;
    float step, power;
};

static inline int ap_nnls_lds_bytes(int M, int F) { return (2 * F + 2 * M) * APQ_TT * 4; }

static inline int ap_prepare_nnls(ApNnlsParams &p, const float *s, int64_t B, int M, int F, int64_t T, int64_t rs, const int32_t *plan,
                                  const float *P, float step, const float *mom, int n_iter, float power, float *out, int64_t ors,
                                  int64_t *grid) {
    if (!s || !plan || !P || !out || (n_iter > 0 && !mom)) AP_FAIL(AP_ERR_INVALID, "nnls: NULL buffer");
    if (B <= 0 || M <= 0 || F <= 0 || T <= 0)
        AP_FAIL(AP_ERR_INVALID, "nnls: s must be non-empty, got (%lld, %d, %lld) and %d bins", (long long)B, M, (long long)T, F);
    if (rs < T || ors < T) AP_FAIL(AP_ERR_INVALID, "nnls: row strides (%lld, %lld) must be >= T = %lld", (long long)rs, (long long)ors, (long long)T);
    if (n_iter < 0) AP_FAIL(AP_ERR_INVALID, "nnls: n_iter must be non-negative, got %d", n_iter);
    if (!(power > 0.0f) || !std::isfinite(power)) AP_FAIL(AP_ERR_INVALID, "nnls: power must be positive, got %g", (double)power);
    if (!(step > 0.0f) || !std::isfinite(step)) AP_FAIL(AP_ERR_INVALID, "nnls: step must be positive and finite, got %g", (double)step);
    if (F > AP_NNLS_MAX_BINS || M > AP_NNLS_MAX_ROWS)
        AP_FAIL(AP_ERR_UNSUPPORTED, "nnls: a (%d, %d) bank is over the limits of %d rows and %d bins", M, F, AP_NNLS_MAX_ROWS, AP_NNLS_MAX_BINS);
    const int64_t tiles = (T + APQ_TT - 1) / APQ_TT;
    if ((double)B * (double)tiles > 2147483647.0 || (double)B * (double)F * (double)(rs > ors ? rs : ors) * 4.0 > 9.0e18)
        AP_FAIL(AP_ERR_UNSUPPORTED, "nnls: more than 2^31 - 1 tiles of %d frames (%lld clips of %lld)", APQ_TT, (long long)B, (long long)T);
    p.s = s; p.plan = plan; p.P = P; p.mom = mom; p.out = out;
    p.T = T; p.rs = rs; p.ors = ors; p.tiles = tiles;
    p.M = M; p.F = F; p.n_iter = n_iter; p.step = step; p.power = power;
    *grid = B * tiles;
    return AP_OK;
}

#ifdef AP_HOST_EMU
AP_DEV void apq_mfma(float a, float b, float (&c)[4]) { emu_mfma_f32_16x16x4f32(a, b, c); }
#else
typedef float apq_v4 __attribute__((ext_vector_type(4)));
AP_DEV void apq_mfma(float a, float b, float (&c)[4]) {
    apq_v4 d = {c[0], c[1], c[2], c[3]};
    d = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, d, 0, 0, 0);
    c[0] = d[0]; c[1] = d[1]; c[2] = d[2]; c[3] = d[3];
}
#endif

AP_KERNEL void __launch_bounds__(APQ_THREADS) ap_nnls_fista_kernel(ApNnlsParams p) {
    const int M = p.M, F = p.F;
    float *z = reinterpret_cast<float *>(ap_smem);                  // [F][16]
    float *x = z + F * APQ_TT;                                      // [F][16]
    float *sl = x + F * APQ_TT;                                     // [M][16]
    float *r = sl + M * APQ_TT;                                     // [M][16]
    const int tid = threadIdx.x, f = tid % APQ_TT, g = tid / APQ_TT;
    const int64_t b = blockIdx.x / p.tiles, t0 = (blockIdx.x - b * p.tiles) * APQ_TT;
    const bool live = t0 + f < p.T;                                 // frames beyond T run on zeros and are not stored
    const int32_t *plan = p.plan;
    if (plan[0] != M || plan[1] != F) return;                       // not this bank's plan: nothing is read through it
    const int32_t *rows = plan + plan[2], *bins = plan + plan[3];
    const float *wr = reinterpret_cast<const float *>(plan + plan[4]), *wc = reinterpret_cast<const float *>(plan + plan[5]);

    const float *sb = p.s + b * M * p.rs + t0 + f;
    for (int m = g; m < M; m += APQ_GROUPS) sl[m * APQ_TT + f] = live ? sb[m * p.rs] : 0.0f;
    __syncthreads();

    {   // x0 = max(P s, 0): D[bin][frame] += P[bin][m] s[m][frame], 16 bins a block
        const int lane = tid & 63, wv = tid >> 6, lr = lane & 15, lq = lane >> 4;
        for (int bin0 = 16 * wv; bin0 < F; bin0 += 16 * APQ_WAVES) {
            const int bin = bin0 + lr;
            const float *Prow = p.P + (int64_t)(bin < F ? bin : F - 1) * M;
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int m0 = 0; m0 < M; m0 += 4) {
                const int m = m0 + lq;
                const bool in = m < M;
                const float a = (in && bin < F) ? Prow[m] : 0.0f;
                const float v = in ? sl[m * APQ_TT + lr] : 0.0f;
                apq_mfma(a, v, acc);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = bin0 + 4 * lq + q;
                if (k < F) {
                    const float v = fmaxf(acc[q], 0.0f);
                    z[k * APQ_TT + lr] = v;
                    x[k * APQ_TT + lr] = v;
                }
            }
        }
    }
    AP_LDS_BARRIER();

    for (int it = 0; it < p.n_iter; ++it) {
        int pass = 0;
        for (int base = 0; base < M; base += APQ_GROUPS, ++pass) {                  // r = A z - s
            const int m = base + ((pass & 1) ? APQ_GROUPS - 1 - g : g);
            if (m < M) {
                const int lo = rows[3 * m], len = rows[3 * m + 1];
                const float *w = wr + rows[3 * m + 2];
                const float *zp = z + lo * APQ_TT + f;
                float acc = 0.0f;
#pragma unroll 4
                for (int j = 0; j < len; ++j) acc = fmaf(w[j], zp[j * APQ_TT], acc);
                r[m * APQ_TT + f] = acc - sl[m * APQ_TT + f];
            }
        }
        AP_LDS_BARRIER();
        const float beta = p.mom[it];
        for (int k = g; k < F; k += APQ_GROUPS) {                                   // x' = max(z - step A^T r, 0), z
            const int lo = bins[3 * k], len = bins[3 * k + 1];
            const float *w = wc + bins[3 * k + 2];
            const float *rp = r + lo * APQ_TT + f;
            float acc = 0.0f;
#pragma unroll 4
            for (int j = 0; j < len; ++j) acc = fmaf(w[j], rp[j * APQ_TT], acc);
            const float xo = x[k * APQ_TT + f];
            const float xn = fmaxf(fmaf(-p.step, acc, z[k * APQ_TT + f]), 0.0f);
            x[k * APQ_TT + f] = xn;
            z[k * APQ_TT + f] = fmaf(beta, xn - xo, xn);
        }
        AP_LDS_BARRIER();
    }

    if (live) {
        float *ob = p.out + b * F * p.ors + t0 + f;
        const float inv = 1.0f / p.power;
        for (int k = g; k < F; k += APQ_GROUPS) {
            const float v = x[k * APQ_TT + f];
            ob[k * p.ors] = p.power == 1.0f ? v : p.power == 2.0f ? sqrtf(v) : powf(v, inv);
        }
    }
}
