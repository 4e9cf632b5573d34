// Dynamic time warping (dtw.py: dtw, dtw_backtracking; the definitions of librosa 0.10's sequence.dtw).
//
// ap_dtw_cost_kernel.  C[b,i,j] = metric(X[b,:,i], Y[b,:,j]) for X (B, d, N), Y (B, d, M):
//   0 euclidean   sqrtf(sum_k (x_k - y_k)^2)          1 sqeuclidean   sum_k (x_k - y_k)^2
//   2 cityblock   sum_k |x_k - y_k|                   3 cosine        1 - x.y / (|x| |y|), |x| |y| < FLT_MIN -> 1
//   A workgroup (4 waves) owns one pair and a tile of 64 x 64 cells.  The features go through LDS in chunks of
//   APDC_KC: rows of X and of Y are read as segments of 64 consecutive frames, once.  Lane = column j, wave q owns
//   the rows 16 q .. 16 q + 15: X is a broadcast read, Y one read per feature, a row of C leaves as one 256-byte
//   segment.  The features are summed in ascending k with explicit fmaf; sqrtf and / are IEEE.
//
// ap_dtw_accumulate_kernel.  The recursion, for the step table (a_s, b_s, add_s, mul_s):
//   best = start(i,j) ? c : +inf, code = start ? 254 : 255;  for s ascending: cand = D[i-a_s, j-b_s] (+) ((mul_s (*) c) (+) add_s),
//   cand < best -> best = cand, code = s;  not (best < +inf) -> +inf, 255.           c = C[i,j] in the band, +inf outside
//   The matrix is cut into tiles of APDT_TH rows x 64 columns; one launch per tile-anti-diagonal, a wave per tile.
//   The wave keeps the tile and its halo (APDT_HA rows above, APDT_HB columns to the left, read from D, which
//   earlier launches wrote; +inf outside the matrix) in LDS as T[APDT_TH + HA][64 + HB]: C is loaded as row segments
//   and D overwrites it in place.  Lane = column; at step t lane l computes row t - l.  Reading T[t - l][l] has the
//   stride 63 (mod the pitch 68: 67) over the lanes: odd, so no two lanes of a half-wave meet in a bank.
//     FAST (the table [[1,1],[0,1],[1,0]], any weights): the three predecessors are the lane's own last value, the
//     left lane's last value (one DPP wave shift; lane 0 takes the halo column) and what that was one step earlier.
//     otherwise: the predecessors are read from T at [t - l - a][l - b]; one wave-level LDS hand-off per step.
//   Every (+) and (*) is one rounded float32 operation (ap_fadd / ap_fmul: never contracted into an fma), the
//   comparison is the strict <: the bits of a cell do not depend on the tiling, the grid or the batch.
//   No workgroup barrier: a wave never waits for another.
//
// ap_dtw_backtrack_kernel.  One wave per pair.  The start column is M - 1, start[b], or (subseq) the first minimum of
//   the last row of D.  A window of 64 x 64 step codes up and to the left of the current cell is loaded into LDS and
//   the path walked inside it (every lane walks, lane 0 writes) until it leaves the window; then the next window.
#pragma once
#include <cfloat>
#include <climits>
#include <cmath>

#include "ap_launch.h"
#include "fft_lds.h"

extern __shared__ __attribute__((aligned(16))) char ap_smem[];

#define APDT_TW 64               // columns of a tile: lane = column
#ifndef APDT_TH
#define APDT_TH 64               // rows of a tile
#endif
#ifndef APDT_WAVES
#define APDT_WAVES 1             // waves (= tiles) per workgroup of the accumulate kernel
#endif
#define APDT_MAX_STEPS 8         // cap on n_steps
#define APDT_MAX_STEP 4          // cap on a step's components
#define APDT_HA APDT_MAX_STEP    // halo rows above a tile
#define APDT_HB APDT_MAX_STEP    // halo columns to its left
#define APDT_P (APDT_TW + APDT_HB)                         // row pitch of T in floats: even, so P - 1 is odd
#define APDT_T_FLOATS ((APDT_TH + APDT_HA) * APDT_P)
#define APDT_WAVE_BYTES (APDT_T_FLOATS * 4 + APDT_TH * APDT_TW)
#define APDT_MAX_LEN (1 << 20)   // cap on N and M
#define APDT_LB 8                // rows loaded per batch (APDT_TH is a multiple); 32 measured slower
#define APDT_CODE_START 254
#define APDT_CODE_NONE 255

#define APDC_TI 64               // rows of a cost tile
#define APDC_TJ 64               // columns of a cost tile: lane = column
#define APDC_KC 32               // features per LDS chunk
#define APDC_THREADS 256
#define APDC_ROWS (APDC_TI / (APDC_THREADS / 64))          // rows a thread owns
#define APDC_MAX_D 1024          // cap on d

#define APBT_W 64                // the backtracking window is APBT_W x APBT_W codes
#define APBT_LDS_BYTES (APBT_W * APBT_W + 64 * 8 + 2 * APDT_MAX_STEPS * 4)

static_assert(APDT_TH % APDT_LB == 0 && APBT_W % APDT_LB == 0, "whole batches of rows");
static_assert(APDT_P % 2 == 0, "an odd lane stride keeps the skewed reads free of bank conflicts");
static_assert(APDT_WAVES * APDT_WAVE_BYTES <= 48 * 1024, "the tiles fit without the opt-in");
static_assert(APDC_ROWS * (APDC_THREADS / 64) == APDC_TI && APDC_TJ == 64, "lane = column, a wave owns whole rows");

struct ApDtwCostParams {
    const float *X;             // (B, d, x_rs)
    const float *Y;             // (B, d, y_rs)
    float *C;                   // (B, N, c_rs)
    int64_t B, N, M, x_rs, y_rs, c_rs, n_ti, n_tj, n_tiles;
    int d, metric, lds_bytes;
};

struct ApDtwAccParams {
    const float *C;             // (B, N, c_rs)
    float *D;                   // (B, N, d_rs)
    uint8_t *S;                 // (B, N, s_rs)
    int64_t B, N, M, c_rs, d_rs, s_rs;
    int64_t band_lo, band_hi;   // in the band: band_lo < j - i < band_hi
    int64_t n_ti, n_tj, n_diag;
    int64_t diag, ti_lo, n_on_diag, n_items;    // of the launch: its anti-diagonal, the first tile row, tiles, tiles x B
    int n_steps, subseq, use_band, fast, max_a, max_b, lds_bytes;
    int a[APDT_MAX_STEPS], b[APDT_MAX_STEPS];
    float add[APDT_MAX_STEPS], mul[APDT_MAX_STEPS];
};

struct ApDtwBtParams {
    const float *D;             // (B, N, d_rs) or NULL
    const uint8_t *S;           // (B, N, s_rs)
    const int32_t *start;       // (B) or NULL
    int32_t *path;              // (B, N + M - 1, 2)
    int32_t *len;               // (B)
    int64_t B, N, M, d_rs, s_rs;
    int n_steps, subseq, lds_bytes;
    int a[APDT_MAX_STEPS], b[APDT_MAX_STEPS];
};

static inline int ap_prepare_dtw_cost(ApDtwCostParams &P, const float *X, const float *Y, int64_t B, int d, int64_t N, int64_t M,
                                      int64_t x_rs, int64_t y_rs, int metric, float *C, int64_t c_rs) {
    if (!X || !Y || !C) AP_FAIL(AP_ERR_INVALID, "dtw_cost: NULL buffer");
    if (B <= 0 || N <= 0 || M <= 0)
        AP_FAIL(AP_ERR_INVALID, "dtw_cost: the sequences must be non-empty, got B = %lld, N = %lld, M = %lld", (long long)B, (long long)N, (long long)M);
    if (d < 1 || d > APDC_MAX_D) AP_FAIL(AP_ERR_INVALID, "dtw_cost: d must lie in [1, %d], got %d", APDC_MAX_D, d);
    if (N > APDT_MAX_LEN || M > APDT_MAX_LEN) AP_FAIL(AP_ERR_UNSUPPORTED, "dtw_cost: N and M must not exceed %d", APDT_MAX_LEN);
    if (metric < 0 || metric > 3) AP_FAIL(AP_ERR_INVALID, "dtw_cost: unknown metric %d (0 euclidean, 1 sqeuclidean, 2 cityblock, 3 cosine)", metric);
    if (x_rs < N) AP_FAIL(AP_ERR_INVALID, "dtw_cost: x_row_stride (%lld) must be >= N = %lld", (long long)x_rs, (long long)N);
    if (y_rs < M) AP_FAIL(AP_ERR_INVALID, "dtw_cost: y_row_stride (%lld) must be >= M = %lld", (long long)y_rs, (long long)M);
    if (c_rs < M) AP_FAIL(AP_ERR_INVALID, "dtw_cost: c_row_stride (%lld) must be >= M = %lld", (long long)c_rs, (long long)M);
    if ((double)B * (double)N * (double)c_rs * 4.0 > 9.0e18 || (double)B * d * (double)x_rs * 4.0 > 9.0e18 || (double)B * d * (double)y_rs * 4.0 > 9.0e18)
        AP_FAIL(AP_ERR_UNSUPPORTED, "dtw_cost: more than 2^63 bytes");
    P.X = X; P.Y = Y; P.C = C;
    P.B = B; P.N = N; P.M = M; P.x_rs = x_rs; P.y_rs = y_rs; P.c_rs = c_rs;
    P.d = d; P.metric = metric;
    P.n_ti = (N + APDC_TI - 1) / APDC_TI;
    P.n_tj = (M + APDC_TJ - 1) / APDC_TJ;
    if ((double)B * (double)P.n_ti * (double)P.n_tj > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "dtw_cost: too many tiles");
    P.n_tiles = B * P.n_ti * P.n_tj;
    P.lds_bytes = APDC_KC * (APDC_TI + APDC_TJ) * 4;
    return AP_OK;
}

static inline int ap_dtw_check_table(const char *who, int n_steps, const int32_t *ab) {
    if (n_steps < 1 || n_steps > APDT_MAX_STEPS) AP_FAIL(AP_ERR_INVALID, "%s: n_steps must lie in [1, %d], got %d", who, APDT_MAX_STEPS, n_steps);
    if (!ab) AP_FAIL(AP_ERR_INVALID, "%s: NULL step table", who);
    for (int s = 0; s < n_steps; ++s) {
        const int a = ab[2 * s], b = ab[2 * s + 1];
        if (a < 0 || b < 0 || (a == 0 && b == 0)) AP_FAIL(AP_ERR_INVALID, "%s: step %d is (%d, %d): components must be >= 0 and not both 0", who, s, a, b);
        if (a > APDT_MAX_STEP || b > APDT_MAX_STEP) AP_FAIL(AP_ERR_UNSUPPORTED, "%s: step %d is (%d, %d): components must not exceed %d", who, s, a, b, APDT_MAX_STEP);
    }
    return AP_OK;
}

// Validation and the geometry of ap_dtw_accumulate_f32 (and of its emulator twin); the launch fields are set by
// ap_dtw_acc_diagonal.
static inline int ap_prepare_dtw_accumulate(ApDtwAccParams &P, const float *C, int64_t B, int64_t N, int64_t M, int64_t c_rs, int n_steps,
                                            const int32_t *ab, const float *add, const float *mul, int subseq, int use_band,
                                            int64_t band_r, float *D, int64_t d_rs, uint8_t *S, int64_t s_rs) {
    if (!C || !D || !S) AP_FAIL(AP_ERR_INVALID, "dtw_accumulate: NULL buffer");
    if (B <= 0 || N <= 0 || M <= 0)
        AP_FAIL(AP_ERR_INVALID, "dtw_accumulate: the cost matrix must be non-empty, got (%lld, %lld, %lld)", (long long)B, (long long)N, (long long)M);
    if (N > APDT_MAX_LEN || M > APDT_MAX_LEN) AP_FAIL(AP_ERR_UNSUPPORTED, "dtw_accumulate: N and M must not exceed %d", APDT_MAX_LEN);
    int rc = ap_dtw_check_table("dtw_accumulate", n_steps, ab);
    if (rc != AP_OK) return rc;
    if (!add || !mul) AP_FAIL(AP_ERR_INVALID, "dtw_accumulate: NULL weights");
    if (c_rs < M) AP_FAIL(AP_ERR_INVALID, "dtw_accumulate: c_row_stride (%lld) must be >= M = %lld", (long long)c_rs, (long long)M);
    if (d_rs < M) AP_FAIL(AP_ERR_INVALID, "dtw_accumulate: d_row_stride (%lld) must be >= M = %lld", (long long)d_rs, (long long)M);
    if (s_rs < M) AP_FAIL(AP_ERR_INVALID, "dtw_accumulate: steps_row_stride (%lld) must be >= M = %lld", (long long)s_rs, (long long)M);
    if (use_band && band_r < 0) AP_FAIL(AP_ERR_INVALID, "dtw_accumulate: the band radius must be >= 0, got %lld", (long long)band_r);
    if ((double)B * (double)N * (double)c_rs * 4.0 > 9.0e18 || (double)B * (double)N * (double)d_rs * 4.0 > 9.0e18 ||
        (double)B * (double)N * (double)s_rs > 9.0e18)
        AP_FAIL(AP_ERR_UNSUPPORTED, "dtw_accumulate: more than 2^63 bytes");
    P.C = C; P.D = D; P.S = S;
    P.B = B; P.N = N; P.M = M; P.c_rs = c_rs; P.d_rs = d_rs; P.s_rs = s_rs;
    P.n_steps = n_steps; P.subseq = subseq ? 1 : 0; P.use_band = use_band ? 1 : 0;
    if (band_r > 2 * (int64_t)APDT_MAX_LEN) band_r = 2 * (int64_t)APDT_MAX_LEN;
    P.band_lo = -band_r - (N > M ? N - M : 0);
    P.band_hi = band_r + (M > N ? M - N : 0);
    P.max_a = 0; P.max_b = 0;
    for (int s = 0; s < APDT_MAX_STEPS; ++s) {
        const bool in = s < n_steps;
        P.a[s] = in ? ab[2 * s] : 1; P.b[s] = in ? ab[2 * s + 1] : 1;
        P.add[s] = in ? add[s] : 0.0f; P.mul[s] = in ? mul[s] : 1.0f;
        if (in && P.a[s] > P.max_a) P.max_a = P.a[s];
        if (in && P.b[s] > P.max_b) P.max_b = P.b[s];
    }
    P.fast = (n_steps == 3 && P.a[0] == 1 && P.b[0] == 1 && P.a[1] == 0 && P.b[1] == 1 && P.a[2] == 1 && P.b[2] == 0) ? 1 : 0;
    P.n_ti = (N + APDT_TH - 1) / APDT_TH;
    P.n_tj = (M + APDT_TW - 1) / APDT_TW;
    P.n_diag = P.n_ti + P.n_tj - 1;
    P.lds_bytes = APDT_WAVES * APDT_WAVE_BYTES;
    P.diag = 0; P.ti_lo = 0; P.n_on_diag = 0; P.n_items = 0;
    return AP_OK;
}

// The launch of tile-anti-diagonal `dg` (ti + tj = dg): its tiles and the number of workgroups.
static inline int64_t ap_dtw_acc_diagonal(ApDtwAccParams &P, int64_t dg) {
    const int64_t lo = dg - (P.n_tj - 1) > 0 ? dg - (P.n_tj - 1) : 0;
    const int64_t hi = dg < P.n_ti - 1 ? dg : P.n_ti - 1;
    P.diag = dg; P.ti_lo = lo; P.n_on_diag = hi - lo + 1;
    P.n_items = P.n_on_diag * P.B;
    const int64_t g = (P.n_items + APDT_WAVES - 1) / APDT_WAVES;
    return g < (1 << 24) ? g : (1 << 24);
}

static inline int ap_prepare_dtw_backtrack(ApDtwBtParams &P, const float *D, const uint8_t *S, const int32_t *start, int64_t B, int64_t N,
                                           int64_t M, int64_t d_rs, int64_t s_rs, int n_steps, const int32_t *ab, int subseq,
                                           int32_t *path, int32_t *len) {
    if (!S || !path || !len) AP_FAIL(AP_ERR_INVALID, "dtw_backtrack: NULL buffer");
    if (B <= 0 || N <= 0 || M <= 0)
        AP_FAIL(AP_ERR_INVALID, "dtw_backtrack: the step matrix must be non-empty, got (%lld, %lld, %lld)", (long long)B, (long long)N, (long long)M);
    if (N > APDT_MAX_LEN || M > APDT_MAX_LEN) AP_FAIL(AP_ERR_UNSUPPORTED, "dtw_backtrack: N and M must not exceed %d", APDT_MAX_LEN);
    int rc = ap_dtw_check_table("dtw_backtrack", n_steps, ab);
    if (rc != AP_OK) return rc;
    if (subseq && !start && !D) AP_FAIL(AP_ERR_INVALID, "dtw_backtrack: subseq needs D or the start columns");
    if (s_rs < M) AP_FAIL(AP_ERR_INVALID, "dtw_backtrack: steps_row_stride (%lld) must be >= M = %lld", (long long)s_rs, (long long)M);
    if (D && d_rs < M) AP_FAIL(AP_ERR_INVALID, "dtw_backtrack: d_row_stride (%lld) must be >= M = %lld", (long long)d_rs, (long long)M);
    if ((double)B * (double)N * (double)s_rs > 9.0e18 || (double)B * (double)N * (double)d_rs * 4.0 > 9.0e18)
        AP_FAIL(AP_ERR_UNSUPPORTED, "dtw_backtrack: more than 2^63 bytes");
    P.D = D; P.S = S; P.start = start; P.path = path; P.len = len;
    P.B = B; P.N = N; P.M = M; P.d_rs = d_rs; P.s_rs = s_rs;
    P.n_steps = n_steps; P.subseq = subseq ? 1 : 0;
    for (int s = 0; s < APDT_MAX_STEPS; ++s) { P.a[s] = s < n_steps ? ab[2 * s] : 1; P.b[s] = s < n_steps ? ab[2 * s + 1] : 1; }
    P.lds_bytes = APBT_LDS_BYTES;
    return AP_OK;
}

static inline int ap_dtw_grid(int64_t n) { return (int)(n < (1 << 24) ? n : (1 << 24)); }

// One rounded float32 operation each: a compiler must not fuse ap_fadd(ap_fmul(m, c), a) into an fma.  A wave-private
// LDS hand-off: the DS unit executes one wave's instructions in order, only the compiler has to be held back.  The
// value of the lane to the left, lane 0 taking `edge`.
#ifdef AP_HOST_EMU
AP_DEV float ap_fadd(float a, float b) { volatile float r = a + b; return r; }
AP_DEV float ap_fmul(float a, float b) { volatile float r = a * b; return r; }
#define APDT_WAVE_SYNC() emu_wave_sync()
AP_DEV int apdt_uniform(int x) { return x; }
AP_DEV float apdt_from_left(float v, float edge) {
    const int lane = (int)(threadIdx.x & 63);
    const float y = emu_lane_perm(v, lane - 1);
    return lane == 0 ? edge : y;
}
#else
// (HIP's __fadd_rn / __fmul_rn are plain a + b and a * b, which the compiler contracts; the pragma takes the `contract`
// flag off these two operations, and it stays off when they are inlined)
AP_DEV float ap_fadd(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
AP_DEV float ap_fmul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
#define APDT_WAVE_SYNC()                                        \
    do {                                                        \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
        __builtin_amdgcn_wave_barrier();                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
    } while (0)
AP_DEV int apdt_uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }      // the same in every lane: a scalar
AP_DEV float apdt_from_left(float v, float edge) {             // DPP wave_shr:1; lane 0 has no source and keeps `edge`
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v), 0x138, 0xF, 0xF, false));
}
#endif

// ---------------------------------------------------------------------------------------------------------------------
// cost
// ---------------------------------------------------------------------------------------------------------------------
template <int METRIC>
__global__ void __launch_bounds__(APDC_THREADS) ap_dtw_cost_kernel(ApDtwCostParams P) {
    float *Xs = reinterpret_cast<float *>(ap_smem);            // [APDC_KC][APDC_TI]
    float *Ys = Xs + APDC_KC * APDC_TI;                        // [APDC_KC][APDC_TJ]
    const int tid = threadIdx.x, lane = tid & 63, r0 = (tid >> 6) * APDC_ROWS;
    const int d = P.d;
    for (int64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
        const int64_t b = tile / (P.n_ti * P.n_tj);
        const int64_t rem = tile - b * P.n_ti * P.n_tj;
        const int64_t i0 = (rem / P.n_tj) * APDC_TI, j0 = (rem % P.n_tj) * APDC_TJ;
        const float *Xb = P.X + b * d * P.x_rs, *Yb = P.Y + b * d * P.y_rs;
        float acc[APDC_ROWS], nx[APDC_ROWS], ny = 0.0f;
#pragma unroll
        for (int u = 0; u < APDC_ROWS; ++u) { acc[u] = 0.0f; nx[u] = 0.0f; }
        for (int k0 = 0; k0 < d; k0 += APDC_KC) {
            const int kc = d - k0 < APDC_KC ? d - k0 : APDC_KC;
            for (int idx = tid; idx < kc * 64; idx += APDC_THREADS) {
                const int k = idx >> 6, c = idx & 63;
                Xs[k * APDC_TI + c] = i0 + c < P.N ? Xb[(int64_t)(k0 + k) * P.x_rs + i0 + c] : 0.0f;
                Ys[k * APDC_TJ + c] = j0 + c < P.M ? Yb[(int64_t)(k0 + k) * P.y_rs + j0 + c] : 0.0f;
            }
            __syncthreads();
            for (int k = 0; k < kc; ++k) {
                const float y = Ys[k * APDC_TJ + lane];
                if (METRIC == 3) ny = fmaf(y, y, ny);
#pragma unroll
                for (int u = 0; u < APDC_ROWS; ++u) {
                    const float x = Xs[k * APDC_TI + r0 + u];
                    if (METRIC == 3) {
                        acc[u] = fmaf(x, y, acc[u]);
                        nx[u] = fmaf(x, x, nx[u]);
                    } else {
                        const float e = x - y;
                        acc[u] = METRIC == 2 ? acc[u] + fabsf(e) : fmaf(e, e, acc[u]);
                    }
                }
            }
            __syncthreads();                                // the chunk is free for the next one
        }
        const int64_t j = j0 + lane;
        if (j < P.M) {
#pragma unroll
            for (int u = 0; u < APDC_ROWS; ++u) {
                const int64_t i = i0 + r0 + u;
                if (i >= P.N) break;
                float v = acc[u];
                if (METRIC == 0) v = sqrtf(v);
                if (METRIC == 3) {
                    float den = sqrtf(nx[u]) * sqrtf(ny);
                    if (den < FLT_MIN) den = 1.0f;
                    v = 1.0f - v / den;
                }
                P.C[(b * P.N + i) * P.c_rs + j] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// accumulate
// ---------------------------------------------------------------------------------------------------------------------
// One candidate of a cell: cand = pred (+) ((mul (*) c) (+) add); the strict < keeps the first minimum and never a NaN
AP_DEV void apdt_try(float pred, float c, float mul, float add, int s, float &best, int &code) {
    const float cand = ap_fadd(pred, ap_fadd(ap_fmul(mul, c), add));
    if (cand < best) { best = cand; code = s; }
}

template <bool FAST>
__global__ void __launch_bounds__(64 * APDT_WAVES) ap_dtw_accumulate_kernel(ApDtwAccParams P) {
    const int lane = threadIdx.x & 63, wave = apdt_uniform((int)(threadIdx.x >> 6));
    float *T = reinterpret_cast<float *>(ap_smem) + wave * APDT_T_FLOATS;                                    // [APDT_TH + HA][APDT_P]
    uint8_t *S = reinterpret_cast<uint8_t *>(ap_smem) + APDT_WAVES * APDT_T_FLOATS * 4 + wave * APDT_TH * APDT_TW;   // [APDT_TH][64]
    const float inf = INFINITY;
    const int HA = APDT_HA, HB = APDT_HB, PT = APDT_P;
    for (int64_t item = (int64_t)blockIdx.x * APDT_WAVES + wave; item < P.n_items; item += (int64_t)gridDim.x * APDT_WAVES) {
        const int64_t b = item / P.n_on_diag;
        const int64_t ti = P.ti_lo + (item - b * P.n_on_diag), tj = P.diag - ti;
        const int64_t i0 = ti * APDT_TH, j0 = tj * APDT_TW;
        const int rows = (int)(P.N - i0 < APDT_TH ? P.N - i0 : APDT_TH);      // of the matrix inside the tile
        const int cols = (int)(P.M - j0 < APDT_TW ? P.M - j0 : APDT_TW);
        const float *Cb = P.C + b * P.N * P.c_rs;
        float *Db = P.D + b * P.N * P.d_rs;
        uint8_t *Sb = P.S + b * P.N * P.s_rs;

        // the halo from D (+inf outside the matrix), C inside (+inf outside the band and beyond the matrix), APDT_LB rows
        // at a time: every load is issued at an index clamped into the payload, the ones that do not count are
        // replaced afterwards, so that no load waits for a branch
        const int64_t gj = j0 + lane, hj = j0 - P.max_b + lane;
        const int64_t gjc = gj < P.M ? gj : P.M - 1, hjc = hj < 0 ? 0 : (hj < P.M ? hj : P.M - 1);
        for (int rb = HA - P.max_a; rb < HA + rows; rb += APDT_LB) {
            float v[APDT_LB], h[APDT_LB];
#pragma unroll
            for (int u = 0; u < APDT_LB; ++u) {
                const int r = rb + u;
                const int64_t gi = i0 - HA + r;
                const int64_t ci = gi < 0 ? 0 : (gi < P.N ? gi : P.N - 1);
                const bool halo = r < HA;
                const float *src = halo ? Db + ci * P.d_rs : Cb + ci * P.c_rs;
                const float x = src[gjc], y = Db[ci * P.d_rs + hjc];
                const bool ok = gi >= 0 && lane < cols && (halo || !P.use_band || (P.band_lo < gj - gi && gj - gi < P.band_hi));
                v[u] = ok ? x : inf;
                h[u] = (gi >= 0 && hj >= 0) ? y : inf;
            }
#pragma unroll
            for (int u = 0; u < APDT_LB; ++u) {
                const int r = rb + u;
                if (r < HA + rows) {
                    T[r * PT + HB + lane] = v[u];
                    if (lane < P.max_b) T[r * PT + HB - P.max_b + lane] = h[u];
                }
            }
        }
        APDT_WAVE_SYNC();

        const int n_t = rows + cols - 1;
        if (FAST) {
            float cur = T[(HA - 1) * PT + HB + lane];           // D[i0 - 1, j]
            float leftprev = T[(HA - 1) * PT + HB - 1];         // lane 0: D[i0 - 1, j0 - 1]
            const bool first = i0 == 0 && (P.subseq || gj == 0);   // row 0 of this column is a start cell
            // c and the halo column's value of the next step are read while this one computes
            float c_next = T[HA * PT + HB + lane], edge_next = T[HA * PT + HB - 1];
            for (int t = 0; t < n_t; ++t) {
                const int r = t - lane;
                const bool active = r >= 0 && r < rows;
                const int rr = active ? r : 0;
                const float c = c_next, edge = edge_next;       // C[i0 + r, j]; D[i0 + t, j0 - 1]
                const int r1 = r + 1 < 0 ? 0 : (r + 1 < rows ? r + 1 : rows - 1);
                c_next = T[(HA + r1) * PT + HB + lane];
                edge_next = T[(HA + (t + 1 < rows ? t + 1 : rows - 1)) * PT + HB - 1];
                const float left = apdt_from_left(cur, edge);
                const float diag = leftprev;
                leftprev = left;
                const bool start = first && r == 0;
                float best = start ? c : inf;
                int code = start ? APDT_CODE_START : APDT_CODE_NONE;
                apdt_try(diag, c, P.mul[0], P.add[0], 0, best, code);
                apdt_try(left, c, P.mul[1], P.add[1], 1, best, code);
                apdt_try(cur, c, P.mul[2], P.add[2], 2, best, code);
                if (!(best < inf)) { best = inf; code = APDT_CODE_NONE; }
                if (active) {
                    cur = best;
                    T[(HA + rr) * PT + HB + lane] = best;
                    S[rr * APDT_TW + lane] = (uint8_t)code;
                }
            }
        } else {
            for (int t = 0; t < n_t; ++t) {
                const int r = t - lane;
                const bool active = r >= 0 && r < rows;
                const int rr = active ? r : 0;
                const float *cell = T + (HA + rr) * PT + HB + lane;
                const float c = cell[0];
                const bool start = i0 == 0 && r == 0 && (P.subseq || gj == 0);
                float best = start ? c : inf;
                int code = start ? APDT_CODE_START : APDT_CODE_NONE;
#pragma unroll
                for (int s = 0; s < APDT_MAX_STEPS; ++s)
                    if (s < P.n_steps) apdt_try(cell[-P.a[s] * PT - P.b[s]], c, P.mul[s], P.add[s], s, best, code);
                if (!(best < inf)) { best = inf; code = APDT_CODE_NONE; }
                if (active) {
                    T[(HA + rr) * PT + HB + lane] = best;
                    S[rr * APDT_TW + lane] = (uint8_t)code;
                }
                APDT_WAVE_SYNC();                               // the next step reads what this one wrote
            }
        }

        // D and the codes leave as row segments
        if (lane < cols) {
#pragma unroll 8
            for (int r = 0; r < rows; ++r) {
                Db[(i0 + r) * P.d_rs + j0 + lane] = T[(HA + r) * PT + HB + lane];
                Sb[(i0 + r) * P.s_rs + j0 + lane] = S[r * APDT_TW + lane];
            }
        }
        APDT_WAVE_SYNC();                                       // the tile is free for the next one
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// backtrack
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) ap_dtw_backtrack_kernel(ApDtwBtParams P) {
    uint8_t *win = reinterpret_cast<uint8_t *>(ap_smem);                       // [APBT_W][APBT_W]
    float *redv = reinterpret_cast<float *>(ap_smem + APBT_W * APBT_W);        // [64]
    int *redj = reinterpret_cast<int *>(redv + 64);                            // [64]
    int *tab = redj + 64;                                                      // [2][APDT_MAX_STEPS]
    const int lane = threadIdx.x & 63;
    if (lane < APDT_MAX_STEPS) { tab[lane] = P.a[lane]; tab[APDT_MAX_STEPS + lane] = P.b[lane]; }
    APDT_WAVE_SYNC();
    const int64_t L = P.N + P.M - 1;
    for (int64_t b = blockIdx.x; b < P.B; b += gridDim.x) {
        const uint8_t *Sb = P.S + b * P.N * P.s_rs;
        int64_t i = P.N - 1, j = P.M - 1;
        if (P.start) {
            j = P.start[b];
        } else if (P.subseq) {
            // the first minimum of the last row: every lane its columns in ascending order, then the lanes in order
            const float *row = P.D + (b * P.N + (P.N - 1)) * P.d_rs;
            float bv = INFINITY;
            int bj = INT_MAX;
            for (int64_t q = lane; q < P.M; q += 64) {
                const float v = row[q];
                if (v < bv) { bv = v; bj = (int)q; }
            }
            redv[lane] = bv; redj[lane] = bj;
            APDT_WAVE_SYNC();
            bv = INFINITY; bj = INT_MAX;
            for (int q = 0; q < 64; ++q) {
                const float v = redv[q];
                const int vj = redj[q];
                if (v < bv || (v == bv && vj < bj)) { bv = v; bj = vj; }
            }
            j = bj == INT_MAX ? 0 : bj;
            APDT_WAVE_SYNC();
        }
        int64_t k = 0;
        int result = 0;                                         // 0: walking, 1: reached a start cell, -1: no path
        if (j < 0 || j >= P.M) result = -1;
        while (result == 0) {
            const int64_t wi0 = i - (APBT_W - 1), wj0 = j - (APBT_W - 1);
            const int64_t gj = wj0 + lane, gjc = gj < 0 ? 0 : gj;
            for (int rb = 0; rb < APBT_W; rb += APDT_LB) {      // clamped loads first, the replacements after
                uint8_t v[APDT_LB];
#pragma unroll
                for (int u = 0; u < APDT_LB; ++u) {
                    const int64_t gi = wi0 + rb + u;
                    v[u] = Sb[(gi < 0 ? 0 : gi) * P.s_rs + gjc];
                }
#pragma unroll
                for (int u = 0; u < APDT_LB; ++u)
                    win[(rb + u) * APBT_W + lane] = (wi0 + rb + u >= 0 && gj >= 0) ? v[u] : (uint8_t)APDT_CODE_NONE;
            }
            APDT_WAVE_SYNC();
            while (true) {
                const int code = win[(int)(i - wi0) * APBT_W + (int)(j - wj0)];
                if (code != APDT_CODE_NONE && lane == 0 && k < L) {
                    int32_t *p = P.path + (b * L + k) * 2;
                    p[0] = (int32_t)i; p[1] = (int32_t)j;
                }
                if (code == APDT_CODE_START) { ++k; result = 1; break; }
                if (code >= P.n_steps || k + 1 >= L) { result = -1; break; }
                ++k;
                i -= tab[code]; j -= tab[APDT_MAX_STEPS + code];
                if (i < 0 || j < 0) { result = -1; break; }
                if (i < wi0 || j < wj0) break;
            }
            APDT_WAVE_SYNC();                                   // the window is free for the next one
        }
        if (lane == 0) P.len[b] = result == 1 ? (int32_t)k : -1;
    }
}
