// Recurrence and cross-similarity matrices (segment.py: recurrence_matrix, cross_similarity, recurrence_to_lag,
// lag_to_recurrence; the definitions of librosa 0.10's segment module).
//
// D[i,j] = metric(ref[:,i], data[:,j]) with the four metrics and the arithmetic of ap_dtw_cost_kernel (kernels_dtw.h:
// features summed in ascending order with explicit fmaf, sqrtf and / IEEE, a product of norms below FLT_MIN counts as 1):
// apsg_term / apsg_finish restate it, and the device test holds the two kernels to the same bits.  D is never stored.
//
// ap_segment_threshold_kernel.  A workgroup owns one query j.  The query's features lie in LDS; thread t computes the
//   distances of the frames i = t, t + 256, ... (a wave reads 64 consecutive frames of one feature row: the rows of ref
//   stay in L2 across the queries) and keeps the order-preserving key of every eligible one (|i - j| >= width, not NaN)
//   in LDS, n_ref words.  tau_j, the k-th smallest, is found exactly by a radix select on the keys (4 passes of 8 bits,
//   a histogram of integer LDS atomics per pass); t_j, the largest index admitted among the frames tied at tau_j, by
//   the same select on the indices of those frames.  k is clipped to the number of eligible frames; with none the
//   record is (NaN, -1), which admits nothing.  One 8-byte record per query leaves the kernel.
//
// ap_segment_bandwidth_kernel.  One workgroup per matrix over kth[j] = tau_j of the queries with a neighbour: the median
//   by the same select (the ranks (m - 1) / 2 and m / 2; fl(fl(a + b) 0.5f)), the mean and the geometric mean as
//   float64 sums in a fixed order (per thread ascending, then a tree over the threads), rounded to float32 once.
//
// ap_segment_write_kernel.  Tiled like the cost kernel: 64 x 64 cells, lane = column j (the query), wave q owns the
//   rows 16 q .. 16 q + 15, the features go through LDS in chunks of APSG_KC.  A cell is a neighbour when it is
//   eligible and (D, i) <= (tau_j, t_j); with sym also (D, j) <= (tau_i, t_i) (the records of the tile's rows lie in
//   LDS); then self sets the diagonal.  Every cell of the payload is written exactly once, as a row segment:
//   1 byte (connectivity) or 4 (distance; affinity = 2^(D scale), scale = fl32(-log2(e) / float64(bw)), v_exp_f32).
//
// ap_segment_lag_kernel.  lag[(i - j) mod t', j] = rec[i, j] and its inverse as one gather: the 127 source rows a tile
//   of 64 x 64 outputs draws from are loaded into LDS as row segments, lane c then reads row r + c (or r - c + 63) at
//   column c: the stride over the lanes is 65 (or -63) words, odd, so no two lanes of a half-wave meet in a bank.
#pragma once
#include <cfloat>
#include <climits>
#include <cmath>

#include "ap_launch.h"
#include "fft_lds.h"

extern __shared__ __attribute__((aligned(16))) char ap_smem[];

#define APSG_THREADS 256
#define APSG_TI 64               // rows of a tile of the write pass
#define APSG_TJ 64               // columns: lane = column
#define APSG_KC 32               // features per LDS chunk
#define APSG_ROWS (APSG_TI / (APSG_THREADS / 64))
#define APSG_MAX_D 1024          // cap on d: the cost kernel's (ap_dtw_max_features)
#define APSG_MAX_LEN 16384       // cap on n and n_ref: the keys of one query are n_ref words of LDS
#define APSG_NONE 0xFFFFFFFFu    // the key of a frame that is not eligible (as a float: a NaN, never eligible)
#define APSG_LAG_ROWS (2 * 64 - 1)
#define APSG_LOG2E 1.4426950408889634

static_assert(APSG_ROWS * (APSG_THREADS / 64) == APSG_TI && APSG_TJ == 64, "lane = column, a wave owns whole rows");
static_assert(APSG_MAX_LEN * 4 + (256 + 8 + APSG_MAX_D) * 4 <= AP_LDS_MAX, "the keys of the longest query fit the LDS of a CU");
static_assert(APSG_MAX_LEN <= 65536, "the index select takes two passes of 8 bits");

struct ApSegThrParams {
    const float *X;             // ref (B, d, x_rs)
    const float *Y;             // data (B, d, y_rs)
    uint32_t *rec;              // (B, n, 2): the bits of tau_j, t_j
    int64_t B, n_ref, n, x_rs, y_rs, n_items, k, width;
    int d, metric, lds_bytes;
};

struct ApSegBwParams {
    const uint32_t *rec;        // (B, n, 2)
    float *bw;                  // (B)
    int64_t B, n;
    int kind, lds_bytes;        // 0 med_k_scalar, 1 mean_k, 2 gmean_k
};

struct ApSegWriteParams {
    const float *X, *Y;
    const uint32_t *rec;
    const float *bw;            // (B) or NULL: then `scale` holds
    void *R;                    // (B, n_ref, r_rs) uint8 (mode 0) or float32
    int64_t B, n_ref, n, x_rs, y_rs, r_rs, n_ti, n_tj, n_tiles, width;
    int d, metric, mode, full, sym, self_diag, lds_bytes;
    float scale;
};

struct ApSegLagParams {
    const void *in;             // (B, rows_in, in_rs)
    void *out;                  // (B, rows_out, out_rs)
    int64_t B, n, tp, rows_in, rows_out, in_rs, out_rs, n_ti, n_tj, n_tiles;
    int to_lag, elem_bytes, lds_bytes;
};

static inline int ap_segment_check_pair(const char *who, const float *X, const float *Y, int64_t B, int d, int64_t n_ref, int64_t n,
                                        int64_t x_rs, int64_t y_rs, int metric, int64_t width) {
    if (!X || !Y) AP_FAIL(AP_ERR_INVALID, "%s: NULL buffer", who);
    if (B <= 0 || n_ref <= 0 || n <= 0)
        AP_FAIL(AP_ERR_INVALID, "%s: the sequences must be non-empty, got B = %lld, n_ref = %lld, n = %lld", who, (long long)B, (long long)n_ref, (long long)n);
    if (d < 1 || d > APSG_MAX_D) AP_FAIL(AP_ERR_INVALID, "%s: d must lie in [1, %d], got %d", who, APSG_MAX_D, d);
    if (n_ref > APSG_MAX_LEN || n > APSG_MAX_LEN) AP_FAIL(AP_ERR_UNSUPPORTED, "%s: n and n_ref must not exceed %d", who, APSG_MAX_LEN);
    if (B > (1 << 20)) AP_FAIL(AP_ERR_UNSUPPORTED, "%s: B must not exceed %d", who, 1 << 20);
    if (metric < 0 || metric > 3) AP_FAIL(AP_ERR_INVALID, "%s: unknown metric %d (0 euclidean, 1 sqeuclidean, 2 cityblock, 3 cosine)", who, metric);
    if (x_rs < n_ref) AP_FAIL(AP_ERR_INVALID, "%s: ref_row_stride (%lld) must be >= n_ref = %lld", who, (long long)x_rs, (long long)n_ref);
    if (y_rs < n) AP_FAIL(AP_ERR_INVALID, "%s: data_row_stride (%lld) must be >= n = %lld", who, (long long)y_rs, (long long)n);
    if (x_rs > ((int64_t)1 << 40) || y_rs > ((int64_t)1 << 40)) AP_FAIL(AP_ERR_UNSUPPORTED, "%s: a row stride above 2^40", who);
    if (width < 0) AP_FAIL(AP_ERR_INVALID, "%s: width must be >= 0, got %lld", who, (long long)width);
    if (width > 0 && n_ref != n) AP_FAIL(AP_ERR_INVALID, "%s: width > 0 is for a recurrence matrix: n_ref (%lld) must equal n (%lld)", who, (long long)n_ref, (long long)n);
    return AP_OK;
}

static inline int ap_prepare_segment_threshold(ApSegThrParams &P, const float *X, const float *Y, int64_t B, int d, int64_t n_ref, int64_t n,
                                               int64_t x_rs, int64_t y_rs, int metric, int64_t k, int64_t width, uint32_t *rec) {
    int rc = ap_segment_check_pair("segment_threshold", X, Y, B, d, n_ref, n, x_rs, y_rs, metric, width);
    if (rc != AP_OK) return rc;
    if (!rec) AP_FAIL(AP_ERR_INVALID, "segment_threshold: NULL buffer");
    if (k < 1) AP_FAIL(AP_ERR_INVALID, "segment_threshold: k must be >= 1, got %lld", (long long)k);
    P.X = X; P.Y = Y; P.rec = rec;
    P.B = B; P.n_ref = n_ref; P.n = n; P.x_rs = x_rs; P.y_rs = y_rs; P.n_items = B * n;
    P.k = k < n_ref ? k : n_ref; P.width = width;
    P.d = d; P.metric = metric;
    P.lds_bytes = (int)((n_ref + 256 + 8 + d) * 4);
    return AP_OK;
}

static inline int ap_prepare_segment_bandwidth(ApSegBwParams &P, const uint32_t *rec, int64_t B, int64_t n, int kind, float *bw) {
    if (!rec || !bw) AP_FAIL(AP_ERR_INVALID, "segment_bandwidth: NULL buffer");
    if (B <= 0 || n <= 0) AP_FAIL(AP_ERR_INVALID, "segment_bandwidth: the records must be non-empty, got B = %lld, n = %lld", (long long)B, (long long)n);
    if (n > APSG_MAX_LEN || B > (1 << 20)) AP_FAIL(AP_ERR_UNSUPPORTED, "segment_bandwidth: n must not exceed %d and B %d", APSG_MAX_LEN, 1 << 20);
    if (kind < 0 || kind > 2) AP_FAIL(AP_ERR_INVALID, "segment_bandwidth: unknown kind %d (0 med_k_scalar, 1 mean_k, 2 gmean_k)", kind);
    P.rec = rec; P.bw = bw; P.B = B; P.n = n; P.kind = kind;
    P.lds_bytes = (256 + 8) * 4 + APSG_THREADS * 8;
    return AP_OK;
}

static inline int ap_prepare_segment_write(ApSegWriteParams &P, const float *X, const float *Y, int64_t B, int d, int64_t n_ref, int64_t n,
                                           int64_t x_rs, int64_t y_rs, int metric, int mode, int64_t width, int full, int sym, int self_diag,
                                           const uint32_t *rec, const float *bw, double bandwidth, void *R, int64_t r_rs) {
    int rc = ap_segment_check_pair("segment_write", X, Y, B, d, n_ref, n, x_rs, y_rs, metric, width);
    if (rc != AP_OK) return rc;
    if (!rec || !R) AP_FAIL(AP_ERR_INVALID, "segment_write: NULL buffer");
    if (mode < 0 || mode > 2) AP_FAIL(AP_ERR_INVALID, "segment_write: unknown mode %d (0 connectivity, 1 distance, 2 affinity)", mode);
    if ((sym || self_diag) && n_ref != n) AP_FAIL(AP_ERR_INVALID, "segment_write: sym and self are for a recurrence matrix: n_ref (%lld) must equal n (%lld)", (long long)n_ref, (long long)n);
    if (r_rs < n) AP_FAIL(AP_ERR_INVALID, "segment_write: out_row_stride (%lld) must be >= n = %lld", (long long)r_rs, (long long)n);
    if (r_rs > ((int64_t)1 << 40)) AP_FAIL(AP_ERR_UNSUPPORTED, "segment_write: a row stride above 2^40");
    if (mode == 2 && !bw && !(bandwidth > 0.0 && bandwidth < INFINITY)) AP_FAIL(AP_ERR_INVALID, "segment_write: the bandwidth must be a positive finite number, got %g", bandwidth);
    P.X = X; P.Y = Y; P.rec = rec; P.bw = mode == 2 ? bw : nullptr; P.R = R;
    P.B = B; P.n_ref = n_ref; P.n = n; P.x_rs = x_rs; P.y_rs = y_rs; P.r_rs = r_rs; P.width = width;
    P.d = d; P.metric = metric; P.mode = mode; P.full = full ? 1 : 0; P.sym = sym ? 1 : 0; P.self_diag = self_diag ? 1 : 0;
    P.scale = (mode == 2 && !bw) ? (float)(-APSG_LOG2E / bandwidth) : 0.0f;
    P.n_ti = (n_ref + APSG_TI - 1) / APSG_TI;
    P.n_tj = (n + APSG_TJ - 1) / APSG_TJ;
    P.n_tiles = B * P.n_ti * P.n_tj;
    P.lds_bytes = APSG_KC * (APSG_TI + APSG_TJ) * 4 + APSG_TI * 8;
    return AP_OK;
}

static inline int ap_prepare_segment_lag(ApSegLagParams &P, const void *in, int64_t B, int64_t n, int64_t tp, int elem_bytes, int to_lag,
                                         int64_t in_rs, void *out, int64_t out_rs) {
    if (!in || !out) AP_FAIL(AP_ERR_INVALID, "segment_lag: NULL buffer");
    if (B <= 0 || n <= 0) AP_FAIL(AP_ERR_INVALID, "segment_lag: the matrix must be non-empty, got B = %lld, n = %lld", (long long)B, (long long)n);
    if (n > APSG_MAX_LEN || B > (1 << 20)) AP_FAIL(AP_ERR_UNSUPPORTED, "segment_lag: n must not exceed %d and B %d", APSG_MAX_LEN, 1 << 20);
    if (tp != n && tp != 2 * n) AP_FAIL(AP_ERR_INVALID, "segment_lag: the lag axis must hold n or 2 n rows (n = %lld), got %lld", (long long)n, (long long)tp);
    if (elem_bytes != 1 && elem_bytes != 4) AP_FAIL(AP_ERR_INVALID, "segment_lag: elements of 1 or 4 bytes, got %d", elem_bytes);
    if (in_rs < n) AP_FAIL(AP_ERR_INVALID, "segment_lag: in_row_stride (%lld) must be >= n = %lld", (long long)in_rs, (long long)n);
    if (out_rs < n) AP_FAIL(AP_ERR_INVALID, "segment_lag: out_row_stride (%lld) must be >= n = %lld", (long long)out_rs, (long long)n);
    if (in_rs > ((int64_t)1 << 40) || out_rs > ((int64_t)1 << 40)) AP_FAIL(AP_ERR_UNSUPPORTED, "segment_lag: a row stride above 2^40");
    P.in = in; P.out = out; P.B = B; P.n = n; P.tp = tp;
    P.to_lag = to_lag ? 1 : 0; P.elem_bytes = elem_bytes;
    P.rows_in = to_lag ? n : tp; P.rows_out = to_lag ? tp : n;
    P.in_rs = in_rs; P.out_rs = out_rs;
    P.n_ti = (P.rows_out + 63) / 64;
    P.n_tj = (n + 63) / 64;
    P.n_tiles = B * P.n_ti * P.n_tj;
    P.lds_bytes = APSG_LAG_ROWS * 64 * elem_bytes;
    return AP_OK;
}

static inline int ap_segment_grid(int64_t n) { return (int)(n < (1 << 24) ? n : (1 << 24)); }

// ---------------------------------------------------------------------------------------------------------------------
// the distance of one pair: the arithmetic of ap_dtw_cost_kernel, operation for operation
// ---------------------------------------------------------------------------------------------------------------------
template <int METRIC>
AP_DEV void apsg_term(float x, float y, float &acc, float &nx) {
    if (METRIC == 3) {
        acc = fmaf(x, y, acc);
        nx = fmaf(x, x, nx);
    } else {
        const float e = x - y;
        acc = METRIC == 2 ? acc + fabsf(e) : fmaf(e, e, acc);
    }
}

template <int METRIC>
AP_DEV float apsg_finish(float acc, float nx, float ny) {
    float v = acc;
    if (METRIC == 0) v = sqrtf(v);
    if (METRIC == 3) {
        float den = sqrtf(nx) * sqrtf(ny);
        if (den < FLT_MIN) den = 1.0f;
        v = 1.0f - v / den;
    }
    return v;
}

// (D, index) <= (tau, t): the tie rule of the selection
AP_DEV bool apsg_admits(float v, int64_t index, float tau, int t) { return v < tau || (v == tau && index <= (int64_t)t); }

#ifdef AP_HOST_EMU
AP_DEV float apsg_exp2(float x) { return exp2f(x); }
#else
AP_DEV float apsg_exp2(float x) { return __builtin_amdgcn_exp2f(x); }    // a result below FLT_MIN may come out as 0
#endif

// The value of 0-based rank `rank` among val(i), i in [0, n), over the i that val accepts: a radix select, 8 bits per
// pass from pass `top` down (no accepted value has a bit above pass `top`).  Every thread of the workgroup calls it and
// gets the value; eq: how many accepted values equal it, below: the rank of the first of them.  hist: 256 words,
// st: 4 words of LDS.  rank must be below the number of accepted values.
template <class F>
AP_DEV unsigned apsg_select(int n, unsigned rank, int top, unsigned *hist, unsigned *st, F val, unsigned &eq, unsigned &rank_in_eq) {
    const int tid = threadIdx.x;
    if (tid == 0) { st[0] = 0u; st[1] = rank; st[2] = 0u; }
    for (int pass = top; pass >= 0; --pass) {
        const int sh = 8 * pass;
        for (int q = tid; q < 256; q += APSG_THREADS) hist[q] = 0u;
        __syncthreads();
        const unsigned prefix = st[0];
        for (int i = tid; i < n; i += APSG_THREADS) {
            unsigned key;
            if (val(i, key) && (pass == top || (key >> (sh + 8)) == (prefix >> (sh + 8)))) atomicAdd(&hist[(key >> sh) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned r = st[1], cum = 0u;
            int dg = 0;
            for (; dg < 255; ++dg) {
                if (cum + hist[dg] > r) break;
                cum += hist[dg];
            }
            st[0] = prefix | ((unsigned)dg << sh);
            st[1] = r - cum;
            st[2] = hist[dg];
        }
        __syncthreads();
    }
    const unsigned v = st[0];
    rank_in_eq = st[1];
    eq = st[2];
    __syncthreads();                                        // st and hist are free for the next select
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// threshold pass
// ---------------------------------------------------------------------------------------------------------------------
template <int METRIC>
__global__ void __launch_bounds__(APSG_THREADS) ap_segment_threshold_kernel(ApSegThrParams P) {
    unsigned *keys = reinterpret_cast<unsigned *>(ap_smem);    // [n_ref]
    unsigned *hist = keys + P.n_ref;                           // [256]
    unsigned *st = hist + 256;                                 // [8]: 0 .. 2 the select's, 4: eligible frames
    float *yq = reinterpret_cast<float *>(st + 8);             // [d]
    const int tid = threadIdx.x, d = P.d, n_ref = (int)P.n_ref;
    for (int64_t item = blockIdx.x; item < P.n_items; item += gridDim.x) {
        const int64_t b = item / P.n, j = item - b * P.n;
        const float *Xb = P.X + b * d * P.x_rs, *Yb = P.Y + b * d * P.y_rs;
        for (int k = tid; k < d; k += APSG_THREADS) yq[k] = Yb[(int64_t)k * P.y_rs + j];
        if (tid == 0) st[4] = 0u;
        __syncthreads();
        float ny = 0.0f;
        if (METRIC == 3)
            for (int k = 0; k < d; ++k) ny = fmaf(yq[k], yq[k], ny);
        unsigned mine = 0u;
        for (int i = tid; i < n_ref; i += APSG_THREADS) {
            float acc = 0.0f, nx = 0.0f;
            for (int k = 0; k < d; ++k) apsg_term<METRIC>(Xb[(int64_t)k * P.x_rs + i], yq[k], acc, nx);
            const float v = apsg_finish<METRIC>(acc, nx, ny);
            const int64_t gap = i > j ? i - j : j - i;
            const bool ok = gap >= P.width && !(v != v);
            keys[i] = ok ? ap_fkey(v + 0.0f) : APSG_NONE;       // (+ 0: a -0 and a +0 tie, as they do for <)
            mine += ok ? 1u : 0u;
        }
        if (mine) atomicAdd(&st[4], mine);
        __syncthreads();
        const unsigned eligible = st[4];
        __syncthreads();
        unsigned tau_key = APSG_NONE;
        int t = -1;
        if (eligible > 0u) {
            const unsigned k_eff = (unsigned)P.k < eligible ? (unsigned)P.k : eligible;
            unsigned eq, r;
            tau_key = apsg_select(n_ref, k_eff - 1u, 3, hist, st, [&](int i, unsigned &key) { key = keys[i]; return key != APSG_NONE; }, eq, r);
            // of the frames tied at tau, those with the r + 1 smallest indices are admitted: t is the index of rank r
            unsigned eq2, r2;
            t = (int)apsg_select(n_ref, r, 1, hist, st, [&](int i, unsigned &key) { key = (unsigned)i; return keys[i] == tau_key; }, eq2, r2);
        }
        if (tid == 0) {
            uint32_t *rec = P.rec + (b * P.n + j) * 2;
            rec[0] = eligible > 0u ? __builtin_bit_cast(uint32_t, ap_fkey_inv(tau_key)) : 0x7FC00000u;
            rec[1] = (uint32_t)t;
        }
        __syncthreads();                                    // the keys are free for the next query
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// bandwidth
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(APSG_THREADS) ap_segment_bandwidth_kernel(ApSegBwParams P) {
    unsigned *hist = reinterpret_cast<unsigned *>(ap_smem);    // [256]
    unsigned *st = hist + 256;                                 // [8]
    double *red = reinterpret_cast<double *>(st + 8);          // [APSG_THREADS]
    const int tid = threadIdx.x, n = (int)P.n;
    for (int64_t b = blockIdx.x; b < P.B; b += gridDim.x) {
        const uint32_t *rec = P.rec + b * P.n * 2;
        if (tid == 0) st[4] = 0u;
        __syncthreads();
        unsigned mine = 0u;
        for (int j = tid; j < n; j += APSG_THREADS) mine += (int32_t)rec[2 * j + 1] >= 0 ? 1u : 0u;
        if (mine) atomicAdd(&st[4], mine);
        __syncthreads();
        const unsigned m = st[4];
        __syncthreads();
        float bw = NAN;                                     // no query has a neighbour: no bandwidth
        if (m > 0u && P.kind == 0) {
            auto val = [&](int j, unsigned &key) { key = ap_fkey(__builtin_bit_cast(float, rec[2 * j])); return (int32_t)rec[2 * j + 1] >= 0; };
            unsigned eq, r;
            const unsigned r_lo = (m - 1u) / 2u, r_hi = m / 2u;
            const float lo = ap_fkey_inv(apsg_select(n, r_lo, 3, hist, st, val, eq, r));
            const float hi = r_hi == r_lo ? lo : ap_fkey_inv(apsg_select(n, r_hi, 3, hist, st, val, eq, r));
            bw = r_hi == r_lo ? lo : (lo + hi) * 0.5f;
        } else if (m > 0u) {
            double s = 0.0;
            for (int j = tid; j < n; j += APSG_THREADS)
                if ((int32_t)rec[2 * j + 1] >= 0) {
                    const double v = (double)__builtin_bit_cast(float, rec[2 * j]);
                    s += P.kind == 2 ? log(v) : v;
                }
            red[tid] = s;
            __syncthreads();
            for (int w = APSG_THREADS / 2; w > 0; w >>= 1) {
                if (tid < w) red[tid] += red[tid + w];
                __syncthreads();
            }
            const double mean = red[0] / (double)m;
            bw = (float)(P.kind == 2 ? exp(mean) : mean);
            __syncthreads();
        }
        if (tid == 0) P.bw[b] = bw;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// write pass
// ---------------------------------------------------------------------------------------------------------------------
template <int METRIC, int MODE>
__global__ void __launch_bounds__(APSG_THREADS) ap_segment_write_kernel(ApSegWriteParams P) {
    float *Xs = reinterpret_cast<float *>(ap_smem);            // [APSG_KC][APSG_TI]
    float *Ys = Xs + APSG_KC * APSG_TI;                        // [APSG_KC][APSG_TJ]
    uint32_t *rowrec = reinterpret_cast<uint32_t *>(Ys + APSG_KC * APSG_TJ);   // [APSG_TI][2]: the records of the tile's rows (sym)
    const int tid = threadIdx.x, lane = tid & 63, r0 = (tid >> 6) * APSG_ROWS;
    const int d = P.d;
    for (int64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
        const int64_t b = tile / (P.n_ti * P.n_tj);
        const int64_t rem = tile - b * P.n_ti * P.n_tj;
        const int64_t i0 = (rem / P.n_tj) * APSG_TI, j0 = (rem % P.n_tj) * APSG_TJ;
        const float *Xb = P.X + b * d * P.x_rs, *Yb = P.Y + b * d * P.y_rs;
        const uint32_t *recb = P.rec + b * P.n * 2;
        if (P.sym && tid < 2 * APSG_TI) {                   // n_ref == n; published by the first barrier below
            const int64_t i = i0 + (tid >> 1);
            rowrec[tid] = i < P.n ? recb[i * 2 + (tid & 1)] : (uint32_t)-1;
        }
        float acc[APSG_ROWS], nx[APSG_ROWS], ny = 0.0f;
#pragma unroll
        for (int u = 0; u < APSG_ROWS; ++u) { acc[u] = 0.0f; nx[u] = 0.0f; }
        for (int k0 = 0; k0 < d; k0 += APSG_KC) {
            const int kc = d - k0 < APSG_KC ? d - k0 : APSG_KC;
            for (int idx = tid; idx < kc * 64; idx += APSG_THREADS) {
                const int k = idx >> 6, c = idx & 63;
                Xs[k * APSG_TI + c] = i0 + c < P.n_ref ? Xb[(int64_t)(k0 + k) * P.x_rs + i0 + c] : 0.0f;
                Ys[k * APSG_TJ + c] = j0 + c < P.n ? Yb[(int64_t)(k0 + k) * P.y_rs + j0 + c] : 0.0f;
            }
            __syncthreads();
            for (int k = 0; k < kc; ++k) {
                const float y = Ys[k * APSG_TJ + lane];
                if (METRIC == 3) ny = fmaf(y, y, ny);
#pragma unroll
                for (int u = 0; u < APSG_ROWS; ++u) apsg_term<METRIC>(Xs[k * APSG_TI + r0 + u], y, acc[u], nx[u]);
            }
            __syncthreads();                                // the chunk is free for the next one
        }
        const int64_t j = j0 + lane;
        if (j < P.n) {
            const float tau_j = __builtin_bit_cast(float, recb[j * 2]);
            const int t_j = (int)recb[j * 2 + 1];
            float scale = 0.0f;
            if (MODE == 2) scale = P.bw ? (float)(-APSG_LOG2E / (double)P.bw[b]) : P.scale;
#pragma unroll
            for (int u = 0; u < APSG_ROWS; ++u) {
                const int64_t i = i0 + r0 + u;
                if (i >= P.n_ref) break;
                const float v = apsg_finish<METRIC>(acc[u], nx[u], ny);
                const int64_t gap = i > j ? i - j : j - i;
                bool on = gap >= P.width && !(v != v);
                if (!P.full) on = on && apsg_admits(v, i, tau_j, t_j);
                if (P.sym && !P.full)
                    on = on && apsg_admits(v, j, __builtin_bit_cast(float, rowrec[2 * (r0 + u)]), (int)rowrec[2 * (r0 + u) + 1]);
                const bool diag = P.self_diag && i == j;    // after sym: the diagonal is set whatever the selection says
                const int64_t o = (b * P.n_ref + i) * P.r_rs + j;
                if (MODE == 0) {
                    reinterpret_cast<uint8_t *>(P.R)[o] = (on || diag) ? 1 : 0;
                } else if (MODE == 1) {
                    reinterpret_cast<float *>(P.R)[o] = diag ? 0.0f : (on ? v : 0.0f);
                } else {
                    reinterpret_cast<float *>(P.R)[o] = diag ? 1.0f : (on ? apsg_exp2(v * scale) : 0.0f);
                }
            }
        }
        if (P.sym) AP_LDS_BARRIER();                        // the rows' records are free for the next tile
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// lag <-> recurrence
// ---------------------------------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(APSG_THREADS) ap_segment_lag_kernel(ApSegLagParams P) {
    T *tile = reinterpret_cast<T *>(ap_smem);                  // [APSG_LAG_ROWS][64]
    const int tid = threadIdx.x, lane = tid & 63, r0 = (tid >> 6) * 16;
    const T *in = reinterpret_cast<const T *>(P.in);
    T *out = reinterpret_cast<T *>(P.out);
    for (int64_t item = blockIdx.x; item < P.n_tiles; item += gridDim.x) {
        const int64_t b = item / (P.n_ti * P.n_tj);
        const int64_t rem = item - b * P.n_ti * P.n_tj;
        const int64_t o0 = (rem / P.n_tj) * 64, j0 = (rem % P.n_tj) * 64;
        // to_lag: out[l, j] = in[(l + j) mod t', j] (0 for a row beyond n); else out[i, j] = in[(i - j) mod t', j]
        const int64_t base = P.to_lag ? o0 + j0 : o0 - j0 - 63;
        for (int idx = tid; idx < APSG_LAG_ROWS * 64; idx += APSG_THREADS) {
            const int rr = idx >> 6, c = idx & 63;
            int64_t row = (base + rr) % P.tp;
            if (row < 0) row += P.tp;
            tile[idx] = (j0 + c < P.n && row < P.rows_in) ? in[(b * P.rows_in + row) * P.in_rs + j0 + c] : (T)0;
        }
        __syncthreads();
        const int64_t j = j0 + lane;
        if (j < P.n) {
#pragma unroll 4
            for (int u = 0; u < 16; ++u) {
                const int r = r0 + u;
                if (o0 + r >= P.rows_out) break;
                const int rr = P.to_lag ? r + lane : r - lane + 63;
                out[(b * P.rows_out + o0 + r) * P.out_rs + j] = tile[rr * 64 + lane];
            }
        }
        __syncthreads();                                    // the tile is free for the next one
    }
}
