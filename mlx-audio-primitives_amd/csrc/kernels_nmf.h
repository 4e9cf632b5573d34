// Non-negative matrix factorisation by multiplicative updates (decompose.py: nmf, decompose; DESIGN.md 9.13, stated in
// numpy by tests/nmf_ref.py).  V (B, F, T) >= 0, rows rs apart; W (B, F, K), H (B, K, T); 1 <= K <= 64, padded in LDS
// (never in HBM) to the template width KP = 16 / 32 / 64 with zeros, which stay zero under both updates.
//
// Every contraction is v_mfma_f32_16x16x4_f32 (apn_mfma): D[i][j] += sum_{c < 4} A[i][c] B[c][j], one wave, lane l
// holding A[l % 16][l / 16] and B[l / 16][l % 16], register r of lane l holding D[4 (l / 16) + r][l % 16].
//
// The two half-steps are one kernel, ap_nmf_tile_kernel<KP, LOSS, SIDE, OBJ>.  Write X for the factor that is updated,
// Y for the one that is held, n for the axis X shares with V (the OWNER axis) and m for the axis that is contracted (the
// WALK axis):   SIDE 0 updates H: X = H, Y = W, m = f, n = t;   SIDE 1 updates W: X = W^T, Y = H^T, m = t, n = f.
// A workgroup (4 waves) owns one item and a tile of 64 owner positions; wave w owns the 16 positions [16 w, 16 w + 16).
// The X tile (KP x 64) is read into LDS once.  The walk axis is taken in chunks of 32: the V chunk (32 x 64) and the Y
// chunk (32 x KP) are staged in LDS in the order they have in HBM (whole row segments), then
//   Frobenius   acc[k][n] += sum_m Y[m][k] V[m][n]                               8 x KP/16 MFMAs per wave
//   KL          P[m][n] = sum_k Y[m][k] X[k][n]  (MFMA over k), the ratio V / (P + eps) replaces V in LDS at the lanes
//               that hold P, and the same contraction as above runs on the ratio tile: it never exists in HBM.
// The numerator stays in KP/16 accumulators of 4 registers.  Epilogue: Frobenius den = sum_k' G[k][k'] X[k'][n] + eps,
// one more MFMA over k with G = Y^T Y from ap_nmf_gram_kernel; KL den = sum_m Y[m][k] + eps, the sums of the same
// kernel.  X <- X * acc / den goes back through the LDS tile and leaves as row segments: X is read and written once and
// Frobenius reads V exactly twice per iteration.  OBJ: the same walk computes P and adds (V - P)^2, or
// V log(V / (P + eps)) - V + P with 0 log 0 = 0, in float64 per lane; the lanes are summed in lane order into one partial
// per tile and ap_nmf_objsum_kernel adds the tiles of an item in tile order.
//
// ap_nmf_gram_kernel<KP, LOSS, SIDE>: one workgroup per item walks m in the same chunks; wave w takes the MFMA steps
// w and w + 4 of a chunk for all (KP/16)^2 blocks of G (Frobenius), the four waves' blocks are added in wave order
// through LDS; lane k of wave 0 sums Y[m][k] in m order (KL).  No atomics anywhere: every sum has one order, which does
// not depend on the grid (the items are walked in a grid-stride loop over a partition that only the shape decides).
//
// LDS banks (ds_read_b32: two groups of 32 lanes, bank = word % 32).  An MFMA operand is read either ROW-WISE, word
// (l / 16) p + l % 16 + const: a half-wave covers rows 0 and 1, 16 words each, free of conflicts when p = 16 (mod 32) -
// p = 80 for the 64-wide tiles, 48, and 16 for KP = 16; or STRIDED, word (l % 16) p + l / 16 + const: 16 rows at two
// adjacent words, free of conflicts when p = 2 (mod 4), since then (l % 16) p mod 32 runs over the 16 even banks -
// p = 34 for the 32-wide chunks and KP + 2 for the W tile.  SIDE 1 keeps the rows of V contiguous in t as they are in
// HBM (pitch 34) and the MFMA reads them strided; SIDE 0 reads everything row-wise.  A factor chunk that KL reads both
// ways (Y in the two contractions) is staged twice, once per pitch.  The ratio is written at word
// (4 (l / 16) + r) p + l % 16: two-way conflicts (4 p = 0 mod 32) on one write per 2 KP/16 + 1 MFMAs, left as they are.
#pragma once
#include <cfloat>
#include <cmath>

#include "ap_launch.h"
#include "fft_lds.h"

extern __shared__ __attribute__((aligned(16))) char ap_smem[];

#define APN_THREADS 256
#define APN_NT 64                // owner positions per tile
#define APN_MC 32                // walk positions per chunk
#define APN_MAX_K 64
#define APN_FROBENIUS 0
#define APN_KL 1
#define APN_GRAM 0               // the kinds of launch
#define APN_UPDATE 1
#define APN_OBJECTIVE 2
#define APN_OBJSUM 3

struct ApNmfParams {
    const float *V;             // (B, F, rs)
    float *W;                   // (B, F, K)
    float *H;                   // (B, K, T)
    float *G;                   // (B, K, K) workspace: Y^T Y of the factor that is held
    float *S;                   // (B, K) workspace: the sums of that factor over the walk axis
    double *part;               // (B, n_tiles) workspace: objective per tile
    double *out;                // (B) objective
    int64_t B, F, T, rs, n_tiles, n_items;
    int K;
    float eps;
};

// words between neighbours of the LDS arrays: (walk m, owner n, component k)
template <int KP, int SIDE>
struct ApnGeom {
    static constexpr int PROW = KP == 16 ? 16 : 80;                             // KP-wide rows that are read row-wise
    static constexpr int V_SM = SIDE == 0 ? 80 : 1, V_SN = SIDE == 0 ? 1 : 34;
    static constexpr int Y_SM = SIDE == 0 ? PROW : 1, Y_SK = SIDE == 0 ? 1 : 34;
    static constexpr int Y2_SM = SIDE == 0 ? KP + 2 : 1, Y2_SK = SIDE == 0 ? 1 : 48;
    static constexpr int X_SK = SIDE == 0 ? 80 : 1, X_SN = SIDE == 0 ? 1 : KP + 2;
    static constexpr int V_FLOATS = SIDE == 0 ? APN_MC * 80 : APN_NT * 34;
    static constexpr int Y_FLOATS = SIDE == 0 ? APN_MC * PROW : KP * 34;
    static constexpr int Y2_FLOATS = SIDE == 0 ? APN_MC * (KP + 2) : KP * 48;
    static constexpr int X_FLOATS = SIDE == 0 ? KP * 80 : APN_NT * (KP + 2);
    static constexpr int G_FLOATS = KP * PROW;
    static constexpr int tile_bytes(int loss, bool obj) {
        return 4 * (V_FLOATS + Y_FLOATS + X_FLOATS + ((loss == APN_KL || obj) ? Y2_FLOATS : G_FLOATS));
    }
    static constexpr int gram_bytes(int loss) { return 4 * (Y_FLOATS + (loss == APN_FROBENIUS ? KP * KP : 0)); }
};
static_assert(ApnGeom<64, 0>::V_FLOATS * 4 >= APN_THREADS * 8 && ApnGeom<64, 1>::V_FLOATS * 4 >= APN_THREADS * 8,
              "the objective's lane sums are staged over the V chunk");

static inline int ap_nmf_kp(int K) { return K <= 16 ? 16 : K <= 32 ? 32 : 64; }

// workspace: G, S, then the objective's partials (one per T-tile)
static inline int64_t ap_nmf_part_offset(int64_t B, int K) { return ((B * K * K + B * K) * 4 + 7) / 8 * 8; }
static inline int64_t ap_nmf_ws_bytes(int64_t B, int64_t T, int K) {
    return ap_nmf_part_offset(B, K) + B * ((T + APN_NT - 1) / APN_NT) * 8;
}

static inline int ap_prepare_nmf(ApNmfParams &P, const float *V, int64_t B, int64_t F, int64_t T, int64_t rs, int K, float *W, float *H,
                                 int loss, float eps, void *workspace) {
    if (!V || !W || !H || !workspace) AP_FAIL(AP_ERR_INVALID, "nmf: NULL buffer");
    if (B <= 0 || F <= 0 || T <= 0) AP_FAIL(AP_ERR_INVALID, "nmf: V must be non-empty, got (%lld, %lld, %lld)", (long long)B, (long long)F, (long long)T);
    if (K < 1 || K > APN_MAX_K) AP_FAIL(AP_ERR_INVALID, "nmf: n_components must be in 1 .. %d, got %d", APN_MAX_K, K);
    if (rs < T) AP_FAIL(AP_ERR_INVALID, "nmf: row_stride (%lld) must be >= T = %lld", (long long)rs, (long long)T);
    if (loss != APN_FROBENIUS && loss != APN_KL) AP_FAIL(AP_ERR_INVALID, "nmf: unknown beta_loss %d (0 frobenius, 1 kullback-leibler)", loss);
    if (!(eps > 0.0f)) AP_FAIL(AP_ERR_INVALID, "nmf: eps must be > 0 (the zero padding of a tile divides 0 by eps)");
    if ((double)B * (double)F * (double)rs * 4.0 > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "nmf: more than 2^63 bytes");
    const int64_t tiles_t = (T + APN_NT - 1) / APN_NT, tiles_f = (F + APN_NT - 1) / APN_NT;
    if ((double)B * (double)(tiles_t > tiles_f ? tiles_t : tiles_f) > 2147483647.0)
        AP_FAIL(AP_ERR_UNSUPPORTED, "nmf: more than 2^31 - 1 tiles (%lld items of %lld x %lld)", (long long)B, (long long)F, (long long)T);
    P.V = V; P.W = W; P.H = H;
    P.G = reinterpret_cast<float *>(workspace);
    P.S = P.G + B * K * K;
    P.part = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + ap_nmf_part_offset(B, K));
    P.out = nullptr;
    P.B = B; P.F = F; P.T = T; P.rs = rs; P.K = K; P.eps = eps;
    P.n_tiles = 0; P.n_items = 0;
    return AP_OK;
}

static inline int ap_nmf_grid(int64_t n) { return (int)(n < (1 << 20) ? n : (1 << 20)); }

#ifdef AP_HOST_EMU
AP_DEV void apn_mfma(float a, float b, float (&c)[4]) { emu_mfma_f32_16x16x4f32(a, b, c); }
#else
typedef float apn_v4 __attribute__((ext_vector_type(4)));
AP_DEV void apn_mfma(float a, float b, float (&c)[4]) {
    apn_v4 d = {c[0], c[1], c[2], c[3]};
    d = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, d, 0, 0, 0);
    c[0] = d[0]; c[1] = d[1]; c[2] = d[2]; c[3] = d[3];
}
#endif

// The chunk [m0, m0 + 32) of the held factor, zeros beyond M and K; TWO: also in the second pitch.
template <int KP, int SIDE, bool TWO>
AP_DEV void apn_stage_y(const float *Wb, const float *Hb, int64_t m0, int64_t M, int K, int64_t T, float *Yl, float *Y2) {
    using Gm = ApnGeom<KP, SIDE>;
    for (int idx = threadIdx.x; idx < APN_MC * KP; idx += APN_THREADS) {
        int m, k;
        float y = 0.0f;
        if (SIDE == 0) {
            m = idx / KP; k = idx % KP;
            if (m0 + m < M && k < K) y = Wb[(m0 + m) * K + k];
        } else {
            k = idx / APN_MC; m = idx % APN_MC;
            if (m0 + m < M && k < K) y = Hb[(int64_t)k * T + m0 + m];
        }
        Yl[m * Gm::Y_SM + k * Gm::Y_SK] = y;
        if (TWO) Y2[m * Gm::Y2_SM + k * Gm::Y2_SK] = y;
    }
}

// The X tile between LDS and HBM: whole row segments of H (SIDE 0) or whole rows of W (SIDE 1).
template <int KP, int SIDE, bool STORE>
AP_DEV void apn_move_x(float *Wb, float *Hb, int64_t n0, int64_t N, int K, int64_t T, float *Xl) {
    using Gm = ApnGeom<KP, SIDE>;
    for (int idx = threadIdx.x; idx < APN_NT * KP; idx += APN_THREADS) {
        int n, k;
        if (SIDE == 0) { k = idx / APN_NT; n = idx % APN_NT; }
        else { n = idx / KP; k = idx % KP; }
        float *l = Xl + k * Gm::X_SK + n * Gm::X_SN;
        if (k < K && n0 + n < N) {
            float *g = SIDE == 0 ? Hb + (int64_t)k * T + n0 + n : Wb + (n0 + n) * K + k;
            if (STORE) *g = *l;
            else *l = *g;
        } else if (!STORE) *l = 0.0f;
    }
}

template <int KP, int LOSS, int SIDE, bool OBJ>
__global__ void __launch_bounds__(APN_THREADS) ap_nmf_tile_kernel(ApNmfParams P) {
    using Gm = ApnGeom<KP, SIDE>;
    constexpr int NB = KP / 16;
    constexpr bool RATIO = LOSS == APN_KL || OBJ;                    // the chunk of W H is needed
    float *Vl = reinterpret_cast<float *>(ap_smem);
    float *Yl = Vl + Gm::V_FLOATS;
    float *Xl = Yl + Gm::Y_FLOATS;
    float *Y2 = Xl + Gm::X_FLOATS;                                   // RATIO
    float *Gl = Y2;                                                  // Frobenius update
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int K = P.K;
    const int64_t M = SIDE == 0 ? P.F : P.T, N = SIDE == 0 ? P.T : P.F;
    const int nl = 16 * wv + lr;                                     // the owner position of this lane's B and D columns
    for (int64_t item = blockIdx.x; item < P.n_items; item += gridDim.x) {
        const int64_t b = item / P.n_tiles, n0 = (item - b * P.n_tiles) * APN_NT;
        const float *Vb = P.V + b * P.F * P.rs;
        float *Wb = P.W + b * P.F * K, *Hb = P.H + b * (int64_t)K * P.T;
        __syncthreads();                                             // the tile before is done with the LDS
        apn_move_x<KP, SIDE, false>(Wb, Hb, n0, N, K, P.T, Xl);
        if (!RATIO)
            for (int idx = tid; idx < KP * KP; idx += APN_THREADS) {
                const int k1 = idx / KP, k = idx % KP;
                Gl[k1 * Gm::PROW + k] = (k1 < K && k < K) ? P.G[(b * K + k1) * K + k] : 0.0f;
            }
        float acc[NB][4];
#pragma unroll
        for (int kb = 0; kb < NB; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[kb][r] = 0.0f;
        double obj = 0.0;
        for (int64_t m0 = 0; m0 < M; m0 += APN_MC) {
            __syncthreads();
            for (int idx = tid; idx < APN_MC * APN_NT; idx += APN_THREADS) {
                int m, n;
                if (SIDE == 0) { m = idx / APN_NT; n = idx % APN_NT; }
                else { n = idx / APN_MC; m = idx % APN_MC; }
                float v = 0.0f;
                if (m0 + m < M && n0 + n < N) v = SIDE == 0 ? Vb[(m0 + m) * P.rs + n0 + n] : Vb[(n0 + n) * P.rs + m0 + m];
                Vl[m * Gm::V_SM + n * Gm::V_SN] = v;
            }
            apn_stage_y<KP, SIDE, RATIO>(Wb, Hb, m0, M, K, P.T, Yl, Y2);
            __syncthreads();
            if (RATIO) {
#pragma unroll
                for (int mb = 0; mb < APN_MC / 16; ++mb) {
                    float p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int k0 = 0; k0 < KP; k0 += 4)
                        apn_mfma(Y2[(mb * 16 + lr) * Gm::Y2_SM + (k0 + lq) * Gm::Y2_SK], Xl[(k0 + lq) * Gm::X_SK + nl * Gm::X_SN], p);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float *vp = Vl + (mb * 16 + 4 * lq + r) * Gm::V_SM + nl * Gm::V_SN;
                        const float v = *vp;
                        if (!OBJ) *vp = v / (p[r] + P.eps);
                        else if (LOSS == APN_FROBENIUS) {
                            const double d = (double)v - (double)p[r];
                            obj += d * d;
                        } else                                                   // (beyond the edges v = p = 0)
                            obj += v > 0.0f ? (double)v * log((double)v / ((double)p[r] + (double)P.eps)) - (double)v + (double)p[r] : (double)p[r];
                    }
                }
                if (!OBJ) __syncthreads();
            }
            if (!OBJ) {
#pragma unroll
                for (int c = 0; c < APN_MC; c += 4) {
                    const float v = Vl[(c + lq) * Gm::V_SM + nl * Gm::V_SN];
#pragma unroll
                    for (int kb = 0; kb < NB; ++kb) apn_mfma(Yl[(c + lq) * Gm::Y_SM + (kb * 16 + lr) * Gm::Y_SK], v, acc[kb]);
                }
            }
        }
        if (OBJ) {
            double *red = reinterpret_cast<double *>(ap_smem);
            __syncthreads();
            red[tid] = obj;
            __syncthreads();
            if (tid == 0) {
                double s = 0.0;
                for (int i = 0; i < APN_THREADS; ++i) s += red[i];
                P.part[item] = s;
            }
        } else {
            float den[NB][4];
#pragma unroll
            for (int kb = 0; kb < NB; ++kb) {
                if (LOSS == APN_FROBENIUS) {
                    float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int k0 = 0; k0 < KP; k0 += 4)
                        apn_mfma(Gl[(k0 + lq) * Gm::PROW + kb * 16 + lr], Xl[(k0 + lq) * Gm::X_SK + nl * Gm::X_SN], d);
#pragma unroll
                    for (int r = 0; r < 4; ++r) den[kb][r] = d[r] + P.eps;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int k = kb * 16 + 4 * lq + r;
                        den[kb][r] = (k < K ? P.S[b * K + k] : 0.0f) + P.eps;
                    }
                }
            }
            __syncthreads();                                         // every read of X as an operand is done
#pragma unroll
            for (int kb = 0; kb < NB; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = kb * 16 + 4 * lq + r;
                    float *xp = Xl + k * Gm::X_SK + nl * Gm::X_SN;
                    if (k < K) *xp = *xp * acc[kb][r] / den[kb][r];  // (rows beyond K hold zeros and are not stored)
                }
            __syncthreads();
            apn_move_x<KP, SIDE, true>(Wb, Hb, n0, N, K, P.T, Xl);
        }
    }
}

// G = Y^T Y (Frobenius) or S = the sums of Y over the walk axis (KL) of the factor that the half-step SIDE holds.
template <int KP, int LOSS, int SIDE>
__global__ void __launch_bounds__(APN_THREADS) ap_nmf_gram_kernel(ApNmfParams P) {
    using Gm = ApnGeom<KP, SIDE>;
    constexpr int NB = KP / 16;
    float *Yl = reinterpret_cast<float *>(ap_smem);
    float *Gs = Yl + Gm::Y_FLOATS;                                   // [KP][KP], Frobenius
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int K = P.K;
    const int64_t M = SIDE == 0 ? P.F : P.T;
    for (int64_t b = blockIdx.x; b < P.n_items; b += gridDim.x) {
        const float *Wb = P.W + b * P.F * K, *Hb = P.H + b * (int64_t)K * P.T;
        float acc[NB][NB][4];
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0f;
        float s = 0.0f;
        for (int64_t m0 = 0; m0 < M; m0 += APN_MC) {
            __syncthreads();
            apn_stage_y<KP, SIDE, false>(Wb, Hb, m0, M, K, P.T, Yl, nullptr);
            __syncthreads();
            if (LOSS == APN_FROBENIUS) {
#pragma unroll
                for (int c = 4 * wv; c < APN_MC; c += 16) {
                    float y[NB];
#pragma unroll
                    for (int i = 0; i < NB; ++i) y[i] = Yl[(c + lq) * Gm::Y_SM + (i * 16 + lr) * Gm::Y_SK];
#pragma unroll
                    for (int i = 0; i < NB; ++i)
#pragma unroll
                        for (int j = 0; j < NB; ++j) apn_mfma(y[i], y[j], acc[i][j]);
                }
            } else if (tid < KP) {
                for (int m = 0; m < APN_MC; ++m) s += Yl[m * Gm::Y_SM + tid * Gm::Y_SK];
            }
        }
        if (LOSS == APN_FROBENIUS) {
            for (int w = 0; w < APN_THREADS / 64; ++w) {                 // the waves' shares, in wave order
                __syncthreads();
                if (wv == w)
#pragma unroll
                    for (int i = 0; i < NB; ++i)
#pragma unroll
                        for (int j = 0; j < NB; ++j)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                float *g = Gs + (i * 16 + 4 * lq + r) * KP + j * 16 + lr;
                                *g = w == 0 ? acc[i][j][r] : *g + acc[i][j][r];
                            }
            }
            __syncthreads();
            for (int idx = tid; idx < KP * KP; idx += APN_THREADS) {
                const int k1 = idx / KP, k = idx % KP;
                if (k1 < K && k < K) P.G[(b * K + k1) * K + k] = Gs[idx];
            }
        } else if (tid < K) P.S[b * K + tid] = s;
    }
}

__global__ void __launch_bounds__(APN_THREADS) ap_nmf_objsum_kernel(ApNmfParams P) {
    for (int64_t b = (int64_t)blockIdx.x * APN_THREADS + threadIdx.x; b < P.B; b += (int64_t)gridDim.x * APN_THREADS) {
        double s = 0.0;
        for (int64_t i = 0; i < P.n_tiles; ++i) s += P.part[b * P.n_tiles + i];
        P.out[b] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// which instantiation and how much LDS; the sequence of launches (shared by nmf.hip and the CPU twin)
// ---------------------------------------------------------------------------------------------------------------------
typedef void (*ApNmfKernel)(ApNmfParams);

template <int KP>
static inline ApNmfKernel apn_kernel_kp(int kind, int loss, int side, int *lds) {
    if (kind == APN_GRAM) {
        *lds = side ? ApnGeom<KP, 1>::gram_bytes(loss) : ApnGeom<KP, 0>::gram_bytes(loss);
        if (loss == APN_FROBENIUS) return side ? ap_nmf_gram_kernel<KP, APN_FROBENIUS, 1> : ap_nmf_gram_kernel<KP, APN_FROBENIUS, 0>;
        return side ? ap_nmf_gram_kernel<KP, APN_KL, 1> : ap_nmf_gram_kernel<KP, APN_KL, 0>;
    }
    if (kind == APN_UPDATE) {
        *lds = side ? ApnGeom<KP, 1>::tile_bytes(loss, false) : ApnGeom<KP, 0>::tile_bytes(loss, false);
        if (loss == APN_FROBENIUS) return side ? ap_nmf_tile_kernel<KP, APN_FROBENIUS, 1, false> : ap_nmf_tile_kernel<KP, APN_FROBENIUS, 0, false>;
        return side ? ap_nmf_tile_kernel<KP, APN_KL, 1, false> : ap_nmf_tile_kernel<KP, APN_KL, 0, false>;
    }
    *lds = ApnGeom<KP, 0>::tile_bytes(loss, true);
    return loss == APN_FROBENIUS ? ap_nmf_tile_kernel<KP, APN_FROBENIUS, 0, true> : ap_nmf_tile_kernel<KP, APN_KL, 0, true>;
}

static inline ApNmfKernel apn_kernel(int K, int kind, int loss, int side, int *lds) {
    const int kp = ap_nmf_kp(K);
    return kp == 16 ? apn_kernel_kp<16>(kind, loss, side, lds) : kp == 32 ? apn_kernel_kp<32>(kind, loss, side, lds)
                                                                          : apn_kernel_kp<64>(kind, loss, side, lds);
}

// go(kernel, grid, lds_bytes, P) enqueues one launch and returns a status
template <class Go>
static inline int apn_launch(Go &go, ApNmfParams P, int kind, int loss, int side) {
    int lds = 0;
    ApNmfKernel kern = apn_kernel(P.K, kind, loss, side, &lds);
    P.n_tiles = ((side ? P.F : P.T) + APN_NT - 1) / APN_NT;
    P.n_items = kind == APN_GRAM ? P.B : P.B * P.n_tiles;
    return go(kern, ap_nmf_grid(P.n_items), lds, P);
}

template <class Go>
static inline int apn_iterate(Go &go, const ApNmfParams &P, int n_iter, int loss, int update_w) {
    for (int it = 0; it < n_iter; ++it) {
        int rc = AP_OK;
        if (it == 0 || update_w) rc = apn_launch(go, P, APN_GRAM, loss, 0);        // a fixed W keeps its G and S
        if (rc == AP_OK) rc = apn_launch(go, P, APN_UPDATE, loss, 0);
        if (rc == AP_OK && update_w) rc = apn_launch(go, P, APN_GRAM, loss, 1);
        if (rc == AP_OK && update_w) rc = apn_launch(go, P, APN_UPDATE, loss, 1);
        if (rc != AP_OK) return rc;
    }
    return AP_OK;
}

template <class Go>
static inline int apn_objective(Go &go, ApNmfParams P, int loss, double *out) {
    if (!out) AP_FAIL(AP_ERR_INVALID, "nmf_objective: NULL buffer");
    P.out = out;
    int rc = apn_launch(go, P, APN_OBJECTIVE, loss, 0);
    if (rc != AP_OK) return rc;
    P.n_tiles = (P.T + APN_NT - 1) / APN_NT;
    return go(ap_nmf_objsum_kernel, ap_grid_1d(P.B, APN_THREADS, 1024), 0, P);
}
