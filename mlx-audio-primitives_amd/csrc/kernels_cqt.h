// Constant-Q / variable-Q transform in direct form (cqt.py: cqt, vqt; the filter bank of librosa 0.10, evaluated exactly:
// no octave recursion, no resampling, no sparsified basis).
//
// ap_cqt_kernel.  For y (B, L), a bank of n_bins complex filters g_k with L_k = tap_offset[k+1] - tap_offset[k] taps
// stored back to back (taps[tap_offset[k] + j] = g_k[m0[k] + j]) and T = 1 + L / hop frames:
//   C[b,k,t] = scale[k] sum_{m = m0[k]}^{m0[k] + L_k - 1} ypad[b, t hop + m] conj(g_k[m])
//   ypad: y outside [0, L) by pad_mode (constant: 0; edge: the nearest sample; reflect: NumPy's "reflect", period
//   2 (L - 1), any distance), computed on load: the padded signal is never stored.
//
//   A workgroup (4 waves) owns one clip, a tile of up to APCQ_TT = 32 frames and a group of APCQ_K = 4 adjacent bins,
//   whose lengths lie within 2^(3 / bins_per_octave) of each other in a real bank.  The group's tap range
//   [lo, hi) = [min m0, max (m0 + L_k)) is walked in chunks of APCQ_C = 256 taps, so nothing but the cap limits L_k.
//
//   Signal.  Frame f, chunk c, column u meets sample t0 hop + lo + q, q = f hop + 256 c + u: the frames of a tile and the
//   chunks of a filter slide over one stretch of the clip.  The tile keeps that stretch in a ring in LDS, slot q mod
//   16384: the (tt - 1) hop + 256 samples chunk 0 needs are loaded once, every later chunk loads the 256 samples the
//   stretch advances by (one per thread) instead of the 32 x 256 its frames meet.  A tile has as many frames as the
//   ring holds, tt = min(32, 1 + 16128 / hop): 32 up to hop 520, one beyond hop 16128, so any hop is served.  The
//   first 256 slots are mirrored behind the ring, so a frame's run of 256 samples never wraps and its reads are one
//   base address plus immediate offsets.  Positions outside the clip cost nothing for constant padding and take the
//   pad arithmetic (one 64-bit modulo for reflect, any distance) only where they occur.
//
//   Taps.  Per chunk a thread loads column tid of each of the 4 bins (0 outside a bin's own range) and the ring's new
//   sample into registers *before* the chunk in LDS is summed and writes them to LDS after it: the loads' latency lies
//   under the 128 packed FMAs per lane of a chunk.
//
//   Sum.  Lanes split the tap index, u = 64 j + lane: signal and tap reads are unit-stride in LDS, free of bank
//   conflicts whatever the hop.  Every wave holds APCQ_R = 8 frames x 4 bins of complex partial sums in registers
//   (64 VGPRs); a step reads 8 + 4 LDS values and issues 32 packed FMAs, (re, im) += (y, y) (g_re, g_im); the conjugate
//   is the sign of the stored imaginary part.  After the last chunk the 64 lanes' partial sums are joined through LDS
//   (a lane adds 32 lanes' values in lane order, then the two halves meet), scale[k] is applied and runs of 8 frames
//   leave per bin.
//
//   Every product is an fmaf and every sum has a fixed order, so the CPU twin (tests/emu/emu_cqt.cpp) gives the
//   device's bits.  The longest chain of dependent additions for band k is
//   d_k = (APCQ_C / 64) n_chunks + 31 + 1,  n_chunks = ceil((hi - lo) / APCQ_C) of the band's group.
//   Tiles are numbered group-major from bin 0: in a real bank the longest filters are dispatched first.
#pragma once
#include <cmath>

#include "ap_launch.h"
#include "fft_lds.h"

extern __shared__ __attribute__((aligned(16))) char ap_smem[];

#define APCQ_WAVES 4            // waves per workgroup; wave w owns the frames t0 + 8 w .. t0 + 8 w + 7 (those below t0 + tt)
#define APCQ_R 8                // frames per wave
#define APCQ_K 4                // bins per workgroup
#define APCQ_TT (APCQ_WAVES * APCQ_R)
#define APCQ_C 256              // taps per chunk = threads per workgroup: a thread stages column u = tid
#define APCQ_RED 32             // values joined per round of the reduction
#define APCQ_RED_STRIDE 65      // floats between the rows of the reduction buffer (odd: the column reads spread over the banks)
#define APCQ_MAX_TAPS (1 << 20) // cap on L_k and on |m0[k]|: with L <= 2^30 every sample position of a tile fits int32
#define APCQ_RING 16384         // samples of the signal ring (a power of two): (tt - 1) hop + APCQ_C of them are live
#define APCQ_LDS_BYTES ((APCQ_RING + APCQ_C) * 4 + APCQ_K * APCQ_C * 8)

static_assert(APCQ_C == 64 * APCQ_WAVES, "a thread stages one column of the chunk");
static_assert(2 * APCQ_R * APCQ_K == 2 * APCQ_RED, "two rounds join a wave's partial sums");
static_assert(APCQ_WAVES * APCQ_RED * APCQ_RED_STRIDE * 4 <= APCQ_LDS_BYTES, "the reduction buffer lies over the staging area");

struct ApCqtParams {
    const float *y;             // (B, L)
    const ap_float2 *taps;      // (tap_offset[n_bins])
    const int64_t *tap_offset;  // (n_bins + 1)
    const int32_t *m0;          // (n_bins)
    const float *scale;         // (n_bins)
    float *out;                 // (B, n_bins, out_rs) complex as (re, im)
    int64_t B, L, T, out_rs, n_tiles, tiles_per_group;
    int hop, pad_mode, n_bins, n_groups, n_tt, lds_bytes;
    int tt, span;               // frames per tile (<= APCQ_TT), live samples of the ring = (tt - 1) hop + APCQ_C <= APCQ_RING
};

// Validation and the launch geometry of ap_cqt_f32 (and of its emulator twin).  The tables are device arrays: their
// contents (L_k <= ap_cqt_max_taps(), ascending offsets) are the caller's to keep.
static inline int ap_prepare_cqt(ApCqtParams &P, const float *y, int64_t B, int64_t L, int hop, int pad_mode, const float *taps,
                                 const int64_t *tap_offset, const int32_t *m0, const float *scale, int n_bins, int64_t T,
                                 float *out, int64_t out_rs) {
    if (!y || !taps || !tap_offset || !m0 || !scale || !out) AP_FAIL(AP_ERR_INVALID, "cqt: NULL buffer");
    if (B <= 0 || L <= 0) AP_FAIL(AP_ERR_INVALID, "cqt: signal must be non-empty, got (%lld, %lld)", (long long)B, (long long)L);
    if (hop < 1) AP_FAIL(AP_ERR_INVALID, "hop_length must be positive, got %d", hop);
    if (n_bins < 1) AP_FAIL(AP_ERR_INVALID, "n_bins must be positive, got %d", n_bins);
    if (pad_mode < AP_PAD_CONSTANT || pad_mode > AP_PAD_REFLECT)
        AP_FAIL(AP_ERR_INVALID, "Unknown pad_mode. Supported: reflect, constant, edge");
    if (T != 1 + L / hop)
        AP_FAIL(AP_ERR_INVALID, "cqt: n_frames mismatch (got %lld, expected %lld)", (long long)T, (long long)(1 + L / hop));
    if (out_rs < T) AP_FAIL(AP_ERR_INVALID, "cqt: out_row_stride (%lld) must be >= T = %lld", (long long)out_rs, (long long)T);
    if (L > ((int64_t)1 << 30)) AP_FAIL(AP_ERR_UNSUPPORTED, "cqt: L must be <= 2^30");
    if ((double)B * (double)n_bins * (double)out_rs * 8.0 > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "cqt: more than 2^63 bytes");
    P.y = y; P.taps = reinterpret_cast<const ap_float2 *>(taps); P.tap_offset = tap_offset; P.m0 = m0; P.scale = scale; P.out = out;
    P.B = B; P.L = L; P.T = T; P.out_rs = out_rs;
    P.hop = hop; P.pad_mode = pad_mode; P.n_bins = n_bins;
    P.n_groups = (n_bins + APCQ_K - 1) / APCQ_K;
    // as many frames per tile as the ring holds: 32 up to hop 520, one beyond hop 16128
    const int64_t fit = 1 + (int64_t)(APCQ_RING - APCQ_C) / hop;
    P.tt = (int)(fit < APCQ_TT ? fit : APCQ_TT);
    P.span = (P.tt - 1) * hop + APCQ_C;
    P.n_tt = (int)((T + P.tt - 1) / P.tt);
    P.tiles_per_group = B * P.n_tt;
    if ((double)P.tiles_per_group * (double)P.n_groups > 9.0e18) AP_FAIL(AP_ERR_UNSUPPORTED, "cqt: too many tiles");
    P.n_tiles = P.tiles_per_group * P.n_groups;
    P.lds_bytes = APCQ_LDS_BYTES;
    return AP_OK;
}

static inline int ap_cqt_grid(const ApCqtParams &P) { return (int)(P.n_tiles < (1 << 24) ? P.n_tiles : (1 << 24)); }

#ifdef AP_HOST_EMU
AP_DEV float apcq_lane_xor(float x, int mask) { return emu_lane_xor(x, mask); }
AP_DEV ap_float2 apcq_fma(float y, ap_float2 g, ap_float2 a) {
    ap_float2 r;
    r.x = fmaf(y, g.x, a.x);
    r.y = fmaf(y, g.y, a.y);
    return r;
}
AP_DEV ap_float2 apcq_zero() { ap_float2 r; r.x = 0.0f; r.y = 0.0f; return r; }
#else
AP_DEV float apcq_lane_xor(float x, int mask) { return __shfl_xor(x, mask, 64); }
AP_DEV ap_float2 apcq_fma(float y, ap_float2 g, ap_float2 a) {        // v_pk_fma_f32
    ap_float2 yy = {y, y};
    return __builtin_elementwise_fma(yy, g, a);
}
AP_DEV ap_float2 apcq_zero() { ap_float2 r = {0.0f, 0.0f}; return r; }
#endif

// ypad[i]: i fits 32 bits (|t0 hop + lo| <= 2^30 + 2^20 and a tile's relative positions stay below 2^22)
AP_DEV float apcq_sample(const float *yb, int i, int L, int mode) {
    if ((unsigned)i < (unsigned)L) return yb[i];
    if (mode == AP_PAD_CONSTANT) return 0.0f;
    if (mode == AP_PAD_EDGE) return yb[i < 0 ? 0 : L - 1];
    if (L == 1) return yb[0];
    const int64_t p = 2 * ((int64_t)L - 1);
    int64_t r = (int64_t)i % p;
    if (r < 0) r += p;
    return yb[r < L ? r : p - r];
}

// relative position q of the tile's signal -> its ring slot; the first APCQ_C slots are mirrored behind the ring, so
// that a run of APCQ_C samples never wraps
AP_DEV void apcq_ring_store(float *ring, int q, float v) {
    const int i = q & (APCQ_RING - 1);
    ring[i] = v;
    if (i < APCQ_C) ring[APCQ_RING + i] = v;
}

// One thread's share of chunk c, into registers: the tap of each bin at column `tid` (0 outside the bin's own range)
// and, from the second chunk on, the one sample by which the ring advances.
AP_DEV void apcq_load(const ApCqtParams &P, const float *yb, int base0, int lo, int c, const int (&m0k)[APCQ_K],
                      const int (&Lk)[APCQ_K], const int64_t (&offk)[APCQ_K], int tid, float &nv, ap_float2 (&tv)[APCQ_K]) {
    const int m = lo + c * APCQ_C + tid;
#pragma unroll
    for (int kk = 0; kk < APCQ_K; ++kk) {
        const int j = m - m0k[kk];
        tv[kk] = (j >= 0 && j < Lk[kk]) ? P.taps[offk[kk] + j] : apcq_zero();
    }
    if (c > 0) nv = apcq_sample(yb, base0 + (c - 1) * APCQ_C + P.span + tid, (int)P.L, P.pad_mode);
}

__global__ void __launch_bounds__(64 * APCQ_WAVES) ap_cqt_kernel(ApCqtParams P) {
    float *ring = reinterpret_cast<float *>(ap_smem);                                  // [APCQ_RING + APCQ_C]
    ap_float2 *tap = reinterpret_cast<ap_float2 *>(ap_smem + (APCQ_RING + APCQ_C) * 4); // [APCQ_K][APCQ_C]
    float *red = reinterpret_cast<float *>(ap_smem);                                   // [APCQ_WAVES][APCQ_RED][65], after the loop
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
        const int g = (int)(tile / P.tiles_per_group);
        const int64_t rem = tile - (int64_t)g * P.tiles_per_group;
        const int64_t b = rem / P.n_tt;
        const int64_t t0 = (rem - b * P.n_tt) * P.tt;
        const int k0 = g * APCQ_K;
        const float *yb = P.y + b * P.L;

        int m0k[APCQ_K], Lk[APCQ_K];
        int64_t offk[APCQ_K];
        int lo = 0x7fffffff, hi = -0x7fffffff;
#pragma unroll
        for (int kk = 0; kk < APCQ_K; ++kk) {
            m0k[kk] = 0; Lk[kk] = 0; offk[kk] = 0;
            if (k0 + kk < P.n_bins) {
                m0k[kk] = P.m0[k0 + kk];
                offk[kk] = P.tap_offset[k0 + kk];
                Lk[kk] = (int)(P.tap_offset[k0 + kk + 1] - offk[kk]);
                if (Lk[kk] > 0) {
                    lo = m0k[kk] < lo ? m0k[kk] : lo;
                    hi = m0k[kk] + Lk[kk] > hi ? m0k[kk] + Lk[kk] : hi;
                }
            }
        }
        const int n_chunks = hi > lo ? (hi - lo + APCQ_C - 1) / APCQ_C : 0;

        ap_float2 acc[APCQ_K][APCQ_R];
#pragma unroll
        for (int kk = 0; kk < APCQ_K; ++kk)
#pragma unroll
            for (int r = 0; r < APCQ_R; ++r) acc[kk][r] = apcq_zero();

        // the tile's signal: relative position q is sample t0 hop + lo + q; frame f, chunk c, column u reads q = f hop + 256 c + u
        const int base0 = (int)(t0 * P.hop + lo);
        if (n_chunks > 0) {
            for (int q0 = 0; q0 < P.span; q0 += 8 * APCQ_C) {
                float fv[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int q = q0 + i * APCQ_C + tid;
                    fv[i] = q < P.span ? apcq_sample(yb, base0 + q, (int)P.L, P.pad_mode) : 0.0f;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int q = q0 + i * APCQ_C + tid;
                    if (q < P.span) apcq_ring_store(ring, q, fv[i]);
                }
            }
        }
        float nv = 0.0f;
        ap_float2 tv[APCQ_K];
        if (n_chunks > 0) apcq_load(P, yb, base0, lo, 0, m0k, Lk, offk, tid, nv, tv);
        for (int c = 0; c < n_chunks; ++c) {
            __syncthreads();                                // the chunk before has been read
#pragma unroll
            for (int kk = 0; kk < APCQ_K; ++kk) tap[kk * APCQ_C + tid] = tv[kk];
            if (c > 0) apcq_ring_store(ring, (c - 1) * APCQ_C + P.span + tid, nv);
            __syncthreads();
            // the next chunk's loads are in flight while this one is summed
            if (c + 1 < n_chunks) apcq_load(P, yb, base0, lo, c + 1, m0k, Lk, offk, tid, nv, tv);
            if (wave * APCQ_R >= P.tt) continue;            // a wave without a frame of the tile (hop > 520)
            const float *sw[APCQ_R];
#pragma unroll
            for (int r = 0; r < APCQ_R; ++r)
                sw[r] = ring + (((unsigned)(wave * APCQ_R + r) * (unsigned)P.hop + (unsigned)(c * APCQ_C)) & (APCQ_RING - 1));
#pragma unroll
            for (int j = 0; j < APCQ_C / 64; ++j) {
                const int u = 64 * j + lane;
                ap_float2 gk[APCQ_K];
#pragma unroll
                for (int kk = 0; kk < APCQ_K; ++kk) gk[kk] = tap[kk * APCQ_C + u];
#pragma unroll
                for (int r = 0; r < APCQ_R; ++r) {
                    const float yv = sw[r][u];
#pragma unroll
                    for (int kk = 0; kk < APCQ_K; ++kk) acc[kk][r] = apcq_fma(yv, gk[kk], acc[kk][r]);
                }
            }
        }

        // join the 64 lanes: value (kk, r, re / im) = 16 kk + 2 r + c, 32 values per round
        __syncthreads();
        float *rw = red + wave * APCQ_RED * APCQ_RED_STRIDE;
        const int v = lane & 31, h = lane >> 5;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int i = 0; i < APCQ_RED; ++i) {
                const int idx = APCQ_RED * p + i;
                const ap_float2 a = acc[idx / (2 * APCQ_R)][(idx / 2) % APCQ_R];
                rw[i * APCQ_RED_STRIDE + lane] = (idx & 1) ? a.y : a.x;
            }
            __syncthreads();
            const float *col = rw + v * APCQ_RED_STRIDE + 32 * h;
            float s = col[0];
#pragma unroll
            for (int i = 1; i < 32; ++i) s += col[i];
            s += apcq_lane_xor(s, 32);
            const int idx = APCQ_RED * p + v;
            const int k = k0 + idx / (2 * APCQ_R);
            const int64_t t = t0 + wave * APCQ_R + (idx / 2) % APCQ_R;
            if (h == 0 && k < P.n_bins && t < P.T && t < t0 + P.tt) {
                const float val = s * P.scale[k];
                P.out[((b * P.n_bins + k) * P.out_rs + t) * 2 + (idx & 1)] = (idx & 1) ? -val : val;   // conj(g)
            }
            __syncthreads();                                // the buffer is free for the next round / tile
        }
    }
}
