// TEST INFRASTRUCTURE ONLY.  The feature kernels (kernels_features.h) built for the CPU through emu_shim.h, behind
// emu_ twins of the C entry points that take HOST pointers.  Same validation and geometry (the ap_prepare_* functions
// of ap_launch.h), same kernel bodies; the extra arguments override what the product's heuristics would hide
// (frames per workgroup, the span / chunked / generic routes, the grid of the grid-stride kernels).
//
// Static LDS: kernels_features.h is the one header that declares static __shared__ arrays.  The shim defines
// __shared__ away, which would give every emulated thread a private copy; for this header alone it becomes
// `static`: one instance per kernel, which is the right model because emu_launch runs workgroups one after another.
// The headers included before the switch are `#pragma once`, so their `extern __shared__ char ap_smem[]` stays as it
// was.
#include "emu_shim.h"

alignas(16) char ap_smem[160 * 1024];

// ---- lane operations the feature kernels use (wave w = threads [64 w, 64 w + 64)) --------------------------------
inline int emu_xchg_i[1024];
inline float __shfl_xor(float x, int mask, int) { return emu_lane_xor(x, mask); }
inline int __shfl_xor(int x, int mask, int) {
    emu_xchg_i[threadIdx.x] = x;
    emu_wave_sync();
    const int y = emu_xchg_i[threadIdx.x ^ (unsigned)mask];
    emu_wave_sync();
    return y;
}
inline float __shfl(float x, int lane, int) { return emu_lane_perm(x, lane); }
inline float __shfl_up(float x, unsigned d, int) {          // lanes below d keep their own value
    emu_xchg[threadIdx.x] = x;
    emu_wave_sync();
    const unsigned lane = threadIdx.x & 63u;
    const float y = lane >= d ? emu_xchg[threadIdx.x - d] : x;
    emu_wave_sync();
    return y;
}

#include "../../mlx-audio-primitives_amd/csrc/ap_launch.h"
#include "../../mlx-audio-primitives_amd/csrc/kernels_generic.h"
#include "../../mlx-audio-primitives_amd/csrc/kernels_bigfft.h"

#undef __shared__
#define __shared__ static
#include "../../mlx-audio-primitives_amd/csrc/kernels_features.h"
#undef __shared__
#define __shared__

static thread_local char g_err[512] = "";
char *ap_error_buffer() { return g_err; }
void ap_set_error(const char *msg) { std::snprintf(g_err, sizeof(g_err), "%s", msg); }

static unsigned emu_grid(int64_t product, int override_grid) { return (unsigned)(override_grid > 0 ? override_grid : product); }

extern "C" {

const char *emu_features_last_error() { return g_err; }
int emu_features_lds_overruns() { return emu_lds_overruns; }
int emu_features_guard_selftest() {
    const int before = emu_lds_overruns;
    emu_lds_limit(1024);
    emu_launch(1, 64, [&] { if (threadIdx.x == 0) ap_smem[2000] = 1; });
    const int seen = emu_lds_overruns - before;
    emu_lds_overruns = before;
    return seen;
}
int emu_features_max_blocks() { return APF_MAX_BLOCKS; }

int emu_spectral_stats_f32(const float *S, int is_complex, int64_t B, int64_t F, int64_t T, const float *freq, float power,
                           const float *centroid_in, float p, int norm, float roll_percent, float amin, float *centroid,
                           float *bandwidth, float *rolloff, float *flatness) {
    ApSpectralParams P;
    int64_t grid = 0;
    int rc = ap_prepare_spectral_stats(P, S, is_complex, B, F, T, freq, power, centroid_in, p, norm, roll_percent, amin,
                                       centroid, bandwidth, rolloff, flatness, APF_TX, &grid);
    if (rc != AP_OK || grid == 0) return rc;
    emu_launch((unsigned)grid, APF_TX * APF_TY, [&] { ap_spectral_stats_kernel(P); });
    return AP_OK;
}

// G > 0 overrides the frames per workgroup; G == 0 keeps the FULL tile of the block kernel (the product halves it
// until 1024 workgroups exist) and the span kernel's own choice.  used[0] = route, used[1] = G that ran.
int emu_frame_stats_f32(const float *y, int64_t B, int64_t L, int frame_length, int hop, int center, int pad_mode,
                        int64_t T, float *rms, float *zcr, int force_span, int G, int *used) {
    ApFrameBlocksParams Q;
    ApFrameStatsParams P;
    int route = 0, lds = 0;
    int64_t grid = 0;
    int rc = ap_prepare_frame_stats(Q, P, y, B, L, frame_length, hop, center, pad_mode, T, rms, zcr, APF_MAX_BLOCKS,
                                    force_span ? 0 : 1, 0, &route, &grid, &lds);
    if (used) { used[0] = route; used[1] = 0; }
    if (rc != AP_OK || route == 0) return rc;
    if (route == AP_FRAME_ROUTE_BLOCKS) {
        if (G > 0) {
            Q.G = G;
            Q.tiles_per_clip = (T + G - 1) / G;
            grid = Q.tiles_per_clip * B;
        }
        if (used) used[1] = Q.G;
        // the kernel's three static arrays hold APF_MAX_BLOCKS slots: a tile of G frames uses G + m - 1 of them
        if (Q.G < 1 || Q.G + Q.m - 1 > APF_MAX_BLOCKS)
            AP_FAIL(AP_ERR_INVALID, "emu: G = %d frames of m = %d blocks need %d slots, the kernel has %d", Q.G, Q.m,
                    Q.G + Q.m - 1, APF_MAX_BLOCKS);
        emu_launch((unsigned)grid, AP_BLOCK, [&] { ap_frame_stats_blocks_kernel(Q); });
        return AP_OK;
    }
    if (G > 0) {
        P.G = G;
        P.tiles_per_clip = (T + G - 1) / G;
        grid = P.tiles_per_clip * B;
        lds = (int)(((int64_t)(G - 1) * hop + frame_length) * sizeof(float));
    }
    if (used) used[1] = P.G;
    if (lds > AP_LDS_MAX) AP_FAIL(AP_ERR_INVALID, "emu: span of %d bytes", lds);
    emu_lds_limit(lds);
    emu_launch((unsigned)grid, AP_BLOCK, [&] { ap_frame_stats_kernel(P); });
    return AP_OK;
}

// used[0] = 1 when the four-samples-per-thread kernel ran
int emu_preemphasis_f32(const float *y, int64_t B, int64_t L, float coef, const float *zi, float *out, float *zf,
                        int grid_override, int *used) {
    int quads = 0, grid = 0;
    int rc = ap_prepare_preemphasis(y, B, L, coef, out, &quads, &grid);
    if (rc != AP_OK) return rc;
    if (used) used[0] = quads;
    if (quads) emu_launch(emu_grid(grid, grid_override), AP_BLOCK, [&] { ap_preemphasis4_kernel(y, B, L, coef, zi, out, zf); });
    else emu_launch(emu_grid(grid, grid_override), AP_BLOCK, [&] { ap_preemphasis_kernel(y, B, L, coef, zi, out, zf); });
    return AP_OK;
}

int64_t emu_deemphasis_workspace_floats(int64_t B, int64_t L) {
    if (B <= 0 || L <= 0) return 0;
    const int64_t chunk = ap_deemphasis_chunk((int64_t)AP_BLOCK * APD_PER);
    return B * ((L + chunk - 1) / chunk);
}

// force: 0 = the product's choice (chunked when ws is given and the clip has more than one chunk), 1 = one workgroup
// per clip whatever the length, 2 = the chunked pair even for a clip of one chunk, 3 = the same with the workgroups
// of the second pass run one at a time in DESCENDING order (a GPU runs them in any order: nothing may depend on the
// last chunk being the last to finish).  used[0] = 1 when chunked.
int emu_deemphasis_f32(const float *y, int64_t B, int64_t L, float coef, const float *zi, float *out, float *zf, float *ws,
                       int force, int *used) {
    int64_t chunk = 0, n_chunks = 0;
    int chunked = 0;
    int rc = ap_prepare_deemphasis(y, B, L, coef, out, ws, (int64_t)AP_BLOCK * APD_PER, &chunk, &n_chunks, &chunked);
    if (rc != AP_OK) return rc;
    if (force == 1) chunked = 0;
    if (force == 2 || force == 3) {
        if (!ws) AP_FAIL(AP_ERR_INVALID, "emu: the chunked route needs a workspace");
        chunked = 1;
    }
    if (used) used[0] = chunked;
    if (chunked) {
        emu_launch((unsigned)(B * n_chunks), AP_BLOCK,
                   [&] { ap_deemphasis_kernel<1>(y, L, coef, zi, zi ? 0 : 1, out, zf, chunk, (int)n_chunks, ws); });
        if (force == 3) {
            for (int64_t wg = B * n_chunks - 1; wg >= 0; --wg)
                emu_launch(1, AP_BLOCK, [&] {
                    blockIdx.x = (unsigned)wg;
                    ap_deemphasis_kernel<2>(y, L, coef, zi, zi ? 0 : 1, out, zf, chunk, (int)n_chunks, ws);
                });
            return AP_OK;
        }
        emu_launch((unsigned)(B * n_chunks), AP_BLOCK,
                   [&] { ap_deemphasis_kernel<2>(y, L, coef, zi, zi ? 0 : 1, out, zf, chunk, (int)n_chunks, ws); });
        return AP_OK;
    }
    emu_launch((unsigned)B, AP_BLOCK, [&] { ap_deemphasis_kernel<0>(y, L, coef, zi, zi ? 0 : 1, out, zf, L, 1, nullptr); });
    return AP_OK;
}

// used[0] = 1 when the rows kernel ran
int emu_savgol_f32(const float *x, int64_t outer, int64_t n, int64_t inner, const float *taps, int width, int mode,
                   float cval, const float *edge, float *out, int force_generic, int grid_override, int *used) {
    int64_t chunks = 0, grid = 0;
    int rc = ap_prepare_savgol(x, outer, n, inner, taps, width, mode, edge, out, AP_BLOCK * APSG_PER, &chunks, &grid);
    if (rc != AP_OK) return rc;
    if (force_generic && chunks > 0) {
        chunks = 0;
        grid = ap_grid_1d(outer * n * inner, AP_BLOCK, kApStreamGrid);
    }
    if (used) used[0] = chunks > 0;
    if (chunks > 0) {
        emu_launch((unsigned)grid, AP_BLOCK,
                   [&] { ap_savgol_rows_kernel(x, outer, (int)n, (int)chunks, taps, width, mode, cval, edge, out); });
        return AP_OK;
    }
    emu_launch(emu_grid(grid, grid_override), AP_BLOCK,
               [&] { ap_savgol_kernel(x, outer, n, inner, taps, width, mode, cval, edge, out); });
    return AP_OK;
}

int emu_extend_f32(const float *x, int64_t B, int64_t L, int64_t n_ext, int mode, float *out, int grid_override) {
    int grid = 0;
    int rc = ap_prepare_extend(x, B, L, n_ext, mode, out, &grid);
    if (rc != AP_OK) return rc;
    emu_launch(emu_grid(grid, grid_override), AP_BLOCK, [&] { ap_extend_kernel(x, B, L, n_ext, mode, out); });
    return AP_OK;
}

// the y dimension of the grid (one row per band) is a host loop here: gridDim.y once, blockIdx.y inside the body
int emu_spectral_contrast_f32(const float *S, int64_t B, int64_t F, int64_t T, const int32_t *bands, int n_bands, int linear,
                              float *out) {
    int64_t blocks = 0;
    int rc = ap_prepare_spectral_contrast(S, B, F, T, bands, n_bands, out, &blocks);
    if (rc != AP_OK) return rc;
    gridDim.y = (unsigned)n_bands;
    for (int band = 0; band < n_bands; ++band)
        emu_launch((unsigned)blocks, AP_BLOCK, [&] {
            blockIdx.y = (unsigned)band;
            ap_spectral_contrast_kernel(S, B, F, T, bands, linear, out);
        });
    gridDim.y = 1;
    return AP_OK;
}

int emu_acf_peaks_f32(const float *r, int64_t rows, int n_lag, int min_lag, int max_lag, float threshold, float sr, float *f0,
                      unsigned char *voiced, float *periodicity) {
    int64_t grid = 0;
    int rc = ap_prepare_acf_peaks(r, rows, n_lag, min_lag, &grid);
    if (rc != AP_OK) return rc;
    emu_launch((unsigned)grid, AP_BLOCK,
               [&] { ap_acf_peak_kernel(r, rows, n_lag, min_lag, max_lag, threshold, sr, f0, voiced, periodicity); });
    return AP_OK;
}

int emu_pcm16_to_f32(const int16_t *x, int64_t n, float scale, float *out, int grid_override) {
    int grid = 0;
    int rc = ap_prepare_pcm16(x, n, out, &grid);
    if (rc != AP_OK || grid == 0) return rc;
    emu_launch(emu_grid(grid, grid_override), AP_BLOCK, [&] { ap_pcm16_to_f32_kernel(x, n, scale, out); });
    return AP_OK;
}

// ---- the autocorrelation glue kernels on their own -----------------------------------------------------------------
int emu_row_mean_f32(const float *y, int64_t B, int64_t n, float *mean) {
    emu_launch((unsigned)B, AP_BLOCK, [&] { ap_row_mean_kernel(y, n, mean); });
    return AP_OK;
}
int emu_autocorr_pad_f32(const float *y, int64_t B, int64_t n, int64_t N, const float *mean, float *padded, int grid_override) {
    emu_launch(emu_grid(ap_grid_1d(B * N, AP_BLOCK, kApStreamGrid), grid_override), AP_BLOCK,
               [&] { ap_autocorr_pad_kernel(y, B, n, N, mean, padded); });
    return AP_OK;
}
int emu_power_spectrum_f32(float *X, int64_t count, int grid_override) {
    emu_launch(emu_grid(ap_grid_1d(count, AP_BLOCK, kApStreamGrid), grid_override), AP_BLOCK,
               [&] { ap_power_spectrum_kernel(reinterpret_cast<ap_float2 *>(X), count); });
    return AP_OK;
}
int emu_autocorr_finish_f32(const float *r, int64_t B, int64_t N, int64_t max_lag, int normalize, float *out, int grid_override) {
    emu_launch(emu_grid(ap_grid_1d(B * max_lag, AP_BLOCK, kApStreamGrid), grid_override), AP_BLOCK,
               [&] { ap_autocorr_finish_kernel(r, B, N, max_lag, normalize, out); });
    return AP_OK;
}

int64_t emu_autocorrelation_nfft(int64_t n) {
    int64_t N = 1;
    while (N < 2 * n - 1) N *= 2;
    return N;
}
int emu_features_cfft_split(int64_t N, int *N1, int *N2) { return ap_cfft_split(N, N1, N2); }

static int emu_cfft_leg(const ApCfftParams &C, int64_t B) {
    emu_lds_limit(C.tile.lds_bytes);
    emu_launch((unsigned)(C.tiles_per_signal * B), AP_BLOCK, [&] { ap_cfft_strided_kernel(C); });
    return AP_OK;
}

// the launch sequence of ap_autocorrelation_f32, kernel for kernel; ws holds 4 B N + B floats
int emu_autocorrelation_f32(const float *y, int64_t B, int64_t n, int64_t max_lag, int normalize, int center, const float *tw1,
                            const float *tw2, float *ws, float *out) {
    if (!y || !out || !ws || !tw1 || !tw2) AP_FAIL(AP_ERR_INVALID, "autocorrelation: NULL buffer");
    if (B <= 0 || n <= 0)
        AP_FAIL(AP_ERR_INVALID, "signal must be 1-dimensional (samples,) or 2-dimensional (batch, samples)");
    if (max_lag <= 0 || max_lag > n) AP_FAIL(AP_ERR_INVALID, "autocorrelation: max_lag must be in [1, n]");
    const int64_t N = emu_autocorrelation_nfft(n);
    int n1, n2;
    if (ap_cfft_split(N, &n1, &n2) != 0)
        AP_FAIL(AP_ERR_UNSUPPORTED, "autocorrelation: n_fft %lld does not split into two on-chip legs", (long long)N);
    ap_float2 *bufA = reinterpret_cast<ap_float2 *>(ws);
    ap_float2 *bufB = bufA + B * N;
    float *padded = reinterpret_cast<float *>(bufB);
    float *mean = ws + 4 * B * N;
    if (center) emu_row_mean_f32(y, B, n, mean);
    emu_autocorr_pad_f32(y, B, n, N, center ? mean : nullptr, padded, 0);
    ApCfftParams L1, L2;
    int rc = ap_prepare_cfft(L1, L2, padded, bufA, bufB, B, N, n1, n2, tw1, tw2, 0, 1, 0, 1.0f);
    if (rc != AP_OK) return rc;
    emu_cfft_leg(L1, B);
    emu_cfft_leg(L2, B);
    emu_power_spectrum_f32(reinterpret_cast<float *>(bufB), B * N, 0);
    float *r = reinterpret_cast<float *>(bufB);
    rc = ap_prepare_cfft(L1, L2, bufB, bufA, r, B, N, n1, n2, tw1, tw2, 1, 0, 1, (float)(1.0 / (double)N));
    if (rc != AP_OK) return rc;
    emu_cfft_leg(L1, B);
    emu_cfft_leg(L2, B);
    emu_autocorr_finish_f32(r, B, N, max_lag, normalize, out, 0);
    return AP_OK;
}

}  // extern "C"
