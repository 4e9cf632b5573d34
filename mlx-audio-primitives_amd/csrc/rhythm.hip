// Translation unit of the rhythm kernels (kernels_rhythm.h): ap_tempogram_f32, ap_tempo_pick_f32, ap_beat_track_f32.
#include <hip/hip_runtime.h>

#define AP_TU_SECONDARY 1
#include "kernels_rhythm.h"

template <class K, class PP>
static int ap_rhythm_launch(K kern, int grid, int block, const PP &P, void *stream, const char *what) {
    if (P.lds_bytes > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, P.lds_bytes);
        if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "hipFuncSetAttribute(LDS=%d): %s", P.lds_bytes, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3((unsigned)block), P.lds_bytes, (hipStream_t)stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return AP_OK;
}

extern "C" {

int ap_tempogram_max_win(void) { return APTG_WMAX; }

int64_t ap_tempogram_agg_floats(int64_t B, int64_t n, int win_length, int center) {
    const int64_t T = ap_tempogram_frames(n, win_length, center);
    if (B <= 0 || T <= 0 || win_length < 1) return 0;
    return B * ((T + APTG_TT - 1) / APTG_TT) * win_length;
}

int ap_tempogram_fused(int win_length) { return ap_tempogram_wave_shape(win_length) ? 1 : 0; }

// tw != NULL asks for the wave kernel (AP_ERR_UNSUPPORTED when it does not serve win_length), NULL for the general one
int ap_tempogram_f32(const float *env, int64_t B, int64_t n, int64_t row_stride, const float *window, int win_length,
                     int center, int norm, const float *tw, float *out, float *agg, void *stream) {
    ApTempogramParams P;
    int rc = ap_prepare_tempogram(P, env, B, n, row_stride, window, win_length, center, norm, tw, out, agg);
    if (rc != AP_OK) return rc;
    if (tw) return ap_rhythm_launch(ap_tempogram_wave_kernel, ap_tempogram_wave_grid(P), 64 * APTG_WAVES, P, stream, "ap_tempogram_f32");
    return ap_rhythm_launch(ap_tempogram_kernel, ap_tempogram_grid(P), 64 * APTG_WAVES, P, stream, "ap_tempogram_f32");
}

int ap_tempo_pick_f32(const float *g, int64_t B, int64_t n_col, int n_lags, int64_t clip_stride, int64_t lag_stride,
                      int64_t col_stride, int64_t n_red, int64_t red_stride, float div, const float *logprior,
                      int32_t *out_idx, void *stream) {
    ApTempoPickParams P;
    int rc = ap_prepare_tempo_pick(P, g, B, n_col, n_lags, clip_stride, lag_stride, col_stride, n_red, red_stride, div,
                                   logprior, out_idx);
    if (rc != AP_OK) return rc;
    return ap_rhythm_launch(ap_tempo_pick_kernel, ap_tempo_pick_grid(P), APTP_BLOCK, P, stream, "ap_tempo_pick_f32");
}

int ap_beat_track_max_frames(void) { return APBT_TMAX; }
int ap_beat_track_max_period(void) { return APBT_PMAX; }

int ap_beat_track_f32(const float *env, int64_t B, int64_t T, int64_t row_stride, const int32_t *period, float tightness,
                      int trim, unsigned char *out_mask, int32_t *out_count, float *out_L, float *out_C, int32_t *out_link,
                      void *stream) {
    ApBeatParams P;
    int rc = ap_prepare_beat_track(P, env, B, T, row_stride, period, tightness, trim, out_mask, out_count, out_L, out_C, out_link);
    if (rc != AP_OK) return rc;
    return ap_rhythm_launch(ap_beat_track_kernel, ap_beat_track_grid(P), APBT_BLOCK, P, stream, "ap_beat_track_f32");
}

}  // extern "C"
