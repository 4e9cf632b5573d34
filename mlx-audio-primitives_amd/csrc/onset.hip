// Translation unit of onset strength and peak picking (kernels_onset.h): ap_onset_strength_f32, ap_peak_pick_f32.
#include <hip/hip_runtime.h>

#define AP_TU_SECONDARY 1
#include "kernels_onset.h"

template <class K, class PP>
static int ap_onset_launch(K kern, int grid, int block, const PP &P, void *stream, const char *what) {
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

int ap_onset_strength_f32(const float *S, int64_t B, int64_t M, int64_t T, int64_t row_stride, const float *ref,
                          int64_t ref_row_stride, int lag, int max_size, int shift, int db_mode, float db_coef,
                          float db_amin, float db_ref, float db_top_db, const uint32_t *smax_key, float *out,
                          int64_t out_row_stride, void *stream) {
    ApOnsetParams P;
    int rc = ap_prepare_onset_strength(P, S, B, M, T, row_stride, ref, ref_row_stride, lag, max_size, shift, db_mode, db_coef,
                                       db_amin, db_ref, db_top_db, smax_key, out, out_row_stride);
    if (rc != AP_OK) return rc;
    if (P.db) return ap_onset_launch(ap_onset_strength_kernel<true>, ap_onset_grid(P), 64 * APON_WAVES, P, stream, "ap_onset_strength_f32");
    return ap_onset_launch(ap_onset_strength_kernel<false>, ap_onset_grid(P), 64 * APON_WAVES, P, stream, "ap_onset_strength_f32");
}

int ap_peak_pick_max_frames(void) { return APPK_TMAX; }

int ap_peak_pick_f32(const float *x, int64_t B, int64_t T, int64_t row_stride, int pre_max, int post_max, int pre_avg,
                     int post_avg, float delta, int wait, int normalize, int guard, int backtrack, const float *energy,
                     int64_t energy_row_stride, unsigned char *out_mask, int32_t *out_count, void *stream) {
    ApPeakPickParams P;
    int rc = ap_prepare_peak_pick(P, x, B, T, row_stride, pre_max, post_max, pre_avg, post_avg, delta, wait, normalize, guard,
                                  backtrack, energy, energy_row_stride, out_mask, out_count);
    if (rc != AP_OK) return rc;
    return ap_onset_launch(ap_peak_pick_kernel, ap_peak_pick_grid(P), APPK_BLOCK, P, stream, "ap_peak_pick_f32");
}

}  // extern "C"
