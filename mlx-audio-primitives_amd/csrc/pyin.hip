// Translation unit of probabilistic YIN (kernels_pyin.h): ap_pyin_observe_f32, ap_pyin_decode_f32 and their caps.
#include <hip/hip_runtime.h>

#define AP_TU_SECONDARY 1
#include "kernels_pyin.h"

template <class K, class PP>
static int ap_pyin_launch(K kern, int grid, int block, const PP &P, void *stream, const char *what) {
    if (P.lds_bytes > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, P.lds_bytes);
        if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "%s: hipFuncSetAttribute(LDS=%d): %s", what, P.lds_bytes, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3((unsigned)block), P.lds_bytes, (hipStream_t)stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return AP_OK;
}

extern "C" {

int ap_pyin_max_bins(void) { return APP_MAX_BINS; }
int ap_pyin_max_width(void) { return 2 * APP_MAX_HALF + 1; }

int ap_pyin_observe_f32(const float *d, int64_t B, int n_lags, int64_t T, int lo, double sr, double fmin, int bins_per_semitone, int n_bins,
                        const float *thr, const float *beta, int n_thresholds, const float *ea, const float *nz, int n_tab,
                        float no_trough_prob, float *E, float *voiced_prob, void *stream) {
    ApPyinObsParams P;
    int rc = ap_prepare_pyin_observe(P, d, B, n_lags, T, lo, sr, fmin, bins_per_semitone, n_bins, thr, beta, n_thresholds, ea, nz, n_tab,
                                     no_trough_prob, E, voiced_prob);
    if (rc != AP_OK) return rc;
    return ap_pyin_launch(ap_pyin_observe_kernel, ap_pyin_grid(P.n_items, 0), APP_OBS_THREADS, P, stream, "ap_pyin_observe_f32");
}

int ap_pyin_decode_f32(const float *E, int64_t B, int n_bins, int64_t T, const float *lw, int half_width, const float *lz, const float *ls,
                       float li, const float *freq, int use_fill, float fill, uint16_t *ptr, int32_t *states, float *f0, uint8_t *voiced,
                       double *logp, int max_blocks, void *stream) {
    ApPyinDecParams P;
    int rc = ap_prepare_pyin_decode(P, E, B, n_bins, T, lw, half_width, lz, ls, li, freq, use_fill, fill, ptr, states, f0, voiced, logp);
    if (rc != AP_OK) return rc;
    return ap_pyin_launch(ap_pyin_decode_kernel, ap_pyin_grid(B, max_blocks), P.threads, P, stream, "ap_pyin_decode_f32");
}

}  // extern "C"
