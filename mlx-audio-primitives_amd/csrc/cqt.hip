// Translation unit of the constant-Q transform (kernels_cqt.h): ap_cqt_f32, ap_cqt_max_taps.
#include <hip/hip_runtime.h>

#define AP_TU_SECONDARY 1
#include "kernels_cqt.h"

extern "C" {

int ap_cqt_max_taps(void) { return APCQ_MAX_TAPS; }

int ap_cqt_f32(const float *y, int64_t B, int64_t L, int hop, int pad_mode, const float *taps, const int64_t *tap_offset,
               const int32_t *m0, const float *scale, int n_bins, int64_t T, float *out, int64_t out_row_stride, void *stream) {
    ApCqtParams P;
    int rc = ap_prepare_cqt(P, y, B, L, hop, pad_mode, taps, tap_offset, m0, scale, n_bins, T, out, out_row_stride);
    if (rc != AP_OK) return rc;
    static_assert(APCQ_LDS_BYTES > 48 * 1024 && APCQ_LDS_BYTES <= AP_LDS_MAX, "the opt-in below");
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(ap_cqt_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, P.lds_bytes);
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "hipFuncSetAttribute(LDS=%d): %s", P.lds_bytes, hipGetErrorString(e));
    hipLaunchKernelGGL(ap_cqt_kernel, dim3((unsigned)ap_cqt_grid(P)), dim3(64 * APCQ_WAVES), P.lds_bytes, (hipStream_t)stream, P);
    e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_cqt_f32: %s", hipGetErrorString(e));
    return AP_OK;
}

}  // extern "C"
