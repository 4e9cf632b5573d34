// Translation unit of harmonic / percussive separation (kernels_hpss.h): ap_hpss_f32, ap_hpss_fused.
#include <hip/hip_runtime.h>

#define AP_TU_SECONDARY 1
#include "kernels_hpss.h"

template <class K>
static int ap_hpss_launch(K kern, const ApHpssParams &P, void *stream) {
    if (P.lds_bytes > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, P.lds_bytes);
        if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "hipFuncSetAttribute(LDS=%d): %s", P.lds_bytes, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)ap_hpss_grid(P)), dim3(64 * APHP_WAVES), P.lds_bytes, (hipStream_t)stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_hpss_f32: %s", hipGetErrorString(e));
    return AP_OK;
}

extern "C" {

int ap_hpss_fused(int k_harm, int k_perc) { return ap_hpss_network_sizes(k_harm, k_perc) ? 1 : 0; }

int ap_hpss_f32(const float *S, int is_complex, int64_t B, int64_t F, int64_t T, int64_t row_stride_in, int k_harm,
                int k_perc, float margin_harm, float margin_perc, float power, int mode, int general, float *out_h,
                float *out_p, int64_t row_stride_out, void *stream) {
    ApHpssParams P;
    int rc = ap_prepare_hpss(P, S, is_complex, B, F, T, row_stride_in, k_harm, k_perc, margin_harm, margin_perc, power,
                             mode, general, out_h, out_p, row_stride_out, 0);
    if (rc != AP_OK) return rc;
    if (P.fused) return is_complex ? ap_hpss_launch(ap_hpss_kernel<true, true>, P, stream)
                                   : ap_hpss_launch(ap_hpss_kernel<false, true>, P, stream);
    return is_complex ? ap_hpss_launch(ap_hpss_kernel<true, false>, P, stream)
                      : ap_hpss_launch(ap_hpss_kernel<false, false>, P, stream);
}

}  // extern "C"
