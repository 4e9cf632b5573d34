// Translation unit of the fused NNLS kernel (kernels_nnls.h): ap_nnls_max_bins, ap_nnls_max_rows, ap_nnls_fista_f32.
// (ap_nnls_plan_words / ap_nnls_plan_host are host builders: host_builders.cpp.)
#include <hip/hip_runtime.h>

#define AP_TU_SECONDARY 1
#include "kernels_nnls.h"

extern "C" {

int ap_nnls_max_bins(void) { return AP_NNLS_MAX_BINS; }
int ap_nnls_max_rows(void) { return AP_NNLS_MAX_ROWS; }

int ap_nnls_fista_f32(const float *s, int64_t B, int M, int F, int64_t T, int64_t row_stride, const int32_t *A_plan, const float *P,
                      float step, const float *momentum, int n_iter, float power, float *out, int64_t out_row_stride, void *stream) {
    ApNnlsParams p;
    int64_t grid = 0;
    int rc = ap_prepare_nnls(p, s, B, M, F, T, row_stride, A_plan, P, step, momentum, n_iter, power, out, out_row_stride, &grid);
    if (rc != AP_OK) return rc;
    const int lds = ap_nnls_lds_bytes(M, F);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(ap_nnls_fista_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_nnls_fista_f32: hipFuncSetAttribute(LDS=%d): %s", lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(ap_nnls_fista_kernel, dim3((unsigned)grid), dim3(APQ_THREADS), lds, (hipStream_t)stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_nnls_fista_f32: %s", hipGetErrorString(e));
    return AP_OK;
}

}  // extern "C"
