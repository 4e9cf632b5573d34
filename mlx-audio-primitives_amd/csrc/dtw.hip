// Translation unit of dynamic time warping (kernels_dtw.h): ap_dtw_cost_f32, ap_dtw_accumulate_f32, ap_dtw_backtrack_i32
// and their caps.
#include <hip/hip_runtime.h>

#define AP_TU_SECONDARY 1
#include "kernels_dtw.h"

template <class K>
static int ap_dtw_cost_launch(K kern, const ApDtwCostParams &P, void *stream) {
    hipLaunchKernelGGL(kern, dim3((unsigned)ap_dtw_grid(P.n_tiles)), dim3(APDC_THREADS), P.lds_bytes, (hipStream_t)stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_dtw_cost_f32: %s", hipGetErrorString(e));
    return AP_OK;
}

extern "C" {

int ap_dtw_max_features(void) { return APDC_MAX_D; }
int ap_dtw_max_steps(void) { return APDT_MAX_STEPS; }
int ap_dtw_max_step(void) { return APDT_MAX_STEP; }
int ap_dtw_max_len(void) { return APDT_MAX_LEN; }

int ap_dtw_cost_f32(const float *X, const float *Y, int64_t B, int d, int64_t N, int64_t M, int64_t x_row_stride, int64_t y_row_stride,
                    int metric, float *C, int64_t c_row_stride, void *stream) {
    ApDtwCostParams P;
    int rc = ap_prepare_dtw_cost(P, X, Y, B, d, N, M, x_row_stride, y_row_stride, metric, C, c_row_stride);
    if (rc != AP_OK) return rc;
    switch (metric) {
    case 0: return ap_dtw_cost_launch(ap_dtw_cost_kernel<0>, P, stream);
    case 1: return ap_dtw_cost_launch(ap_dtw_cost_kernel<1>, P, stream);
    case 2: return ap_dtw_cost_launch(ap_dtw_cost_kernel<2>, P, stream);
    default: return ap_dtw_cost_launch(ap_dtw_cost_kernel<3>, P, stream);
    }
}

// One launch per tile-anti-diagonal, in order on the caller's stream: a tile reads only what earlier launches wrote.
int ap_dtw_accumulate_f32(const float *C, int64_t B, int64_t N, int64_t M, int64_t c_row_stride, int n_steps, const int32_t *steps_ab,
                          const float *weights_add, const float *weights_mul, int subseq, int use_band, int64_t band_r, float *D,
                          int64_t d_row_stride, uint8_t *steps, int64_t steps_row_stride, void *stream) {
    ApDtwAccParams P;
    int rc = ap_prepare_dtw_accumulate(P, C, B, N, M, c_row_stride, n_steps, steps_ab, weights_add, weights_mul, subseq, use_band, band_r,
                                       D, d_row_stride, steps, steps_row_stride);
    if (rc != AP_OK) return rc;
    for (int64_t dg = 0; dg < P.n_diag; ++dg) {
        const unsigned g = (unsigned)ap_dtw_acc_diagonal(P, dg);
        if (P.fast) hipLaunchKernelGGL(ap_dtw_accumulate_kernel<true>, dim3(g), dim3(64 * APDT_WAVES), P.lds_bytes, (hipStream_t)stream, P);
        else hipLaunchKernelGGL(ap_dtw_accumulate_kernel<false>, dim3(g), dim3(64 * APDT_WAVES), P.lds_bytes, (hipStream_t)stream, P);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_dtw_accumulate_f32: %s", hipGetErrorString(e));
    }
    return AP_OK;
}

int ap_dtw_backtrack_i32(const float *D, const uint8_t *steps, const int32_t *start, int64_t B, int64_t N, int64_t M, int64_t d_row_stride,
                         int64_t steps_row_stride, int n_steps, const int32_t *steps_ab, int subseq, int32_t *path, int32_t *len,
                         void *stream) {
    ApDtwBtParams P;
    int rc = ap_prepare_dtw_backtrack(P, D, steps, start, B, N, M, d_row_stride, steps_row_stride, n_steps, steps_ab, subseq, path, len);
    if (rc != AP_OK) return rc;
    hipLaunchKernelGGL(ap_dtw_backtrack_kernel, dim3((unsigned)ap_dtw_grid(B)), dim3(64), P.lds_bytes, (hipStream_t)stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_dtw_backtrack_i32: %s", hipGetErrorString(e));
    return AP_OK;
}

}  // extern "C"
