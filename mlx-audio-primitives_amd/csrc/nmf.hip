// Translation unit of the NMF kernels (kernels_nmf.h): ap_nmf_workspace_bytes, ap_nmf_mu_f32, ap_nmf_objective_f32,
// ap_nmf_max_components.
#include <hip/hip_runtime.h>

#define AP_TU_SECONDARY 1
#include "kernels_nmf.h"

namespace {
struct ApNmfGo {
    hipStream_t stream;
    int operator()(ApNmfKernel kern, int grid, int lds, const ApNmfParams &P) const {
        if (lds > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "nmf: hipFuncSetAttribute(LDS=%d): %s", lds, hipGetErrorString(e));
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(APN_THREADS), lds, stream, P);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "nmf: %s", hipGetErrorString(e));
        return AP_OK;
    }
};
}  // namespace

extern "C" {

int ap_nmf_max_components(void) { return APN_MAX_K; }

int64_t ap_nmf_workspace_bytes(int64_t B, int64_t F, int64_t T, int K, int beta_loss) {
    (void)F; (void)beta_loss;
    if (B <= 0 || T <= 0 || K < 1 || K > APN_MAX_K) return 0;
    return ap_nmf_ws_bytes(B, T, K);
}

int ap_nmf_mu_f32(const float *V, int64_t B, int64_t F, int64_t T, int64_t row_stride, int K, float *W, float *H, int n_iter,
                  int beta_loss, int update_w, float eps, void *workspace, void *stream) {
    ApNmfParams P;
    int rc = ap_prepare_nmf(P, V, B, F, T, row_stride, K, W, H, beta_loss, eps, workspace);
    if (rc != AP_OK) return rc;
    if (n_iter < 0) AP_FAIL(AP_ERR_INVALID, "nmf: n_iter must be >= 0, got %d", n_iter);
    ApNmfGo go{(hipStream_t)stream};
    return apn_iterate(go, P, n_iter, beta_loss, update_w);
}

int ap_nmf_objective_f32(const float *V, int64_t B, int64_t F, int64_t T, int64_t row_stride, int K, const float *W, const float *H,
                         int beta_loss, float eps, double *out_f64, void *workspace, void *stream) {
    ApNmfParams P;
    int rc = ap_prepare_nmf(P, V, B, F, T, row_stride, K, const_cast<float *>(W), const_cast<float *>(H), beta_loss, eps, workspace);
    if (rc != AP_OK) return rc;
    ApNmfGo go{(hipStream_t)stream};
    return apn_objective(go, P, beta_loss, out_f64);
}

}  // extern "C"
