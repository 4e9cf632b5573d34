// Translation unit of per-channel energy normalisation (kernels_pcen.h): ap_pcen_f32.
#include <hip/hip_runtime.h>

#define AP_TU_SECONDARY 1
#include "kernels_pcen.h"

template <class K>
static int ap_pcen_launch(K kern, const ApPcenParams &P, void *stream) {
    hipLaunchKernelGGL(kern, dim3((unsigned)ap_pcen_grid(P)), dim3(64 * APPC_WAVES), 0, (hipStream_t)stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_pcen_f32: %s", hipGetErrorString(e));
    return AP_OK;
}

extern "C" {

int ap_pcen_f32(const float *S, int64_t B, int64_t M, int64_t T, int64_t row_stride, const float *ref, int64_t ref_row_stride,
                int max_size, double b, float gain, float bias, float power, float eps, const float *zi, float *out,
                int64_t out_row_stride, float *zf, void *stream) {
    ApPcenParams P;
    int rc = ap_prepare_pcen(P, S, B, M, T, row_stride, ref, ref_row_stride, max_size, b, gain, bias, power, eps, zi, out,
                             out_row_stride, zf);
    if (rc != AP_OK) return rc;
    if (P.chain == APPC_LOG) return ap_pcen_launch(ap_pcen_kernel<APPC_LOG>, P, stream);
    if (P.chain == APPC_POWER) return ap_pcen_launch(ap_pcen_kernel<APPC_POWER>, P, stream);
    return ap_pcen_launch(ap_pcen_kernel<APPC_GENERAL>, P, stream);
}

}  // extern "C"
