// Translation unit of the phase vocoder (kernels_pv.h): ap_phase_vocoder_frames, ap_phase_vocoder_f32.
#include <hip/hip_runtime.h>

#define AP_TU_SECONDARY 1
#include "kernels_pv.h"

template <int W>
static int ap_pv_launch(const ApPvParams &P, void *stream) {
    hipLaunchKernelGGL(ap_pv_kernel<W>, dim3((unsigned)ap_pv_grid(P)), dim3(64 * (W == 1 ? APPV_WAVES : W)), 0, (hipStream_t)stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_phase_vocoder_f32: %s", hipGetErrorString(e));
    return AP_OK;
}

extern "C" {

int64_t ap_phase_vocoder_frames(int64_t T, double rate) { return ap_pv_frames(T, rate); }

int ap_phase_vocoder_waves(int64_t rows, int64_t T_out) { return rows > 0 && T_out > 0 ? ap_pv_waves(rows, T_out) : 1; }

int ap_phase_vocoder_f32(const float *D, int64_t rows, int64_t T, int64_t row_stride, double rate, int64_t T_out, float *out,
                         int64_t out_row_stride, void *stream) {
    ApPvParams P;
    int rc = ap_prepare_pv(P, D, rows, T, row_stride, rate, T_out, out, out_row_stride);
    if (rc != AP_OK) return rc;
    if (P.W == 16) return ap_pv_launch<16>(P, stream);
    if (P.W == 4) return ap_pv_launch<4>(P, stream);
    return ap_pv_launch<1>(P, stream);
}

}  // extern "C"
