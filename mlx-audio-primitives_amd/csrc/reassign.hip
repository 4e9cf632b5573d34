// Translation unit of reassigned_spectrogram (kernels_reassign.h): ap_reassign_f32.
#include <hip/hip_runtime.h>

#define AP_TU_SECONDARY 1
#include "kernels_reassign.h"

template <class K>
static int ap_reassign_launch(K kern, int grid, int block, const ApReassignParams &P, void *stream) {
    if (P.lds_bytes > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, P.lds_bytes);
        if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_reassign_f32: hipFuncSetAttribute(LDS=%d): %s", P.lds_bytes, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3((unsigned)block), P.lds_bytes, (hipStream_t)stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_reassign_f32: %s", hipGetErrorString(e));
    return AP_OK;
}

template <int PADGEN>
static int ap_reassign_wave(const ApReassignParams &P, void *stream) {
    const int grid = ap_reassign_wave_grid(P), block = 64 * APS_WAVES;
    const bool rf = (P.flags & AP_REASSIGN_FREQ) != 0, rt = (P.flags & AP_REASSIGN_TIME) != 0;
    if (rf && rt) return ap_reassign_launch(ap_reassign2048_wave_kernel<PADGEN, true, true>, grid, block, P, stream);
    if (rf) return ap_reassign_launch(ap_reassign2048_wave_kernel<PADGEN, true, false>, grid, block, P, stream);
    return ap_reassign_launch(ap_reassign2048_wave_kernel<PADGEN, false, true>, grid, block, P, stream);
}

extern "C" {

int ap_reassign_f32(const float *y, int64_t B, int64_t L, int n_fft, int hop, const float *win_h, const float *win_dh,
                    const float *win_th, const float *tw, int center, int pad_mode, int64_t T, double sr, double ref_power, int flags,
                    float *freqs, float *times, float *mags, int64_t out_row_stride, void *stream) {
    ApReassignParams P;
    int rc = ap_prepare_reassign(P, y, B, L, n_fft, hop, win_h, win_dh, win_th, tw, center, pad_mode, T, sr, ref_power, flags, freqs,
                                 times, mags, out_row_stride);
    if (rc != AP_OK) return rc;
    if (P.wave) return P.padgen ? ap_reassign_wave<1>(P, stream) : ap_reassign_wave<0>(P, stream);
    return ap_reassign_launch(ap_reassign_tile_kernel, (int)P.n_groups, AP_BLOCK, P, stream);
}

}  // extern "C"
