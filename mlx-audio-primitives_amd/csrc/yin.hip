// Translation unit of the YIN f0 tracker (kernels_yin.h): ap_yin_f32, ap_yin_cmnd_f32, ap_yin_fused.
#include <hip/hip_runtime.h>

#define AP_TU_SECONDARY 1
#include "kernels_yin.h"

template <class K>
static int ap_yin_launch(K kern, int grid, int block, const ApYinParams &P, void *stream, const char *what) {
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

// tw != NULL asks for the wave kernel (AP_ERR_UNSUPPORTED when it does not serve the shape), NULL for the general one
template <bool CURVE>
static int ap_yin_dispatch(const ApYinParams &P, const float *tw, void *stream, const char *what) {
    if (tw) {
        if (!ap_yin_wave_shape(P.n, P.hop, P.L))
            AP_FAIL(AP_ERR_UNSUPPORTED, "%s: the wave kernel serves frame_length 2048 / 1024 with an even hop_length", what);
        if (P.n == 2048) return ap_yin_launch(ap_yin_wave_kernel<2048, CURVE>, ap_yin_wave_grid(P), 64 * APY_WAVES, P, stream, what);
        return ap_yin_launch(ap_yin_wave_kernel<1024, CURVE>, ap_yin_wave_grid(P), 64 * APY_WAVES, P, stream, what);
    }
    return ap_yin_launch(ap_yin_general_kernel<CURVE>, ap_yin_general_grid(P), AP_BLOCK, P, stream, what);
}

extern "C" {

int ap_yin_fused(int frame_length, int hop, int64_t L) { return ap_yin_wave_shape(frame_length, hop, L) ? 1 : 0; }

int ap_yin_f32(const float *y, int64_t B, int64_t L, int frame_length, int hop, int center, int lo, int hi, float sr,
               float trough_threshold, const float *tw, float *f0, float *aper, void *stream) {
    ApYinParams P;
    if (!f0) AP_FAIL(AP_ERR_INVALID, "yin: NULL buffer");
    int rc = ap_prepare_yin(P, y, B, L, frame_length, hop, center, lo, hi, sr, trough_threshold, tw, f0, aper, nullptr);
    if (rc != AP_OK) return rc;
    return ap_yin_dispatch<false>(P, tw, stream, "ap_yin_f32");
}

int ap_yin_cmnd_f32(const float *y, int64_t B, int64_t L, int frame_length, int hop, int center, int lo, int hi,
                    const float *tw, float *out, void *stream) {
    ApYinParams P;
    if (!out) AP_FAIL(AP_ERR_INVALID, "yin_cmnd: NULL buffer");
    int rc = ap_prepare_yin(P, y, B, L, frame_length, hop, center, lo, hi, 1.0f, 0.0f, tw, nullptr, nullptr, out);
    if (rc != AP_OK) return rc;
    return ap_yin_dispatch<true>(P, tw, stream, "ap_yin_cmnd_f32");
}

}  // extern "C"
