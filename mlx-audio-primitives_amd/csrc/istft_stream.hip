// Translation unit of the streaming ISTFT (kernels_istft_stream.h): ap_istft_stream_f32 and its workspace query.
#include <hip/hip_runtime.h>

#include "kernels_istft_stream.h"

template <int N>
static int ap_launch_istft_stream(const ApIstftStreamParams &P, int64_t B, void *stream) {
    auto kern = ap_istft_stream_kernel<N>;
    if (P.lds_bytes > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, P.lds_bytes);
        if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "hipFuncSetAttribute(LDS=%d): %s", P.lds_bytes, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)(P.tiles_per_clip * B)), dim3(AP_BLOCK), P.lds_bytes, (hipStream_t)stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_istft_stream_f32: %s", hipGetErrorString(e));
    return AP_OK;
}

extern "C" {

int64_t ap_istft_stream_workspace_floats(int64_t B, int64_t T, int n_fft, int hop) {
    (void)hop;
    if (B <= 0 || T <= 0 || n_fft <= 0 || ap_istft_stream_fused(n_fft)) return 0;
    return B * T * (int64_t)n_fft;
}

int ap_istft_stream_f32(const float *S, int64_t B, int64_t T, int64_t row_stride, int n_fft, int hop,
                        const float *window, const float *tw, int64_t frame0, const float *carry_in, float *carry_out,
                        int final_, int64_t lo, int64_t hi, float *frames_ws, float *out, void *stream) {
    ApIstftStreamParams P;
    int rc = ap_prepare_istft_stream(P, S, B, T, row_stride, n_fft, hop, window, tw, frame0, carry_in, carry_out,
                                     final_, lo, hi, out);
    if (rc != AP_OK) return rc;
    if (B == 0 || (T == 0 && n_fft == hop)) return AP_OK;          // nothing to write
    switch (n_fft) {
        case 2048: return ap_launch_istft_stream<2048>(P, B, stream);
        case 1024: return ap_launch_istft_stream<1024>(P, B, stream);
        case 512: return ap_launch_istft_stream<512>(P, B, stream);
        case 400: return ap_launch_istft_stream<400>(P, B, stream);
        case 256: return ap_launch_istft_stream<256>(P, B, stream);
        default: break;
    }
    if (T > 0) {
        if (row_stride != T) AP_FAIL(AP_ERR_UNSUPPORTED, "istft_stream: n_fft=%d needs a dense spectrum (row_stride == T)", n_fft);
        if (!frames_ws) AP_FAIL(AP_ERR_INVALID, "istft_stream: NULL workspace");
        rc = ap_irfft_frames_f32(S, B, T, n_fft, tw, frames_ws, stream);
        if (rc != AP_OK) return rc;
        P.frames = frames_ws;
    }
    hipLaunchKernelGGL(ap_istft_stream_ola_kernel, dim3((unsigned)(P.blocks_per_row * B)), dim3(AP_BLOCK), 0,
                       (hipStream_t)stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_istft_stream_f32(overlap-add): %s", hipGetErrorString(e));
    return AP_OK;
}

}  // extern "C"
