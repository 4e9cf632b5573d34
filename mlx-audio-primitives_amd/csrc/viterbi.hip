// Translation unit of the sequence decoders (kernels_viterbi.h): ap_viterbi_emission_f32, ap_viterbi_decode_f32,
// ap_viterbi_binary_f32 and their caps.
#include <hip/hip_runtime.h>

#define AP_TU_SECONDARY 1
#include "kernels_viterbi.h"

static int ap_viterbi_launched(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return AP_OK;
}

extern "C" {

int ap_viterbi_max_states(void) { return APV_MAX_STATES; }
int ap_viterbi_max_steps(void) { return APV_MAX_STEPS; }

int ap_viterbi_emission_f32(const float *prob, int64_t B, int64_t S, int64_t T, int64_t row_stride, int mode, const float *lps, float *E,
                            int32_t *flags, void *stream) {
    ApViterbiEmisParams P;
    int rc = ap_prepare_viterbi_emission(P, prob, B, S, T, row_stride, mode, lps, E, flags);
    if (rc != AP_OK) return rc;
    hipError_t e = hipMemsetAsync(flags, 0, (size_t)B * sizeof(int32_t), (hipStream_t)stream);
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_viterbi_emission_f32: hipMemsetAsync: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(ap_viterbi_emission_kernel, dim3((unsigned)ap_viterbi_grid(P.n_items)), dim3(APV_THREADS), P.lds_bytes,
                       (hipStream_t)stream, P);
    return ap_viterbi_launched("ap_viterbi_emission_f32");
}

int ap_viterbi_decode_f32(const float *E, int64_t B, int64_t S, int64_t T, const float *lt, const float *li, uint16_t *ptr,
                          int32_t *states, double *logp, void *stream) {
    // lt in LDS up to AP_VITERBI_LT_LDS states (default and ceiling: APV_LT_LDS_MAX; 0: always from global memory)
    static const int lt_lds_max = std::getenv("AP_VITERBI_LT_LDS") ? std::atoi(std::getenv("AP_VITERBI_LT_LDS")) : APV_LT_LDS_MAX;
    ApViterbiDecParams P;
    int rc = ap_prepare_viterbi_decode(P, E, B, S, T, lt, li, ptr, states, logp, lt_lds_max);
    if (rc != AP_OK) return rc;
    const dim3 grid((unsigned)ap_viterbi_grid(B));
    const dim3 block(APV_THREADS);
    if (P.lt_lds) {
        if (P.lds_bytes > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(ap_viterbi_decode_kernel<true, 1>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, P.lds_bytes);
            if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_viterbi_decode_f32: hipFuncSetAttribute(LDS=%d): %s", P.lds_bytes, hipGetErrorString(e));
        }
        hipLaunchKernelGGL((ap_viterbi_decode_kernel<true, 1>), grid, block, P.lds_bytes, (hipStream_t)stream, P);
    } else if (P.n_pass == 1) hipLaunchKernelGGL((ap_viterbi_decode_kernel<false, 1>), grid, block, P.lds_bytes, (hipStream_t)stream, P);
    else if (P.n_pass == 2) hipLaunchKernelGGL((ap_viterbi_decode_kernel<false, 2>), grid, block, P.lds_bytes, (hipStream_t)stream, P);
    else if (P.n_pass == 3) hipLaunchKernelGGL((ap_viterbi_decode_kernel<false, 3>), grid, block, P.lds_bytes, (hipStream_t)stream, P);
    else hipLaunchKernelGGL((ap_viterbi_decode_kernel<false, 4>), grid, block, P.lds_bytes, (hipStream_t)stream, P);
    return ap_viterbi_launched("ap_viterbi_decode_f32");
}

int ap_viterbi_binary_f32(const float *E, int64_t B, int64_t S, int64_t T, const float *lt, int per_label, const float *li, uint32_t *bits,
                          int32_t *states, double *logp, void *stream) {
    ApViterbiBinParams P;
    int rc = ap_prepare_viterbi_binary(P, E, B, S, T, lt, per_label, li, bits, states, logp);
    if (rc != AP_OK) return rc;
    hipLaunchKernelGGL(ap_viterbi_binary_kernel, dim3((unsigned)ap_viterbi_grid(P.n_items)), dim3(64), P.lds_bytes, (hipStream_t)stream, P);
    return ap_viterbi_launched("ap_viterbi_binary_f32");
}

}  // extern "C"
