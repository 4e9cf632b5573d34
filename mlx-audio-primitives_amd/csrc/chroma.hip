// Translation unit of the chroma features (kernels_chroma.h): ap_chroma_fold_f32, ap_chroma_cens_f32 and their caps.
#include <hip/hip_runtime.h>

#define AP_TU_SECONDARY 1
#include "kernels_chroma.h"

template <class K>
static int ap_chroma_fold_launch(K kern, const ApChromaFoldParams &P, void *stream) {
    hipLaunchKernelGGL(kern, dim3((unsigned)ap_chroma_grid(P.n_tiles)), dim3(64 * APCH_WAVES), P.lds_bytes, (hipStream_t)stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_chroma_fold_f32: %s", hipGetErrorString(e));
    return AP_OK;
}

template <int NACC>
static int ap_chroma_fold_kind(const ApChromaFoldParams &P, void *stream) {
    if (P.in_kind == 0) return ap_chroma_fold_launch(ap_chroma_fold_kernel<NACC, 0>, P, stream);
    if (P.in_kind == 1) return ap_chroma_fold_launch(ap_chroma_fold_kernel<NACC, 1>, P, stream);
    return ap_chroma_fold_launch(ap_chroma_fold_kernel<NACC, 2>, P, stream);
}

extern "C" {

int ap_chroma_max_out(void) { return APCH_MAX_OUT; }
int ap_chroma_max_smooth(void) { return APCN_MAX_SMOOTH; }

int ap_chroma_fold_f32(const float *x, int in_kind, int64_t B, int K, int64_t T, int64_t in_row_stride, const float *w, int n_out,
                       int pre_l1, int use_threshold, float threshold, int norm, float *out, int64_t out_row_stride, void *stream) {
    ApChromaFoldParams P;
    int rc = ap_prepare_chroma_fold(P, x, in_kind, B, K, T, in_row_stride, w, n_out, pre_l1, use_threshold, threshold, norm, out,
                                    out_row_stride);
    if (rc != AP_OK) return rc;
    switch (P.nacc) {
    case 6: return ap_chroma_fold_kind<6>(P, stream);
    case 12: return ap_chroma_fold_kind<12>(P, stream);
    case 24: return ap_chroma_fold_kind<24>(P, stream);
    case 36: return ap_chroma_fold_kind<36>(P, stream);
    default: return ap_chroma_fold_kind<48>(P, stream);
    }
}

int ap_chroma_cens_f32(const float *chroma, int64_t B, int n, int64_t T, int64_t in_row_stride, const float *taps, int n_taps,
                       int norm, float *out, int64_t out_row_stride, void *stream) {
    ApChromaCensParams P;
    int rc = ap_prepare_chroma_cens(P, chroma, B, n, T, in_row_stride, taps, n_taps, norm, out, out_row_stride);
    if (rc != AP_OK) return rc;
    hipLaunchKernelGGL(ap_chroma_cens_kernel, dim3((unsigned)ap_chroma_grid(P.n_tiles)), dim3(APCN_THREADS), P.lds_bytes,
                       (hipStream_t)stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_chroma_cens_f32: %s", hipGetErrorString(e));
    return AP_OK;
}

}  // extern "C"
