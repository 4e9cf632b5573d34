// Translation unit of the recurrence / cross-similarity kernels (kernels_segment.h): ap_segment_threshold_f32,
// ap_segment_bandwidth_f32, ap_segment_write_f32, ap_segment_lag and ap_segment_max_len.
#include <hip/hip_runtime.h>

#define AP_TU_SECONDARY 1
#include "kernels_segment.h"

template <class K, class PP>
static int ap_segment_launch(K kern, int64_t items, const PP &P, void *stream, const char *what) {
    if (P.lds_bytes > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, P.lds_bytes);
        if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "hipFuncSetAttribute(LDS=%d): %s", P.lds_bytes, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)ap_segment_grid(items)), dim3(APSG_THREADS), P.lds_bytes, (hipStream_t)stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return AP_OK;
}

template <int METRIC>
static int ap_segment_write_mode(const ApSegWriteParams &P, void *stream) {
    const char *what = "ap_segment_write_f32";
    switch (P.mode) {
    case 0: return ap_segment_launch(ap_segment_write_kernel<METRIC, 0>, P.n_tiles, P, stream, what);
    case 1: return ap_segment_launch(ap_segment_write_kernel<METRIC, 1>, P.n_tiles, P, stream, what);
    default: return ap_segment_launch(ap_segment_write_kernel<METRIC, 2>, P.n_tiles, P, stream, what);
    }
}

extern "C" {

int ap_segment_max_len(void) { return APSG_MAX_LEN; }

int ap_segment_threshold_f32(const float *ref, const float *data, int64_t B, int d, int64_t n_ref, int64_t n, int64_t ref_row_stride,
                             int64_t data_row_stride, int metric, int64_t k, int64_t width, uint32_t *records, void *stream) {
    ApSegThrParams P;
    int rc = ap_prepare_segment_threshold(P, ref, data, B, d, n_ref, n, ref_row_stride, data_row_stride, metric, k, width, records);
    if (rc != AP_OK) return rc;
    const char *what = "ap_segment_threshold_f32";
    switch (metric) {
    case 0: return ap_segment_launch(ap_segment_threshold_kernel<0>, P.n_items, P, stream, what);
    case 1: return ap_segment_launch(ap_segment_threshold_kernel<1>, P.n_items, P, stream, what);
    case 2: return ap_segment_launch(ap_segment_threshold_kernel<2>, P.n_items, P, stream, what);
    default: return ap_segment_launch(ap_segment_threshold_kernel<3>, P.n_items, P, stream, what);
    }
}

int ap_segment_bandwidth_f32(const uint32_t *records, int64_t B, int64_t n, int kind, float *bw, void *stream) {
    ApSegBwParams P;
    int rc = ap_prepare_segment_bandwidth(P, records, B, n, kind, bw);
    if (rc != AP_OK) return rc;
    return ap_segment_launch(ap_segment_bandwidth_kernel, B, P, stream, "ap_segment_bandwidth_f32");
}

int ap_segment_write_f32(const float *ref, const float *data, int64_t B, int d, int64_t n_ref, int64_t n, int64_t ref_row_stride,
                         int64_t data_row_stride, int metric, int mode, int64_t width, int full, int sym, int self_diag,
                         const uint32_t *records, const float *bw, double bandwidth, void *out, int64_t out_row_stride, void *stream) {
    ApSegWriteParams P;
    int rc = ap_prepare_segment_write(P, ref, data, B, d, n_ref, n, ref_row_stride, data_row_stride, metric, mode, width, full, sym, self_diag,
                                      records, bw, bandwidth, out, out_row_stride);
    if (rc != AP_OK) return rc;
    switch (metric) {
    case 0: return ap_segment_write_mode<0>(P, stream);
    case 1: return ap_segment_write_mode<1>(P, stream);
    case 2: return ap_segment_write_mode<2>(P, stream);
    default: return ap_segment_write_mode<3>(P, stream);
    }
}

int ap_segment_lag(const void *in, int64_t B, int64_t n, int64_t t_lag, int elem_bytes, int to_lag, int64_t in_row_stride, void *out,
                   int64_t out_row_stride, void *stream) {
    ApSegLagParams P;
    int rc = ap_prepare_segment_lag(P, in, B, n, t_lag, elem_bytes, to_lag, in_row_stride, out, out_row_stride);
    if (rc != AP_OK) return rc;
    if (elem_bytes == 1) return ap_segment_launch(ap_segment_lag_kernel<uint8_t>, P.n_tiles, P, stream, "ap_segment_lag");
    return ap_segment_launch(ap_segment_lag_kernel<uint32_t>, P.n_tiles, P, stream, "ap_segment_lag");
}

}  // extern "C"
