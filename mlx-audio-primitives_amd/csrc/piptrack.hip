// Translation unit of piptrack / estimate_tuning / pitch_tuning (kernels_piptrack.h): ap_piptrack_f32,
// ap_piptrack_records_f32, ap_piptrack_tuning_f32, ap_pitch_hist_f32 and their caps.
#include <hip/hip_runtime.h>

#define AP_TU_SECONDARY 1
#include "kernels_piptrack.h"

template <class K>
static int ap_piptrack_launch(K kern, const ApPiptrackParams &P, void *stream, const char *who) {
    hipLaunchKernelGGL(kern, dim3((unsigned)ap_piptrack_grid(P.n_tiles)), dim3(64 * APPT_WAVES), P.lds_bytes, (hipStream_t)stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return AP_OK;
}

extern "C" {

int ap_piptrack_max_bins(void) { return APPT_MAX_BINS; }
int ap_piptrack_max_records(void) { return (int)APPT_MAX_RECORDS; }

int ap_piptrack_f32(const float *S, int in_kind, int64_t B, int F, int64_t T, int64_t in_row_stride, int k_lo, int k_hi,
                    float threshold, int ref_mode, float ref_value, const float *ref, float bin_hz, float *pitches,
                    float *magnitudes, int64_t out_row_stride, void *stream) {
    ApPiptrackParams P;
    int rc = ap_prepare_piptrack(P, S, in_kind, B, F, T, in_row_stride, k_lo, k_hi, threshold, ref_mode, ref_value, ref, bin_hz, 0,
                                 pitches, magnitudes, out_row_stride, 0, nullptr, 0, nullptr);
    if (rc != AP_OK) return rc;
    if (P.kind == 0) return ap_piptrack_launch(ap_piptrack_kernel<0, false>, P, stream, "ap_piptrack_f32");
    return ap_piptrack_launch(ap_piptrack_kernel<1, false>, P, stream, "ap_piptrack_f32");
}

int ap_piptrack_records_f32(const float *S, int in_kind, int64_t B, int F, int64_t T, int64_t in_row_stride, int k_lo, int k_hi,
                            float threshold, int ref_mode, float ref_value, const float *ref, float bin_hz, int per_clip,
                            float *records, int64_t capacity, uint64_t *counters, void *stream) {
    ApPiptrackParams P;
    int rc = ap_prepare_piptrack(P, S, in_kind, B, F, T, in_row_stride, k_lo, k_hi, threshold, ref_mode, ref_value, ref, bin_hz, 1,
                                 nullptr, nullptr, 0, per_clip, records, capacity, (ap_u64 *)counters);
    if (rc != AP_OK) return rc;
    hipError_t e = hipMemsetAsync(counters, 0, (size_t)(per_clip ? B : 1) * sizeof(uint64_t), (hipStream_t)stream);
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_piptrack_records_f32: %s", hipGetErrorString(e));
    if (P.kind == 0) return ap_piptrack_launch(ap_piptrack_kernel<0, true>, P, stream, "ap_piptrack_records_f32");
    return ap_piptrack_launch(ap_piptrack_kernel<1, true>, P, stream, "ap_piptrack_records_f32");
}

int ap_piptrack_tuning_f32(const float *records, const uint64_t *counters, int64_t G, int64_t capacity, double bins_per_octave,
                           const double *edges, int n_bins, float *threshold_out, uint64_t *counts, void *stream) {
    ApTuningParams Q;
    int rc = ap_prepare_piptrack_tuning(Q, records, (const ap_u64 *)counters, G, capacity, bins_per_octave, edges, n_bins,
                                        threshold_out, (ap_u64 *)counts);
    if (rc != AP_OK) return rc;
    hipLaunchKernelGGL(ap_piptrack_tuning_kernel, dim3((unsigned)G), dim3(APPT_SEL_THREADS), Q.lds_bytes, (hipStream_t)stream, Q);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_piptrack_tuning_f32: %s", hipGetErrorString(e));
    return AP_OK;
}

int ap_pitch_hist_f32(const float *frequencies, int64_t n, double bins_per_octave, const double *edges, int n_bins, uint64_t *counts,
                      void *stream) {
    ApPitchHistParams H;
    int rc = ap_prepare_pitch_hist(H, frequencies, n, bins_per_octave, edges, n_bins, (ap_u64 *)counts);
    if (rc != AP_OK) return rc;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_bins * sizeof(uint64_t), (hipStream_t)stream);
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_pitch_hist_f32: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(ap_pitch_hist_kernel, dim3((unsigned)ap_pitch_hist_grid(n)), dim3(APPT_HIST_THREADS), H.lds_bytes,
                       (hipStream_t)stream, H);
    e = hipGetLastError();
    if (e != hipSuccess) AP_FAIL(AP_ERR_HIP, "ap_pitch_hist_f32: %s", hipGetErrorString(e));
    return AP_OK;
}

}  // extern "C"
