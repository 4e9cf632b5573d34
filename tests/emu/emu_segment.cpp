// TEST INFRASTRUCTURE ONLY.  The recurrence / cross-similarity kernels (kernels_segment.h) built for the CPU through
// emu_shim.h, behind emu_ twins of ap_segment_threshold_f32 / ap_segment_bandwidth_f32 / ap_segment_write_f32 /
// ap_segment_lag that take HOST pointers.  Same validation and geometry (ap_prepare_segment_*), same kernel bodies;
// `grid` > 0 overrides the number of workgroups (queries and tiles are then walked in a grid-stride loop).
#include "emu_shim.h"

alignas(16) char ap_smem[160 * 1024];

// the integer LDS atomic of the histograms (the emulated threads are OS threads)
inline unsigned atomicAdd(unsigned *p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }

#include "../../mlx-audio-primitives_amd/csrc/kernels_segment.h"

static thread_local char g_err[512] = "";
char *ap_error_buffer() { return g_err; }
void ap_set_error(const char *msg) { std::snprintf(g_err, sizeof(g_err), "%s", msg); }

// {threads, tile rows, tile columns, features per chunk, cap on d, cap on n; last call: grid, lds_bytes}
static int g_geom[8] = {APSG_THREADS, APSG_TI, APSG_TJ, APSG_KC, APSG_MAX_D, APSG_MAX_LEN, 0, 0};

template <class F>
static void launch(int64_t items, int grid, int lds_bytes, F &&body) {
    const unsigned g = (unsigned)(grid > 0 ? grid : ap_segment_grid(items));
    g_geom[6] = (int)g; g_geom[7] = lds_bytes;
    emu_lds_limit(lds_bytes);
    emu_launch(g, APSG_THREADS, body);
}

template <int METRIC>
static void write_mode(const ApSegWriteParams &P, int grid) {
    switch (P.mode) {
    case 0: launch(P.n_tiles, grid, P.lds_bytes, [&] { ap_segment_write_kernel<METRIC, 0>(P); }); break;
    case 1: launch(P.n_tiles, grid, P.lds_bytes, [&] { ap_segment_write_kernel<METRIC, 1>(P); }); break;
    default: launch(P.n_tiles, grid, P.lds_bytes, [&] { ap_segment_write_kernel<METRIC, 2>(P); }); break;
    }
}

extern "C" {

const char *emu_segment_last_error() { return g_err; }
const int *emu_segment_geometry() { return g_geom; }
int emu_segment_lds_overruns() { return emu_lds_overruns; }

int emu_segment_threshold_f32(const float *ref, const float *data, int64_t B, int d, int64_t n_ref, int64_t n, int64_t ref_row_stride,
                              int64_t data_row_stride, int metric, int64_t k, int64_t width, uint32_t *records, int grid) {
    ApSegThrParams P;
    int rc = ap_prepare_segment_threshold(P, ref, data, B, d, n_ref, n, ref_row_stride, data_row_stride, metric, k, width, records);
    if (rc != AP_OK) return rc;
    switch (metric) {
    case 0: launch(P.n_items, grid, P.lds_bytes, [&] { ap_segment_threshold_kernel<0>(P); }); break;
    case 1: launch(P.n_items, grid, P.lds_bytes, [&] { ap_segment_threshold_kernel<1>(P); }); break;
    case 2: launch(P.n_items, grid, P.lds_bytes, [&] { ap_segment_threshold_kernel<2>(P); }); break;
    default: launch(P.n_items, grid, P.lds_bytes, [&] { ap_segment_threshold_kernel<3>(P); }); break;
    }
    return AP_OK;
}

int emu_segment_bandwidth_f32(const uint32_t *records, int64_t B, int64_t n, int kind, float *bw, int grid) {
    ApSegBwParams P;
    int rc = ap_prepare_segment_bandwidth(P, records, B, n, kind, bw);
    if (rc != AP_OK) return rc;
    launch(B, grid, P.lds_bytes, [&] { ap_segment_bandwidth_kernel(P); });
    return AP_OK;
}

int emu_segment_write_f32(const float *ref, const float *data, int64_t B, int d, int64_t n_ref, int64_t n, int64_t ref_row_stride,
                          int64_t data_row_stride, int metric, int mode, int64_t width, int full, int sym, int self_diag,
                          const uint32_t *records, const float *bw, double bandwidth, void *out, int64_t out_row_stride, int grid) {
    ApSegWriteParams P;
    int rc = ap_prepare_segment_write(P, ref, data, B, d, n_ref, n, ref_row_stride, data_row_stride, metric, mode, width, full, sym, self_diag,
                                      records, bw, bandwidth, out, out_row_stride);
    if (rc != AP_OK) return rc;
    switch (metric) {
    case 0: write_mode<0>(P, grid); break;
    case 1: write_mode<1>(P, grid); break;
    case 2: write_mode<2>(P, grid); break;
    default: write_mode<3>(P, grid); break;
    }
    return AP_OK;
}

int emu_segment_lag(const void *in, int64_t B, int64_t n, int64_t t_lag, int elem_bytes, int to_lag, int64_t in_row_stride, void *out,
                    int64_t out_row_stride, int grid) {
    ApSegLagParams P;
    int rc = ap_prepare_segment_lag(P, in, B, n, t_lag, elem_bytes, to_lag, in_row_stride, out, out_row_stride);
    if (rc != AP_OK) return rc;
    if (elem_bytes == 1) launch(P.n_tiles, grid, P.lds_bytes, [&] { ap_segment_lag_kernel<uint8_t>(P); });
    else launch(P.n_tiles, grid, P.lds_bytes, [&] { ap_segment_lag_kernel<uint32_t>(P); });
    return AP_OK;
}

}  // extern "C"
