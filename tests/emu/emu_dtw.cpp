// TEST INFRASTRUCTURE ONLY.  The DTW kernels (kernels_dtw.h) built for the CPU through emu_shim.h, behind emu_ twins of
// ap_dtw_cost_f32 / ap_dtw_accumulate_f32 / ap_dtw_backtrack_i32 that take HOST pointers.  Same validation and geometry
// (ap_prepare_dtw_*), same kernel bodies, the same host loop over the tile-anti-diagonals; `grid` > 0 overrides the
// number of workgroups of every launch (the work items are then walked in a grid-stride loop).
#include "emu_shim.h"

alignas(16) char ap_smem[160 * 1024];

#include "../../mlx-audio-primitives_amd/csrc/kernels_dtw.h"

static thread_local char g_err[512] = "";
char *ap_error_buffer() { return g_err; }
void ap_set_error(const char *msg) { std::snprintf(g_err, sizeof(g_err), "%s", msg); }

extern "C" {

const char *emu_dtw_last_error() { return g_err; }

// {accumulate: tile width, tile height, waves per workgroup, halo rows, halo columns, cap on n_steps, cap on a component,
//  cap on N and M; cost: tile rows, tile columns, features per chunk, cap on d; backtrack: window;
//  last call: launches, largest grid, lds_bytes, fast path}
static int g_geom[17] = {APDT_TW, APDT_TH, APDT_WAVES, APDT_HA, APDT_HB, APDT_MAX_STEPS, APDT_MAX_STEP, APDT_MAX_LEN,
                         APDC_TI, APDC_TJ, APDC_KC, APDC_MAX_D, APBT_W, 0, 0, 0, 0};
const int *emu_dtw_geometry() { return g_geom; }
int emu_dtw_lds_overruns() { return emu_lds_overruns; }

int emu_dtw_cost_f32(const float *X, const float *Y, int64_t B, int d, int64_t N, int64_t M, int64_t x_row_stride, int64_t y_row_stride,
                     int metric, float *C, int64_t c_row_stride, int grid) {
    ApDtwCostParams P;
    int rc = ap_prepare_dtw_cost(P, X, Y, B, d, N, M, x_row_stride, y_row_stride, metric, C, c_row_stride);
    if (rc != AP_OK) return rc;
    const unsigned g = (unsigned)(grid > 0 ? grid : ap_dtw_grid(P.n_tiles));
    g_geom[13] = 1; g_geom[14] = (int)g; g_geom[15] = P.lds_bytes; g_geom[16] = 0;
    emu_lds_limit(P.lds_bytes);
    switch (metric) {
    case 0: emu_launch(g, APDC_THREADS, [&] { ap_dtw_cost_kernel<0>(P); }); break;
    case 1: emu_launch(g, APDC_THREADS, [&] { ap_dtw_cost_kernel<1>(P); }); break;
    case 2: emu_launch(g, APDC_THREADS, [&] { ap_dtw_cost_kernel<2>(P); }); break;
    default: emu_launch(g, APDC_THREADS, [&] { ap_dtw_cost_kernel<3>(P); }); break;
    }
    return AP_OK;
}

int emu_dtw_accumulate_f32(const float *C, int64_t B, int64_t N, int64_t M, int64_t c_row_stride, int n_steps, const int32_t *steps_ab,
                           const float *weights_add, const float *weights_mul, int subseq, int use_band, int64_t band_r, float *D,
                           int64_t d_row_stride, uint8_t *steps, int64_t steps_row_stride, int grid) {
    ApDtwAccParams P;
    int rc = ap_prepare_dtw_accumulate(P, C, B, N, M, c_row_stride, n_steps, steps_ab, weights_add, weights_mul, subseq, use_band, band_r,
                                       D, d_row_stride, steps, steps_row_stride);
    if (rc != AP_OK) return rc;
    g_geom[13] = (int)P.n_diag; g_geom[14] = 0; g_geom[15] = P.lds_bytes; g_geom[16] = P.fast;
    for (int64_t dg = 0; dg < P.n_diag; ++dg) {
        unsigned g = (unsigned)ap_dtw_acc_diagonal(P, dg);
        if (grid > 0) g = (unsigned)grid;
        if ((int)g > g_geom[14]) g_geom[14] = (int)g;
        emu_lds_limit(P.lds_bytes);
        if (P.fast) emu_launch(g, 64 * APDT_WAVES, [&] { ap_dtw_accumulate_kernel<true>(P); });
        else emu_launch(g, 64 * APDT_WAVES, [&] { ap_dtw_accumulate_kernel<false>(P); });
    }
    return AP_OK;
}

int emu_dtw_backtrack_i32(const float *D, const uint8_t *steps, const int32_t *start, int64_t B, int64_t N, int64_t M, int64_t d_row_stride,
                          int64_t steps_row_stride, int n_steps, const int32_t *steps_ab, int subseq, int32_t *path, int32_t *len,
                          int grid) {
    ApDtwBtParams P;
    int rc = ap_prepare_dtw_backtrack(P, D, steps, start, B, N, M, d_row_stride, steps_row_stride, n_steps, steps_ab, subseq, path, len);
    if (rc != AP_OK) return rc;
    const unsigned g = (unsigned)(grid > 0 ? grid : ap_dtw_grid(B));
    g_geom[13] = 1; g_geom[14] = (int)g; g_geom[15] = P.lds_bytes; g_geom[16] = 0;
    emu_lds_limit(P.lds_bytes);
    emu_launch(g, 64, [&] { ap_dtw_backtrack_kernel(P); });
    return AP_OK;
}

}  // extern "C"
