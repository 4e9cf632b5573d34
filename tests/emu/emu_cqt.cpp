// TEST INFRASTRUCTURE ONLY.  The constant-Q kernel (kernels_cqt.h) built for the CPU through emu_shim.h, behind an emu_
// twin of ap_cqt_f32 that takes HOST pointers.  Same validation and geometry (ap_prepare_cqt), same kernel body;
// `grid` > 0 overrides the number of workgroups (the tiles are then walked in a grid-stride loop).
#include "emu_shim.h"

alignas(16) char ap_smem[160 * 1024];

#include "../../mlx-audio-primitives_amd/csrc/kernels_cqt.h"

static thread_local char g_err[512] = "";
char *ap_error_buffer() { return g_err; }
void ap_set_error(const char *msg) { std::snprintf(g_err, sizeof(g_err), "%s", msg); }

extern "C" {

const char *emu_cqt_last_error() { return g_err; }

// the tile constants and what the prepare step chose:
// {frames per tile (as many as the signal ring holds at this hop, at most 32), bins per group, taps per chunk, lanes, reduction chain, n_groups, n_tt, grid, lds_bytes, max taps}
static int g_geom[10];
const int *emu_cqt_geometry() { return g_geom; }
int emu_cqt_lds_overruns() { return emu_lds_overruns; }

int emu_cqt_f32(const float *y, int64_t B, int64_t L, int hop, int pad_mode, const float *taps, const int64_t *tap_offset,
                const int32_t *m0, const float *scale, int n_bins, int64_t T, float *out, int64_t out_row_stride, int grid) {
    ApCqtParams P;
    int rc = ap_prepare_cqt(P, y, B, L, hop, pad_mode, taps, tap_offset, m0, scale, n_bins, T, out, out_row_stride);
    if (rc != AP_OK) return rc;
    const unsigned g = (unsigned)(grid > 0 ? grid : ap_cqt_grid(P));
    g_geom[0] = P.tt; g_geom[1] = APCQ_K; g_geom[2] = APCQ_C; g_geom[3] = 64; g_geom[4] = 32;
    g_geom[5] = P.n_groups; g_geom[6] = P.n_tt; g_geom[7] = (int)g; g_geom[8] = P.lds_bytes; g_geom[9] = APCQ_MAX_TAPS;
    emu_lds_limit(P.lds_bytes);
    emu_launch(g, 64 * APCQ_WAVES, [&] { ap_cqt_kernel(P); });
    return AP_OK;
}

}  // extern "C"
