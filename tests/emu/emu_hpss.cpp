// TEST INFRASTRUCTURE ONLY.  The HPSS kernels (kernels_hpss.h) built for the CPU through emu_shim.h, behind an emu_
// twin of ap_hpss_f32 that takes HOST pointers.  Same validation and geometry (ap_prepare_hpss), same kernel body;
// `f_tile` > 0 overrides the tile height so that a small array spans several tiles along F (a tile is always 64
// frames wide), `grid` > 0 the number of workgroups (the tiles are then walked in a grid-stride loop).
#include "emu_shim.h"

alignas(16) char ap_smem[160 * 1024];

#include "../../mlx-audio-primitives_amd/csrc/kernels_hpss.h"

static thread_local char g_err[512] = "";
char *ap_error_buffer() { return g_err; }
void ap_set_error(const char *msg) { std::snprintf(g_err, sizeof(g_err), "%s", msg); }

extern "C" {

const char *emu_hpss_last_error() { return g_err; }
int emu_hpss_lds_overruns() { return emu_lds_overruns; }
int emu_hpss_fused(int k_harm, int k_perc) { return ap_hpss_network_sizes(k_harm, k_perc) ? 1 : 0; }
int emu_hpss_net_comparators() { return APHP_NET_N; }
int emu_hpss_net_ops() { return APHP_NET_OPS; }
int emu_hpss_default_tile() { return APHP_FT; }

// geometry the prepare step chose: {fused, f_tile, n_ft, n_tt, lds_bytes}
static int g_geom[5];
const int *emu_hpss_geometry() { return g_geom; }

int emu_hpss_f32(const float *S, int is_complex, int64_t B, int64_t F, int64_t T, int64_t row_stride_in, int k_harm,
                 int k_perc, float margin_harm, float margin_perc, float power, int mode, int general, float *out_h,
                 float *out_p, int64_t row_stride_out, int f_tile, int grid) {
    ApHpssParams P;
    int rc = ap_prepare_hpss(P, S, is_complex, B, F, T, row_stride_in, k_harm, k_perc, margin_harm, margin_perc, power,
                             mode, general, out_h, out_p, row_stride_out, f_tile);
    if (rc != AP_OK) return rc;
    g_geom[0] = P.fused; g_geom[1] = P.f_tile; g_geom[2] = P.n_ft; g_geom[3] = P.n_tt; g_geom[4] = P.lds_bytes;
    const unsigned g = (unsigned)(grid > 0 ? grid : ap_hpss_grid(P));
    emu_lds_limit(P.lds_bytes);
    if (P.fused) {
        if (is_complex) emu_launch(g, 64 * APHP_WAVES, [&] { ap_hpss_kernel<true, true>(P); });
        else emu_launch(g, 64 * APHP_WAVES, [&] { ap_hpss_kernel<false, true>(P); });
    } else {
        if (is_complex) emu_launch(g, 64 * APHP_WAVES, [&] { ap_hpss_kernel<true, false>(P); });
        else emu_launch(g, 64 * APHP_WAVES, [&] { ap_hpss_kernel<false, false>(P); });
    }
    return AP_OK;
}

}  // extern "C"
