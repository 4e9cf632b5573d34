// TEST INFRASTRUCTURE ONLY.  The PCEN kernel (kernels_pcen.h) built for the CPU through emu_shim.h, behind an emu_ twin
// of ap_pcen_f32 that takes HOST pointers.  Same validation, power table and geometry (ap_prepare_pcen), same kernel
// body; `grid` > 0 overrides the number of workgroups (the rows are then walked in a grid-stride loop).
#include "emu_shim.h"

alignas(16) char ap_smem[160 * 1024];

#include "../../mlx-audio-primitives_amd/csrc/kernels_pcen.h"

static thread_local char g_err[512] = "";
char *ap_error_buffer() { return g_err; }
void ap_set_error(const char *msg) { std::snprintf(g_err, sizeof(g_err), "%s", msg); }

extern "C" {

const char *emu_pcen_last_error() { return g_err; }

// what the prepare step chose: {chain, n_tt, grid}
static int g_geom[3];
const int *emu_pcen_geometry() { return g_geom; }

int emu_pcen_f32(const float *S, int64_t B, int64_t M, int64_t T, int64_t row_stride, const float *ref, int64_t ref_row_stride,
                 int max_size, double b, float gain, float bias, float power, float eps, const float *zi, float *out,
                 int64_t out_row_stride, float *zf, int grid) {
    ApPcenParams P;
    int rc = ap_prepare_pcen(P, S, B, M, T, row_stride, ref, ref_row_stride, max_size, b, gain, bias, power, eps, zi, out,
                             out_row_stride, zf);
    if (rc != AP_OK) return rc;
    const unsigned g = (unsigned)(grid > 0 ? grid : ap_pcen_grid(P));
    g_geom[0] = P.chain; g_geom[1] = P.n_tt; g_geom[2] = (int)g;
    if (P.chain == APPC_LOG) emu_launch(g, 64 * APPC_WAVES, [&] { ap_pcen_kernel<APPC_LOG>(P); });
    else if (P.chain == APPC_POWER) emu_launch(g, 64 * APPC_WAVES, [&] { ap_pcen_kernel<APPC_POWER>(P); });
    else emu_launch(g, 64 * APPC_WAVES, [&] { ap_pcen_kernel<APPC_GENERAL>(P); });
    return AP_OK;
}

}  // extern "C"
