// TEST INFRASTRUCTURE ONLY.  The onset kernels (kernels_onset.h) built for the CPU through emu_shim.h, behind emu_
// twins of ap_onset_strength_f32 and ap_peak_pick_f32 that take HOST pointers.  Same validation and geometry
// (ap_prepare_onset_strength, ap_prepare_peak_pick), same kernel bodies; `grid` > 0 overrides the number of
// workgroups (the tiles / rows are then walked in a grid-stride loop).
#include "emu_shim.h"

alignas(16) char ap_smem[160 * 1024];

#include "../../mlx-audio-primitives_amd/csrc/kernels_onset.h"

static thread_local char g_err[512] = "";
char *ap_error_buffer() { return g_err; }
void ap_set_error(const char *msg) { std::snprintf(g_err, sizeof(g_err), "%s", msg); }

extern "C" {

const char *emu_onset_last_error() { return g_err; }
int emu_onset_lds_overruns() { return emu_lds_overruns; }
int emu_peak_pick_max_frames() { return APPK_TMAX; }

// geometry the prepare step chose: {staged, n_tt, lds_bytes}
static int g_geom[3];
const int *emu_onset_geometry() { return g_geom; }

int emu_onset_strength_f32(const float *S, int64_t B, int64_t M, int64_t T, int64_t row_stride, const float *ref,
                           int64_t ref_row_stride, int lag, int max_size, int shift, int db_mode, float db_coef,
                           float db_amin, float db_ref, float db_top_db, const unsigned *smax_key, float *out,
                           int64_t out_row_stride, int grid) {
    ApOnsetParams P;
    int rc = ap_prepare_onset_strength(P, S, B, M, T, row_stride, ref, ref_row_stride, lag, max_size, shift, db_mode, db_coef,
                                       db_amin, db_ref, db_top_db, smax_key, out, out_row_stride);
    if (rc != AP_OK) return rc;
    g_geom[0] = P.staged; g_geom[1] = P.n_tt; g_geom[2] = P.lds_bytes;
    const unsigned g = (unsigned)(grid > 0 ? grid : ap_onset_grid(P));
    emu_lds_limit(P.lds_bytes);
    if (P.db) emu_launch(g, 64 * APON_WAVES, [&] { ap_onset_strength_kernel<true>(P); });
    else emu_launch(g, 64 * APON_WAVES, [&] { ap_onset_strength_kernel<false>(P); });
    return AP_OK;
}

// the float32 dB values the kernel computes on load (the reference of the dB-mode tests takes these)
int emu_onset_db_values(const float *S, int64_t n, float db_coef, float db_amin, float db_ref, float db_top_db,
                        const unsigned *smax_key, float *out) {
    ApDbParams D;
    D.coef = db_coef; D.amin = db_amin; D.ref_value = db_ref; D.top_db = db_top_db >= 0.0f ? db_top_db : -1.0f;
    D.ref_key = nullptr; D.smax_key = smax_key;
    const float ref = ap_db_ref(D), floor_v = ap_db_floor(D, ref);
    for (int64_t i = 0; i < n; ++i) out[i] = fmaxf(ap_db_value(D, ref, S[i]), floor_v);
    return AP_OK;
}

unsigned emu_onset_fkey(float v) { return ap_fkey(v); }

int emu_peak_pick_f32(const float *x, int64_t B, int64_t T, int64_t row_stride, int pre_max, int post_max, int pre_avg,
                      int post_avg, float delta, int wait, int normalize, int guard, int backtrack, const float *energy,
                      int64_t energy_row_stride, unsigned char *out_mask, int *out_count, int grid) {
    ApPeakPickParams P;
    int rc = ap_prepare_peak_pick(P, x, B, T, row_stride, pre_max, post_max, pre_avg, post_avg, delta, wait, normalize, guard,
                                  backtrack, energy, energy_row_stride, out_mask, out_count);
    if (rc != AP_OK) return rc;
    const unsigned g = (unsigned)(grid > 0 ? grid : ap_peak_pick_grid(P));
    emu_lds_limit(P.lds_bytes);
    emu_launch(g, APPK_BLOCK, [&] { ap_peak_pick_kernel(P); });
    return AP_OK;
}

}  // extern "C"
