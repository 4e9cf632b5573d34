// TEST INFRASTRUCTURE ONLY.  The rhythm kernels (kernels_rhythm.h) built for the CPU through emu_shim.h, behind emu_
// twins of ap_tempogram_f32, ap_tempo_pick_f32 and ap_beat_track_f32 that take HOST pointers.  Same validation and
// geometry (ap_prepare_*), same kernel bodies; `grid` > 0 overrides the number of workgroups (the tiles / columns /
// rows are then walked in a grid-stride loop).
#include "emu_shim.h"

alignas(16) char ap_smem[160 * 1024];

#include "../../mlx-audio-primitives_amd/csrc/kernels_rhythm.h"

static thread_local char g_err[512] = "";
char *ap_error_buffer() { return g_err; }
void ap_set_error(const char *msg) { std::snprintf(g_err, sizeof(g_err), "%s", msg); }

extern "C" {

const char *emu_rhythm_last_error() { return g_err; }
int emu_rhythm_lds_overruns() { return emu_lds_overruns; }
int emu_tempogram_max_win() { return APTG_WMAX; }
int emu_beat_track_max_frames() { return APBT_TMAX; }
int emu_beat_track_max_period() { return APBT_PMAX; }
int emu_beat_half(int P) { return apbt_half(P); }

int64_t emu_tempogram_agg_floats(int64_t B, int64_t n, int W, int center) {
    const int64_t T = ap_tempogram_frames(n, W, center);
    if (B <= 0 || T <= 0 || W < 1) return 0;
    return B * ((T + APTG_TT - 1) / APTG_TT) * W;
}

int emu_tempogram_f32(const float *env, int64_t B, int64_t n, int64_t rs, const float *window, int W, int center, int norm,
                      const float *tw, float *out, float *agg, int grid) {
    ApTempogramParams P;
    int rc = ap_prepare_tempogram(P, env, B, n, rs, window, W, center, norm, tw, out, agg);
    if (rc != AP_OK) return rc;
    emu_lds_limit(P.lds_bytes);
    if (tw) {
        emu_launch((unsigned)(grid > 0 ? grid : ap_tempogram_wave_grid(P)), 64 * APTG_WAVES, [&] { ap_tempogram_wave_kernel(P); });
        return AP_OK;
    }
    emu_launch((unsigned)(grid > 0 ? grid : ap_tempogram_grid(P)), 64 * APTG_WAVES, [&] { ap_tempogram_kernel(P); });
    return AP_OK;
}

int emu_tempo_pick_f32(const float *g, int64_t B, int64_t n_col, int W, int64_t sb, int64_t sk, int64_t sc, int64_t n_red,
                       int64_t sr, float div, const float *prior, int *idx, int grid) {
    ApTempoPickParams P;
    int rc = ap_prepare_tempo_pick(P, g, B, n_col, W, sb, sk, sc, n_red, sr, div, prior, idx);
    if (rc != AP_OK) return rc;
    emu_lds_limit(P.lds_bytes);
    emu_launch((unsigned)(grid > 0 ? grid : ap_tempo_pick_grid(P)), APTP_BLOCK, [&] { ap_tempo_pick_kernel(P); });
    return AP_OK;
}

int emu_beat_track_f32(const float *env, int64_t B, int64_t T, int64_t rs, const int *period, float tightness, int trim,
                       unsigned char *mask, int *count, float *L, float *C, int *link, int grid) {
    ApBeatParams P;
    int rc = ap_prepare_beat_track(P, env, B, T, rs, period, tightness, trim, mask, count, L, C, link);
    if (rc != AP_OK) return rc;
    emu_lds_limit(P.lds_bytes);
    emu_launch((unsigned)(grid > 0 ? grid : ap_beat_track_grid(P)), APBT_BLOCK, [&] { ap_beat_track_kernel(P); });
    return AP_OK;
}

}  // extern "C"
