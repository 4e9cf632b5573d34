// TEST INFRASTRUCTURE ONLY.  The YIN kernels (kernels_yin.h) built for the CPU through emu_shim.h, behind emu_
// twins of ap_yin_f32 / ap_yin_cmnd_f32 that take HOST pointers.  Same validation and geometry
// (ap_prepare_yin), same kernel bodies; `grid` > 0 overrides the persistent grid so that a handful of frames is
// spread over several waves and workgroups.
#include "emu_shim.h"

alignas(16) char ap_smem[160 * 1024];

#include "../../mlx-audio-primitives_amd/csrc/kernels_yin.h"

static thread_local char g_err[512] = "";
char *ap_error_buffer() { return g_err; }
void ap_set_error(const char *msg) { std::snprintf(g_err, sizeof(g_err), "%s", msg); }

template <bool CURVE>
static int emu_yin_run(const ApYinParams &P, const float *tw, int grid) {
    emu_lds_limit(P.lds_bytes);
    if (tw) {
        if (!ap_yin_wave_shape(P.n, P.hop, P.L)) AP_FAIL(AP_ERR_UNSUPPORTED, "yin: the wave kernel serves frame_length 2048 / 1024 with an even hop_length");
        const unsigned g = (unsigned)(grid > 0 ? grid : ap_yin_wave_grid(P));
        if (P.n == 2048) emu_launch(g, 64 * APY_WAVES, [&] { ap_yin_wave_kernel<2048, CURVE>(P); });
        else emu_launch(g, 64 * APY_WAVES, [&] { ap_yin_wave_kernel<1024, CURVE>(P); });
    } else {
        emu_launch((unsigned)(grid > 0 ? grid : ap_yin_general_grid(P)), AP_BLOCK, [&] { ap_yin_general_kernel<CURVE>(P); });
    }
    return AP_OK;
}

extern "C" {

const char *emu_yin_last_error() { return g_err; }
int emu_yin_lds_overruns() { return emu_lds_overruns; }
int emu_yin_fused(int frame_length, int hop, int64_t L) { return ap_yin_wave_shape(frame_length, hop, L) ? 1 : 0; }

int emu_yin_f32(const float *y, int64_t B, int64_t L, int frame_length, int hop, int center, int lo, int hi, float sr,
                float trough_threshold, const float *tw, float *f0, float *aper, int grid) {
    ApYinParams P;
    if (!f0) AP_FAIL(AP_ERR_INVALID, "yin: NULL buffer");
    int rc = ap_prepare_yin(P, y, B, L, frame_length, hop, center, lo, hi, sr, trough_threshold, tw, f0, aper, nullptr);
    if (rc != AP_OK) return rc;
    return emu_yin_run<false>(P, tw, grid);
}

int emu_yin_cmnd_f32(const float *y, int64_t B, int64_t L, int frame_length, int hop, int center, int lo, int hi,
                     const float *tw, float *out, int grid) {
    ApYinParams P;
    if (!out) AP_FAIL(AP_ERR_INVALID, "yin_cmnd: NULL buffer");
    int rc = ap_prepare_yin(P, y, B, L, frame_length, hop, center, lo, hi, 1.0f, 0.0f, tw, nullptr, nullptr, out);
    if (rc != AP_OK) return rc;
    return emu_yin_run<true>(P, tw, grid);
}

}  // extern "C"
