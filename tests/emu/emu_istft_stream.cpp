// TEST INFRASTRUCTURE ONLY.  The streaming ISTFT kernels (kernels_istft_stream.h) built for the CPU through
// emu_shim.h, behind an emu_ twin of ap_istft_stream_f32 that takes HOST pointers and a tile size G (small
// tiles put halos across workgroups).  Same validation / geometry (ap_prepare_istft_stream), same kernel bodies;
// the two-launch path runs ap_irfft_generic_kernel (kernels_generic.h) for its transforms.
#include "emu_shim.h"

alignas(16) char ap_smem[160 * 1024];

#include "../../mlx-audio-primitives_amd/csrc/kernels_generic.h"
#include "../../mlx-audio-primitives_amd/csrc/kernels_istft_stream.h"

static thread_local char g_err[512] = "";
char *ap_error_buffer() { return g_err; }
void ap_set_error(const char *msg) { std::snprintf(g_err, sizeof(g_err), "%s", msg); }

template <int N>
static void emu_stream_fused(const ApIstftStreamParams &P, int64_t B) {
    emu_lds_limit(P.lds_bytes);
    emu_launch((unsigned)(P.tiles_per_clip * B), AP_BLOCK, [&] { ap_istft_stream_kernel<N>(P); });
}

extern "C" {

const char *emu_istft_stream_last_error() { return g_err; }
int emu_istft_stream_lds_overruns() { return emu_lds_overruns; }

int emu_istft_stream_f32(const float *S, int64_t B, int64_t T, int64_t row_stride, int n_fft, int hop,
                         const float *window, const float *tw, int64_t frame0, const float *carry_in,
                         float *carry_out, int final_, int64_t lo, int64_t hi, float *frames_ws, float *out, int G) {
    ApIstftStreamParams P;
    int rc = ap_prepare_istft_stream(P, S, B, T, row_stride, n_fft, hop, window, tw, frame0, carry_in, carry_out,
                                     final_, lo, hi, out, G);
    if (rc != AP_OK) return rc;
    if (B == 0 || (T == 0 && n_fft == hop)) return AP_OK;
    switch (n_fft) {
        case 2048: emu_stream_fused<2048>(P, B); return AP_OK;
        case 1024: emu_stream_fused<1024>(P, B); return AP_OK;
        case 512: emu_stream_fused<512>(P, B); return AP_OK;
        case 400: emu_stream_fused<400>(P, B); return AP_OK;
        case 256: emu_stream_fused<256>(P, B); return AP_OK;
        default: break;
    }
    if (T > 0) {
        if (row_stride != T) AP_FAIL(AP_ERR_UNSUPPORTED, "istft_stream: dense spectrum needed");
        ApIrfftParams Q;
        rc = ap_prepare_irfft(Q, S, B, T, n_fft, tw, frames_ws);
        if (rc != AP_OK) return rc;
        emu_lds_limit(Q.tile.lds_bytes);
        emu_launch((unsigned)(Q.tiles_per_clip * B), AP_BLOCK, [&] { ap_irfft_generic_kernel(Q); });
        P.frames = frames_ws;
    }
    emu_launch((unsigned)(P.blocks_per_row * B), AP_BLOCK, [&] { ap_istft_stream_ola_kernel(P); });
    return AP_OK;
}

}  // extern "C"
