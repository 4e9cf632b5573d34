// TEST INFRASTRUCTURE ONLY.  The sequence-decoding kernels (kernels_viterbi.h) built for the CPU through emu_shim.h,
// behind emu_ twins of ap_viterbi_emission_f32 / ap_viterbi_decode_f32 / ap_viterbi_binary_f32 that take HOST pointers.
// Same validation and geometry (ap_prepare_viterbi_*), same kernel bodies; `grid` > 0 overrides the number of
// workgroups (the work items are then walked in a grid-stride loop); `lt_lds_max` is the threshold the HIP entry takes
// from its default.
#include <cstring>

#include "emu_shim.h"

alignas(16) char ap_smem[160 * 1024];

#include "../../mlx-audio-primitives_amd/csrc/kernels_viterbi.h"

static thread_local char g_err[512] = "";
char *ap_error_buffer() { return g_err; }
void ap_set_error(const char *msg) { std::snprintf(g_err, sizeof(g_err), "%s", msg); }

extern "C" {

const char *emu_viterbi_last_error() { return g_err; }

// {block, cap on S, cap on T, lanes per state at most, backtrack chunk, lt-in-LDS ceiling, emission tile, steps per word,
//  labels per wave; last call: grid, lds_bytes, lanes per state, lt in LDS}
static int g_geom[13] = {APV_THREADS, APV_MAX_STATES, APV_MAX_STEPS, APV_MAX_G, APV_CHUNK, APV_LT_LDS_MAX, APVE_TILE, APVB_WORD,
                         APVB_TILE, 0, 0, 0, 0};
const int *emu_viterbi_geometry() { return g_geom; }
int emu_viterbi_lds_overruns() { return emu_lds_overruns; }

int emu_viterbi_emission_f32(const float *prob, int64_t B, int64_t S, int64_t T, int64_t row_stride, int mode, const float *lps, float *E,
                             int32_t *flags, int grid) {
    ApViterbiEmisParams P;
    int rc = ap_prepare_viterbi_emission(P, prob, B, S, T, row_stride, mode, lps, E, flags);
    if (rc != AP_OK) return rc;
    std::memset(flags, 0, (size_t)B * sizeof(int32_t));
    const unsigned g = (unsigned)(grid > 0 ? grid : ap_viterbi_grid(P.n_items));
    g_geom[9] = (int)g; g_geom[10] = P.lds_bytes; g_geom[11] = 0; g_geom[12] = 0;
    emu_lds_limit(P.lds_bytes);
    emu_launch(g, APV_THREADS, [&] { ap_viterbi_emission_kernel(P); });
    return AP_OK;
}

int emu_viterbi_decode_f32(const float *E, int64_t B, int64_t S, int64_t T, const float *lt, const float *li, uint16_t *ptr,
                           int32_t *states, double *logp, int lt_lds_max, int grid) {
    ApViterbiDecParams P;
    int rc = ap_prepare_viterbi_decode(P, E, B, S, T, lt, li, ptr, states, logp, lt_lds_max);
    if (rc != AP_OK) return rc;
    const unsigned g = (unsigned)(grid > 0 ? grid : ap_viterbi_grid(B));
    g_geom[9] = (int)g; g_geom[10] = P.lds_bytes; g_geom[11] = P.G; g_geom[12] = P.lt_lds;
    emu_lds_limit(P.lds_bytes);
    if (P.lt_lds) emu_launch(g, APV_THREADS, [&] { ap_viterbi_decode_kernel<true, 1>(P); });
    else if (P.n_pass == 1) emu_launch(g, APV_THREADS, [&] { ap_viterbi_decode_kernel<false, 1>(P); });
    else if (P.n_pass == 2) emu_launch(g, APV_THREADS, [&] { ap_viterbi_decode_kernel<false, 2>(P); });
    else if (P.n_pass == 3) emu_launch(g, APV_THREADS, [&] { ap_viterbi_decode_kernel<false, 3>(P); });
    else emu_launch(g, APV_THREADS, [&] { ap_viterbi_decode_kernel<false, 4>(P); });
    return AP_OK;
}

int emu_viterbi_binary_f32(const float *E, int64_t B, int64_t S, int64_t T, const float *lt, int per_label, const float *li,
                           uint32_t *bits, int32_t *states, double *logp, int grid) {
    ApViterbiBinParams P;
    int rc = ap_prepare_viterbi_binary(P, E, B, S, T, lt, per_label, li, bits, states, logp);
    if (rc != AP_OK) return rc;
    const unsigned g = (unsigned)(grid > 0 ? grid : ap_viterbi_grid(P.n_items));
    g_geom[9] = (int)g; g_geom[10] = P.lds_bytes; g_geom[11] = 0; g_geom[12] = 0;
    emu_lds_limit(P.lds_bytes);
    emu_launch(g, 64, [&] { ap_viterbi_binary_kernel(P); });
    return AP_OK;
}

}  // extern "C"
