// TEST INFRASTRUCTURE ONLY.  The chroma kernels (kernels_chroma.h) built for the CPU through emu_shim.h, behind emu_
// twins of ap_chroma_fold_f32 / ap_chroma_cens_f32 that take HOST pointers.  Same validation and geometry
// (ap_prepare_chroma_fold / ap_prepare_chroma_cens), same kernel bodies; `grid` > 0 overrides the number of workgroups
// (the tiles are then walked in a grid-stride loop).
#include "emu_shim.h"

alignas(16) char ap_smem[160 * 1024];

#include "../../mlx-audio-primitives_amd/csrc/kernels_chroma.h"

static thread_local char g_err[512] = "";
char *ap_error_buffer() { return g_err; }
void ap_set_error(const char *msg) { std::snprintf(g_err, sizeof(g_err), "%s", msg); }

template <int NACC>
static void fold_kind(const ApChromaFoldParams &P, unsigned g) {
    if (P.in_kind == 0) emu_launch(g, 64 * APCH_WAVES, [&] { ap_chroma_fold_kernel<NACC, 0>(P); });
    else if (P.in_kind == 1) emu_launch(g, 64 * APCH_WAVES, [&] { ap_chroma_fold_kernel<NACC, 1>(P); });
    else emu_launch(g, 64 * APCH_WAVES, [&] { ap_chroma_fold_kernel<NACC, 2>(P); });
}

extern "C" {

const char *emu_chroma_last_error() { return g_err; }

// {fold: frames per tile, waves, bins per run, cap on n_out; cens: frames per tile, cap on n_taps, threads;
//  last call: accumulators, grid, lds_bytes}
static int g_geom[10] = {APCH_TT, APCH_WAVES, APCH_U, APCH_MAX_OUT, APCN_TT, APCN_MAX_SMOOTH, APCN_THREADS, 0, 0, 0};
const int *emu_chroma_geometry() { return g_geom; }
int emu_chroma_lds_overruns() { return emu_lds_overruns; }

int emu_chroma_fold_f32(const float *x, int in_kind, int64_t B, int K, int64_t T, int64_t in_row_stride, const float *w, int n_out,
                        int pre_l1, int use_threshold, float threshold, int norm, float *out, int64_t out_row_stride, int grid) {
    ApChromaFoldParams P;
    int rc = ap_prepare_chroma_fold(P, x, in_kind, B, K, T, in_row_stride, w, n_out, pre_l1, use_threshold, threshold, norm, out,
                                    out_row_stride);
    if (rc != AP_OK) return rc;
    const unsigned g = (unsigned)(grid > 0 ? grid : ap_chroma_grid(P.n_tiles));
    g_geom[7] = P.nacc; g_geom[8] = (int)g; g_geom[9] = P.lds_bytes;
    emu_lds_limit(P.lds_bytes);
    switch (P.nacc) {
    case 6: fold_kind<6>(P, g); break;
    case 12: fold_kind<12>(P, g); break;
    case 24: fold_kind<24>(P, g); break;
    case 36: fold_kind<36>(P, g); break;
    default: fold_kind<48>(P, g); break;
    }
    return AP_OK;
}

int emu_chroma_cens_f32(const float *chroma, int64_t B, int n, int64_t T, int64_t in_row_stride, const float *taps, int n_taps,
                        int norm, float *out, int64_t out_row_stride, int grid) {
    ApChromaCensParams P;
    int rc = ap_prepare_chroma_cens(P, chroma, B, n, T, in_row_stride, taps, n_taps, norm, out, out_row_stride);
    if (rc != AP_OK) return rc;
    const unsigned g = (unsigned)(grid > 0 ? grid : ap_chroma_grid(P.n_tiles));
    g_geom[7] = 0; g_geom[8] = (int)g; g_geom[9] = P.lds_bytes;
    emu_lds_limit(P.lds_bytes);
    emu_launch(g, APCN_THREADS, [&] { ap_chroma_cens_kernel(P); });
    return AP_OK;
}

}  // extern "C"
