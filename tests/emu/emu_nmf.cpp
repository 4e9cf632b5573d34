// TEST INFRASTRUCTURE ONLY.  The NMF kernels (kernels_nmf.h) built for the CPU through emu_shim.h and the MFMA model of
// emu_mfma.h, behind emu_ twins of ap_nmf_mu_f32 / ap_nmf_objective_f32 that take HOST pointers.  Same validation,
// same sequence of launches (apn_iterate / apn_objective), same kernel bodies; `grid` > 0 overrides the workgroups.
#include "emu_mfma.h"

alignas(16) char ap_smem[160 * 1024];

#include "../../mlx-audio-primitives_amd/csrc/kernels_nmf.h"

static thread_local char g_err[512] = "";
char *ap_error_buffer() { return g_err; }
void ap_set_error(const char *msg) { std::snprintf(g_err, sizeof(g_err), "%s", msg); }

struct EmuNmfGo {
    int grid;
    int operator()(ApNmfKernel kern, int g, int lds, const ApNmfParams &P) const {
        emu_lds_limit(lds > 0 ? lds : 16);
        emu_launch((unsigned)(grid > 0 ? grid : g), APN_THREADS, [&] { kern(P); });
        return AP_OK;
    }
};

extern "C" {

const char *emu_nmf_last_error() { return g_err; }
int emu_nmf_lds_overruns() { return emu_lds_overruns; }
int64_t emu_nmf_workspace_bytes(int64_t B, int64_t T, int K) { return ap_nmf_ws_bytes(B, T, K); }

int emu_nmf_mu_f32(const float *V, int64_t B, int64_t F, int64_t T, int64_t rs, int K, float *W, float *H, int n_iter, int loss,
                   int update_w, float eps, void *workspace, int grid) {
    ApNmfParams P;
    int rc = ap_prepare_nmf(P, V, B, F, T, rs, K, W, H, loss, eps, workspace);
    if (rc != AP_OK) return rc;
    EmuNmfGo go{grid};
    return apn_iterate(go, P, n_iter, loss, update_w);
}

int emu_nmf_objective_f32(const float *V, int64_t B, int64_t F, int64_t T, int64_t rs, int K, float *W, float *H, int loss, float eps,
                          double *out, void *workspace, int grid) {
    ApNmfParams P;
    int rc = ap_prepare_nmf(P, V, B, F, T, rs, K, W, H, loss, eps, workspace);
    if (rc != AP_OK) return rc;
    EmuNmfGo go{grid};
    return apn_objective(go, P, loss, out);
}

}  // extern "C"
