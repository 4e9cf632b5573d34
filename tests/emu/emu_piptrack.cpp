// TEST INFRASTRUCTURE ONLY.  The piptrack kernels (kernels_piptrack.h) built for the CPU through emu_shim.h, behind emu_
// twins of ap_piptrack_f32 / ap_piptrack_records_f32 / ap_piptrack_tuning_f32 / ap_pitch_hist_f32 that take HOST
// pointers.  Same validation and geometry (the ap_prepare_* steps), same kernel bodies; `grid` > 0 overrides the number
// of workgroups (tiles, groups and elements are then walked in a grid-stride loop).
#include <cstring>

#include "emu_shim.h"

alignas(16) char ap_smem[160 * 1024];

// What the kernels need and the shim lacks: integer atomics (the emulated threads are OS threads), a wave ballot and a
// broadcast of lane 0's value, both over the shim's per-wave barrier.
inline unsigned atomicAdd(unsigned *p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline unsigned atomicMin(unsigned *p, unsigned v) {
    unsigned old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
static unsigned long long emu_wave_words[1024];
inline unsigned long long emu_ballot64(bool p) {
    emu_wave_words[threadIdx.x] = p ? 1ull : 0ull;
    emu_wave_sync();
    unsigned long long m = 0;
    const unsigned w0 = threadIdx.x & ~63u;
    for (unsigned l = 0; l < 64; ++l) m |= emu_wave_words[w0 + l] << l;
    emu_wave_sync();
    return m;
}
inline unsigned long long emu_first_u64(unsigned long long v) {
    emu_wave_words[threadIdx.x] = v;
    emu_wave_sync();
    const unsigned long long r = emu_wave_words[threadIdx.x & ~63u];
    emu_wave_sync();
    return r;
}

#include "../../mlx-audio-primitives_amd/csrc/kernels_piptrack.h"

static thread_local char g_err[512] = "";
char *ap_error_buffer() { return g_err; }
void ap_set_error(const char *msg) { std::snprintf(g_err, sizeof(g_err), "%s", msg); }

static void launch_peaks(const ApPiptrackParams &P, unsigned g) {
    emu_lds_limit(P.lds_bytes);
    if (P.compact) {
        if (P.kind == 0) emu_launch(g, 64 * APPT_WAVES, [&] { ap_piptrack_kernel<0, true>(P); });
        else emu_launch(g, 64 * APPT_WAVES, [&] { ap_piptrack_kernel<1, true>(P); });
    } else {
        if (P.kind == 0) emu_launch(g, 64 * APPT_WAVES, [&] { ap_piptrack_kernel<0, false>(P); });
        else emu_launch(g, 64 * APPT_WAVES, [&] { ap_piptrack_kernel<1, false>(P); });
    }
}

extern "C" {

const char *emu_piptrack_last_error() { return g_err; }

// {frames per tile, waves, rows loaded ahead, records staged per wave, select threads, histogram threads, cap on bins;
//  last call: grid, lds_bytes}
static int g_geom[9] = {APPT_TT, APPT_WAVES, APPT_U, APPT_WCAP, APPT_SEL_THREADS, APPT_HIST_THREADS, APPT_MAX_BINS, 0, 0};
const int *emu_piptrack_geometry() { return g_geom; }
int emu_piptrack_lds_overruns() { return emu_lds_overruns; }

int emu_piptrack_f32(const float *S, int in_kind, int64_t B, int F, int64_t T, int64_t in_row_stride, int k_lo, int k_hi,
                     float threshold, int ref_mode, float ref_value, const float *ref, float bin_hz, float *pitches,
                     float *magnitudes, int64_t out_row_stride, int grid) {
    ApPiptrackParams P;
    int rc = ap_prepare_piptrack(P, S, in_kind, B, F, T, in_row_stride, k_lo, k_hi, threshold, ref_mode, ref_value, ref, bin_hz, 0,
                                 pitches, magnitudes, out_row_stride, 0, nullptr, 0, nullptr);
    if (rc != AP_OK) return rc;
    const unsigned g = (unsigned)(grid > 0 ? grid : ap_piptrack_grid(P.n_tiles));
    g_geom[7] = (int)g; g_geom[8] = P.lds_bytes;
    launch_peaks(P, g);
    return AP_OK;
}

int emu_piptrack_records_f32(const float *S, int in_kind, int64_t B, int F, int64_t T, int64_t in_row_stride, int k_lo, int k_hi,
                             float threshold, int ref_mode, float ref_value, const float *ref, float bin_hz, int per_clip,
                             float *records, int64_t capacity, uint64_t *counters, int grid) {
    ApPiptrackParams P;
    int rc = ap_prepare_piptrack(P, S, in_kind, B, F, T, in_row_stride, k_lo, k_hi, threshold, ref_mode, ref_value, ref, bin_hz, 1,
                                 nullptr, nullptr, 0, per_clip, records, capacity, (ap_u64 *)counters);
    if (rc != AP_OK) return rc;
    std::memset(counters, 0, (size_t)(per_clip ? B : 1) * sizeof(uint64_t));
    const unsigned g = (unsigned)(grid > 0 ? grid : ap_piptrack_grid(P.n_tiles));
    g_geom[7] = (int)g; g_geom[8] = P.lds_bytes;
    launch_peaks(P, g);
    return AP_OK;
}

int emu_piptrack_tuning_f32(const float *records, const uint64_t *counters, int64_t G, int64_t capacity, double bins_per_octave,
                            const double *edges, int n_bins, float *threshold_out, uint64_t *counts, int grid) {
    ApTuningParams Q;
    int rc = ap_prepare_piptrack_tuning(Q, records, (const ap_u64 *)counters, G, capacity, bins_per_octave, edges, n_bins,
                                        threshold_out, (ap_u64 *)counts);
    if (rc != AP_OK) return rc;
    const unsigned g = (unsigned)(grid > 0 ? grid : G);
    g_geom[7] = (int)g; g_geom[8] = Q.lds_bytes;
    emu_lds_limit(Q.lds_bytes);
    emu_launch(g, APPT_SEL_THREADS, [&] { ap_piptrack_tuning_kernel(Q); });
    return AP_OK;
}

int emu_pitch_hist_f32(const float *frequencies, int64_t n, double bins_per_octave, const double *edges, int n_bins,
                       uint64_t *counts, int grid) {
    ApPitchHistParams H;
    int rc = ap_prepare_pitch_hist(H, frequencies, n, bins_per_octave, edges, n_bins, (ap_u64 *)counts);
    if (rc != AP_OK) return rc;
    std::memset(counts, 0, (size_t)n_bins * sizeof(uint64_t));
    const unsigned g = (unsigned)(grid > 0 ? grid : ap_pitch_hist_grid(n));
    g_geom[7] = (int)g; g_geom[8] = H.lds_bytes;
    emu_lds_limit(H.lds_bytes);
    emu_launch(g, APPT_HIST_THREADS, [&] { ap_pitch_hist_kernel(H); });
    return AP_OK;
}

}  // extern "C"
