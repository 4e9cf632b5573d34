// The dB conversion shared by every kernel that converts on load or on store (kernels_pointwise.h: ap_to_db_kernel,
// ap_dct_kernel; kernels_onset.h): one definition, so that every route gives the same bits.
#pragma once
#include "fft_lds.h"

struct ApDbParams {
    float coef, amin, ref_value, top_db;     // top_db < 0: no clip
    const unsigned *ref_key, *smax_key;
};
AP_DEV float ap_db_ref(const ApDbParams &D) {
    return fmaxf(D.ref_key ? ap_fkey_inv(*D.ref_key) : D.ref_value, D.amin);
}
AP_DEV float ap_db_value(const ApDbParams &D, float ref, float s) {
    return D.coef * log10f(fmaxf(s, D.amin) / ref);
}
AP_DEV float ap_db_floor(const ApDbParams &D, float ref) {
    return D.top_db >= 0.0f ? ap_db_value(D, ref, ap_fkey_inv(*D.smax_key)) - D.top_db : -INFINITY;
}
