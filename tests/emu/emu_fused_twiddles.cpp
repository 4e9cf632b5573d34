// TEST INFRASTRUCTURE ONLY.  The scalar twins of the fused twiddle primitives of csrc/fft_lds.h ("twiddles folded
// into the butterfly level that consumes them"), built for the CPU through emu_shim.h, one call each on host values.
#include "emu_shim.h"

#include "../../mlx-audio-primitives_amd/csrc/fft_lds.h"

extern "C" {

// in: n records of 6 complex (a, b, x2, x3, wa = (c, s), wb) and the constants (ca, ta, cb, tb); out: n records of
// 24 complex: the (sum, difference) of ap_sumdiff_c1 / _c2 / _w1 / _w2, then the four outputs each of
// ap_fft4_twiddled, ap_fft4_twiddled3, ap_fft4_c and ap_fft4_c_a2mi on (a, b, x2, x3).
int emu_fused_twiddle_prims(const float *in, int64_t n, float ca, float ta, float cb, float tb, float *out) {
    const ap_float2 *I = reinterpret_cast<const ap_float2 *>(in);
    ap_float2 *O = reinterpret_cast<ap_float2 *>(out);
    for (int64_t i = 0; i < n; ++i, I += 6, O += 24) {
        const ap_float2 a = I[0], b = I[1], x2 = I[2], x3 = I[3], wa = I[4], wb = I[5];
        ap_sumdiff_c1(a, b, cb, tb, O[0], O[1]);
        ap_sumdiff_c2(a, ca, ta, b, cb, tb, O[2], O[3]);
        ap_sumdiff_w1(a, b, wb, O[4], O[5]);
        ap_sumdiff_w2(a, wa, b, wb, O[6], O[7]);
        ap_fft4_twiddled(a, wa, b, wb, x2, wb, x3, wa, O[8], O[9], O[10], O[11]);
        O[12] = a; O[13] = b; O[14] = x2; O[15] = x3;
        ap_fft4_twiddled3(O[12], O[13], wb, O[14], wa, O[15], wb);
        O[16] = a; O[17] = b; O[18] = x2; O[19] = x3;
        ap_fft4_c(O[16], O[17], O[18], O[19], ca, ta, cb, tb, ca, tb);
        O[20] = a; O[21] = b; O[22] = x2; O[23] = x3;
        ap_fft4_c_a2mi(O[20], O[21], O[22], O[23], ca, ta, cb, tb);
    }
    return 0;
}

}  // extern "C"
