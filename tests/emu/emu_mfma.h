// TEST INFRASTRUCTURE ONLY.  A model of __builtin_amdgcn_mfma_f32_16x16x4f32 (v_mfma_f32_16x16x4_f32) for the fiber
// emulator of emu_shim.h, in the way of emu_lane_perm: every lane of the wave puts its operands into an exchange
// buffer, the wave meets, and every lane computes its four registers of D.
//   lane l holds A[l % 16][l / 16] and B[l / 16][l % 16];  register r of lane l is D[4 (l / 16) + r][l % 16];
//   D[i][j] = C[i][j] + sum_{c < 4} A[i][c] B[c][j], here as four fused multiply-adds in c order.
// A kernel written to a wrong model agrees with it: the layout is settled by tests/test_gpu_nmf.py on the hardware, not
// here.  (v_mfma_f32_32x32x2_f32 is not modelled: no kernel uses it.)
#pragma once
#include "emu_shim.h"

inline float emu_mfma_a[1024], emu_mfma_b[1024];

inline void emu_mfma_f32_16x16x4f32(float a, float b, float (&c)[4]) {      // all 64 lanes of the wave call it together
    emu_mfma_a[threadIdx.x] = a;
    emu_mfma_b[threadIdx.x] = b;
    emu_wave_sync();
    const unsigned base = threadIdx.x & ~63u, lane = threadIdx.x & 63u, j = lane & 15u;
    for (unsigned r = 0; r < 4; ++r) {
        const unsigned i = 4 * (lane >> 4) + r;
        for (unsigned k = 0; k < 4; ++k) c[r] = std::fmaf(emu_mfma_a[base + 16 * k + i], emu_mfma_b[base + 16 * k + j], c[r]);
    }
    emu_wave_sync();
}
