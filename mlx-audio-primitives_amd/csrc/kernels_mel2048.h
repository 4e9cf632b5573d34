// Fused mel-spectrogram for n_fft = 2048, the run kernel: 8 independent waves per CU, each wave
// one frame at a time in registers + its own LDS exchange buffer, output runs in registers.
//
// Same transform and contraction as ap_mel2048_wave_kernel (kernels_wave.h: 16 x 16 x 4 complex
// transform of the packed frame, paired real split, |X|^p plane, plan-based banded contraction),
// re-cut around what the round-2 measurements showed (profiles/README.md, tools/diag_clock.py,
// tools/power_probe.py):
//
//   * the chip runs this kernel at its POWER limit (1 340-1 355 W of board power, shader clock
//     2.2-2.35 GHz and falling whenever the pipes are kept busier): what shortens a launch is
//     less energy per frame - fewer instructions, fewer LDS and L2 bytes - not more waves (a
//     12-wave, 168-VGPR build spilled; alternating priorities between the co-resident waves
//     evened out their speeds and lowered the clock by the same factor);
//   * so everything frame-invariant is a template parameter or a register: the number of
//     contraction passes (NPASS), the hop class (HOPJ), (clip, frame) advanced incrementally
//     instead of a 64-bit division per frame, part descriptors as ready-made LDS addresses, rows
//     >= n_mels computed like the others and simply not stored, the window pairs and the split
//     twiddles of the lane in registers for the whole kernel (48 VGPRs: 16 LDS reads and 14
//     packed multiplies fewer per frame);
//   * the last radix-4 runs in registers, not across the quad: exchange #2 hands every lane four
//     whole radix-4 groups that are also each other's mirrors (g and 256 - g), so the radix-4s and
//     the paired real split take the lane's 16 bins without another LDS round trip - 32 packed adds
//     and 8 selects instead of the 64 v_fmac_f32_dpp, 32 v_cndmask and the s_nop pads of the DPP
//     quad stage (apm_quad8), and 8 ds_read_b128 instead of 17 ds_read_b64 for the split;
//   * the two twiddle tables are one row per lane (apm_fill_tables): eight and six aligned
//     ds_read_b128 per frame instead of 15 paired 8-byte reads each at half the LDS rate;
//   * no twiddle is a complex multiply of its own: the W16 constants inside both radix-16s, the W_1024
//     twiddles (applied by the lane that READS exchange #1) and the W_64 twiddles (read side of exchange
//     #2, none for input a = 0) are FMA addends of the butterfly level that consumes them (fft_lds.h,
//     "twiddles folded into the butterfly"): 30 packed instructions fewer per frame;
//   * the 8-frame output run of a lane's two mel rows lives in registers (32 contiguous bytes per
//     row and lane, as in ap_mel1024_wave_kernel): no output tile in LDS; the partial sums
//     alias the idle upper half of the wave's exchange buffer;
//   * with hop 512 the filterbank is contracted for two frames at a time (PAIR, below at the kernel): the
//     weight quads, the same for every frame, are read once per pair, and the two partial sums of a slot
//     travel as 8 bytes - 10.6 LDS instructions and 23 LDS-array cycles fewer per frame (profiles/README.md
//     "Round 7"); the window table is gone from LDS, the window pairs live in registers.
//
// Serves constant padding / center=False, power 2 or 1, n_mels <= 128, plans of <= 256 entries
// whose rows have <= 4 parts; everything else stays on ap_mel2048_wave_kernel.
// Reference: mel.py:245-352 (stft.py:130 + mel.py:344-350).
#pragma once
#include <type_traits>
#include "kernels_wave.h"

#define APM_WAVES 8           // waves per workgroup (2 per SIMD, 256 VGPRs each)
#define APM_RUN 8             // frames per output run held in registers
#define APM_PARTIAL_OFF 1152  // float offset of the partial sums inside the wave's X buffer (plane: 1025 floats)

// Which frame-invariant per-lane tables stay in REGISTERS for the whole kernel instead of being
// re-read from LDS every frame (bit mask; 8 waves per CU leave 256 VGPRs per lane).  The product
// uses APM_REGS: with the two twiddle tables as well hipcc's scheduler spills inside the frame loop.
#define APM_REG_WIN 1         // window pairs                 32 VGPRs, saves 16 ds_read_b64 per frame
#define APM_REG_TW1 2         // W_1024^((4 i + a) k) row     32 VGPRs, saves 8 ds_read_b128
#define APM_REG_TW2 4         // W_64^(a c) of the 4 groups   24 VGPRs, saves 6 ds_read_b128
#define APM_REG_SPLIT 8       // W_2048^k / 2 of the 8 split pairs, 16 VGPRs (always in registers: apm_split;
                              // the bit stays in APM_REGS so that the instantiations keep their names)
#define APM_REGS (APM_REG_WIN | APM_REG_SPLIT)

// Exchange #2 holds the second radix-16's outputs grouped by the last radix-4: the 4 inputs a of
// group g = k1 + 16 c (outputs Z[g + 256 q]) are 32 contiguous bytes at complex slot apm_gidx(g), with
// 16 bytes of padding after every 8 groups: the 16 ds_write_b64 of a frame are conflict-free and the
// 8 ds_read_b128 take 48 bank cycles (ideal 32; tools/lds_banks.py).  Largest slot 1085 < APW_X_COMPLEX.
AP_DEV int apm_gidx(int g) { return 4 * g + 2 * (g >> 3); }

// Lane layout of the in-register radix-4 + split: the lane with index L takes the groups L, L + 64,
// 192 - L, 256 - L (L = 0: 0, 64, 192, 128) - g pairs with 256 - g, as bin k = g + 256 q mirrors to
// 1024 - k = (256 - g) + 256 (3 - q), so the split of all 16 bins happens in the lane's registers.
// L is the lane permuted within its half: the four 16-lane sets of a ds_read_b128 ({0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31}, + 32) then read 16 consecutive groups each, which the padding above serves with
// at most 2-way conflicts; every |X|^p store still covers 32 consecutive bins per half-wave.
struct ApmPairLane {
    int L, lp;           // the lane's index, and L or 128 (L = 0) for pairs 2 and 3
    bool l0;             // L == 0: groups 0 and 128 pair with themselves, bin 512 on its own
    int rd[4];           // exchange slots of the lane's four groups
};

AP_DEV ApmPairLane apm_pair_lane_init(int lane) {
    ApmPairLane p;
    p.L = apm_lane_index(lane);                    // 0,16,20,4,24,8,12,28 (kernels_wave.h)
    p.l0 = p.L == 0;
    p.lp = p.l0 ? 128 : p.L;
    p.rd[0] = apm_gidx(p.L);
    p.rd[1] = apm_gidx(p.L + 64);
    p.rd[2] = apm_gidx(192 - p.L);
    p.rd[3] = apm_gidx(256 - p.lp);
    return p;
}

// forward transform of apw_forward up to exchange #2; the W_64 twiddles and the last radix-4 are left to
// apm_split, the exchange hands it whole groups.  Both twiddle multiplies ride on the butterfly level that
// consumes them (fft_lds.h): the values cross the exchanges untwiddled, the reading lane 4 k + a takes
// W_1024^((4 i + a) k) of element i into the first level of the second radix-16 (8 pairs of 5 instructions
// for 30 + 16), and the W16 twiddles inside both radix-16s sit in their second levels (finish_fused).
// tw1row / tw2row: the lane's rows of the two twiddle tables (apm_fill_tables), 16-byte aligned: eight and six
// ds_read_b128.  t2: the lane's W_64 twiddles for apm_split, read here ahead of the stores of exchange #2
// (with the reads of exchange #1, live across the second radix-16, three instantiations spilled).
#ifdef AP_PACKED_COMPLEX
// (as vector loads: read through the ap_float4 struct the four floats become a chain of scalar loads)
typedef float apm_float4v __attribute__((ext_vector_type(4)));
template <int N>
AP_DEV void apm_load_row(const ap_float2 *row, ap_float2 (&t)[N]) {
    const apm_float4v *src = reinterpret_cast<const apm_float4v *>(row);
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
        const apm_float4v v = src[j];
        t[2 * j] = __builtin_shufflevector(v, v, 0, 1);
        t[2 * j + 1] = __builtin_shufflevector(v, v, 2, 3);
    }
}
#else
template <int N>
AP_DEV void apm_load_row(const ap_float2 *row, ap_float2 (&t)[N]) {
    const ap_float4 *src = reinterpret_cast<const ap_float4 *>(row);
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
        const ap_float4 v = src[j];
        t[2 * j] = ap_mk(v.x, v.y);
        t[2 * j + 1] = ap_mk(v.z, v.w);
    }
}
#endif
// (the samples x and the window pairs w go in separately: the window rides on the first butterfly level)
template <int REGS>
AP_DEV void apm_forward(const ap_float2 (&x)[16], const ap_float2 (&w)[16], ap_float2 *X, const ap_float2 *tw1row,
                        const ap_float2 *tw2row, const ap_float2 (&t1r)[16], const ap_float2 (&t2r)[12],
                        ap_float2 (&t2)[12], const ApwLane &c) {
    const int lane = c.lane;
    ap_float2 v[16], t1[16];
    if (REGS & APM_REG_TW1) {
#pragma unroll
        for (int i = 0; i < 16; ++i) t1[i] = t1r[i];
    } else {
        apm_load_row(tw1row, t1);
    }
    ApButterfly<16>::run_weighted_fused(x, w, v);
    {
        const int a = lane & 3, bq = lane >> 2;
#pragma unroll
        for (int k = 0; k < 16; ++k) X[APW_T1(k * 4 + a) + bq] = v[k];
    }
    AP_WAVE_SYNC();
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = X[APW_T1(lane) + i];
    AP_WAVE_SYNC();
    ApButterfly<16>::run_twiddled_fused(v, t1, v);
    if (REGS & APM_REG_TW2) {
#pragma unroll
        for (int i = 0; i < 12; ++i) t2[i] = t2r[i];
    } else {
        apm_load_row(tw2row, t2);
    }
    // exchange #2: v[cc] is input a = lane & 3 of group k1 + 16 cc (apm_gidx(k1 + 16 cc) = apm_gidx(k1) + 68 cc)
    const int wb = apm_gidx(c.k1p) + (lane & 3);
#pragma unroll
    for (int cc = 0; cc < 16; ++cc) X[wb + 68 * cc] = v[cc];
    AP_WAVE_SYNC();
}

// The lane's four groups out of the exchange, their radix-4s with the W_64^(a c) twiddles of the inputs
// a = 1..3 folded into the first level (ap_fft4_twiddled3: 12 instructions a group for 6 + 8; t2[3 s + a - 1],
// row of apm_fill_tables) and the eight paired real splits of apw_split, all in registers; |X|^p of the 16
// bins (and bin 512 on lane L = 0) into the plane pp, which aliases X.
// wsp[i]: W_2048^k / 2 of pair i (apm_split_twiddles).
//   pair   0      1        2         3         4         5         6         7
//   k      L      L + 256  512 - lp  256 - lp  L + 64    L + 320   448 - L   192 - L
AP_DEV void apm_pair_bins(const ApmPairLane &p, int (&k)[8]) {
    k[0] = p.L; k[1] = p.L + 256; k[2] = 512 - p.lp; k[3] = 256 - p.lp;
    k[4] = p.L + 64; k[5] = p.L + 320; k[6] = 448 - p.L; k[7] = 192 - p.L;
}

AP_DEV void apm_split_twiddles(const ApmPairLane &p, const ap_float2 *tw, ap_float2 (&wsp)[8]) {
    int k[8];
    apm_pair_bins(p, k);
#pragma unroll
    for (int i = 0; i < 8; ++i) wsp[i] = ap_scale(tw[k[i]], 0.5f);
}

// POFF: constant float offset of the plane from pp (the mel kernel's parking plane: the stores then share
// the address registers of the plane in the exchange buffer, the distance is an instruction offset)
template <int PMODE, int POFF = 0>
AP_DEV void apm_split(const ap_float2 *X, float *pp, const ApmPairLane &p, const ap_float2 (&wsp)[8],
                      const ap_float2 (&t2)[12], const ApwLane &c, float power) {
    ap_float2 z[4][4];                    // z[s][q] = Z[g_s + 256 q] after the radix-4s
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const ap_float4 *src = reinterpret_cast<const ap_float4 *>(X + p.rd[s]);
        const ap_float4 lo = src[0], hi = src[1];
        z[s][0] = ap_mk(lo.x, lo.y); z[s][1] = ap_mk(lo.z, lo.w);
        z[s][2] = ap_mk(hi.x, hi.y); z[s][3] = ap_mk(hi.z, hi.w);
    }
    AP_WAVE_SYNC();
#pragma unroll
    for (int s = 0; s < 4; ++s)
        ap_fft4_twiddled3(z[s][0], z[s][1], t2[3 * s], z[s][2], t2[3 * s + 1], z[s][3], t2[3 * s + 2]);
    // (Z[k], Z[1024 - k]) of the eight pairs; L = 0: (Z0, Z0), (Z256, Z768), (Z384, Z640), (Z128, Z896)
    const ap_float2 zk[8] = {z[0][0], z[0][1], z[3][1], z[3][0], z[1][0], z[1][1], z[2][1], z[2][0]};
    const ap_float2 zm[8] = {p.l0 ? z[0][0] : z[3][3], p.l0 ? z[0][3] : z[3][2], p.l0 ? z[3][2] : z[0][2],
                             p.l0 ? z[3][3] : z[0][3], z[2][3], z[2][2], z[1][2], z[1][3]};
    int k[8];
    apm_pair_bins(p, k);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const ap_float2 a = ap_add_conj(zk[i], zm[i]);
        const ap_float2 d = ap_sub_conj(zk[i], zm[i]);
        const ap_float2 u = ap_mul_fw(d, wsp[i]);
        const ap_float2 xk = ap_fma_add_mi(a, c.half, u);
        const ap_float2 xm = ap_fma_sub_mi(a, c.half, u);
        pp[k[i] + POFF] = apw_pow2x<PMODE>(xk.x, xk.y, power);
        pp[APW_NC - k[i] + POFF] = apw_pow2x<PMODE>(xm.x, xm.y, power);
    }
    if (p.l0) pp[APW_NC / 2 + POFF] = apw_pow2x<PMODE>(z[0][2].x, z[0][2].y, power);   // X[512] = conj Z[512]
}

#ifdef AP_DIAG_STAMPS
// Diagnostic build only (tools/diag_clock.py; buffer in kernels_wave.h)
#define AP_DIAG_BEGIN() unsigned long long ap_dt0, ap_dr0; \
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(ap_dt0), "=s"(ap_dr0)::"memory")
#define AP_DIAG_END(widx) do { unsigned long long ap_dt1, ap_dr1; \
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(ap_dt1), "=s"(ap_dr1)::"memory"); \
    if ((threadIdx.x & 63) == 0 && (widx) < 256 * 16) { ap_diag_stamps[4 * (widx)] = ap_dt1 - ap_dt0; ap_diag_stamps[4 * (widx) + 1] = ap_dr1 - ap_dr0; ap_diag_stamps[4 * (widx) + 2] = ap_dr0; ap_diag_stamps[4 * (widx) + 3] = ap_dr1; } } while (0)
#else
#define AP_DIAG_BEGIN() do {} while (0)
#define AP_DIAG_END(widx) do {} while (0)
#endif

// The two (three) waves of a SIMD do not share it evenly: issue is arbitrated by priority, then AGE,
// so the first-dispatched wave of every SIMD ran its 54 frames in 144 us and the second in 186 us
// (tools/diag_clock.py), and the kernel lasts as long as the slow one.  The later-dispatched waves
// therefore raise their priority on every other frame: over two frames each side wins once, all
// waves finish together and the SIMDs stay shared until the end.  (At the power limit this buys
// nothing by itself - the clock drops as the SIMDs stay busier - but it keeps the tail short
// whenever the kernel is not power-bound: short batches, cooler boards.)
#ifdef AP_HOST_EMU
#define AP_FAIR_SHARE(wave, nw, f) do {} while (0)
#else
#define AP_FAIR_SHARE(wave, nw, f)                                   \
    do {                                                             \
        if ((wave) >= (nw) / 2 + ((nw) > 8 ? 2 : 0)) {               \
            if ((f) & 1) __builtin_amdgcn_s_setprio(1);              \
            else __builtin_amdgcn_s_setprio(0);                      \
        } else if ((nw) > 8 && (wave) >= 4) {                        \
            if ((f) & 1) __builtin_amdgcn_s_setprio(0);              \
            else __builtin_amdgcn_s_setprio(1);                      \
        }                                                            \
    } while (0)
#endif

// 16 bytes of a plane or of the weight table as ONE vector load (read through the ap_float4 struct the pair
// contraction's quads came out as ds_read2_b32 halves)
#ifdef AP_PACKED_COMPLEX
AP_DEV ap_float4 apm_load4(const ap_float4 *p) {
    const apm_float4v v = *reinterpret_cast<const apm_float4v *>(p);
    ap_float4 r;
    r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w;
    return r;
}
#else
AP_DEV ap_float4 apm_load4(const ap_float4 *p) { return *p; }
#endif

// PAIR (hop 512 only; the launcher picks it wherever ap_prepare_mel_run found room, P.pair): the filterbank is
// contracted for two frames at a time.  The four frame bodies of a loop trip are two pairs (rotations 0-1 and
// 2-3): the frames of the even rotations leave their |X|^p plane in the wave's parking area (APM_PARK_COMPLEX,
// right behind the exchange buffer), those of the odd rotations in the exchange buffer as ever, and one
// contraction reads every weight quad once for both planes, runs the FMA chains of each frame in the order of
// the single-frame contraction, and moves the two partial sums of a slot as one 8-byte store and one 8-byte
// load.  A pair needs its second frame in the same clip and stretch; a stretch that enters at an odd rotation,
// a clip end or a stretch end on the first frame of a pair take the single-frame contraction (of the parked
// plane, for an even rotation) - every frame gets the same bits on either path.  With PAIR the partial-sum
// slots are 8 bytes apart on both paths (one set of slot addresses).  The launcher (audioprims.hip) is the one
// place that picks PAIR, from P.pair; the default is what the CPU emulator's launcher instantiates, and the emulator
// build stops a launch whose carve-up is for the other value.  Every plan of ap_mel_plan_host (<= 4 passes of 256
// weight quads, <= 512 slots) leaves room for the parking planes: the PAIR = 0 twin of a hop-512 instantiation
// serves caller-made plans only.
template <int PMODE, int NPASS, int HOPJ, int IN16 = 0, int NW = APM_WAVES, int REGS = APM_REGS, int PAIR = (HOPJ == 4)>
__global__ void __launch_bounds__(64 * NW, NW / 4) ap_mel2048_run_kernel(ApMelWaveParams P) {
    static_assert(IN16 != 1 || (REGS & APM_REG_WIN), "the PCM scale rides on the register-resident window");
    static_assert(APM_MEL_WIN_LDS || (REGS & APM_REG_WIN), "ap_prepare_mel_run leaves no room for a window table");
    static_assert(!PAIR || HOPJ == 4, "pairs are two of the four rotations of the hop-512 loop");
    constexpr int XS = APW_X_COMPLEX + (PAIR ? APM_PARK_COMPLEX : 0);     // complex slots between the waves' buffers
    constexpr int SS = PAIR ? 2 : 1;                                      // floats between two partial-sum slots
    static_assert(2 * APM_PARK_COMPLEX >= 4 * (APW_NC / 4 + 4), "groups 256 .. 259: the contraction's read-ahead");
#ifdef AP_HOST_EMU
    // the emulator's launcher instantiates the default PAIR: the LDS carve-up must be the one for it
    if ((PAIR != 0) != (P.pair != 0)) { fprintf(stderr, "ap_mel2048_run_kernel: PAIR = %d on a carve-up for pair = %d\n", PAIR, P.pair); abort(); }
#endif
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = AP_UNIFORM(tid >> 6);
    ap_float2 *X = reinterpret_cast<ap_float2 *>(ap_smem) + wave * XS;
    ap_float2 *TW2 = reinterpret_cast<ap_float2 *>(ap_smem + P.off_tw2);               // [64][14]
    const ap_float2 *TW1 = reinterpret_cast<const ap_float2 *>(ap_smem + P.off_tw1);   // [64][18]
    const ap_float2 *WIN = reinterpret_cast<const ap_float2 *>(ap_smem + P.off_win);   // [1024] pairs
    const ap_float4 *WQ = reinterpret_cast<const ap_float4 *>(ap_smem + P.off_wq);     // [n_quads]
    float *pp = reinterpret_cast<float *>(X);                 // |X|^p plane of this wave (floats 0..1024)
    float *partial = pp + APM_PARTIAL_OFF;                    // partial sums: idle part of X during the contraction
    const int M = P.n_mels;

    // ---------------- workgroup tables in LDS (once; the only workgroup barrier) ------
    {
        const int nt = 64 * NW;
        ap_float4 *wq = reinterpret_cast<ap_float4 *>(ap_smem + P.off_wq);
        for (int i = tid; i < P.n_quads; i += nt) wq[i] = reinterpret_cast<const ap_float4 *>(P.quads)[i];
        apm_fill_tables(TW2, reinterpret_cast<ap_float2 *>(ap_smem + P.off_tw1),
                        (REGS & APM_REG_WIN) ? nullptr : reinterpret_cast<ap_float2 *>(ap_smem + P.off_win),
                        P.tw, P.window, tid, nt);
    }
    AP_LDS_BARRIER();
    const ApwLane lc = apw_lane_init(lane, TW2, P.tw, APM_TW_ROW);
    const ApmPairLane pl = apm_pair_lane_init(lane);
    // per-lane tables kept in registers (REGS): straight from the global tables
    ap_float2 winr[16], t1r[16], t2r[12], wsp[8];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        winr[j] = (REGS & APM_REG_WIN) ? reinterpret_cast<const ap_float2 *>(P.window)[lane + 64 * j] : ap_mk(0.0f, 0.0f);
        if (IN16 == 1) winr[j] = ap_scale(winr[j], 1.0f / 32768.0f);      // 16-bit PCM -> [-1, 1): folded into the window
        t1r[j] = (REGS & APM_REG_TW1) ? P.tw[2 * (4 * j + (lane & 3)) * (lane >> 2)] : ap_mk(0.0f, 0.0f);
        if (j < 12)
            t2r[j] = (REGS & APM_REG_TW2) ? P.tw[32 * (j % 3 + 1) * (apm_lane_group(pl.L, j / 3) >> 4)] : ap_mk(0.0f, 0.0f);
    }
    apm_split_twiddles(pl, P.tw, wsp);
    // frame-invariant contraction state: LDS addresses of this lane's entries
    const ap_float4 *pqa[NPASS], *pqb[NPASS];
    float *sa[NPASS], *sb[NPASS];
    float fz[NPASS];
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
        const int pi = lane + 64 * ps;
        ap_int4 pd;
        pd.x = P.n_slots; pd.y = 0; pd.z = P.n_slots; pd.w = 0;          // idle entry: zero weights, dump slot
        if (pi < P.n_parts) pd = reinterpret_cast<const ap_int4 *>(P.parts)[pi];
        pqa[ps] = reinterpret_cast<const ap_float4 *>(pp) + pd.y;
        pqb[ps] = reinterpret_cast<const ap_float4 *>(pp) + pd.w;
        sa[ps] = partial + SS * pd.x;
        sb[ps] = partial + SS * (pd.z < 0 ? P.n_slots : pd.z);
        fz[ps] = pd.z < 0 ? 1.0f : 0.0f;                                  // one long part: both halves to slot A
    }
    // PAIR: the read-ahead of the parked plane (floats 1025 .. 2 APM_PARK_COMPLEX - 1) is never written in the
    // frame loop and is multiplied by zero weights: zero, once (in the exchange buffer these floats are the
    // wave's own exchange data, finite whenever its samples are)
    if (PAIR) {
        for (int i = APW_NC + 1 + lane; i < 2 * APM_PARK_COMPLEX; i += 64) pp[2 * APW_X_COMPLEX + i] = 0.0f;
    }
    int rs0[2], cnt[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = lane + 64 * i;
        rs0[i] = row < M ? P.rowstart[row] : 0;
        cnt[i] = row < M ? P.rowstart[row + 1] - rs0[i] : 0;
        rs0[i] *= SS;
    }
    AP_LDS_BARRIER();

    const int64_t worker = (int64_t)blockIdx.x * NW + wave;
    const int64_t n_workers = (int64_t)gridDim.x * NW;
    const int64_t n_frames = P.n_clips * P.T;
    const int64_t f_lo = n_frames * worker / n_workers, f_hi = n_frames * (worker + 1) / n_workers;
    const int Ti = (int)P.T;
    float vmax = -INFINITY;
    AP_DIAG_BEGIN();
    if (f_lo < f_hi) {
        int64_t b = f_lo / P.T;                   // the only division: (clip, frame) advance incrementally
        int t = (int)(f_lo - b * P.T);
        // IN16: P.y points at int16 samples (the ingest conversion rides on the
        // sample loads; half the HBM read bytes of the float32 path)
        const int16_t *y16 = reinterpret_cast<const int16_t *>(P.y);
        // IN16 == 2: float32 samples with reflect / edge padding (or odd hops): the frames that reach over a clip
        // end take the index-remapping loader, every other frame the bounds-checked loads
        ApClip clip = ap_clip_make(P.y + (IN16 == 1 ? 0 : b * P.L), IN16 == 1 ? 0 : P.L);
        ApClip16 clip16 = ap_clip16_make(y16 + (IN16 == 1 ? b * P.L : 0), IN16 == 1 ? P.L : 0);
        auto ld2 = [&](int64_t bb, int base, int p) __attribute__((always_inline)) -> ap_float2 {
            if (IN16 == 1) return ap_clip16_load2(clip16, p);
            if (IN16 == 2 && !(base >= 0 && (int64_t)base + 2 * APW_NC <= P.L)) {
                const float *yb = P.y + bb * P.L;
                return ap_mk(ap_load_padded(yb, P.L, p, P.pad_mode), ap_load_padded(yb, P.L, p + 1, P.pad_mode));
            }
            return ap_clip_load2(clip, p);
        };
        // Sample pair j of the frame in hand lives in raw[(j + HOPJ rot) & 15]: with hop = 128 HOPJ, pair j of
        // frame t + 1 is pair j + HOPJ of frame t, so the HOPJ new pairs of the next frame overwrite the HOPJ
        // oldest registers and nothing moves.  `rot` has to be a compile-time constant for that (registers
        // cannot be indexed), hence a loop trip of U = 16 / HOPJ frames, one copy of the body per rotation.
        // (The earlier form shifted the 12 surviving pairs every frame: 24 v_mov_b64, 5 % of the issue slots.)
        constexpr int U = HOPJ == 4 ? 4 : 1;
        ap_float2 raw[16];
        auto load_frame = [&](int tt, auto rot_tag) {
            constexpr int ROT = decltype(rot_tag)::value;
            const int base = tt * P.hop - P.pad;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int p = base + 2 * (lane + 64 * j);
                raw[(j + HOPJ * ROT) & 15] = ld2(b, base, p);
            }
        };
        // U = 4: the stretch's first frame takes the register rotation r0 = t mod 4 and the run half (t / 4) mod 2, so
        // that frame t sits at position t mod 8 of the run registers: full runs are then the clip's frames 8 k .. 8 k + 7
        // and leave as ALIGNED 32-byte pieces of their rows (rows `Ts` floats apart; with Ts a multiple of 8 the
        // pieces are whole sectors - the output's write amplification was 1.9 x with runs that started wherever the
        // stretch did).  A clip that ends inside the stretch breaks the alignment for the rest of it.
        const int r0 = U == 4 ? (t & 3) : 0;
        if (r0 == 1) load_frame(t, std::integral_constant<int, 1 % U>());
        else if (r0 == 2) load_frame(t, std::integral_constant<int, 2 % U>());
        else if (r0 == 3) load_frame(t, std::integral_constant<int, 3 % U>());
        else load_frame(t, std::integral_constant<int, 0>());
        // The run of finished frames (rows lane and lane + 64) waits in registers for a 32-byte store:
        // position p8 = 4 h + rot of an 8-frame cycle (U = 4: static register, uniform half h), or a
        // shift register (U = 1).
        float acc0[APM_RUN], acc1[APM_RUN];
#pragma unroll
        for (int i = 0; i < APM_RUN; ++i) { acc0[i] = 0.0f; acc1[i] = 0.0f; }
        int nrun = 0, half = U == 4 ? ((t >> 2) & 1) : 0;
        int64_t f = f_lo;

        // transform of the frame in hand, the loads of the next one and the |X|^p plane, poff_tag floats behind pp
        auto transform = [&](auto rot_tag, auto poff_tag, const bool clip_ends, const bool more) __attribute__((always_inline)) {
            constexpr int ROT = decltype(rot_tag)::value;
            constexpr int NROT = (ROT + 1) % U;
            AP_FAIR_SHARE(wave, NW, f);
            ap_float2 t2[12];                  // the lane's W_64 twiddles: read in apm_forward, used in apm_split
            {
                ap_float2 xs[16], ws[16];         // renamings: no instructions
#pragma unroll
                for (int j = 0; j < 16; ++j) xs[j] = raw[(j + HOPJ * ROT) & 15];
                if (REGS & APM_REG_WIN) {
#pragma unroll
                    for (int j = 0; j < 16; ++j) ws[j] = winr[j];
                } else {
#pragma unroll
                    for (int j = 0; j < 16; ++j) ws[j] = WIN[lane + 64 * j];
                }
                AP_SCHED_FENCE();
                apm_forward<REGS>(xs, ws, X, TW1 + APM_TW_ROW * lane, TW2 + APM_TW2_ROW * lane, t1r, t2r, t2, lc);
            }
            // The next frame of this wave's stretch, in flight during split + contraction
            AP_SCHED_FENCE();
            if (more) {
                if (clip_ends) {                  // next clip starts
                    if (IN16 == 1) clip16 = ap_clip16_make(y16 + (b + 1) * P.L, P.L);
                    else clip = ap_clip_make(P.y + (b + 1) * P.L, P.L);
                }
                // hop = 128 HOPJ: only the HOPJ new pairs are loaded, the shared samples stay where they are;
                // a new clip (and HOPJ = 0) loads the other pairs as well, into the same registers.  (One
                // code path on purpose: with the full load in a branch of its own the register allocator
                // copied all 12 surviving pairs out and back on every frame.)
                const int base = (clip_ends ? 0 : t + 1) * P.hop - P.pad;
#pragma unroll
                for (int j = 16 - HOPJ; j < 16; ++j) {
                    const int p = base + 2 * (lane + 64 * j);
                    raw[(j + HOPJ * NROT) & 15] = ld2(clip_ends ? b + 1 : b, base, p);
                }
                if (HOPJ == 0 || clip_ends) {
#pragma unroll
                    for (int j = 0; j < 16 - HOPJ; ++j) {
                        const int p = base + 2 * (lane + 64 * j);
                        raw[(j + HOPJ * NROT) & 15] = ld2(clip_ends ? b + 1 : b, base, p);
                    }
                }
            }
            AP_SCHED_FENCE();
            apm_split<PMODE, decltype(poff_tag)::value>(X, pp, pl, wsp, t2, lc, P.power);
            AP_WAVE_SYNC();
        };
        // the frame's row sums into the run registers, the run's store when it is due, and on to the next frame
        auto finish = [&](auto rot_tag, const float (&sum2)[2], const bool clip_ends, const bool more) __attribute__((always_inline)) {
            constexpr int ROT = decltype(rot_tag)::value;
            // the frame's position in the run registers, and the position of the run's first frame
            int pos;
            if (U == 1) {
#pragma unroll
                for (int i = 0; i < APM_RUN - 1; ++i) { acc0[i] = acc0[i + 1]; acc1[i] = acc1[i + 1]; }
                acc0[APM_RUN - 1] = sum2[0];
                acc1[APM_RUN - 1] = sum2[1];
                pos = APM_RUN - 1;
            } else {
                if (half) { acc0[4 + ROT] = sum2[0]; acc1[4 + ROT] = sum2[1]; }        // uniform branch
                else { acc0[ROT] = sum2[0]; acc1[ROT] = sum2[1]; }
                pos = 4 * half + ROT;
            }
            ++nrun;
            AP_WAVE_SYNC();
            // ---- store the run when it is full, the clip ends or the stretch ends ---------------
            if ((U == 1 ? nrun == APM_RUN : pos == APM_RUN - 1) || clip_ends || !more) {
                // frame t - nrun + 1 + g sits in register pos - nrun + 1 + g
                const int first = pos - nrun + 1;
                float *ob = P.out + b * (int64_t)M * P.Ts + (t - nrun + 1);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int row = lane + 64 * i;
                    if (row < M) {
                        float *dst = ob + (int64_t)row * P.Ts;
                        const float *src = i == 0 ? acc0 : acc1;
                        if (nrun == APM_RUN) {      // 32 contiguous bytes: two 16-byte stores (4-byte aligned)
                            ap_rsp_f4u lo, hi;
                            lo.x = src[0]; lo.y = src[1]; lo.z = src[2]; lo.w = src[3];
                            hi.x = src[4]; hi.y = src[5]; hi.z = src[6]; hi.w = src[7];
                            *reinterpret_cast<ap_rsp_f4u *>(dst) = lo;
                            *reinterpret_cast<ap_rsp_f4u *>(dst + 4) = hi;
                        } else {
#pragma unroll
                            for (int g = 0; g < APM_RUN; ++g)
                                if (g >= first && g <= pos) dst[g - first] = src[g];
                        }
                    }
                }
                nrun = 0;
            }
            if (clip_ends) { t = 0; ++b; } else { ++t; }
            ++f;
        };
        constexpr int PARKQ = 2 * APW_X_COMPLEX / 4;              // 16-byte groups from a plane to its parking twin
        static_assert(2 * APW_X_COMPLEX % 4 == 0 && (APW_X_COMPLEX + APM_PARK_COMPLEX) % 2 == 0, "16-byte aligned planes");
        // ---- plan-based contraction of one frame: NPASS branch-free passes (kernels_wave.h), then the row sums
        // (<= 4 adjacent slots per row).  PQ: 0 = the plane in the exchange buffer, PARKQ = the parked one
        auto contract = [&](auto pq_tag, float (&sum2)[2]) __attribute__((always_inline)) {
            constexpr int PQ = decltype(pq_tag)::value;
#pragma unroll
            for (int ps = 0; ps < NPASS; ++ps) {
                const ap_float4 *wq = WQ + 256 * ps + lane;
                ap_float4 w[4], q[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) w[i] = wq[64 * i];
                q[0] = pqa[ps][PQ]; q[1] = pqa[ps][PQ + 1]; q[2] = pqb[ps][PQ]; q[3] = pqb[ps][PQ + 1];
                float acc[2] = {0.0f, 0.0f};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[i >> 1] = fmaf(w[i].x, q[i].x, acc[i >> 1]);
                    acc[i >> 1] = fmaf(w[i].y, q[i].y, acc[i >> 1]);
                    acc[i >> 1] = fmaf(w[i].z, q[i].z, acc[i >> 1]);
                    acc[i >> 1] = fmaf(w[i].w, q[i].w, acc[i >> 1]);
                }
                *sa[ps] = fmaf(fz[ps], acc[1], acc[0]);
                *sb[ps] = acc[1];
            }
            AP_WAVE_SYNC();
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float p0 = partial[rs0[i]], p1 = partial[rs0[i] + SS], p2 = partial[rs0[i] + 2 * SS],
                            p3 = partial[rs0[i] + 3 * SS];
                float sum = cnt[i] > 0 ? p0 : 0.0f;
                sum += cnt[i] > 1 ? p1 : 0.0f;
                sum += cnt[i] > 2 ? p2 : 0.0f;
                sum += cnt[i] > 3 ? p3 : 0.0f;
                sum2[i] = sum;
                vmax = fmaxf(vmax, cnt[i] > 0 ? sum : vmax);
            }
        };
        // ---- the same for the two frames of a pair (parked plane -> sum0, exchange buffer -> sum1): every weight
        // quad is read once, each frame's FMA chains run in the order of `contract`, slot s holds (first, second)
        auto contract_pair = [&](float (&sum0)[2], float (&sum1)[2]) __attribute__((always_inline)) {
#pragma unroll
            for (int ps = 0; ps < NPASS; ++ps) {
                const ap_float4 *wq = WQ + 256 * ps + lane;
                ap_float4 w[4], q0[4], q1[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) w[i] = apm_load4(wq + 64 * i);
                q0[0] = apm_load4(pqa[ps] + PARKQ); q0[1] = apm_load4(pqa[ps] + PARKQ + 1);
                q0[2] = apm_load4(pqb[ps] + PARKQ); q0[3] = apm_load4(pqb[ps] + PARKQ + 1);
                q1[0] = apm_load4(pqa[ps]); q1[1] = apm_load4(pqa[ps] + 1);
                q1[2] = apm_load4(pqb[ps]); q1[3] = apm_load4(pqb[ps] + 1);
                // (AP_PIN on the second frame's accumulators: left alone, the SLP vectoriser pairs the two frames'
                // chains into v_pk_fma_f32 whose operands - one value of each plane, out of different ds_read_b128 -
                // first have to be moved next to each other: 88 v_mov_b32 and 48 packed FMAs for 96 plain ones)
                // (the same holds for the two fz products, which as a packed FMA keep a second copy of fz[ps] in
                // registers for the whole kernel: the first frame's result is pinned before the second frame's chain ends)
                float a0[2] = {0.0f, 0.0f}, a1[2] = {0.0f, 0.0f};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a0[i >> 1] = fmaf(w[i].x, q0[i].x, a0[i >> 1]);
                    a0[i >> 1] = fmaf(w[i].y, q0[i].y, a0[i >> 1]);
                    a0[i >> 1] = fmaf(w[i].z, q0[i].z, a0[i >> 1]);
                    a0[i >> 1] = fmaf(w[i].w, q0[i].w, a0[i >> 1]);
                    a1[i >> 1] = fmaf(w[i].x, q1[i].x, a1[i >> 1]); AP_PIN(a1[i >> 1]);
                    a1[i >> 1] = fmaf(w[i].y, q1[i].y, a1[i >> 1]); AP_PIN(a1[i >> 1]);
                    a1[i >> 1] = fmaf(w[i].z, q1[i].z, a1[i >> 1]); AP_PIN(a1[i >> 1]);
                    if (i < 3) { a1[i >> 1] = fmaf(w[i].w, q1[i].w, a1[i >> 1]); AP_PIN(a1[i >> 1]); }
                }
                float s0 = fmaf(fz[ps], a0[1], a0[0]);
                AP_PIN(s0);
                a1[1] = fmaf(w[3].w, q1[3].w, a1[1]); AP_PIN(a1[1]);
                *reinterpret_cast<ap_float2 *>(sa[ps]) = ap_mk(s0, fmaf(fz[ps], a1[1], a1[0]));
                *reinterpret_cast<ap_float2 *>(sb[ps]) = ap_mk(a0[1], a1[1]);
            }
            AP_WAVE_SYNC();
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const ap_float2 *pr = reinterpret_cast<const ap_float2 *>(partial + rs0[i]);
                const ap_float2 p0 = pr[0], p1 = pr[1], p2 = pr[2], p3 = pr[3];
                float s0 = cnt[i] > 0 ? p0.x : 0.0f, s1 = cnt[i] > 0 ? p0.y : 0.0f;
                s0 += cnt[i] > 1 ? p1.x : 0.0f; s1 += cnt[i] > 1 ? p1.y : 0.0f;
                s0 += cnt[i] > 2 ? p2.x : 0.0f; s1 += cnt[i] > 2 ? p2.y : 0.0f;
                s0 += cnt[i] > 3 ? p3.x : 0.0f; s1 += cnt[i] > 3 ? p3.y : 0.0f;
                sum0[i] = s0; sum1[i] = s1;
                vmax = fmaxf(vmax, cnt[i] > 0 ? fmaxf(s0, s1) : vmax);
            }
        };
        // one frame; returns false after the last frame of the stretch.  PAIR: the frames of the even rotations
        // always leave their plane in the parking area; where the next frame belongs to the same clip and stretch
        // (`paired`, uniform) they stop there and the odd rotation's body contracts both frames at once.
        bool paired = false;
        auto frame = [&](auto rot_tag) __attribute__((always_inline)) -> bool {
            constexpr int ROT = decltype(rot_tag)::value;
            constexpr bool FIRST = PAIR && ROT % 2 == 0;
            const bool clip_ends = t + 1 == Ti;
            const bool more = f + 1 < f_hi;
            transform(rot_tag, std::integral_constant<int, FIRST ? 4 * PARKQ : 0>(), clip_ends, more);
            float sum2[2];
            if (FIRST) {
                paired = !clip_ends && more;
                // (paired: `finish` books the frame with row sums that the second frame's body overwrites before any
                // store - the frame neither fills a run nor ends anything; an early return here instead cost 12 VGPRs)
                sum2[0] = sum2[1] = 0.0f;
                if (!paired) contract(std::integral_constant<int, PARKQ>(), sum2);
            } else if (PAIR && paired) {
                float sum0[2];
                contract_pair(sum0, sum2);
                if (half) { acc0[4 + (ROT + 3) % 4] = sum0[0]; acc1[4 + (ROT + 3) % 4] = sum0[1]; }   // uniform branch
                else { acc0[(ROT + 3) % 4] = sum0[0]; acc1[(ROT + 3) % 4] = sum0[1]; }
                paired = false;
            } else {
                contract(std::integral_constant<int, 0>(), sum2);
            }
            finish(rot_tag, sum2, clip_ends, more);
            return more;
        };
        if (U == 1) {
            while (frame(std::integral_constant<int, 0>())) {}
        } else {
            int skip = r0;                        // the first trip enters at rotation r0 (uniform branches)
            for (;;) {
                if (skip <= 0 && !frame(std::integral_constant<int, 0>())) break;
                if (skip <= 1 && !frame(std::integral_constant<int, 1 % U>())) break;
                if (skip <= 2 && !frame(std::integral_constant<int, 2 % U>())) break;
                if (!frame(std::integral_constant<int, 3 % U>())) break;
                skip = 0;
                half ^= 1;
            }
        }
    }
    AP_DIAG_END((int)worker);
    if (P.max_key) {                  // one atomic per wave: lanes -> LDS -> lane 0
        AP_WAVE_SYNC();
        partial[lane] = vmax;
        AP_WAVE_SYNC();
        if (lane == 0) {
            float m = partial[0];
            for (int i = 1; i < 64; ++i) m = fmaxf(m, partial[i]);
            ap_atomic_max_u32(P.max_key, ap_fkey(m));
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Spectral centroid / bandwidth / rolloff / flatness of every frame straight from the audio, n_fft = 2048
// (reference features.py:57-442: an STFT, |.|, |.|^p and sum / cumsum / argmax chains per call).  The
// transform, the paired split and the |X|^p plane are those of the mel run kernel above; instead of the
// filterbank contraction the wave reduces its frame's 1025 plane values: lane l owns the 16 contiguous
// bins 16 l .. 16 l + 15 (lane 63 bin 1024 as well), sums them, and the 64 lane sums are combined with
// wave shuffles; the rolloff lane is found from an exclusive scan of the lane sums.  Nothing but the
// samples is read from HBM and 4-16 bytes per frame are written: the complex spectrum (8.2 KB per frame,
// written and read back by the two-kernel route of kernels_features.h) never exists.
// ---------------------------------------------------------------------------------------------
#ifdef AP_HOST_EMU
AP_DEV float apm_lane_xor(float x, int mask) { return emu_lane_xor(x, mask); }
AP_DEV float apm_lane_up(float x, int d, int lane) { return emu_lane_perm(x, lane - d); }
#else
AP_DEV float apm_lane_xor(float x, int mask) { return __shfl_xor(x, mask, 64); }
AP_DEV float apm_lane_up(float x, int d, int lane) { return __shfl_up(x, d, 64); }
#endif
AP_DEV float apm_wave_sum(float x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += apm_lane_xor(x, off);
    return x;
}

// FLAT: flatness wanted (17 logs per lane and frame); PGEN: bandwidth exponent p != 2 (powf in the loop -
// a template flag so that the usual p = 2 build stays inside the instruction cache)
template <int PMODE, int HOPJ, int FLAT, int PGEN = 0, int NW = APM_WAVES, int REGS = APM_REGS>
__global__ void __launch_bounds__(64 * NW, NW / 4) ap_spec2048_run_kernel(ApSpecWaveParams P) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = AP_UNIFORM(tid >> 6);
    ap_float2 *X = reinterpret_cast<ap_float2 *>(ap_smem) + wave * APW_X_COMPLEX;
    ap_float2 *TW2 = reinterpret_cast<ap_float2 *>(ap_smem + P.off_tw2);
    const ap_float2 *TW1 = reinterpret_cast<const ap_float2 *>(ap_smem + P.off_tw1);
    const ap_float2 *WIN = reinterpret_cast<const ap_float2 *>(ap_smem + P.off_win);
    float *pp = reinterpret_cast<float *>(X);                 // |X|^p plane of this wave (floats 0..1024)
    apm_fill_tables(TW2, reinterpret_cast<ap_float2 *>(ap_smem + P.off_tw1),
                    reinterpret_cast<ap_float2 *>(ap_smem + P.off_win), P.tw, P.window, tid, 64 * NW);
    AP_LDS_BARRIER();
    const ApwLane lc = apw_lane_init(lane, TW2, P.tw, APM_TW_ROW);
    const ApmPairLane pl = apm_pair_lane_init(lane);
    ap_float2 winr[16], t1r[16], t2r[12], wsp[8];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        winr[j] = (REGS & APM_REG_WIN) ? reinterpret_cast<const ap_float2 *>(P.window)[lane + 64 * j] : ap_mk(0.0f, 0.0f);
        t1r[j] = (REGS & APM_REG_TW1) ? P.tw[2 * (4 * j + (lane & 3)) * (lane >> 2)] : ap_mk(0.0f, 0.0f);
        if (j < 12)
            t2r[j] = (REGS & APM_REG_TW2) ? P.tw[32 * (j % 3 + 1) * (apm_lane_group(pl.L, j / 3) >> 4)] : ap_mk(0.0f, 0.0f);
    }
    apm_split_twiddles(pl, P.tw, wsp);
    float fk[17];                                             // bin centres of this lane's bins
#pragma unroll
    for (int i = 0; i < 16; ++i) fk[i] = P.freq[16 * lane + i];
    fk[16] = lane == 63 ? P.freq[APW_NC] : 0.0f;
    AP_LDS_BARRIER();

    const int64_t worker = (int64_t)blockIdx.x * NW + wave;
    const int64_t n_workers = (int64_t)gridDim.x * NW;
    const int64_t n_frames = P.n_clips * P.T;
    const int64_t f_lo = n_frames * worker / n_workers, f_hi = n_frames * (worker + 1) / n_workers;
    const int Ti = (int)P.T;
    if (f_lo >= f_hi) return;
    int64_t b = f_lo / P.T;
    int t = (int)(f_lo - b * P.T);
    ApClip clip = ap_clip_make(P.y + b * P.L, P.L);
    constexpr int U = HOPJ == 4 ? 4 : 1;                      // see ap_mel2048_run_kernel
    ap_float2 raw[16];
    auto load_frame = [&](int tt, auto rot_tag) {
        constexpr int ROT = decltype(rot_tag)::value;
        const int base = tt * P.hop - P.pad;
#pragma unroll
        for (int j = 0; j < 16; ++j) raw[(j + HOPJ * ROT) & 15] = ap_clip_load2(clip, base + 2 * (lane + 64 * j));
    };
    load_frame(t, std::integral_constant<int, 0>());
    int64_t f = f_lo;
    const float F_all = (float)(APW_NC + 1);

    auto frame = [&](auto rot_tag) -> bool {
        constexpr int ROT = decltype(rot_tag)::value;
        constexpr int NROT = (ROT + 1) % U;
        const bool clip_ends = t + 1 == Ti;
        const bool more = f + 1 < f_hi;
        ap_float2 t2[12];
        {
            ap_float2 xs[16], ws[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) xs[j] = raw[(j + HOPJ * ROT) & 15];
            if (REGS & APM_REG_WIN) {
#pragma unroll
                for (int j = 0; j < 16; ++j) ws[j] = winr[j];
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j) ws[j] = WIN[lane + 64 * j];
            }
            AP_SCHED_FENCE();
            apm_forward<REGS>(xs, ws, X, TW1 + APM_TW_ROW * lane, TW2 + APM_TW2_ROW * lane, t1r, t2r, t2, lc);
        }
        AP_SCHED_FENCE();
        if (more) {
            if (clip_ends) clip = ap_clip_make(P.y + (b + 1) * P.L, P.L);
            const int base = (clip_ends ? 0 : t + 1) * P.hop - P.pad;
#pragma unroll
            for (int j = 16 - HOPJ; j < 16; ++j)
                raw[(j + HOPJ * NROT) & 15] = ap_clip_load2(clip, base + 2 * (lane + 64 * j));
            if (HOPJ == 0 || clip_ends) {
#pragma unroll
                for (int j = 0; j < 16 - HOPJ; ++j)
                    raw[(j + HOPJ * NROT) & 15] = ap_clip_load2(clip, base + 2 * (lane + 64 * j));
            }
        }
        AP_SCHED_FENCE();
        apm_split<PMODE>(X, pp, pl, wsp, t2, lc, P.power);
        AP_WAVE_SYNC();
        // ---- this lane's 16 (17) contiguous bins -------------------------------------------
        float v[17];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const ap_float4 a = reinterpret_cast<const ap_float4 *>(pp)[4 * lane + q4];
            v[4 * q4] = a.x; v[4 * q4 + 1] = a.y; v[4 * q4 + 2] = a.z; v[4 * q4 + 3] = a.w;
        }
        v[16] = lane == 63 ? pp[APW_NC] : 0.0f;
        AP_WAVE_SYNC();                           // the plane is free for the next frame's transform
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int i = 0; i < 17; ++i) { s0 += v[i]; s1 = fmaf(fk[i], v[i], s1); }
        const float tot = apm_wave_sum(s0), tf = apm_wave_sum(s1);
        const float cen = tf / (tot + 1e-10f);
        const int64_t o = b * P.T + t;
        if (P.centroid && lane == 0) P.centroid[o] = cen;
        if (FLAT) {                               // features.py:427-437: exp(mean log max(S, amin)) / mean max(S, amin)
            float sl = 0.0f, sa = 0.0f;
#pragma unroll
            for (int i = 0; i < 17; ++i) {
                const float c = fmaxf(v[i], P.amin);
                if (i < 16 || lane == 63) { sl += logf(c); sa += c; }
            }
            const float tl = apm_wave_sum(sl), ta = apm_wave_sum(sa);
            if (P.flatness && lane == 0) P.flatness[o] = expf(tl / F_all) / (ta / F_all + 1e-10f);
        }
        if (P.bandwidth) {                        // features.py:242-266
            float dev = 0.0f;
#pragma unroll
            for (int i = 0; i < 17; ++i) {
                const float d = fabsf(fk[i] - cen);
                dev = fmaf(v[i], PGEN ? powf(d, P.p) : d * d, dev);
            }
            float w = apm_wave_sum(dev);
            if (P.norm) w = w / (tot + 1e-10f);
            if (lane == 0) P.bandwidth[o] = PGEN ? powf(w, 1.0f / P.p) : sqrtf(w);
        }
        if (P.rolloff) {                          // features.py:342-360: first bin whose running sum reaches the threshold
            float incl = s0;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const float up = apm_lane_up(incl, d, lane);
                if (lane >= d) incl += up;
            }
            const float before = incl - s0;
            const float thr = tot * P.roll_percent;
            const bool mine = (before + s0 >= thr) && (lane == 0 || before < thr);
            float run = before, fsel = lane == 63 ? fk[16] : fk[15];
            bool found = false;
#pragma unroll
            for (int i = 0; i < 17; ++i) {
                if (i < 16 || lane == 63) {
                    run += v[i];
                    if (!found && run >= thr) { found = true; fsel = fk[i]; }
                }
            }
            // lowest candidate of the wave (the tree-ordered scan is monotone only up to rounding, so there
            // may be none or two); no candidate: the last bin; sums that never reach thr (NaNs): bin 0
            float cand = (mine && found) ? fsel : INFINITY;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) cand = fminf(cand, apm_lane_xor(cand, off));
            const float last = apm_lane_xor(fk[16], 63);               // lane 0 gets lane 63's bin 1024
            if (lane == 0) P.rolloff[o] = !(tot >= thr) ? fk[0] : (cand < INFINITY ? cand : last);
        }
        if (clip_ends) { t = 0; ++b; } else { ++t; }
        ++f;
        return more;
    };
    if (U == 1) {
        while (frame(std::integral_constant<int, 0>())) {}
    } else {
        for (;;) {
            if (!frame(std::integral_constant<int, 0>())) break;
            if (!frame(std::integral_constant<int, 1 % U>())) break;
            if (!frame(std::integral_constant<int, 2 % U>())) break;
            if (!frame(std::integral_constant<int, 3 % U>())) break;
        }
    }
}
