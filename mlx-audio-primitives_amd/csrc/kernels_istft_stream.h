// Streaming (chunked) ISTFT with a carried overlap-add: ap_istft_stream_f32 (include/audioprims.h).
//
// A stream of frames S[:, :, 0..K) arrives in calls of T frames; frame0 frames came before the call.  Frame f
// covers absolute samples [f hop, f hop + n), so once K frames are in, every sample p < K hop is finished (no
// later frame touches it).  A call
//   * starts every sample's sum from the carried, UNNORMALISED partial sum of the earlier frames (carry_in:
//     samples [frame0 hop, frame0 hop + n - hop); ignored when frame0 == 0),
//   * adds the windowed inverse transforms of its own frames in increasing frame order,
//   * divides the samples it finishes by max(sum w^2, 1e-8), the envelope of the absolute frame indices that
//     touch the sample (frames 0 .. min(p / hop, K - 1); never carried),
//   * writes the samples of [lo, hi) and, unless it is the final call, the new carry (samples [K hop, K hop +
//     n - hop)).  The final call also normalises and writes the pending n - hop samples with the end envelope.
// Every sample's sum is the same fmaf chain over frames 0, 1, 2, ... whatever the chunking, every frame's
// inverse transform is computed by the same code whatever its position in a call, and the envelope depends
// on p and K only: the concatenated outputs are bit-identical over any chunking.
//
// Fused path (n_fft = 2048, 1024, 512, 400, 256; one launch): a 256-thread workgroup owns the samples that G
// consecutive frames of one clip finish.  It recomputes the H = ceil(n / hop) - 1 frames of the call before
// them (its halo) instead of exchanging partial sums with the neighbouring workgroup, runs the inverse
// transforms Gb frames at a time through the LDS Stockham engine (fft_lds.h) and accumulates into an LDS row
// of its samples; the workgroup of a clip's last frames also produces the carry (or, final, the tail).
// Other n_fft: ap_irfft_frames_f32 into a (B, T, n) workspace, then ap_istft_stream_ola_kernel (two launches).
#pragma once
#include "ap_launch.h"
#include "fft_lds.h"

extern __shared__ __attribute__((aligned(16))) char ap_smem[];

#define AP_ISTFTS_G 16              // frames a workgroup finishes (fewer when hop is large, see the prepare step)
#define AP_ISTFTS_FFT_LDS 40960     // bytes of the two ping-pong transform buffers
#define AP_ISTFTS_ACC_MAX 16384     // floats of the sample row

struct ApIstftStreamParams {
    const ap_float2 *S;       // (B, F, row_stride) complex; fused path
    const float *frames;      // (B, T, n) inverse transforms, already scaled by 1/n; two-launch path
    const float *window;      // (n)
    const ap_float2 *tw;      // (n) (cos, sin)(2 pi j / n)
    const float *carry_in;    // (B, n - hop); read when frame0 > 0
    float *carry_out;         // (B, n - hop); written unless final_
    float *out;               // (B, hi - lo)
    int64_t T, row_stride, frame0, lo, hi;
    int64_t tiles_per_clip;   // fused path: max(1, ceil(T / G))
    int64_t blocks_per_row;   // two-launch path
    int n, hop, H, G, Gb, fstride, final_;
    int acc_off, lds_bytes;
    ApFftPlan plan;
};

static inline bool ap_istft_stream_fused(int n_fft) {
    return n_fft == 2048 || n_fft == 1024 || n_fft == 512 || n_fft == 400 || n_fft == 256;
}

// Validation and geometry.  G > 0 overrides the frames per workgroup (the CPU emulator test uses small tiles
// so that halos cross workgroups and calls shorter than the halo occur).
static inline int ap_prepare_istft_stream(ApIstftStreamParams &P, const float *S, int64_t B, int64_t T,
                                          int64_t row_stride, int n_fft, int hop, const float *window,
                                          const float *tw, int64_t frame0, const float *carry_in, float *carry_out,
                                          int final_, int64_t lo, int64_t hi, float *out, int G = 0) {
    if (B < 0 || T < 0) AP_FAIL(AP_ERR_INVALID, "istft_stream: negative batch (%lld) or frame count (%lld)",
                                (long long)B, (long long)T);
    if (n_fft <= 0) AP_FAIL(AP_ERR_INVALID, "istft_stream: n_fft must be positive, got %d", n_fft);
    if (hop <= 0 || hop > n_fft)
        AP_FAIL(AP_ERR_INVALID, "istft_stream: hop_length (%d) must be in (0, n_fft = %d]", hop, n_fft);
    if (frame0 < 0) AP_FAIL(AP_ERR_INVALID, "istft_stream: frame0 must be non-negative");
    if (!window) AP_FAIL(AP_ERR_INVALID, "istft_stream: NULL window");
    if (T > 0 && (!S || !tw)) AP_FAIL(AP_ERR_INVALID, "istft_stream: NULL spectrum or twiddles");
    if (row_stride < T)
        AP_FAIL(AP_ERR_INVALID, "istft_stream: row_stride (%lld) must be >= the number of frames (%lld)",
                (long long)row_stride, (long long)T);
    const int64_t C = n_fft - hop;
    const int64_t K = frame0 + T;
    if (final_ && K == 0) AP_FAIL(AP_ERR_INVALID, "istft_stream: the final call needs at least one frame");
    if (B > 0 && C > 0 && frame0 > 0 && !carry_in) AP_FAIL(AP_ERR_INVALID, "istft_stream: NULL carry_in");
    if (B > 0 && C > 0 && !final_ && !carry_out) AP_FAIL(AP_ERR_INVALID, "istft_stream: NULL carry_out");
    if (B > 0 && C > 0 && frame0 > 0 && !final_ && carry_in + B * C > carry_out && carry_out + B * C > carry_in)
        AP_FAIL(AP_ERR_INVALID, "istft_stream: carry_out must not alias carry_in");
    const int64_t start = frame0 * hop;
    const int64_t end = final_ ? (K - 1) * hop + n_fft : K * hop;
    if (hi < lo || (hi > lo && (lo < start || hi > end)))   // an empty range may sit anywhere
        AP_FAIL(AP_ERR_INVALID, "istft_stream: output range [%lld, %lld) is not inside the samples [%lld, %lld) "
                "this call finishes", (long long)lo, (long long)hi, (long long)start, (long long)end);
    if (B > 0 && hi > lo && !out) AP_FAIL(AP_ERR_INVALID, "istft_stream: NULL output");
    if (ap_make_plan(n_fft, &P.plan) != 0) AP_FAIL(AP_ERR_UNSUPPORTED, "n_fft=%d: cannot build FFT plan", n_fft);
    P.S = reinterpret_cast<const ap_float2 *>(S);
    P.frames = nullptr;
    P.window = window;
    P.tw = reinterpret_cast<const ap_float2 *>(tw);
    P.carry_in = carry_in;
    P.carry_out = carry_out;
    P.out = out;
    P.T = T;
    P.row_stride = row_stride;
    P.frame0 = frame0;
    P.lo = lo;
    P.hi = hi;
    P.n = n_fft;
    P.hop = hop;
    P.H = (n_fft + hop - 1) / hop - 1;
    P.final_ = final_ ? 1 : 0;
    P.fstride = P.plan.nc + 1;
    const int64_t per_frame = 2 * (int64_t)P.fstride * (int64_t)sizeof(ap_float2);
    int gb = (int)(AP_ISTFTS_FFT_LDS / per_frame);
    P.Gb = gb < 1 ? 1 : (gb > AP_MAX_G ? AP_MAX_G : gb);
    int g = (int)((AP_ISTFTS_ACC_MAX - C) / hop);
    if (g > AP_ISTFTS_G) g = AP_ISTFTS_G;
    if (G > 0 && G < g) g = G;
    P.G = g < 1 ? 1 : g;
    const int64_t lds = P.Gb * per_frame + (int64_t)sizeof(float) * (P.G * (int64_t)hop + C);
    if (ap_istft_stream_fused(n_fft) && lds > AP_LDS_MAX)         // (the two-launch path uses no LDS)
        AP_FAIL(AP_ERR_UNSUPPORTED, "istft_stream: n_fft=%d does not fit the %d KiB LDS of one CU", n_fft,
                AP_LDS_MAX / 1024);
    P.acc_off = (int)(P.Gb * per_frame);
    P.lds_bytes = (int)lds;
    P.tiles_per_clip = T > 0 ? (T + P.G - 1) / P.G : 1;
    const int64_t span = T * hop + C;                   // samples [frame0 hop, K hop + n - hop)
    P.blocks_per_row = (span + AP_BLOCK - 1) / AP_BLOCK;
    if (P.tiles_per_clip * B > kApMaxGrid || P.blocks_per_row * B > kApMaxGrid)
        AP_FAIL(AP_ERR_UNSUPPORTED, "istft_stream: grid too large");
    return AP_OK;
}

// ---- device helpers shared by both paths ----------------------------------------------------------------------
// Partial sum of absolute sample p carried in from the earlier calls (0 for the first call).
AP_DEV float ap_istfts_carry(const ApIstftStreamParams &P, int64_t b, int64_t p) {
    const int64_t C = P.n - P.hop;
    const int64_t i = p - P.frame0 * P.hop;
    return (P.frame0 > 0 && i < C) ? P.carry_in[b * C + i] : 0.0f;
}

// Sample p with its complete sum over the call's frames: into the carry (not finished, not final), or
// normalised by the envelope of frames 0 .. min(p / hop, K - 1), increasing frame order, into out[lo, hi).
AP_DEV void ap_istfts_store(const ApIstftStreamParams &P, int64_t b, int64_t p, float acc) {
    const int n = P.n, hop = P.hop;
    const int64_t K = P.frame0 + P.T;
    const int64_t done = K * hop;
    if (p >= done && !P.final_) {
        P.carry_out[b * (int64_t)(n - hop) + (p - done)] = acc;
        return;
    }
    if (p < P.lo || p >= P.hi) return;
    int64_t f = p - n + 1 <= 0 ? 0 : (p - n + hop) / hop;   // first frame touching p: ceil((p - n + 1) / hop)
    int64_t fe = p / hop;
    if (fe > K - 1) fe = K - 1;
    float wss = 0.0f;
    for (; f <= fe; ++f) {
        const float w = P.window[(int)(p - f * hop)];
        wss = fmaf(w, w, wss);
    }
    P.out[b * (P.hi - P.lo) + (p - P.lo)] = acc / fmaxf(wss, 1e-8f);
}

// ---- fused path: one launch, grid = B x tiles_per_clip, AP_BLOCK threads ---------------------------------------
// N = n_fft (even).  LDS: two transform buffers of Gb frames (fstride complex values each), then the row of
// samples the workgroup finishes (G hop, plus the n - hop carried / tail samples for a clip's last workgroup).
template <int N>
__global__ void __launch_bounds__(AP_BLOCK) ap_istft_stream_kernel(ApIstftStreamParams P) {
    static_assert(N % 2 == 0, "fused streaming ISTFT: even n_fft only");
    constexpr int NC = N / 2;
    const ApFftPlan &pl = P.plan;
    const int hop = P.hop, G = P.G, Gb = P.Gb, fstride = P.fstride;
    ap_float2 *bufA = reinterpret_cast<ap_float2 *>(ap_smem);
    ap_float2 *bufB = bufA + (size_t)Gb * fstride;
    float *acc = reinterpret_cast<float *>(ap_smem + P.acc_off);
    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x;
    const int64_t b = bid / P.tiles_per_clip;
    const int64_t tile = bid - b * P.tiles_per_clip;
    const bool last = tile == P.tiles_per_clip - 1;
    const int64_t t0 = tile * G;                                   // first frame the workgroup finishes (call index)
    const int Gt = last ? (int)(P.T - t0) : G;                     // 0 only for a call without frames
    const int64_t P0 = (P.frame0 + t0) * hop;                      // first sample of the row (absolute)
    const int span = Gt * hop + (last ? N - hop : 0);
    // every thread owns the same row positions i = tid + 256 j in every phase below: the row needs no barrier
    for (int i = tid; i < span; i += AP_BLOCK) acc[i] = ap_istfts_carry(P, b, P0 + i);

    const int64_t ta = t0 - P.H < 0 ? 0 : t0 - P.H;                // the halo: earlier frames of this call
    const int nf = (int)(t0 + Gt - ta);
    const ap_float2 *Sb = P.S + b * (int64_t)(NC + 1) * P.row_stride;
    const float scale = 1.0f / (float)N;
    for (int f0 = 0; f0 < nf; f0 += Gb) {
        const int gb = nf - f0 < Gb ? nf - f0 : Gb;
        AP_LDS_BARRIER();                                          // the previous batch's transforms are consumed
        // conj of the packed half-length spectrum (the inverse through the forward engine, as ap_irfft_generic_kernel)
        for (int item = tid; item < NC * Gb; item += AP_BLOCK) {
            const int k = item / Gb;
            const int g = item - k * Gb;
            ap_float2 zc = ap_mk(0.0f, 0.0f);
            if (g < gb) {
                const int64_t col = ta + f0 + g;
                ap_float2 xk = Sb[(int64_t)k * P.row_stride + col];
                ap_float2 xm = Sb[(int64_t)(NC - k) * P.row_stride + col];
                if (k == 0) { xk.y = 0.0f; xm.y = 0.0f; }          // DC / Nyquist imaginary parts ignored
                const float ax = xk.x + xm.x, ay = xk.y - xm.y;
                const float dx = xk.x - xm.x, dy = xk.y + xm.y;
                const ap_float2 w = P.tw[k];
                const float ox = w.x * dx - w.y * dy, oy = w.x * dy + w.y * dx;
                zc = ap_mk(ax - oy, -(ay + ox));
            }
            bufA[g * fstride + k] = zc;
        }
        AP_LDS_BARRIER();
        const ap_float2 *Y = ap_fft_tile(bufA, bufB, pl, P.tw, Gb, fstride, tid, AP_BLOCK);
        const int64_t fa = P.frame0 + ta + f0;                     // absolute index of the batch's first frame
        // only the row positions the batch reaches, still visited as i = tid + 256 j
        const int64_t r0 = fa * hop - P0, r1 = r0 + (int64_t)(gb - 1) * hop + N;
        const int ilo = r0 < 0 ? 0 : (int)r0;
        const int ihi = r1 < span ? (int)r1 : span;
        for (int i = (ilo & ~(AP_BLOCK - 1)) + tid; i < ihi; i += AP_BLOCK) {
            if (i < ilo) continue;
            const int64_t p = P0 + i;
            float a = acc[i];
            for (int g = 0; g < gb; ++g) {
                const int64_t s = p - (fa + g) * hop;
                if (s >= 0 && s < N) {
                    const ap_float2 v = Y[g * fstride + (int)(s >> 1)];
                    const float x = ((s & 1) ? -v.y : v.x) * scale;
                    a = fmaf(P.window[s], x, a);
                }
            }
            acc[i] = a;
        }
    }
    for (int i = tid; i < span; i += AP_BLOCK) ap_istfts_store(P, b, P0 + i, acc[i]);
}

// ---- two-launch path: the carried overlap-add of ap_irfft_frames_f32's frames -----------------------------------
// One thread per sample of [frame0 hop, K hop + n - hop); grid = B x blocks_per_row.
AP_KERNEL void __launch_bounds__(AP_BLOCK) ap_istft_stream_ola_kernel(ApIstftStreamParams P) {
    const int64_t bid = blockIdx.x;
    const int64_t b = bid / P.blocks_per_row;
    const int64_t i = (bid - b * P.blocks_per_row) * AP_BLOCK + threadIdx.x;
    const int n = P.n, hop = P.hop;
    if (i >= P.T * hop + (n - hop)) return;
    const int64_t p = P.frame0 * hop + i;
    float a = ap_istfts_carry(P, b, p);
    int64_t t = i - n + 1 <= 0 ? 0 : (i - n + hop) / hop;
    int64_t tl = i / hop;
    if (tl > P.T - 1) tl = P.T - 1;
    const float *fb = P.frames + b * P.T * (int64_t)n;
    for (; t <= tl; ++t) {
        const int s = (int)(i - t * hop);
        a = fmaf(P.window[s], fb[t * n + s], a);
    }
    ap_istfts_store(P, b, p, a);
}
