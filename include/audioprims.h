/*
 * audioprims.h — C ABI of libaudioprims_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary that takes the place of the reference's native
 * extension (nanobind module `_ext`, /root/reference/csrc/bindings.cpp:11-485)
 * and of the two third-party device calls on the hot path that have no source
 * under the reference (`mx.fft.rfft`, stft.py:130; `mx.fft.irfft`, stft.py:295).
 *
 * Conventions
 *  - plain C, no torch / HIP types in signatures.  `stream` is a hipStream_t
 *    passed as void* (NULL = the default stream).
 *  - every pointer marked [dev] is device memory owned and pre-allocated by the
 *    caller; [host] is host memory.  The library never allocates or frees device
 *    memory, never synchronises: it only enqueues kernels on `stream`
 *    (the reference's Metal paths force eval() before encoding,
 *    overlap_add.cpp:45-48 — not reproduced).
 *  - all arrays are contiguous float32 (complex = interleaved re,im float32),
 *    row-major, shapes as in the reference's Python API.
 *  - return value: 0 = ok; AP_ERR_INVALID (<0) = invalid argument (the
 *    reference throws std::invalid_argument -> Python ValueError, e.g.
 *    overlap_add.cpp:205-222); AP_ERR_UNSUPPORTED; AP_ERR_HIP = a HIP runtime
 *    error at launch.  ap_last_error() returns a thread-local message.
 *  - re-entrant, no hidden state: windows, filterbanks, twiddles and FIR taps
 *    are inputs (built on the host in float64 by the ap_*_host builders below,
 *    cached per device by the caller).
 */
#ifndef AUDIOPRIMS_H
#define AUDIOPRIMS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AP_OK 0
#define AP_ERR_INVALID (-1)
#define AP_ERR_UNSUPPORTED (-2)
#define AP_ERR_HIP (-3)

/* pad modes — stft.py:441-468, pad_signal.metal:10-121 */
#define AP_PAD_CONSTANT 0
#define AP_PAD_EDGE 1
#define AP_PAD_REFLECT 2

/* window kinds — windows.cpp:179-228 */
#define AP_WIN_HANN 0
#define AP_WIN_HAMMING 1
#define AP_WIN_BLACKMAN 2
#define AP_WIN_BARTLETT 3
#define AP_WIN_RECTANGULAR 4

int ap_version(void);
const char *ap_last_error(void);

/* ---------------------------------------------------------------------- *
 * Host-side builders (float64 internally).  Replace the CPU-stream parts of
 * the reference extension.
 * ---------------------------------------------------------------------- */

/* generate_window(window_type, length, periodic) — bindings.cpp:105-130,
 * windows.cpp:179-228: float64 build, cast to float32, average with own
 * reverse (windows.cpp:73-78); periodic = (length+1)-point window minus the
 * last point.  out_host: `length` floats. */
int ap_generate_window_host(int kind, int length, int periodic, float *out_host);

/* hz_to_mel / mel_to_hz(arr, htk) — bindings.cpp:133-181, mel_filterbank.cpp:70-106.
 * float64 in/out on the host. */
int ap_hz_to_mel_host(const double *hz, int64_t n, int htk, double *out);
int ap_mel_to_hz_host(const double *mel, int64_t n, int htk, double *out);

/* mel_filterbank(sr, n_fft, n_mels, fmin, fmax, htk, norm) — bindings.cpp:183-221,
 * mel_filterbank.cpp:108-239 (librosa's fdiff/ramps formulation, float64, one cast).
 * fmax < 0 means sr/2.  norm_slaney: 1 = "slaney", 0 = none.
 * out_host: n_mels*(n_fft/2+1) floats. */
int ap_mel_filterbank_host(int sr, int n_fft, int n_mels, double fmin, double fmax,
                           int htk, int norm_slaney, float *out_host);

/* get_dct_matrix(n_out, n_in, norm) — bindings.cpp:313-335, dct.cpp:24-101:
 * DCT-II basis evaluated in FLOAT32 like the reference's native path (dct.cpp:59).
 * out_host: n_out*n_in floats. */
int ap_dct_matrix_host(int n_out, int n_in, int ortho, float *out_host);

/* Twiddle table for an n_fft-point real transform: out_host[2j] = cos(2*pi*j/n),
 * out_host[2j+1] = sin(2*pi*j/n), j in [0,n), float64-evaluated, exact at the
 * quadrant points.  (Stands in for whatever mx.fft precomputes internally.) */
int ap_twiddle_table_host(int n_fft, float *out_host);

/* FIR of scipy.signal.resample_poly for the reduced ratio up/down (the reference's
 * resample_poly is exactly that SciPy call, resample.py:279-281):
 *   firwin(2*10*max(up,down)+1, 1/max(up,down), window=('kaiser', 5.0)) cast to float32,
 *   times up (float32), with n_pre_pad = down - half_len % down zeros prepended.
 * out_host must hold ap_resample_poly_ntaps(up, down) floats; n_pre_remove_out gets
 * (half_len + n_pre_pad) / down, the number of leading outputs SciPy discards. */
int ap_resample_poly_ntaps(int up, int down);
int ap_resample_poly_taps_host(int up, int down, float *out_host, int *n_pre_remove_out);

/* 1 if the LDS FFT engine can transform n_fft-point real frames, else 0. */
int ap_fft_supported(int n_fft);

/* ---------------------------------------------------------------------- *
 * Device primitives — 1:1 with the reference extension's hot-path entries.
 * ---------------------------------------------------------------------- */

/* pad_signal(signal (B,L), pad_length, mode) -> (B, L+2*pad) — bindings.cpp:76-102,
 * pad_signal.cpp:133-162.  reflect requires pad <= L-1 (pad_signal.cpp:102-105). */
int ap_pad_f32(const float *x /*dev*/, int64_t B, int64_t L, int64_t pad, int mode,
               float *out /*dev (B, L+2*pad)*/, void *stream);

/* frame_signal(signal (B,L), frame_length, hop) -> (B,T,frame_length),
 * T = 1 + (L-frame_length)/hop — bindings.cpp:48-74, frame_signal.cpp:119-155. */
int ap_frame_f32(const float *x /*dev*/, int64_t B, int64_t L, int frame_length, int hop,
                 float *out /*dev (B,T,frame_length)*/, void *stream);

/* overlap_add(frames (B,T,N), window (N,), hop, output_length) -> (B,out_len)
 * — bindings.cpp:15-46, overlap_add.cpp:195-233, overlap_add.metal:16-55:
 *   out[b,i] = sum_f w[p-fH]*frames[b,f,p-fH] / max(sum_f w[p-fH]^2, 1e-8),  p = i + out_offset
 * `out_offset` (>=0) lets istft fold its centre trim (stft.py:315-329) into the
 * same pass; the reference entry is out_offset = 0. */
int ap_overlap_add_f32(const float *frames /*dev*/, const float *window /*dev*/, int64_t B,
                       int64_t T, int n_fft, int hop, int64_t out_offset, int64_t out_len,
                       float *out /*dev (B,out_len)*/, void *stream);

/* ---------------------------------------------------------------------- *
 * Fused transforms — replace `_stft_core` (pad -> frame -> *window -> mx.fft.rfft,
 * stft.py:109-133) plus the transpose (stft.py:216), and mel.py:310-350.
 * ---------------------------------------------------------------------- */

/* stft: y (B,L) -> out (B, F=n_fft/2+1, T) complex64 (interleaved).
 *   window : n_fft floats, already centre-padded (stft.py:88-106)
 *   tw     : table from ap_twiddle_table_host(n_fft) copied to the device
 *   center : pad n_fft/2 both sides with `pad_mode` without materialising it
 *   T must equal 1 + (L + 2*pad - n_fft)/hop (_frame_impl.py:61). */
int ap_stft_f32(const float *y /*dev*/, int64_t B, int64_t L, int n_fft, int hop,
                const float *window /*dev*/, const float *tw /*dev*/, int center, int pad_mode,
                int64_t T, float *out /*dev (B,F,T,2)*/, void *stream);

/* The same with the rows of `out` `row_stride` complex values apart (row_stride >= T; the (B, F, T)
 * result is then a strided view of a (B, F, row_stride) buffer and the columns T..row_stride-1 are
 * never written).  With row_stride a multiple of 16 and a 128-byte aligned `out` every group of 16
 * frames leaves as whole 128-byte lines - the workspace layout of the Griffin-Lim loop
 * (griffinlim.py:129-180), where the spectra never leave the library.  No reference counterpart:
 * mx.fft.rfft + transpose (stft.py:130,216) always yields the dense layout, which is row_stride = T. */
int ap_stft_rows_f32(const float *y /*dev*/, int64_t B, int64_t L, int n_fft, int hop,
                     const float *window /*dev*/, const float *tw /*dev*/, int center, int pad_mode,
                     int64_t T, int64_t row_stride, float *out /*dev (B,F,row_stride,2)*/, void *stream);

/* Mel contraction plan.  The filterbank is tiny and built on the host (mel.py:100-168),
 * so its sparsity is analysed on the host once and shipped to the device next to it.
 * ap_mel_plan_host fills a device-bound blob `plan` (int32 words, copy it to HBM) and a
 * 16-int host descriptor `desc` that the caller hands back to ap_melspec_f32:
 *   desc[0] flags   AP_PLAN_BANDED | AP_PLAN_PARTS      desc[1] n_mels   desc[2] n_bins
 *   desc[3] total words of the blob
 *   desc[4] off band_lo[M]   desc[5] off band_len[M]    (span holding all non-zeros of a filter)
 *   desc[6] off parts[n_parts][4] = (slot, first 4-bin group, n_groups<=4, first quad)
 *   desc[7] n_parts          desc[8] off quads[n_quads][4] float weights   desc[9] n_quads
 *   desc[10] off rowstart[M+1]: row m's partial sums live in slots [rowstart[m], rowstart[m+1])
 *   desc[11] off wave_parts[n_wave_parts][4]: the same parts dealt to wavefront lanes (entry
 *            64 p + l = lane l of pass p) as (slot A, group A, slot B, group B): the entry's
 *            weight rows 0-1 go with |X|^p groups A, A+1 and sum into slot A, rows 2-3 go with
 *            groups B, B+1 and sum into slot B - a second part of <= 2 groups - or, slot B = -1,
 *            on top of slot A (one part of 3-4 groups), or into the dump slot n_parts (nothing
 *            there; an idle lane has both slots = n_parts).  Entries are ordered so that the
 *            16-byte LDS reads of one pass fall into different banks
 *   desc[13] off wave_quads[n_wave_quads][4]: lane-interleaved weights, row i of entry 64 p + l at
 *            256 p + 64 i + l (zero where a part ends)
 *   desc[12] n_wave_parts (multiple of 64)   desc[14] n_wave_quads = 4 n_wave_parts
 *   desc[15] largest number of parts of one row
 * Parts split each filter's span into runs of <= 4 aligned 4-bin groups, sorted by
 * length, so the wave kernel can contract with 16-byte LDS reads.  Zeros outside a
 * span contribute exactly 0 to the reference's matmul (mel.py:344-350), so using the
 * plan does not change which products are summed. */
#define AP_PLAN_BANDED 1
#define AP_PLAN_PARTS 2
#define AP_PLAN_FORCE_GENERIC 256   /* caller-set in desc[0]: keep the generic LDS engine (tests) */
#define AP_PLAN_DESC_INTS 16
int64_t ap_mel_plan_words(const float *fb_host /*(M,F)*/, int n_mels, int n_bins);
int ap_mel_plan_host(const float *fb_host /*(M,F)*/, int n_mels, int n_bins,
                     int32_t *plan_host, int32_t *desc_host /*16 ints*/);

/* melspectrogram: y (B,L) -> out (B, n_mels, T) = fb @ |stft(y)|^power, fused
 * (no (B,F,T) intermediate).  fb is the dense (n_mels, F) filterbank
 * (mel.py:100-168); plan (device) + desc (host) come from ap_mel_plan_host, both may
 * be NULL: dense contraction.  n_fft = 2048 with a PARTS plan runs the wave-per-frame
 * kernel (kernels_wave.h); everything else the generic LDS engine (kernels_generic.h). */
int ap_melspec_f32(const float *y /*dev*/, int64_t B, int64_t L, int n_fft, int hop,
                   const float *window /*dev*/, const float *tw /*dev*/, int center,
                   int pad_mode, int64_t T, const float *fb /*dev (M,F)*/,
                   const int32_t *plan /*dev*/, const int32_t *desc /*host, 16 ints*/,
                   int n_mels, float power, float *out /*dev (B,M,T)*/, void *stream);

/* The same, and also raises *max_key_dev (order-preserving key as in ap_reduce_max_f32, reset by
 * the call) to max(out): mfcc's top_db clip needs the global maximum of the mel power, and the
 * n_fft = 2048 kernel gets it for one atomic per wavefront instead of another pass over out. */
int ap_melspec_max_f32(const float *y /*dev*/, int64_t B, int64_t L, int n_fft, int hop,
                       const float *window /*dev*/, const float *tw /*dev*/, int center, int pad_mode,
                       int64_t T, const float *fb /*dev*/, const int32_t *plan /*dev or NULL*/,
                       const int32_t *desc /*host or NULL*/, int n_mels, float power,
                       float *out /*dev*/, uint32_t *max_key_dev /*dev or NULL*/, void *stream);
/* The same with the rows of `out` `row_stride` floats apart (row_stride >= T: the (B, M, T) result is a strided view of
 * a (B, M, row_stride) buffer, the columns T..row_stride-1 are never written).  With row_stride a multiple of 8 the
 * n_fft = 2048 run kernel's 8-frame output runs are whole aligned 32-byte sectors.  Served by that kernel only
 * (ap_melspec_rows_fused says whether it applies: n_fft = 2048, power 1 or 2, <= 128 filters, constant padding with
 * an even hop or center = 0); AP_ERR_UNSUPPORTED otherwise.  No reference counterpart: mx.matmul yields dense rows. */
int ap_melspec_rows_fused(int n_fft, int hop, int center, int pad_mode, int n_mels, float power,
                          const int32_t *plan /*host or NULL*/, const int32_t *desc /*host*/);
int ap_melspec_rows_f32(const float *y /*dev*/, int64_t B, int64_t L, int n_fft, int hop,
                        const float *window /*dev*/, const float *tw /*dev*/, int center, int pad_mode,
                        int64_t T, int64_t row_stride, const float *fb /*dev*/, const int32_t *plan /*dev*/,
                        const int32_t *desc /*host*/, int n_mels, float power, float *out /*dev (B,M,row_stride)*/,
                        uint32_t *max_key_dev /*dev or NULL*/, void *stream);

/* irfft of every frame: S (B,F,T) complex64 -> frames (B,T,n_fft) float32,
 * 1/n_fft scaled; imaginary parts of the DC and Nyquist bins are ignored —
 * mx.fft.irfft(·, n=n_fft) at stft.py:292-295 (incl. the transpose). */
int ap_irfft_frames_f32(const float *S /*dev (B,F,T,2)*/, int64_t B, int64_t T, int n_fft,
                        const float *tw /*dev*/, float *frames /*dev (B,T,n_fft)*/,
                        void *stream);

/* istft core: irfft + window + overlap-add + sum(w^2) normalise + trim.
 *   out[b,i] = OLA(position i + out_offset), i in [0,out_len)
 *   frames_ws : caller-provided workspace of ap_istft_workspace_floats(...) floats (B*T*n_fft
 *               in general; 0 — the pointer may then be NULL — when the fused n_fft = 2048
 *               kernel applies: the frames stay in LDS and never reach HBM).
 * Length logic (stft.py:300-338) stays in the caller. */
int64_t ap_istft_workspace_floats(int64_t B, int64_t T, int n_fft, int hop, int64_t out_offset);
int ap_istft_f32(const float *S /*dev (B,F,T,2)*/, int64_t B, int64_t T, int n_fft, int hop,
                 const float *window /*dev*/, const float *tw /*dev*/, float *frames_ws /*dev*/,
                 int64_t out_offset, int64_t out_len, float *out /*dev (B,out_len)*/,
                 void *stream);

/* The same from a spectrum whose rows are `row_stride` complex values apart (the layout ap_stft_rows_f32
 * writes; row_stride == T is the dense layout).  n_fft = 2048 with hop in {256, 512, 1024} and row_stride <= 490 000
 * (a clip is addressed as one buffer resource: 1025 row_stride 8 bytes < 0xF0000000), and the eight-frame sizes
 * (n_fft 512 / 400 / 256) only - the fused kernels, no workspace; AP_ERR_UNSUPPORTED otherwise - copy to a dense
 * array and call ap_istft_f32. */
int ap_istft_rows_f32(const float *S /*dev (B,F,row_stride,2)*/, int64_t B, int64_t T, int64_t row_stride,
                      int n_fft, int hop, const float *window /*dev*/, const float *tw /*dev*/,
                      int64_t out_offset, int64_t out_len, float *out /*dev (B,out_len)*/, void *stream);

/* Streaming ISTFT (center=False frames; the centre trim is the caller's lo / hi).  A call feeds T frames
 * whose absolute index starts at frame0 (frames fed by the earlier calls); with K = frame0 + T every sample
 * p < K*hop is finished.  The call
 *   - starts each sample's sum from carry_in, the unnormalised partial sums of samples
 *     [frame0*hop, frame0*hop + n_fft - hop) (ignored, may be NULL, when frame0 == 0),
 *   - adds its frames' windowed inverse transforms in increasing frame order,
 *   - writes out[b, p - lo] = sum / max(sum of w^2 over the frames 0..min(p/hop, K-1) touching p, 1e-8)
 *     for p in [lo, hi), where frame0*hop <= lo <= hi <= K*hop, or <= (K-1)*hop + n_fft when final_ = 1
 *     (the pending tail, normalised with the end-of-stream envelope),
 *   - unless final_, writes carry_out: the partial sums of samples [K*hop, K*hop + n_fft - hop).
 * Concatenated over any chunking the outputs are bit-identical.  0 < hop <= n_fft; T may be 0 (flush);
 * S rows are row_stride >= T complex values apart, batch stride F*row_stride.  carry_out must not alias
 * carry_in.  No allocation, no synchronisation, no state across calls.  n_fft 2048 / 1024 / 512 / 400 /
 * 256: one fused launch, no workspace; other n_fft: row_stride == T, ap_irfft_frames_f32 into frames_ws
 * (ap_istft_stream_workspace_floats(...) floats) and a carried overlap-add (two launches). */
int64_t ap_istft_stream_workspace_floats(int64_t B, int64_t T, int n_fft, int hop);
int ap_istft_stream_f32(const float *S /*dev (B,F,row_stride,2)*/, int64_t B, int64_t T, int64_t row_stride,
                        int n_fft, int hop, const float *window /*dev*/, const float *tw /*dev*/, int64_t frame0,
                        const float *carry_in /*dev (B,n_fft-hop)*/, float *carry_out /*dev (B,n_fft-hop)*/,
                        int final_, int64_t lo, int64_t hi, float *frames_ws /*dev or NULL*/,
                        float *out /*dev (B,hi-lo)*/, void *stream);

/* resample_poly core: x (B,L) -> out (B, n_out), n_out = ceil(L*up/down),
 *   out[b,o] = sum_i taps[t - up*i] * x[b,i],  t = (o + n_pre_remove)*down,
 * float32 accumulation in increasing i like SciPy's upfirdn (padtype "constant").
 * up/down must already be gcd-reduced (resample.py:255-257). */
int ap_resample_poly_f32(const float *x /*dev*/, int64_t B, int64_t L, int up, int down,
                         const float *taps /*dev*/, int n_taps, int n_pre_remove,
                         int64_t n_out, float *out /*dev*/, void *stream);

/* scipy.signal.resample_poly's other padtypes (the reference forwards `padtype` to SciPy,
 * resample.py:279-281).  AP_EXT_* are scipy.signal.upfirdn's extension modes; ap_extend_f32 writes
 * (B, L + 2 n_ext): n_ext extension samples either side of each row (bit-identical to SciPy's
 * _extend_left / _extend_right).  ap_resample_poly_padded_f32 = extension into `ws`
 * (B * (L + 2 * ap_resample_poly_pad_samples(up, down, n_taps)) floats) + the polyphase filter; mode
 * AP_EXT_CONSTANT needs no workspace and is ap_resample_poly_f32.  'mean' / 'median' / 'minimum' /
 * 'maximum' are host-side: subtract the row statistic, filter with zeros outside, add it back. */
#define AP_EXT_CONSTANT 0
#define AP_EXT_WRAP 1
#define AP_EXT_EDGE 2
#define AP_EXT_SMOOTH 3
#define AP_EXT_SYMMETRIC 4
#define AP_EXT_REFLECT 5
#define AP_EXT_ANTISYMMETRIC 6
#define AP_EXT_ANTIREFLECT 7
#define AP_EXT_LINE 8
int ap_extend_f32(const float *x /*dev*/, int64_t B, int64_t L, int64_t n_ext, int mode,
                  float *out /*dev (B, L + 2 n_ext)*/, void *stream);
int64_t ap_resample_poly_pad_samples(int up, int down, int n_taps);
int ap_resample_poly_padded_f32(const float *x /*dev*/, int64_t B, int64_t L, int up, int down,
                                const float *taps /*dev*/, int n_taps, int n_pre_remove, int64_t n_out,
                                int mode, float *ws /*dev*/, float *out /*dev*/, void *stream);

/* linear-interpolation resampler (resample.py:142-212): positions j*(L-1)/(n_out-1)
 * evaluated in float64 like the reference's NumPy code. */
int ap_resample_linear_f32(const float *x /*dev*/, int64_t B, int64_t L, int64_t n_out,
                           double scale, float *out /*dev*/, void *stream);

/* FFT resampler = scipy.signal.resample(x, num) for real float32 rows (reference
 * resample.py:97,123): complex FFT of length Nx (four-step, both legs in LDS), SciPy's
 * Nyquist-aware spectrum truncation / zero-padding, inverse FFT of length num, scale num/Nx.
 *   ap_cfft_split_host(N, &N1, &N2): N = N1*N2 with both <= 4096, -1 if the length cannot be
 *     split (then the call below returns AP_ERR_UNSUPPORTED);
 *   tw_* : twiddle tables (ap_twiddle_table_host) of the four leg lengths on the device;
 *   ws   : workspace of 2 * B * max(Nx, num) complex64 (= 16 * B * max(Nx,num) bytes). */
int ap_cfft_split_host(int64_t N, int *N1, int *N2);
int ap_resample_fft_f32(const float *x /*dev (B,Nx)*/, int64_t B, int64_t Nx, int64_t num,
                        const float *tw_x1, const float *tw_x2, const float *tw_y1,
                        const float *tw_y2 /*dev*/, float *ws /*dev*/, float *out /*dev (B,num)*/,
                        void *stream);

/* The same for lengths with a prime factor > 4096: either transform may run as a chirp-z (Bluestein)
 * convolution of a supported length M >= 2 N - 1 (a power of two).  Mx / My = 0 keeps the direct
 * four-step transform for that side (tw_*: legs of N); Mx / My > 0: tw_* are the leg tables of M,
 * chirp_* (N complex64) = exp(-i pi n^2 / N), spec_* (M complex64) = FFT_M of conj(chirp) laid out
 * circularly (b[n] = b[M - n] = conj(chirp[n])), both built on the host in float64.
 *   ws : 2 * B * max(Nx, num, Mx, My) complex64. */
int ap_resample_fft_chirp_f32(const float *x /*dev (B,Nx)*/, int64_t B, int64_t Nx, int64_t num,
                              int64_t Mx, const float *tw_x1, const float *tw_x2,
                              const float *chirp_x, const float *spec_x,
                              int64_t My, const float *tw_y1, const float *tw_y2,
                              const float *chirp_y, const float *spec_y /*dev*/,
                              float *ws /*dev*/, float *out /*dev (B,num)*/, void *stream);

/* magnitude / phase / |S|^p of a complex64 array of n elements —
 * stft.py:347-379 (mx.abs, mx.arctan2). */
int ap_magnitude_f32(const float *S /*dev*/, int64_t n, float *out /*dev*/, void *stream);
int ap_phase_f32(const float *S /*dev*/, int64_t n, float *out /*dev*/, void *stream);
/* The same two from a spectrum whose rows are `row_stride` complex values apart (ap_stft_rows_f32) into a dense
 * (rows, T) float array: mode 0 = |S|, mode 1 = atan2(im, re). */
int ap_complex_unary_rows_f32(const float *S /*dev (rows,row_stride,2)*/, int64_t rows, int64_t T, int64_t row_stride,
                              int mode, float *out /*dev (rows,T)*/, void *stream);

/* ---------------------------------------------------------------------- *
 * Tails of the hot path: Griffin-Lim projection, dB conversion, DCT (mfcc).
 * ---------------------------------------------------------------------- */

/* Griffin-Lim (griffinlim.py:123-178), element-wise over (B*F, T):
 *   mode 0: rebuilt = S * exp(i*angles) (and tprev = rebuilt if tprev != NULL)
 *   mode 1: R' = S * exp(i*atan2(R.im, R.re)); rebuilt = R' + momentum*(R' - tprev);
 *           tprev = R' (when momentum > 0).  R has TR frames per row; frames >= TR
 *           count as zero (the reference crops / zero-pads R to T, :156-165). */
int ap_gl_project_f32(int mode, const float *S /*dev (BF,T)*/, const float *angles /*dev*/,
                      const float *R /*dev (BF,TR,2)*/, int64_t TR, int64_t BF, int64_t T,
                      float momentum, float *tprev /*dev (BF,T,2)*/, float *rebuilt /*dev*/,
                      void *stream);

/* out[i] = float32(low + (high-low) * next_double_i) of NumPy's PCG64 stream whose CURRENT state
 * is (state, inc) as reported by numpy.random.default_rng(seed).bit_generator.state, split in
 * 64-bit halves — i.e. exactly default_rng(seed).uniform(low, high, n).astype(float32)
 * (reference griffinlim.py:112-115), generated on the device. */
int ap_pcg64_uniform_f32(uint64_t state_hi, uint64_t state_lo, uint64_t inc_hi, uint64_t inc_lo,
                         double low, double high, int64_t n, float *out /*dev*/, void *stream);

/* The whole Griffin-Lim loop (griffinlim.py:123-191) enqueued by ONE call: rebuilt = S*exp(i*angles);
 * n_iter x { istft -> stft -> project+momentum }; final istft.  All buffers are the caller's:
 *   rebuilt, tprev : (B,F,T) complex64 scratch      R : (B,F,TR) complex64 scratch, TR = frames of stft(y)
 *   frames_ws : (B,T,n_fft) float32                 y : (B, y_len) float32 = the result
 * out_offset / y_len are istft's trim (see ap_istft_f32); TR must equal 1 + (y_len + 2*pad - n_fft)/hop. */
int ap_griffinlim_f32(const float *S /*dev (B,F,T)*/, const float *angles /*dev (B,F,T)*/, int64_t B,
                      int64_t T, int n_fft, int hop, const float *window /*dev*/,
                      const float *tw /*dev*/, int center, int pad_mode, int64_t out_offset,
                      int64_t y_len, int64_t TR, int n_iter, float momentum, float *rebuilt,
                      float *tprev, float *R, float *frames_ws, float *y /*dev*/, void *stream);

/* The same loop with the three complex workspaces held in rows `row_stride` complex values apart
 * ((B, F, row_stride) each; row_stride even, >= T, ideally a multiple of 16 with 128-byte aligned buffers so
 * that every 16-frame group is one whole line per row).  n_fft = 2048, hop in {256, 512, 1024}, TR == T (the
 * stft of the y_len-sample signal has as many frames as S) - AP_ERR_UNSUPPORTED otherwise: use
 * ap_griffinlim_f32.  S and angles are dense (B, F, T).  No frames workspace: the istft is the fused kernel. */
int ap_griffinlim_rows_f32(const float *S /*dev (B,F,T)*/, const float *angles /*dev (B,F,T)*/, int64_t B,
                           int64_t T, int64_t row_stride, int n_fft, int hop, const float *window /*dev*/,
                           const float *tw /*dev*/, int center, int pad_mode, int64_t out_offset,
                           int64_t y_len, int n_iter, float momentum, float *rebuilt, float *tprev, float *R,
                           float *y /*dev*/, void *stream);

/* out[0] = mean((a - b)^2) over n floats, deterministic (float64 partial sums per workgroup, added in a fixed
 * order): the reconstruction error griffinlim_iter returns (griffinlim.py:268-269).  ws: scratch of
 * ap_mse_workspace_doubles() float64 values. */
int64_t ap_mse_workspace_doubles(void);
int ap_mse_f32(const float *a /*dev*/, const float *b /*dev*/, int64_t n, double *ws /*dev*/, float *out /*dev*/,
               void *stream);

/* max over n floats into *key_dev (uint32 order-preserving key; caller provides the
 * 4-byte word, the call resets it first).  Used for ref=max and by ap_to_db_f32. */
int ap_reduce_max_f32(const float *x /*dev*/, int64_t n, uint32_t *key_dev, void *stream);

/* _to_db (convert.py:14-60): out = coef*log10(max(S,amin)/max(ref,amin)), then if
 * top_db >= 0: out = max(out, GLOBAL max(out) - top_db).  ref = *ref_key_dev (a key from
 * ap_reduce_max_f32) when ref_key_dev != NULL, else ref_value.  ws_dev: 4-byte scratch.
 * The conversion is monotone, so the clip floor is dB(max(S)) - top_db: one read-only max
 * reduction of S, then a single read+write pass. */
int ap_to_db_f32(const float *S /*dev*/, int64_t n, float coef, float amin, float ref_value,
                 const uint32_t *ref_key_dev, float top_db, float *out /*dev*/,
                 uint32_t *ws_dev, void *stream);

/* db_to_power (div=10) / db_to_amplitude (div=20): ref * 10^(x/div) — convert.py:100-198 */
int ap_from_db_f32(const float *x /*dev*/, int64_t n, float ref, float div, float *out /*dev*/,
                   void *stream);

/* dct(x, n, axis, norm) — bindings.cpp:337-368, dct.cpp:103-159, mfcc.py:69-140:
 *   x viewed as (outer, n_in, inner); out[o,k,i] = row_scale[k] * sum_m C[k,m] x[o,m,i];
 *   C is the (n_out, n_in) basis (ap_dct_matrix_host); row_scale may be NULL (lifter,
 *   mfcc.py:277-282). */
int ap_dct_f32(const float *x /*dev*/, const float *C /*dev (n_out,n_in)*/,
               const float *row_scale /*dev or NULL*/, int64_t outer, int n_in, int64_t inner,
               int n_out, float *out /*dev*/, void *stream);

/* mfcc tail (mfcc.py:253-287): power_to_db (+ top_db clip against the global maximum) fused into
 * the DCT's loads: out[o,k,i] = row_scale[k] * sum_m C[k,m] * dB(S[o,m,i]).  The dB array is
 * never materialised.  Arguments as in ap_to_db_f32 and ap_dct_f32; n_in * 64 (n_out <= 16) or
 * n_in * 128 bytes must fit 64 KiB of LDS (AP_ERR_UNSUPPORTED otherwise: use the two calls). */
int ap_db_dct_f32(const float *S /*dev*/, const float *C /*dev (n_out,n_in)*/,
                  const float *row_scale /*dev or NULL*/, int64_t outer, int n_in, int64_t inner,
                  int n_out, float coef, float amin, float ref_value, const uint32_t *ref_key_dev,
                  float top_db, uint32_t *ws_dev, int max_ready /* *ws_dev already holds max(S) */,
                  float *out /*dev*/, void *stream);

/* ---------------------------------------------------------------------- *
 * Callers that sit directly on the STFT / on the frames.
 * ---------------------------------------------------------------------- */

/* spectral_centroid / spectral_bandwidth / spectral_rolloff / spectral_flatness —
 * features.py:57-442, bindings.cpp:371-484 (spectral.cpp:8-257).  One pass over a spectrogram
 * S (B, F, T): real magnitudes (is_complex = 0) or the complex STFT (is_complex = 1: |X| is taken
 * on load); `power` raises it (features.py:52-54).  Outputs are (B, T) rows; NULL = not wanted.
 *   centroid  = sum(f S) / (sum S + 1e-10)
 *   bandwidth = (sum(S |f - c|^p) / (sum S + 1e-10))^(1/p)   (norm = 0: without the normaliser);
 *               c = centroid_in (B, T) when given, else the centroid above
 *   rolloff   = freq of the first bin whose running sum of S reaches roll_percent * sum S
 *   flatness  = exp(mean log max(S, amin)) / (mean max(S, amin) + 1e-10) */
int ap_spectral_stats_f32(const float *S /*dev*/, int is_complex, int64_t B, int64_t F, int64_t T,
                          const float *freq /*dev (F)*/, float power, const float *centroid_in /*dev or NULL*/,
                          float p, int norm, float roll_percent, float amin, float *centroid /*dev or NULL*/,
                          float *bandwidth, float *rolloff, float *flatness, void *stream);

/* spectral_contrast (reference features.py:445-595): bands (n_bands, 3) int32 on the device = first bin, one past
 * the last bin, number of extreme values k of every octave band (host-built from the bin frequencies as the
 * reference does); out (B, n_bands, T) = mean of the k largest minus mean of the k smallest magnitudes of the band,
 * as 10 log10 differences unless `linear`. */
int ap_spectral_contrast_f32(const float *S /*dev (B,F,T)*/, int64_t B, int64_t F, int64_t T,
                             const int32_t *bands /*dev*/, int n_bands, int linear, float *out /*dev*/, void *stream);

/* The same statistics straight from the audio for n_fft = 2048 (reference features.py:24-55: every
 * feature call runs its own STFT first): transform, |X|^power and the per-frame reductions in ONE kernel,
 * the complex spectrum never reaches HBM.  ap_spectral_audio_fused: 1 when the shape is served (n_fft
 * 2048, center=False or constant padding with an even hop); otherwise use ap_stft_f32 + ap_spectral_stats_f32.
 * Arguments as ap_stft_f32 + ap_spectral_stats_f32 (no centroid_in). */
int ap_spectral_audio_fused(int64_t L, int n_fft, int hop, int center, int pad_mode);
int ap_spectral_audio_f32(const float *y /*dev (B,L)*/, int64_t B, int64_t L, int n_fft, int hop,
                          const float *window, const float *tw, int center, int pad_mode, int64_t T,
                          const float *freq /*dev (n_fft/2+1)*/, float power, float p, int norm,
                          float roll_percent, float amin, float *centroid, float *bandwidth,
                          float *rolloff, float *flatness /*dev (B,T) or NULL*/, void *stream);

/* rms(y, frame_length, hop_length, center, pad_mode) and zero_crossing_rate(...) —
 * framing.py:81-150, features.py:598-722: per frame sqrt(mean x^2) and the fraction of samples
 * i >= 1 of the frame with (x[i] >= 0) != (x[i-1] >= 0).  pad = frame_length / 2 if center else 0,
 * pad_mode AP_PAD_CONSTANT or AP_PAD_EDGE; T = 1 + (L + 2 pad - frame_length) / hop.  Outputs (B, T). */
int ap_frame_stats_f32(const float *y /*dev (B,L)*/, int64_t B, int64_t L, int frame_length, int hop,
                       int center, int pad_mode, int64_t T, float *rms /*dev or NULL*/,
                       float *zcr /*dev or NULL*/, void *stream);

/* preemphasis(y, coef, zi) — framing.py:154-296: out[n] = y[n] - coef y[n-1], out[0] = y[0] + zi[b]
 * (zi == NULL: 2 y[0] - y[1]); zf[b] = y[L-1] (NULL = not wanted). */
int ap_preemphasis_f32(const float *y /*dev (B,L)*/, int64_t B, int64_t L, float coef,
                       const float *zi /*dev (B) or NULL*/, float *out /*dev*/, float *zf /*dev (B) or NULL*/,
                       void *stream);

/* deemphasis(y, coef, zi) — framing.py:298-392 (scipy.signal.lfilter([1], [1, -coef])):
 * out[n] = y[n] + coef out[n-1], out[0] = y[0] + zi[b].  zi == NULL: zero state and the reference's
 * correction ((2-coef) y[0] - y[1]) / (3-coef) * coef^n subtracted.  zf[b] = coef * out[L-1] of the
 * uncorrected recursion (lfilter's final state). */
int ap_deemphasis_f32(const float *y /*dev (B,L)*/, int64_t B, int64_t L, float coef,
                      const float *zi /*dev (B) or NULL*/, float *out /*dev*/, float *zf /*dev (B) or NULL*/,
                      void *stream);
/* The same with a workspace of ap_deemphasis_workspace_floats(B, L) floats: clips longer than 16 384
 * samples are filtered in chunks on workgroups of their own (chunk end states first, then every chunk
 * from the composed state it is entered with).  ws = NULL (or a short clip): one workgroup per clip. */
int64_t ap_deemphasis_workspace_floats(int64_t B, int64_t L);
int ap_deemphasis_ws_f32(const float *y /*dev*/, int64_t B, int64_t L, float coef, const float *zi /*dev (B) or NULL*/,
                         float *out /*dev*/, float *zf /*dev (B) or NULL*/, float *ws /*dev*/, void *stream);

/* delta(data, width, order, axis, mode) — mfcc.py:290-368 = scipy.signal.savgol_filter: FIR along the
 * middle axis of x viewed as (outer, n, inner); taps (width) in correlation order; mode AP_SG_*;
 * edge: (2 * (width/2), width) rows for mode AP_SG_INTERP (polynomial fit of the first / last
 * `width` samples), else NULL. */
#define AP_SG_INTERP 0
#define AP_SG_NEAREST 1
#define AP_SG_MIRROR 2
#define AP_SG_CONSTANT 3
#define AP_SG_WRAP 4
int ap_savgol_f32(const float *x /*dev*/, int64_t outer, int64_t n, int64_t inner, const float *taps /*dev*/,
                  int width, int mode, float cval, const float *edge /*dev or NULL*/, float *out /*dev*/,
                  void *stream);

/* 16-bit PCM ingest (the reference assumes float arrays already in memory,
 * README.md:34-38): out = x * scale (scale = 1/32768 for full-scale [-1, 1)). */
int ap_pcm16_to_f32(const int16_t *x /*dev*/, int64_t n, float scale, float *out /*dev*/, void *stream);

/* melspectrogram straight from 16-bit PCM: same arguments as ap_melspec_max_f32 with y (B, L) int16.
 * Where the n_fft = 2048 run kernel applies (ap_melspec_pcm16_fused() != 0: constant padding or
 * center = 0, power 2, n_mels <= 128, even L / hop) the conversion rides on the kernel's sample
 * loads (half the HBM read bytes, no float copy of the batch); otherwise the samples are first
 * converted into scratch_f32 (B*L floats, required then) and the float path runs. */
int ap_melspec_pcm16_fused(int64_t L, int n_fft, int hop, int center, int pad_mode, int n_mels, float power,
                           const int32_t *desc /*host*/);
int ap_melspec_pcm16_f32(const int16_t *y /*dev (B,L)*/, int64_t B, int64_t L, int n_fft, int hop,
                         const float *window /*dev*/, const float *tw /*dev*/, int center, int pad_mode,
                         int64_t T, const float *fb /*dev*/, const int32_t *plan /*dev*/,
                         const int32_t *desc /*host*/, int n_mels, float power, float *out /*dev*/,
                         uint32_t *max_key /*dev or NULL*/, float *scratch_f32 /*dev (B,L) or NULL*/, void *stream);

/* autocorrelation(y, max_lag, normalize, center) — pitch.py:16-115, bindings.cpp:224-252
 * (autocorrelation.cpp:10-84): r = irfft(|rfft(y - mean(y), n_fft)|^2)[:max_lag], divided by
 * max(r[0], 1e-10) when normalize; n_fft = ap_autocorrelation_nfft(n) = the next power of two
 * >= 2 n - 1 = N1 * N2 (ap_cfft_split_host).  tw1 / tw2: twiddle tables of the two legs
 * (ap_twiddle_table_host(N1), (N2)); ws: 4 B n_fft + B floats of scratch; out: (B, max_lag). */
int64_t ap_autocorrelation_nfft(int64_t n);
int ap_autocorrelation_f32(const float *y /*dev (B,n)*/, int64_t B, int64_t n, int64_t max_lag, int normalize,
                           int center, const float *tw1 /*dev*/, const float *tw2 /*dev*/, float *ws /*dev*/,
                           float *out /*dev*/, void *stream);

/* pitch_detect_acf / periodicity (reference pitch.py:118-369) from the raw autocorrelation r (rows, n_lag) of
 * every centred frame: on r / r[0] over the lags min_lag .. max_lag the first local maximum above `threshold`
 * (else the global maximum, if above it) gives f0 = sr / lag and voiced = 1; periodicity = the maximum.
 * Rows with r[0] <= 1e-10 stay 0.  Any of the three outputs may be NULL. */
int ap_acf_peaks_f32(const float *r /*dev*/, int64_t rows, int n_lag, int min_lag, int max_lag,
                     float threshold, float sr, float *f0 /*dev (rows)*/,
                     unsigned char *voiced /*dev (rows)*/, float *periodicity /*dev (rows)*/, void *stream);

/* yin / yin_cmnd (pitch.py; de Cheveigne & Kawahara 2002).  Frames of frame_length = n (even, 4 .. 8192) every
 * `hop` samples, T = ap_n_frames of stft (center: n / 2 zeros on both sides); with W = n / 2 and the lags
 * 1 <= lo < hi <= n - W - 1:
 *   d(tau) = sum_{j<W} (x[j] - x[j + tau])^2,  d'(0) = 1,  d'(tau) = d(tau) tau / sum_{k=1..tau} d(k)
 *   (1 where that sum is 0; no absolute floor: d' is invariant under scaling of y).
 * ap_yin_cmnd_f32 stores d'(lo .. hi) as out (B, hi - lo + 1, T).  ap_yin_f32 picks on that curve the first lag
 * with d' < trough_threshold that is below its left and not above its right neighbour (values outside the curve
 * count as +inf), else the first global minimum; interior picks are refined by the parabola through the three
 * values; f0 = sr / lag (B, T), aper (optional) = d' at the picked integer lag.
 * tw selects the kernel: the twiddle table of ap_twiddle_table_host(n) asks for the fused wave-per-frame kernel
 * (three on-chip n-point transforms per frame; AP_ERR_UNSUPPORTED when ap_yin_fused(n, hop, L) == 0, i.e. unless
 * n = 2048 or 1024, hop even, L <= 2^28); NULL runs the general kernel (one workgroup per frame, direct sums, any n). */
int ap_yin_fused(int frame_length, int hop, int64_t L);
int ap_yin_f32(const float *y /*dev (B,L)*/, int64_t B, int64_t L, int frame_length, int hop, int center, int lo,
               int hi, float sr, float trough_threshold, const float *tw /*dev or NULL*/, float *f0 /*dev (B,T)*/,
               float *aper /*dev (B,T) or NULL*/, void *stream);
int ap_yin_cmnd_f32(const float *y /*dev (B,L)*/, int64_t B, int64_t L, int frame_length, int hop, int center,
                    int lo, int hi, const float *tw /*dev or NULL*/, float *out /*dev (B,hi-lo+1,T)*/, void *stream);

/* hpss / hpss_medians (decompose.py; Fitzgerald 2010, librosa.decompose.hpss).  S: (B, F, T) float32, or complex
 * pairs when is_complex, rows row_stride_in elements apart (>= T; the padding is never read).  With M = |S| (S itself
 * when real):
 *   harm[b,f,t] = element of rank k_harm / 2 (0-based, ascending) of M[b, f, r(t - k_harm/2 + j, T)], j < k_harm
 *   perc[b,f,t] = the same along f with k_perc and r(., F)
 *   r(i, n) = i mod 2n, mirrored as 2n - 1 - i when that is >= n  (scipy.ndimage mode="reflect")
 *   softmask(X, R) = 0.5 (both margins 1) or 0 where max(X, R) < FLT_MIN, else with Z = max(X, R):
 *                    (X/Z)^power / ((X/Z)^power + (R/Z)^power);  power = INFINITY: X > R as 0 / 1
 *   mask_h = softmask(harm, perc * margin_harm),  mask_p = softmask(perc, harm * margin_perc)
 * mode 0 stores the components S * mask_h, S * mask_p (of S's kind: complex pairs for a complex S), mode 1 the two
 * masks, mode 2 the two medians (real); rows of the outputs are row_stride_out elements apart (>= T; the padding is
 * never written).  Either output may be NULL (then it is not computed), not both.  k_harm, k_perc in 1 .. 255;
 * ap_hpss_fused(k_harm, k_perc) != 0 (for (31, 31)) says the comparator-network kernel serves the sizes; general != 0
 * forces the rank-counting kernel, which serves every size and returns the same bits.  Results are defined for finite,
 * non-negative M.  AP_ERR_INVALID: sizes, strides, margins < 1, power <= 0, an output overlapping S or the other
 * output; AP_ERR_UNSUPPORTED: F or T beyond 2^28, more than 2^31 - 1 tiles. */
int ap_hpss_fused(int k_harm, int k_perc);
int ap_hpss_f32(const float *S /*dev*/, int is_complex, int64_t B, int64_t F, int64_t T, int64_t row_stride_in,
                int k_harm, int k_perc, float margin_harm, float margin_perc, float power, int mode, int general,
                float *out_h /*dev or NULL*/, float *out_p /*dev or NULL*/, int64_t row_stride_out, void *stream);

/* onset_strength (onset.py; librosa.onset.onset_strength).  S: (B, M, T) float32, rows row_stride elements apart
 * (>= T; the padding is never read); ref: NULL or an array of the same shape, rows ref_row_stride apart.
 *   R[b,m,t] = ref[b,m,t], or without ref the maximum of S[b, r(j, M), t] over j in [m - max_size/2, m + (max_size-1)/2]
 *              (r: SciPy's mode="reflect"; scipy.ndimage.maximum_filter1d along m; max_size in 1 .. 255, 1: S itself)
 *   flux[b,u] = (1 / M) sum_m max(0, S[b, m, u + lag] - R[b, m, u]),   0 <= u < T - lag
 *   out[b,t]  = flux[b, t - shift] for shift <= t < T, 0 for t < shift   (shift >= lag >= 1; out rows out_row_stride apart)
 * db_mode != 0: S holds power and every value of S is replaced on load by
 *   max(db_coef log10(max(s, db_amin) / max(db_ref, db_amin)), floor),  floor = that of max(S) - db_top_db
 * with max(S) read from *smax_key (the order-preserving key ap_melspec_max_f32 / ap_reduce_max_f32 leave; db_top_db < 0:
 * no floor): the values ap_to_db_f32 would store, bit for bit.  ref is never converted.  Results are defined for finite S.
 * AP_ERR_INVALID: sizes, lag, max_size, shift < lag, strides, an output overlapping an input; AP_ERR_UNSUPPORTED: M or T
 * beyond 2^28, more than 2^31 - 1 tiles of 64 frames. */
int ap_onset_strength_f32(const float *S /*dev*/, int64_t B, int64_t M, int64_t T, int64_t row_stride,
                          const float *ref /*dev or NULL*/, int64_t ref_row_stride, int lag, int max_size, int shift,
                          int db_mode, float db_coef, float db_amin, float db_ref, float db_top_db,
                          const uint32_t *smax_key /*dev or NULL*/, float *out /*dev (B,T)*/, int64_t out_row_stride,
                          void *stream);

/* peak_pick / onset_detect (onset.py; librosa.util.peak_pick, librosa.onset.onset_detect).  x: (B, T) float32, rows
 * row_stride apart, T <= ap_peak_pick_max_frames() (AP_ERR_UNSUPPORTED beyond).  Per row, in one launch:
 *   normalize != 0: x = (x - min x) / (max x - min x + FLT_MIN)
 *   candidates: x[n] == max x[max(0, n - pre_max) : min(n + post_max, T)] and
 *               x[n] >= mean x[max(0, n - pre_avg) : min(n + post_avg, T)] + delta   (float32 sum in index order)
 *   kept, from the left: a candidate more than `wait` frames after the last kept one
 *   backtrack != 0: a kept frame n moves to the largest k <= n with k = 0, or 1 <= k <= T - 2 and e[k] <= e[k-1] and
 *               e[k] < e[k+1]; e = energy (rows energy_row_stride apart), or the values the candidates saw when NULL
 *   guard != 0: a row that is all zero or holds a non-finite value keeps nothing (onset_detect)
 * out_mask (B, T): 1 at the kept (moved) frames, 0 elsewhere; out_count (B) or NULL: the ones per row.
 * pre_max, pre_avg, wait >= 0; post_max, post_avg >= 1. */
int ap_peak_pick_max_frames(void);
int ap_peak_pick_f32(const float *x /*dev*/, int64_t B, int64_t T, int64_t row_stride, int pre_max, int post_max,
                     int pre_avg, int post_avg, float delta, int wait, int normalize, int guard, int backtrack,
                     const float *energy /*dev or NULL*/, int64_t energy_row_stride, unsigned char *out_mask /*dev*/,
                     int32_t *out_count /*dev or NULL*/, void *stream);

/* tempogram (rhythm.py; librosa.feature.tempogram): the windowed autocorrelation of an onset envelope per frame.
 * env: (B, n) float32, rows row_stride apart; window: (W) on the device, W = win_length <= ap_tempogram_max_win()
 * (AP_ERR_UNSUPPORTED beyond); h = W / 2.
 *   center != 0: p = env between two linear ramps of h values, e[0] i / h and e[n-1] (h - 1 - j) / h (computed on load,
 *                no padded copy), T = n;  center == 0: p = env, T = n - W + 1 (AP_ERR_INVALID when n < W)
 *   x_t[i] = w[i] p[t + i];  ac[k, t] = sum_{i < W - k} x_t[i] x_t[i + k], 0 <= k < W, i ascending
 *   norm != 0: tg = ac / max_k |ac[k, t]| per frame (left alone where that maximum is below FLT_MIN);  norm == 0: tg = ac
 * out (B, W, T) or NULL: tg.  agg or NULL: ap_tempogram_agg_floats(B, n, W, center) floats, (B, ceil(T / 64), W):
 * sum_t tg[k, t] over the 64 frames of every tile, added in frame order - what ap_tempo_pick_f32 joins into the mean
 * without the tempogram ever being stored.  At least one of the two.
 * tw selects the kernel: the twiddle table of ap_twiddle_table_host(1024) asks for the wave-per-frame kernel (W windowed
 * values zero-padded to a 1024-point real transform, |A|^2, inverse: two on-chip transforms per frame; AP_ERR_UNSUPPORTED
 * when ap_tempogram_fused(W) == 0, i.e. W > 512); NULL runs the general kernel (direct sums in float64, any W). */
int ap_tempogram_max_win(void);
int ap_tempogram_fused(int win_length);
int64_t ap_tempogram_agg_floats(int64_t B, int64_t n, int win_length, int center);
int ap_tempogram_f32(const float *env /*dev*/, int64_t B, int64_t n, int64_t row_stride, const float *window /*dev (W)*/,
                     int win_length, int center, int norm, const float *tw /*dev or NULL*/, float *out /*dev or NULL*/,
                     float *agg /*dev or NULL*/, void *stream);

/* tempo (rhythm.py; librosa.feature.tempo): per column c of clip b, with
 *   g[k] = (sum_{r < n_red} G[b clip_stride + k lag_stride + c col_stride + r red_stride]) / div      (r ascending)
 * out_idx[b n_col + c] = the first k in 0 .. n_lags - 1 maximising log1p(1e6 g[k]) + logprior[k].  The strides serve
 * the tile sums of ap_tempogram_f32 (n_red tiles, div = T), a stored tempogram's mean over frames (n_red = T,
 * red_stride = 1, div = T) and its single frames (n_col = T, n_red = 1, div = 1). */
int ap_tempo_pick_f32(const float *g /*dev*/, int64_t B, int64_t n_col, int n_lags, int64_t clip_stride, int64_t lag_stride,
                      int64_t col_stride, int64_t n_red, int64_t red_stride, float div, const float *logprior /*dev (n_lags)*/,
                      int32_t *out_idx /*dev (B, n_col)*/, void *stream);

/* beat_track (rhythm.py; librosa.beat.beat_track, Ellis 2007).  env: (B, T) float32, rows row_stride apart,
 * T <= ap_beat_track_max_frames() (AP_ERR_UNSUPPORTED beyond); period (B) on the device: the beat period P of every row
 * in frames.  Per row, one workgroup, with h = rint(P / 2) (halves to even):
 *   o'[i]   = o[i] / std(o, ddof = 1)
 *   L[i]    = sum_{k = -P .. P} exp(-0.5 (32 k / P)^2) o'[i - k]                    (o' = 0 outside the row)
 *   C[i]    = L[i] + max_{d = 2P, 2P - 1, .., h} (-tightness ln(d / P)^2 + C[i - d]),  C[j] = 0 for j < 0
 *   link[i] = i - d of the first maximum in that order; -1 while no frame j <= i has had L[j] >= 0.01 max(L)
 *   M[i]    = C[i] > C[i-1] and C[i] >= C[i+1] (M[0] = 0, M[T-1] = C[T-1] > C[T-2])
 *   tail    = the largest i with M[i] and 2 C[i] > median{C[j] : M[j]};  beats = tail, link[tail], .. while >= 0, reversed
 *   s[j]    = 0.5 L[b[j-1]] + L[b[j]] + 0.5 L[b[j+1]];  kept: b[lo .. hi], lo / hi the first / last j with
 *             s[j] > (trim ? 0.5 sqrt(mean s^2) : 0), both inclusive
 * A row that is all zero, holds a non-finite value, has zero deviation or T < 2, has no M[i] or no s[j] above the
 * threshold keeps nothing.  out_mask (B, T): 1 at the kept beats; out_count (B): their number, or -1 (and no beats) for
 * a row whose period lies outside 2 .. ap_beat_track_max_period().  out_L, out_C, out_link (B, T) or NULL: the
 * intermediates (0, 0, -1 for a row that keeps nothing before the dynamic programme). */
int ap_beat_track_max_frames(void);
int ap_beat_track_max_period(void);
int ap_beat_track_f32(const float *env /*dev*/, int64_t B, int64_t T, int64_t row_stride, const int32_t *period /*dev (B)*/,
                      float tightness, int trim, unsigned char *out_mask /*dev*/, int32_t *out_count /*dev*/,
                      float *out_L /*dev or NULL*/, float *out_C /*dev or NULL*/, int32_t *out_link /*dev or NULL*/,
                      void *stream);

/* pcen (pcen.py, streaming.py: StreamingPCEN; librosa.pcen, Wang et al. 2017).  S: (B, M, T) float32 >= 0, rows
 * row_stride elements apart (>= T; the padding is never read); ref: NULL or an array of the same shape, rows
 * ref_row_stride apart; out: the same shape, rows out_row_stride apart (the padding is never written).  With a = 1 - b:
 *   R[b,m,t] = ref[b,m,t], or without ref the maximum of S[b, r(j, M), t] over j in [m - max_size/2, m + (max_size-1)/2]
 *              (r: SciPy's mode="reflect"; scipy.ndimage.maximum_filter1d along m; max_size in 1 .. 255, 1: S itself)
 *   Msm[t]   = b R[t] + a Msm[t-1],  a Msm[-1] = zi[b M + m]  (NULL: 1 - b, the steady state of a unit input, for every row)
 *   smooth   = (eps + Msm)^-gain
 *   out      = (S smooth + bias)^power - bias^power, evaluated as bias^power expm1(power log1p(S smooth / bias));
 *              log1p(S smooth) when power = 0; (S smooth)^power when bias = 0
 *   zf[b M + m] = a Msm[T-1]  (NULL: not wanted): the zi of the call that continues the rows
 * b crosses as a double: the float32 powers a^k, k <= 64, that the kernel's scan multiplies by are rounded from float64
 * powers.  One launch, one read of S (and ref) and one write of out; results are defined for finite S >= 0.
 * AP_ERR_INVALID: sizes, b outside [0, 1], b = 0 without zi, negative gain / bias / power, eps below FLT_MIN, max_size, strides,
 * an output overlapping an input; AP_ERR_UNSUPPORTED: M or T beyond 2^28. */
int ap_pcen_f32(const float *S /*dev*/, int64_t B, int64_t M, int64_t T, int64_t row_stride,
                const float *ref /*dev or NULL*/, int64_t ref_row_stride, int max_size, double b, float gain, float bias,
                float power, float eps, const float *zi /*dev (B*M) or NULL*/, float *out /*dev*/, int64_t out_row_stride,
                float *zf /*dev (B*M) or NULL*/, void *stream);

/* cqt / vqt (cqt.py; the filter bank of librosa 0.10's cqt / vqt in direct form).  y: (B, L) float32; taps: the n_bins
 * complex filters back to back as (re, im) pairs, filter k at taps[tap_offset[k] .. tap_offset[k+1]), its first tap at
 * position m0[k] relative to the frame's centre; T = 1 + L / hop (AP_ERR_INVALID otherwise).
 *   C[b,k,t] = scale[k] sum_{j < L_k} ypad[b, t hop + m0[k] + j] conj(taps[tap_offset[k] + j]),  L_k = tap_offset[k+1] - tap_offset[k]
 *   ypad: y outside [0, L) by pad_mode (AP_PAD_CONSTANT, AP_PAD_EDGE, AP_PAD_REFLECT: NumPy's "reflect" at any distance),
 *   computed on load.
 * out: (B, n_bins, T) complex64 as (re, im) pairs, rows out_row_stride complex values apart (>= T; the padding is never
 * written).  tap_offset, m0, scale and taps are device arrays; the caller keeps 0 <= L_k <= ap_cqt_max_taps() and
 * |m0[k]| <= ap_cqt_max_taps().  One launch; every product is a fused multiply-add and every sum has a fixed order
 * (csrc/kernels_cqt.h).  AP_ERR_INVALID: sizes, hop, pad_mode, T, the stride; AP_ERR_UNSUPPORTED: L > 2^30. */
int ap_cqt_max_taps(void);
int ap_cqt_f32(const float *y /*dev*/, int64_t B, int64_t L, int hop, int pad_mode, const float *taps /*dev, float2*/,
               const int64_t *tap_offset /*dev (n_bins+1)*/, const int32_t *m0 /*dev (n_bins)*/,
               const float *scale /*dev (n_bins)*/, int n_bins, int64_t T, float *out /*dev*/, int64_t out_row_stride,
               void *stream);

/* chroma_stft / chroma_cqt / tonnetz (chroma.py): fold a spectrum onto n_out rows, threshold and normalise, one pass.
 * x: (B, K, T), rows in_row_stride elements apart (>= T), clips K rows apart; in_kind 0: float32, v = x; 1: complex64
 * as (re, im), v = |z|; 2: complex64, v = re^2 + im^2.  w: (n_out, K) row-major on the device, or NULL for the identity
 * (then K == n_out).  Per frame, in this order:
 *   a_c = sum_k w[c,k] v_k;  pre_l1: a_c /= max(sum_k |v_k|, -> 1 below FLT_MIN);  use_threshold: a_c < threshold -> 0;
 *   norm 0: none, 1: sum |a|, 2: sqrt(sum a^2), 3: max |a|, a norm below FLT_MIN counts as 1;  out_c = a_c / norm.
 * out: (B, n_out, T) float32, rows out_row_stride apart (>= T; the padding is never written).  One read of x, one write
 * of out; every product is a fused multiply-add, every sum has a fixed order, sqrt and / are IEEE (csrc/kernels_chroma.h):
 * a frame's bits do not depend on the batch.  A NaN stays in its frame.  AP_ERR_INVALID: NULL x / out, sizes, n_out above
 * ap_chroma_max_out(), a stride below T, an unknown in_kind or norm, w == NULL with K != n_out. */
int ap_chroma_max_out(void);
int ap_chroma_fold_f32(const float *x /*dev*/, int in_kind, int64_t B, int K, int64_t T, int64_t in_row_stride,
                       const float *w /*dev (n_out*K) or NULL*/, int n_out, int pre_l1, int use_threshold, float threshold,
                       int norm, float *out /*dev*/, int64_t out_row_stride, void *stream);

/* chroma_cens (chroma.py): chroma (B, n, T) float32, rows in_row_stride apart.  Per frame: L1-normalise (rule above),
 * quantise q = 0.25 ([v > 0.4] + [v > 0.2] + [v > 0.1] + [v > 0.05]); along time, when n_taps > 0,
 * s[t] = sum_j taps[j] q[t + (n_taps - 1) / 2 - j] with q = 0 outside [0, T) (SciPy's "same"); then normalise by `norm`
 * as above.  One launch, the quantised values stay in LDS.  n <= ap_chroma_max_out(), n_taps <= ap_chroma_max_smooth(). */
int ap_chroma_max_smooth(void);
int ap_chroma_cens_f32(const float *chroma /*dev*/, int64_t B, int n, int64_t T, int64_t in_row_stride,
                       const float *taps /*dev (n_taps) or NULL*/, int n_taps, int norm, float *out /*dev*/,
                       int64_t out_row_stride, void *stream);

/* dtw / dtw_backtracking (dtw.py): dynamic time warping, the definition of DESIGN.md 9.9 (csrc/kernels_dtw.h).
 * Caps: d <= ap_dtw_max_features(), n_steps <= ap_dtw_max_steps(), a step's components <= ap_dtw_max_step(),
 * N, M <= ap_dtw_max_len().  AP_ERR_INVALID: NULL buffers, empty sizes, a stride below the row length, an unknown metric,
 * a step with a negative component or (0, 0); AP_ERR_UNSUPPORTED: a size or a step component above its cap.
 *
 * ap_dtw_cost_f32: X (B, d, N) and Y (B, d, M) float32, rows x_row_stride / y_row_stride apart, pairs d rows apart;
 * C (B, N, M), rows c_row_stride apart.  metric 0: sqrt(sum (x - y)^2), 1: sum (x - y)^2, 2: sum |x - y|,
 * 3: 1 - x.y / (|x| |y|) with a product of norms below FLT_MIN counted as 1.  Features summed in ascending order.
 *
 * ap_dtw_accumulate_f32: steps_ab (host, n_steps pairs (a, b)), weights_add / weights_mul (host, n_steps), taken by
 * value.  use_band: cells with not (-band_r - max(N - M, 0) < j - i < band_r + max(M - N, 0)) cost +inf (a predicate,
 * C is not copied).  D (B, N, M) float32 and steps (B, N, M) uint8 (the winning step, 254: the path starts here, 255:
 * unreachable), rows d_row_stride / steps_row_stride apart.  One launch per tile-anti-diagonal on `stream`.  Every
 * addition and multiplication is rounded on its own and the comparison is the strict <: the bits of D and steps depend
 * on nothing but C and the arguments.  Nothing outside the N x M payload of a row is read or written.
 *
 * ap_dtw_backtrack_i32: follows steps from (N - 1, j0) until a cell with code 254; j0 = start[b] when start is given,
 * else the first minimum of D's last row when subseq (D may be NULL otherwise), else M - 1.  path (B, N + M - 1, 2)
 * int32 holds (i, j) from the end of the path to its start, len (B) the number of cells or -1 when there is no path. */
int ap_dtw_max_features(void);
int ap_dtw_max_steps(void);
int ap_dtw_max_step(void);
int ap_dtw_max_len(void);
int ap_dtw_cost_f32(const float *X /*dev*/, const float *Y /*dev*/, int64_t B, int d, int64_t N, int64_t M, int64_t x_row_stride,
                    int64_t y_row_stride, int metric, float *C /*dev*/, int64_t c_row_stride, void *stream);
int ap_dtw_accumulate_f32(const float *C /*dev*/, int64_t B, int64_t N, int64_t M, int64_t c_row_stride, int n_steps,
                          const int32_t *steps_ab /*host (2 n_steps)*/, const float *weights_add /*host*/,
                          const float *weights_mul /*host*/, int subseq, int use_band, int64_t band_r, float *D /*dev*/,
                          int64_t d_row_stride, uint8_t *steps /*dev*/, int64_t steps_row_stride, void *stream);
int ap_dtw_backtrack_i32(const float *D /*dev or NULL*/, const uint8_t *steps /*dev*/, const int32_t *start /*dev (B) or NULL*/,
                         int64_t B, int64_t N, int64_t M, int64_t d_row_stride, int64_t steps_row_stride, int n_steps,
                         const int32_t *steps_ab /*host (2 n_steps)*/, int subseq, int32_t *path /*dev*/, int32_t *len /*dev*/,
                         void *stream);

/* recurrence_matrix / cross_similarity / recurrence_to_lag / lag_to_recurrence (segment.py): k-nearest-neighbour
 * matrices, the definition of DESIGN.md 9.11 (csrc/kernels_segment.h).  ref (B, d, n_ref) and data (B, d, n) float32, rows
 * ref_row_stride / data_row_stride apart; D[i, j] = metric(ref[:, i], data[:, j]) with the metrics and the bits of the
 * DTW cost kernel; D is never stored.  Caps: d as for DTW, n and n_ref <= ap_segment_max_len().  Frame i is eligible
 * for query j when |i - j| >= width (width > 0 needs n_ref == n) and D[i, j] is no NaN.
 *
 * ap_segment_threshold_f32: records (B, n, 2) of 32-bit words: the bits of tau_j, the k-th smallest eligible distance of
 * query j (k clipped to the eligible frames), and t_j (int32), the largest index admitted among the frames tied at
 * tau_j; (NaN, -1) when no frame is eligible.  Frame i is a neighbour of j when (D[i, j], i) <= (tau_j, t_j).
 *
 * ap_segment_bandwidth_f32: bw (B) float32 from tau_j over the queries with t_j >= 0: kind 0 their median (an even
 * count: fl(fl(a + b) 0.5f) of the middle two), 1 their mean, 2 their geometric mean (float64 sums in a fixed order,
 * rounded once); NaN when no query has a neighbour.
 *
 * ap_segment_write_f32: out (B, n_ref, n), rows out_row_stride apart, uint8 for mode 0 (connectivity: 1), float32 for
 * mode 1 (distance: D) and 2 (affinity: 2^(D fl32(-log2(e) / bw)), bw = bw[b] (dev) when given, else `bandwidth`); 0
 * where i is no neighbour of j.  full: every eligible frame counts as one.  sym (n_ref == n): also j must be a
 * neighbour of i.  self_diag (n_ref == n), applied last: the diagonal is 1 (modes 0, 2) or 0 (mode 1).  Every cell of
 * the payload is written once, nothing behind a row's n columns.
 *
 * ap_segment_lag: elements of elem_bytes (1 or 4).  to_lag: in (B, n, n), out (B, t_lag, n), t_lag = n or 2 n,
 * out[(i - j) mod t_lag, j] = in[i, j], 0 in the rows no i maps to; else in (B, t_lag, n), out (B, n, n),
 * out[i, j] = in[(i - j) mod t_lag, j]. */
int ap_segment_max_len(void);
int ap_segment_threshold_f32(const float *ref /*dev*/, const float *data /*dev*/, int64_t B, int d, int64_t n_ref, int64_t n,
                             int64_t ref_row_stride, int64_t data_row_stride, int metric, int64_t k, int64_t width,
                             uint32_t *records /*dev*/, void *stream);
int ap_segment_bandwidth_f32(const uint32_t *records /*dev*/, int64_t B, int64_t n, int kind, float *bw /*dev*/, void *stream);
int ap_segment_write_f32(const float *ref /*dev*/, const float *data /*dev*/, int64_t B, int d, int64_t n_ref, int64_t n,
                         int64_t ref_row_stride, int64_t data_row_stride, int metric, int mode, int64_t width, int full, int sym,
                         int self_diag, const uint32_t *records /*dev*/, const float *bw /*dev (B) or NULL*/, double bandwidth,
                         void *out /*dev*/, int64_t out_row_stride, void *stream);
int ap_segment_lag(const void *in /*dev*/, int64_t B, int64_t n, int64_t t_lag, int elem_bytes, int to_lag, int64_t in_row_stride,
                   void *out /*dev*/, int64_t out_row_stride, void *stream);

/* viterbi / viterbi_discriminative / viterbi_binary (sequence.py): hidden-Markov decoding, the definition of DESIGN.md 9.12
 * (csrc/kernels_viterbi.h).  Caps: S <= ap_viterbi_max_states() for the dense decode, T <= ap_viterbi_max_steps().
 * AP_ERR_INVALID: NULL buffers, empty sizes, a stride below the row length, an unknown mode; AP_ERR_UNSUPPORTED: a size
 * above its cap.  Nothing is allocated and nothing synchronises.
 *
 * ap_viterbi_emission_f32: prob (B, S, T) float32, rows row_stride apart (the padding is never read), sequences S rows
 * apart.  With tiny = FLT_MIN: mode 0: E (B, T, S) = logf(p + tiny); mode 1: the same minus lps[j], lps (S) the float32 log
 * state priors; mode 2: E (B, T, S, 2) with [.., 1] = logf(p + tiny) - lps[l, 1] and [.., 0] = logf((1 - p) + tiny) - lps[l, 0],
 * lps (S, 2).  flags (B) int32 is cleared on `stream` and takes bit 0 for a sequence with a NaN or a value outside [0, 1],
 * bit 1 (mode 1) for one with a column whose sum is not within 1e-8 + 1e-5 of 1.
 *
 * ap_viterbi_decode_f32: E (B, T, S), lt (S, S) the float32 log transitions [from, to], li (S) the log initial
 * distribution.  v_0 = E_0 + li; at step t >= 1 ptr[t, j] is the smallest i that maximises v[i] + lt[i, j] and
 * v'[j] = E[t, j] + that maximum; after every step, step 0 included, m = max v is subtracted from v and added, in time
 * order, to a float64 sum.  The last state is the first maximum of the final v, states[t] = ptr[t + 1, states[t + 1]],
 * logp = the sum + v[states[T - 1]].  ptr (B, T, S) uint16 is scratch the caller provides (row 0 is written as 0),
 * states (B, T) int32, logp (B) float64.  Every addition is one rounded float32 operation: the outputs depend on nothing
 * but E, lt and li.
 *
 * ap_viterbi_binary_f32: S independent two-state chains per sequence on E (B, T, S, 2): lt (4) shared, or (S, 4) with
 * per_label, as [from][to]; li (S, 2).  The recursion of the dense decode; bits (B, ceil(T / 16), S) uint32 is scratch
 * (two pointer bits per step), states (B, S, T) int32, logp (B, S) float64. */
int ap_viterbi_max_states(void);
int ap_viterbi_max_steps(void);
int ap_viterbi_emission_f32(const float *prob /*dev*/, int64_t B, int64_t S, int64_t T, int64_t row_stride, int mode,
                            const float *lps /*dev or NULL*/, float *E /*dev*/, int32_t *flags /*dev (B)*/, void *stream);
int ap_viterbi_decode_f32(const float *E /*dev*/, int64_t B, int64_t S, int64_t T, const float *lt /*dev*/, const float *li /*dev*/,
                          uint16_t *ptr /*dev*/, int32_t *states /*dev*/, double *logp /*dev*/, void *stream);
int ap_viterbi_binary_f32(const float *E /*dev*/, int64_t B, int64_t S, int64_t T, const float *lt /*dev*/, int per_label,
                          const float *li /*dev*/, uint32_t *bits /*dev*/, int32_t *states /*dev*/, double *logp /*dev*/, void *stream);

/* piptrack / estimate_tuning / pitch_tuning (pitch.py): the definition of DESIGN.md 9.10 (csrc/kernels_piptrack.h).
 * S: (B, F, T) magnitudes, rows in_row_stride elements apart (>= T; the padding is never read), clips F rows apart;
 * in_kind 0: float32, 1: complex64 as (re, im), |z| = sqrtf(fmaf(im, im, re re)) taken on load.  Per frame, with
 * a, b, c = S[k-1], S[k], S[k+1], every operation rounded on its own:
 *   avg = 0.5 (c - a);  den = (2 b - c) - a;  shift = avg / (den + (|den| < FLT_MIN ? 1 : 0));  avg = shift = 0 at k = F - 1
 *   ref_value = threshold max_k S[k] (ref_mode 0), ref_value as given (1), |ref[b, t]| (2; ref (B, T) dense)
 *   X[k] = S[k] > ref_value ? S[k] : 0;  peak(k) = X[k] > X[k-1] and X[k] >= X[min(k+1, F-1)] and max(k_lo, 1) <= k < k_hi
 *   pitch = peak ? ((float)k + shift) bin_hz : 0;  magnitude = peak ? S[k] + (0.5 avg) shift : 0
 * ap_piptrack_f32 writes pitches and magnitudes (B, F, T) float32, rows out_row_stride apart (the padding is never
 * written).  ap_piptrack_records_f32 writes nothing dense: every peak with pitch > 0 leaves the pair (magnitude, pitch) in
 * records (G, capacity, 2), G = per_clip ? B : 1, in no particular order, and counters[g] (zeroed by the call) ends as
 * the number of peaks of group g whether they fitted or not (records beyond capacity are dropped).
 * AP_ERR_INVALID: NULL buffers, empty sizes, F < 2, strides, k_lo / k_hi outside 0 <= k_lo <= k_hi <= F, a negative
 * threshold, unknown in_kind / ref_mode; AP_ERR_UNSUPPORTED: capacity above ap_piptrack_max_records().
 *
 * ap_piptrack_tuning_f32: per group with n = counters[g] <= capacity records (a group with more is left untouched):
 * threshold_out[g] = the float32 median of the magnitudes (odd n: the order statistic n / 2; even n: (m[n/2 - 1] +
 * m[n/2]) 0.5f; n = 0: 0), found exactly by a radix select; counts (G, n_bins): the histogram of the residuals
 *   r = fmod(bins_per_octave log2((double)pitch / 27.5), 1) taken into [-0.5, 0.5), in float64,
 * of the records with magnitude >= threshold, over the bins edges[i] <= r < edges[i+1] (edges: device, n_bins + 1
 * doubles, ascending from -0.5 to 0.5).  ap_pitch_hist_f32: the same histogram of n frequencies, those not > 0 skipped;
 * counts (n_bins) is zeroed by the call.  n_bins <= ap_piptrack_max_bins(). */
int ap_piptrack_max_bins(void);
int ap_piptrack_max_records(void);
int ap_piptrack_f32(const float *S /*dev*/, int in_kind, int64_t B, int F, int64_t T, int64_t in_row_stride, int k_lo, int k_hi,
                    float threshold, int ref_mode, float ref_value, const float *ref /*dev (B*T) or NULL*/, float bin_hz,
                    float *pitches /*dev*/, float *magnitudes /*dev*/, int64_t out_row_stride, void *stream);
int ap_piptrack_records_f32(const float *S /*dev*/, int in_kind, int64_t B, int F, int64_t T, int64_t in_row_stride, int k_lo,
                            int k_hi, float threshold, int ref_mode, float ref_value, const float *ref /*dev (B*T) or NULL*/,
                            float bin_hz, int per_clip, float *records /*dev*/, int64_t capacity, uint64_t *counters /*dev (G)*/,
                            void *stream);
int ap_piptrack_tuning_f32(const float *records /*dev*/, const uint64_t *counters /*dev (G)*/, int64_t G, int64_t capacity,
                           double bins_per_octave, const double *edges /*dev (n_bins+1)*/, int n_bins,
                           float *threshold_out /*dev (G)*/, uint64_t *counts /*dev (G*n_bins)*/, void *stream);
int ap_pitch_hist_f32(const float *frequencies /*dev*/, int64_t n, double bins_per_octave, const double *edges /*dev (n_bins+1)*/,
                      int n_bins, uint64_t *counts /*dev (n_bins)*/, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AUDIOPRIMS_H */
