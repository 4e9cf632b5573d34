"""Windows and case tables shared by test_emu_windows.py and test_gpu_windows.py (helper, no tests).

A periodic Hann window hides frame-edge and window-indexing slips: w[0] = 0, the first and last few weights are
~1e-5, w[N - k] = w[k], and its overlap-add envelope vanishes at the ends of a non-centred signal.  The three
windows here do not:

  rough   rough_window(n_fft) as an array: uniform in [0.25, 1], asymmetric, every index its own weight
  boxcar  by name: full weight on both frame edges; the named builder path without symmetrisation
  short   rough_window(win_length) with win_length = n_fft - 101 (n_fft - 37 for n_fft <= 256): an odd
          zero-pad, so the left pad is one shorter than the right one

With weights >= 0.25 the envelope sum w^2 is >= 0.0625 wherever the non-zero part of a frame reaches, so the
inverse tests compare every output sample at the normal bar.  The zero pads of the short window reach no
further than 51 samples, less than the n_fft / 2 a centred inverse trims; without centring they would leave
the first 50 and last 51 samples of a stream with no support at all, so the short window's inverse cases are
centred only (the envelope floor each inverse test asserts could not hold otherwise).  Its hops are
<= win_length / 2.
"""

from collections import namedtuple

import numpy as np

KINDS = ("rough", "boxcar", "short")

Win = namedtuple("Win", "arg win_length padded floor")
# arg: what the public API / the oracle take as `window`; padded: the float32 (n_fft,) array a kernel reads;
# floor: the least sum w^2 a reached sample may have


def rough_window(n, seed=None):
    return np.random.default_rng(n if seed is None else seed).uniform(0.25, 1.0, n).astype(np.float32)


def short_length(n_fft):
    return n_fft - 37 if n_fft <= 256 else n_fft - 101


def make_window(kind, n_fft):
    if kind == "boxcar":
        return Win("boxcar", n_fft, np.ones(n_fft, np.float32), 1.0)
    if kind == "rough":
        w = rough_window(n_fft)
        return Win(w, n_fft, w, 0.0625)
    assert kind == "short", kind
    wl = short_length(n_fft)
    w = rough_window(wl)
    left = (n_fft - wl) // 2
    padded = np.pad(w, (left, n_fft - wl - left))
    assert (n_fft - wl) % 2 == 1 and padded[left - 1] == 0.0 and padded[left] != 0.0
    return Win(w, wl, padded, 0.0625)


def envelope(win, n_fft, hop, T):
    """float64 sum of w^2 over the T frames' span, (T - 1) hop + n_fft samples."""
    w2 = win.padded.astype(np.float64) ** 2
    wss = np.zeros((T - 1) * hop + n_fft)
    for t in range(T):
        wss[t * hop:t * hop + n_fft] += w2
    return wss


def assert_envelope_floor(win, n_fft, hop, T, lo, hi):
    """A condition on the reference, not on the kernel: every compared sample [lo, hi) of the overlap-add
    span has sum w^2 >= the window's floor, so none needs a mask or a wider bar."""
    wss = envelope(win, n_fft, hop, T)
    assert 0 <= lo < hi <= wss.shape[0], (lo, hi, wss.shape[0])
    assert wss[lo:hi].min() >= win.floor, (wss[lo:hi].min(), win.floor)


def istft_span(n_fft, hop, T, center, length):
    """[lo, hi) of the overlap-add span that istft(..., center, length) returns."""
    lo = n_fft // 2 if center else 0
    natural = (T - 1) * hop + n_fft - 2 * lo
    return lo, lo + (natural if length is None else length)


def spectrum(B, n_fft, T, seed):
    rng = np.random.default_rng(seed)
    F = n_fft // 2 + 1
    return (rng.standard_normal((B, F, T)) + 1j * rng.standard_normal((B, F, T))).astype(np.complex64)


# ---- forward cases for the emulator: n_fft, hop, L, B, pad_mode, center -------------------------------------------
# the smallest shapes test_emu_kernels.py uses per engine; B >= 2 and L % hop != 0 unless noted
EMU_STFT_CASES = [
    (2048, 512, 10753, 3, "constant", True),    # wave kernel: carried row windows, clip change in a stretch
    (2048, 512, 9300, 2, "constant", False),
    (2048, 512, 6000, 2, "reflect", True),      # index-remapped edge frames
    (2048, 255, 5000, 2, "constant", True),     # odd hop
    (1024, 256, 5377, 3, "constant", True),
    (1024, 300, 6100, 2, "constant", False),
    (1024, 256, 4000, 2, "reflect", True),
    (1024, 255, 3000, 2, "constant", True),
    (512, 128, 4001, 2, "constant", True),
    (512, 256, 2049, 2, "constant", False),
    (512, 128, 4001, 2, "reflect", True),
    (512, 77, 3001, 2, "constant", True),
    (400, 160, 3333, 2, "constant", True),
    (400, 77, 1000, 2, "constant", False),
    (400, 160, 5001, 3, "edge", True),
    (400, 33, 2000, 2, "reflect", True),
    (256, 64, 1501, 2, "constant", True),
    (256, 64, 1501, 2, "constant", False),
    (256, 64, 1501, 2, "reflect", True),
    (256, 33, 700, 2, "constant", True),
    (154, 30, 801, 2, "constant", True),        # generic mixed radix 2 * 7 * 11
    (154, 30, 801, 2, "constant", False),
    (154, 31, 801, 2, "edge", True),
]

# kernels_stft16.h: hop, L, B, pad_mode, center, Ts, grid_cap, misalign, force_unaligned (test_emu_stft16's arguments)
EMU_STFT16_CASES = [
    (512, 10753, 3, "constant", True, None, 2, 0, False),     # dense rows: carries, clip change in a stretch
    (512, 9300, 2, "constant", False, None, 2, 5, False),
    (512, 6000, 2, "reflect", True, None, 2, 0, False),
    (255, 5000, 2, "constant", True, None, 2, 1, False),      # odd hop: index-remapped loads
    (512, 10753, 3, "constant", True, 32, 2, 0, False),       # padded rows: whole lines
    (512, 20001, 2, "edge", True, 48, 3, 0, False),
    (512, 20001, 2, "constant", True, 48, 3, 0, True),        # the carry path on the padded layout
    (512, 9300, 2, "constant", False, 32, 2, 0, False),
    (255, 9000, 2, "constant", True, 48, 2, 0, False),
    (512, 10753, 3, "constant", True, 32, 2, 0, 3),           # whole-group tile
    (512, 20001, 2, "edge", True, 48, 3, 0, 3),
]

# mel kernels: n_fft, sr, M, hop, L, B, power, pad_mode, center
EMU_MEL_CASES = [
    (2048, 22050, 128, 512, 9001, 2, 2.0, "constant", True),   # run kernel, hop 512 register reuse
    (2048, 22050, 128, 512, 9001, 2, 1.0, "constant", False),
    (2048, 22050, 128, 512, 7001, 2, 1.0, "edge", True),       # run kernel, index-remapped edge frames
    (2048, 22050, 128, 333, 6000, 2, 2.0, "constant", True),   # odd hop
    (2048, 22050, 128, 256, 7001, 2, 2.0, "constant", True),   # run kernel, full reload per frame
    (2048, 22050, 64, 512, 7001, 2, 2.0, "reflect", True),     # fewer filters: the tile kernel serves them
    (1024, 22050, 128, 256, 9001, 2, 2.0, "constant", True),   # wave512
    (1024, 22050, 80, 128, 5001, 2, 1.0, "constant", False),
    (1024, 22050, 80, 256, 6001, 2, 2.0, "reflect", True),
    (1024, 22050, 40, 255, 4000, 2, 1.5, "constant", True),
    (400, 16000, 80, 160, 5001, 3, 2.0, "constant", True),     # frames8, R = 25
    (400, 16000, 80, 160, 1300, 2, 1.0, "constant", False),
    (400, 16000, 40, 160, 5001, 3, 2.0, "edge", True),
    (400, 16000, 40, 33, 2000, 2, 2.0, "constant", True),
    (512, 22050, 128, 128, 4001, 2, 2.0, "constant", True),    # frames8, R = 32 (window in LDS)
    (512, 22050, 40, 256, 3001, 2, 1.0, "constant", False),
    (512, 16000, 40, 128, 4001, 2, 2.0, "reflect", True),
    (512, 16000, 40, 77, 3001, 2, 2.0, "constant", True),
    (256, 8000, 32, 64, 1501, 3, 2.0, "constant", True),       # frames8, R = 16
    (256, 16000, 64, 100, 1111, 2, 1.0, "constant", False),
    (256, 16000, 40, 64, 1501, 2, 2.0, "reflect", True),
    (256, 16000, 40, 33, 1111, 2, 2.0, "constant", True),
]

# ---- inverse cases for the emulator --------------------------------------------------------------------------------
# hop of the short window's cases: <= short_length / 2 and one the fused kernel of that n_fft serves
SHORT_HOP = {2048: 512, 1024: 256, 512: 128, 400: 100, 256: 64, 154: 30, 300: 75}

# fused kernels (eb.istft_fused): n_fft, hop, L, B, grid_cap.  Two workgroups on three clips where the kernel carries
# along a stretch (a clip change inside a stretch, a stretch that starts inside a clip)
EMU_ISTFT_FUSED_CASES = [
    (2048, 512, 7001, 3, 2), (2048, 1024, 15001, 2, 2), (2048, 256, 5001, 2, 2),
    (1024, 256, 5377, 3, 2), (1024, 128, 4001, 2, 3), (1024, 512, 9001, 2, 2),
    (512, 128, 5001, 3, 1), (512, 256, 5001, 2, 1), (512, 128, 9001, 2, 2),
    (400, 160, 5001, 2, 1), (400, 100, 4101, 3, 1),
    (256, 64, 3001, 2, 1), (256, 33, 1500, 2, 1),
]

# kernels_istft16.h: hop, L, B, grid_cap, Ts, variant (test_emu_istft16's arguments; every variant, dense and padded
# rows, every hop the kernel serves)
EMU_ISTFT16_CASES = [
    (512, 10753, 3, 2, None, 0),     # T = 22: two 16-frame groups per clip, the second with 6 frames; clip change in a stretch
    (512, 12400, 2, 4, 30, 0),       # T = 25 on rows of 30: the clip ends after a first step (one frame in the last group)
    (1024, 15001, 2, 2, None, 0),
    (256, 5001, 2, 2, None, 0),
    (1024, 15001, 2, 2, 16, 1),      # the eight-round staging pass, padded rows
    (512, 10753, 2, 5, None, 2),     # loads issued in the staging pass; stretches that start inside a clip
    (256, 5001, 2, 2, None, 3),
]

# irfft_frames + overlap_add: n_fft, hop, L, B
EMU_ISTFT_UNFUSED_CASES = [(2048, 512, 7001, 2), (1024, 256, 5001, 2), (512, 128, 4001, 2), (400, 160, 3001, 2),
                           (256, 64, 1501, 2), (154, 30, 801, 2)]

# stream kernel: n_fft, hop, chunkings of K frames (test_emu_istft_stream.CASES, two or three chunkings each)
EMU_STREAM_CASES = [
    (2048, 512, [[9], [0, 2, 0, 1, 1, 4, 1], [3, 0, 6]]),
    (1024, 256, [[6], [1, 0, 5], [2, 4]]),
    (512, 128, [[11], [0, 1, 2, 0, 5, 3], [4, 7]]),
    (400, 160, [[7], [1, 0, 2, 4], [2, 2, 2, 1]]),
    (256, 64, [[8], [1] * 8, [0, 3, 5]]),
    (300, 75, [[7], [1] * 7, [0, 3, 0, 4]]),          # the two-launch path (irfft frames + carried overlap-add)
]
