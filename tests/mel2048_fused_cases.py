"""Cases shared by test_emu_mel2048_fused_twiddles.py (CPU emulator) and test_gpu_mel2048_fused_twiddles.py
(GPU): pure tones on the bins whose twiddles the n_fft = 2048 run kernels now apply on the read side of their
two exchanges, and a float64 reference for the accuracy figure.  Not a test module.

Bin k = g + 256 q belongs to radix-4 group g; its W_64^(a c) twiddles depend on c = g >> 4, and the lane with
index L takes the groups L, L + 64, 192 - L, 256 - L (L = 0: 0, 64, 192, 128).  The groups below are those
where c changes (15 / 16 / 17), the mirrored groups around 64, 128 and 192, the ends, and the L = 0 lane."""

import numpy as np

from oracle import audio_oracle as ao

SR, N_FFT = 22050, 2048
HOPS = (512, 256)
POWERS = (2.0, 1.0)
B, L = 3, 9000                      # 18 / 36 frames a clip: clip ends inside the emulated waves' stretches
GROUPS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255)
TONE_BINS = tuple(g + 256 * q for g in GROUPS for q in range(4)) + (1024,)
# every tone alone in a clip (B clips a call, the last call filled up from the front) and all of them in one
ALONE = tuple(tuple(TONE_BINS[(i + j) % len(TONE_BINS)] for j in range(B)) for i in range(0, len(TONE_BINS), B))


def tones(bins_per_clip, seed):
    """One clip per entry of bins_per_clip: cosines centred on its bins, random amplitudes and phases."""
    rng = np.random.default_rng(seed)
    n = np.arange(L)
    y = np.zeros((len(bins_per_clip), L))
    for b, bins in enumerate(bins_per_clip):
        for k in bins:
            amp = rng.uniform(0.2, 1.0)
            phase = rng.uniform(0, 2 * np.pi) if k not in (0, 1024) else 0.0
            y[b] += amp * np.cos(2 * np.pi * k * n / N_FFT + phase)
    return y.astype(np.float32)


def alone(i):
    """Call i of the 'each alone in a clip' cases: (B, L) with one tone a clip."""
    return tones([[k] for k in ALONE[i]], seed=500 + i)


def mixed():
    """All tones in every clip, other amplitudes and phases per clip."""
    return tones([TONE_BINS] * B, seed=499)


def box_filterbank():
    """128 rows of 8 bins each over bins 0..1023, the last row reaching bin 1024 (the bank of
    test_emu_mel2048_pair_bins.py): every bin counts once, a |X|^p value on a wrong bin shows in its row."""
    fb = np.zeros((128, N_FFT // 2 + 1), np.float32)
    for m in range(128):
        fb[m, 8 * m: 8 * m + 8] = 1.0
    fb[127, 1024] = 1.0
    return fb


def box_reference(y, hop, power):
    """The oracle's |STFT|^power through the box bank, (B, 128, T)."""
    S = np.stack([np.abs(ao.stft(y[b], n_fft=N_FFT, hop_length=hop, center=True, pad_mode="constant"))
                  for b in range(y.shape[0])]).astype(np.float64)
    return np.einsum("mf,bft->bmt", box_filterbank().astype(np.float64), S ** power)


def mel_f64(y, win, fb, hop, power):
    """Mel spectrogram in float64 from end to end (centred frames, constant padding): (B, M, T)."""
    y = np.asarray(y, np.float64)
    yp = np.pad(y, ((0, 0), (N_FFT // 2, N_FFT // 2)))
    T = 1 + y.shape[1] // hop
    idx = hop * np.arange(T)[:, None] + np.arange(N_FFT)[None, :]
    S = np.abs(np.fft.rfft(yp[:, idx] * np.asarray(win, np.float64), axis=-1)) ** power      # (B, T, F)
    return np.einsum("mf,btf->bmt", np.asarray(fb, np.float64), S)


def worst_frame_error(A, R):
    """Largest |A - R| of a frame over that frame's largest reference value, worst frame of the batch."""
    err = np.abs(np.asarray(A, np.float64) - R).max(axis=1)
    return float((err / R.max(axis=1)).max())
