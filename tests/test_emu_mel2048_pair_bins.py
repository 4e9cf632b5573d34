"""CPU: the n_fft = 2048 run kernels (kernels_mel2048.h) on the SIMT emulator, with pure tones on the
bins their in-register radix-4 + split treats specially.  A lane takes the radix-4 groups L, L + 64,
192 - L and 256 - L; the lane with L = 0 takes groups 0, 64, 192 and 128 instead, whose bins pair with
bins of the same group (0 / 1024, 256 / 768, 128 / 896, 384 / 640) or with none (512).  The tones sit
on exactly those bins, alone and mixed, at power 2 and 1, and the clip lengths put clip starts inside
the stretches of the emulated waves."""

import os
import sys

import numpy as np
import pytest

from oracle import audio_oracle as ao

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_bind as eb  # noqa: E402

SR, N_FFT, HOP = 22050, 2048, 512
SPECIAL_BINS = [0, 64, 128, 192, 256, 384, 512, 640, 768, 896, 1024]


def _tones(bins, B, L, seed):
    """B clips of cosines centred on `bins` (period 2048 / bin), amplitudes and phases per clip."""
    rng = np.random.default_rng(seed)
    n = np.arange(L)
    y = np.zeros((B, L))
    for b in range(B):
        for k in bins:
            amp = rng.uniform(0.2, 1.0)
            phase = rng.uniform(0, 2 * np.pi) if k not in (0, 1024) else 0.0
            y[b] += amp * np.cos(2 * np.pi * k * n / N_FFT + phase)
    return y.astype(np.float32)


def _box_filterbank():
    """128 rows of 8 bins each over bins 0..1023, the last row reaching bin 1024: every bin counts once,
    so a |X|^p value on a wrong bin (or missing) shows in its row."""
    fb = np.zeros((128, N_FFT // 2 + 1), np.float32)
    for m in range(128):
        fb[m, 8 * m: 8 * m + 8] = 1.0
    fb[127, 1024] = 1.0
    return fb


def _power_spec(y, power):
    S = np.stack([np.abs(ao.stft(y[b], n_fft=N_FFT, hop_length=HOP, center=True, pad_mode="constant"))
                  for b in range(y.shape[0])])
    return S ** power


# L: 3 clips of 18 frames on one emulated 8-wave workgroup (stretches of 6-7 frames: the second and third
# clips start inside a stretch); 2 clips of 13 frames (every wave's stretch crosses or touches a clip start)
@pytest.mark.parametrize("power", [2.0, 1.0])
@pytest.mark.parametrize("B,L", [(3, 9000), (2, 6200)])
@pytest.mark.parametrize("which", ["each", "mixed"])
def test_emu_run_kernel_special_bins(power, B, L, which):
    win = ao.padded_window("hann", N_FFT, N_FFT)
    groups = [[k] for k in SPECIAL_BINS] if which == "each" else [SPECIAL_BINS]
    fb_mel = ao.mel_filterbank(SR, N_FFT, 128)
    fb_box = _box_filterbank()
    for i, bins in enumerate(groups):
        y = _tones(bins, B, L, seed=100 + 7 * i + B)
        # the product's filterbank, against the oracle
        R = ao.melspectrogram(y, sr=SR, n_fft=N_FFT, hop_length=HOP, n_mels=128, power=power)
        A = eb.melspec(y, N_FFT, HOP, win, fb_mel, power=power)
        np.testing.assert_allclose(A, R, rtol=1e-4, atol=1e-4, err_msg=f"mel, bins {bins}")
        # every bin 0..1024 in exactly one row
        Rb = np.einsum("mf,bft->bmt", fb_box.astype(np.float64), _power_spec(y.astype(np.float64), power))
        Ab = eb.melspec(y, N_FFT, HOP, win, fb_box, power=power)
        np.testing.assert_allclose(Ab, Rb, rtol=1e-4, atol=1e-4,
                                   err_msg=f"box rows, bins {bins}")


@pytest.mark.parametrize("B,L", [(3, 9000)])
def test_emu_spectral_statistics_special_bins(B, L):
    """ap_spec2048_run_kernel shares the transform and split: its centroid weighs every bin by its
    frequency, bins 0 and 1024 included."""
    win = ao.padded_window("hann", N_FFT, N_FFT)
    kw = dict(sr=SR, n_fft=N_FFT, hop_length=HOP, center=True)
    for i, bins in enumerate([[k] for k in SPECIAL_BINS] + [SPECIAL_BINS]):
        y = _tones(bins, B, L, seed=300 + i)
        got = eb.spectral_from_audio(y, SR, HOP, win, center=True, want=("centroid",))["centroid"]
        for b in range(B):
            np.testing.assert_allclose(got[b], ao.spectral_centroid(y[b], **kw)[0], rtol=2e-4, atol=1e-2,
                                       err_msg=f"bins {bins}")
