"""GPU: time_stretch and pitch_shift (effects.py) as compositions of stft, phase_vocoder, istft and the FFT resampler."""

import numpy as np
import pytest
import torch

import mlx_audio_primitives_amd as ap

pytestmark = pytest.mark.gpu

SR = 22050


def sine(freq=440.0, n=SR):
    return np.sin(2.0 * np.pi * freq * np.arange(n) / SR).astype(np.float32)


@pytest.mark.parametrize("n_fft", [2048, 400])
@pytest.mark.parametrize("rate", [0.8, 1.5])
def test_time_stretch_is_stft_vocoder_istft(n_fft, rate):
    L = 6000
    y = torch.from_numpy(np.random.default_rng(7).standard_normal((2, L)).astype(np.float32)).cuda()
    for x in (y[0], y):
        want = ap.istft(ap.phase_vocoder(ap.stft(x, n_fft=n_fft), rate=rate), n_fft=n_fft, length=int(round(L / rate)))
        got = ap.time_stretch(x, rate=rate, n_fft=n_fft)
        assert got.shape == x.shape[:-1] + (int(round(L / rate)),) and torch.equal(got, want)
        # a host array; pad_mode is stft's alone
        assert torch.equal(ap.time_stretch(x.cpu().numpy(), rate=rate, n_fft=n_fft, center=True, pad_mode="constant"), got)


@pytest.mark.parametrize("n_steps,freq", [(12, 880.0), (-12, 220.0)])
def test_pitch_shift_moves_a_sine(n_steps, freq):
    y = sine()
    out = ap.pitch_shift(torch.from_numpy(y).cuda(), sr=SR, n_steps=n_steps)
    assert out.shape == y.shape and out.dtype == torch.float32
    peak = int(np.argmax(np.abs(np.fft.rfft(out.cpu().numpy().astype(np.float64)))))      # bins of sr / L = 1 Hz
    print(f"pitch_shift {n_steps:+d}: peak at {peak} Hz")
    assert abs(peak - freq) <= 1
    both = torch.from_numpy(np.stack([y, y])).cuda()
    scaled = ap.pitch_shift(both, sr=SR, n_steps=n_steps, scale=True)
    assert scaled.shape == (2, SR)
    assert torch.equal(scaled, ap.pitch_shift(both, sr=SR, n_steps=n_steps) / np.float32(np.sqrt(2.0 ** (-n_steps / 12))))


def test_pitch_shift_by_nothing_is_the_round_trip():
    """n_steps = 0: rate 1, the vocoder is the identity; the parity suite's STFT round-trip bound, 1e-5 max abs."""
    y = sine()
    out = ap.pitch_shift(y, sr=SR, n_steps=0)
    err = float(np.max(np.abs(out.cpu().numpy() - y)))
    print(f"pitch_shift 0: max |out - y| = {err:.2e}")
    assert out.shape == y.shape and err <= 1e-5
