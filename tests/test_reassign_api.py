"""CPU: the public surface of reassigned_spectrogram - export, build list, ABI symbol, argument errors, window tables.  No device work."""

import importlib

import numpy as np
import pytest
import torch

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _build, _extension as ext

reassign = importlib.import_module("mlx_audio_primitives_amd.reassign")
Y = np.zeros(4096, np.float32)


def test_exported_built_and_in_the_abi():
    assert ap.reassigned_spectrogram is reassign.reassigned_spectrogram and "reassigned_spectrogram" in ap.__all__
    assert "reassign.hip" in _build.SOURCES
    assert "ap_reassign_f32" in ext.ABI_SYMBOLS and ext.lib().ap_reassign_f32 is not None


@pytest.mark.parametrize("kwargs, match", [
    (dict(ref_power=-1.0), "ref_power must be non-negative"),
    (dict(reassign_frequencies=False, reassign_times=False), "must be True"),
    (dict(S=np.zeros((1025, 3), np.complex64)), "precomputed S"),
    (dict(ref_power=np.max), "callable ref_power"),
    (dict(dtype=np.float64), "float32"),
    (dict(hop_length=0), "hop_length must be positive"),
    (dict(win_length=4096), "must be <= n_fft"),
])
def test_argument_errors(kwargs, match):
    with pytest.raises(ValueError, match=match):
        ap.reassigned_spectrogram(Y, **kwargs)


@pytest.mark.parametrize("window", ["hann", "hamming"])
@pytest.mark.parametrize("n_fft, win_length", [(16, 16), (27, 27), (32, 20), (27, 12)])
def test_window_tables_follow_the_formulas(window, n_fft, win_length):
    first = reassign._get_reassign_tables(window, win_length, n_fft, "cpu")
    h, dh, th = (t.numpy() for t in first)
    w = ap.get_window(window, win_length, device="cpu").numpy().astype(np.float64)
    left = (n_fft - win_length) // 2
    want_h = np.concatenate([np.zeros(left), w, np.zeros(n_fft - win_length - left)])
    tau = np.arange(n_fft) + (0.5 if n_fft % 2 == 0 else 0.0) - n_fft // 2
    want_dh = np.array([(want_h[(i + 1) % n_fft] - want_h[(i - 1) % n_fft]) / 2 for i in range(n_fft)])
    assert np.array_equal(h, want_h.astype(np.float32))
    assert np.array_equal(dh, want_dh.astype(np.float32)) and np.array_equal(th, (want_h * tau).astype(np.float32))
    if window == "hamming" and win_length == n_fft:
        assert dh[-1] == np.float32((want_h[0] - want_h[-2]) / 2) != 0      # the wrap: the window does not end at zero
    assert reassign._get_reassign_tables(window, win_length, n_fft, "cpu") is first           # built once, then cached


def test_no_gpu_is_a_loud_error():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no HIP device"):
        ap.reassigned_spectrogram(Y)
