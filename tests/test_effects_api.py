"""CPU: the public surface of effects.py and the host side of the phase vocoder's C entry points."""

import inspect
import os

import numpy as np
import pytest

from conftest import ROOT

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _extension as ext

SIGNATURES = {"phase_vocoder": ["rate", "hop_length", "n_fft"], "time_stretch": ["rate"],
              "pitch_shift": ["sr", "n_steps", "bins_per_octave", "res_type", "scale"]}


def test_names_symbols_and_keyword_only_signatures():
    header = open(os.path.join(ROOT, "include", "audioprims.h")).read()
    for sym in ("ap_phase_vocoder_f32", "ap_phase_vocoder_frames"):
        assert sym in ext.ABI_SYMBOLS and sym + "(" in header and getattr(ext.lib(), sym) is not None
    for name, keys in SIGNATURES.items():
        assert name in ap.__all__
        params = list(inspect.signature(getattr(ap, name)).parameters.values())
        named = [p for p in params[1:] if p.kind is not inspect.Parameter.VAR_KEYWORD]
        assert params[0].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and [p.name for p in named] == keys
        assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in named)


@pytest.mark.parametrize("rate", [1.0 / 3.0, 0.1, 7.0, 0.5, 0.77, 0.9, 1.0, 1.25, 1.3, 2.0, 3.7, 4.0, 2.0 ** (-7 / 12)])
def test_frames_follow_numpy_arange(rate):
    for T in (0, 1, 2, 3, 7, 63, 64, 70, 130, 200, 431, 3000, 25840):
        assert ext.lib().ap_phase_vocoder_frames(T, rate) == len(np.arange(0, T, rate)), (T, rate)
    assert ext.lib().ap_phase_vocoder_frames(10, 0.0) == -1


def test_value_errors():
    D, y = np.ones((5, 4), np.complex64), np.zeros(4096, np.float32)
    for rate in (0, -1.0, float("nan"), float("inf"), "2"):
        with pytest.raises(ValueError, match="rate must be a positive number"):
            ap.phase_vocoder(D, rate=rate)
        with pytest.raises(ValueError, match="rate must be a positive number"):
            ap.time_stretch(y, rate=rate)
    with pytest.raises(ValueError, match="hop_length must be a positive integer"):
        ap.phase_vocoder(D, rate=1.0, hop_length=0)
    with pytest.raises(ValueError, match="n_fft must be a positive integer"):
        ap.phase_vocoder(D, rate=1.0, n_fft=2.5)
    with pytest.raises(ValueError, match="must be complex"):
        ap.phase_vocoder(D.real, rate=1.0)
    for res_type in ("linear", "soxr_hq"):
        with pytest.raises(ValueError, match='"fft"'):
            ap.pitch_shift(y, sr=22050, n_steps=2, res_type=res_type)
