"""CPU: the public surface of piptrack / pitch_tuning / estimate_tuning: signatures, defaults, exports, every validation
error by the name of its argument (all raised before a device is asked for), the bin range against a brute-force mask,
the NumPy model on hand-made columns, and the tuning=None messages of cqt / chroma."""

import importlib
import inspect

import numpy as np
import pytest

import piptrack_ref as R

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _build
from mlx_audio_primitives_amd import _extension as ext

M = importlib.import_module("mlx_audio_primitives_amd.pitch")
S0 = np.ones((9, 4), np.float32)
Y0 = np.zeros(4096, np.float32)


def test_signatures_defaults_and_exports():
    for n in ("piptrack", "pitch_tuning", "estimate_tuning"):
        assert n in ap.__all__ and getattr(ap, n) is getattr(M, n)
    sig = inspect.signature(ap.piptrack)
    assert all(p.kind is p.KEYWORD_ONLY for p in sig.parameters.values())
    assert {k: p.default for k, p in sig.parameters.items()} == dict(
        y=None, sr=22050, S=None, n_fft=2048, hop_length=None, fmin=150.0, fmax=4000.0, threshold=0.1, win_length=None,
        window="hann", center=True, pad_mode="constant", ref=None)
    sig = inspect.signature(ap.pitch_tuning)
    assert list(sig.parameters) == ["frequencies", "resolution", "bins_per_octave"]
    assert sig.parameters["resolution"].default == 0.01 and sig.parameters["bins_per_octave"].default == 12
    assert sig.parameters["resolution"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(ap.estimate_tuning)
    assert {k: p.default for k, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY} == dict(
        y=None, sr=22050, S=None, n_fft=2048, resolution=0.01, bins_per_octave=12)
    assert any(p.kind is p.VAR_KEYWORD for p in sig.parameters.values())
    assert "piptrack.hip" in _build.SOURCES
    for s in ("ap_piptrack_f32", "ap_piptrack_records_f32", "ap_piptrack_tuning_f32", "ap_pitch_hist_f32", "ap_piptrack_max_bins",
              "ap_piptrack_max_records"):
        assert s in ext.ABI_SYMBOLS
    assert ext.lib().ap_piptrack_max_bins() >= 1000 and ext.lib().ap_piptrack_max_records() == 2 ** 31 - 1


@pytest.mark.parametrize("fn,kw,exc,word", [
    (ap.piptrack, dict(), ValueError, "y and S"), (ap.piptrack, dict(y=Y0, S=S0), ValueError, "y and S"),
    (ap.piptrack, dict(S=np.ones(9, np.float32)), ValueError, "S must be 2D"),
    (ap.piptrack, dict(S=np.ones((1, 1, 9, 4), np.float32)), ValueError, "S must be 2D"),
    (ap.piptrack, dict(y=np.zeros((1, 1, 4096), np.float32)), ValueError, "y must be 1D"),
    (ap.piptrack, dict(S=np.ones((1, 4), np.float32)), ValueError, "at least 2 frequency bins"),
    (ap.piptrack, dict(S=S0, fmin=5000.0), ValueError, "fmin"), (ap.piptrack, dict(S=S0, fmin=20000.0, fmax=30000.0), ValueError, "fmin"),
    (ap.piptrack, dict(S=S0, fmin=-5.0, fmax=0.0), ValueError, "fmax"), (ap.piptrack, dict(S=S0, fmin="a"), ValueError, "fmin"),
    (ap.piptrack, dict(S=S0, threshold=-0.1), ValueError, "threshold"), (ap.piptrack, dict(S=S0, threshold=float("nan")), ValueError, "threshold"),
    (ap.piptrack, dict(S=S0, ref=np.mean), TypeError, "ref"), (ap.piptrack, dict(S=S0, ref="max"), TypeError, "ref"),
    (ap.piptrack, dict(S=S0, ref=float("nan")), ValueError, "ref"), (ap.piptrack, dict(S=S0, ref=np.ones((2, 2, 2))), ValueError, "ref"),
    (ap.piptrack, dict(S=S0, sr=0), ValueError, "sr"), (ap.piptrack, dict(y=Y0, n_fft=1), ValueError, "n_fft"),
    (ap.piptrack, dict(y=Y0, hop_length=0), ValueError, "hop_length"),
    (ap.estimate_tuning, dict(S=S0, resolution=0.0), ValueError, "resolution"), (ap.estimate_tuning, dict(S=S0, resolution=1.0), ValueError, "resolution"),
    (ap.estimate_tuning, dict(S=S0, resolution=1e-6), ValueError, "resolution"),
    (ap.estimate_tuning, dict(S=S0, bins_per_octave=0), ValueError, "bins_per_octave"),
    (ap.estimate_tuning, dict(S=S0, bins_per_octave=12.5), ValueError, "bins_per_octave"),
    (ap.estimate_tuning, dict(S=S0, n_mels=3), TypeError, "n_mels"), (ap.estimate_tuning, dict(S=S0, per_clip=2), ValueError, "per_clip"),
    (ap.estimate_tuning, dict(S=S0, _capacity=0), ValueError, "_capacity"), (ap.estimate_tuning, dict(), ValueError, "y and S"),
    (ap.estimate_tuning, dict(S=S0, threshold=-1), ValueError, "threshold"), (ap.estimate_tuning, dict(S=S0, ref=np.mean), TypeError, "ref"),
    (ap.estimate_tuning, dict(S=S0, fmin=9e9), ValueError, "fmin"),
])
def test_rejected_arguments_are_named(fn, kw, exc, word):
    with pytest.raises(exc, match=word):
        fn(**kw)


def test_pitch_tuning_rejects_by_name():
    for kw, word in ((dict(resolution=0), "resolution"), (dict(resolution=1.5), "resolution"), (dict(bins_per_octave=0), "bins_per_octave")):
        with pytest.raises(ValueError, match=word):
            ap.pitch_tuning(np.array([440.0]), **kw)
    with pytest.warns(UserWarning, match="empty"):
        assert ap.pitch_tuning(np.zeros(0, np.float32)) == 0.0


@pytest.mark.parametrize("sr,n_fft,fmin,fmax", [
    (22050, 2048, 150.0, 4000.0), (22050, 2048, 0.0, 4000.0), (22050, 2048, 150.0, 20000.0), (22050, 2048, -3.0, 1e9),
    (16000, 400, 62.5, 1000.0), (16000, 400, 40.0, 8000.0), (44100, 512, 86.1328125, 86.1328125 * 3), (8000, 2, 0.0, 4000.0),
    (22050, 1024, 21.533203125, 11025.0), (48000, 4096, 11.71875, 11.72), (22050.5, 330, 1.0, 11025.25),
])
def test_bin_range_against_the_brute_force_mask(sr, n_fft, fmin, fmax):
    F = n_fft // 2 + 1
    k_lo, k_hi = M._bin_range(sr, n_fft, fmin, fmax, F)
    f = np.arange(F, dtype=np.float64) * float(sr) / n_fft
    mask = (f >= max(fmin, 0.0)) & (f < min(fmax, sr / 2.0))
    np.testing.assert_array_equal(mask, (np.arange(F) >= k_lo) & (np.arange(F) < k_hi))
    assert (k_lo, k_hi) == R.bin_range(sr, n_fft, fmin, fmax, F) and 0 <= k_lo <= k_hi <= F


def test_the_model_on_hand_made_columns():
    cols = np.array([[0, 1, 3, 3, 3, 1, 0, 0], [0, 1, 0, 0, 0, 1, 2, 4], [0, 0, 0, 0, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6, 7, 7]], np.float32).T[None]
    p, m = R.piptrack(cols, k_range=(0, 8), threshold=0.0, sr=14)            # sr / n_fft = 1: pitches are in bins
    assert p.dtype == np.float32 and m.dtype == np.float32 and not np.isnan(p).any() and not np.isnan(m).any()
    assert list(np.nonzero(p[0, :, 0])[0]) == [2], "on a plateau only its first bin is a peak"
    assert p[0, 2, 0] == 2.5 and m[0, 2, 0] == np.float32(3.0) + np.float32(0.5) * np.float32(0.5)      # a, b, c = 1, 3, 3
    assert list(np.nonzero(p[0, :, 1])[0]) == [1, 7] and p[0, 7, 1] == 7.0 and m[0, 7, 1] == 4.0, "a peak at F - 1 has no shift"
    assert not p[0, :, 2].any() and not m[0, :, 2].any(), "an all-zero frame has no peak"
    assert list(np.nonzero(p[0, :, 3])[0]) == [6], "den = 0 on the ramp divides by 1 and makes no peak; bin 0 never is one"
    p2, _ = R.piptrack(cols, k_range=(3, 7), threshold=0.0, sr=14)
    assert list(np.nonzero(p2[0, :, 1])[0]) == [] and list(np.nonzero(p2[0, :, 3])[0]) == [6]
    p3, _ = R.piptrack(cols, k_range=(0, 8), ref=3.5, sr=14)                # |ref| is the threshold itself
    assert list(np.nonzero(p3[0, :, 0])[0]) == [] and list(np.nonzero(p3[0, :, 1])[0]) == [7]
    assert R.median([3, 1, 2]) == 2 and R.median([4, 1, 2, 3]) == 2.5 and R.median([]) == 0 and R.median([5]) == 5
    assert R.pitch_tuning(np.array([440.0, 880.0, 27.5])) == 0.0 and R.pitch_tuning(np.zeros(3)) == 0.0
    assert abs(R.pitch_tuning(440.0 * 2.0 ** (np.array([0.2, 12.2, -11.8]) / 12.0)) - 0.2) <= 0.01


def test_the_model_on_the_end_to_end_fixture():
    """The margin tests/test_gpu_piptrack.py asserts on the device, established here from the model alone."""
    for d, want in ((-0.3, -0.32), (0.0, -0.01), (0.23, 0.21)):
        S, wrong = R.magnitude(R.spectrum(R.harmonics(d)[None], 2048, 512))
        est = R.estimate_tuning(S, sr=22050)
        assert abs(est - want) < 1e-9 and abs(est - d) <= 0.02 + 1e-12 and not wrong.any()


def test_tuning_none_points_at_estimate_tuning():
    y = np.zeros(4096, np.float32)
    for fn, kw in ((ap.cqt, dict()), (ap.vqt, dict())):
        with pytest.raises(ValueError, match="tuning.*estimate_tuning"):
            fn(y, tuning=None, **kw)
    for fn in (ap.chroma_stft, ap.chroma_cqt, ap.chroma_cens, ap.tonnetz):
        with pytest.raises(ValueError, match="tuning.*estimate_tuning"):
            fn(y=y, tuning=None)
    with pytest.raises(ValueError, match="tuning.*estimate_tuning"):
        ap.chroma_filterbank(sr=8000, n_fft=64, tuning=None)
    assert "not implemented" not in importlib.import_module("mlx_audio_primitives_amd.chroma").__doc__.split("tuning=None")[1][:80]
