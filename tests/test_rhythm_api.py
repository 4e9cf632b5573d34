"""CPU: the host side of rhythm.py - validation before any device work, tempo_frequencies, the window length and the
prior table of tempo, the period of bpm= and the units / sparse rules of beat_track.  Nothing here touches a GPU."""

import inspect

import numpy as np
import pytest

import rhythm_ref as R

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import rhythm


def test_exported_with_librosas_signatures():
    for name in ("tempogram", "tempo", "beat_track", "tempo_frequencies"):
        assert name in ap.__all__ and getattr(ap, name) is getattr(rhythm, name)
    sig = inspect.signature(ap.tempogram).parameters
    assert list(sig) == ["y", "sr", "onset_envelope", "hop_length", "win_length", "center", "window", "norm"]
    assert all(p.kind == p.KEYWORD_ONLY for p in sig.values())
    assert sig["win_length"].default == 384 and sig["norm"].default == np.inf and sig["window"].default == "hann"
    sig = inspect.signature(ap.tempo).parameters
    assert list(sig) == ["y", "sr", "onset_envelope", "tg", "hop_length", "start_bpm", "std_bpm", "ac_size", "max_tempo",
                         "aggregate", "prior"]
    assert sig["ac_size"].default == 8.0 and sig["max_tempo"].default == 320.0 and sig["aggregate"].default is np.mean
    sig = inspect.signature(ap.beat_track).parameters
    assert list(sig) == ["y", "sr", "onset_envelope", "hop_length", "start_bpm", "tightness", "trim", "bpm", "prior", "units",
                         "sparse"]
    assert sig["tightness"].default == 100 and sig["trim"].default is True and sig["units"].default == "frames"


def test_tempo_frequencies():
    bpm = ap.tempo_frequencies(384)
    assert bpm.dtype == np.float64 and bpm.shape == (384,) and bpm[0] == np.inf
    np.testing.assert_array_equal(bpm, R.tempo_frequencies(384))
    assert bpm[1] == 60.0 * 22050 / 512 and np.all(np.diff(bpm[1:]) < 0)
    np.testing.assert_array_equal(ap.tempo_frequencies(5, hop_length=256, sr=16000)[1:], 60.0 * 16000 / (256 * np.arange(1.0, 5)))
    assert ap.tempo_frequencies(0).shape == (0,) and list(ap.tempo_frequencies(1)) == [np.inf]
    with pytest.raises(ValueError, match="n_bins"):
        ap.tempo_frequencies(-1)


def test_tempo_window_and_prior_table():
    assert rhythm._window_length(8.0, 22050, 512) == 344 == R.tempo_window()
    assert rhythm._window_length(4.0, 16000, 160) == 400
    W = 344
    lp = rhythm._log_prior(W, 22050, 512, 120.0, 1.0, 320.0, None)
    np.testing.assert_array_equal(lp, R.log_prior(W))
    bpm = ap.tempo_frequencies(W)
    first = int(np.argmax(bpm < 320.0))
    assert first == 9 and np.all(np.isneginf(lp[:first])) and np.all(np.isfinite(lp[first:]))
    k = int(np.argmax(lp))
    assert abs(bpm[k] - 120.0) < 4.0
    np.testing.assert_allclose(lp[first:], -0.5 * (np.log2(bpm[first:]) - np.log2(120.0)) ** 2, rtol=1e-14)
    lp = rhythm._log_prior(W, 22050, 512, 120.0, 1.0, None, None)           # no limit: lag 0 is excluded all the same
    assert np.isneginf(lp[0]) and np.all(np.isfinite(lp[1:]))
    lp = rhythm._log_prior(W, 22050, 512, 120.0, 1.0, 1e9, None)
    assert np.isneginf(lp[0]) and np.all(np.isfinite(lp[1:]))

    class Flat:
        def logpdf(self, x):
            return np.where(np.isfinite(x), -np.log(300.0), 0.0)

    lp = rhythm._log_prior(W, 22050, 512, 120.0, 1.0, 320.0, Flat())
    assert np.all(np.isneginf(lp[:first])) and np.all(lp[first:] == -np.log(300.0))
    with pytest.raises(TypeError, match="logpdf"):
        rhythm._log_prior(W, 22050, 512, 120.0, 1.0, 320.0, object())
    with pytest.raises(ValueError, match="start_bpm"):
        rhythm._log_prior(W, 22050, 512, 0.0, 1.0, 320.0, None)
    with pytest.raises(ValueError, match="std_bpm"):
        rhythm._log_prior(W, 22050, 512, 120.0, 0.0, 320.0, None)


def test_period_from_bpm_and_half_to_even():
    fps = 22050 / 512
    P = rhythm._periods(120.0, 3, False, 22050, 512)
    assert P.dtype == np.int32 and list(P) == [int(np.rint(60 * fps / 120.0))] * 3 == [22] * 3
    assert list(rhythm._periods(np.array([60.0, 120.0, 240.0]), 3, False, 22050, 512)) == [43, 22, 11]
    assert list(rhythm._periods([100.0], 1, True, 22050, 512)) == [26]
    # rint: halves to even, as np.rint
    assert list(rhythm._periods(120.0, 1, True, 5, 1)) == [2] and list(rhythm._periods(120.0, 1, True, 7, 1)) == [4]    # 2.5, 3.5
    with pytest.raises(ValueError, match="at least 2"):
        rhythm._periods(60 * fps / 1.4, 1, True, 22050, 512)
    with pytest.raises(ValueError, match="not supported"):
        rhythm._periods(0.5, 1, True, 22050, 512)
    with pytest.raises(ValueError, match="strictly positive"):
        rhythm._periods(0.0, 1, True, 22050, 512)
    with pytest.raises(NotImplementedError, match="per frame"):
        rhythm._periods(np.full(50, 120.0), 1, True, 22050, 512)
    with pytest.raises(NotImplementedError, match="per frame"):
        rhythm._periods(np.full((2, 50), 120.0), 2, False, 22050, 512)
    # h = rint(P / 2) of the kernels, halves to even (the reference's; the emulator test compares the kernel's)
    assert [R.half(P) for P in (2, 3, 5, 7)] == [1, 2, 2, 4]


def test_validation_before_any_device_work():
    e = np.ones(50, np.float32)
    with pytest.raises(ValueError, match="win_length"):
        ap.tempogram(onset_envelope=e, win_length=0)
    with pytest.raises(ValueError, match="hop_length"):
        ap.tempogram(onset_envelope=e, hop_length=0)
    with pytest.raises(ValueError, match="sr"):
        ap.tempo(onset_envelope=e, sr=0)
    for norm in (1, 2, -np.inf, "max"):
        with pytest.raises(NotImplementedError, match="norm"):
            ap.tempogram(onset_envelope=e, norm=norm)
    with pytest.raises(NotImplementedError, match="aggregate"):
        ap.tempo(onset_envelope=e, aggregate=np.median)
    with pytest.raises(ValueError, match="tg must be"):
        ap.tempo(tg=np.ones(5, np.float32))
    with pytest.raises(ValueError, match="units"):
        ap.beat_track(onset_envelope=e, units="beats")
    with pytest.raises(ValueError, match="needs sparse=True"):
        ap.beat_track(onset_envelope=e, units="time", sparse=False)
    with pytest.raises(ValueError, match="sparse=True needs 1D"):
        ap.beat_track(onset_envelope=np.ones((2, 50), np.float32))
    with pytest.raises(ValueError, match="sparse=True needs 1D"):
        ap.beat_track(y=np.ones((2, 5000), np.float32))
    with pytest.raises(ValueError, match="tightness"):
        ap.beat_track(onset_envelope=e, tightness=0)
    with pytest.raises(ValueError, match="either y or onset_envelope"):
        ap.beat_track()
    with pytest.raises(ValueError, match="1D or 2D"):
        ap.beat_track(onset_envelope=np.ones((2, 3, 4), np.float32), sparse=False)
    with pytest.raises(ValueError, match="16384"):
        ap.beat_track(onset_envelope=np.ones(16385, np.float32), bpm=120.0)
    with pytest.raises(ValueError, match="at least 2"):
        ap.beat_track(onset_envelope=e, bpm=2000.0)
    with pytest.raises(NotImplementedError, match="per frame"):
        ap.beat_track(onset_envelope=e, bpm=np.full(50, 120.0))
