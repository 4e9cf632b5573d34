"""CPU: the host side of chroma_stft / chroma_cqt / chroma_cens / tonnetz (mlx-audio-primitives_amd/chroma.py): the
signatures, the two matrix builders against the float64 definitions in tests/chroma_ref.py and against the facts a
musician would check, the tonnetz basis, every rejected argument by name, the bank caches.  Every check happens before
a device is asked for, so nothing here needs one."""

import importlib
import inspect

import numpy as np
import pytest

import chroma_ref as R

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _build
from mlx_audio_primitives_amd import _extension as _x

M = importlib.import_module("mlx_audio_primitives_amd.chroma")

Y = np.zeros(4096, np.float32)
KW = inspect.Parameter.KEYWORD_ONLY


def test_names_are_exported_and_built():
    for n in ("chroma_stft", "chroma_cqt", "chroma_cens", "tonnetz", "chroma_filterbank", "cq_to_chroma"):
        assert n in ap.__all__ and n in M.__all__ and callable(getattr(ap, n))
    assert "chroma.hip" in _build.SOURCES
    for s in ("ap_chroma_max_out", "ap_chroma_fold_f32", "ap_chroma_max_smooth", "ap_chroma_cens_f32"):
        assert s in _x.ABI_SYMBOLS and getattr(_x.lib(), s) is not None
    assert _x.lib().ap_chroma_max_out() >= 36 and _x.lib().ap_chroma_max_smooth() >= 129


def test_signatures_are_librosas():
    def defaults(f):
        sig = inspect.signature(f)
        assert all(p.kind is KW for p in sig.parameters.values() if p.kind is not inspect.Parameter.VAR_KEYWORD), f
        return {k: p.default for k, p in sig.parameters.items()}

    assert defaults(ap.chroma_stft) == dict(
        y=None, sr=22050, S=None, norm=np.inf, n_fft=2048, hop_length=512, win_length=None, window="hann", center=True,
        pad_mode="constant", tuning=0.0, n_chroma=12, ctroct=5.0, octwidth=2, base_c=True)
    assert defaults(ap.chroma_cqt) == dict(
        y=None, sr=22050, C=None, hop_length=512, fmin=None, norm=np.inf, threshold=0.0, tuning=0.0, n_chroma=12, n_octaves=7,
        window=None, bins_per_octave=36, cqt_mode="full")
    assert defaults(ap.chroma_cens) == dict(
        y=None, sr=22050, C=None, hop_length=512, fmin=None, tuning=0.0, n_chroma=12, n_octaves=7, bins_per_octave=36,
        cqt_mode="full", window=None, norm=2, win_len_smooth=41, smoothing_window="hann")
    sig = inspect.signature(ap.tonnetz)
    assert list(sig.parameters) == ["y", "sr", "chroma", "kwargs"]
    assert sig.parameters["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert [sig.parameters[k].default for k in ("y", "sr", "chroma")] == [None, 22050, None]
    E = inspect.Parameter.empty
    assert defaults(ap.chroma_filterbank) == dict(sr=E, n_fft=E, n_chroma=12, tuning=0.0, ctroct=5.0, octwidth=2, norm=2, base_c=True)
    sig = inspect.signature(ap.cq_to_chroma)
    assert list(sig.parameters) == ["n_input", "bins_per_octave", "n_chroma", "fmin", "window", "base_c"]
    assert all(sig.parameters[k].kind is KW for k in list(sig.parameters)[1:])
    assert [sig.parameters[k].default for k in list(sig.parameters)[1:]] == [12, 12, None, None, True]
    for f in (ap.chroma_stft, ap.chroma_cqt, ap.chroma_cens, ap.tonnetz):
        assert "librosa" in f.__doc__ and "None" in f.__doc__ and "tuning" in f.__doc__      # the default that differs is documented


@pytest.mark.parametrize("kw", [
    dict(sr=22050, n_fft=2048), dict(sr=22050, n_fft=2048, octwidth=None), dict(sr=22050, n_fft=2048, norm=1, base_c=False),
    dict(sr=22050, n_fft=2048, norm=np.inf, tuning=0.3), dict(sr=22050, n_fft=2048, norm=None, ctroct=4.0, octwidth=1.5),
    dict(sr=8000, n_fft=401, n_chroma=24), dict(sr=16000, n_fft=512, n_chroma=36, tuning=-0.25), dict(sr=8000, n_fft=64, n_chroma=7),
], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_chroma_filterbank_against_the_definition(kw):
    w = ap.chroma_filterbank(**kw)
    assert w.dtype == np.float32 and w.shape == (kw.get("n_chroma", 12), 1 + kw["n_fft"] // 2) and not w.flags.writeable
    want = R.chroma_filterbank(**kw)
    # float64 on both sides, rounded once: half an ulp of float32, plus the libm's last bits through exp and log2
    assert np.all(np.abs(w.astype(np.float64) - want) <= R.U * np.abs(want) + 1e-12 * np.abs(want).max() + 2.0 ** -150)


def test_chroma_filterbank_facts():
    w = ap.chroma_filterbank(sr=22050, n_fft=2048)
    assert w.shape == (12, 1025)
    f = np.arange(1025) * 22050.0 / 2048
    for hz, row in ((440.0, 9), (1760.0, 9), (261.63, 0)):
        k = int(np.argmin(np.abs(f - hz)))
        assert int(np.argmax(w[:, k])) == row, (hz, k, w[:, k])
    u = ap.chroma_filterbank(sr=22050, n_fft=2048, octwidth=None, norm=2).astype(np.float64)
    np.testing.assert_allclose(np.sqrt((u * u).sum(axis=0)), 1.0, rtol=0, atol=12 * R.U)
    a = ap.chroma_filterbank(sr=22050, n_fft=2048, base_c=False)
    np.testing.assert_array_equal(np.roll(a, -3, axis=0), w)


def test_cq_to_chroma_facts():
    w = ap.cq_to_chroma(84, bins_per_octave=12)
    assert w.dtype == np.float32 and w.shape == (12, 84) and not w.flags.writeable
    np.testing.assert_array_equal(w, np.tile(np.eye(12, dtype=np.float32), 7))
    w = ap.cq_to_chroma(252, bins_per_octave=36)
    assert w.shape == (12, 252)
    assert set(np.flatnonzero(w[0]) % 36) == {35, 0, 1} and np.flatnonzero(w[0]).size == 21
    np.testing.assert_array_equal(w.sum(axis=0), np.ones(252, np.float32))
    w = ap.cq_to_chroma(36, bins_per_octave=12, fmin=55.0)
    assert int(np.argmax(w[:, 0])) == 9 and w[9, 0] == 1.0
    w = ap.cq_to_chroma(36, bins_per_octave=12, fmin=55.0, base_c=False)
    assert int(np.argmax(w[:, 0])) == 0
    with pytest.raises(ValueError, match="bins_per_octave"):
        ap.cq_to_chroma(84, bins_per_octave=30, n_chroma=12)


@pytest.mark.parametrize("kw", [
    dict(n_input=84), dict(n_input=252, bins_per_octave=36), dict(n_input=100, bins_per_octave=24, n_chroma=12, fmin=55.0),
    dict(n_input=50, bins_per_octave=36, n_chroma=36, fmin=100.0, base_c=False), dict(n_input=5, bins_per_octave=12),
    dict(n_input=252, bins_per_octave=36, window=np.array([0.25, 0.5, 0.25])), dict(n_input=60, bins_per_octave=12, window=np.array([1.0, -2.0, 0.5, 3.0])),
], ids=lambda kw: "-".join(f"{k}{np.size(v) if k == 'window' else v}" for k, v in kw.items()))
def test_cq_to_chroma_against_the_definition(kw):
    kw = dict(kw)
    n = kw.pop("n_input")
    w = ap.cq_to_chroma(n, **kw)
    want = R.cq_to_chroma(n, **kw)
    assert w.shape == want.shape
    assert np.all(np.abs(w.astype(np.float64) - want) <= R.U * np.abs(want) + 1e-15)


@pytest.mark.parametrize("n_chroma", [12, 24, 7])
def test_tonnetz_basis(n_chroma):
    p = M._phi64(n_chroma)
    assert p.shape == (6, n_chroma) and p.dtype == np.float64
    np.testing.assert_allclose(p, R.phi(n_chroma), rtol=0, atol=1e-15)
    if n_chroma % 12 == 0:
        assert np.all(np.abs(p.sum(axis=1)) <= 1e-13)
    r = np.sqrt(p[0::2] ** 2 + p[1::2] ** 2)
    np.testing.assert_allclose(r, np.array([1.0, 1.0, 0.5])[:, None] * np.ones((1, n_chroma)), rtol=0, atol=1e-14)


def test_every_rejected_argument_by_name():
    cap = _x.lib().ap_chroma_max_out()
    smooth = _x.lib().ap_chroma_max_smooth()
    C2 = np.zeros((252, 4), np.float32)
    cases = [
        (ap.chroma_stft, dict(), "y and S"), (ap.chroma_stft, dict(y=Y, S=C2), "y and S"),
        (ap.chroma_stft, dict(y=Y, tuning=None), "tuning"), (ap.chroma_stft, dict(y=Y, norm=3), "norm"),
        (ap.chroma_stft, dict(y=Y, n_chroma=0), "n_chroma"), (ap.chroma_stft, dict(y=Y, n_chroma=cap + 1), "n_chroma"),
        (ap.chroma_stft, dict(y=Y, n_fft=1), "n_fft"), (ap.chroma_stft, dict(y=Y, hop_length=0), "hop_length"),
        (ap.chroma_stft, dict(y=Y, sr=0), "sr"), (ap.chroma_stft, dict(y=Y, octwidth=0), "octwidth"),
        (ap.chroma_stft, dict(y=Y, tuning=float("nan")), "tuning"),
        (ap.chroma_stft, dict(S=np.zeros((2, 2, 5, 5), np.float32)), "S must be 2D"),
        (ap.chroma_stft, dict(S=np.zeros((5, 4), np.complex64)), "S must be real"),
        (ap.chroma_cqt, dict(), "y and C"), (ap.chroma_cqt, dict(y=Y, C=C2), "y and C"),
        (ap.chroma_cqt, dict(y=Y, tuning=None), "tuning"), (ap.chroma_cqt, dict(y=Y, cqt_mode="hybrid"), "cqt_mode"),
        (ap.chroma_cqt, dict(y=Y, norm=0), "norm"), (ap.chroma_cqt, dict(y=Y, n_chroma=5), "bins_per_octave"),
        (ap.chroma_cqt, dict(y=Y, n_chroma=cap + 1, bins_per_octave=cap + 1), "n_chroma"),
        (ap.chroma_cqt, dict(y=Y, n_octaves=0), "n_octaves"), (ap.chroma_cqt, dict(y=Y, hop_length=0), "hop_length"),
        (ap.chroma_cqt, dict(y=Y, hop_length=2.5), "hop_length"), (ap.chroma_cqt, dict(y=Y, threshold="a"), "threshold"),
        (ap.chroma_cqt, dict(y=Y, fmin=-1.0), "fmin"), (ap.chroma_cqt, dict(y=Y, window=np.ones((2, 2))), "window"),
        (ap.chroma_cqt, dict(y=Y, bins_per_octave=0), "bins_per_octave"), (ap.chroma_cqt, dict(y=Y, sr=-1), "sr"),
        (ap.chroma_cqt, dict(C=np.zeros(5, np.float32)), "C must be 2D"),
        (ap.chroma_cens, dict(), "y and C"), (ap.chroma_cens, dict(y=Y, tuning=None), "tuning"),
        (ap.chroma_cens, dict(y=Y, norm=7), "norm"), (ap.chroma_cens, dict(y=Y, cqt_mode="hybrid"), "cqt_mode"),
        (ap.chroma_cens, dict(y=Y, win_len_smooth=-1), "win_len_smooth"), (ap.chroma_cens, dict(y=Y, win_len_smooth=2.5), "win_len_smooth"),
        (ap.chroma_cens, dict(y=Y, win_len_smooth=smooth - 1), "cap"), (ap.chroma_cens, dict(y=Y, smoothing_window="kaiser"), "window"),
        (ap.chroma_cens, dict(y=Y, smoothing_window=np.ones((2, 2))), "smoothing_window"),
        (ap.chroma_cens, dict(y=Y, smoothing_window=np.ones(smooth + 1)), "cap"),
        (ap.tonnetz, dict(), "y and chroma"), (ap.tonnetz, dict(y=Y, chroma=C2), "y and chroma"),
        (ap.tonnetz, dict(y=Y, tuning=None), "tuning"), (ap.tonnetz, dict(chroma=np.zeros(12, np.float32)), "chroma must be 2D"),
        (ap.tonnetz, dict(chroma=np.zeros((12, 3), np.complex64)), "chroma must be real"),
        (ap.tonnetz, dict(chroma=np.zeros((12, 0), np.float32)), "at least one"),
        (ap.chroma_filterbank, dict(sr=22050, n_fft=1), "n_fft"), (ap.chroma_filterbank, dict(sr=0, n_fft=64), "sr"),
        (ap.chroma_filterbank, dict(sr=8000, n_fft=64, n_chroma=0), "n_chroma"),
        (ap.chroma_filterbank, dict(sr=8000, n_fft=64, tuning=None), "tuning"),
        (ap.chroma_filterbank, dict(sr=8000, n_fft=64, norm="max"), "norm"),
        (ap.chroma_filterbank, dict(sr=8000, n_fft=64, octwidth=-1), "octwidth"),
        (ap.chroma_filterbank, dict(sr=8000, n_fft=64, ctroct=float("inf")), "ctroct"),
    ]
    for f, kw, word in cases:
        with pytest.raises(ValueError, match=word):
            f(**kw)
    for n, kw, word in ((0, dict(), "n_input"), (12, dict(bins_per_octave=0), "bins_per_octave"), (12, dict(n_chroma=0), "n_chroma"),
                        (12, dict(fmin=0.0), "fmin"), (12, dict(window=np.ones((2, 2))), "window"), (12, dict(bins_per_octave=13), "multiple")):
        with pytest.raises(ValueError, match=word):
            ap.cq_to_chroma(n, **kw)
    with pytest.raises(TypeError):
        ap.chroma_cqt(Y)                                    # keyword-only
    with pytest.raises(ValueError, match="tuning"):         # cqt itself keeps raising
        ap.cqt(Y, tuning=None)


def test_smoothing_taps():
    t = M._smoothing_taps(41, "hann")
    assert t.dtype == np.float32 and t.shape == (43,) and not t.flags.writeable
    assert t[0] == 0.0 and t[-1] == 0.0 and abs(float(t.astype(np.float64).sum()) - 1.0) <= 43 * R.U
    np.testing.assert_allclose(t, R.hann_taps(41), rtol=0, atol=4 * R.U * float(t.max()))
    np.testing.assert_array_equal(t, t[::-1])
    assert M._smoothing_taps(None, "hann") is None and M._smoothing_taps(0, "hann") is None
    np.testing.assert_array_equal(M._smoothing_taps(41, np.array([0.5, 0.25])), np.array([0.5, 0.25], np.float32))
    w = _x.generate_window_host("hamming", 7, False).astype(np.float64)
    np.testing.assert_array_equal(M._smoothing_taps(5, "hamming"), (w / w.sum()).astype(np.float32))


def test_the_banks_are_cached_under_their_content():
    M._host_bank_cache.clear()
    a = M._cached_host(("cq", 252, 36, 12, None, None), lambda: ap.cq_to_chroma(252, bins_per_octave=36))
    b = M._cached_host(("cq", 252, 36, 12, None, None), lambda: 1 / 0)
    assert a is b and len(M._host_bank_cache) == 1
    assert a[0].shape == (12, 252) and len(a[1]) == 32
    c = M._cached_host(("other key",), lambda: ap.cq_to_chroma(252, bins_per_octave=36, fmin=R.C1))
    assert c is not a and c[1] == a[1]                    # the same content has the same digest: one device copy
    d = M._cached_host(("cq", 252, 36, 12, 55.0, None), lambda: ap.cq_to_chroma(252, bins_per_octave=36, fmin=55.0))
    assert d[1] != a[1]
    e = M._cached_host(("t",), lambda: np.ascontiguousarray(a[0].reshape(24, 126)))
    assert e[1] != a[1]                                   # the shape is part of the content
    for i in range(40):
        M._cached_host(("fill", i), lambda: np.zeros((1, 1), np.float32))
    assert len(M._host_bank_cache) <= 32
    M._host_bank_cache.clear()
