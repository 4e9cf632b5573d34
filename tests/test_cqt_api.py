"""CPU: the host side of cqt / vqt / cqt_frequencies (mlx-audio-primitives_amd/cqt.py): the signatures, the band
frequencies against the closed form, the filter lengths of the named configurations, the packed bank against the
float64 definition in tests/cqt_ref.py, every rejected parameter, the bank cache.  Every check happens before a device
is asked for, so nothing here needs one."""

import importlib
import inspect

import numpy as np
import pytest
import torch

import cqt_ref as R

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _extension as _x

C = importlib.import_module("mlx_audio_primitives_amd.cqt")

Y = np.zeros(4096, np.float32)
SMALL = dict(sr=8000, fmin=500.0, n_bins=17)


def bank(func="cqt", **kw):
    """The packed host bank the public call would use."""
    d = {k: p.default for k, p in inspect.signature(getattr(ap, func)).parameters.items() if k != "y"}
    d.update(kw)
    args, _ = C._parameters(d["sr"], d["hop_length"], d["fmin"], d["n_bins"], d["bins_per_octave"], d["tuning"], d["filter_scale"],
                            d["norm"], d["sparsity"], d["window"], d["scale"], d["pad_mode"], d["dtype"],
                            d["gamma"] if func == "vqt" else 0.0, d.get("intervals", "equal"))
    return C._bank(*args)


def test_names_are_exported():
    for n in ("cqt", "vqt", "cqt_frequencies"):
        assert n in ap.__all__ and callable(getattr(ap, n))
    for s in ("ap_cqt_f32", "ap_cqt_max_taps"):
        assert s in _x.ABI_SYMBOLS and getattr(_x.lib(), s) is not None
    assert _x.lib().ap_cqt_max_taps() >= 11686


def test_signatures_are_librosas():
    sig = inspect.signature(ap.cqt)
    names = list(sig.parameters)
    assert names == ["y", "sr", "hop_length", "fmin", "n_bins", "bins_per_octave", "tuning", "filter_scale", "norm", "sparsity",
                     "window", "scale", "pad_mode", "res_type", "dtype"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[1:])
    assert {n: sig.parameters[n].default for n in names[1:]} == dict(
        sr=22050, hop_length=512, fmin=None, n_bins=84, bins_per_octave=12, tuning=0.0, filter_scale=1, norm=1, sparsity=0.01,
        window="hann", scale=True, pad_mode="constant", res_type="soxr_hq", dtype=None)
    sig = inspect.signature(ap.vqt)
    names = list(sig.parameters)
    assert names == ["y", "sr", "hop_length", "fmin", "n_bins", "intervals", "gamma", "bins_per_octave", "tuning", "filter_scale",
                     "norm", "sparsity", "window", "scale", "pad_mode", "res_type", "dtype"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[1:])
    assert {n: sig.parameters[n].default for n in names[1:]} == dict(
        sr=22050, hop_length=512, fmin=None, n_bins=84, intervals="equal", gamma=None, bins_per_octave=12, tuning=0.0,
        filter_scale=1, norm=1, sparsity=0.01, window="hann", scale=True, pad_mode="constant", res_type="soxr_hq", dtype=None)
    sig = inspect.signature(ap.cqt_frequencies)
    assert list(sig.parameters) == ["n_bins", "fmin", "bins_per_octave", "tuning"]
    assert sig.parameters["bins_per_octave"].default == 12 and sig.parameters["tuning"].default == 0.0
    assert sig.parameters["fmin"].default is inspect.Parameter.empty


def test_cqt_frequencies_closed_form():
    for n, fmin, bpo, tuning in ((84, R.C1, 12, 0.0), (17, 500.0, 12, 0.0), (37, 800.0, 36, 0.25), (1, 440.0, 7, -0.5)):
        f = ap.cqt_frequencies(n, fmin=fmin, bins_per_octave=bpo, tuning=tuning)
        assert f.dtype == np.float64 and f.shape == (n,)
        want = np.array([fmin * 2.0 ** ((k + tuning) / bpo) for k in range(n)])
        np.testing.assert_allclose(f, want, rtol=4e-16)
        np.testing.assert_array_equal(f, R.frequencies(n, fmin, bpo, tuning))
    assert ap.cqt_frequencies(84, R.C1)[12] == pytest.approx(2 * R.C1, rel=1e-15)
    for bad in (dict(n_bins=0, fmin=1.0), dict(n_bins=2.0, fmin=1.0), dict(n_bins=4, fmin=0.0), dict(n_bins=4, fmin=-3.0),
                dict(n_bins=4, fmin=1.0, bins_per_octave=0), dict(n_bins=4, fmin=1.0, tuning=float("nan"))):
        with pytest.raises(ValueError):
            ap.cqt_frequencies(**bad)


@pytest.mark.parametrize("func, kw, first, last, total", [
    ("cqt", dict(), 11685, 97, 206580),
    ("cqt", dict(sr=8000, fmin=500.0, n_bins=17), 277, 111, None),
    ("cqt", dict(sr=8000, fmin=33.8, n_bins=3), 4103, 3655, None),
    ("cqt", dict(sr=8000, fmin=800.0, n_bins=37, bins_per_octave=36), 519, 259, None),
    ("vqt", dict(sr=8000, fmin=100.0, n_bins=25), 421, 221, None),
], ids=["defaults", "17bins", "3bins-long", "bpo36", "vqt"])
def test_bank_lengths_and_content(func, kw, first, last, total):
    """The lengths of the named configurations, and the packed float32 bank against the float64 definition: m0 and the
    scale exact, every tap within 4 u of the filter's largest tap (the project's windows are float32 values: u for the
    window's rounding, u for what that does to the norm, sqrt(2) u for the complex tap's own rounding)."""
    taps, off, m0, s, _ = bank(func, **kw)
    L = np.diff(off)
    assert (L[0], L[-1]) == (first, last) and np.all(np.diff(L) <= 0)
    if total is not None:
        assert L.sum() == total and off[-1] == total
    assert taps.dtype == np.complex64 and off.dtype == np.int64 and m0.dtype == np.int32 and s.dtype == np.float32
    assert np.all((L % 2 == 1))                                  # odd unless N_k is an exact even integer
    ref_kw = dict(sr=22050, fmin=R.C1, n_bins=84)
    ref_kw.update(kw)
    want, m0_ref, s_ref = R.real_bank(func, ref_kw)
    np.testing.assert_array_equal(m0, m0_ref)
    np.testing.assert_array_equal(s, s_ref.astype(np.float32))
    for k in (0, len(L) // 2, len(L) - 1):
        g = taps[off[k]:off[k + 1]].astype(np.complex128)
        assert np.max(np.abs(g - want[k])) <= 4.0 * R.U * np.max(np.abs(want[k]))
        assert abs(np.abs(g).sum() - 1.0) < 1e-6                 # norm = 1


def test_norm_scale_and_gamma():
    for norm, measure in ((1, lambda g: np.abs(g).sum()), (2, lambda g: np.sqrt((np.abs(g) ** 2).sum())), (np.inf, lambda g: np.abs(g).max())):
        taps, off, _, _, _ = bank(norm=norm, **SMALL)
        for k in (0, 16):
            assert abs(measure(taps[off[k]:off[k + 1]].astype(np.complex128)) - 1.0) < 1e-6
    taps, off, _, _, _ = bank(norm=None, window="boxcar", **SMALL)
    np.testing.assert_allclose(np.abs(taps), 1.0, rtol=1e-6)
    _, N, _, _ = R.lengths(8000, 500.0, 17)
    np.testing.assert_array_equal(bank(scale=False, **SMALL)[3], N.astype(np.float32))
    np.testing.assert_array_equal(bank(scale=True, **SMALL)[3], np.sqrt(N).astype(np.float32))
    # vqt with gamma = 0 is cqt; the default gamma shortens the low bands
    assert bank("vqt", gamma=0, **SMALL)[4] == bank("cqt", **SMALL)[4]
    assert np.diff(bank("vqt", **SMALL)[1])[0] < np.diff(bank("cqt", **SMALL)[1])[0]
    alpha = (2 ** (1 / 6) - 1) / (2 ** (1 / 6) + 1)
    assert R.default_gamma(12) == pytest.approx(alpha * 24.7 / 0.108, rel=1e-15)
    _, N_v, _, _ = R.lengths(8000, 500.0, 17, gamma=alpha * 24.7 / 0.108)
    np.testing.assert_array_equal(bank("vqt", scale=False, **SMALL)[3], N_v.astype(np.float32))


@pytest.mark.parametrize("func, kw, match", [
    ("cqt", dict(sr=8000, fmin=500.0, n_bins=37), "n_bins"),                     # the top band passes Nyquist
    ("cqt", dict(sr=8000, fmin=510.0, n_bins=36), "n_bins"),                     # f_35 = 3851 Hz is below 4000, its passband edge is not
    ("cqt", dict(tuning=None), "tuning"),
    ("vqt", dict(intervals="pythagorean"), "intervals"),
    ("vqt", dict(intervals=[1.0, 1.5]), "intervals"),
    ("cqt", dict(dtype=np.complex128), "dtype"),
    ("cqt", dict(dtype=np.float32), "dtype"),
    ("cqt", dict(sr=22050, fmin=0.05, n_bins=3), "cap"),                          # L_0 = 7.6 million taps
    ("cqt", dict(sparsity=1.0), "sparsity"), ("cqt", dict(sparsity=-0.1), "sparsity"),
    ("cqt", dict(hop_length=0), "hop_length"), ("cqt", dict(hop_length=64.0), "hop_length"),
    ("cqt", dict(n_bins=0), "n_bins"), ("cqt", dict(bins_per_octave=0), "bins_per_octave"), ("cqt", dict(fmin=-1.0), "fmin"),
    ("cqt", dict(filter_scale=0), "filter_scale"), ("cqt", dict(norm=3), "norm"), ("cqt", dict(sr=0), "sr"),
    ("vqt", dict(gamma=-1.0), "gamma"), ("cqt", dict(pad_mode="wrap"), "pad_mode"), ("cqt", dict(window="kaiser"), "window"),
])
def test_rejected_parameters_name_themselves(func, kw, match):
    with pytest.raises(ValueError, match=match):
        getattr(ap, func)(Y, **kw)


def test_nyquist_rule_uses_the_window_bandwidth():
    """f_top (1 + 0.5 enbw / Q) <= sr / 2: 1.5 bins for hann, from a 1000-point window otherwise (boxcar: 1)."""
    assert C._enbw("hann") == 1.5
    assert C._enbw("boxcar") == pytest.approx(1.0, abs=1e-12)
    w = np.hamming(1001)[:1000]
    assert C._enbw("hamming") == pytest.approx(1000 * (w ** 2).sum() / w.sum() ** 2, rel=1e-5)
    f, N, _, _ = R.lengths(8000, 500.0, 36)
    Q = 1.0 / ((2 ** (1 / 6) - 1) / (2 ** (1 / 6) + 1))
    assert f[-1] * (1 + 0.5 * 1.5 / Q) <= 4000 < f[-1] * 2 ** (1 / 12) * (1 + 0.5 * 1.5 / Q)
    bank(sr=8000, fmin=500.0, n_bins=36)                                     # the last configuration that fits
    with pytest.raises(ValueError, match="Nyquist"):
        bank(sr=8000, fmin=500.0, n_bins=37)


def test_input_kinds_and_reflect_precondition():
    with pytest.raises(ValueError, match="1D .* or 2D"):
        ap.cqt(np.zeros((2, 3, 4096), np.float32), **SMALL)
    with pytest.raises(ValueError, match="at least one sample"):
        ap.cqt(np.zeros((2, 0), np.float32), **SMALL)
    with pytest.raises(ValueError, match="must be real"):
        ap.cqt(np.zeros(4096, np.complex64), **SMALL)
    with pytest.raises(TypeError, match="window"):
        ap.cqt(Y, window=np.ones(16, np.float32), **SMALL)
    # the longest filter of SMALL reaches 139 samples back: reflect needs 140 samples, the other modes do not
    with pytest.raises(ValueError, match="reflect padding requires"):
        ap.cqt(np.zeros(139, np.float32), pad_mode="reflect", **SMALL)
    for kw in (dict(pad_mode="reflect", y=np.zeros(140, np.float32)), dict(pad_mode="edge", y=np.zeros(5, np.float32)),
               dict(pad_mode="constant", y=np.zeros(5, np.float32))):
        y = kw.pop("y")
        try:
            out = ap.cqt(y, **kw, **SMALL)
        except RuntimeError as e:
            assert not torch.cuda.is_available() and "no HIP device" in str(e)
        else:
            assert tuple(out.shape) == (17, 1 + len(y) // 512)


def test_unused_parameters_are_accepted():
    """res_type and sparsity change nothing: the same bank whatever they say."""
    assert bank(sparsity=0.0, **SMALL)[4] == bank(sparsity=0.5, **SMALL)[4] == bank(**SMALL)[4]
    for kw in (dict(res_type="kaiser_best"), dict(res_type=None), dict(sparsity=0.0), dict(dtype=np.complex64),
               dict(dtype=torch.complex64), dict(hop_length=1), dict(hop_length=100)):
        try:
            ap.cqt(Y, **kw, **SMALL)
        except RuntimeError as e:
            assert not torch.cuda.is_available() and "no HIP device" in str(e)


def test_bank_cache_equal_content_and_no_aliasing():
    """Equal arguments give the same host bank and one device entry; another window is another bank with another key;
    the arrays handed out are read-only, so no caller can change what the next one gets."""
    a, b = bank(**SMALL), bank(**dict(SMALL))
    assert a[4] == b[4] and all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))
    digests = {w: bank(window=w, **SMALL)[4] for w in ("hann", "hamming", "boxcar", "blackman")}
    assert len(set(digests.values())) == 4
    assert bank(window="Hann", **SMALL)[4] == digests["hann"] and bank(window="hanning", **SMALL)[4] == digests["hann"]
    assert not np.array_equal(bank(window="hann", **SMALL)[0], bank(window="hamming", **SMALL)[0])
    for arr in a[:4]:
        with pytest.raises(ValueError):
            arr[...] = 0
    # the device cache, on the host device: equal content, one entry per (content, device); bounded
    before = dict(C._device_bank_cache)
    try:
        C._device_bank_cache.clear()
        d1 = C._device_bank(bank(window="hann", **SMALL), torch.device("cpu"))
        d2 = C._device_bank(bank(window="hann", **SMALL), torch.device("cpu"))
        d3 = C._device_bank(bank(window="hamming", **SMALL), torch.device("cpu"))
        assert all(x is y for x, y in zip(d1, d2)) and len(C._device_bank_cache) == 2
        assert d3[0].data_ptr() != d1[0].data_ptr() and not torch.equal(d3[0], d1[0])
        np.testing.assert_array_equal(d1[0].numpy().view(np.complex64), bank(**SMALL)[0])
        for n in range(40):
            C._device_bank(bank(fmin=500.0 + n, sr=8000, n_bins=3), torch.device("cpu"))
        assert len(C._device_bank_cache) <= 32
    finally:
        C._device_bank_cache.clear()
        C._device_bank_cache.update(before)


def test_no_device_is_a_loud_error():
    """Without a device a valid call raises, float32 and int16 input alike; with one it returns the documented shape."""
    for f in (ap.cqt, ap.vqt):
        for y, kw, shape in ((np.zeros(22050, np.float32), dict(), (84, 44)), (np.zeros((2, 4000), np.int16), SMALL, (2, 17, 8))):
            if torch.cuda.is_available():
                out = f(y, **kw)
                assert tuple(out.shape) == shape and out.dtype == torch.complex64
            else:
                with pytest.raises(RuntimeError, match="no HIP device"):
                    f(y, **kw)
