"""CPU: the public face of pyin, its host tables, its rejections, and the share of decisive frames of the GPU test's
inputs, shown with the reference alone."""

import inspect
import math
import os

import numpy as np
import pytest

import pyin_ref as R
import yin_ref as Y
from conftest import ROOT

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _extension as _x
from mlx_audio_primitives_amd import pitch

C2, C7 = 65.40639132514966, 2093.004522404789
TABLES = lambda n_lags, **kw: pitch._pyin_tables(fmin=C2, fmax=C7, sr=22050, hop=512, n_lags=n_lags, **kw)  # noqa: E731
DEFAULTS = dict(sr=22050, frame_length=2048, win_length=None, hop_length=None, n_thresholds=100, beta_parameters=(2, 18),
                boltzmann_parameter=2, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01,
                center=True, pad_mode="constant")


def test_name_signature_and_symbols():
    assert "pyin" in ap.__all__ and ap.pyin is pitch.pyin
    sig = inspect.signature(ap.pyin).parameters
    assert list(sig)[0] == "y" and all(p.kind is p.KEYWORD_ONLY for n, p in sig.items() if n != "y")
    assert sig["fmin"].default is inspect.Parameter.empty and sig["fmax"].default is inspect.Parameter.empty
    assert all(sig[name].default == value for name, value in DEFAULTS.items()) and math.isnan(sig["fill_na"].default)
    header = open(os.path.join(ROOT, "include", "audioprims.h")).read()
    for sym in ("ap_pyin_max_bins", "ap_pyin_max_width", "ap_pyin_observe_f32", "ap_pyin_decode_f32"):
        assert f" {sym}(" in header and sym in _x.ABI_SYMBOLS and getattr(_x.lib(), sym) is not None
    assert _x.lib().ap_pyin_max_bins() >= 1024 and _x.lib().ap_pyin_max_width() >= 401


def test_default_tables():
    t = TABLES(329)
    assert (t["n_bins"], t["W"], t["bps"]) == (601, 101, 10)
    x = np.arange(101) / 100
    closed = 1.0 - (1.0 - x) ** 19 - 19 * x * (1.0 - x) ** 18            # I_x(2, 18)
    np.testing.assert_allclose(t["beta"], np.maximum(np.diff(closed), 0), rtol=1e-6, atol=1e-12)
    for a, b in ((2, 18), (1, 1), (5, 3)):
        beta = TABLES(329, beta_parameters=(a, b))["beta"]
        assert abs(float(beta.astype(np.float64).sum()) - 1.0) < 1e-6 and (beta >= 0).all()
        try:
            from scipy.stats import beta as sbeta
        except ImportError:
            continue
        np.testing.assert_allclose(beta, np.diff(sbeta.cdf(x, a, b)), rtol=1e-6, atol=1e-12)
    k = np.arange(166.0)
    np.testing.assert_array_equal(t["thr"], (x[1:]).astype(np.float32))
    np.testing.assert_array_equal(t["ea"], np.exp(-2 * k).astype(np.float32))
    np.testing.assert_allclose(t["nz"][1:] * np.cumsum(t["ea"].astype(np.float64))[:-1], 1.0, rtol=1e-6)     # the ranks sum to 1
    assert t["li"] == np.float32(math.log(1 / 1202)) and t["freq"][0] == np.float32(C2)
    np.testing.assert_allclose(t["freq"][120] / t["freq"][0], 2.0, rtol=1e-6)


def test_band_tables_are_transition_local():
    for n, W in [(2, 1), (2, 2), (3, 2), (8, 4), (9, 8), (64, 64), (65, 3), (601, 101)]:
        lw, lz, ls = pitch._pyin_band(n, W, 0.25)
        h, dense = W // 2, np.zeros((n, n))
        for i in range(n):
            for j in range(max(0, i - h), min(n - 1, i + h) + 1):
                dense[i, j] = math.exp(float(lw[j - i + h]) - float(lz[i]))
        np.testing.assert_allclose(dense, ap.transition_local(n, W, window="triangle"), atol=1e-6, err_msg=f"{n} {W}")
        np.testing.assert_allclose(np.exp(ls.astype(np.float64)).reshape(2, 2), ap.transition_loop(2, 0.75), atol=1e-7)


@pytest.mark.parametrize("kw,match", [
    (dict(beta_parameters=(2.5, 18)), "beta_parameters"), (dict(switch_prob=-0.1), "switch_prob"), (dict(switch_prob=1.5), "switch_prob"),
    (dict(resolution=0.0), "resolution"), (dict(resolution=1.0), "resolution"), (dict(fmin=100.0, fmax=110.0), "transition width"),
    (dict(fmin=500.0, fmax=100.0), "less than fmax")])
def test_rejections_come_before_the_device(kw, match):
    with pytest.raises(ValueError, match=match):
        ap.pyin(np.zeros(4096, np.float32), **{**dict(fmin=C2, fmax=C7), **kw})


@pytest.mark.parametrize("fl,hop,fmin,fmax", [(2048, 512, C2, C7), (512, 128, 200.0, 2000.0)])
def test_inputs_of_the_gpu_test_are_decisive(fl, hop, fmin, fmax):
    """The reference alone on float32-rounded float64 curves of test_gpu_pyin.py's signals: at most 0.5 % non-decisive frames."""
    lo, hi, W = Y.periods(22050, fmin, fmax, fl)
    sig = Y.signals(22050, 11025)
    for name in ("vibrato", "glide", "bursts", "noise"):
        curve = Y.cmnd64(Y.frames_of(sig[name].astype(np.float32), fl, hop, True), lo, hi, W)[:, lo:hi + 1].T.astype(np.float32)
        n_bins = int(math.floor(120 * math.log2(fmax / fmin))) + 1
        P, vsum, dec = R.observe64(curve, lo, 22050.0, fmin, 10, n_bins, TABLES(hi - lo + 1), 0.01)
        assert 1.0 - dec.mean() <= 0.005 and (P >= 0).all() and (vsum <= 1.0 + 1e-6).all() and (vsum[1:-1] > 0).all(), name
