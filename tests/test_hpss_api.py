"""CPU: hpss / hpss_medians / hpss_audio / harmonic / percussive are exported with librosa's signatures, validate
their arguments before any device work and fail loudly without a GPU.  The C entry point rejects bad geometry with a
status, not a launch."""

import ctypes
import inspect

import numpy as np
import pytest

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _build
from mlx_audio_primitives_amd import _extension as ext

NAMES = ("hpss", "hpss_medians", "hpss_audio", "harmonic", "percussive")


def test_exported():
    from mlx_audio_primitives_amd import decompose

    for name in NAMES:
        assert name in ap.__all__ and callable(getattr(ap, name)) and getattr(ap, name) is getattr(decompose, name)
    assert "hpss.hip" in _build.SOURCES
    for sym in ("ap_hpss_fused", "ap_hpss_f32"):
        assert sym in ext.ABI_SYMBOLS and getattr(ext.lib(), sym) is not None


def test_signatures_follow_librosa():
    p = inspect.signature(ap.hpss).parameters
    assert list(p) == ["S", "kernel_size", "power", "mask", "margin"]
    assert p["S"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and p["S"].default is inspect.Parameter.empty
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in p.items() if k != "S")
    assert {k: p[k].default for k in list(p)[1:]} == {"kernel_size": 31, "power": 2.0, "mask": False, "margin": 1.0}
    q = inspect.signature(ap.hpss_medians).parameters
    assert list(q) == ["S", "kernel_size"] and q["kernel_size"].kind is inspect.Parameter.KEYWORD_ONLY
    assert q["kernel_size"].default == 31
    for fn in (ap.hpss_audio, ap.harmonic, ap.percussive):
        r = inspect.signature(fn).parameters
        assert list(r) == ["y", "kernel_size", "power", "margin", "n_fft", "hop_length", "win_length", "window", "center",
                           "pad_mode"]
        assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in r.items() if k != "y")
        assert {k: r[k].default for k in list(r)[1:]} == {
            "kernel_size": 31, "power": 2.0, "margin": 1.0, "n_fft": 2048, "hop_length": None, "win_length": None,
            "window": "hann", "center": True, "pad_mode": "constant"}
    with pytest.raises(TypeError):
        ap.hpss(np.zeros((4, 4), np.float32), 31)          # keyword-only, as in librosa


S = np.zeros((2, 9, 12), np.float32)
Y = np.zeros(8192, np.float32)
KS = "kernel_size must be an integer in 1 .. 255"


@pytest.mark.parametrize("kw,match", [
    (dict(kernel_size=0), KS), (dict(kernel_size=256), KS), (dict(kernel_size=31.0), KS), (dict(kernel_size=True), KS),
    (dict(kernel_size=(31, 0)), KS), (dict(kernel_size=(31, 31, 31)), KS), (dict(kernel_size=-3), KS),
    (dict(margin=0.5), r"Margins must be >= 1\.0\. A typical range is between 1 and 10\."),
    (dict(margin=(1.0, 0.99)), "Margins must be >= 1.0"),
    (dict(margin=float("nan")), "Margins must be >= 1.0"),
    (dict(power=0.0), "power must be strictly positive"),
    (dict(power=-1.0), "power must be strictly positive"),
])
def test_validation_errors(kw, match):
    """Raised before any device work: these hold with and without a GPU."""
    with pytest.raises(ValueError, match=match):
        ap.hpss(S, **kw)
    with pytest.raises(ValueError, match=match):
        ap.hpss_audio(Y, **kw)
    with pytest.raises(ValueError, match=match):
        ap.harmonic(Y, **kw)
    with pytest.raises(ValueError, match=match):
        ap.percussive(Y, **kw)
    if "kernel_size" in kw:
        with pytest.raises(ValueError, match=match):
            ap.hpss_medians(S, **kw)


def test_more_validation_errors():
    for fn in (ap.hpss, ap.hpss_medians):
        with pytest.raises(ValueError, match="S must be 2D or 3D, got 1D"):
            fn(np.zeros(8, np.float32))
        with pytest.raises(ValueError, match="S must be 2D or 3D, got 4D"):
            fn(np.zeros((1, 2, 3, 4), np.float32))
        with pytest.raises(ValueError, match="S must be float32 or complex64, got torch.float64"):
            fn(np.zeros((4, 4), np.float64))
        with pytest.raises(ValueError, match="S must be float32 or complex64, got torch.complex128"):
            fn(np.zeros((4, 4), np.complex128))
        with pytest.raises(ValueError, match="S must be float32 or complex64"):
            fn(np.zeros((4, 4), np.int16))
    with pytest.raises(ValueError, match="y must be 1D or 2D, got 3D"):
        ap.hpss_audio(np.zeros((1, 2, 4096), np.float32))


def test_no_gpu_is_a_loud_error():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for call in (lambda: ap.hpss(S), lambda: ap.hpss(S.astype(np.complex64), mask=True), lambda: ap.hpss_medians(S),
                 lambda: ap.hpss_audio(Y), lambda: ap.harmonic(Y), lambda: ap.percussive(Y)):
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()


def test_fused_predicate():
    lib = ext.lib()
    assert lib.ap_hpss_fused(31, 31) == 1
    for k in ((31, 17), (17, 31), (1, 1), (255, 255), (32, 32), (0, 0)):
        assert lib.ap_hpss_fused(*k) == 0


def test_c_entry_validates_before_launching():
    """Status codes and messages for bad arguments; the pointers are never dereferenced on these paths."""
    lib = ext.lib()
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    s, h, p = base, base + 4096, base + 8192
    inf = float("inf")

    def err(*a):
        rc = lib.ap_hpss_f32(*a)
        assert rc in (ext.AP_ERR_INVALID, ext.AP_ERR_UNSUPPORTED), rc
        return rc, lib.ap_last_error().decode()

    #    S  cplx B  F  T rs  kh  kp  mh   mp   pow mode gen  h  p rs  stream
    assert err(None, 0, 1, 4, 8, 8, 31, 31, 1.0, 1.0, 2.0, 0, 0, h, p, 8, None)[0] == ext.AP_ERR_INVALID
    assert err(s, 0, 1, 4, 8, 8, 31, 31, 1.0, 1.0, 2.0, 0, 0, None, None, 8, None)[0] == ext.AP_ERR_INVALID
    for B, F, T in ((0, 4, 8), (1, 0, 8), (1, 4, 0), (1, -4, 8)):
        rc, msg = err(s, 0, B, F, T, 8, 31, 31, 1.0, 1.0, 2.0, 0, 0, h, p, 8, None)
        assert rc == ext.AP_ERR_INVALID and "non-empty" in msg
    for kh, kp in ((0, 31), (31, 0), (256, 31), (31, 256), (-1, -1)):
        for general in (0, 1):
            rc, msg = err(s, 0, 1, 4, 8, 8, kh, kp, 1.0, 1.0, 2.0, 0, general, h, p, 8, None)
            assert rc == ext.AP_ERR_INVALID and KS in msg
    assert "row strides" in err(s, 0, 1, 4, 8, 7, 31, 31, 1.0, 1.0, 2.0, 0, 0, h, p, 8, None)[1]
    assert "row strides" in err(s, 1, 1, 4, 8, 8, 31, 31, 1.0, 1.0, 2.0, 0, 0, h, p, 7, None)[1]
    assert "Margins must be >= 1.0" in err(s, 0, 1, 4, 8, 8, 31, 31, 1.0, 0.5, 2.0, 0, 0, h, p, 8, None)[1]
    assert "power must be strictly positive" in err(s, 0, 1, 4, 8, 8, 31, 31, 1.0, 1.0, -inf, 0, 0, h, p, 8, None)[1]
    assert "mode must be" in err(s, 0, 1, 4, 8, 8, 31, 31, 1.0, 1.0, inf, 5, 0, h, p, 8, None)[1]
    rc, msg = err(s, 0, 1, 4, 8, 8, 31, 31, 1.0, 1.0, 2.0, 0, 0, s, p, 8, None)          # in place
    assert rc == ext.AP_ERR_INVALID and "overlaps S" in msg
    rc, msg = err(s, 1, 1, 4, 8, 8, 31, 31, 1.0, 1.0, 2.0, 0, 0, h, s + 8 * 31, 8, None)  # the last complex value of S
    assert rc == ext.AP_ERR_INVALID and "overlaps S" in msg
    assert "outputs overlap" in err(s, 0, 1, 4, 8, 8, 31, 31, 1.0, 1.0, 2.0, 1, 0, h, h + 64, 8, None)[1]
    # extents the 32-bit (f, t) arithmetic cannot address: a status, never a wrapped index
    far = base + (1 << 50)
    rc, msg = err(s, 0, 1, (1 << 28) + 1, 8, 8, 31, 31, 1.0, 1.0, 2.0, 2, 0, far, None, 8, None)
    assert rc == ext.AP_ERR_UNSUPPORTED and "2^28" in msg
    rc, msg = err(s, 0, 1, 4, (1 << 31) + 8, (1 << 31) + 8, 31, 31, 1.0, 1.0, 2.0, 2, 1, far, None, (1 << 31) + 8, None)
    assert rc == ext.AP_ERR_UNSUPPORTED and "2^28" in msg
    rc, msg = err(s, 0, 1 << 33, 4, 8, 8, 31, 31, 1.0, 1.0, 2.0, 2, 0, far, None, 8, None)
    assert rc == ext.AP_ERR_UNSUPPORTED and "tiles" in msg
