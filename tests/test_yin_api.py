"""CPU: yin / yin_cmnd are exported with librosa's signature, validate their arguments before any device work,
and fail loudly without a GPU.  The C entry points reject bad geometry with a status, not a launch."""

import ctypes
import inspect

import numpy as np
import pytest

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _build
from mlx_audio_primitives_amd import _extension as ext


def test_exported():
    assert "yin" in ap.__all__ and "yin_cmnd" in ap.__all__
    assert callable(ap.yin) and callable(ap.yin_cmnd)
    assert "yin.hip" in _build.SOURCES
    for sym in ("ap_yin_fused", "ap_yin_f32", "ap_yin_cmnd_f32"):
        assert sym in ext.ABI_SYMBOLS and getattr(ext.lib(), sym) is not None


def test_signatures_follow_librosa():
    p = inspect.signature(ap.yin).parameters
    assert list(p) == ["y", "fmin", "fmax", "sr", "frame_length", "win_length", "hop_length", "trough_threshold",
                       "center", "pad_mode", "return_aperiodicity"]
    assert p["y"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in p.items() if k != "y")
    assert p["fmin"].default is inspect.Parameter.empty and p["fmax"].default is inspect.Parameter.empty
    assert {k: p[k].default for k in list(p)[3:]} == {
        "sr": 22050, "frame_length": 2048, "win_length": None, "hop_length": None, "trough_threshold": 0.1,
        "center": True, "pad_mode": "constant", "return_aperiodicity": False}
    q = inspect.signature(ap.yin_cmnd).parameters
    assert list(q) == ["y", "fmin", "fmax", "sr", "frame_length", "hop_length", "center", "pad_mode"]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in q.items() if k != "y")


Y = np.zeros(8192, np.float32)


@pytest.mark.parametrize("fn", [ap.yin, ap.yin_cmnd], ids=["yin", "yin_cmnd"])
@pytest.mark.parametrize("kw,match", [
    (dict(fmin=500.0, fmax=100.0), r"fmin \(500.0\) must be less than fmax \(100.0\)"),
    (dict(fmin=100.0, fmax=100.0), "must be less than fmax"),
    (dict(fmin=0.0, fmax=100.0), "fmin must be positive, got 0.0"),
    (dict(fmin=65.0, fmax=2093.0, sr=0), "sr must be positive, got 0"),
    (dict(fmin=65.0, fmax=2093.0, hop_length=0), "hop_length must be positive, got 0"),
    (dict(fmin=65.0, fmax=2093.0, hop_length=-3), "hop_length must be positive, got -3"),
    (dict(fmin=65.0, fmax=2093.0, frame_length=2047), "frame_length must be even and in 4 .. 8192, got 2047"),
    (dict(fmin=65.0, fmax=2093.0, frame_length=2), "frame_length must be even and in 4 .. 8192, got 2"),
    (dict(fmin=65.0, fmax=2093.0, frame_length=16384), "frame_length must be even and in 4 .. 8192, got 16384"),
    (dict(fmin=65.0, fmax=2093.0, pad_mode="wrap"), "Unknown pad_mode"),
    # sr / fmax = 31.5 -> lo = 31, but a 64-sample frame only holds lags up to 31
    (dict(fmin=100.0, fmax=700.0, frame_length=64), "no lags between"),
])
def test_validation_errors(fn, kw, match):
    with pytest.raises(ValueError, match=match):
        fn(Y, **kw)


def test_more_validation_errors():
    with pytest.raises(ValueError, match="win_length must be None or frame_length // 2 = 1024, got 512"):
        ap.yin(Y, fmin=65.0, fmax=2093.0, win_length=512)
    with pytest.raises(ValueError, match=r"Signal length \(1000\) must be >= frame_length \(2048\)"):
        ap.yin(np.zeros(1000, np.float32), fmin=65.0, fmax=2093.0, center=False)
    with pytest.raises(ValueError, match=r"Signal length \(10\) must be >= frame_length \(2048\)"):
        ap.yin_cmnd(np.zeros((2, 10), np.float32), fmin=65.0, fmax=2093.0, center=False)
    with pytest.raises(ValueError, match="y must be 1D or 2D, got 3D"):
        ap.yin(np.zeros((2, 2, 4096), np.float32), fmin=65.0, fmax=2093.0)
    with pytest.raises(TypeError):
        ap.yin(Y, 65.0, 2093.0)                        # fmin / fmax are keyword-only, as in librosa
    with pytest.raises(TypeError):
        ap.yin(Y)


def test_no_gpu_is_a_loud_error():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no HIP device"):
        ap.yin(Y, fmin=65.0, fmax=2093.0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        ap.yin_cmnd(Y, fmin=65.0, fmax=2093.0)


def test_fused_predicate():
    lib = ext.lib()
    assert lib.ap_yin_fused(2048, 512, 220500) == 1
    assert lib.ap_yin_fused(2048, 2, 44100) == 1
    assert lib.ap_yin_fused(2048, 511, 220500) == 0          # odd hop: frames start inside a sample pair
    assert lib.ap_yin_fused(2048, 512, (1 << 28) + 2) == 0   # sample offsets past 32 bits
    assert lib.ap_yin_fused(2048, 512, 0) == 0
    assert lib.ap_yin_fused(1024, 256, 220500) == 1
    assert lib.ap_yin_fused(1024, 255, 220500) == 0
    for n in (512, 1536, 400, 4096):
        assert lib.ap_yin_fused(n, n // 4, 220500) == 0


def test_c_entries_validate_before_launching():
    """Status codes and messages for bad geometry; the pointers are never dereferenced on these paths."""
    lib = ext.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def err(rc):
        assert rc in (ext.AP_ERR_INVALID, ext.AP_ERR_UNSUPPORTED)
        return rc, lib.ap_last_error().decode()

    assert err(lib.ap_yin_f32(None, 1, 8192, 2048, 512, 1, 10, 340, 22050.0, 0.1, None, p, None, None))[0] == ext.AP_ERR_INVALID
    assert err(lib.ap_yin_f32(p, 1, 8192, 2048, 512, 1, 10, 340, 22050.0, 0.1, None, None, None, None))[0] == ext.AP_ERR_INVALID
    assert "frame_length must be even" in err(lib.ap_yin_f32(p, 1, 8192, 2050 + 1, 512, 1, 10, 340, 22050.0, 0.1, None, p, None, None))[1]
    assert "hop_length must be positive" in err(lib.ap_yin_f32(p, 1, 8192, 2048, 0, 1, 10, 340, 22050.0, 0.1, None, p, None, None))[1]
    assert "lag range" in err(lib.ap_yin_f32(p, 1, 8192, 2048, 512, 1, 10, 1024, 22050.0, 0.1, None, p, None, None))[1]
    assert "lag range" in err(lib.ap_yin_cmnd_f32(p, 1, 8192, 2048, 512, 1, 0, 340, None, p, None))[1]
    assert "lag range" in err(lib.ap_yin_cmnd_f32(p, 1, 8192, 2048, 512, 1, 340, 340, None, p, None))[1]
    assert "Signal length" in err(lib.ap_yin_cmnd_f32(p, 1, 1000, 2048, 512, 0, 10, 340, None, p, None))[1]
    assert "sr must be positive" in err(lib.ap_yin_f32(p, 1, 8192, 2048, 512, 1, 10, 340, 0.0, 0.1, None, p, None, None))[1]
    # asking for the wave kernel on a shape it does not serve: AP_ERR_UNSUPPORTED, so that the caller falls back
    rc, msg = err(lib.ap_yin_f32(p, 1, 8192, 512, 128, 1, 10, 240, 22050.0, 0.1, p, p, None, None))
    assert rc == ext.AP_ERR_UNSUPPORTED and "wave kernel" in msg
    rc, msg = err(lib.ap_yin_cmnd_f32(p, 1, 8192, 2048, 511, 1, 10, 340, p, p, None))
    assert rc == ext.AP_ERR_UNSUPPORTED and "wave kernel" in msg
