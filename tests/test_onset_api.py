"""CPU: onset_strength / peak_pick / onset_detect are exported with librosa's signatures, validate their arguments
before any device work and fail loudly without a GPU.  The C entry points reject bad geometry with a status, not a
launch."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _build, onset
from mlx_audio_primitives_amd import _extension as ext

NAMES = ("onset_strength", "peak_pick", "onset_detect")
SYMBOLS = ("ap_onset_strength_f32", "ap_peak_pick_max_frames", "ap_peak_pick_f32")
KW = inspect.Parameter.KEYWORD_ONLY


def test_exported():
    for name in NAMES:
        assert name in ap.__all__ and callable(getattr(ap, name)) and getattr(ap, name) is getattr(onset, name)
    assert "onset.hip" in _build.SOURCES
    header = open(os.path.join(ROOT, "include", "audioprims.h")).read()
    declared = set(re.findall(r"\b(ap_[a-z0-9_]+)\s*\(", header))
    for sym in SYMBOLS:
        assert sym in declared and sym in ext.ABI_SYMBOLS and getattr(ext.lib(), sym) is not None
    assert ext.lib().ap_peak_pick_max_frames() >= 16384


def test_signatures_follow_librosa():
    p = inspect.signature(ap.onset_strength).parameters
    assert list(p) == ["y", "sr", "S", "lag", "max_size", "ref", "detrend", "center", "feature", "aggregate", "kwargs"]
    assert all(v.kind is KW for k, v in p.items() if k != "kwargs") and p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert {k: v.default for k, v in p.items() if k != "kwargs"} == {
        "y": None, "sr": 22050, "S": None, "lag": 1, "max_size": 1, "ref": None, "detrend": False, "center": True,
        "feature": None, "aggregate": None}
    q = inspect.signature(ap.peak_pick).parameters
    assert list(q) == ["x", "pre_max", "post_max", "pre_avg", "post_avg", "delta", "wait", "sparse"]
    assert q["x"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and all(v.kind is KW for k, v in q.items() if k != "x")
    assert all(q[k].default is inspect.Parameter.empty for k in list(q)[:-1]) and q["sparse"].default is True
    r = inspect.signature(ap.onset_detect).parameters
    assert list(r) == ["y", "sr", "onset_envelope", "hop_length", "backtrack", "energy", "units", "normalize", "sparse", "kwargs"]
    assert all(v.kind is KW for k, v in r.items() if k != "kwargs") and r["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert {k: v.default for k, v in r.items() if k != "kwargs"} == {
        "y": None, "sr": 22050, "onset_envelope": None, "hop_length": 512, "backtrack": False, "energy": None,
        "units": "frames", "normalize": True, "sparse": True}
    with pytest.raises(TypeError):
        ap.onset_strength(np.zeros(4096, np.float32))          # keyword-only, as in librosa
    with pytest.raises(TypeError):
        ap.peak_pick(np.zeros(8, np.float32), 1, 1, 1, 1, 0.0, 0)


S = np.zeros((2, 9, 12), np.float32)
ENV = np.zeros(40, np.float32)
PP = dict(pre_max=1, post_max=1, pre_avg=4, post_avg=5, delta=0.07, wait=1)


@pytest.mark.parametrize("kw,exc,match", [
    (dict(), ValueError, "needs y or S"),
    (dict(S=S, lag=0), ValueError, "lag must be a positive integer"),
    (dict(S=S, lag=-2), ValueError, "lag must be a positive integer"),
    (dict(S=S, lag=1.0), ValueError, "lag must be a positive integer"),
    (dict(S=S, lag=True), ValueError, "lag must be a positive integer"),
    (dict(S=S, max_size=0), ValueError, r"max_size must be an integer in 1 \.\. 255"),
    (dict(S=S, max_size=256), ValueError, r"max_size must be an integer in 1 \.\. 255"),
    (dict(S=S, max_size=3.0), ValueError, r"max_size must be an integer in 1 \.\. 255"),
    (dict(S=S, detrend=True), NotImplementedError, "detrend"),
    (dict(S=S, feature=ap.melspectrogram), NotImplementedError, "feature"),
    (dict(S=S, aggregate=np.median), NotImplementedError, "aggregate"),
    (dict(S=S, aggregate=np.max), NotImplementedError, "aggregate"),
    (dict(S=np.zeros(8, np.float32)), ValueError, "S must be 2D or 3D, got 1D"),
    (dict(S=np.zeros((2, 2), np.complex64)), ValueError, "S must be real"),
    (dict(S=S, ref=np.zeros(8, np.float32)), ValueError, "ref must be 2D or 3D, got 1D"),
    (dict(S=S, hop_length=0), ValueError, "n_fft and hop_length must be positive integers"),
])
def test_onset_strength_errors(kw, exc, match):
    """Raised before any device work: these hold with and without a GPU."""
    with pytest.raises(exc, match=match):
        ap.onset_strength(**kw)
    if "S" in kw and kw["S"] is S:
        kw = dict(kw, y=np.zeros(8192, np.float32))
        del kw["S"]
        with pytest.raises(exc, match=match):
            ap.onset_strength(**kw)


@pytest.mark.parametrize("kw,match", [
    (dict(pre_max=-1), "pre_max must be a non-negative integer"),
    (dict(pre_max=1.0), "pre_max must be a non-negative integer"),
    (dict(pre_avg=-1), "pre_avg must be a non-negative integer"),
    (dict(pre_avg=True), "pre_avg must be a non-negative integer"),
    (dict(wait=-1), "wait must be a non-negative integer"),
    (dict(wait=0.5), "wait must be a non-negative integer"),
    (dict(post_max=0), "post_max must be a positive integer"),
    (dict(post_max=2.0), "post_max must be a positive integer"),
    (dict(post_avg=0), "post_avg must be a positive integer"),
    (dict(post_avg=-3), "post_avg must be a positive integer"),
    (dict(delta=-0.1), "delta must be a non-negative number"),
    (dict(delta=float("nan")), "delta must be a non-negative number"),
])
def test_peak_pick_errors(kw, match):
    with pytest.raises(ValueError, match=match):
        ap.peak_pick(ENV, **dict(PP, **kw))
    with pytest.raises(ValueError, match=match):
        ap.peak_pick(ENV, sparse=False, **dict(PP, **kw))


def test_more_peak_pick_and_onset_detect_errors():
    with pytest.raises(ValueError, match="sparse=True needs 1D input"):
        ap.peak_pick(np.zeros((2, 40), np.float32), **PP)
    with pytest.raises(ValueError, match="x must be 1D or 2D, got 3D"):
        ap.peak_pick(np.zeros((1, 2, 40), np.float32), sparse=False, **PP)
    with pytest.raises(ValueError, match="needs y or onset_envelope"):
        ap.onset_detect()
    with pytest.raises(ValueError, match="units must be one of"):
        ap.onset_detect(onset_envelope=ENV, units="seconds")
    for units in ("samples", "time"):
        with pytest.raises(ValueError, match="needs sparse=True"):
            ap.onset_detect(onset_envelope=ENV, units=units, sparse=False)
    with pytest.raises(ValueError, match="sparse=True needs 1D input"):
        ap.onset_detect(onset_envelope=np.zeros((2, 40), np.float32))
    with pytest.raises(ValueError, match="sparse=True needs 1D input"):
        ap.onset_detect(y=np.zeros((2, 8192), np.float32))
    with pytest.raises(ValueError, match="onset_envelope must be 1D or 2D, got 3D"):
        ap.onset_detect(onset_envelope=np.zeros((1, 2, 40), np.float32), sparse=False)
    with pytest.raises(ValueError, match="post_max must be a positive integer"):
        ap.onset_detect(onset_envelope=ENV, post_max=0)
    with pytest.raises(ValueError, match="wait must be a non-negative integer"):
        ap.onset_detect(onset_envelope=ENV, wait=-1)
    with pytest.raises(ValueError, match="hop_length must be a positive integer"):
        ap.onset_detect(onset_envelope=ENV, hop_length=0)
    with pytest.raises(TypeError, match="unexpected keyword"):
        ap.onset_detect(onset_envelope=ENV, post_maximum=3)


def test_default_windows_and_shift_arithmetic():
    """librosa's defaults at sr = 22050, hop_length = 512: pre_max, post_max, pre_avg, post_avg, wait = 1, 1, 4, 5, 1."""
    assert onset._detect_parameters(22050, 512, {}) == ((1, 1, 4, 5), 0.07, 1)
    assert onset._detect_parameters(44100, 512, {}) == ((2, 1, 8, 9), 0.07, 2)
    assert onset._detect_parameters(22050, 256, {}) == ((2, 1, 8, 9), 0.07, 2)
    assert onset._detect_parameters(22050, 512, dict(wait=7, delta=0.5, pre_max=2.5)) == ((3, 1, 4, 5), 0.5, 7)
    # the flux of frames u and u + lag belongs to frame u + lag of a centred STFT plus n_fft // (2 hop) frames
    assert onset._shift(1, True, 2048, 512) == 3 and onset._shift(1, False, 2048, 512) == 1
    assert onset._shift(2, True, 512, 128) == 4 and onset._shift(5, True, 2048, 1024) == 6
    assert onset._shift(1, True, 400, 512) == 1


def test_no_gpu_is_a_loud_error():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    y = np.zeros(8192, np.float32)
    for call in (lambda: ap.onset_strength(S=S), lambda: ap.onset_strength(y=y), lambda: ap.peak_pick(ENV, **PP),
                 lambda: ap.onset_detect(onset_envelope=ENV), lambda: ap.onset_detect(y=y)):
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()


def test_c_entries_validate_before_launching():
    """Status codes and messages for bad arguments; the pointers are never dereferenced on these paths."""
    lib = ext.lib()
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    s, o = base, base + 8192

    def strength(*a):
        rc = lib.ap_onset_strength_f32(*a)
        assert rc in (ext.AP_ERR_INVALID, ext.AP_ERR_UNSUPPORTED), rc
        return rc, lib.ap_last_error().decode()

    #                S  B  M  T rs  ref rsr lag ms shift db coef  amin  ref  top   key  out rso stream
    assert strength(None, 1, 4, 8, 8, None, 0, 1, 1, 1, 0, 10.0, 1e-10, 1.0, -1.0, None, o, 8, None)[0] == ext.AP_ERR_INVALID
    assert "non-empty" in strength(s, 1, 4, 0, 8, None, 0, 1, 1, 1, 0, 10.0, 1e-10, 1.0, -1.0, None, o, 8, None)[1]
    assert "lag must be a positive integer" in strength(s, 1, 4, 8, 8, None, 0, 0, 1, 1, 0, 10.0, 1e-10, 1.0, -1.0, None, o, 8, None)[1]
    assert "max_size must be an integer in 1 .. 255" in strength(s, 1, 4, 8, 8, None, 0, 1, 256, 1, 0, 10.0, 1e-10, 1.0, -1.0, None, o, 8, None)[1]
    assert "must be >= lag" in strength(s, 1, 4, 8, 8, None, 0, 3, 1, 2, 0, 10.0, 1e-10, 1.0, -1.0, None, o, 8, None)[1]
    assert "row strides" in strength(s, 1, 4, 8, 7, None, 0, 1, 1, 1, 0, 10.0, 1e-10, 1.0, -1.0, None, o, 8, None)[1]
    assert "top_db needs the key" in strength(s, 1, 4, 8, 8, None, 0, 1, 1, 1, 1, 10.0, 1e-10, 1.0, 80.0, None, o, 8, None)[1]
    assert "overlaps" in strength(s, 1, 4, 8, 8, None, 0, 1, 1, 1, 0, 10.0, 1e-10, 1.0, -1.0, None, s + 16, 8, None)[1]
    rc, msg = strength(s, 1, 4, (1 << 28) + 1, (1 << 28) + 1, None, 0, 1, 1, 1, 0, 10.0, 1e-10, 1.0, -1.0, None, base + (1 << 50), (1 << 28) + 1, None)
    assert rc == ext.AP_ERR_UNSUPPORTED and "2^28" in msg

    def pick(*a):
        rc = lib.ap_peak_pick_f32(*a)
        assert rc in (ext.AP_ERR_INVALID, ext.AP_ERR_UNSUPPORTED), rc
        return rc, lib.ap_last_error().decode()

    #            x  B  T rs  pre post pre post delta wait norm guard bt energy rse mask count stream
    assert pick(None, 1, 8, 8, 1, 1, 1, 1, 0.0, 0, 0, 0, 0, None, 0, o, None, None)[0] == ext.AP_ERR_INVALID
    assert "non-empty" in pick(s, 1, 0, 8, 1, 1, 1, 1, 0.0, 0, 0, 0, 0, None, 0, o, None, None)[1]
    assert "non-negative" in pick(s, 1, 8, 8, -1, 1, 1, 1, 0.0, 0, 0, 0, 0, None, 0, o, None, None)[1]
    assert "positive" in pick(s, 1, 8, 8, 1, 1, 1, 0, 0.0, 0, 0, 0, 0, None, 0, o, None, None)[1]
    assert "wait must be" in pick(s, 1, 8, 8, 1, 1, 1, 1, 0.0, -1, 0, 0, 0, None, 0, o, None, None)[1]
    assert "row strides" in pick(s, 1, 8, 7, 1, 1, 1, 1, 0.0, 0, 0, 0, 0, None, 0, o, None, None)[1]
    limit = lib.ap_peak_pick_max_frames()
    rc, msg = pick(s, 1, limit + 1, limit + 1, 1, 1, 1, 1, 0.0, 0, 0, 0, 0, None, 0, base + (1 << 40), None, None)
    assert rc == ext.AP_ERR_UNSUPPORTED and str(limit) in msg
