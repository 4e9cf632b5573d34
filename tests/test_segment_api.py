"""CPU: the host side of recurrence_matrix / cross_similarity / recurrence_to_lag / lag_to_recurrence
(mlx-audio-primitives_amd/segment.py): the signatures, the exports, every rejected argument by its message, the default k
and the limits of width; and the model of tests/segment_ref.py against sklearn's brute-force neighbours.  Every check
happens before a device is asked for, so nothing here needs one: an argument set that passes validation ends in the
"no HIP device" error."""

import importlib
import inspect

import numpy as np
import pytest
import torch

import dtw_ref
import segment_ref as R

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _build
from mlx_audio_primitives_amd import _extension as _x

MOD = importlib.import_module("mlx_audio_primitives_amd.segment")

KW = inspect.Parameter.KEYWORD_ONLY
Y = np.zeros((3, 9), np.float32)
X = np.zeros((3, 7), np.float32)
NAMES = ("recurrence_matrix", "cross_similarity", "recurrence_to_lag", "lag_to_recurrence")
SYMBOLS = ("ap_segment_max_len", "ap_segment_threshold_f32", "ap_segment_bandwidth_f32", "ap_segment_write_f32", "ap_segment_lag")

needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="with a device the call goes through")


def test_names_are_exported_and_built():
    for n in NAMES:
        assert n in ap.__all__ and n in MOD.__all__ and callable(getattr(ap, n))
    assert "segment.hip" in _build.SOURCES
    for s in SYMBOLS:
        assert s in _x.ABI_SYMBOLS and getattr(_x.lib(), s) is not None
    assert _x.lib().ap_segment_max_len() >= 16384, "a five-minute clip at the default hop is 12 920 frames"


def test_signatures_are_librosas():
    sig = inspect.signature(ap.recurrence_matrix)
    assert list(sig.parameters) == ["data", "k", "width", "metric", "sym", "sparse", "mode", "bandwidth", "self", "axis", "full"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [None, 1, "euclidean", False, False, "connectivity", None, False, -1, False]
    assert all(sig.parameters[k].kind is KW for k in list(sig.parameters)[1:])
    sig = inspect.signature(ap.cross_similarity)
    assert list(sig.parameters) == ["data", "data_ref", "k", "metric", "sparse", "mode", "bandwidth", "full"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, "euclidean", False, "connectivity", None, False]
    assert all(sig.parameters[k].kind is KW for k in list(sig.parameters)[2:])
    sig = inspect.signature(ap.recurrence_to_lag)
    assert list(sig.parameters) == ["rec", "pad", "axis"] and [sig.parameters[k].default for k in ("pad", "axis")] == [True, -1]
    assert all(sig.parameters[k].kind is KW for k in ("pad", "axis"))
    sig = inspect.signature(ap.lag_to_recurrence)
    assert list(sig.parameters) == ["lag", "axis"] and sig.parameters["axis"].default == -1 and sig.parameters["axis"].kind is KW
    for n in NAMES:
        assert "librosa" in getattr(ap, n).__doc__
    assert "synchronis" in ap.recurrence_matrix.__doc__ and "synchronis" in ap.cross_similarity.__doc__


COMMON = [
    (dict(sparse=True), "sparse=True is not implemented"),
    (dict(metric="chebyshev"), "Unknown metric"), (dict(metric=None), "Unknown metric"),
    (dict(mode="affinities"), "Unknown mode"), (dict(mode=None), "Unknown mode"),
    (dict(bandwidth="mean_k_avg"), "not implemented"), (dict(bandwidth="gmean_k_avg"), "not implemented"),
    (dict(bandwidth="mean_k_avg_and_pair"), "not implemented"), (dict(bandwidth=np.ones((9, 9))), "not implemented"),
    (dict(bandwidth=torch.ones(9, 9)), "not implemented"), (dict(bandwidth="median"), "Unknown bandwidth"),
    (dict(bandwidth=0.0), "positive finite"), (dict(bandwidth=-1.0), "positive finite"), (dict(bandwidth=float("inf")), "positive finite"),
    (dict(bandwidth=float("nan")), "positive finite"),
    (dict(k=0), "k must be a positive integer"), (dict(k=-3), "k must be a positive integer"), (dict(k=2.5), "k must be a positive integer"),
    (dict(k=True), "k must be a positive integer"), (dict(k="3"), "k must be a positive integer"),
]


@pytest.mark.parametrize("kw, msg", COMMON + [
    (dict(axis=0), "axis=0 is not implemented"), (dict(axis=1), "is not implemented"),
    (dict(width=0), "width"), (dict(width=5), "width"), (dict(width=-1), "width"), (dict(width=1.0), "width must be an integer"),
    (dict(data=np.zeros((3, 2), np.float32)), "width"),
    (dict(data=np.zeros((3, 9), np.complex64)), "must be real"), (dict(data=np.zeros((3, 9), bool)), "must be real"),
    (dict(data=np.zeros((3, 0), np.float32)), "must not be empty"), (dict(data=np.zeros((0, 9), np.float32)), "must not be empty"),
    (dict(data=np.zeros(9, np.float32)), "2D"), (dict(data=np.zeros((1, 1, 3, 9), np.float32)), "2D"),
    (dict(data=np.zeros((1025, 9), np.float32)), "features are above"),
    (dict(data=torch.zeros(1, 16385)), "frames are above"),
])
def test_recurrence_matrix_rejects_before_any_device_call(kw, msg):
    kw = dict(kw)
    data = kw.pop("data", Y)
    with pytest.raises(ValueError, match=msg):
        ap.recurrence_matrix(data, **kw)


@pytest.mark.parametrize("kw, msg", COMMON + [
    (dict(data_ref=np.zeros((4, 7), np.float32)), "same number of features"),
    (dict(data=np.zeros((2, 3, 9), np.float32), data_ref=np.zeros((3, 3, 7), np.float32)), "same number of pairs"),
    (dict(data_ref=np.zeros((1, 3, 7), np.float32)), "both be 2D or both be 3D"),
    (dict(data_ref=np.zeros((3, 7), np.complex128)), "must be real"), (dict(data_ref=np.zeros((3, 0), np.float32)), "must not be empty"),
    (dict(data=np.zeros((3, 0), np.float32)), "must not be empty"), (dict(data_ref=np.zeros(7, np.float32)), "2D"),
    (dict(data=np.zeros((1025, 9), np.float32), data_ref=np.zeros((1025, 7), np.float32)), "features are above"),
    (dict(data_ref=torch.zeros(3, 16385)), "n_ref=16385 frames are above"), (dict(data=torch.zeros(3, 16385)), "n=16385 frames are above"),
])
def test_cross_similarity_rejects_before_any_device_call(kw, msg):
    kw = dict(kw)
    data, ref = kw.pop("data", Y), kw.pop("data_ref", X)
    with pytest.raises(ValueError, match=msg):
        ap.cross_similarity(data, ref, **kw)
    with pytest.raises(TypeError):
        ap.cross_similarity(data, ref, 3)                       # k is keyword-only
    assert "axis" not in inspect.signature(ap.cross_similarity).parameters


@pytest.mark.parametrize("fn, arg, kw, msg", [
    ("recurrence_to_lag", np.zeros((4, 4), np.float32), dict(axis=0), "not implemented"),
    ("lag_to_recurrence", np.zeros((4, 4), np.float32), dict(axis=0), "not implemented"),
    ("recurrence_to_lag", np.zeros((4, 5), np.float32), {}, "must be square"), ("recurrence_to_lag", np.zeros((8, 4), np.float32), {}, "must be square"),
    ("lag_to_recurrence", np.zeros((6, 4), np.float32), {}, "square or hold twice"),
    ("recurrence_to_lag", np.zeros((4, 4), np.float64), {}, "bool or float32"), ("lag_to_recurrence", np.zeros((4, 4), np.int32), {}, "bool or float32"),
    ("recurrence_to_lag", np.zeros(4, np.float32), {}, "2D or 3D"), ("lag_to_recurrence", np.zeros((0, 0), np.float32), {}, "must not be empty"),
])
def test_lag_conversions_reject_before_any_device_call(fn, arg, kw, msg):
    with pytest.raises(ValueError, match=msg):
        getattr(ap, fn)(arg, **kw)


@needs_no_gpu
def test_valid_arguments_reach_the_device():
    """What validation lets through asks for the device, and without one that is the loud error."""
    for call in (lambda: ap.recurrence_matrix(Y), lambda: ap.recurrence_matrix(Y, width=4, k=100, sym=True, self=True, full=True),
                 lambda: ap.recurrence_matrix(np.zeros((3, 1), np.float32), width=1), lambda: ap.recurrence_matrix(Y[None], mode="affinity", bandwidth=2),
                 lambda: ap.recurrence_matrix(Y, mode="affinity", bandwidth="gmean_k"), lambda: ap.cross_similarity(Y, X, k=np.int64(3)),
                 lambda: ap.cross_similarity(Y.astype(np.float64), X.tolist(), mode="distance", bandwidth="mean_k"),
                 lambda: ap.recurrence_to_lag(np.zeros((4, 4), bool), pad=False), lambda: ap.lag_to_recurrence(np.zeros((2, 8, 4), np.float32))):
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()


def test_default_k_and_the_limits_of_width():
    for t, want in ((0, 0), (1, 2), (2, 4), (4, 4), (5, 6), (9, 6), (10, 8), (12919, 228), (12920, 228), (16384, 256)):
        assert MOD._default_k(t) == want == R.default_k(t), t
        assert t == 0 or want == 2 * int(np.ceil(np.sqrt(t)))
    assert R.default_k_recurrence(9, 1) == 6 and R.default_k_recurrence(9, 4) == 4 and R.default_k_cross(7) == 6
    for n in (1, 2, 3, 4, 9, 10):
        top = (n - 1) // 2
        for width in range(0, top + 3):
            ok = 1 <= width <= top or (n == 1 and width == 1)
            try:
                ap.recurrence_matrix(np.zeros((2, n), np.float32), width=width)
                reached = True
            except ValueError as e:
                assert "width" in str(e)
                reached = False
            except RuntimeError as e:                           # no device: validation let it through
                assert "no HIP device" in str(e)
                reached = True
            assert reached == ok, (n, width)


@pytest.mark.parametrize("metric", dtw_ref.METRICS)
def test_the_model_selects_what_sklearn_selects(metric):
    """Tie-free random data: the neighbours of the model over float32 distances are those of
    sklearn.neighbors.NearestNeighbors(algorithm="brute"), the selection librosa builds on."""
    pytest.importorskip("sklearn")
    ref, data = dtw_ref.features(1, 6, 45, 70)[0], dtw_ref.features(1, 6, 60, 71)[0]
    D = dtw_ref.cost(ref[None], data[None], metric)[0][0].astype(np.float32)
    for k in (1, 7, 45):
        assert np.array_equal(R.neighbours(D, k)[0], R.sklearn_neighbours(ref, data, k, metric))
    D = dtw_ref.cost(data[None], data[None], metric)[0][0].astype(np.float32)
    for k, width in ((1, 1), (R.default_k_recurrence(60, 3), 3), (5, 29)):
        mask, tau, t = R.neighbours(D, k, width)
        assert np.array_equal(mask, R.sklearn_neighbours(data, data, k, metric, width))
        assert (mask.sum(axis=0) == min(k, 60 - 2 * width + 1)).all() or width == 29
        assert np.array_equal(mask, R.eligible(D, width) & ((D < tau) | ((D == tau) & (np.arange(60)[:, None] <= t))))
