"""CPU: the host side of dtw / dtw_backtracking (mlx-audio-primitives_amd/dtw.py): the signatures, the exports, every
rejected argument by name, and the band predicate against the definition in tests/dtw_ref.py.  Every check happens
before a device is asked for, so nothing here needs one."""

import importlib
import inspect

import numpy as np
import pytest

import dtw_ref as R

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _build
from mlx_audio_primitives_amd import _extension as _x

MOD = importlib.import_module("mlx_audio_primitives_amd.dtw")

KW = inspect.Parameter.KEYWORD_ONLY
X = np.zeros((3, 5), np.float32)
Y = np.zeros((3, 7), np.float32)
C = np.zeros((5, 7), np.float32)


def test_names_are_exported_and_built():
    for n in ("dtw", "dtw_backtracking"):
        assert n in ap.__all__ and n in MOD.__all__ and callable(getattr(ap, n))
    assert "dtw.hip" in _build.SOURCES
    for s in ("ap_dtw_max_features", "ap_dtw_max_steps", "ap_dtw_max_step", "ap_dtw_max_len", "ap_dtw_cost_f32",
              "ap_dtw_accumulate_f32", "ap_dtw_backtrack_i32"):
        assert s in _x.ABI_SYMBOLS and getattr(_x.lib(), s) is not None
    L = _x.lib()
    assert L.ap_dtw_max_features() >= 128 and L.ap_dtw_max_steps() >= 8 and L.ap_dtw_max_step() >= 2 and L.ap_dtw_max_len() >= 7750


def test_signatures_are_librosas():
    sig = inspect.signature(ap.dtw)
    assert list(sig.parameters) == ["X", "Y", "C", "metric", "step_sizes_sigma", "weights_add", "weights_mul", "subseq", "backtrack",
                                    "global_constraints", "band_rad", "return_steps"]
    assert all(sig.parameters[k].kind is KW for k in list(sig.parameters)[2:])
    assert all(sig.parameters[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for k in ("X", "Y"))
    assert [p.default for p in sig.parameters.values()] == [None, None, None, "euclidean", None, None, None, False, True, False, 0.25,
                                                            False]
    sig = inspect.signature(ap.dtw_backtracking)
    assert list(sig.parameters) == ["steps", "step_sizes_sigma", "subseq", "start"]
    assert all(sig.parameters[k].kind is KW for k in list(sig.parameters)[1:])
    assert [sig.parameters[k].default for k in list(sig.parameters)[1:]] == [None, False, None]
    assert "librosa" in ap.dtw.__doc__ and "254" in ap.dtw.__doc__ and "librosa" in ap.dtw_backtracking.__doc__


@pytest.mark.parametrize("kw, name", [
    (dict(), "exactly one"), (dict(X=X), "exactly one"), (dict(Y=Y), "exactly one"),
    (dict(X=X, Y=Y, C=C), "exactly one"), (dict(X=X, C=C), "exactly one"),
    (dict(X=X, Y=np.zeros((4, 7), np.float32)), "features d"),
    (dict(X=np.zeros((2, 3, 5), np.float32), Y=np.zeros((3, 3, 7), np.float32)), "pairs B"),
    (dict(X=X, Y=np.zeros((1, 3, 7), np.float32)), "both be 2D or both be 3D"),
    (dict(X=X, Y=Y, metric="chebyshev"), "metric"), (dict(C=C, metric="l2"), "metric"), (dict(X=X, Y=Y, metric=None), "metric"),
    (dict(C=C, step_sizes_sigma=[[1, 1], [-1, 1]]), "step_sizes_sigma"),
    (dict(C=C, step_sizes_sigma=[[1, 1], [0, 0]]), "step_sizes_sigma"),
    (dict(C=C, step_sizes_sigma=[[1, 1], [0, 99]]), "step_sizes_sigma"),
    (dict(C=C, step_sizes_sigma=[[1, 1]] * 9), "step_sizes_sigma"),
    (dict(C=C, step_sizes_sigma=[1, 1]), "step_sizes_sigma"), (dict(C=C, step_sizes_sigma=[[1.0, 1.0]]), "step_sizes_sigma"),
    (dict(C=C, step_sizes_sigma=[]), "step_sizes_sigma"),
    (dict(C=C, weights_add=[0.0, 0.0]), "weights_add"), (dict(C=C, weights_mul=[1.0] * 4), "weights_mul"),
    (dict(C=C, step_sizes_sigma=[[1, 1], [1, 2]], weights_mul=[1.0] * 3), "weights_mul"),
    (dict(C=C, weights_add=[[0.0, 0.0, 0.0]]), "weights_add"),
    (dict(C=C, band_rad=0.0), "band_rad"), (dict(C=C, band_rad=1.5), "band_rad"), (dict(C=C, band_rad=-0.25), "band_rad"),
    (dict(C=C, band_rad=float("nan")), "band_rad"), (dict(C=C, band_rad=None, global_constraints=True), "band_rad"),
    (dict(C=np.zeros((0, 7), np.float32)), "C"), (dict(C=np.zeros((5, 0), np.float32)), "C"), (dict(C=np.zeros((0, 5, 7), np.float32)), "C"),
    (dict(C=np.zeros(5, np.float32)), "C"), (dict(C=np.zeros((5, 7), np.complex64)), "C"),
    (dict(X=np.zeros((3, 0), np.float32), Y=Y), "X"), (dict(X=X, Y=np.zeros((3, 0), np.float32)), "Y"),
    (dict(X=np.zeros((0, 5), np.float32), Y=np.zeros((0, 7), np.float32)), "X"),
    (dict(X=np.zeros(5, np.float32), Y=Y), "X"), (dict(X=X, Y=np.zeros((3, 7), np.complex64)), "Y"),
], ids=lambda v: v if isinstance(v, str) else "-".join(v) or "nothing")
def test_dtw_rejects_by_name(kw, name):
    with pytest.raises(ValueError, match=name):
        ap.dtw(**kw)


def test_dtw_names_the_argument_above_a_cap():
    L = _x.lib()
    d_cap, len_cap = L.ap_dtw_max_features(), L.ap_dtw_max_len()
    with pytest.raises(ValueError, match="d="):
        ap.dtw(np.zeros((d_cap + 1, 2), np.float32), np.zeros((d_cap + 1, 2), np.float32))
    with pytest.raises(ValueError, match="N="):
        ap.dtw(np.zeros((1, len_cap + 1), np.float32), np.zeros((1, 2), np.float32))
    with pytest.raises(ValueError, match="M="):
        ap.dtw(np.zeros((1, 2), np.float32), np.zeros((1, len_cap + 1), np.float32))
    with pytest.raises(ValueError, match="step_sizes_sigma"):
        ap.dtw(C=C, step_sizes_sigma=[[1, 1], [L.ap_dtw_max_step() + 1, 1]])


@pytest.mark.parametrize("kw, name", [
    (dict(steps=np.zeros((5, 7), np.int32)), "steps"), (dict(steps=np.zeros((5, 7), np.float32)), "steps"),
    (dict(steps=np.zeros(5, np.uint8)), "steps"), (dict(steps=np.zeros((0, 7), np.uint8)), "steps"),
    (dict(steps=np.zeros((5, 7), np.uint8), step_sizes_sigma=[[0, 0]]), "step_sizes_sigma"),
    (dict(steps=np.zeros((5, 7), np.uint8), start=7), "start"), (dict(steps=np.zeros((5, 7), np.uint8), start=-1), "start"),
    (dict(steps=np.zeros((5, 7), np.uint8), start=1.5), "start"), (dict(steps=np.zeros((2, 5, 7), np.uint8), start=[1, 2, 3]), "start"),
], ids=lambda v: v if isinstance(v, str) else "-".join(k for k in v))
def test_dtw_backtracking_rejects_by_name(kw, name):
    with pytest.raises(ValueError, match=name):
        ap.dtw_backtracking(**kw)


@pytest.mark.parametrize("N, M", [(5, 9), (9, 9), (9, 5), (1, 7), (7, 1), (40, 41), (64, 37)])
def test_band_predicate_is_the_definitions(N, M):
    i, j = np.meshgrid(np.arange(N), np.arange(M), indexing="ij")
    for band_rad in (0.1, 0.25, 0.5, 0.75, 1.0):
        r = MOD._band_radius(band_rad, N, M)
        assert r == R.band_radius(band_rad, N, M) == int(np.rint(band_rad * min(N, M)))
        got = MOD._in_band(i, j, N, M, r)
        want = np.zeros((N, M), bool)
        for a in range(N):
            for b in range(M):
                want[a, b] = -r - max(N - M, 0) < b - a < r + max(M - N, 0)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(R.in_band(i, j, N, M, r), want)
        if r >= 1:
            assert want[0, 0] and want[N - 1, M - 1], "both ends of the path lie inside the band"
    assert MOD._band_radius(0.25, 10, 30) == 2 and MOD._band_radius(0.25, 6, 6) == 2 and MOD._band_radius(0.25, 14, 14) == 4   # 2.5, 1.5, 3.5: to even
