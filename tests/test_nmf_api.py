"""CPU: the public surface of nmf / decompose.decompose and what they refuse before any device is touched."""

import types

import numpy as np
import pytest

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _build

S = np.ones((2, 6, 9), np.float32)
W = np.ones((2, 6, 3), np.float32)
H = np.ones((2, 3, 9), np.float32)


def test_surface():
    assert "nmf" in ap.__all__ and callable(ap.nmf)
    assert isinstance(ap.decompose, types.ModuleType) and "decompose" not in ap.__all__
    assert callable(ap.decompose.decompose) and ap.decompose.nmf is ap.nmf
    assert "nmf.hip" in _build.SOURCES
    assert ap._extension.lib().ap_nmf_max_components() == ap.decompose.MAX_COMPONENTS == 64


@pytest.mark.parametrize("call", [
    lambda: ap.nmf(S, 0),
    lambda: ap.nmf(S, 65),
    lambda: ap.nmf(S, 3, beta_loss="itakura-saito"),
    lambda: ap.nmf(S, 3, init="nndsvd"),
    lambda: ap.nmf(S.astype(np.float64), 3),
    lambda: ap.nmf(S, 3, init="custom", W=W, H=H[:, :, :8]),
    lambda: ap.nmf(S, 3, init="custom", W=W[:, :5], H=H),
    lambda: ap.nmf(S, 3, init="custom", W=W),
    lambda: ap.nmf(S, 3, update_components=False),
    lambda: ap.nmf(S, 3, update_components=False, W=W[0, :, :2]),
    lambda: ap.decompose.decompose(S, 3, transformer=object()),
    lambda: ap.decompose.decompose(S, 3, fit=False),
], ids=["K=0", "K=65", "loss", "init", "dtype", "H-shape", "W-shape", "H-missing", "W-missing", "dictionary-shape", "transformer",
        "fit=False"])
def test_refused(call):
    with pytest.raises(ValueError):
        call()


def test_n_components_none_names_the_limit():
    with pytest.raises(ValueError, match="64"):
        ap.decompose.decompose(np.ones((65, 4), np.float32))
