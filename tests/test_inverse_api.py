"""CPU: inverse.py's surface and refusals (no device), the host plan of the NNLS kernel, nnls_ref on a known solution."""

import inspect

import numpy as np
import pytest

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _build, _extension as ext, inverse

import nnls_ref as R

MEL = np.ones((2, 128, 5), np.float32)


def test_surface():
    for n in ("mel_to_stft", "mel_to_audio", "mfcc_to_mel", "mfcc_to_audio"):
        assert n in ap.__all__ and getattr(ap, n) is getattr(inverse, n)
    assert "nnls.hip" in _build.SOURCES
    assert (ext.lib().ap_nnls_max_bins(), ext.lib().ap_nnls_max_rows()) == (inverse.MAX_BINS, inverse.MAX_ROWS) == (1025, 255)
    d = lambda f: {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not p.empty}  # noqa: E731
    assert d(ap.mel_to_stft) == dict(sr=22050, n_fft=2048, power=2.0, n_iter=100, filterbank=None)
    assert d(ap.mel_to_audio) == dict(sr=22050, n_fft=2048, hop_length=None, win_length=None, window="hann", center=True,
                                      pad_mode="constant", power=2.0, n_iter=32, length=None, nnls_iter=100, random_state=None)
    assert d(ap.mfcc_to_mel) == d(ap.mfcc_to_audio) == dict(n_mels=128, dct_type=2, norm="ortho", ref=1.0, lifter=0)


@pytest.mark.parametrize("call", [
    lambda: ap.mfcc_to_mel(MEL[:, :20], lifter=-1),
    lambda: ap.mfcc_to_mel(MEL[:, :20], dct_type=3),
    lambda: ap.mel_to_stft(MEL, power=0.0),
    lambda: ap.mel_to_stft(MEL, n_iter=-1),
    lambda: ap.mel_to_stft(MEL, filterbank=np.ones((127, 1025), np.float32)),
    lambda: ap.mel_to_stft(MEL, filterbank=np.ones((128, 1024), np.float32)),
    lambda: ap.mel_to_stft(MEL, filterbank=-np.ones((128, 1025), np.float32)),
    lambda: ap.mel_to_stft(MEL, n_fft=4096),
    lambda: ap.mel_to_stft(np.ones((256, 5), np.float32)),
], ids=["lifter", "dct_type", "power", "n_iter", "bank-rows", "bank-bins", "bank-negative", "F-over", "M-over"])
def test_refused(call):
    with pytest.raises(ValueError):
        call()


@pytest.mark.parametrize("name", ["mel-256-128", "dense-5-33"])
def test_host_plan_rebuilds_the_bank(name):
    A = R.bank(name)
    (M, F), plan = A.shape, ext.nnls_plan_host(A)
    assert tuple(plan[:2]) == (M, F) and plan[6] == plan.size
    w = plan.view(np.float32)
    by_row, by_bin = np.zeros_like(A), np.zeros_like(A)
    for m, (lo, n, off) in enumerate(plan[plan[2]:plan[2] + 3 * M].reshape(M, 3)):
        by_row[m, lo:lo + n] = w[plan[4] + off:plan[4] + off + n]
    for k, (lo, n, off) in enumerate(plan[plan[3]:plan[3] + 3 * F].reshape(F, 3)):
        by_bin[lo:lo + n, k] = w[plan[5] + off:plan[5] + off + n]
    assert np.array_equal(by_row, A) and np.array_equal(by_bin, A)
    host = inverse._bank_host(A)                                             # what the package hands the kernel
    assert np.array_equal(host[2], R.inputs(A)[0]) and np.float32(host[3]) == np.float32(R.inputs(A)[1])


def test_reference_finds_a_known_solution():
    A = np.array([[1, 1, 0, 0, 0], [0, 1, 1, 1, 0], [0, 0, 0, 1, 1]], np.float32)
    x = np.array([[1.0], [2.0], [1.0], [2.0], [1.0]])          # A^T (1, 1, 1): the minimum-norm solution of A x = s, >= 0
    for n_iter in (0, 50):
        np.testing.assert_allclose(R.fista(A, (A @ x).astype(np.float32), n_iter), x, atol=1e-6)
    np.testing.assert_allclose(inverse._momentum_host(3), [0.0, 0.2817535, 0.43404278], rtol=1e-6)   # (t - 1) / t' from t = 1
