"""GPU: the fused NNLS kernel against tests/nnls_ref.py (bound: 4 x the float32 NumPy route's error), and inverse.py."""

import numpy as np
import pytest
import scipy.fft
import torch

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import inverse

import nnls_ref as R

pytestmark = pytest.mark.gpu
TILE = inverse.FRAME_TILE


def padded(a, pad=3):            # (NaN-filled device buffer, `pad` columns wider than a; its view of a's shape, = a if float32)
    buf = torch.full(a.shape[:-1] + (a.shape[-1] + pad,), float("nan"), device="cuda")
    view = buf[..., :a.shape[-1]]
    if a.dtype == np.float32:
        view.copy_(torch.tensor(a))
    return buf, view


@pytest.mark.parametrize("n_iter", R.N_ITERS)
@pytest.mark.parametrize("name", R.BANKS)
def test_kernel_against_float64(name, n_iter):
    A, s = R.bank(name), R.case(name, 3, TILE + 1)
    (_, sv), (obuf, ov) = padded(s), padded(np.empty((3, A.shape[1], TILE + 1)))
    out = inverse.nnls_fista(sv, A, n_iter=n_iter, out=ov)
    assert out.data_ptr() == ov.data_ptr() and bool(torch.isnan(obuf[..., TILE + 1:]).all())       # the pad is untouched
    got = ov.cpu().numpy()
    dense = inverse.nnls_fista(s, A, n_iter=n_iter)
    assert dense.shape == (3, A.shape[1], TILE + 1) and dense.dtype == torch.float32 and dense.is_cuda
    assert np.array_equal(dense.cpu().numpy(), got)                                                # a second run, dense rows
    assert np.array_equal(inverse.nnls_fista(s[1], A, n_iter=n_iter).cpu().numpy(), got[1])       # alone and in a batch
    assert np.isfinite(got).all() and (got >= 0).all() and not got[:, :, -1].any()                 # the all-zero frame
    ref, x0 = R.fista(A, s, n_iter), R.fista(A, s, 0)
    err, bound = R.err(got, ref), 4 * R.F32_ERR[name, n_iter]
    print(f"{name} n_iter={n_iter}: {err:.2e} of {bound:.2e}")
    assert err <= bound
    uncovered = ~A.any(0)                                                                           # no gradient: x0
    assert (np.abs(got[:, uncovered] - x0[:, uncovered]) <= 4 * R.F32_ERR[name, 0] * np.abs(x0).max(-2, keepdims=True)).all()
    if n_iter == 100 and name in R.BANKS[:2]:                               # the residual: the reference's own, below the start's
        res = [np.linalg.norm(A.astype(np.float64) @ x - s) / np.linalg.norm(s)
               for x in (got.astype(np.float64), ref, inverse.nnls_fista(s, A, n_iter=0).cpu().numpy().astype(np.float64))]
        print(f"residual {res[0]:.3e}, float64 {res[1]:.3e}, n_iter=0 {res[2]:.3e}")
        assert res[0] <= 1.05 * res[1] + 1e-6 and res[0] < res[2]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, TILE, TILE + 1])
def test_frame_counts_and_power(B, T):
    name, n_iter = "htk-400-80", 32
    A, s = R.bank(name), R.case(name, B, T)
    got = inverse.nnls_fista(s, A, n_iter=n_iter).cpu().numpy()
    assert got.shape == (B, A.shape[1], T) and R.err(got, R.fista(A, s, n_iter)) <= 4 * R.F32_ERR[name, n_iter]
    assert np.array_equal(inverse.nnls_fista(s, A, n_iter=n_iter, power=2.0).cpu().numpy(), np.sqrt(got))
    # powf(x, 1.0f / 1.5f): the device library's 1 ulp and the half ulp of rounding the reference, 2^-23 each at most
    np.testing.assert_allclose(inverse.nnls_fista(s, A, n_iter=n_iter, power=1.5).cpu().numpy(),
                               got.astype(np.float64) ** float(np.float32(1) / np.float32(1.5)), rtol=2 ** -22, atol=0)


def test_public_functions():
    sr, n_fft, t = 22050, 2048, np.arange(16384) / 22050
    y = (np.sin(2 * np.pi * 440 * t) + 0.5 * np.sin(2 * np.pi * 880 * t)).astype(np.float32)
    mel = ap.melspectrogram(np.stack([y, y[::-1]]), sr=sr, n_fft=n_fft)
    S = ap.mel_to_stft(mel, sr=sr, n_fft=n_fft)
    assert S.shape == (2, 1025, mel.shape[-1]) and ap.mel_to_stft(mel[0], sr=sr, n_fft=n_fft).shape == S.shape[1:]
    mag = ap.magnitude(ap.stft(y, n_fft=n_fft)).cpu().numpy()[:, 8]
    est = S[0, :, 8].cpu().numpy()
    for band in (slice(0, 61), slice(61, 1025)):                            # one tone each: bins 41 and 82
        assert abs(int(est[band].argmax()) - int(mag[band].argmax())) <= 1
    audio = ap.mel_to_audio(mel, sr=sr, n_fft=n_fft, n_iter=4, length=16000, random_state=3)
    assert audio.shape == (2, 16000) and audio.dtype == torch.float32
    assert torch.equal(audio, ap.griffinlim(S, n_iter=4, n_fft=n_fft, length=16000, random_state=3))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        S_side = ap.mel_to_stft(mel, sr=sr, n_fft=n_fft)
    side.synchronize()
    assert torch.equal(S_side, S)
    assert ap.mfcc_to_audio(ap.mfcc(S=ap.power_to_db(mel), n_mfcc=128), n_iter=2, length=8000).shape == (2, 8000)


@pytest.mark.parametrize("norm", ["ortho", None])
def test_mfcc_to_mel_inverts_mfcc(norm):
    db = np.random.default_rng(3).uniform(-80, 0, (2, 40, 9)).astype(np.float32)
    c = ap.mfcc(S=db, n_mfcc=40, lifter=22, norm=norm).cpu().numpy()
    lift = (1 + 11 * np.sin(np.pi * np.arange(1, 41) / 22)) / (1 if norm else 2)       # dct(norm=None) is half of SciPy's
    inv = lambda dt: 10 ** (scipy.fft.idct((c / lift[:, None]).astype(dt), axis=-2, type=2, norm=norm) / dt(10))  # noqa: E731
    ref = inv(np.float64)
    got = ap.mfcc_to_mel(c, n_mels=40, lifter=22, norm=norm).cpu().numpy()
    err, bound = np.abs(got / ref - 1).max(), 4 * np.abs(inv(np.float32) / ref - 1).max()
    print(f"norm={norm}: {err:.2e} of {bound:.2e}")
    assert err <= bound
    # the power mfcc started from: two 40-term float32 contractions within 40 * 80 * 2^-23 = 4e-4 dB each, times ln(10) / 10
    np.testing.assert_allclose(got, 10 ** (db / 10.0), rtol=2e-4)
