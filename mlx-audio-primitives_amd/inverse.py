"""Feature inversion (librosa.feature.inverse's four functions): mel_to_stft, mel_to_audio, mfcc_to_mel, mfcc_to_audio.

``mel_to_stft`` solves, per frame, min_x ||A x - s||^2 with x >= 0 for the (n_mels, F) bank A by accelerated projected
gradient with a fixed step and a fixed iteration count: ONE launch of a fused kernel that reads the mel tile once, keeps
the iterates in LDS for every iteration and writes the magnitude once (csrc/kernels_nnls.h; stated in
numpy by tests/nnls_ref.py).  The starting point max(pinv(A) s, 0), the step 1 / lambda_max(A A^T) and the momentum
table are float64 on the host, cached per bank and device next to the filterbank caches of mel.py.  librosa's L-BFGS-B
solver is not reproduced: the result is the same minimiser approached by another route.

``mfcc_to_mel`` is the existing DCT contraction kernel run with the inverse basis (the lifter undone inside the basis)
followed by ``db_to_power``; ``mel_to_audio`` / ``mfcc_to_audio`` end in the fused ``griffinlim``.
"""

from __future__ import annotations

import hashlib
from functools import lru_cache

import numpy as np
import torch

from . import _extension as _x
from ._validation import validate_non_negative, validate_positive
from .convert import db_to_power
from .griffinlim import griffinlim
from .mel import mel_filterbank
from .stft import _padded_row_stride

MAX_BINS = 1025                         # ap_nnls_max_bins()
MAX_ROWS = 255                          # ap_nnls_max_rows()
FRAME_TILE = 16                         # frames a workgroup owns (APQ_TT)

_host_cache: dict[tuple, tuple] = {}
_device_cache: dict[tuple, tuple] = {}
_momentum_cache: dict[tuple, torch.Tensor] = {}


def _bank_host(fb_np: np.ndarray) -> tuple:
    """(key, plan int32, pinv float32 (F, M), step) of a non-negative (M, F) float32 bank: float64 on the host, cached by
    content.  ValueError for a bank that is negative somewhere, all zero, or over the kernel's limits."""
    key = (hashlib.sha256(fb_np.tobytes()).digest(), fb_np.shape)
    hit = _host_cache.get(key)
    if hit is None:
        M, F = fb_np.shape
        if M > MAX_ROWS or F > MAX_BINS:
            raise ValueError(f"a ({M}, {F}) filterbank is over the limits of {MAX_ROWS} rows and {MAX_BINS} bins")
        plan = _x.nnls_plan_host(fb_np)                                  # refuses negative / non-finite entries
        A = fb_np.astype(np.float64)
        top = float(np.linalg.eigvalsh(A @ A.T)[-1])
        if not top > 0.0:
            raise ValueError("filterbank must not be all zero")
        hit = (key, plan, np.ascontiguousarray(np.linalg.pinv(A), dtype=np.float32), 1.0 / top)
        if len(_host_cache) >= 32:
            _host_cache.pop(next(iter(_host_cache)))
        _host_cache[key] = hit
    return hit


def _bank_device(host: tuple, dev) -> tuple:
    """(plan, pinv) of `_bank_host`'s entry on `dev`, cached."""
    key = host[0] + (str(dev),)
    hit = _device_cache.get(key)
    if hit is None:
        hit = (torch.from_numpy(host[1]).to(dev), torch.from_numpy(host[2]).to(dev))
        if len(_device_cache) >= 32:
            _device_cache.pop(next(iter(_device_cache)))
        _device_cache[key] = hit
    return hit


@lru_cache(maxsize=64)
def _momentum_host(n_iter: int) -> np.ndarray:
    """(t - 1) / t' of t' = (1 + sqrt(1 + 4 t^2)) / 2 from t = 1, float64 rounded to float32 once."""
    out, t = np.empty(n_iter, np.float64), 1.0
    for i in range(n_iter):
        t_next = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        out[i] = (t - 1.0) / t_next
        t = t_next
    return out.astype(np.float32)


def _momentum(n_iter: int, dev) -> torch.Tensor:
    key = (n_iter, str(dev))
    hit = _momentum_cache.get(key)
    if hit is None:
        hit = _momentum_cache[key] = torch.from_numpy(_momentum_host(n_iter)).to(dev)
    return hit


def _as_bank(filterbank) -> np.ndarray:
    fb = filterbank.detach().cpu().numpy() if isinstance(filterbank, torch.Tensor) else np.asarray(filterbank)
    fb = np.ascontiguousarray(fb, dtype=np.float32)
    if fb.ndim != 2 or 0 in fb.shape:
        raise ValueError(f"filterbank must have shape (n_bands, n_bins), got {tuple(fb.shape)}")
    return fb


def nnls_fista(s, filterbank, *, n_iter: int = 100, power: float = 1.0, out: torch.Tensor | None = None) -> torch.Tensor:
    """argmin_{x >= 0} ||filterbank x - s||^2 per frame, then x ** (1 / power): the kernel behind `mel_to_stft`.

    s: (M, T) or (batch, M, T) float32 >= 0, dense or a view of rows padded behind T; filterbank: any non-negative
    (M, F) matrix within the limits (255 rows, 1025 bins); out: None or a (batch, F, T) float32 device tensor, dense or
    such a view, that receives the result.  Everything that can be refused is refused before a device is needed."""
    if not isinstance(s, torch.Tensor):
        s = torch.as_tensor(np.asarray(s))
    if s.ndim not in (2, 3):
        raise ValueError(f"M must be 2D or 3D, got {s.ndim}D")
    if s.is_complex():
        raise ValueError(f"M must be real (a mel power or magnitude spectrogram), got {s.dtype}")
    validate_positive(power, "power")
    validate_non_negative(n_iter, "n_iter")
    fb = _as_bank(filterbank)
    if s.shape[-2] != fb.shape[0]:
        raise ValueError(f"M has {s.shape[-2]} rows but the filterbank has {fb.shape[0]}: shapes {tuple(s.shape)} and {tuple(fb.shape)}")
    host = _bank_host(fb)
    dev = s.device if s.is_cuda else _x.require_device()
    _x.lib()
    if not (s.is_cuda and s.dtype == torch.float32):
        s = s.to(device=dev, dtype=torch.float32)                        # a padded-row view on the device stays a view
    two_d = s.ndim == 2
    if two_d:
        s = s[None]
    B, M, T = s.shape
    F = fb.shape[1]
    rs = _padded_row_stride(s)
    if rs is None:
        s, rs = s.contiguous(), T
    if out is None:
        out = torch.empty((B, F, T), dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, F, T)
              and (out.is_contiguous() or _padded_row_stride(out))):
        raise ValueError(f"out must be a float32 device tensor of shape {(B, F, T)} with dense or padded rows")
    ors = _padded_row_stride(out) or T
    if B and T:
        plan, pinv = _bank_device(host, dev)
        mom = _momentum(int(n_iter), dev) if n_iter else None
        _x.check(_x.dlib(dev).ap_nnls_fista_f32(_x.ptr(s), B, M, F, T, rs, _x.ptr(plan), _x.ptr(pinv), float(host[3]),
                                                None if mom is None else _x.ptr(mom), int(n_iter), float(power), _x.ptr(out),
                                                ors, _x.stream_ptr(dev)))
    return out[0] if two_d else out


def mel_to_stft(M, *, sr: float = 22050, n_fft: int = 2048, power: float = 2.0, n_iter: int = 100, filterbank=None,
                **kwargs) -> torch.Tensor:
    """Approximate STFT magnitude of a mel spectrogram (librosa.feature.inverse.mel_to_stft).

    M: (n_mels, T) or (batch, n_mels, T), the output of `melspectrogram(..., power=power)`.  Returns the magnitude
    (.., n_fft // 2 + 1, T): the non-negative least-squares solution of `mel_basis @ x = M` after `n_iter` accelerated
    projected-gradient iterations, to the power 1 / power.  kwargs go to `mel_filterbank` (fmin, fmax, htk, norm);
    `filterbank` replaces the mel basis by any non-negative (n_mels, n_fft // 2 + 1) matrix (`bark_filterbank`, ..)."""
    validate_positive(n_fft, "n_fft")
    if not isinstance(M, torch.Tensor):
        M = torch.as_tensor(np.asarray(M))
    if M.ndim not in (2, 3):
        raise ValueError(f"M must be 2D or 3D, got {M.ndim}D")
    if filterbank is None:
        fb = mel_filterbank(sr, int(n_fft), int(M.shape[-2]), device="cpu", **kwargs)
    else:
        if kwargs:
            raise TypeError(f"mel_to_stft() got filterbank= and the mel_filterbank keywords {sorted(kwargs)}")
        fb = _as_bank(filterbank)
        if fb.shape[1] != 1 + int(n_fft) // 2:
            raise ValueError(f"filterbank must have shape (n_bands, {1 + int(n_fft) // 2}), got {tuple(fb.shape)}")
    return nnls_fista(M, fb, n_iter=n_iter, power=power)


def mel_to_audio(M, *, sr: float = 22050, n_fft: int = 2048, hop_length: int | None = None, win_length: int | None = None,
                 window="hann", center: bool = True, pad_mode: str = "constant", power: float = 2.0, n_iter: int = 32,
                 length: int | None = None, nnls_iter: int = 100, random_state: int | None = None, **kwargs) -> torch.Tensor:
    """Waveform of a mel spectrogram (librosa.feature.inverse.mel_to_audio): `griffinlim(mel_to_stft(M))`.

    n_iter is Griffin-Lim's, nnls_iter `mel_to_stft`'s; random_state seeds Griffin-Lim's initial phase; kwargs go to
    `mel_filterbank`.  Returns (length,) or (batch, length) float32."""
    S = mel_to_stft(M, sr=sr, n_fft=n_fft, power=power, n_iter=nnls_iter, **kwargs)
    return griffinlim(S, n_iter=n_iter, hop_length=hop_length, win_length=win_length, n_fft=n_fft, window=window,
                      center=center, length=length, pad_mode=pad_mode, random_state=random_state)


@lru_cache(maxsize=64)
def _idct_basis(n_mels: int, n_mfcc: int, norm, lifter: float) -> np.ndarray:
    """(n_mels, n_mfcc) float32, built in float64: the inverse of this package's `dct(., n=n_mels, norm=norm)` on its
    first n_mfcc coefficients, divided by the lifter, as one matrix.  norm="ortho" is the transposed basis; norm=None
    (`dct` sums x cos, half of SciPy's unnormalised DCT-II) is the transposed basis times 2 / n_mels, 1 / n_mels for k = 0:
    scipy.fft.idct(2 c, type=2, n=n_mels)."""
    n, k = np.arange(n_mels, dtype=np.float64)[:, None], np.arange(n_mfcc, dtype=np.float64)[None, :]
    basis = np.cos(np.pi * k * (2.0 * n + 1.0) / (2.0 * n_mels))
    if norm == "ortho":
        basis *= np.where(k == 0, np.sqrt(1.0 / n_mels), np.sqrt(2.0 / n_mels))
    else:
        basis *= np.where(k == 0, 1.0, 2.0) / n_mels
    if lifter > 0:
        basis /= 1.0 + (lifter / 2.0) * np.sin(np.pi * (k + 1.0) / lifter) + np.finfo(np.float32).tiny
    return np.ascontiguousarray(basis, dtype=np.float32)


def mfcc_to_mel(mfcc, *, n_mels: int = 128, dct_type: int = 2, norm: str | None = "ortho", ref: float = 1.0,
                lifter: float = 0) -> torch.Tensor:
    """Mel power spectrogram of MFCCs (librosa.feature.inverse.mfcc_to_mel): undo the lifter, invert the DCT-II onto
    n_mels bands (the coefficients beyond n_mfcc count as zero), then `db_to_power(., ref)`.

    mfcc: (n_mfcc, T) or (batch, n_mfcc, T).  Returns (.., n_mels, T) float32."""
    if dct_type != 2:
        raise ValueError(f"Only DCT type 2 is supported, got {dct_type}")
    if norm not in ("ortho", None):
        raise ValueError(f"Unknown norm: '{norm}'. Supported: 'ortho', None")
    validate_positive(n_mels, "n_mels")
    if lifter < 0:
        raise ValueError(f"lifter must be non-negative, got {lifter}")
    ndim = getattr(mfcc, "ndim", None)
    if ndim not in (2, 3):
        raise ValueError(f"mfcc must be 2D or 3D, got {ndim}D")
    n_mfcc = int(mfcc.shape[-2])
    if not 1 <= n_mfcc <= n_mels:
        raise ValueError(f"mfcc must hold between 1 and n_mels={n_mels} coefficients, got {n_mfcc}")
    basis_np = _idct_basis(int(n_mels), n_mfcc, norm, float(lifter))
    x = _x.to_device_f32(mfcc)
    two_d = x.ndim == 2
    if two_d:
        x = x[None]
    B, _, T = x.shape
    basis = torch.from_numpy(basis_np).to(x.device)
    logmel = torch.empty((B, int(n_mels), T), dtype=torch.float32, device=x.device)
    if logmel.numel():
        _x.check(_x.dlib(x.device).ap_dct_f32(_x.ptr(x), _x.ptr(basis), None, B, n_mfcc, T, int(n_mels), _x.ptr(logmel),
                                              _x.stream_ptr(x.device)))
    out = db_to_power(logmel, ref=ref)
    return out[0] if two_d else out


def mfcc_to_audio(mfcc, *, n_mels: int = 128, dct_type: int = 2, norm: str | None = "ortho", ref: float = 1.0,
                  lifter: float = 0, **kwargs) -> torch.Tensor:
    """Waveform of MFCCs (librosa.feature.inverse.mfcc_to_audio): `mel_to_audio(mfcc_to_mel(..), **kwargs)`."""
    return mel_to_audio(mfcc_to_mel(mfcc, n_mels=n_mels, dct_type=dct_type, norm=norm, ref=ref, lifter=lifter), **kwargs)


__all__ = ["mel_to_stft", "mel_to_audio", "mfcc_to_mel", "mfcc_to_audio", "nnls_fista"]
