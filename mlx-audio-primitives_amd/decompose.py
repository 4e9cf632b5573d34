"""Harmonic / percussive source separation by median filtering (no counterpart in the reference; the signatures
of librosa.decompose.hpss and librosa.effects.hpss / harmonic / percussive).

On M = |S|: `harm` is the running median of every row along time, `perc` of every column along frequency
(scipy.ndimage.median_filter with mode="reflect", bit for bit), and librosa's soft mask of one against the other
(times its margin) splits S.  One fused kernel per call (csrc/kernels_hpss.h): a comparator network
on registers for the default 31 x 31 windows, rank counting for every other size up to 255; the medians and masks
never reach HBM unless they are what is asked for.

Deviations from librosa, on purpose: the components are S * mask (librosa: |S| * mask * S / |S|, one rounding more,
the same zero at |S| = 0); non-negativity of a real S is not checked (a synchronising readback): results are defined
for finite, non-negative magnitudes.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _extension as _x
from .stft import _padded_row_stride, istft, stft

_MODE_COMPONENTS, _MODE_MASKS, _MODE_MEDIANS = 0, 1, 2


def _kernel_sizes(kernel_size):
    pair = tuple(kernel_size) if isinstance(kernel_size, (tuple, list)) else (kernel_size, kernel_size)
    if len(pair) != 2 or any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 255
                             for k in pair):
        raise ValueError(f"kernel_size must be an integer in 1 .. 255, or a (harmonic, percussive) pair of them, "
                         f"got {kernel_size!r}")
    return int(pair[0]), int(pair[1])


def _margins(margin):
    pair = tuple(margin) if isinstance(margin, (tuple, list)) else (margin, margin)
    if len(pair) != 2:
        raise ValueError(f"margin must be a number or a (harmonic, percussive) pair, got {margin!r}")
    if not all(float(m) >= 1.0 for m in pair):
        raise ValueError("Margins must be >= 1.0. A typical range is between 1 and 10.")
    return float(pair[0]), float(pair[1])


def _power(power):
    if not float(power) > 0.0:
        raise ValueError("power must be strictly positive")
    return float(power)


def _spectrum(S):
    """Validated (S as a torch tensor, was it 2D?) - still wherever the caller had it."""
    if not isinstance(S, torch.Tensor):
        S = torch.as_tensor(np.asarray(S))
    if S.ndim not in (2, 3):
        raise ValueError(f"S must be 2D or 3D, got {S.ndim}D")
    if S.dtype not in (torch.float32, torch.complex64):
        raise ValueError(f"S must be float32 or complex64, got {S.dtype}")
    return S, S.ndim == 2


def _run(S, kh, kp, mh, mp, power, mode, want_h=True, want_p=True, general=False):
    """One ap_hpss_f32 call on a validated 2D / 3D spectrum: (out_h, out_p), None for an output not asked for.
    `general` forces the rank-counting kernel (the cross-check of the network kernel)."""
    S, two_d = _spectrum(S)
    dev = S.device if S.is_cuda else _x.require_device()
    _x.lib()
    S = S.to(dev)
    if two_d:
        S = S[None]
    B, F, T = S.shape
    cplx = S.is_complex()
    cplx_out = cplx and mode == _MODE_COMPONENTS
    row_stride = _padded_row_stride(S) if B * F * T else None
    if row_stride is None:
        S = S.contiguous()
    rs_in = row_stride if row_stride is not None else T
    # line-padded complex rows in -> line-padded complex rows out (istft reads them in place); everything else dense
    rs_out = rs_in if cplx_out else T

    def alloc():
        if cplx_out and B * F * T:
            return torch.view_as_complex(torch.empty((B, F, rs_out, 2), dtype=torch.float32, device=dev))[:, :, :T]
        return torch.empty((B, F, T), dtype=torch.complex64 if cplx_out else torch.float32, device=dev)

    def raw(t):
        return _x.ptr(torch.view_as_real(t) if t.is_complex() else t)

    out_h = alloc() if want_h else None
    out_p = alloc() if want_p else None
    if B * F * T:
        _x.check(_x.dlib(dev).ap_hpss_f32(raw(S), int(cplx), B, F, T, rs_in, kh, kp, mh, mp, power, mode,
                                          int(bool(general)), None if out_h is None else raw(out_h),
                                          None if out_p is None else raw(out_p), rs_out, _x.stream_ptr(dev)))
    if two_d:
        out_h, out_p = (None if o is None else o[0] for o in (out_h, out_p))
    return out_h, out_p


def hpss(S, *, kernel_size=31, power: float = 2.0, mask: bool = False, margin=1.0):
    """Harmonic / percussive separation of a spectrum (librosa.decompose.hpss).

    S: (F, T) or (batch, F, T), real float32 (a magnitude) or complex64, dense or the line-padded view `stft`
    returns.  kernel_size and margin: a number or a (harmonic, percussive) pair; power: exponent of the soft mask
    (inf: hard mask).  Returns (harmonic, percussive) of S's dtype, or the two real masks with mask=True.  For a
    line-padded complex S the components are line-padded views of the same row stride, which `istft` reads in place."""
    kh, kp = _kernel_sizes(kernel_size)
    mh, mp = _margins(margin)
    power = _power(power)
    _spectrum(S)
    return _run(S, kh, kp, mh, mp, power, _MODE_MASKS if mask else _MODE_COMPONENTS)


def hpss_medians(S, *, kernel_size=31):
    """The two median filters of `hpss` alone: (harm, perc), real and dense; harm = the median of |S| over
    kernel_size[0] frames along time, perc over kernel_size[1] bins along frequency, both with SciPy's "reflect"
    boundary (equal to scipy.ndimage.median_filter in every bit)."""
    kh, kp = _kernel_sizes(kernel_size)
    _spectrum(S)
    return _run(S, kh, kp, 1.0, 1.0, 2.0, _MODE_MEDIANS)


def _audio(y, want_h, want_p, kernel_size, power, margin, n_fft, hop_length, win_length, window, center, pad_mode):
    kh, kp = _kernel_sizes(kernel_size)
    mh, mp = _margins(margin)
    power = _power(power)
    ndim = len(np.shape(y)) if not isinstance(y, torch.Tensor) else y.ndim
    if ndim not in (1, 2):
        raise ValueError(f"y must be 1D or 2D, got {ndim}D")
    L = int(y.shape[-1]) if hasattr(y, "shape") else len(y)
    S = stft(y, n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window, center=center,
             pad_mode=pad_mode)
    H, P = _run(S, kh, kp, mh, mp, power, _MODE_COMPONENTS, want_h, want_p)
    back = dict(hop_length=hop_length, win_length=win_length, n_fft=n_fft, window=window, center=center, length=L)
    return (None if H is None else istft(H, **back)), (None if P is None else istft(P, **back))


def hpss_audio(y, *, kernel_size=31, power: float = 2.0, margin=1.0, n_fft: int = 2048,
               hop_length: int | None = None, win_length: int | None = None, window="hann", center: bool = True,
               pad_mode: str = "constant"):
    """(y_harmonic, y_percussive) of a signal (samples,) or (batch, samples), each of y's length
    (librosa.effects.hpss): stft -> hpss -> istft of both components."""
    return _audio(y, True, True, kernel_size, power, margin, n_fft, hop_length, win_length, window, center, pad_mode)


def harmonic(y, *, kernel_size=31, power: float = 2.0, margin=1.0, n_fft: int = 2048,
             hop_length: int | None = None, win_length: int | None = None, window="hann", center: bool = True,
             pad_mode: str = "constant"):
    """The harmonic part of a signal (librosa.effects.harmonic); the percussive component is neither masked nor stored."""
    return _audio(y, True, False, kernel_size, power, margin, n_fft, hop_length, win_length, window, center, pad_mode)[0]


def percussive(y, *, kernel_size=31, power: float = 2.0, margin=1.0, n_fft: int = 2048,
               hop_length: int | None = None, win_length: int | None = None, window="hann", center: bool = True,
               pad_mode: str = "constant"):
    """The percussive part of a signal (librosa.effects.percussive); the harmonic component is neither masked nor stored."""
    return _audio(y, False, True, kernel_size, power, margin, n_fft, hop_length, win_length, window, center, pad_mode)[1]


__all__ = ["hpss", "hpss_medians", "hpss_audio", "harmonic", "percussive"]
