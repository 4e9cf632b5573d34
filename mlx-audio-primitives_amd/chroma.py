"""Chroma features (no counterpart in the reference; the signatures of librosa 0.10's librosa.feature.chroma_stft,
chroma_cqt, chroma_cens, tonnetz and librosa.filters.chroma, cq_to_chroma).

Two fused kernels (csrc/kernels_chroma.h), each one pass over a spectrum another kernel produced:

    fold   v_k = S, |C| or |X|^2;  a_c = sum_k w[c,k] v_k;  optional a /= sum_k |v_k|;  a_c < threshold -> 0;
           out = a / norm(a)                                                  (chroma_stft, chroma_cqt, tonnetz)
    cens   v = chroma / sum_c |chroma|;  q = 0.25 ([v > .4] + [v > .2] + [v > .1] + [v > .05]);
           s = q smoothed along time ("same");  out = s / norm(s)              (chroma_cens)

A norm (1, 2, inf) below the smallest normal float32 counts as 1: an all-zero frame stays zero (librosa's
util.normalize with fill=None).  The matrices w are built on the host in float64, rounded once to float32 and cached
per device under their content.

Deviations from librosa, on purpose.  tuning defaults to 0.0 where librosa's default None estimates it from the signal;
tuning=None raises ValueError (pass tuning=estimate_tuning(y=y, sr=sr, bins_per_octave=...)).  chroma_cqt reads this package's direct-form cqt
(any hop_length >= 1, nothing decimated); cqt_mode other than "full" raises.  No parity with librosa's numbers is
claimed: the specification is the float64 definition in tests/chroma_ref.py.
"""

from __future__ import annotations

import hashlib
import math

import numpy as np
import torch

from . import _extension as _x
from .cqt import _C1, _is_real, _signal
from .cqt import cqt as _cqt
from .onset import _is_int, _rows

_TINY = float(np.finfo(np.float32).tiny)
_NORM_CODES = {None: 0, 1: 1, 2: 2, np.inf: 3}

_device_bank_cache: dict[tuple, torch.Tensor] = {}
_host_bank_cache: dict[tuple, tuple] = {}


# ---------------------------------------------------------------------------------------------------------------------
# host builders
# ---------------------------------------------------------------------------------------------------------------------
def _norm_arg(norm, name="norm"):
    if norm is not None and (not _is_real(norm) or norm not in (1, 2, np.inf)):
        raise ValueError(f"{name} must be 1, 2, inf or None, got {norm!r}")
    return None if norm is None else (np.inf if norm == np.inf else int(norm))


def _n_chroma_arg(n_chroma):
    if not _is_int(n_chroma) or n_chroma < 1:
        raise ValueError(f"n_chroma must be a positive integer, got {n_chroma!r}")
    return int(n_chroma)


def _tuning_arg(tuning):
    if tuning is None:
        raise ValueError("tuning=None (estimate the tuning from the signal) is not done here; pass "
                         "tuning=estimate_tuning(y=y, sr=sr, bins_per_octave=...) or a number of bins")
    if not _is_real(tuning) or not math.isfinite(float(tuning)):
        raise ValueError(f"tuning must be a finite number, got {tuning!r}")
    return float(tuning)


def _sr_arg(sr):
    if not _is_real(sr) or not float(sr) > 0.0 or not math.isfinite(float(sr)):
        raise ValueError(f"sr must be strictly positive, got {sr!r}")
    return float(sr)


def _normalize_columns(w: np.ndarray, norm) -> np.ndarray:
    """w / norm of each column; a norm below the smallest normal float32 counts as 1."""
    if norm is None:
        return w
    a = np.abs(w)
    n = a.max(axis=0) if norm == np.inf else a.sum(axis=0) if norm == 1 else np.sqrt((a * a).sum(axis=0))
    return w / np.where(n < _TINY, 1.0, n)


def _convolve_same(rows: np.ndarray, taps: np.ndarray) -> np.ndarray:
    """s[t] = sum_j taps[j] q[t + (n_taps - 1) // 2 - j] along the last axis, q = 0 outside (SciPy's "same")."""
    n, T = len(taps), rows.shape[-1]
    h = (n - 1) // 2
    padded = np.zeros(rows.shape[:-1] + (T + n - 1,), np.float64)
    padded[..., n - 1 - h:n - 1 - h + T] = rows
    out = np.zeros(rows.shape, np.float64)
    for j in range(n):
        out += taps[j] * padded[..., n - 1 - j:n - 1 - j + T]
    return out


def _finish(a: np.ndarray) -> np.ndarray:
    out = np.ascontiguousarray(a.astype(np.float32))          # the one rounding
    out.setflags(write=False)
    return out


def chroma_filterbank(*, sr: float, n_fft: int, n_chroma: int = 12, tuning: float = 0.0, ctroct: float = 5.0, octwidth=2,
                      norm=2, base_c: bool = True) -> np.ndarray:
    """The matrix that folds an STFT onto pitch classes (librosa.filters.chroma): float32 (n_chroma, 1 + n_fft // 2),
    read-only, built in float64 and rounded once.  Bin k lies at fb[k] = n_chroma log2(f_k / (A440 / 16)) chroma
    bins; row c weighs it by a Gaussian of its distance to c modulo the octave, as wide as the bin spacing;
    the columns are normalised by `norm` (1, 2, inf or None), weighted by a Gaussian in octaves around `ctroct` of width
    `octwidth` (None: no weighting), and the rows are rotated so that row 0 is C (base_c) or A."""
    sr = _sr_arg(sr)
    if not _is_int(n_fft) or n_fft < 2:
        raise ValueError(f"n_fft must be an integer >= 2, got {n_fft!r}")
    n_chroma = _n_chroma_arg(n_chroma)
    tuning = _tuning_arg(tuning)
    norm = _norm_arg(norm)
    if not _is_real(ctroct) or not math.isfinite(float(ctroct)):
        raise ValueError(f"ctroct must be a finite number, got {ctroct!r}")
    if octwidth is not None and (not _is_real(octwidth) or not float(octwidth) > 0.0 or not math.isfinite(float(octwidth))):
        raise ValueError(f"octwidth must be strictly positive or None, got {octwidth!r}")
    n_fft = int(n_fft)
    fr = np.linspace(0.0, sr, n_fft, endpoint=False)[1:]
    a440 = 440.0 * 2.0 ** (tuning / n_chroma)
    fb = n_chroma * np.log2(fr / (a440 / 16.0))
    fb = np.concatenate(([fb[0] - 1.5 * n_chroma], fb))
    bw = np.concatenate((np.maximum(np.diff(fb), 1.0), [1.0]))
    h = np.round(n_chroma / 2.0)
    D = np.remainder(fb[None, :] - np.arange(n_chroma, dtype=np.float64)[:, None] + h + 10 * n_chroma, n_chroma) - h
    w = np.exp(-0.5 * (2.0 * D / bw[None, :]) ** 2)
    w = _normalize_columns(w, norm)
    if octwidth is not None:
        w = w * np.exp(-0.5 * ((fb / n_chroma - float(ctroct)) / float(octwidth)) ** 2)[None, :]
    if base_c:
        w = np.roll(w, -3 * (n_chroma // 12), axis=0)
    return _finish(w[:, :1 + n_fft // 2])


def cq_to_chroma(n_input: int, *, bins_per_octave: int = 12, n_chroma: int = 12, fmin=None, window=None,
                 base_c: bool = True) -> np.ndarray:
    """The matrix that folds a constant-Q spectrum of n_input bands onto pitch classes (librosa.filters.cq_to_chroma):
    float32 (n_chroma, n_input), read-only.  Each pitch class sums the bins_per_octave / n_chroma bands around it in
    every octave; fmin (None: C1) sets which row band 0 falls into; window: None or 1-D taps that smooth each row
    along the bands ("same" convolution)."""
    if not _is_int(n_input) or n_input < 1:
        raise ValueError(f"n_input must be a positive integer, got {n_input!r}")
    if not _is_int(bins_per_octave) or bins_per_octave < 1:
        raise ValueError(f"bins_per_octave must be a positive integer, got {bins_per_octave!r}")
    n_chroma = _n_chroma_arg(n_chroma)
    if bins_per_octave % n_chroma != 0:
        raise ValueError(f"bins_per_octave={bins_per_octave} must be an integer multiple of n_chroma={n_chroma}")
    if fmin is None:
        fmin = _C1
    if not _is_real(fmin) or not float(fmin) > 0.0 or not math.isfinite(float(fmin)):
        raise ValueError(f"fmin must be strictly positive, got {fmin!r}")
    n_input, bpo = int(n_input), int(bins_per_octave)
    m = bpo // n_chroma
    w = np.repeat(np.eye(n_chroma), m, axis=1)
    w = np.roll(w, -(m // 2), axis=1)
    w = np.tile(w, int(math.ceil(n_input / bpo)))[:, :n_input]
    r = np.mod(69.0 + 12.0 * math.log2(float(fmin) / 440.0), 12.0)
    if not base_c:
        r -= 9.0
    w = np.roll(w, int(np.round(r * (n_chroma / 12.0))), axis=0)
    if window is not None:
        taps = np.asarray(window, np.float64)
        if taps.ndim != 1 or taps.size < 1:
            raise ValueError(f"window must be None or a 1-D array of taps, got shape {taps.shape}")
        w = _convolve_same(w, taps)
    return _finish(w)


def _phi64(n_chroma: int) -> np.ndarray:
    """The tonal-centroid basis (6, n_chroma) in float64: fifths, minor thirds, major thirds as (sin, cos) pairs."""
    V = np.outer([7.0 / 6, 7.0 / 6, 3.0 / 2, 3.0 / 2, 2.0 / 3, 2.0 / 3], np.linspace(0.0, 12.0, n_chroma, endpoint=False))
    V[::2] -= 0.5
    R = np.array([1.0, 1.0, 1.0, 1.0, 0.5, 0.5])
    return R[:, None] * np.cos(np.pi * V)


# ---------------------------------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------------------------------
def _cached_host(key, build):
    """A host matrix under its arguments, with the sha256 of its bytes (bounded, oldest out first)."""
    hit = _host_bank_cache.get(key)
    if hit is None:
        w = build()
        hit = (w, hashlib.sha256(w.tobytes() + repr(w.shape).encode()).digest())
        if len(_host_bank_cache) >= 32:
            _host_bank_cache.pop(next(iter(_host_bank_cache)))
        _host_bank_cache[key] = hit
    return hit


def _device_bank(host, dev) -> torch.Tensor:
    """The matrix on `dev`, cached under its content (bounded, oldest out first)."""
    w, digest = host
    key = (digest, str(dev))
    hit = _device_bank_cache.get(key)
    if hit is None:
        hit = torch.from_numpy(w.copy()).to(dev)
        if len(_device_bank_cache) >= 32:
            _device_bank_cache.pop(next(iter(_device_bank_cache)))
        _device_bank_cache[key] = hit
    return hit


def _check_n_chroma(n_chroma):
    cap = int(_x.lib().ap_chroma_max_out())
    if n_chroma > cap:
        raise ValueError(f"n_chroma={n_chroma} is above the kernel's cap of {cap}")


def _one_of(y, other, name):
    if (y is None) == (other is None):
        raise ValueError(f"exactly one of y and {name} must be given")


def _spectrum(S, name, allow_complex):
    """(device tensor (B, K, T) float32 / complex64, was it 2D?).  Validation first, the device after."""
    if not isinstance(S, torch.Tensor):
        S = torch.as_tensor(np.asarray(S))
    if S.ndim not in (2, 3):
        raise ValueError(f"{name} must be 2D (bins, frames) or 3D (batch, bins, frames), got {S.ndim}D")
    if S.is_complex() and not allow_complex:
        raise ValueError(f"{name} must be real, got {S.dtype}")
    if 0 in S.shape[-2:]:
        raise ValueError(f"{name} must hold at least one bin and one frame, got shape {tuple(S.shape)}")
    want = torch.complex64 if S.is_complex() else torch.float32
    dev = S.device if S.is_cuda else _x.require_device()
    _x.lib()
    if not (S.is_cuda and S.dtype == want):
        S = S.to(device=dev, dtype=want)                    # a padded-row view on the device stays a view
    two_d = S.ndim == 2
    return (S[None] if two_d else S), two_d


def _fold(x: torch.Tensor, in_kind: int, host, *, pre_l1=False, threshold=None, norm=None) -> torch.Tensor:
    """One launch of ap_chroma_fold_f32 on x (B, K, T) with the host matrix (w, digest)."""
    B, K, T = x.shape
    n_out = host[0].shape[0]
    dev = x.device
    out = torch.empty((B, n_out, T), dtype=torch.float32, device=dev)
    if B:
        x, rs = _rows(x)
        w = _device_bank(host, dev)
        _x.check(_x.dlib(dev).ap_chroma_fold_f32(_x.ptr(x), int(in_kind), B, K, T, rs, _x.ptr(w), n_out, int(bool(pre_l1)),
                                                 int(threshold is not None), float(threshold or 0.0), _NORM_CODES[norm],
                                                 _x.ptr(out), T, _x.stream_ptr(dev)))
    return out


def chroma_stft(*, y=None, sr: float = 22050, S=None, norm=np.inf, n_fft: int = 2048, hop_length: int = 512, win_length=None,
                window="hann", center: bool = True, pad_mode: str = "constant", tuning=0.0, n_chroma: int = 12,
                ctroct: float = 5.0, octwidth=2, base_c: bool = True):
    """Chromagram of a power spectrogram (librosa.feature.chroma_stft's signature).

    y: (samples,) or (batch, samples), float32 or int16 PCM: |stft(y)|^2 is taken inside the fold kernel, which reads
    stft's result (its line-padded rows included) in place.  S: a real power spectrogram (F, T) or (batch, F, T)
    instead; n_fft is then 2 (F - 1).  Exactly one of y and S.  norm: 1, 2, inf or None, per frame.  tuning is a number
    of chroma bins; the default is 0.0 where librosa's is None (estimate it), and tuning=None raises ValueError.
    The other arguments are chroma_filterbank's.  Returns float32 (n_chroma, T) or (batch, n_chroma, T) on the
    input's device and current stream."""
    _one_of(y, S, "S")
    norm = _norm_arg(norm)
    n_chroma = _n_chroma_arg(n_chroma)
    _tuning_arg(tuning)
    if S is not None:
        x, squeeze = _spectrum(S, "S", allow_complex=False)
        if x.shape[1] < 2:
            raise ValueError(f"S must hold at least 2 frequency bins, got {x.shape[1]}")
        n_fft, kind = 2 * (x.shape[1] - 1), 0
    else:
        if not _is_int(n_fft) or n_fft < 2:
            raise ValueError(f"n_fft must be an integer >= 2, got {n_fft!r}")
        if not _is_int(hop_length) or hop_length < 1:
            raise ValueError(f"hop_length must be a positive integer, got {hop_length!r}")
        kind = 2
    _check_n_chroma(n_chroma)
    # the filter bank's own column norm is librosa's fixed 2; `norm` is the per-frame one
    key = ("stft", _sr_arg(sr), int(n_fft), n_chroma, float(tuning), repr(ctroct), repr(octwidth), bool(base_c))
    host = _cached_host(key, lambda: chroma_filterbank(sr=sr, n_fft=int(n_fft), n_chroma=n_chroma, tuning=tuning, ctroct=ctroct,
                                                       octwidth=octwidth, norm=2, base_c=base_c))
    if y is not None:
        from .stft import stft

        yd, squeeze = _signal(y)
        x = stft(yd, n_fft=int(n_fft), hop_length=int(hop_length), win_length=win_length, window=window, center=center,
                 pad_mode=pad_mode)
    out = _fold(x, kind, host, norm=norm)
    return out[0] if squeeze else out


def _chroma_cqt_args(hop_length, fmin, norm, threshold, tuning, n_chroma, n_octaves, window, bins_per_octave, cqt_mode):
    if cqt_mode != "full":
        raise ValueError(f"cqt_mode: only 'full' is implemented (there is no hybrid_cqt), got {cqt_mode!r}")
    norm = _norm_arg(norm)
    n_chroma = _n_chroma_arg(n_chroma)
    tuning = _tuning_arg(tuning)
    if threshold is not None and (not _is_real(threshold) or math.isnan(float(threshold))):
        raise ValueError(f"threshold must be a number or None, got {threshold!r}")
    if not _is_int(n_octaves) or n_octaves < 1:
        raise ValueError(f"n_octaves must be a positive integer, got {n_octaves!r}")
    if not _is_int(bins_per_octave) or bins_per_octave < 1:
        raise ValueError(f"bins_per_octave must be a positive integer, got {bins_per_octave!r}")
    if not _is_int(hop_length) or hop_length < 1:
        raise ValueError(f"hop_length must be a positive integer, got {hop_length!r}")
    if bins_per_octave % n_chroma != 0:
        raise ValueError(f"bins_per_octave={bins_per_octave} must be an integer multiple of n_chroma={n_chroma}")
    if fmin is not None and (not _is_real(fmin) or not float(fmin) > 0.0 or not math.isfinite(float(fmin))):
        raise ValueError(f"fmin must be strictly positive, got {fmin!r}")
    if window is not None:
        window = np.asarray(window, np.float64)
        if window.ndim != 1 or window.size < 1:
            raise ValueError(f"window must be None or a 1-D array of taps, got shape {window.shape}")
    return norm, n_chroma, tuning, None if threshold is None else float(threshold), window


def chroma_cqt(*, y=None, sr: float = 22050, C=None, hop_length: int = 512, fmin=None, norm=np.inf, threshold=0.0, tuning=0.0,
               n_chroma: int = 12, n_octaves: int = 7, window=None, bins_per_octave: int = 36, cqt_mode: str = "full"):
    """Chromagram of a constant-Q spectrum (librosa.feature.chroma_cqt's signature).

    y: (samples,) or (batch, samples), float32 or int16 PCM: cqt(y, n_bins=n_octaves * bins_per_octave, ...) and the
    fold kernel takes |C| as it reads the complex result; |C| is never stored.  C: a constant-Q spectrum (K, T) or
    (batch, K, T) instead, real (used as it is) or complex (its magnitude is taken in the kernel).  Exactly one of y
    and C.  fmin=None: C1.  threshold: chroma values below it become 0 before the normalisation; None turns it off.
    norm: 1, 2, inf or None, per frame.  window: None or 1-D taps that smooth the fold matrix across bands.  tuning
    is a number of bins; the default is 0.0 where librosa's is None (estimate it), and tuning=None raises ValueError.
    cqt_mode: only "full".  Returns float32 (n_chroma, T) or (batch, n_chroma, T) on the input's device and current
    stream."""
    _one_of(y, C, "C")
    norm, n_chroma, tuning, threshold, window = _chroma_cqt_args(hop_length, fmin, norm, threshold, tuning, n_chroma, n_octaves,
                                                                  window, bins_per_octave, cqt_mode)
    if C is not None:
        x, squeeze = _spectrum(C, "C", allow_complex=True)
        kind = 1 if x.is_complex() else 0
    else:
        _check_n_chroma(n_chroma)
        _sr_arg(sr)
        c = _cqt(y, sr=sr, hop_length=hop_length, fmin=fmin, n_bins=int(n_octaves) * int(bins_per_octave),
                 bins_per_octave=bins_per_octave, tuning=tuning)
        squeeze = c.ndim == 2
        x, kind = (c[None] if squeeze else c), 1
    K = int(x.shape[1])
    key = ("cq", K, int(bins_per_octave), n_chroma, None if fmin is None else float(fmin), None if window is None else window.tobytes())
    host = _cached_host(key, lambda: cq_to_chroma(K, bins_per_octave=bins_per_octave, n_chroma=n_chroma, fmin=fmin, window=window))
    _check_n_chroma(n_chroma)
    out = _fold(x, kind, host, threshold=threshold, norm=norm)
    return out[0] if squeeze else out


def _smoothing_taps(win_len_smooth, smoothing_window):
    """The smoothing taps as a read-only float32 array, or None."""
    if not isinstance(smoothing_window, str):
        taps = np.asarray(smoothing_window, np.float64)
        if taps.ndim != 1 or taps.size < 1:
            raise ValueError(f"smoothing_window must be a window name or a 1-D array of taps, got shape {taps.shape}")
    else:
        if win_len_smooth is None or win_len_smooth == 0:
            return None
        if not _is_int(win_len_smooth) or win_len_smooth < 0:
            raise ValueError(f"win_len_smooth must be a non-negative integer or None, got {win_len_smooth!r}")
        name = smoothing_window.lower()
        if name not in _x.WINDOW_KINDS:
            raise ValueError(f"Unknown window type: '{name}'. Supported: {', '.join(sorted(_x.WINDOW_KINDS))}")
        taps = _x.generate_window_host(name, int(win_len_smooth) + 2, False).astype(np.float64)
        taps = taps / taps.sum()
    cap = int(_x.lib().ap_chroma_max_smooth())
    if taps.size > cap:
        raise ValueError(f"the smoothing window has {taps.size} taps (win_len_smooth + 2), above the kernel's cap of {cap}")
    return _finish(taps)


def _cens(x: torch.Tensor, taps, norm) -> torch.Tensor:
    """One launch of ap_chroma_cens_f32 on chroma x (B, n, T) float32."""
    B, n, T = x.shape
    dev = x.device
    out = torch.empty((B, n, T), dtype=torch.float32, device=dev)
    if B:
        x, rs = _rows(x)
        td = None if taps is None else _device_bank((taps, hashlib.sha256(b"taps" + taps.tobytes()).digest()), dev)
        _x.check(_x.dlib(dev).ap_chroma_cens_f32(_x.ptr(x), B, n, T, rs, None if td is None else _x.ptr(td),
                                                 0 if taps is None else int(taps.size), _NORM_CODES[norm], _x.ptr(out), T,
                                                 _x.stream_ptr(dev)))
    return out


def chroma_cens(*, y=None, sr: float = 22050, C=None, hop_length: int = 512, fmin=None, tuning=0.0, n_chroma: int = 12,
                n_octaves: int = 7, bins_per_octave: int = 36, cqt_mode: str = "full", window=None, norm=2,
                win_len_smooth=41, smoothing_window="hann"):
    """Chroma energy normalised statistics (librosa.feature.chroma_cens's signature).

    chroma_cqt(..., norm=None) (threshold 0), then one kernel: every frame is L1-normalised, quantised to
    0.25 ([v > .4] + [v > .2] + [v > .1] + [v > .05]), smoothed along time with the window's taps ("same", zeros beyond
    the clip) and normalised by `norm`.  The taps are the symmetric window of win_len_smooth + 2 points divided by its
    sum; smoothing_window may also be a 1-D array of taps; win_len_smooth None or 0: no smoothing.  tuning defaults to
    0.0 where librosa's is None, and tuning=None raises ValueError.  Everything else as chroma_cqt."""
    norm = _norm_arg(norm)
    taps = _smoothing_taps(win_len_smooth, smoothing_window)
    chroma = chroma_cqt(y=y, sr=sr, C=C, hop_length=hop_length, fmin=fmin, norm=None, tuning=tuning, n_chroma=n_chroma,
                        n_octaves=n_octaves, window=window, bins_per_octave=bins_per_octave, cqt_mode=cqt_mode)
    squeeze = chroma.ndim == 2
    out = _cens(chroma[None] if squeeze else chroma, taps, norm)
    return out[0] if squeeze else out


def tonnetz(*, y=None, sr: float = 22050, chroma=None, **kwargs):
    """Tonal centroid features (librosa.feature.tonnetz's signature): the chroma of every frame, L1-normalised, projected
    onto the six-dimensional basis of fifths, minor thirds and major thirds.  chroma: (n_chroma, T) or (batch, n_chroma,
    T), real; default chroma_cqt(y=y, sr=sr, **kwargs) (whose tuning defaults to 0.0 where librosa's is None).  Exactly
    one of y and chroma.  One launch of the fold kernel.  Returns float32 (6, T) or (batch, 6, T)."""
    _one_of(y, chroma, "chroma")
    if chroma is None:
        chroma = chroma_cqt(y=y, sr=sr, **kwargs)
    elif kwargs:
        raise ValueError(f"unexpected arguments with chroma given: {sorted(kwargs)}")
    x, squeeze = _spectrum(chroma, "chroma", allow_complex=False)
    n_chroma = int(x.shape[1])
    host = _cached_host(("phi", n_chroma), lambda: _finish(_phi64(n_chroma)))
    out = _fold(x, 0, host, pre_l1=True)
    return out[0] if squeeze else out


__all__ = ["chroma_filterbank", "cq_to_chroma", "chroma_stft", "chroma_cqt", "chroma_cens", "tonnetz"]
