"""Constant-Q and variable-Q transforms (no counterpart in the reference; the signatures of librosa 0.10's
librosa.cqt, librosa.vqt and librosa.cqt_frequencies).

One fused kernel (csrc/kernels_cqt.h) evaluates the filter bank in direct form: every band has its own
window length (97 to 11 685 samples at the defaults), the padding is computed as the samples are loaded, and every
coefficient is one sum of fused multiply-adds in a fixed order.

    r = 2^(1 / bins_per_octave);  f_k = fmin 2^(tuning / bins_per_octave) r^k;  alpha = (r^2 - 1) / (r^2 + 1)
    Q = filter_scale / alpha;  N_k = Q sr / (f_k + gamma / alpha)         (cqt: gamma = 0)
    m0_k = floor(-N_k / 2), m1_k = floor(N_k / 2), L_k = m1_k - m0_k
    g_k[m] = w[m - m0_k] exp(2 pi i f_k m / sr), w = get_window(window, L_k), normalised by `norm`
    C[k, t] = s_k sum_{m = m0_k}^{m1_k - 1} ypad[t hop_length + m] conj(g_k[m]),  s_k = sqrt(N_k) if scale else N_k

The bank is built on the host in float64, rounded once to float32 and cached per device.

Deviations from librosa, on purpose.  This is librosa's ideal filter bank evaluated exactly; librosa itself
approximates it by octave-wise downsampling and a sparsified frequency-domain basis, so the two agree only as far as
that approximation goes, and no parity with librosa's numbers is claimed.  Because nothing is decimated, hop_length
may be any integer >= 1, and res_type and sparsity are accepted (sparsity validated) but unused.  tuning=None
(librosa: estimate the tuning from the signal) and intervals other than "equal" raise ValueError; the output is
complex64.
"""

from __future__ import annotations

import hashlib
import math
from functools import lru_cache

import numpy as np
import torch

from . import _extension as _x
from .onset import _is_int

_C1 = 32.70319566257483            # note_to_hz("C1")

_device_bank_cache: dict[tuple, tuple] = {}


def _is_real(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def cqt_frequencies(n_bins: int, fmin: float, bins_per_octave: int = 12, tuning: float = 0.0) -> np.ndarray:
    """Centre frequencies of the bands, float64 (n_bins,): fmin 2^(tuning / bins_per_octave) 2^(k / bins_per_octave)."""
    if not _is_int(n_bins) or n_bins < 1:
        raise ValueError(f"n_bins must be a positive integer, got {n_bins!r}")
    if not _is_int(bins_per_octave) or bins_per_octave < 1:
        raise ValueError(f"bins_per_octave must be a positive integer, got {bins_per_octave!r}")
    if not _is_real(fmin) or not float(fmin) > 0.0 or not math.isfinite(float(fmin)):
        raise ValueError(f"fmin must be strictly positive, got {fmin!r}")
    if not _is_real(tuning) or not math.isfinite(float(tuning)):
        raise ValueError(f"tuning must be a finite number, got {tuning!r}")
    bpo = int(bins_per_octave)
    return float(fmin) * 2.0 ** (float(tuning) / bpo) * 2.0 ** (np.arange(int(n_bins), dtype=np.float64) / bpo)


def _window_host(window: str, n: int) -> np.ndarray:
    """The project's periodic window of n points as float64 values."""
    if not isinstance(window, str):
        raise TypeError(f"window must be a window name (every band has its own length), got {type(window).__name__}")
    name = window.lower()
    if name not in _x.WINDOW_KINDS:
        raise ValueError(f"Unknown window type: '{name}'. Supported: {', '.join(sorted(_x.WINDOW_KINDS))}")
    return _x.generate_window_host(name, int(n), True).astype(np.float64)


@lru_cache(maxsize=32)
def _enbw(window: str) -> float:
    """Equivalent noise bandwidth of the window in bins: 1.5 for hann, else from 1000 points."""
    if window.lower() in ("hann", "hanning"):
        return 1.5
    w = _window_host(window, 1000)
    return float(1000.0 * np.sum(w * w) / np.sum(np.abs(w)) ** 2)


def _lengths(sr, fmin, n_bins, bins_per_octave, tuning, filter_scale, gamma):
    """(f_k, N_k, m0_k, L_k, Q, alpha) in float64 / int64."""
    f = cqt_frequencies(n_bins, fmin, bins_per_octave, tuning)
    r2 = 2.0 ** (2.0 / bins_per_octave)
    alpha = (r2 - 1.0) / (r2 + 1.0)
    Q = float(filter_scale) / alpha
    N = Q * float(sr) / (f + float(gamma) / alpha)
    m0 = np.floor(-N / 2.0).astype(np.int64)
    m1 = np.floor(N / 2.0).astype(np.int64)
    return f, N, m0, m1 - m0, Q, alpha


@lru_cache(maxsize=32)
def _bank(sr, fmin, n_bins, bins_per_octave, tuning, filter_scale, norm, window, gamma, scale):
    """The packed bank on the host: (taps complex64 back to back, tap_offset int64 (n_bins + 1), m0 int32, s float32,
    sha256 of all four).  Read-only arrays."""
    f, N, m0, L, Q, _ = _lengths(sr, fmin, n_bins, bins_per_octave, tuning, filter_scale, gamma)
    if f[-1] * (1.0 + 0.5 * _enbw(window) / Q) > sr / 2.0:
        raise ValueError(f"n_bins={n_bins} from fmin={fmin} reaches {f[-1]:.6g} Hz: the top band's passband exceeds the "
                         f"Nyquist frequency sr / 2 = {sr / 2.0:.6g} Hz; reduce n_bins or fmin")
    cap = int(_x.lib().ap_cqt_max_taps())
    if int(L.max()) > cap or int(np.abs(m0).max()) > cap:
        raise ValueError(f"the longest filter has {int(L.max())} taps (sr={sr}, fmin={fmin}, filter_scale={filter_scale}), "
                         f"above the kernel's cap of {cap}; raise fmin or lower filter_scale")
    if int(L.min()) < 1:
        raise ValueError(f"the shortest filter has no tap (sr={sr}, fmin={fmin}, n_bins={n_bins}, filter_scale={filter_scale})")
    off = np.zeros(n_bins + 1, np.int64)
    off[1:] = np.cumsum(L)
    taps = np.empty(int(off[-1]), np.complex128)
    for k in range(n_bins):
        m = m0[k] + np.arange(L[k], dtype=np.float64)
        g = _window_host(window, int(L[k])) * np.exp(2j * np.pi * f[k] * m / sr)
        if norm == 1:
            g = g / np.abs(g).sum()
        elif norm == 2:
            g = g / math.sqrt(float((np.abs(g) ** 2).sum()))
        elif norm == np.inf:
            g = g / np.abs(g).max()
        taps[off[k]:off[k + 1]] = g
    taps = taps.astype(np.complex64)                    # the one rounding
    s = (np.sqrt(N) if scale else N).astype(np.float32)
    m0 = m0.astype(np.int32)
    digest = hashlib.sha256(taps.tobytes() + off.tobytes() + m0.tobytes() + s.tobytes()).digest()
    for a in (taps, off, m0, s):
        a.setflags(write=False)
    return taps, off, m0, s, digest


def _device_bank(host, dev):
    """The bank's four arrays on `dev`, cached under their content (bounded, oldest out first)."""
    taps, off, m0, s, digest = host
    key = (digest, str(dev))
    hit = _device_bank_cache.get(key)
    if hit is None:
        hit = (torch.from_numpy(taps.view(np.float32).copy()).to(dev), torch.from_numpy(off.copy()).to(dev),
               torch.from_numpy(m0.copy()).to(dev), torch.from_numpy(s.copy()).to(dev))
        if len(_device_bank_cache) >= 32:
            _device_bank_cache.pop(next(iter(_device_bank_cache)))
        _device_bank_cache[key] = hit
    return hit


def _parameters(sr, hop_length, fmin, n_bins, bins_per_octave, tuning, filter_scale, norm, sparsity, window, scale, pad_mode,
                dtype, gamma, intervals):
    """The validated arguments of _bank, plus the pad mode's code."""
    if intervals != "equal":
        raise ValueError(f"intervals: only 'equal' is implemented, got {intervals!r}")
    if tuning is None:
        raise ValueError("tuning=None (estimate the tuning from the signal) is not done here; pass "
                         "tuning=estimate_tuning(y=y, sr=sr, bins_per_octave=...) or a number of bins")
    if dtype is not None and dtype not in (np.complex64, torch.complex64, "complex64"):
        raise ValueError(f"dtype must be None or complex64, got {dtype!r}")
    if not _is_real(sr) or not float(sr) > 0.0 or not math.isfinite(float(sr)):
        raise ValueError(f"sr must be strictly positive, got {sr!r}")
    if not _is_int(hop_length) or hop_length < 1:
        raise ValueError(f"hop_length must be a positive integer, got {hop_length!r}")
    if hop_length > 2 ** 31 - 1:
        raise ValueError(f"hop_length must be below 2^31, got {hop_length!r}")
    if fmin is None:
        fmin = _C1
    if not _is_real(filter_scale) or not float(filter_scale) > 0.0 or not math.isfinite(float(filter_scale)):
        raise ValueError(f"filter_scale must be strictly positive, got {filter_scale!r}")
    if not _is_real(sparsity) or not 0.0 <= float(sparsity) < 1.0:
        raise ValueError(f"sparsity must lie in [0, 1), got {sparsity!r}")
    if norm is not None and (not _is_real(norm) or norm not in (1, 2, np.inf)):
        raise ValueError(f"norm must be 1, 2, inf or None, got {norm!r}")
    if gamma is not None and (not _is_real(gamma) or not float(gamma) >= 0.0 or not math.isfinite(float(gamma))):
        raise ValueError(f"gamma must be non-negative or None, got {gamma!r}")
    if pad_mode not in _x.PAD_MODES:
        raise ValueError(f"Unknown pad_mode: '{pad_mode}'. Supported: reflect, constant, edge")
    cqt_frequencies(n_bins, fmin, bins_per_octave, tuning)            # n_bins, fmin, bins_per_octave, tuning
    if not isinstance(window, str):
        raise TypeError(f"window must be a window name (every band has its own length), got {type(window).__name__}")
    bpo = int(bins_per_octave)
    if gamma is None:
        r2 = 2.0 ** (2.0 / bpo)
        gamma = (r2 - 1.0) / (r2 + 1.0) * 24.7 / 0.108
    norm = None if norm is None else (np.inf if norm == np.inf else int(norm))
    return (float(sr), float(fmin), int(n_bins), bpo, float(tuning), float(filter_scale), norm, window.lower(), float(gamma),
            bool(scale)), _x.PAD_MODES[pad_mode]


def _signal(y):
    """y as a (B, L) float32 device tensor, and whether it came as 1D.  Validation first, the device after."""
    from .mel import _is_pcm16, pcm16_to_float

    ndim = y.ndim if isinstance(y, (torch.Tensor, np.ndarray)) else np.ndim(y)
    if ndim not in (1, 2):
        raise ValueError(f"y must be 1D (samples,) or 2D (batch, samples), got {ndim}D")
    if isinstance(y, torch.Tensor) and y.is_complex() or isinstance(y, np.ndarray) and np.iscomplexobj(y):
        raise ValueError("y must be real")
    yd = pcm16_to_float(y) if _is_pcm16(y) else _x.to_device_f32(y)
    return (yd[None] if ndim == 1 else yd), ndim == 1


def _run(y, bank_args, pad_code, hop_length):
    n_bins = bank_args[2]
    host = _bank(*bank_args)
    shape = tuple(y.shape) if isinstance(y, (torch.Tensor, np.ndarray)) else np.shape(y)
    if len(shape) not in (1, 2):
        raise ValueError(f"y must be 1D (samples,) or 2D (batch, samples), got {len(shape)}D")
    L = int(shape[-1])
    if L < 1:
        raise ValueError("y must hold at least one sample")
    if L > 2 ** 30:
        raise ValueError(f"y must hold at most 2^30 samples, got {L}")
    m0, off = host[2].astype(np.int64), host[1]
    reach = int(max((-m0).max(), (m0 + np.diff(off)).max()))
    if pad_code == _x.PAD_MODES["reflect"] and reach > L - 1:
        raise ValueError(f"reflect padding requires the longest filter's half length ({reach}) <= signal_length - 1 ({L - 1})")
    yd, one_d = _signal(y)
    dev = yd.device
    B = yd.shape[0]
    T = 1 + L // int(hop_length)
    out = torch.empty((B, n_bins, T), dtype=torch.complex64, device=dev)
    if B:
        taps, offd, m0d, sd = _device_bank(host, dev)
        _x.check(_x.dlib(dev).ap_cqt_f32(_x.ptr(yd), B, L, int(hop_length), pad_code, _x.ptr(taps), _x.ptr(offd), _x.ptr(m0d),
                                         _x.ptr(sd), n_bins, T, _x.ptr(out), T, _x.stream_ptr(dev)))
    return out[0] if one_d else out


def cqt(y, *, sr: float = 22050, hop_length: int = 512, fmin=None, n_bins: int = 84, bins_per_octave: int = 12,
        tuning=0.0, filter_scale: float = 1, norm=1, sparsity: float = 0.01, window="hann", scale: bool = True,
        pad_mode: str = "constant", res_type="soxr_hq", dtype=None):
    """Constant-Q transform (librosa.cqt's signature; the module docstring has the definition).

    y: (samples,) or (batch, samples), float32 or int16 PCM (converted by pcm16_to_float).  fmin=None: C1 =
    32.70319566257483 Hz.  norm: 1, 2, inf or None.  pad_mode: constant, edge or reflect (reflect needs a clip longer
    than half the longest filter, as stft does for n_fft // 2).  hop_length: any integer >= 1.  Evaluated exactly in
    direct form: res_type and sparsity are accepted and unused; for tuning=None pass
    tuning=estimate_tuning(y=y, sr=sr, bins_per_octave=bins_per_octave).
    Returns complex64 (n_bins, T) or (batch, n_bins, T), T = 1 + samples // hop_length."""
    args, pad_code = _parameters(sr, hop_length, fmin, n_bins, bins_per_octave, tuning, filter_scale, norm, sparsity, window,
                                 scale, pad_mode, dtype, 0.0, "equal")
    return _run(y, args, pad_code, hop_length)


def vqt(y, *, sr: float = 22050, hop_length: int = 512, fmin=None, n_bins: int = 84, intervals="equal", gamma=None,
        bins_per_octave: int = 12, tuning=0.0, filter_scale: float = 1, norm=1, sparsity: float = 0.01, window="hann",
        scale: bool = True, pad_mode: str = "constant", res_type="soxr_hq", dtype=None):
    """Variable-Q transform (librosa.vqt's signature): cqt with N_k = Q sr / (f_k + gamma / alpha), which widens the
    low bands.  gamma=None: alpha 24.7 / 0.108 (the ERB slope); gamma=0 is cqt.  intervals: only "equal".  Everything
    else as cqt, evaluated exactly in direct form (res_type and sparsity accepted and unused)."""
    args, pad_code = _parameters(sr, hop_length, fmin, n_bins, bins_per_octave, tuning, filter_scale, norm, sparsity, window,
                                 scale, pad_mode, dtype, gamma, intervals)
    return _run(y, args, pad_code, hop_length)


__all__ = ["cqt", "vqt", "cqt_frequencies"]
