"""Autocorrelation, pitch_detect_acf, periodicity — same API as /root/reference/mlx_audio_primitives/pitch.py
(native mirror csrc/primitives/autocorrelation.cpp:10-84).

Wiener-Khinchin on the device: centre, zero-pad to the next power of two >= 2 n - 1, forward and
inverse four-step FFT (both legs LDS-resident, the transform ``resample(res_type="fft")`` uses),
|.|^2 in between, first max_lag lags, normalised by r[0].  The reference's Python path does the two
FFTs in NumPy on the host (pitch.py:88-99).

yin / yin_cmnd (no counterpart in the reference; librosa's signature): the YIN f0 tracker and its
cumulative-mean-normalised difference curve on the fused wave-per-frame kernel of csrc/kernels_yin.h
(frame_length 2048 / 1024) or its direct-sum general kernel.
"""

from __future__ import annotations

import ctypes

import torch

from . import _extension as _x
from .stft import _get_twiddles


def autocorrelation(y, max_lag: int | None = None, normalize: bool = True, center: bool = True) -> torch.Tensor:
    """r[k] = sum_n y[n] y[n + k] for k < max_lag (default: all n lags), (max_lag,) or (batch, max_lag)."""
    y = _x.to_device_f32(y)
    if y.ndim not in (1, 2):
        raise ValueError("signal must be 1-dimensional (samples,) or 2-dimensional (batch, samples)")
    one_d = y.ndim == 1
    if one_d:
        y = y[None, :]
    y = y.contiguous()
    B, n = y.shape
    if max_lag is None or max_lag <= 0:          # bindings.cpp: -1 = all lags
        max_lag = n
    max_lag = min(int(max_lag), n)
    dev = y.device
    out = torch.empty((B, max_lag), dtype=torch.float32, device=dev)
    if B > 0 and n > 0:
        lib = _x.lib()
        N = int(lib.ap_autocorrelation_nfft(n))
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        if lib.ap_cfft_split_host(N, ctypes.addressof(a), ctypes.addressof(b)) != 0:
            raise ValueError(f"autocorrelation: signals of {n} samples need a {N}-point transform, beyond "
                             "the on-chip four-step FFT (4096 x 4096)")
        tw1, tw2 = _get_twiddles(a.value, dev), _get_twiddles(b.value, dev)
        ws = torch.empty(4 * B * N + B, dtype=torch.float32, device=dev)
        _x.check(_x.dlib(dev).ap_autocorrelation_f32(_x.ptr(y), B, n, max_lag, int(bool(normalize)),
                                                     int(bool(center)), _x.ptr(tw1), _x.ptr(tw2), _x.ptr(ws),
                                                     _x.ptr(out), _x.stream_ptr(dev)))
    return out[0] if one_d else out


def _frame_acf_peaks(y, sr, fmin, fmax, frame_length, hop_length, threshold, center, want):
    """Shared body of pitch_detect_acf / periodicity (reference pitch.py:118-369): constant centre padding,
    frames, the raw autocorrelation of every centred frame on the device (the four-step FFT pair of
    `autocorrelation`), then one pass that picks the peak of r / r[0] in the lag range.  The reference walks
    the frames in a Python loop with two NumPy FFTs each."""
    from ._validation import validate_positive

    validate_positive(frame_length, "frame_length")
    validate_positive(hop_length, "hop_length")
    if want == "pitch" and fmin >= fmax:
        raise ValueError(f"fmin ({fmin}) must be less than fmax ({fmax})")
    min_lag, max_lag = int(sr / fmax), int(sr / fmin)
    y = _x.to_device_f32(y)
    one_d = y.ndim == 1
    if one_d:
        y = y[None, :]
    if y.ndim != 2:
        raise ValueError(f"y must be 1D or 2D, got {y.ndim}D")
    y = y.contiguous()
    B, L = y.shape
    dev = y.device
    pad = frame_length // 2 if center else 0
    Lp = L + 2 * pad
    T = 1 + (Lp - frame_length) // hop_length if Lp >= frame_length else 0
    f0 = torch.zeros((B, max(T, 0)), dtype=torch.float32, device=dev)
    voiced = torch.zeros((B, max(T, 0)), dtype=torch.uint8, device=dev)
    per = torch.zeros((B, max(T, 0)), dtype=torch.float32, device=dev)
    if B > 0 and T > 0:
        d = _x.dlib(dev)
        st = _x.stream_ptr(dev)
        yp = y
        if pad:
            yp = torch.empty((B, Lp), dtype=torch.float32, device=dev)
            _x.check(d.ap_pad_f32(_x.ptr(y), B, L, pad, _x.PAD_MODES["constant"], _x.ptr(yp), st))
        # Lags beyond the frame are treated as 0 here.  Deviation from the reference when sr / fmin >= frame_length
        # (e.g. frame_length = 1024, sr = 22050, fmin = 20): its r is the full n_fft-long irfft, so it then sees the
        # mirrored negative lags in r[frame_length:] and a slice cut at n_fft (pitch.py:189-214).  No fixture of the
        # reference covers that shape ("parity unpinned"); the search range inside the frame is identical.
        n_lag = min(max_lag + 1, frame_length)
        # one clip's frames at a time (a few clips per pass when they are short): bounded workspace
        per_pass = max(1, min(B, (1 << 15) // max(T, 1)))
        for b0 in range(0, B, per_pass):
            nb = min(per_pass, B - b0)
            frames = torch.empty((nb * T, frame_length), dtype=torch.float32, device=dev)
            _x.check(d.ap_frame_f32(_x.ptr(yp[b0:b0 + nb]), nb, Lp, int(frame_length), int(hop_length), _x.ptr(frames), st))
            r = autocorrelation(frames, max_lag=n_lag, normalize=False, center=True)
            _x.check(d.ap_acf_peaks_f32(_x.ptr(r), nb * T, n_lag, min_lag, max_lag, float(threshold), float(sr),
                                        _x.ptr(f0[b0:b0 + nb]), _x.ptr(voiced[b0:b0 + nb]), _x.ptr(per[b0:b0 + nb]), st))
    return f0, voiced.bool(), per, one_d


def pitch_detect_acf(y, sr: int = 22050, fmin: float = 50.0, fmax: float = 2000.0, frame_length: int = 2048,
                     hop_length: int = 512, threshold: float = 0.1, center: bool = True):
    """(f0, voiced_flag) per frame: f0 = sr / lag of the first local maximum above `threshold` of the normalised
    autocorrelation in [sr / fmax, sr / fmin] (reference pitch.py:118-264).  (n_frames,) or (batch, n_frames)."""
    f0, voiced, _, one_d = _frame_acf_peaks(y, sr, fmin, fmax, frame_length, hop_length, threshold, center, "pitch")
    return (f0[0], voiced[0]) if one_d else (f0, voiced)


def periodicity(y, sr: int = 22050, fmin: float = 50.0, fmax: float = 2000.0, frame_length: int = 2048,
                hop_length: int = 512, center: bool = True) -> torch.Tensor:
    """Largest normalised autocorrelation in the lag range per frame, (1, n_frames) or (batch, 1, n_frames)
    (reference pitch.py:267-369)."""
    _, _, per, one_d = _frame_acf_peaks(y, sr, fmin, fmax, frame_length, hop_length, 0.0, center, "periodicity")
    per = per[:, None, :]
    return per[0] if one_d else per


def _yin_setup(y, fmin, fmax, sr, frame_length, hop_length, center, pad_mode, who):
    """Validation, lag range and device input shared by yin / yin_cmnd: (y (B, L), one_d, lo, hi, hop, center)."""
    import math

    from ._validation import validate_positive

    validate_positive(sr, "sr")
    if not isinstance(frame_length, int) or frame_length % 2 or not 4 <= frame_length <= 8192:
        raise ValueError(f"frame_length must be even and in 4 .. 8192, got {frame_length}")
    if hop_length is None:
        hop_length = frame_length // 4
    validate_positive(hop_length, "hop_length")
    if fmin is None or fmax is None:
        raise ValueError("fmin and fmax must be provided")
    validate_positive(fmin, "fmin")
    if fmin >= fmax:
        raise ValueError(f"fmin ({fmin}) must be less than fmax ({fmax})")
    if pad_mode not in _x.PAD_MODES:
        raise ValueError(f"Unknown pad_mode '{pad_mode}'. Supported: constant, edge, reflect")
    lo = max(int(math.floor(sr / fmax)), 1)
    hi = min(int(math.ceil(sr / fmin)), frame_length - frame_length // 2 - 1)
    if lo >= hi:
        raise ValueError(f"{who}: no lags between sr / fmax and sr / fmin inside the frame (lo = {lo}, hi = {hi}); "
                         "lower fmin, raise fmax or use a longer frame_length")
    ndim, L = len(y.shape), (y.shape[-1] if len(y.shape) else 0)
    if ndim not in (1, 2):
        raise ValueError(f"y must be 1D or 2D, got {ndim}D")
    Lp = L + (2 * (frame_length // 2) if center else 0)
    if Lp < frame_length:
        raise ValueError(f"Signal length ({Lp}) must be >= frame_length ({frame_length}). Consider padding the signal.")
    y = _x.to_device_f32(y)
    one_d = y.ndim == 1
    if one_d:
        y = y[None, :]
    y = y.contiguous()
    if center and pad_mode != "constant":
        # edge / reflect: pad on the device, then frames without centring ("constant" needs no copy: samples
        # outside the clip read as 0 inside the kernels)
        pad = frame_length // 2
        yp = torch.empty((y.shape[0], L + 2 * pad), dtype=torch.float32, device=y.device)
        if y.shape[0] > 0:
            _x.check(_x.dlib(y.device).ap_pad_f32(_x.ptr(y), y.shape[0], L, pad, _x.PAD_MODES[pad_mode], _x.ptr(yp),
                                                  _x.stream_ptr(y.device)))
        y, center = yp, False
    return y, one_d, lo, hi, int(hop_length), bool(center)


def _yin_call(entry, y, frame_length, hop, args):
    """Run `entry` on the fused wave kernel where it serves the shape, else (or with AP_YIN_GENERAL=1) on the
    general kernel.  `args(tw)` builds the argument list."""
    import os

    dev = y.device
    d = _x.dlib(dev)
    fused = bool(_x.lib().ap_yin_fused(frame_length, hop, y.shape[1])) and os.environ.get("AP_YIN_GENERAL") != "1"
    rc = _x.AP_ERR_UNSUPPORTED
    if fused:
        rc = getattr(d, entry)(*args(_x.ptr(_get_twiddles(frame_length, dev))))
    if rc == _x.AP_ERR_UNSUPPORTED:
        rc = getattr(d, entry)(*args(None))
    _x.check(rc)


def yin(y, *, fmin, fmax, sr: float = 22050, frame_length: int = 2048, win_length: int | None = None,
        hop_length: int | None = None, trough_threshold: float = 0.1, center: bool = True,
        pad_mode: str = "constant", return_aperiodicity: bool = False):
    """Fundamental frequency per frame with YIN (de Cheveigne & Kawahara 2002), librosa's signature.

    On the cumulative-mean-normalised difference d' of every frame (`yin_cmnd`) over the lags
    floor(sr / fmax) .. ceil(sr / fmin): the first local minimum below `trough_threshold`, else the first global
    minimum, refined by a parabola; f0 = sr / lag.  (n_frames,) or (batch, n_frames) float32 Hz; with
    `return_aperiodicity` also d' at the chosen lag (the voicing measure: near 0 = periodic, near 1 = not).
    `win_length` is accepted for signature compatibility and must be None or frame_length // 2."""
    if win_length is not None and win_length != frame_length // 2:
        raise ValueError(f"win_length must be None or frame_length // 2 = {frame_length // 2}, got {win_length}")
    y, one_d, lo, hi, hop, center = _yin_setup(y, fmin, fmax, sr, frame_length, hop_length, center, pad_mode, "yin")
    B, L = y.shape
    T = 1 + (L + (2 * (frame_length // 2) if center else 0) - frame_length) // hop
    f0 = torch.empty((B, T), dtype=torch.float32, device=y.device)
    aper = torch.empty((B, T), dtype=torch.float32, device=y.device) if return_aperiodicity else None
    if B > 0:
        st = _x.stream_ptr(y.device)
        _yin_call("ap_yin_f32", y, frame_length, hop,
                  lambda tw: (_x.ptr(y), B, L, frame_length, hop, int(center), lo, hi, float(sr),
                              float(trough_threshold), tw, _x.ptr(f0), None if aper is None else _x.ptr(aper), st))
    if one_d:
        f0, aper = f0[0], (None if aper is None else aper[0])
    return (f0, aper) if return_aperiodicity else f0


def yin_cmnd(y, *, fmin, fmax, sr: float = 22050, frame_length: int = 2048, hop_length: int | None = None,
             center: bool = True, pad_mode: str = "constant") -> torch.Tensor:
    """YIN's cumulative-mean-normalised difference d'(tau) of every frame for the lags tau = floor(sr / fmax) ..
    ceil(sr / fmin) (clamped to the frame): (n_lags, n_frames) or (batch, n_lags, n_frames) float32.  The curve
    `yin` picks its troughs on, and the input of probabilistic trackers."""
    y, one_d, lo, hi, hop, center = _yin_setup(y, fmin, fmax, sr, frame_length, hop_length, center, pad_mode, "yin_cmnd")
    B, L = y.shape
    T = 1 + (L + (2 * (frame_length // 2) if center else 0) - frame_length) // hop
    out = torch.empty((B, hi - lo + 1, T), dtype=torch.float32, device=y.device)
    if B > 0:
        st = _x.stream_ptr(y.device)
        _yin_call("ap_yin_cmnd_f32", y, frame_length, hop,
                  lambda tw: (_x.ptr(y), B, L, frame_length, hop, int(center), lo, hi, tw, _x.ptr(out), st))
    return out[0] if one_d else out
