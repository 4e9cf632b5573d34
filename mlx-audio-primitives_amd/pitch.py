"""Autocorrelation, pitch_detect_acf, periodicity — same API as /root/reference/mlx_audio_primitives/pitch.py
(native mirror csrc/primitives/autocorrelation.cpp:10-84).

Wiener-Khinchin on the device: centre, zero-pad to the next power of two >= 2 n - 1, forward and
inverse four-step FFT (both legs LDS-resident, the transform ``resample(res_type="fft")`` uses),
|.|^2 in between, first max_lag lags, normalised by r[0].  The reference's Python path does the two
FFTs in NumPy on the host (pitch.py:88-99).

yin / yin_cmnd (no counterpart in the reference; librosa's signature): the YIN f0 tracker and its
cumulative-mean-normalised difference curve on the fused wave-per-frame kernel of csrc/kernels_yin.h
(frame_length 2048 / 1024) or its direct-sum general kernel.

piptrack / estimate_tuning / pitch_tuning (no counterpart in the reference; librosa's signatures): parabolically
interpolated STFT peaks on one kernel that reads stft's rows in place, and the tuning they favour from a compact
record buffer, an exact median by radix select and an integer histogram (csrc/kernels_piptrack.h).
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


# ---------------------------------------------------------------------------------------------------------------------
# piptrack / pitch_tuning / estimate_tuning (csrc/kernels_piptrack.h; librosa 0.10's signatures)
# ---------------------------------------------------------------------------------------------------------------------
_edges_cache: dict[tuple, torch.Tensor] = {}


def _bin_range(sr: float, n_fft: int, fmin: float, fmax: float, F: int):
    """(k_lo, k_hi): the bins with max(fmin, 0) <= k sr / n_fft < min(fmax, sr / 2), in float64, clipped to [0, F]."""
    import math

    lo, hi = max(float(fmin), 0.0), min(float(fmax), float(sr) / 2.0)
    if not lo < hi:
        raise ValueError(f"fmin ({fmin}) must be less than fmax ({fmax}) after clipping to [0, sr / 2]")

    def first_at_or_above(v):
        k = int(math.ceil(v * n_fft / float(sr)))
        while k > 0 and (k - 1) * float(sr) / n_fft >= v:
            k -= 1
        while k * float(sr) / n_fft < v:
            k += 1
        return min(max(k, 0), F)

    return first_at_or_above(lo), first_at_or_above(hi)


def _tuning_bins(resolution, bins_per_octave):
    """Validated (n_bins, float64 edges) of the residual histogram."""
    import math

    import numpy as np

    from .cqt import _is_real
    from .onset import _is_int

    if not _is_real(resolution) or not 0.0 < float(resolution) < 1.0:
        raise ValueError(f"resolution must lie in (0, 1), got {resolution!r}")
    if not _is_int(bins_per_octave) or bins_per_octave < 1:
        raise ValueError(f"bins_per_octave must be a positive integer, got {bins_per_octave!r}")
    n_bins = int(math.ceil(1.0 / float(resolution)))
    cap = int(_x.lib().ap_piptrack_max_bins())
    if n_bins > cap:
        raise ValueError(f"resolution={resolution!r} needs {n_bins} histogram bins, above the kernel's cap of {cap}")
    return n_bins, np.linspace(-0.5, 0.5, n_bins + 1)


def _device_edges(edges, dev) -> torch.Tensor:
    key = (len(edges), str(dev))
    hit = _edges_cache.get(key)
    if hit is None:
        hit = torch.from_numpy(edges.copy()).to(dev)
        if len(_edges_cache) >= 32:
            _edges_cache.pop(next(iter(_edges_cache)))
        _edges_cache[key] = hit
    return hit


def _piptrack_args(y, sr, S, n_fft, hop_length, fmin, fmax, threshold, ref):
    """Everything piptrack checks before the device is touched: (n_fft, hop_length, ref_mode, ref_value, ref array)."""
    import math

    import numpy as np

    from .chroma import _one_of, _sr_arg
    from .cqt import _is_real
    from .onset import _is_int

    _one_of(y, S, "S")
    sr = _sr_arg(sr)
    for name, v in (("fmin", fmin), ("fmax", fmax)):
        if not _is_real(v) or math.isnan(float(v)):
            raise ValueError(f"{name} must be a number, got {v!r}")
    if not _is_real(threshold) or not float(threshold) >= 0.0:
        raise ValueError(f"threshold must be non-negative, got {threshold!r}")
    ref_mode, ref_value, ref_arr = 0, 0.0, None
    if ref is not None:
        if callable(ref):
            if ref is not np.max:
                raise TypeError("ref: a callable other than numpy.max is not supported; pass None, a number or an array")
        elif _is_real(ref):
            if math.isnan(float(ref)):
                raise ValueError(f"ref must not be NaN, got {ref!r}")
            ref_mode, ref_value = 1, abs(float(ref))
        elif isinstance(ref, (torch.Tensor, np.ndarray, list, tuple)):
            ref_arr = ref if isinstance(ref, torch.Tensor) else torch.as_tensor(np.asarray(ref, dtype=np.float32))
            if ref_arr.is_complex() or ref_arr.ndim > 2:
                raise ValueError(f"ref must be real and broadcastable to (batch, frames), got shape {tuple(ref_arr.shape)}")
            ref_mode = 2
        else:
            raise TypeError(f"ref must be None, numpy.max, a number or an array, got {type(ref).__name__}")
    if S is None:
        if not _is_int(n_fft) or n_fft < 2:
            raise ValueError(f"n_fft must be an integer >= 2, got {n_fft!r}")
        if hop_length is not None and (not _is_int(hop_length) or hop_length < 1):
            raise ValueError(f"hop_length must be a positive integer or None, got {hop_length!r}")
    return sr, ref_mode, ref_value, ref_arr


def _piptrack_input(y, sr, S, n_fft, hop_length, fmin, fmax, win_length, window, center, pad_mode):
    """(x (B, F, T) float32 / complex64 on the device, was it 2D?, n_fft, k_lo, k_hi)."""
    from .chroma import _spectrum
    from .cqt import _signal

    if S is not None:
        shape = tuple(S.shape) if hasattr(S, "shape") else ()
        if len(shape) not in (2, 3):
            raise ValueError(f"S must be 2D (bins, frames) or 3D (batch, bins, frames), got {len(shape)}D")
        if shape[-2] < 2:
            raise ValueError(f"S must hold at least 2 frequency bins, got {shape[-2]}")
        n_fft = 2 * (shape[-2] - 1)
        k_lo, k_hi = _bin_range(sr, n_fft, fmin, fmax, shape[-2])
        x, squeeze = _spectrum(S, "S", allow_complex=True)
    else:
        from .stft import stft

        n_fft = int(n_fft)
        k_lo, k_hi = _bin_range(sr, n_fft, fmin, fmax, n_fft // 2 + 1)
        yd, squeeze = _signal(y)
        x = stft(yd, n_fft=n_fft, hop_length=None if hop_length is None else int(hop_length), win_length=win_length,
                 window=window, center=center, pad_mode=pad_mode)
    return x, squeeze, n_fft, k_lo, k_hi


def _rows_any(x: torch.Tensor):
    """(tensor, row stride in elements, in_kind) of a (B, F, T) float32 / complex64 device tensor, kept in place when
    its rows are dense or padded (onset._rows)."""
    from .onset import _rows

    xr, rs = _rows(x)
    return xr, rs, int(x.is_complex())


def _ref_on_device(ref_arr, B, T, dev):
    if ref_arr is None:
        return None
    r = ref_arr.to(device=dev, dtype=torch.float32)
    try:
        r = torch.broadcast_to(r, (B, T))
    except RuntimeError:
        raise ValueError(f"ref of shape {tuple(ref_arr.shape)} is not broadcastable to (batch, frames) = ({B}, {T})") from None
    return r.contiguous()


def piptrack(*, y=None, sr: float = 22050, S=None, n_fft: int = 2048, hop_length=None, fmin: float = 150.0,
             fmax: float = 4000.0, threshold: float = 0.1, win_length=None, window="hann", center: bool = True,
             pad_mode: str = "constant", ref=None):
    """Pitch tracking on thresholded, parabolically interpolated STFT peaks (librosa.piptrack's signature).

    y: (samples,) or (batch, samples), float32 or int16 PCM: stft(y), whose (line-padded) complex rows the peak kernel
    reads in place.  S: a magnitude spectrogram (F, T) or (batch, F, T) instead, real (taken as the magnitude) or complex
    (|z| is taken on load); n_fft is then 2 (F - 1).  Exactly one of y and S.  hop_length=None: n_fft // 4.  A bin k with
    max(fmin, 0) <= k sr / n_fft < min(fmax, sr / 2) is a peak when its thresholded magnitude exceeds the bin below and
    is not below the bin above; the threshold is `threshold` times the frame's maximum (ref=None or numpy.max), |ref|
    for a number, or |ref| per frame for an array broadcastable to (batch, frames).  Returns (pitches, magnitudes),
    float32 (F, T) or (batch, F, T) on the input's device and current stream: the interpolated frequency in Hz and the
    interpolated magnitude at the peaks, zero elsewhere.  The definition is DESIGN.md 9.10 / tests/piptrack_ref.py."""
    import numpy as np

    sr, ref_mode, ref_value, ref_arr = _piptrack_args(y, sr, S, n_fft, hop_length, fmin, fmax, threshold, ref)
    x, squeeze, n_fft, k_lo, k_hi = _piptrack_input(y, sr, S, n_fft, hop_length, fmin, fmax, win_length, window, center, pad_mode)
    B, F, T = x.shape
    dev = x.device
    pitches = torch.empty((B, F, T), dtype=torch.float32, device=dev)
    mags = torch.empty((B, F, T), dtype=torch.float32, device=dev)
    if B and T:
        xr, rs, kind = _rows_any(x)
        rd = _ref_on_device(ref_arr, B, T, dev)
        _x.check(_x.dlib(dev).ap_piptrack_f32(_x.ptr(xr), kind, B, F, T, rs, k_lo, k_hi, float(threshold), ref_mode, ref_value,
                                              None if rd is None else _x.ptr(rd), float(np.float32(sr / n_fft)), _x.ptr(pitches),
                                              _x.ptr(mags), T, _x.stream_ptr(dev)))
    return (pitches[0], mags[0]) if squeeze else (pitches, mags)


def _pick_tuning(counts, edges) -> float:
    """edges[argmax(counts)], the first maximum winning."""
    import numpy as np

    return float(edges[int(np.argmax(counts))])


def _warn_no_pitch():
    import warnings

    warnings.warn("Trying to estimate tuning from empty frequency set.", UserWarning, stacklevel=3)


def pitch_tuning(frequencies, *, resolution: float = 0.01, bins_per_octave: int = 12) -> float:
    """The tuning deviation (in fractions of a bin, in [-0.5, 0.5)) that the frequencies favour (librosa.pitch_tuning):
    the left edge of the fullest bin of the histogram of r = bins_per_octave log2(f / 27.5) mod 1, taken into
    [-0.5, 0.5), over ceil(1 / resolution) equal bins; r is computed in float64 from the float32 f > 0, the counts are
    integers (one kernel; the argmax and the edges stay on the host).  frequencies: any tensor or array, on the host or
    the device.  No positive frequency gives a UserWarning and 0.0."""
    import numpy as np

    n_bins, edges = _tuning_bins(resolution, bins_per_octave)
    f = frequencies if isinstance(frequencies, torch.Tensor) else torch.as_tensor(np.asarray(frequencies, dtype=np.float32))
    if f.is_complex():
        raise ValueError("frequencies must be real")
    if f.numel() == 0:
        _warn_no_pitch()
        return 0.0
    f = _x.to_device_f32(f).reshape(-1)
    dev = f.device
    counts = torch.empty(n_bins, dtype=torch.int64, device=dev)
    _x.check(_x.dlib(dev).ap_pitch_hist_f32(_x.ptr(f), f.numel(), float(bins_per_octave), _x.ptr(_device_edges(edges, dev)), n_bins,
                                            _x.ptr(counts), _x.stream_ptr(dev)))
    counts = counts.cpu().numpy()
    if not counts.any():
        _warn_no_pitch()
        return 0.0
    return _pick_tuning(counts, edges)


def _tuning_records(x, k_lo, k_hi, threshold, ref_mode, ref_value, ref_arr, bin_hz, per_clip, n_bins, edges, bins_per_octave,
                    capacity):
    """(number of peaks, median magnitude, counts, runs) with the first three per group as host arrays (G,), (G,),
    (G, n_bins): the compact peak kernel and the selection kernel, run again with the exact capacity when the first
    guess was too small; runs is 1 or 2."""
    B, F, T = x.shape
    dev = x.device
    G = B if per_clip else 1
    xr, rs, kind = _rows_any(x)
    rd = _ref_on_device(ref_arr, B, T, dev)
    cap_max = int(_x.lib().ap_piptrack_max_records())
    if capacity is None:
        capacity = max(1024, -(-(B // G) * F * T // 16))              # peaks are 1 to 2 % of the bins on tonal input
    capacity = min(int(capacity), cap_max)
    d, st = _x.dlib(dev), _x.stream_ptr(dev)
    de = _device_edges(edges, dev)
    counters = torch.empty(G, dtype=torch.int64, device=dev)
    thr = torch.empty(G, dtype=torch.float32, device=dev)
    counts = torch.empty((G, n_bins), dtype=torch.int64, device=dev)
    for attempt in range(2):
        records = torch.empty((G, capacity, 2), dtype=torch.float32, device=dev)
        _x.check(d.ap_piptrack_records_f32(_x.ptr(xr), kind, B, F, T, rs, k_lo, k_hi, float(threshold), ref_mode, ref_value,
                                           None if rd is None else _x.ptr(rd), bin_hz, int(per_clip), _x.ptr(records), capacity,
                                           _x.ptr(counters), st))
        _x.check(d.ap_piptrack_tuning_f32(_x.ptr(records), _x.ptr(counters), G, capacity, float(bins_per_octave), _x.ptr(de), n_bins,
                                          _x.ptr(thr), _x.ptr(counts), st))
        n = counters.cpu().numpy()
        need = int(n.max())
        if need <= capacity:
            return n, thr.cpu().numpy(), counts.cpu().numpy(), attempt + 1
        if need > cap_max:
            raise ValueError(f"estimate_tuning: {need} peaks in one group, above the kernel's cap of {cap_max}; use per_clip=True "
                             "or a smaller batch")
        capacity = need
    raise RuntimeError("estimate_tuning: the peak count changed between two runs on the same input")


def estimate_tuning(*, y=None, sr: float = 22050, S=None, n_fft: int = 2048, resolution: float = 0.01,
                    bins_per_octave: int = 12, **kwargs):
    """The tuning deviation of a signal or spectrogram in fractions of a bin (librosa.estimate_tuning's signature):
    pitch_tuning of the piptrack peaks whose magnitude is at least the median peak magnitude.  y, S, n_fft and
    **kwargs (hop_length, fmin, fmax, threshold, win_length, window, center, pad_mode, ref) are piptrack's.  Returns one
    Python float over the whole input, batched or not, as librosa does; per_clip=True with batched input returns a
    float64 array (batch,), every clip with its own median and histogram.  Nothing dense is written: the peak kernel
    leaves (magnitude, pitch) records, a second kernel selects the median exactly and counts the residuals (DESIGN.md
    9.10).  Pass the result on as `tuning=` to cqt / chroma_stft / chroma_cqt (in their bins_per_octave / n_chroma)."""
    import numpy as np

    per_clip = kwargs.pop("per_clip", False)
    capacity = kwargs.pop("_capacity", None)
    allowed = ("hop_length", "fmin", "fmax", "threshold", "win_length", "window", "center", "pad_mode", "ref")
    unknown = sorted(k for k in kwargs if k not in allowed)
    if unknown:
        raise TypeError(f"estimate_tuning got unexpected keyword arguments {unknown}; piptrack's are {list(allowed)}")
    if not isinstance(per_clip, (bool, np.bool_)):
        raise ValueError(f"per_clip must be a bool, got {per_clip!r}")
    if capacity is not None and (not isinstance(capacity, int) or capacity < 1):
        raise ValueError(f"_capacity must be a positive integer, got {capacity!r}")
    kw = dict(hop_length=None, fmin=150.0, fmax=4000.0, threshold=0.1, win_length=None, window="hann", center=True,
              pad_mode="constant", ref=None)
    kw.update(kwargs)
    sr, ref_mode, ref_value, ref_arr = _piptrack_args(y, sr, S, n_fft, kw["hop_length"], kw["fmin"], kw["fmax"], kw["threshold"],
                                                      kw["ref"])
    n_bins, edges = _tuning_bins(resolution, bins_per_octave)
    x, squeeze, n_fft, k_lo, k_hi = _piptrack_input(y, sr, S, n_fft, kw["hop_length"], kw["fmin"], kw["fmax"], kw["win_length"],
                                                    kw["window"], kw["center"], kw["pad_mode"])
    B, F, T = x.shape
    per_clip = bool(per_clip) and not squeeze
    if B == 0 or T == 0:
        n, counts = np.zeros(B if per_clip else 1, np.int64), np.zeros((B if per_clip else 1, n_bins), np.int64)
    else:
        n, _, counts, _ = _tuning_records(x, k_lo, k_hi, kw["threshold"], ref_mode, ref_value, ref_arr,
                                          float(np.float32(sr / n_fft)), per_clip, n_bins, edges, bins_per_octave, capacity)
    out = np.array([_pick_tuning(counts[g], edges) if n[g] > 0 else 0.0 for g in range(len(n))], np.float64)
    if (n == 0).any():
        _warn_no_pitch()
    return out if per_clip else float(out[0])
