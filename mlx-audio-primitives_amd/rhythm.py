"""Tempogram, tempo and beat tracking on the onset envelope (no counterpart in the reference; the signatures of
librosa.feature.tempogram, librosa.feature.tempo, librosa.beat.beat_track and librosa.tempo_frequencies).

tempogram is the windowed autocorrelation of the envelope per frame (csrc/kernels_rhythm.h): win_length
<= 512 on a wave-per-frame kernel (two on-chip 1024-point transforms per frame), any win_length up to 8192 on a
direct-sum kernel (AP_TEMPOGRAM_GENERAL=1 forces it); the linear ramps that pad a centred envelope are computed as the
kernels load, so no padded copy is written.  tempo picks, per
clip or per frame, the lag that maximises log1p(1e6 g) + a log-normal prior; from an envelope and with the mean the
tempogram kernel leaves the sums over its 64-frame tiles only and the tempogram never reaches memory.  beat_track is
Ellis' dynamic programme, one workgroup per row in one launch; without bpm= its period is the lag index the pick left
on the device, so nothing is read back in between.

Deviations from librosa, on purpose: the trim keeps the last beat above the threshold (librosa 0.10.0 drops it: its
slice ends before it); a beat period below 2 frames is a ValueError (librosa's window is ill-defined there); a row that
yields no beats reports tempo 0.0; norms other than inf / None, aggregates other than the mean / None and a per-frame
bpm are not implemented (NotImplementedError); non-negativity / finiteness of the envelope is not checked by tempogram
and tempo.
"""

from __future__ import annotations

import os

import numpy as np
import torch

from . import _extension as _x
from .stft import _get_twiddles
from .onset import _UNITS, _envelope, _is_int, onset_strength
from .windows import get_window


def tempo_frequencies(n_bins: int, *, hop_length: int = 512, sr: float = 22050) -> np.ndarray:
    """Tempo (beats per minute) of every lag bin of a tempogram: bpm[0] = inf, bpm[k] = 60 sr / (hop_length k).
    (n_bins,) float64, on the host."""
    if not _is_int(n_bins) or n_bins < 0:
        raise ValueError(f"n_bins must be a non-negative integer, got {n_bins!r}")
    bpm = np.full(int(n_bins), np.inf, np.float64)
    if n_bins > 1:
        bpm[1:] = 60.0 * float(sr) / (float(hop_length) * np.arange(1.0, int(n_bins)))
    return bpm


def _check_rate(sr, hop_length):
    if isinstance(sr, bool) or not isinstance(sr, (int, float, np.integer, np.floating)) or not float(sr) > 0.0:
        raise ValueError(f"sr must be a positive number, got {sr!r}")
    if not _is_int(hop_length) or hop_length < 1:
        raise ValueError(f"hop_length must be a positive integer, got {hop_length!r}")


def _window(window, W: int, dev) -> torch.Tensor:
    """The (W,) float32 window on `dev`: a name the library builds (float64 on the host, windows.py), an array of
    length W, or any other scipy.signal.get_window specification where SciPy is installed."""
    if isinstance(window, (torch.Tensor, np.ndarray, list)):
        w = torch.as_tensor(np.asarray(window) if isinstance(window, list) else window)
        if w.ndim != 1 or w.shape[0] != W:
            raise ValueError(f"Window array length ({tuple(w.shape)}) must match win_length ({W})")
        return w.to(device=dev, dtype=torch.float32).contiguous()
    if isinstance(window, str) and window.lower() in _x.WINDOW_KINDS:
        if W == 1:                                   # a window of one sample is 1 (scipy.signal.get_window)
            return torch.ones(1, dtype=torch.float32, device=dev)
        return get_window(window, W, fftbins=True, device=dev)
    if isinstance(window, (str, tuple, float, int)) and not isinstance(window, bool):
        try:
            from scipy.signal import get_window as _scipy_window
        except ImportError as e:
            raise ValueError(f"window {window!r} is not one the library builds ({', '.join(sorted(_x.WINDOW_KINDS))}) "
                             "and SciPy is not installed") from e
        return torch.from_numpy(np.asarray(_scipy_window(window, W, fftbins=True), np.float32)).to(dev)
    raise TypeError(f"window must be a name, a tuple or an array, got {type(window).__name__}")


def _env_rows(onset_envelope, y, sr, hop_length):
    """The validated envelope as ((B, n) float32 device tensor, row stride, was it 1D?): a device tensor whose rows are
    dense or a fixed stride apart stays where it is."""
    if onset_envelope is None:
        if y is None:
            raise ValueError("either y or onset_envelope must be given")
        onset_envelope = onset_strength(y=y, sr=sr, hop_length=hop_length)
    e = _envelope(onset_envelope, "onset_envelope")
    dev = e.device if e.is_cuda else _x.require_device()
    _x.lib()
    one_d = e.ndim == 1
    if not (e.is_cuda and e.dtype == torch.float32):
        e = e.to(device=dev, dtype=torch.float32)
    if one_d:
        e = e[None]
    B, n = e.shape
    if B * n and (n == 1 or e.stride(1) == 1) and (B == 1 or e.stride(0) >= n):
        return e, int(e.stride(0)) if B > 1 else n, one_d
    return e.contiguous(), n, one_d


def _tempogram(e, rs, W, center, window, norm, want_out, want_agg):
    """One ap_tempogram_f32 call on (B, n) rows: (tg (B, W, T) or None, tile sums (B, n_tiles, W) or None, T)."""
    B, n = e.shape
    dev = e.device
    if W > int(_x.lib().ap_tempogram_max_win()):
        raise ValueError(f"win_length beyond {int(_x.lib().ap_tempogram_max_win())} is not supported, got {W}")
    T = n if center else n - W + 1
    if n == 0 or T <= 0:
        if not center and n < W:
            raise ValueError(f"the envelope ({n} frames) is shorter than win_length ({W})")
        raise ValueError("the envelope must be non-empty")
    w = _window(window, W, dev)
    out = torch.empty((B, W, T), dtype=torch.float32, device=dev) if want_out else None
    agg = None
    if want_agg:
        agg = torch.empty(int(_x.lib().ap_tempogram_agg_floats(B, n, W, int(center))), dtype=torch.float32,
                          device=dev).view(B, -1, W)
    if B:
        # the wave-per-frame kernel where it serves win_length, else (or with AP_TEMPOGRAM_GENERAL=1) the general one
        d = _x.dlib(dev)
        args = (None if out is None else _x.ptr(out), None if agg is None else _x.ptr(agg), _x.stream_ptr(dev))
        rc = _x.AP_ERR_UNSUPPORTED
        if _x.lib().ap_tempogram_fused(W) and os.environ.get("AP_TEMPOGRAM_GENERAL") != "1":
            rc = d.ap_tempogram_f32(_x.ptr(e), B, n, rs, _x.ptr(w), W, int(center), int(norm), _x.ptr(_get_twiddles(1024, dev)), *args)
        if rc == _x.AP_ERR_UNSUPPORTED:
            rc = d.ap_tempogram_f32(_x.ptr(e), B, n, rs, _x.ptr(w), W, int(center), int(norm), None, *args)
        _x.check(rc)
    return out, agg, T


def _norm_flag(norm):
    if norm is None:
        return 0
    if isinstance(norm, (int, float, np.integer, np.floating)) and not isinstance(norm, bool) and norm == np.inf:
        return 1
    raise NotImplementedError("norm: only np.inf and None are implemented")


def tempogram(*, y=None, sr: float = 22050, onset_envelope=None, hop_length: int = 512, win_length: int = 384,
              center: bool = True, window="hann", norm=np.inf):
    """Autocorrelation tempogram (librosa.feature.tempogram).

    onset_envelope: (n,) or (batch, n) float32, rows dense or a fixed stride apart, used in place; without it
    onset_strength(y=y, sr=sr, hop_length=hop_length).  With W = win_length, h = W // 2,
    p = np.pad(e, h, mode="linear_ramp", end_values=0) and T = n (center) or p = e and T = n - W + 1, and
    w = get_window(window, W, fftbins=True):

        x_t[i]   = w[i] p[t + i]
        ac[k, t] = sum_{i < W - k} x_t[i] x_t[i + k]
        tg[k, t] = ac[k, t] / max_k |ac[k, t]|          (norm=np.inf; left alone where the maximum is below FLT_MIN)

    norm=None returns ac.  (W, T) or (batch, W, T) float32."""
    _check_rate(sr, hop_length)
    if not _is_int(win_length) or win_length < 1:
        raise ValueError(f"win_length must be a positive integer, got {win_length!r}")
    flag = _norm_flag(norm)
    e, rs, one_d = _env_rows(onset_envelope, y, sr, hop_length)
    out, _, _ = _tempogram(e, rs, int(win_length), bool(center), window, flag, True, False)
    return out[0] if one_d else out


def _log_prior(W, sr, hop_length, start_bpm, std_bpm, max_tempo, prior) -> np.ndarray:
    """(W,) float64: the log-normal prior over tempo_frequencies(W) (or prior.logpdf of them), -inf at lag 0 and at
    every lag before the first one slower than max_tempo."""
    bpm = tempo_frequencies(W, hop_length=hop_length, sr=sr)
    if prior is None:
        if not float(start_bpm) > 0.0:
            raise ValueError(f"start_bpm must be strictly positive, got {start_bpm!r}")
        if not float(std_bpm) > 0.0:
            raise ValueError(f"std_bpm must be strictly positive, got {std_bpm!r}")
        with np.errstate(divide="ignore", invalid="ignore"):
            lp = -0.5 * ((np.log2(bpm) - np.log2(float(start_bpm))) / float(std_bpm)) ** 2
    else:
        if not hasattr(prior, "logpdf"):
            raise TypeError("prior must have a logpdf method (e.g. a frozen scipy.stats distribution)")
        lp = np.array(prior.logpdf(bpm), dtype=np.float64).reshape(W)
    if max_tempo is not None:
        lp[:int(np.argmax(bpm < float(max_tempo)))] = -np.inf
    if W:
        lp[0] = -np.inf
    return lp


_table_cache: dict[tuple, torch.Tensor] = {}


def _cached(key, build):
    """Small host-built tables (the prior, the bpm table) once per device, as windows.py keeps its windows."""
    hit = _table_cache.get(key)
    if hit is None:
        if len(_table_cache) >= 64:
            _table_cache.clear()
        hit = _table_cache[key] = build()
    return hit


def _prior_on_device(W, sr, hop_length, start_bpm, std_bpm, max_tempo, prior, dev) -> torch.Tensor:
    def build():
        return torch.from_numpy(_log_prior(W, sr, hop_length, start_bpm, std_bpm, max_tempo, prior).astype(np.float32)).to(dev)
    if prior is not None:                        # an object of the caller's: not cached
        return build()
    return _cached(("prior", W, float(sr), int(hop_length), float(start_bpm), float(std_bpm),
                    None if max_tempo is None else float(max_tempo), str(dev)), build)


def _bpm_on_device(W, sr, hop_length, dev) -> torch.Tensor:
    return _cached(("bpm", W, float(sr), int(hop_length), str(dev)),
                   lambda: torch.from_numpy(tempo_frequencies(W, hop_length=hop_length, sr=sr)).to(dev))


def _window_length(ac_size, sr, hop_length) -> int:
    return int(np.floor(float(ac_size) * float(sr) / float(hop_length)))


def _tempo_index(e, rs, tg, sr, hop_length, start_bpm, std_bpm, ac_size, max_tempo, per_frame, prior):
    """(lag indices (B, n_col) int32 on the device, bpm table (W,) float64 on the device) from envelope rows or from a
    (B, W, T) tempogram."""
    if tg is None:
        W = _window_length(ac_size, sr, hop_length)
        if W < 1:
            raise ValueError(f"ac_size * sr / hop_length must be at least 1 frame, got {ac_size!r}")
        B = e.shape[0]
        dev = e.device
        stored, agg, T = _tempogram(e, rs, W, True, "hann", 1, per_frame, not per_frame)
    else:
        B, W, T = tg.shape
        dev = tg.device
        stored, agg = tg, None
        if W < 1 or T < 1:
            raise ValueError(f"tg must be non-empty, got {tuple(tg.shape)}")
    lp = _prior_on_device(W, sr, hop_length, start_bpm, std_bpm, max_tempo, prior, dev)
    n_col = T if per_frame else 1
    idx = torch.empty((B, n_col), dtype=torch.int32, device=dev)
    if B:
        if agg is not None:
            nt = agg.shape[1]
            args = (_x.ptr(agg), B, 1, W, nt * W, 1, 0, nt, W, float(T))
        elif per_frame:
            args = (_x.ptr(stored), B, T, W, W * T, T, 1, 1, 0, 1.0)
        else:
            args = (_x.ptr(stored), B, 1, W, W * T, T, 0, T, 1, float(T))
        _x.check(_x.dlib(dev).ap_tempo_pick_f32(*args, _x.ptr(lp), _x.ptr(idx), _x.stream_ptr(dev)))
    return idx, _bpm_on_device(W, sr, hop_length, dev)


def _aggregate_flag(aggregate) -> bool:
    """per_frame?"""
    if aggregate is None:
        return True
    if aggregate in (np.mean, torch.mean):
        return False
    raise NotImplementedError("aggregate: only the mean (np.mean, torch.mean) and None are implemented")


def tempo(*, y=None, sr: float = 22050, onset_envelope=None, tg=None, hop_length: int = 512, start_bpm: float = 120,
          std_bpm: float = 1.0, ac_size: float = 8.0, max_tempo: float | None = 320.0, aggregate=np.mean, prior=None):
    """Tempo in beats per minute (librosa.feature.tempo).

    tg: a tempogram (W, T) or (batch, W, T); without it the tempogram of the envelope (onset_envelope, or
    onset_strength(y=y)) with win_length = floor(ac_size sr / hop_length), centred, hann, max-normalised.  With
    g[k] = mean_t tg[k, t] (aggregate = np.mean: one value per clip) or g[k] = tg[k, t] (aggregate=None: one per
    frame): the first lag k that maximises log1p(1e6 g[k]) + logprior[k], as 60 sr / (hop_length k), where logprior
    is -0.5 ((log2 bpm - log2 start_bpm) / std_bpm)^2 or prior.logpdf(bpm), and -inf for lag 0 and every lag faster
    than max_tempo.  Defined for non-negative envelopes.  float64 on the device: (1,) / (batch, 1), or (T,) /
    (batch, T) with aggregate=None.  From an envelope and with the mean the tempogram is never stored."""
    _check_rate(sr, hop_length)
    per_frame = _aggregate_flag(aggregate)
    if tg is not None:
        if not isinstance(tg, torch.Tensor):
            tg = torch.as_tensor(np.asarray(tg))
        if tg.ndim not in (2, 3) or tg.is_complex():
            raise ValueError(f"tg must be a real (W, T) or (batch, W, T) array, got {tuple(tg.shape)}")
        one_d = tg.ndim == 2
        dev = tg.device if tg.is_cuda else _x.require_device()
        _x.lib()
        tg = tg.to(device=dev, dtype=torch.float32)
        tg = (tg[None] if one_d else tg).contiguous()
        e = rs = None
    else:
        e, rs, one_d = _env_rows(onset_envelope, y, sr, hop_length)
    idx, bpm = _tempo_index(e, rs, tg, sr, hop_length, start_bpm, std_bpm, ac_size, max_tempo, per_frame, prior)
    out = bpm[idx.long()]
    return out[0] if one_d else out


def _periods(bpm, B, one_d, sr, hop_length) -> np.ndarray:
    """(B,) int32 beat periods of bpm= (a scalar or one value per row): rint(60 (sr / hop_length) / bpm)."""
    v = np.asarray(bpm.detach().cpu().numpy() if isinstance(bpm, torch.Tensor) else bpm, dtype=np.float64)
    if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != 1 and (one_d or v.shape[0] != B)):
        raise NotImplementedError("bpm: a scalar or one value per row; a tempo per frame is not implemented")
    v = np.broadcast_to(v.reshape(-1), (B,)).astype(np.float64)
    if not (np.isfinite(v).all() and (v > 0).all()):
        raise ValueError(f"bpm must be strictly positive, got {bpm!r}")
    P = np.rint(60.0 * (float(sr) / float(hop_length)) / v)
    limit = int(_x.lib().ap_beat_track_max_period())
    if (P < 2).any():
        raise ValueError(f"bpm = {float(v[np.argmin(P)])} is a beat period of {int(P.min())} frames; at least 2 are needed "
                         "(lower hop_length)")
    if (P > limit).any():
        raise ValueError(f"beat periods beyond {limit} frames are not supported, got {int(P.max())}")
    return P.astype(np.int32)


def beat_track(*, y=None, sr: float = 22050, onset_envelope=None, hop_length: int = 512, start_bpm: float = 120.0,
               tightness: float = 100, trim: bool = True, bpm=None, prior=None, units: str = "frames",
               sparse: bool = True):
    """Beat tracking by dynamic programming (librosa.beat.beat_track; Ellis 2007).  Returns (tempo, beats).

    The envelope o is the one given or onset_strength(y=y, sr=sr, hop_length=hop_length), (T,) or (batch, T) with
    T <= 16384.  The period P of a row is rint(60 (sr / hop_length) / bpm) for bpm= (a scalar or one value per row),
    else the lag tempo() picks, which stays on the device.  With h = rint(P / 2) (halves to even), per row:

        o'[i]   = o[i] / std(o, ddof=1)
        L[i]    = sum_{k=-P..P} exp(-0.5 (32 k / P)^2) o'[i - k]
        C[i]    = L[i] + max_{d = 2P .. h} (-tightness ln(d / P)^2 + C[i - d]),   C[j] = 0 for j < 0
        link[i] = i - d of the first maximum (the largest d on a tie); -1 before the first L[j] >= 0.01 max(L)
        tail    = the last local maximum of C with 2 C[i] > the median of C over its local maxima
        beats   = tail, link[tail], ... reversed, trimmed at both ends to s[j] > 0.5 rms(s) (trim; else > 0),
                  s = L at the beats smoothed by hann(5)

    A row that is all zero, constant, holds a non-finite value or has T < 2 yields no beats; a row without beats has
    tempo 0.0.  Deviations from librosa: the last beat above the trim threshold is kept (librosa 0.10.0 drops it), and
    a period below 2 frames is a ValueError.  tempo: float64 () or (batch,) on the device.  beats: units "frames",
    "samples" or "time" (sparse=True, 1D input only: the indices), or with sparse=False a bool tensor of the
    envelope's shape.  Without bpm= the call ends with one small synchronising readback (the per-row counts, to report
    a period outside 2 .. 2048 frames); with bpm= and sparse=False nothing is read back."""
    _check_rate(sr, hop_length)
    if units not in _UNITS:
        raise ValueError(f"units must be one of {_UNITS}, got {units!r}")
    if units != "frames" and not sparse:
        raise ValueError(f"units={units!r} needs sparse=True")
    if isinstance(tightness, bool) or not isinstance(tightness, (int, float, np.integer, np.floating)) or not float(tightness) > 0.0:
        raise ValueError(f"tightness must be strictly positive, got {tightness!r}")
    if onset_envelope is None:
        if y is None:
            raise ValueError("either y or onset_envelope must be given")
        ndim = len(np.shape(y)) if not isinstance(y, torch.Tensor) else y.ndim
        if sparse and ndim != 1:
            raise ValueError("sparse=True needs 1D input; use sparse=False for a batch")
        onset_envelope = onset_strength(y=y, sr=sr, hop_length=hop_length)
    env = _envelope(onset_envelope, "onset_envelope")
    if sparse and env.ndim != 1:
        raise ValueError("sparse=True needs 1D input; use sparse=False for a batch")
    one_d = env.ndim == 1
    B, T = (1, env.shape[0]) if one_d else tuple(env.shape)
    limit = int(_x.lib().ap_beat_track_max_frames())
    if T > limit:
        raise ValueError(f"beat_track: rows of more than {limit} frames are not supported, got {T}")
    periods = None if bpm is None else _periods(bpm, B, one_d, sr, hop_length)          # (validated before any device work)
    e, rs, _ = _env_rows(env, None, sr, hop_length)
    dev = e.device
    fps_bpm = 60.0 * float(sr) / float(hop_length)
    if bpm is not None:
        period = torch.from_numpy(periods).to(dev)
        tempo_out = torch.from_numpy(np.broadcast_to(np.asarray(
            bpm.detach().cpu().numpy() if isinstance(bpm, torch.Tensor) else bpm, np.float64).reshape(-1), (B,)).copy()).to(dev)
    elif B * T:
        idx, table = _tempo_index(e, rs, None, sr, hop_length, start_bpm, 1.0, 8.0, 320.0, False, prior)
        period = idx.view(B)
        tempo_out = table[period.long()]
    mask = torch.zeros((B, T), dtype=torch.uint8, device=dev)
    if B * T:
        count = torch.empty(B, dtype=torch.int32, device=dev)
        _x.check(_x.dlib(dev).ap_beat_track_f32(_x.ptr(e), B, T, rs, _x.ptr(period), float(tightness), int(bool(trim)),
                                                _x.ptr(mask), _x.ptr(count), None, None, None, _x.stream_ptr(dev)))
        if bpm is None and bool((count < 0).any()):
            raise ValueError(f"the estimated beat period is outside 2 .. {int(_x.lib().ap_beat_track_max_period())} frames "
                             f"({fps_bpm:.1f} / tempo); pass bpm= or lower hop_length")
        tempo_out = torch.where(count > 0, tempo_out, torch.zeros_like(tempo_out))
    else:
        tempo_out = torch.zeros(B, dtype=torch.float64, device=dev)
    mask = mask.view(torch.bool)
    tempo_out = tempo_out[0] if one_d else tempo_out
    if not sparse:
        return tempo_out, (mask[0] if one_d else mask)
    frames = torch.nonzero(mask[0]).squeeze(1)
    if units == "samples":
        return tempo_out, frames * int(hop_length)
    if units == "time":
        return tempo_out, frames.to(torch.float64) * int(hop_length) / float(sr)
    return tempo_out, frames


__all__ = ["tempo_frequencies", "tempogram", "tempo", "beat_track"]
