"""Onset strength, peak picking and onset detection (no counterpart in the reference; the signatures of
librosa.onset.onset_strength, librosa.util.peak_pick and librosa.onset.onset_detect).

onset_strength is the spectral flux of a log-power spectrogram, one fused kernel (csrc/kernels_onset.h, DESIGN.md
9.4): the reference level (the spectrogram itself, its running maximum along frequency, or an array of the caller),
the half-wave rectified difference `lag` frames apart, the mean over the bins and the shift to the frame the flux
belongs to, in one pass over S.  From audio, the mel kernel leaves the key of max(mel) on the device and the flux
kernel converts to dB as it loads, so the dB array is never written; both routes give the same bits.

peak_pick / onset_detect run one workgroup per row: normalisation, the candidate tests, the greedy `wait` pass over
the candidates and the backtrack to the preceding energy minimum, in one launch.

Deviations from librosa, on purpose: detrend=True, feature= and an aggregate other than the mean are not implemented
(NotImplementedError); non-negativity / finiteness of S is not checked (a synchronising readback): the envelope is
defined for finite S.
"""

from __future__ import annotations

import inspect

import numpy as np
import torch

from . import _extension as _x
from .mel import melspectrogram

_TOP_DB, _AMIN = 80.0, 1e-10


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _rows(a: torch.Tensor):
    """A (B, M, T) float32 device tensor as (tensor, row stride): kept in place when its rows are dense or padded and
    its clips are M rows apart, else copied."""
    B, M, T = a.shape
    sb, sm, st = a.stride()
    if B * M * T and (T == 1 or st == 1):
        rs = sm if M > 1 else (sb if B > 1 else T)
        if rs >= T and (B == 1 or sb == M * rs):
            return a, int(rs)
    return a.contiguous(), int(T)


def _shift(lag: int, center: bool, n_fft: int, hop_length: int) -> int:
    """Frames between flux[u] and the envelope frame it belongs to: the lag, plus the frames a centred STFT leads by."""
    return int(lag) + (int(n_fft) // (2 * int(hop_length)) if center else 0)


def _spectrum(S, name="S"):
    """Validated (tensor wherever the caller had it, was it 2D?)."""
    if not isinstance(S, torch.Tensor):
        S = torch.as_tensor(np.asarray(S))
    if S.ndim not in (2, 3):
        raise ValueError(f"{name} must be 2D or 3D, got {S.ndim}D")
    if S.is_complex():
        raise ValueError(f"{name} must be real (a log-power spectrogram), got {S.dtype}")
    return S, S.ndim == 2


def _to_dev(S: torch.Tensor, dev):
    if S.is_cuda and S.dtype == torch.float32 and S.device == dev:
        return S                                     # a padded-row view stays a view
    return S.to(device=dev, dtype=torch.float32)


def onset_strength(*, y=None, sr: float = 22050, S=None, lag: int = 1, max_size: int = 1, ref=None,
                   detrend: bool = False, center: bool = True, feature=None, aggregate=None, **kwargs):
    """Spectral-flux onset strength envelope (librosa.onset.onset_strength).

    S: a log-power spectrogram (M, T) or (batch, M, T), float32, dense or a padded-row view, used as given.  Without
    S: power_to_db(melspectrogram(y, sr=sr, n_fft=2048, hop_length=512, **kwargs)), top_db = 80 against the maximum of
    the whole batch.  With R = ref (an array of S's shape), S itself (max_size = 1) or the running maximum of S over
    max_size bins (scipy.ndimage.maximum_filter1d(S, max_size, axis=-2)):

        flux[u] = mean_m max(0, S[m, u + lag] - R[m, u])
        env[t]  = flux[t - shift] for t >= shift, else 0;  shift = lag + (n_fft // (2 * hop_length) if center else 0)

    (n_fft, hop_length from kwargs, defaults 2048 / 512, also when S is given.)  Returns (T,) or (batch, T) float32."""
    if aggregate is not None and aggregate not in (np.mean, torch.mean):
        raise NotImplementedError("aggregate: only the mean (None, np.mean, torch.mean) is implemented")
    if detrend:
        raise NotImplementedError("detrend=True is not implemented")
    if feature is not None:
        raise NotImplementedError("feature: only the default mel spectrogram is implemented")
    if not _is_int(lag) or lag < 1:
        raise ValueError(f"lag must be a positive integer, got {lag!r}")
    if not _is_int(max_size) or not 1 <= max_size <= 255:
        raise ValueError(f"max_size must be an integer in 1 .. 255, got {max_size!r}")
    if y is None and S is None:
        raise ValueError("onset_strength needs y or S")
    n_fft = kwargs.get("n_fft", 2048)
    hop_length = kwargs.get("hop_length", 512)
    if not _is_int(n_fft) or n_fft < 1 or not _is_int(hop_length) or hop_length < 1:
        raise ValueError(f"n_fft and hop_length must be positive integers, got {n_fft!r}, {hop_length!r}")
    shift = _shift(lag, center, n_fft, hop_length)
    if ref is not None:
        ref, _ = _spectrum(ref, "ref")

    max_key = None
    if S is not None:
        S, two_d = _spectrum(S)
        dev = S.device if S.is_cuda else _x.require_device()
        _x.lib()
        S = _to_dev(S, dev)
    else:
        from .mel import _is_pcm16, _melspectrogram_max, _to_device_pcm16

        mel = dict(kwargs, n_fft=int(n_fft), hop_length=int(hop_length))
        mel.setdefault("power", 2.0)
        a = inspect.signature(melspectrogram).bind(y, sr=sr, **mel)      # TypeError for a keyword melspectrogram lacks
        a.apply_defaults()
        a = a.arguments
        y = _to_device_pcm16(y) if _is_pcm16(y) else _x.to_device_f32(y)
        dev = y.device
        # the key of max(mel); starts as the key of 0.0 (0x80000000), which is what an empty signal's all-zero mel holds
        max_key = torch.full((1,), -2 ** 31, dtype=torch.int32, device=dev)
        S = _melspectrogram_max(y, a["sr"], a["n_fft"], a["hop_length"], a["win_length"], a["window"], a["center"],
                                a["pad_mode"], a["power"], a["n_mels"], a["fmin"], a["fmax"], a["htk"], a["norm"], max_key,
                                lines=True)
        two_d = S.ndim == 2
    if two_d:
        S = S[None]
    B, M, T = S.shape
    if ref is not None:
        if two_d and ref.ndim == 2:
            ref = ref[None]
        if tuple(ref.shape) != (B, M, T):
            raise ValueError(f"ref must have the shape of S {tuple(S.shape[1:] if two_d else S.shape)}, got {tuple(ref.shape)}")
        ref = _to_dev(ref, dev)
    out = torch.zeros((B, T), dtype=torch.float32, device=dev) if B * M * T == 0 else \
        torch.empty((B, T), dtype=torch.float32, device=dev)
    if B * M * T:
        S, rs = _rows(S)
        rs_ref = 0
        if ref is not None:
            ref, rs_ref = _rows(ref)
        _x.check(_x.dlib(dev).ap_onset_strength_f32(
            _x.ptr(S), B, M, T, rs, None if ref is None else _x.ptr(ref), rs_ref, int(lag), int(max_size), shift,
            int(max_key is not None), 10.0, _AMIN, 1.0, _TOP_DB, None if max_key is None else max_key.data_ptr(),
            _x.ptr(out), T, _x.stream_ptr(dev)))
    return out[0] if two_d else out


def _window_args(pre_max, post_max, pre_avg, post_avg, delta, wait):
    for name, v in (("pre_max", pre_max), ("pre_avg", pre_avg), ("wait", wait)):
        if not _is_int(v) or v < 0:
            raise ValueError(f"{name} must be a non-negative integer, got {v!r}")
    for name, v in (("post_max", post_max), ("post_avg", post_avg)):
        if not _is_int(v) or v < 1:
            raise ValueError(f"{name} must be a positive integer, got {v!r}")
    if isinstance(delta, bool) or not isinstance(delta, (int, float, np.integer, np.floating)) or not float(delta) >= 0.0:
        raise ValueError(f"delta must be a non-negative number, got {delta!r}")
    big = 1 << 30                                    # a window or a wait beyond any row: the same as the row's length
    return tuple(min(int(v), big) for v in (pre_max, post_max, pre_avg, post_avg)), float(delta), min(int(wait), big)


def _envelope(x, name):
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x))
    if x.ndim not in (1, 2):
        raise ValueError(f"{name} must be 1D or 2D, got {x.ndim}D")
    if x.is_complex():
        raise ValueError(f"{name} must be real, got {x.dtype}")
    return x


def _pick(x, windows, delta, wait, normalize, guard, backtrack, energy):
    """One ap_peak_pick_f32 call on a validated 1D / 2D envelope: the bool mask of x's shape."""
    dev = x.device if x.is_cuda else _x.require_device()
    _x.lib()
    one_d = x.ndim == 1
    x = x.to(device=dev, dtype=torch.float32)
    x = (x[None] if one_d else x).contiguous()
    B, T = x.shape
    if energy is not None:
        energy = energy.to(device=dev, dtype=torch.float32)
        energy = (energy[None] if energy.ndim == 1 else energy).contiguous()
        if tuple(energy.shape) != (B, T):
            raise ValueError(f"energy must have the shape of the envelope {tuple(x.shape)}, got {tuple(energy.shape)}")
    mask = torch.zeros((B, T), dtype=torch.uint8, device=dev) if B * T == 0 else \
        torch.empty((B, T), dtype=torch.uint8, device=dev)
    if B * T:
        count = torch.empty(B, dtype=torch.int32, device=dev)
        _x.check(_x.dlib(dev).ap_peak_pick_f32(
            _x.ptr(x), B, T, T, *windows, delta, wait, int(bool(normalize)), int(bool(guard)), int(bool(backtrack)),
            None if energy is None else _x.ptr(energy), T, _x.ptr(mask), _x.ptr(count), _x.stream_ptr(dev)))
    mask = mask.view(torch.bool)
    return mask[0] if one_d else mask


def peak_pick(x, *, pre_max: int, post_max: int, pre_avg: int, post_avg: int, delta: float, wait: int,
              sparse: bool = True):
    """Peaks of an envelope (librosa.util.peak_pick).  x: (T,) or (batch, T).  Frame n is a candidate iff
    x[n] == max(x[max(0, n - pre_max) : min(n + post_max, T)]) and
    x[n] >= mean(x[max(0, n - pre_avg) : min(n + post_avg, T)]) + delta; candidates are kept from the left, each at
    least wait + 1 frames after the last kept one.  sparse=True (1D input only): int64 frame indices on the device;
    sparse=False: a bool tensor of x's shape."""
    windows, delta, wait = _window_args(pre_max, post_max, pre_avg, post_avg, delta, wait)
    x = _envelope(x, "x")
    if sparse and x.ndim != 1:
        raise ValueError("sparse=True needs 1D input; use sparse=False for a batch")
    mask = _pick(x, windows, delta, wait, False, False, False, None)
    return torch.nonzero(mask).squeeze(1) if sparse else mask


def _detect_parameters(sr, hop_length, kwargs):
    """((pre_max, post_max, pre_avg, post_avg), delta, wait) of onset_detect: librosa's defaults, overridden by kwargs."""
    kw = {"pre_max": 0.03 * sr // hop_length, "post_max": 0.00 * sr // hop_length + 1,
          "pre_avg": 0.10 * sr // hop_length, "post_avg": 0.10 * sr // hop_length + 1,
          "wait": 0.03 * sr // hop_length, "delta": 0.07}
    unknown = sorted(set(kwargs) - set(kw))
    if unknown:
        raise TypeError(f"onset_detect() got unexpected keyword arguments {unknown}")
    kw.update(kwargs)
    for k in ("pre_max", "post_max", "pre_avg", "post_avg", "wait"):        # librosa rounds these up to integers
        v = kw[k]
        if not _is_int(v):
            if isinstance(v, bool) or not isinstance(v, (float, np.floating)) or not np.isfinite(v):
                raise ValueError(f"{k} must be a number of frames, got {v!r}")
            kw[k] = int(np.ceil(v))
    return _window_args(kw["pre_max"], kw["post_max"], kw["pre_avg"], kw["post_avg"], kw["delta"], kw["wait"])


_UNITS = ("frames", "samples", "time")


def onset_detect(*, y=None, sr: float = 22050, onset_envelope=None, hop_length: int = 512, backtrack: bool = False,
                 energy=None, units: str = "frames", normalize: bool = True, sparse: bool = True, **kwargs):
    """Onset events by peak picking on the onset strength envelope (librosa.onset.onset_detect).

    The envelope is the one given, or onset_strength(y=y, sr=sr, hop_length=hop_length); normalised to [0, 1] per row
    (normalize); a row that is all zero or holds a non-finite value yields no onsets.  kwargs override the window
    parameters of peak_pick (pre_max = 0.03 sr // hop_length, post_max = 0.00 sr // hop_length + 1, pre_avg =
    0.10 sr // hop_length, post_avg = 0.10 sr // hop_length + 1, wait = 0.03 sr // hop_length, delta = 0.07).
    backtrack: every onset moves back to the preceding local minimum of `energy` (default: the envelope peak picking
    saw).  units: "frames", "samples" (frames * hop_length) or "time" (seconds, float64), the last two with
    sparse=True only.  sparse=False: a bool tensor of the envelope's shape."""
    if units not in _UNITS:
        raise ValueError(f"units must be one of {_UNITS}, got {units!r}")
    if units != "frames" and not sparse:
        raise ValueError(f"units={units!r} needs sparse=True")
    if y is None and onset_envelope is None:
        raise ValueError("onset_detect needs y or onset_envelope")
    if not _is_int(hop_length) or hop_length < 1:
        raise ValueError(f"hop_length must be a positive integer, got {hop_length!r}")
    windows, delta, wait = _detect_parameters(sr, hop_length, kwargs)
    if onset_envelope is None:
        ndim = len(np.shape(y)) if not isinstance(y, torch.Tensor) else y.ndim
        if sparse and ndim != 1:
            raise ValueError("sparse=True needs 1D input; use sparse=False for a batch")
        onset_envelope = onset_strength(y=y, sr=sr, hop_length=hop_length)
    env = _envelope(onset_envelope, "onset_envelope")
    if sparse and env.ndim != 1:
        raise ValueError("sparse=True needs 1D input; use sparse=False for a batch")
    if energy is not None:
        energy = _envelope(energy, "energy")
    mask = _pick(env, windows, delta, wait, normalize, True, backtrack, energy if backtrack else None)
    if not sparse:
        return mask
    frames = torch.nonzero(mask).squeeze(1)
    if units == "samples":
        return frames * int(hop_length)
    if units == "time":
        return frames.to(torch.float64) * int(hop_length) / float(sr)
    return frames


__all__ = ["onset_strength", "peak_pick", "onset_detect"]
