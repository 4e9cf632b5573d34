"""Per-channel energy normalisation (no counterpart in the reference; the signature of librosa.pcen, Wang et al. 2017).

One fused kernel (csrc/kernels_pcen.h): the first-order smoother along time as a wave-wide scan per
(clip, band) row, the optional running maximum over bins, the gain control and the root compression in one pass over
S.  The smoother never reaches memory.  The compression is evaluated as bias^power expm1(power log1p(S smooth / bias)),
which keeps its relative precision for quiet input where (S smooth + bias)^power - bias^power cancels.

zi / return_zf carry a row's filter state from one call to the next (StreamingPCEN in streaming.py does that): the
pieces of a spectrogram cut anywhere along time give the offline result to rounding.

Deviations from librosa, on purpose: axis must be the last axis and max_axis the one before it
(NotImplementedError otherwise); complex S raises ValueError instead of being replaced by its magnitude; non-negativity
and finiteness of S are not checked (a synchronising readback): the result is defined for finite S >= 0.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from . import _extension as _x
from .onset import _is_int, _rows, _spectrum, _to_dev


def _is_real(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def smoothing_coefficient(time_constant: float, sr: float, hop_length: int) -> float:
    """b of the smoother for a time constant in seconds: t = time_constant sr / hop_length frames,
    b = (sqrt(1 + 4 t^2) - 1) / (2 t^2), in float64."""
    t = float(time_constant) * float(sr) / float(hop_length)
    return (math.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t)


def _parameters(sr, hop_length, gain, bias, power, time_constant, eps, b, max_size, axis, max_axis, zi_given):
    """Validated (b as a Python float, gain, bias, power, eps, max_size)."""
    for name, v in (("gain", gain), ("bias", bias), ("power", power)):
        if not _is_real(v) or not float(v) >= 0.0 or not math.isfinite(float(v)):
            raise ValueError(f"{name} must be a non-negative number, got {v!r}")
    if not _is_real(eps) or not float(eps) > 0.0 or not math.isfinite(float(eps)):
        raise ValueError(f"eps must be strictly positive, got {eps!r}")
    if float(np.float32(eps)) < float(np.finfo(np.float32).tiny):
        raise ValueError(f"eps must be a positive normal float32 (>= {float(np.finfo(np.float32).tiny):.4e}), got {eps!r}")
    if not _is_real(time_constant) or not float(time_constant) > 0.0 or not math.isfinite(float(time_constant)):
        raise ValueError(f"time_constant must be strictly positive, got {time_constant!r}")
    if not _is_int(max_size) or not 1 <= max_size <= 255:
        raise ValueError(f"max_size must be an integer in 1 .. 255, got {max_size!r}")
    if b is None:
        if not _is_real(sr) or not float(sr) > 0.0:
            raise ValueError(f"sr must be strictly positive, got {sr!r}")
        if not _is_int(hop_length) or hop_length < 1:
            raise ValueError(f"hop_length must be a positive integer, got {hop_length!r}")
        b = smoothing_coefficient(time_constant, sr, hop_length)
    if not _is_real(b) or not 0.0 <= float(b) <= 1.0:
        raise ValueError(f"b must lie in [0, 1], got {b!r}")
    if float(b) == 0.0 and not zi_given:
        raise ValueError("b = 0 needs zi: the steady state of the smoother (scipy.signal.lfilter_zi) is undefined")
    if not _is_int(axis) or not isinstance(max_axis, (type(None), int, np.integer)) or isinstance(max_axis, bool):
        raise ValueError(f"axis and max_axis must be integers, got {axis!r}, {max_axis!r}")
    return float(b), float(gain), float(bias), float(power), float(eps), int(max_size)


def _axes(ndim, axis, max_axis, max_size):
    if not -ndim <= axis < ndim:
        raise ValueError(f"axis {axis} is out of range for {ndim}D input")
    if axis % ndim != ndim - 1:
        raise NotImplementedError("axis: only the last axis (time) is implemented")
    if max_axis is not None:
        if not -ndim <= max_axis < ndim:
            raise ValueError(f"max_axis {max_axis} is out of range for {ndim}D input")
        if max_axis % ndim != ndim - 2:
            raise NotImplementedError("max_axis: only the axis before time (the bins) is implemented")


def _state(zi, B, M, two_d):
    """zi as a tensor that broadcasts to (B, M, 1); it must broadcast to (B, M, 1) / (M, 1)."""
    if not isinstance(zi, torch.Tensor):
        zi = torch.as_tensor(np.asarray(zi))
    if zi.is_complex():
        raise ValueError(f"zi must be real, got {zi.dtype}")
    want = (M, 1) if two_d else (B, M, 1)
    try:
        ok = torch.broadcast_shapes(tuple(zi.shape), want) == want
    except RuntimeError:
        ok = False
    if not ok:
        raise ValueError(f"zi must broadcast to {want}, got {tuple(zi.shape)}")
    return zi


def _run(S, two_d, ref, zi, return_zf, b, gain, bias, power, eps, max_size):
    """One ap_pcen_f32 call on a validated spectrogram (any device); what pcen and StreamingPCEN share."""
    if two_d:
        S = S[None]
    B, M, T = S.shape
    if ref is not None:
        ref, _ = _spectrum(ref, "ref")
        if two_d and ref.ndim == 2:
            ref = ref[None]
        if tuple(ref.shape) != (B, M, T):
            raise ValueError(f"ref must have the shape of S {tuple(S.shape[1:] if two_d else S.shape)}, got {tuple(ref.shape)}")
    if zi is not None:
        zi = _state(zi, B, M, two_d)
    dev = S.device if S.is_cuda else _x.require_device()
    _x.lib()
    S = _to_dev(S, dev)
    if ref is not None:
        ref = _to_dev(ref, dev)
    if zi is not None:
        zi = zi.to(device=dev, dtype=torch.float32).expand((B, M, 1)).reshape(B * M).contiguous()
    out = torch.empty((B, M, T), dtype=torch.float32, device=dev)
    zf = torch.empty((B, M, 1), dtype=torch.float32, device=dev) if return_zf else None
    if B * M * T:
        S, rs = _rows(S)
        rs_ref = 0
        if ref is not None:
            ref, rs_ref = _rows(ref)
        _x.check(_x.dlib(dev).ap_pcen_f32(
            _x.ptr(S), B, M, T, rs, None if ref is None else _x.ptr(ref), rs_ref, max_size, b, gain, bias, power, eps,
            None if zi is None else _x.ptr(zi), _x.ptr(out), T, None if zf is None else _x.ptr(zf), _x.stream_ptr(dev)))
    elif return_zf and B * M:
        # no frame: the state passes through
        zf = (zi if zi is not None else torch.full((B * M,), 1.0 - b, dtype=torch.float32, device=dev)).reshape(B, M, 1).clone()
    if two_d:
        out = out[0]
        zf = None if zf is None else zf[0]
    return (out, zf) if return_zf else out


def pcen(S, *, sr: float = 22050, hop_length: int = 512, gain: float = 0.98, bias: float = 2, power: float = 0.5,
         time_constant: float = 0.400, eps: float = 1e-6, b=None, max_size: int = 1, ref=None, axis: int = -1,
         max_axis=None, zi=None, return_zf: bool = False):
    """Per-channel energy normalisation (librosa.pcen).

    S: a non-negative spectrogram (M, T) or (batch, M, T), float32, dense or a padded-row view, used as given (a mel
    spectrogram scaled as the model expects, e.g. melspectrogram(y) * 2**31).  With a = 1 - b and
    R = ref (an array of S's shape), S itself (max_size = 1) or the running maximum of S over max_size bins
    (scipy.ndimage.maximum_filter1d(S, max_size, axis=-2)):

        Msm[t] = b R[t] + a Msm[t - 1]                      scipy.signal.lfilter([b], [1, b - 1], R, zi=zi)
        out    = (S / (eps + Msm)^gain + bias)^power - bias^power
                 log1p(S / (eps + Msm)^gain) for power = 0;  (S / (eps + Msm)^gain)^power for bias = 0

    b: the smoothing coefficient; None: (sqrt(1 + 4 t^2) - 1) / (2 t^2) with t = time_constant sr / hop_length.
    zi: the filter state a row starts from, broadcastable to (batch, M, 1) / (M, 1); None: 1 - b for every row
    (scipy.signal.lfilter_zi: the steady state of a unit input).  return_zf=True: (out, zf), zf (batch, M, 1) / (M, 1)
    float32 on the device, the zi of the call that continues the rows.  Returns float32 of S's shape."""
    S, two_d = _spectrum(S)
    b, gain, bias, power, eps, max_size = _parameters(sr, hop_length, gain, bias, power, time_constant, eps, b, max_size,
                                                      axis, max_axis, zi is not None)
    _axes(S.ndim, int(axis), None if max_axis is None else int(max_axis), max_size)
    return _run(S, two_d, ref, zi, bool(return_zf), b, gain, bias, power, eps, max_size)


__all__ = ["pcen"]
