"""Recurrence and cross-similarity matrices (no counterpart in the reference; the signatures of librosa 0.10's
librosa.segment.recurrence_matrix, cross_similarity, recurrence_to_lag and lag_to_recurrence).

Three kernels and a gather (csrc/kernels_segment.h); the N x M distance matrix is never stored:

    threshold   (tau_j, t_j): the k-th smallest eligible distance of query j by an exact radix select, and the largest
                index admitted among the frames tied there                       a workgroup per query, 8 bytes out
    bandwidth   median / mean / geometric mean of tau_j, on the device, in a fixed order      one small launch
    write       R[i, j] from D[i, j] recomputed and (D, i) <= (tau_j, t_j); sym, self, the mode   every cell written once
    lag         lag[(i - j) mod t', j] = rec[i, j] and its inverse               row segments through LDS

D[i, j] = metric(ref[:, i], data[:, j]) has the bits of dtw's cost kernel.  The neighbours of query j are the first k
eligible frames in the order (D[i, j], i): ties go to the smaller index, a NaN distance is never a neighbour.

Deviations from librosa, on purpose.  The metrics are dtw's four, computed on the device, not sklearn's; ties are
broken by index where sklearn's order is unspecified; a batch dimension is accepted (every matrix of a batch gets its
own bandwidth); sparse output, the axis argument, per-pair bandwidths and array bandwidths are not implemented and
raise ValueError (where librosa raises ParameterError).  No parity with librosa's numbers is claimed: the specification
is tests/segment_ref.py.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from . import _extension as _x
from .cqt import _is_real
from .dtw import _METRICS, _device_of, _on_device, _real_input
from .onset import _rows

_MODES = {"connectivity": 0, "distance": 1, "affinity": 2}
_BANDWIDTHS = {"med_k_scalar": 0, "mean_k": 1, "gmean_k": 2}
_BANDWIDTHS_NOT_IMPLEMENTED = ("mean_k_avg", "gmean_k_avg", "mean_k_avg_and_pair")


# ---------------------------------------------------------------------------------------------------------------------
# validation (no device)
# ---------------------------------------------------------------------------------------------------------------------
def _default_k(n_eligible: int) -> int:
    """librosa's default: 2 ceil(sqrt(t)), t the frames a query can choose from."""
    t = max(int(n_eligible), 0)
    r = math.isqrt(t)
    return 2 * (r if r * r == t else r + 1)


def _check_k(k):
    if k is None:
        return None
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 1:
        raise ValueError(f"k must be a positive integer, got {k!r}")
    return int(k)


def _check_common(metric, sparse, mode, bandwidth, axis, full):
    """(metric code, mode code, bandwidth kind or None, bandwidth value or None)."""
    if sparse:
        raise ValueError("sparse=True is not implemented: the result is a dense tensor on the device")
    if axis != -1:
        raise ValueError(f"axis={axis!r} is not implemented: frames lie along the last axis (axis=-1)")
    if not isinstance(metric, str) or metric not in _METRICS:
        raise ValueError(f"Unknown metric: {metric!r}. Supported: {', '.join(_METRICS)}")
    if not isinstance(mode, str) or mode not in _MODES:
        raise ValueError(f"Unknown mode: {mode!r}. Supported: {', '.join(_MODES)}")
    kind, value = None, None
    if bandwidth is None:
        kind = 0
    elif isinstance(bandwidth, str):
        if bandwidth in _BANDWIDTHS_NOT_IMPLEMENTED:
            raise ValueError(f"bandwidth={bandwidth!r} is not implemented: per-pair bandwidths are out of scope; use one of"
                             f" {', '.join(_BANDWIDTHS)} or a positive number")
        if bandwidth not in _BANDWIDTHS:
            raise ValueError(f"Unknown bandwidth: {bandwidth!r}. Supported: {', '.join(_BANDWIDTHS)} or a positive number")
        kind = _BANDWIDTHS[bandwidth]
    elif _is_real(bandwidth):
        value = float(bandwidth)
        if not (value > 0.0 and math.isfinite(value)):
            raise ValueError(f"bandwidth must be a positive finite number, got {bandwidth!r}")
    else:
        raise ValueError(f"bandwidth={type(bandwidth).__name__} is not implemented: an array of per-pair bandwidths is out of"
                         " scope; pass a positive number or the name of an estimate")
    return _METRICS[metric], _MODES[mode], kind, value


def _check_sizes(d, n_ref, n):
    lib = _x.lib()
    cap = int(lib.ap_dtw_max_features())
    if d > cap:
        raise ValueError(f"d={d} features are above the kernel's cap of {cap}")
    cap = int(lib.ap_segment_max_len())
    for name, v in (("n_ref", n_ref), ("n", n)):
        if v > cap:
            raise ValueError(f"{name}={v} frames are above the kernel's cap of {cap}")


# ---------------------------------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------------------------------
def _threshold(X, x_rs, Y, y_rs, B, d, n_ref, n, metric, k, width):
    """ap_segment_threshold_f32: the records (B, n, 2) int32 (the bits of tau_j, t_j)."""
    dev = Y.device
    rec = torch.empty((B, n, 2), dtype=torch.int32, device=dev)
    _x.check(_x.dlib(dev).ap_segment_threshold_f32(_x.ptr(X), _x.ptr(Y), B, d, n_ref, n, x_rs, y_rs, metric, int(k), int(width), _x.ptr(rec),
                                                   _x.stream_ptr(dev)))
    return rec


def _bandwidth(rec, kind):
    """ap_segment_bandwidth_f32: one float32 per matrix, on the device."""
    B, n, _ = rec.shape
    bw = torch.empty((B,), dtype=torch.float32, device=rec.device)
    _x.check(_x.dlib(rec.device).ap_segment_bandwidth_f32(_x.ptr(rec), B, n, int(kind), _x.ptr(bw), _x.stream_ptr(rec.device)))
    return bw


def _knn_matrix(Xt, Yt, two_d, metric, mode, k, width, full, sym, self_diag, kind, value):
    """R (B, n_ref, n) of ref Xt (B, d, n_ref) and data Yt (B, d, n), validated."""
    dev = _device_of(Yt, Xt)
    Yd = _on_device(Yt, dev, torch.float32)
    Xd = Yd if Xt is Yt else _on_device(Xt, dev, torch.float32)
    if two_d:
        Xd, Yd = Xd[None], Yd[None]
    B, d, n = Yd.shape
    n_ref = Xd.shape[2]
    Yd, y_rs = _rows(Yd)
    Xd, x_rs = (Yd, y_rs) if Xt is Yt else _rows(Xd)
    rec = _threshold(Xd, x_rs, Yd, y_rs, B, d, n_ref, n, metric, k, width)
    bw = None
    if mode == 2 and value is None:
        bw = _bandwidth(rec, kind)
        host = bw.cpu().numpy()                             # the one synchronisation: an estimate may be unusable
        bad = ~(np.isfinite(host) & (host > 0.0))
        if bad.any():
            b = int(np.argmax(bad))
            raise ValueError(f"the estimated bandwidth of matrix {b} is {host[b]!r}, not a positive finite number (the k-th"
                             " neighbours' distances are zero, infinite, or no query has a neighbour): pass bandwidth= a positive number")
    R = torch.empty((B, n_ref, n), dtype=torch.uint8 if mode == 0 else torch.float32, device=dev)
    _x.check(_x.dlib(dev).ap_segment_write_f32(_x.ptr(Xd), _x.ptr(Yd), B, d, n_ref, n, x_rs, y_rs, metric, mode, int(width), int(bool(full)),
                                               int(bool(sym)), int(bool(self_diag)), _x.ptr(rec), None if bw is None else _x.ptr(bw),
                                               1.0 if value is None else value, _x.ptr(R), n, _x.stream_ptr(dev)))
    if mode == 0:
        R = R.view(torch.bool)
    return R[0] if two_d else R


def recurrence_matrix(data, *, k=None, width=1, metric="euclidean", sym=False, sparse=False, mode="connectivity", bandwidth=None,
                      self=False, axis=-1, full=False):
    """The self-similarity (recurrence) matrix of a feature sequence (librosa.segment.recurrence_matrix's signature).

    data: (d, n) or (batch, d, n), real.  A float32 tensor on the device is read in place (its rows may be padded views,
    as chroma_* return them); anything else is copied to the device.  R[i, j] is non-zero only if frame i is one of the
    k nearest neighbours of frame j among the frames with |i - j| >= width, in the order (distance, index): ties go
    to the smaller index and a NaN distance is never a neighbour.  metric: "euclidean", "sqeuclidean", "cityblock" or
    "cosine" with the bits of dtw's cost matrix.  k: a positive integer, default 2 ceil(sqrt(n - 2 width + 1)), clipped
    to the eligible frames.  width: 1 <= width <= (n - 1) // 2 (or n == 1 with width == 1).  full: every eligible frame
    is kept and k only defines the bandwidth.  mode: "connectivity" gives torch.bool, "distance" the distances and
    "affinity" exp(-distance / bandwidth) as float32.  bandwidth: a positive number, or the estimate None /
    "med_k_scalar" (the median of the distances to the k-th neighbours), "mean_k" or "gmean_k" (their mean, their
    geometric mean), computed on the device, one per matrix of a batch; librosa's per-pair estimates and array
    bandwidths are not implemented.  sym: R = min(R, R^T): only mutual neighbours stay.  self: the diagonal is set to 1
    (connectivity, affinity) or 0 (distance).  sparse=True and axis != -1 are not implemented.

    Returns R (n, n) or (batch, n, n) on the input's device, computed on its current stream.  Nothing synchronises,
    except that an estimated bandwidth in affinity mode is copied to the host (4 bytes per matrix) to raise ValueError
    when it is not a positive finite number.  Every rejected argument raises ValueError before any device call."""
    metric_c, mode_c, kind, value = _check_common(metric, sparse, mode, bandwidth, axis, full)
    k = _check_k(k)
    Yt = _real_input(data, "data", (2, 3), "2D (d, n) or 3D (batch, d, n)")
    d, n = int(Yt.shape[-2]), int(Yt.shape[-1])
    if isinstance(width, bool) or not isinstance(width, (int, np.integer)):
        raise ValueError(f"width must be an integer, got {width!r}")
    width = int(width)
    if not (1 <= width <= (n - 1) // 2 or (n == 1 and width == 1)):
        raise ValueError(f"width={width} must be at least 1 and at most (data.shape[-1] - 1) // 2 = {(n - 1) // 2}")
    _check_sizes(d, n, n)
    if k is None:
        k = _default_k(n - 2 * width + 1)
    k = max(min(k, n), 1)
    return _knn_matrix(Yt, Yt, Yt.ndim == 2, metric_c, mode_c, k, width, full, sym, self, kind, value)


def cross_similarity(data, data_ref, *, k=None, metric="euclidean", sparse=False, mode="connectivity", bandwidth=None, full=False):
    """The cross-similarity matrix of two feature sequences (librosa.segment.cross_similarity's signature).

    data: (d, n) or (batch, d, n) and data_ref: (d, n_ref) or (batch, d, n_ref), real, read or copied as for
    recurrence_matrix.  R[i, j] is non-zero only if data_ref[:, i] is one of the k nearest neighbours of data[:, j]
    among all frames of data_ref, in the order (distance, index).  k: a positive integer, default
    2 ceil(sqrt(n_ref)), clipped to n_ref.  metric, mode, bandwidth, full and sparse as for recurrence_matrix.

    Returns R (n_ref, n) or (batch, n_ref, n) on the input's device, computed on its current stream; the one possible
    synchronisation is recurrence_matrix's.  Every rejected argument raises ValueError before any device call."""
    metric_c, mode_c, kind, value = _check_common(metric, sparse, mode, bandwidth, -1, full)
    k = _check_k(k)
    Yt = _real_input(data, "data", (2, 3), "2D (d, n) or 3D (batch, d, n)")
    Xt = _real_input(data_ref, "data_ref", (2, 3), "2D (d, n_ref) or 3D (batch, d, n_ref)")
    if Xt.ndim != Yt.ndim:
        raise ValueError(f"data and data_ref must both be 2D or both be 3D, got {Yt.ndim}D and {Xt.ndim}D")
    if Xt.shape[-2] != Yt.shape[-2]:
        raise ValueError(f"data and data_ref must hold the same number of features d, got {Yt.shape[-2]} and {Xt.shape[-2]}")
    if Yt.ndim == 3 and Xt.shape[0] != Yt.shape[0]:
        raise ValueError(f"data and data_ref must hold the same number of pairs (batch), got {Yt.shape[0]} and {Xt.shape[0]}")
    d, n, n_ref = int(Yt.shape[-2]), int(Yt.shape[-1]), int(Xt.shape[-1])
    _check_sizes(d, n_ref, n)
    if k is None:
        k = _default_k(n_ref)
    k = max(min(k, n_ref), 1)
    return _knn_matrix(Xt, Yt, Yt.ndim == 2, metric_c, mode_c, k, 0, full, False, False, kind, value)


def _lag_input(a, name, lag_side):
    if not isinstance(a, torch.Tensor):
        a = torch.as_tensor(np.asarray(a))
    if a.dtype not in (torch.bool, torch.float32):
        raise ValueError(f"{name} must be bool or float32, got {a.dtype}")
    if a.ndim not in (2, 3):
        raise ValueError(f"{name} must be 2D or 3D (batch first), got {a.ndim}D")
    if 0 in a.shape:
        raise ValueError(f"{name} must not be empty, got shape {tuple(a.shape)}")
    rows, n = int(a.shape[-2]), int(a.shape[-1])
    if rows != n and not (lag_side and rows == 2 * n):
        raise ValueError(f"{name} must be square" + (" or hold twice as many lags as frames" if lag_side else "")
                         + f", got shape {tuple(a.shape)}")
    cap = int(_x.lib().ap_segment_max_len())
    if n > cap:
        raise ValueError(f"n={n} frames are above the kernel's cap of {cap}")
    return a


def _lag(a, to_lag: bool, t_lag: int):
    two_d = a.ndim == 2
    dev = _device_of(a)
    ad = a if a.is_cuda else a.to(dev)
    ad = ad[None] if two_d else ad
    is_bool = ad.dtype == torch.bool
    src = ad.view(torch.uint8) if is_bool else ad
    B, rows_in, n = src.shape
    src, in_rs = _rows(src)
    out = torch.empty((B, t_lag if to_lag else n, n), dtype=src.dtype, device=dev)
    _x.check(_x.dlib(dev).ap_segment_lag(_x.ptr(src), B, n, int(t_lag), 1 if is_bool else 4, int(to_lag), in_rs, _x.ptr(out), n,
                                         _x.stream_ptr(dev)))
    if is_bool:
        out = out.view(torch.bool)
    return out[0] if two_d else out


def recurrence_to_lag(rec, *, pad=True, axis=-1):
    """A recurrence matrix as a lag matrix (librosa.segment.recurrence_to_lag's signature):
    lag[(i - j) mod t', j] = rec[i, j] with t' = 2 n (pad=True; the rows no i maps to are 0) or t' = n.

    rec: (n, n) or (batch, n, n), bool or float32.  axis other than -1 is not implemented.  Returns (t', n) or
    (batch, t', n) of rec's dtype on its device."""
    if axis != -1:
        raise ValueError(f"axis={axis!r} is not implemented: the lag runs along the rows (axis=-1)")
    a = _lag_input(rec, "rec", False)
    n = int(a.shape[-1])
    return _lag(a, True, 2 * n if pad else n)


def lag_to_recurrence(lag, *, axis=-1):
    """The inverse of recurrence_to_lag (librosa.segment.lag_to_recurrence's signature):
    rec[i, j] = lag[(i - j) mod t', j].

    lag: (t', n) or (batch, t', n) with t' = n or 2 n, bool or float32.  Returns (n, n) or (batch, n, n)."""
    if axis != -1:
        raise ValueError(f"axis={axis!r} is not implemented: the lag runs along the rows (axis=-1)")
    a = _lag_input(lag, "lag", True)
    return _lag(a, False, int(a.shape[-2]))


__all__ = ["recurrence_matrix", "cross_similarity", "recurrence_to_lag", "lag_to_recurrence"]
