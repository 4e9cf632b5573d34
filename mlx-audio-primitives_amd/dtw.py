"""Dynamic time warping (no counterpart in the reference; the signatures of librosa 0.10's librosa.sequence.dtw and
dtw_backtracking).

Three kernels (csrc/kernels_dtw.h):

    cost        C[i,j] = metric(X[:,i], Y[:,j])                                tiled through LDS, one pass over X and Y
    accumulate  D[i,j] = min_s D[i - a_s, j - b_s] + (mul_s C[i,j] + add_s)     a wavefront over tiles, one launch per
                steps[i,j] = the s that won, 254 at a start cell, 255 unreachable   tile-anti-diagonal
    backtrack   follows steps from the end cell to a start cell                 one wave per pair, windows in LDS

Every addition and multiplication of the recursion is one rounded float32 operation and the comparison is the strict <
(the first minimum wins, a NaN never does): D, steps and the path equal the plain sequential definition in every bit,
whatever the tiling or the batch.  The global constraint is a predicate inside the kernel (cells outside the band cost
+inf); C is never copied.

Deviations from librosa, on purpose.  steps is uint8 and holds 254 / 255 next to the step indices, and backtracking
stops at a 254 cell (with subseq: anywhere in row 0); the cost metrics are the four below, computed on the device, not
scipy's cdist; a batch dimension is accepted; an unreachable end raises ValueError instead of librosa's
ParameterError.  No parity with librosa's numbers is claimed: the specification is tests/dtw_ref.py.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _extension as _x
from .cqt import _is_real
from .onset import _rows

_METRICS = {"euclidean": 0, "sqeuclidean": 1, "cityblock": 2, "cosine": 3}
_DEFAULT_STEPS = ((1, 1), (0, 1), (1, 0))


# ---------------------------------------------------------------------------------------------------------------------
# validation (no device)
# ---------------------------------------------------------------------------------------------------------------------
def _band_radius(band_rad: float, N: int, M: int) -> int:
    """r of the band: band_rad min(N, M), rounded half to even."""
    return int(round(float(band_rad) * min(int(N), int(M))))


def _in_band(i, j, N: int, M: int, r: int):
    """The global constraint: -r - max(N - M, 0) < j - i < r + max(M - N, 0)."""
    return (-r - max(N - M, 0) < j - i) & (j - i < r + max(M - N, 0))


def _step_table(step_sizes_sigma, weights_add, weights_mul):
    """(steps int32 (n, 2), add float32 (n), mul float32 (n)), validated against the kernel's caps."""
    lib = _x.lib()
    if step_sizes_sigma is None:
        step_sizes_sigma = _DEFAULT_STEPS
    try:
        raw = np.asarray(step_sizes_sigma)
    except Exception:
        raw = None
    if raw is None or raw.ndim != 2 or raw.shape[1] != 2 or raw.shape[0] < 1 or raw.dtype.kind not in "iu":
        raise ValueError(f"step_sizes_sigma must be an (n_steps, 2) array of integers, got {step_sizes_sigma!r}")
    n = raw.shape[0]
    cap_n, cap = int(lib.ap_dtw_max_steps()), int(lib.ap_dtw_max_step())
    if n > cap_n:
        raise ValueError(f"step_sizes_sigma has {n} steps, above the kernel's cap of {cap_n}")
    if (raw < 0).any():
        raise ValueError(f"step_sizes_sigma must not hold a negative component, got {raw.tolist()}")
    if (raw == 0).all(axis=1).any():
        raise ValueError(f"step_sizes_sigma must not hold the step (0, 0), got {raw.tolist()}")
    if (raw > cap).any():
        raise ValueError(f"step_sizes_sigma holds a component above the kernel's cap of {cap}, got {raw.tolist()}")
    weights = []
    for name, w, default in (("weights_add", weights_add, 0.0), ("weights_mul", weights_mul, 1.0)):
        if w is None:
            w = np.full(n, default, np.float32)
        else:
            w = np.asarray(w)
            if w.ndim != 1 or w.shape[0] != n or w.dtype.kind not in "fiu":
                raise ValueError(f"{name} must hold one real number per step ({n}), got shape {w.shape}")
            w = w.astype(np.float32)
        weights.append(np.ascontiguousarray(w))
    return np.ascontiguousarray(raw.astype(np.int32)), weights[0], weights[1]


def _real_input(a, name, ndims, what):
    """`a` as a torch tensor (on whatever device it lives), real, with one of the `ndims` dimensions, non-empty."""
    if not isinstance(a, torch.Tensor):
        a = torch.as_tensor(np.asarray(a))
    if a.is_complex() or a.dtype == torch.bool:
        raise ValueError(f"{name} must be real, got {a.dtype}")
    if a.ndim not in ndims:
        raise ValueError(f"{name} must be {what}, got {a.ndim}D")
    if 0 in a.shape:
        raise ValueError(f"{name} must not be empty, got shape {tuple(a.shape)}")
    return a


def _check_len(N, M, names=("N", "M")):
    cap = int(_x.lib().ap_dtw_max_len())
    for n, v in zip(names, (N, M)):
        if v > cap:
            raise ValueError(f"{n}={v} is above the kernel's cap of {cap}")


def _on_device(a: torch.Tensor, dev, dtype) -> torch.Tensor:
    if not (a.is_cuda and a.dtype == dtype):
        a = a.to(device=dev, dtype=dtype)                   # a padded-row view on the device stays a view
    return a


def _device_of(*tensors):
    for t in tensors:
        if t is not None and t.is_cuda:
            return t.device
    return _x.require_device()


# ---------------------------------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------------------------------
def _cost(X: torch.Tensor, Y: torch.Tensor, metric: int) -> torch.Tensor:
    """One launch of ap_dtw_cost_f32: C (B, N, M) of X (B, d, N), Y (B, d, M) float32 on one device."""
    B, d, N = X.shape
    M = Y.shape[2]
    dev = X.device
    C = torch.empty((B, N, M), dtype=torch.float32, device=dev)
    X, x_rs = _rows(X)
    Y, y_rs = _rows(Y)
    _x.check(_x.dlib(dev).ap_dtw_cost_f32(_x.ptr(X), _x.ptr(Y), B, d, N, M, x_rs, y_rs, int(metric), _x.ptr(C), M, _x.stream_ptr(dev)))
    return C


def _accumulate(C: torch.Tensor, table, subseq: bool, band_r):
    """ap_dtw_accumulate_f32 on C (B, N, M): (D float32, steps uint8)."""
    B, N, M = C.shape
    dev = C.device
    ab, add, mul = table
    D = torch.empty((B, N, M), dtype=torch.float32, device=dev)
    S = torch.empty((B, N, M), dtype=torch.uint8, device=dev)
    C, c_rs = _rows(C)
    _x.check(_x.dlib(dev).ap_dtw_accumulate_f32(_x.ptr(C), B, N, M, c_rs, int(ab.shape[0]), ab.ctypes.data, add.ctypes.data,
                                                mul.ctypes.data, int(bool(subseq)), int(band_r is not None), int(band_r or 0),
                                                _x.ptr(D), M, _x.ptr(S), M, _x.stream_ptr(dev)))
    return D, S


def _backtrack(S: torch.Tensor, D, start, ab: np.ndarray, subseq: bool):
    """ap_dtw_backtrack_i32 on the codes S (B, N, M): the list of B paths, slices of one device buffer.  The lengths
    come back with one synchronising copy."""
    B, N, M = S.shape
    dev = S.device
    path = torch.empty((B, N + M - 1, 2), dtype=torch.int32, device=dev)
    lens = torch.empty((B,), dtype=torch.int32, device=dev)
    S, s_rs = _rows(S)
    d_rs = M
    if D is not None:
        D, d_rs = _rows(D)
    _x.check(_x.dlib(dev).ap_dtw_backtrack_i32(None if D is None else _x.ptr(D), _x.ptr(S), None if start is None else _x.ptr(start),
                                               B, N, M, d_rs, s_rs, int(ab.shape[0]), ab.ctypes.data, int(bool(subseq)),
                                               _x.ptr(path), _x.ptr(lens), _x.stream_ptr(dev)))
    n_cells = lens.cpu().tolist()                           # the one synchronisation
    for b, n in enumerate(n_cells):
        if n < 0:
            raise ValueError(f"pair {b}: the end of the warping path cannot be reached from a start cell with these steps"
                             " and constraints")
    return [path[b, :n] for b, n in enumerate(n_cells)]


def dtw(X=None, Y=None, *, C=None, metric: str = "euclidean", step_sizes_sigma=None, weights_add=None, weights_mul=None,
        subseq: bool = False, backtrack: bool = True, global_constraints: bool = False, band_rad: float = 0.25,
        return_steps: bool = False):
    """Dynamic time warping (librosa.sequence.dtw's signature).

    X: (d, N) or (batch, d, N) and Y: (d, M) or (batch, d, M), real: the cost is metric(X[:, i], Y[:, j]) with metric
    one of "euclidean", "sqeuclidean", "cityblock", "cosine" (1 - x.y / (|x||y|); a product of norms below the smallest
    normal float32 counts as 1).  Or C: (N, M) or (batch, N, M), a cost matrix.  Exactly one of (X and Y) and C.  A
    float32 tensor on the device is read in place (rows may be padded); anything else is copied to the device.
    step_sizes_sigma: (n_steps, 2) non-negative integers, default [[1, 1], [0, 1], [1, 0]]; weights_add / weights_mul:
    one number per step, default 0 / 1.  subseq: the path may start anywhere in row 0 and ends at the first minimum of
    the last row.  global_constraints: only cells with -r - max(N - M, 0) < j - i < r + max(M - N, 0),
    r = round(band_rad min(N, M)), may be visited.

    Returns D float32 (N, M) or (batch, N, M); with backtrack, wp: the path from its end to its start as int32 (L, 2)
    (a list of such tensors for a batch; the one synchronisation of the call reads their lengths); with return_steps,
    steps uint8 shaped like D (the winning step, 254 where a path starts, 255 where none arrives).  As in librosa the
    values come as a tuple in this order, or D alone when nothing else is asked for.  Raises ValueError, naming the
    pair, when the end cell cannot be reached.  Everything runs on the input's device and current stream."""
    if C is None:
        if X is None or Y is None:
            raise ValueError("exactly one of (X and Y) and C must be given: got neither C nor both of X and Y")
    elif X is not None or Y is not None:
        raise ValueError("exactly one of (X and Y) and C must be given: got C together with X or Y")
    if metric not in _METRICS:
        raise ValueError(f"Unknown metric: {metric!r}. Supported: {', '.join(_METRICS)}")
    table = _step_table(step_sizes_sigma, weights_add, weights_mul)
    if not _is_real(band_rad) or not (0.0 < float(band_rad) <= 1.0):
        raise ValueError(f"band_rad must lie in (0, 1], got {band_rad!r}")
    if C is not None:
        Ct = _real_input(C, "C", (2, 3), "2D (N, M) or 3D (batch, N, M)")
        two_d = Ct.ndim == 2
        N, M = int(Ct.shape[-2]), int(Ct.shape[-1])
        _check_len(N, M)
    else:
        Xt = _real_input(X, "X", (2, 3), "2D (d, N) or 3D (batch, d, N)")
        Yt = _real_input(Y, "Y", (2, 3), "2D (d, M) or 3D (batch, d, M)")
        if Xt.ndim != Yt.ndim:
            raise ValueError(f"X and Y must both be 2D or both be 3D, got {Xt.ndim}D and {Yt.ndim}D")
        two_d = Xt.ndim == 2
        if Xt.shape[-2] != Yt.shape[-2]:
            raise ValueError(f"X and Y must hold the same number of features d, got {Xt.shape[-2]} and {Yt.shape[-2]}")
        if not two_d and Xt.shape[0] != Yt.shape[0]:
            raise ValueError(f"X and Y must hold the same number of pairs B, got {Xt.shape[0]} and {Yt.shape[0]}")
        d, N, M = int(Xt.shape[-2]), int(Xt.shape[-1]), int(Yt.shape[-1])
        cap = int(_x.lib().ap_dtw_max_features())
        if d > cap:
            raise ValueError(f"d={d} features are above the kernel's cap of {cap}")
        _check_len(N, M)
    band_r = _band_radius(band_rad, N, M) if global_constraints else None

    if C is not None:
        dev = _device_of(Ct)
        Cd = _on_device(Ct, dev, torch.float32)
        Cd = Cd[None] if two_d else Cd
    else:
        dev = _device_of(Xt, Yt)
        Xd, Yd = _on_device(Xt, dev, torch.float32), _on_device(Yt, dev, torch.float32)
        Cd = _cost(Xd[None] if two_d else Xd, Yd[None] if two_d else Yd, _METRICS[metric])
    D, S = _accumulate(Cd, table, subseq, band_r)
    out = [D[0] if two_d else D]
    if backtrack:
        wp = _backtrack(S, D if subseq else None, None, table[0], subseq)
        out.append(wp[0] if two_d else wp)
    if return_steps:
        out.append(S[0] if two_d else S)
    return tuple(out) if len(out) > 1 else out[0]


def dtw_backtracking(steps, *, step_sizes_sigma=None, subseq: bool = False, start=None):
    """The warping path of a step matrix (librosa.sequence.dtw_backtracking's signature).

    steps: uint8 (N, M) or (batch, N, M) as dtw(..., return_steps=True) returns it.  step_sizes_sigma: the table it was
    computed with.  start: the column of the last row the path ends in, an integer or one per pair; None: M - 1.
    subseq is accepted for librosa's signature: the path stops at a cell with code 254 either way, and the subsequence
    end is the first minimum of D's last row, which dtw itself uses (pass it as `start`).  Returns int32 (L, 2), or a
    list of such tensors for a batch; raises ValueError, naming the pair, when there is no path."""
    ab = _step_table(step_sizes_sigma, None, None)[0]
    St = _real_input(steps, "steps", (2, 3), "2D (N, M) or 3D (batch, N, M)")
    if St.dtype != torch.uint8:
        raise ValueError(f"steps must be uint8 as dtw returns it, got {St.dtype}")
    two_d = St.ndim == 2
    B, N, M = (1 if two_d else int(St.shape[0])), int(St.shape[-2]), int(St.shape[-1])
    _check_len(N, M)
    cols = None
    if start is not None:
        cols = np.asarray(start)
        if cols.dtype.kind not in "iu" or cols.ndim > 1 or (cols.ndim == 1 and cols.shape[0] != B):
            raise ValueError(f"start must be an integer or one integer per pair ({B}), got {start!r}")
        cols = np.broadcast_to(cols, (B,)).astype(np.int32)
        if (cols < 0).any() or (cols >= M).any():
            raise ValueError(f"start must lie in [0, {M}), got {start!r}")
    dev = _device_of(St)
    Sd = _on_device(St, dev, torch.uint8)
    startd = None if cols is None else torch.from_numpy(np.ascontiguousarray(cols)).to(dev)
    wp = _backtrack(Sd[None] if two_d else Sd, None, startd, ab, False)
    return wp[0] if two_d else wp


__all__ = ["dtw", "dtw_backtracking"]
