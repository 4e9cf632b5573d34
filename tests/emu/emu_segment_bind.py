"""ctypes bindings for tests/emu/libapemu_segment.so (TEST INFRASTRUCTURE ONLY).

Runs the recurrence / cross-similarity kernel source (kernels_segment.h) on the CPU through the SIMT emulator of
emu_shim.h.  Built on demand with g++; never imported by the product package.  Every buffer lies between poisoned
bands and every row has poisoned pad columns behind it (NaN for float32, 0xEE for bytes)."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

import emu_dtw_bind as _d

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "mlx-audio-primitives_amd", "csrc")
LIB = os.path.join(HERE, "libapemu_segment.so")
SRC = os.path.join(HERE, "emu_segment.cpp")

_p, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
BAND = _d.BAND
BYTE_POISON = _d.BYTE_POISON
WORD_POISON = 0xEEEEEEEE
METRICS = _d.METRICS
MODES = {"connectivity": 0, "distance": 1, "affinity": 2}
KINDS = {"med_k_scalar": 0, "mean_k": 1, "gmean_k": 2}


def compile_lib(out, src=SRC, defines=()):
    tmp = f"{out}.{os.getpid()}.tmp"
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-pthread", "-I", HERE] + [f"-D{d}" for d in defines]
                          + ["-o", tmp, src])
    os.replace(tmp, out)
    return out


def build(force=False):
    deps = [SRC, os.path.join(HERE, "emu_shim.h"), os.path.join(ROOT, "include", "audioprims.h")] + [
        os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")
    ]
    if not force and os.path.exists(LIB):
        if os.path.getmtime(LIB) >= max(os.path.getmtime(d) for d in deps):
            return LIB
    return compile_lib(LIB)


def declare(L):
    L.emu_segment_last_error.restype = ctypes.c_char_p
    L.emu_segment_geometry.restype = ctypes.POINTER(ctypes.c_int)
    L.emu_segment_threshold_f32.argtypes = [_p, _p, _i64, _int, _i64, _i64, _i64, _i64, _int, _i64, _i64, _p, _int]
    L.emu_segment_bandwidth_f32.argtypes = [_p, _i64, _i64, _int, _p, _int]
    L.emu_segment_write_f32.argtypes = [_p, _p, _i64, _int, _i64, _i64, _i64, _i64, _int, _int, _i64, _int, _int, _int, _p, _p,
                                        ctypes.c_double, _p, _i64, _int]
    L.emu_segment_lag.argtypes = [_p, _i64, _i64, _i64, _int, _int, _i64, _p, _i64, _int]
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = declare(ctypes.CDLL(build()))
    return _lib


def use(handle):
    """Route every call through another build of the twin (the mutation tests); None: the regular one."""
    global _lib
    _lib = handle


class Status(ValueError):
    def __init__(self, rc, msg):
        super().__init__(msg)
        self.rc = rc


def _check(rc):
    if rc != 0:
        raise Status(rc, lib().emu_segment_last_error().decode())


def last_error():
    return lib().emu_segment_last_error().decode()


def constants():
    g = lib().emu_segment_geometry()
    names = ("threads", "tile_rows", "tile_cols", "chunk", "max_features", "max_len")
    return {n: g[i] for i, n in enumerate(names)}


def geometry():
    g = lib().emu_segment_geometry()
    return dict(grid=g[6], lds_bytes=g[7])


def _lds_clean():
    assert lib().emu_segment_lds_overruns() == 0, "LDS beyond the bytes the host asked for was written"


def _words(n):
    """(raw uint32 array of n poisoned words between poisoned bands, pointer to the payload)."""
    raw = np.full(n + 2 * BAND, WORD_POISON, np.uint32)
    return raw, raw.ctypes.data + 4 * BAND


def _words_payload(raw, what):
    assert (raw[:BAND] == WORD_POISON).all() and (raw[-BAND:] == WORD_POISON).all(), f"{what}: a band was written"
    _lds_clean()
    return raw[BAND:-BAND]


class Pair:
    """ref (B, d, n_ref) and data (B, d, n) in guarded buffers with NaN pad columns; data alone: a recurrence pair, the
    two share one buffer."""

    def __init__(self, ref, data, pad_ref=0, pad_data=0):
        self.data = np.asarray(data, np.float32)
        self.B, self.d, self.n = self.data.shape
        self._yraw, self.yptr, self.y_rs = _d._rows(self.data, pad_data)
        if ref is None:
            self.ref, self.n_ref, self._xraw, self.xptr, self.x_rs = self.data, self.n, self._yraw, self.yptr, self.y_rs
        else:
            self.ref = np.asarray(ref, np.float32)
            self.n_ref = self.ref.shape[2]
            self._xraw, self.xptr, self.x_rs = _d._rows(self.ref, pad_ref)


def threshold(pair, metric, k, width=0, grid=0):
    """(tau float32 (B, n), t int32 (B, n)) through the emulated C entry."""
    raw, ptr = _words(pair.B * pair.n * 2)
    _check(lib().emu_segment_threshold_f32(pair.xptr, pair.yptr, pair.B, pair.d, pair.n_ref, pair.n, pair.x_rs, pair.y_rs, METRICS[metric],
                                           int(k), int(width), ptr, int(grid)))
    rec = _words_payload(raw, "records").reshape(pair.B, pair.n, 2)
    assert not (rec[..., 1] == WORD_POISON).any(), "a record was not written"
    return rec[..., 0].copy().view(np.float32), rec[..., 1].copy().view(np.int32)


def _records(tau, t):
    rec = np.stack([np.ascontiguousarray(tau, np.float32).view(np.uint32), np.ascontiguousarray(t, np.int32).view(np.uint32)], axis=-1)
    raw, ptr = _words(rec.size)
    raw[BAND:-BAND] = rec.ravel()
    return raw, ptr


def bandwidth(tau, t, kind, grid=0):
    """bw float32 (B) of the records through the emulated C entry."""
    B, n = tau.shape
    rraw, rptr = _records(tau, t)
    braw = np.full(B + 2 * BAND, np.nan, np.float32)
    braw[BAND:-BAND] = -7.0
    _check(lib().emu_segment_bandwidth_f32(rptr, B, n, KINDS[kind], braw.ctypes.data + 4 * BAND, int(grid)))
    assert np.isnan(braw[:BAND]).all() and np.isnan(braw[-BAND:]).all(), "a band of bw was written"
    _lds_clean()
    return braw[BAND:-BAND].copy()


def write(pair, metric, mode, tau, t, *, width=0, full=False, sym=False, self_diag=False, bw=None, bandwidth_value=1.0, pad_out=0, grid=0):
    """R (B, n_ref, n): bool (connectivity) or float32, through the emulated C entry.  bw: float32 (B) as the device
    estimate, else bandwidth_value holds.  The output lies between poisoned bands with poisoned pad columns; every
    cell of the payload must have been written."""
    B, n_ref, n = pair.B, pair.n_ref, pair.n
    rraw, rptr = _records(tau, t)
    rs = n + pad_out
    is_byte = mode == "connectivity"
    oraw = np.full(B * n_ref * rs + 2 * BAND, BYTE_POISON if is_byte else np.nan, np.uint8 if is_byte else np.float32)
    bwraw, bwptr = (None, None) if bw is None else _d._guarded(np.asarray(bw, np.float32))
    _check(lib().emu_segment_write_f32(pair.xptr, pair.yptr, B, pair.d, n_ref, n, pair.x_rs, pair.y_rs, METRICS[metric], MODES[mode], int(width),
                                       int(bool(full)), int(bool(sym)), int(bool(self_diag)), rptr, bwptr, float(bandwidth_value),
                                       oraw.ctypes.data + oraw.itemsize * BAND, rs, int(grid)))
    got = _payload(oraw, B, n_ref, n, rs, "R")
    if is_byte:
        assert ((got == 0) | (got == 1)).all(), "a cell is neither 0 nor 1, or was not written"
        return got.astype(bool)
    assert not np.isnan(got).any(), "a cell is NaN or was not written"
    return got


def _payload(raw, B, R, T, rs, what):
    body = raw[BAND:-BAND].reshape(B, R, rs)
    if raw.dtype == np.float32:
        clean = np.isnan(raw[:BAND]).all() and np.isnan(raw[-BAND:]).all() and np.isnan(body[:, :, T:]).all()
    elif raw.dtype == np.uint32:
        clean = (raw[:BAND] == WORD_POISON).all() and (raw[-BAND:] == WORD_POISON).all() and (body[:, :, T:] == WORD_POISON).all()
    else:
        clean = (raw[:BAND] == BYTE_POISON).all() and (raw[-BAND:] == BYTE_POISON).all() and (body[:, :, T:] == BYTE_POISON).all()
    assert clean, f"{what}: a band or a pad column was written"
    _lds_clean()
    return body[:, :, :T].copy()


def lag(a, to_lag, pad=True, *, pad_in=0, pad_out=0, grid=0):
    """recurrence_to_lag (to_lag) / lag_to_recurrence of a (B, rows, n) bool or float32 through the emulated C entry."""
    a = np.asarray(a)
    is_bool = a.dtype == np.bool_
    src = a.view(np.uint8) if is_bool else a.view(np.uint32)
    B, rows_in, n = src.shape
    tp = (2 * n if pad else n) if to_lag else rows_in
    rows_out = tp if to_lag else n
    poison = BYTE_POISON if is_bool else WORD_POISON
    body = np.full((B, rows_in, n + pad_in), poison, src.dtype)
    body[:, :, :n] = src
    iraw = np.full(body.size + 2 * BAND, poison, src.dtype)
    iraw[BAND:-BAND] = body.ravel()
    rs = n + pad_out
    oraw = np.full(B * rows_out * rs + 2 * BAND, poison, src.dtype)
    _check(lib().emu_segment_lag(iraw.ctypes.data + src.itemsize * BAND, B, n, tp, src.itemsize, int(bool(to_lag)), n + pad_in,
                                 oraw.ctypes.data + src.itemsize * BAND, rs, int(grid)))
    got = _payload(oraw, B, rows_out, n, rs, "lag")
    assert (got != poison).all(), "a cell was not written"
    return got.view(np.bool_) if is_bool else got.view(a.dtype)


def raw_status(fn, *args):
    """The status of a prepare step for arguments that must not launch."""
    return getattr(lib(), fn)(*args)
