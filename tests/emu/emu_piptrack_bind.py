"""ctypes bindings for tests/emu/libapemu_piptrack.so (TEST INFRASTRUCTURE ONLY).

Runs the piptrack kernel source (kernels_piptrack.h) on the CPU through the SIMT emulator of emu_shim.h.  Built on
demand with g++; never imported by the product package."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "mlx-audio-primitives_amd", "csrc")
LIB = os.path.join(HERE, "libapemu_piptrack.so")

_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_f = ctypes.c_float
_d = ctypes.c_double

BAND = 64          # NaN floats before and after every float buffer


def build(force=False):
    srcs = [os.path.join(HERE, "emu_piptrack.cpp")]
    deps = srcs + [os.path.join(HERE, "emu_shim.h"), os.path.join(ROOT, "include", "audioprims.h")] + [
        os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")
    ]
    if not force and os.path.exists(LIB):
        if os.path.getmtime(LIB) >= max(os.path.getmtime(d) for d in deps):
            return LIB
    tmp = f"{LIB}.{os.getpid()}.tmp"
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-pthread", "-o", tmp] + srcs)
    os.replace(tmp, LIB)
    return LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        _lib.emu_piptrack_last_error.restype = ctypes.c_char_p
        _lib.emu_piptrack_geometry.restype = ctypes.POINTER(ctypes.c_int)
        _lib.emu_piptrack_f32.argtypes = [_p, _int, _i64, _int, _i64, _i64, _int, _int, _f, _int, _f, _p, _f, _p, _p, _i64, _int]
        _lib.emu_piptrack_records_f32.argtypes = [_p, _int, _i64, _int, _i64, _i64, _int, _int, _f, _int, _f, _p, _f, _int, _p, _i64,
                                                  _p, _int]
        _lib.emu_piptrack_tuning_f32.argtypes = [_p, _p, _i64, _i64, _d, _p, _int, _p, _p, _int]
        _lib.emu_pitch_hist_f32.argtypes = [_p, _i64, _d, _p, _int, _p, _int]
    return _lib


class Status(ValueError):
    def __init__(self, rc, msg):
        super().__init__(msg)
        self.rc = rc


def _check(rc):
    if rc != 0:
        raise Status(rc, lib().emu_piptrack_last_error().decode())


def constants():
    """The tile constants of kernels_piptrack.h."""
    g = lib().emu_piptrack_geometry()
    return dict(tile=g[0], waves=g[1], ahead=g[2], stage=g[3], select_threads=g[4], hist_threads=g[5], max_bins=g[6])


def geometry():
    g = lib().emu_piptrack_geometry()
    return dict(grid=g[7], lds_bytes=g[8])


def _guarded(a):
    a = np.ascontiguousarray(a, np.float32).ravel()
    raw = np.full(a.size + 2 * BAND, np.nan, np.float32)
    raw[BAND:BAND + a.size] = a
    return raw, raw.ctypes.data + 4 * BAND


def _rows_in(x, pad):
    """x (B, F, T) float32 / complex64 with `pad` NaN columns behind every row: (raw, pointer, row stride, in_kind)."""
    B, F, T = x.shape
    rs = T + pad
    if np.iscomplexobj(x):
        body = np.full((B, F, rs), complex(np.nan, np.nan), np.complex64)
        body[:, :, :T] = x
        raw, ptr = _guarded(body.view(np.float32))
        return raw, ptr, rs, 1
    body = np.full((B, F, rs), np.nan, np.float32)
    body[:, :, :T] = x
    raw, ptr = _guarded(body)
    return raw, ptr, rs, 0


def ref_args(ref, B, T):
    """(ref_mode, ref_value, array kept alive, pointer) of piptrack's ref."""
    if ref is None:
        return 0, 0.0, None, None
    if np.ndim(ref) == 0:
        return 1, abs(float(np.float32(ref))), None, None
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(ref, np.float32), (B, T)))
    raw, ptr = _guarded(r)
    return 2, 0.0, raw, ptr


def _no_overrun():
    assert lib().emu_piptrack_lds_overruns() == 0, "LDS beyond the bytes the host asked for was written"


def dense(x, k_lo, k_hi, bin_hz, *, threshold=0.1, ref=None, pad_in=0, pad_out=0, grid=0):
    """(pitches, magnitudes) (B, F, T) float32 of x (B, F, T) float32 / complex64 through the emulated C entry.  Asserts
    that no band and no pad column was written and that every payload value was: x lies between NaN bands and NaN pad
    columns, so a read outside a row shows as a NaN (or a lost peak) in the frame that read it."""
    x = np.asarray(x)
    x = x.astype(np.complex64 if np.iscomplexobj(x) else np.float32)
    B, F, T = x.shape
    xraw, xptr, in_rs, kind = _rows_in(x, pad_in)
    mode, value, rraw, rptr = ref_args(ref, B, T)
    rs = T + pad_out
    outs = [np.full(B * F * rs + 2 * BAND, np.nan, np.float32) for _ in range(2)]
    _check(lib().emu_piptrack_f32(xptr, kind, B, F, T, in_rs, k_lo, k_hi, float(threshold), mode, value, rptr, float(bin_hz),
                                  outs[0].ctypes.data + 4 * BAND, outs[1].ctypes.data + 4 * BAND, rs, int(grid)))
    _no_overrun()
    got = []
    for o in outs:
        body = o[BAND:-BAND].reshape(B, F, rs)
        assert np.isnan(o[:BAND]).all() and np.isnan(o[-BAND:]).all() and np.isnan(body[:, :, T:]).all(), "a band or a pad column was written"
        got.append(body[:, :, :T].copy())
        assert not np.isnan(got[-1]).any(), "a value is NaN or was not written"
    return got[0], got[1]


def records(x, k_lo, k_hi, bin_hz, capacity, *, threshold=0.1, ref=None, per_clip=False, pad_in=0, grid=0):
    """(counters (G,) uint64, records (G, capacity, 2) float32, NaN where nothing was written) of the compact mode."""
    x = np.asarray(x)
    x = x.astype(np.complex64 if np.iscomplexobj(x) else np.float32)
    B, F, T = x.shape
    xraw, xptr, in_rs, kind = _rows_in(x, pad_in)
    mode, value, rraw, rptr = ref_args(ref, B, T)
    G = B if per_clip else 1
    rec = np.full(G * capacity * 2 + 2 * BAND, np.nan, np.float32)
    counters = np.full(G + 2, 0xDEADBEEF, np.uint64)
    _check(lib().emu_piptrack_records_f32(xptr, kind, B, F, T, in_rs, k_lo, k_hi, float(threshold), mode, value, rptr, float(bin_hz),
                                          int(per_clip), rec.ctypes.data + 4 * BAND, capacity, counters.ctypes.data + 8, int(grid)))
    _no_overrun()
    assert np.isnan(rec[:BAND]).all() and np.isnan(rec[-BAND:]).all(), "a band of the record buffer was written"
    assert counters[0] == 0xDEADBEEF and counters[-1] == 0xDEADBEEF, "a word beside the counters was written"
    return counters[1:-1].copy(), rec[BAND:-BAND].reshape(G, capacity, 2).copy()


def tuning(rec, counters, edges, bins_per_octave=12, *, grid=0):
    """(threshold (G,) float32, counts (G, n_bins) int64) of records (G, capacity, 2) and counters (G,)."""
    rec = np.ascontiguousarray(rec, np.float32)
    G, capacity, _ = rec.shape
    rraw, rptr = _guarded(rec)
    counters = np.ascontiguousarray(counters, np.uint64)
    edges = np.ascontiguousarray(edges, np.float64)
    n_bins = edges.size - 1
    thr = np.full(G + 2 * BAND, np.nan, np.float32)
    counts = np.full(G * n_bins + 2, 0xDEADBEEF, np.uint64)
    _check(lib().emu_piptrack_tuning_f32(rptr, counters.ctypes.data, G, capacity, float(bins_per_octave), edges.ctypes.data, n_bins,
                                         thr.ctypes.data + 4 * BAND, counts.ctypes.data + 8, int(grid)))
    _no_overrun()
    assert np.isnan(thr[:BAND]).all() and np.isnan(thr[-BAND:]).all()
    assert counts[0] == 0xDEADBEEF and counts[-1] == 0xDEADBEEF, "a word beside the counts was written"
    return thr[BAND:-BAND].copy(), counts[1:-1].reshape(G, n_bins).astype(np.int64)


def pitch_hist(f, edges, bins_per_octave=12, *, grid=0):
    """counts (n_bins,) int64 of the frequencies f."""
    fraw, fptr = _guarded(np.asarray(f, np.float32))
    n = np.asarray(f).size
    edges = np.ascontiguousarray(edges, np.float64)
    n_bins = edges.size - 1
    counts = np.full(n_bins + 2, 0xDEADBEEF, np.uint64)
    _check(lib().emu_pitch_hist_f32(fptr, n, float(bins_per_octave), edges.ctypes.data, n_bins, counts.ctypes.data + 8, int(grid)))
    _no_overrun()
    assert counts[0] == 0xDEADBEEF and counts[-1] == 0xDEADBEEF, "a word beside the counts was written"
    return counts[1:-1].astype(np.int64)


def raw_dense(args):
    """The status of the prepare step for arguments that must not launch."""
    return lib().emu_piptrack_f32(*args)
