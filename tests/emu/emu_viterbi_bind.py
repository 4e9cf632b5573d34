"""ctypes bindings for tests/emu/libapemu_viterbi.so (TEST INFRASTRUCTURE ONLY).

Runs the sequence-decoding kernel source (kernels_viterbi.h) on the CPU through the SIMT emulator of emu_shim.h.  Built
on demand with g++; never imported by the product package.  Every buffer lies between poisoned bands, the rows of prob
have NaN pad columns behind them (a read there puts a NaN into an emission and raises the flag), and LDS beyond the
bytes the host asked for is watched."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "mlx-audio-primitives_amd", "csrc")
LIB = os.path.join(HERE, "libapemu_viterbi.so")
SRC = os.path.join(HERE, "emu_viterbi.cpp")

_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int

BAND = 64           # poisoned elements before and after every buffer
POISON = {np.dtype(np.float32): np.nan, np.dtype(np.float64): np.nan, np.dtype(np.uint16): 0xEEEE, np.dtype(np.uint32): 0xEEEEEEEE,
          np.dtype(np.int32): -(2 ** 31)}


def compile_lib(out, src=SRC):
    tmp = f"{out}.{os.getpid()}.tmp"
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-pthread", "-I", HERE, "-o", tmp, src])
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
    L.emu_viterbi_last_error.restype = ctypes.c_char_p
    L.emu_viterbi_geometry.restype = ctypes.POINTER(ctypes.c_int)
    L.emu_viterbi_emission_f32.argtypes = [_p, _i64, _i64, _i64, _i64, _int, _p, _p, _p, _int]
    L.emu_viterbi_decode_f32.argtypes = [_p, _i64, _i64, _i64, _p, _p, _p, _p, _p, _int, _int]
    L.emu_viterbi_binary_f32.argtypes = [_p, _i64, _i64, _i64, _p, _int, _p, _p, _p, _p, _int]
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = declare(ctypes.CDLL(build()))
    return _lib


class Status(ValueError):
    def __init__(self, rc, msg):
        super().__init__(msg)
        self.rc = rc


def _check(rc):
    if rc != 0:
        raise Status(rc, lib().emu_viterbi_last_error().decode())


def last_error():
    return lib().emu_viterbi_last_error().decode()


def constants():
    """The constants of kernels_viterbi.h."""
    g = lib().emu_viterbi_geometry()
    names = ("block", "max_states", "max_steps", "max_g", "chunk", "lt_lds_max", "emission_tile", "word", "labels")
    return {n: g[i] for i, n in enumerate(names)}


def geometry():
    """What the prepare step chose for the last call."""
    g = lib().emu_viterbi_geometry()
    return dict(grid=g[9], lds_bytes=g[10], lanes_per_state=g[11], lt_lds=g[12])


def _is_poison(a):
    fill = POISON[a.dtype]
    return np.isnan(a) if a.dtype.kind == "f" else a == np.array(fill).astype(a.dtype)


def _guarded(a):
    """(raw array with poisoned bands, pointer to the payload) of an input array."""
    a = np.ascontiguousarray(a).ravel()
    raw = np.full(a.size + 2 * BAND, POISON[a.dtype], a.dtype)
    raw[BAND:BAND + a.size] = a
    return raw, raw.ctypes.data + a.dtype.itemsize * BAND


def _out(n, dtype):
    """(raw, pointer) of an output of n elements: poison everywhere."""
    raw = np.full(n + 2 * BAND, POISON[np.dtype(dtype)], dtype)
    return raw, raw.ctypes.data + raw.dtype.itemsize * BAND


def _payload(raw, shape, what, written=True):
    assert _is_poison(raw[:BAND]).all() and _is_poison(raw[-BAND:]).all(), f"{what}: a band was written"
    assert lib().emu_viterbi_lds_overruns() == 0, "LDS beyond the bytes the host asked for was written"
    body = raw[BAND:-BAND].reshape(shape).copy()
    if written:
        assert not _is_poison(body).any(), f"{what}: an element is poison or was not written"
    return body


def emission(prob, mode, lps=None, *, pad=0, grid=0):
    """(E float32 (B, T, S) or (B, T, S, 2), flags int32 (B)) of prob (B, S, T) through the emulated C entry; `pad` NaN
    columns behind every row of prob."""
    prob = np.asarray(prob, np.float32)
    B, S, T = prob.shape
    body = np.full((B, S, T + pad), np.nan, np.float32)
    body[:, :, :T] = prob
    praw, pptr = _guarded(body)
    lraw, lptr = (None, None) if lps is None else _guarded(np.asarray(lps, np.float32))
    shape = (B, T, S, 2) if mode == 2 else (B, T, S)
    eraw, eptr = _out(int(np.prod(shape)), np.float32)
    fraw, fptr = _out(B, np.int32)
    _check(lib().emu_viterbi_emission_f32(pptr, B, S, T, T + pad, int(mode), lptr, eptr, fptr, int(grid)))
    flags = _payload(fraw, (B,), "flags")
    E = _payload(eraw, shape, "E", written=False)           # a NaN emission is legitimate where the input is out of range
    for b in range(B):
        assert flags[b] & 1 or not np.isnan(E[b]).any(), f"sequence {b}: an emission is NaN or was not written"
    return E, flags


def decode(E, lt, li, *, lt_lds_max=None, grid=0):
    """(ptr uint16 (B, T, S), states int32 (B, T), logp float64 (B)) of E (B, T, S) through the emulated C entry."""
    E = np.asarray(E, np.float32)
    B, T, S = E.shape
    eraw, eptr = _guarded(E)
    traw, tptr = _guarded(np.asarray(lt, np.float32))
    iraw, iptr = _guarded(np.asarray(li, np.float32))
    praw, pptr = _out(B * T * S, np.uint16)
    sraw, sptr = _out(B * T, np.int32)
    lraw, lptr = _out(B, np.float64)
    cap = constants()["lt_lds_max"] if lt_lds_max is None else int(lt_lds_max)
    _check(lib().emu_viterbi_decode_f32(eptr, B, S, T, tptr, iptr, pptr, sptr, lptr, cap, int(grid)))
    return _payload(praw, (B, T, S), "ptr"), _payload(sraw, (B, T), "states"), _payload(lraw, (B,), "logp")


def binary(E, lt, li, *, grid=0):
    """(bits uint32 (B, ceil(T / 16), S), states int32 (B, S, T), logp float64 (B, S)) of E (B, T, S, 2); lt (2, 2) shared
    or (S, 2, 2) per label."""
    E = np.asarray(E, np.float32)
    B, T, S, _ = E.shape
    lt = np.asarray(lt, np.float32)
    eraw, eptr = _guarded(E)
    traw, tptr = _guarded(lt)
    iraw, iptr = _guarded(np.asarray(li, np.float32))
    nw = (T + 15) // 16
    braw, bptr = _out(B * nw * S, np.uint32)
    sraw, sptr = _out(B * S * T, np.int32)
    lraw, lptr = _out(B * S, np.float64)
    _check(lib().emu_viterbi_binary_f32(eptr, B, S, T, tptr, int(lt.ndim == 3), iptr, bptr, sptr, lptr, int(grid)))
    return _payload(braw, (B, nw, S), "bits"), _payload(sraw, (B, S, T), "states"), _payload(lraw, (B, S), "logp")


def emission_raw(prob_ptr, B, S, T, rs, mode, lps_ptr, e_ptr, flags_ptr):
    """The status of the prepare step for arguments that must not launch."""
    return lib().emu_viterbi_emission_f32(prob_ptr, B, S, T, rs, mode, lps_ptr, e_ptr, flags_ptr, 0)


def decode_raw(e_ptr, B, S, T, lt_ptr, li_ptr, ptr_ptr, states_ptr, logp_ptr):
    return lib().emu_viterbi_decode_f32(e_ptr, B, S, T, lt_ptr, li_ptr, ptr_ptr, states_ptr, logp_ptr, 0, 0)


def binary_raw(e_ptr, B, S, T, lt_ptr, li_ptr, bits_ptr, states_ptr, logp_ptr):
    return lib().emu_viterbi_binary_f32(e_ptr, B, S, T, lt_ptr, 0, li_ptr, bits_ptr, states_ptr, logp_ptr, 0)
