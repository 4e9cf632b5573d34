"""ctypes bindings for tests/emu/libapemu_features.so (TEST INFRASTRUCTURE ONLY).

Runs the feature kernels (kernels_features.h) on the CPU through the SIMT emulator of emu_shim.h.  Built on demand
with g++; never imported by the product package.

Every array a kernel sees is an interior slice of a larger one (`Guarded`): inputs are surrounded by NaN, so a read
outside the array poisons the result; outputs are pre-filled with the sentinel -777 and surrounded by it, so a write
outside the array - or an element never written - shows.  The slice starts a chosen number of elements (0..3) past a
16-byte boundary, which selects the kernels' 16-byte / 4-byte routes."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "mlx-audio-primitives_amd", "csrc")
LIB = os.path.join(HERE, "libapemu_features.so")

_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_f = ctypes.c_float

SENTINEL = -777.0
GUARD = 96                      # elements on either side

PAD_MODES = {"constant": 0, "edge": 1}
SG_MODES = {"interp": 0, "nearest": 1, "mirror": 2, "constant": 3, "wrap": 4}
EXT_MODES = {"constant": 0, "wrap": 1, "edge": 2, "smooth": 3, "symmetric": 4, "reflect": 5, "antisymmetric": 6,
             "antireflect": 7, "line": 8}
ROUTE_BLOCKS, ROUTE_SPAN = 1, 2


def build(force=False):
    srcs = [os.path.join(HERE, "emu_features.cpp"), os.path.join(CSRC, "host_builders.cpp")]
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
        L = ctypes.CDLL(build())
        L.emu_features_last_error.restype = ctypes.c_char_p
        L.ap_twiddle_table_host.argtypes = [_int, _p]
        L.emu_spectral_stats_f32.argtypes = [_p, _int, _i64, _i64, _i64, _p, _f, _p, _f, _int, _f, _f, _p, _p, _p, _p]
        L.emu_frame_stats_f32.argtypes = [_p, _i64, _i64, _int, _int, _int, _int, _i64, _p, _p, _int, _int, _p]
        L.emu_preemphasis_f32.argtypes = [_p, _i64, _i64, _f, _p, _p, _p, _int, _p]
        L.emu_deemphasis_workspace_floats.argtypes = [_i64, _i64]
        L.emu_deemphasis_workspace_floats.restype = _i64
        L.emu_deemphasis_f32.argtypes = [_p, _i64, _i64, _f, _p, _p, _p, _p, _int, _p]
        L.emu_savgol_f32.argtypes = [_p, _i64, _i64, _i64, _p, _int, _int, _f, _p, _p, _int, _int, _p]
        L.emu_extend_f32.argtypes = [_p, _i64, _i64, _i64, _int, _p, _int]
        L.emu_spectral_contrast_f32.argtypes = [_p, _i64, _i64, _i64, _p, _int, _int, _p]
        L.emu_acf_peaks_f32.argtypes = [_p, _i64, _int, _int, _int, _f, _f, _p, _p, _p]
        L.emu_pcm16_to_f32.argtypes = [_p, _i64, _f, _p, _int]
        L.emu_row_mean_f32.argtypes = [_p, _i64, _i64, _p]
        L.emu_autocorr_pad_f32.argtypes = [_p, _i64, _i64, _i64, _p, _p, _int]
        L.emu_power_spectrum_f32.argtypes = [_p, _i64, _int]
        L.emu_autocorr_finish_f32.argtypes = [_p, _i64, _i64, _i64, _int, _p, _int]
        L.emu_autocorrelation_nfft.argtypes = [_i64]
        L.emu_autocorrelation_nfft.restype = _i64
        L.emu_features_cfft_split.argtypes = [_i64, _p, _p]
        L.emu_autocorrelation_f32.argtypes = [_p, _i64, _i64, _i64, _int, _int, _p, _p, _p, _p]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise ValueError(lib().emu_features_last_error().decode())


class Guarded:
    """An array of `shape` inside a larger buffer, `off` elements past a 16-byte boundary."""

    def __init__(self, shape, dtype, fill, off=0, guard=GUARD):
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.n = int(np.prod(self.shape, dtype=np.int64))
        self.fill = fill
        item = np.dtype(dtype).itemsize
        per16 = 16 // item
        self.buf = np.full(self.n + 2 * guard + 2 * per16, fill, dtype)
        s = guard
        while ((self.buf.ctypes.data + s * item) % 16) != (off % per16) * item:
            s += 1
        self.s = s
        assert (self.ptr % 16) == (off % per16) * item

    @classmethod
    def of(cls, data, off=0, dtype=np.float32):
        data = np.ascontiguousarray(data, dtype)
        g = cls(data.shape, dtype, np.nan if np.dtype(dtype).kind == "f" else 12345, off)
        g.view[...] = data
        return g

    @classmethod
    def out(cls, shape, off=0, dtype=np.float32, fill=SENTINEL, guard=GUARD):
        return cls(shape, dtype, fill, off, guard)

    @property
    def ptr(self):
        return self.buf.ctypes.data + self.s * self.buf.itemsize

    @property
    def view(self):
        return self.buf[self.s:self.s + self.n].reshape(self.shape)

    def _same(self, a):
        return np.isnan(a) if isinstance(self.fill, float) and np.isnan(self.fill) else a == self.fill

    def bands_intact(self):
        return bool(self._same(self.buf[:self.s]).all() and self._same(self.buf[self.s + self.n:]).all())

    def result(self):
        """The interior, after checking that nothing outside it was written and every element of it was."""
        assert self.bands_intact(), "write outside the output array"
        v = self.view.copy()
        assert not (v == self.fill).any(), f"{int((v == self.fill).sum())} output elements never written"
        return v


def _opt(g):
    return None if g is None else g.ptr


def spectral_stats(S, freq, *, is_complex=False, power=1.0, p=2.0, norm=True, roll_percent=0.85, amin=1e-10,
                   centroid_in=None, want=("centroid", "bandwidth", "rolloff", "flatness"), off=0):
    """S (B, F, T) real or (B, F, T, 2) complex-as-pairs.  Returns {name: (B, T)} of the wanted statistics."""
    S = np.ascontiguousarray(S, np.float32)
    B, F, T = S.shape[:3]
    gS, gf = Guarded.of(S, 2 * (off % 2) if is_complex else off), Guarded.of(freq, off)
    gc = None if centroid_in is None else Guarded.of(np.asarray(centroid_in, np.float32).reshape(B, T))
    outs = {k: (Guarded.out((B, T), off) if k in want else None) for k in ("centroid", "bandwidth", "rolloff", "flatness")}
    _check(lib().emu_spectral_stats_f32(gS.ptr, int(is_complex), B, F, T, gf.ptr, power, _opt(gc), p, int(norm),
                                        roll_percent, amin, *[_opt(outs[k]) for k in
                                                              ("centroid", "bandwidth", "rolloff", "flatness")]))
    assert gS.bands_intact() and gf.bands_intact()
    return {k: g.result() for k, g in outs.items() if g is not None}


def n_frames(L, frame_length, hop, center):
    return 1 + (L + (2 * (frame_length // 2) if center else 0) - frame_length) // hop


def frame_stats(y, *, frame_length, hop, center=True, pad_mode="constant", rms=True, zcr=True, force_span=False, G=0,
                off=0):
    """(rms or None, zcr or None, route, G that ran) of a (B, L) batch; rows (B, T)."""
    y = np.ascontiguousarray(np.atleast_2d(y), np.float32)
    B, L = y.shape
    T = n_frames(L, frame_length, hop, center)
    gy = Guarded.of(y, off)
    gr = Guarded.out((B, T)) if rms else None
    gz = Guarded.out((B, T)) if zcr else None
    used = (ctypes.c_int * 2)()
    _check(lib().emu_frame_stats_f32(gy.ptr, B, L, frame_length, hop, int(center), PAD_MODES[pad_mode], T, _opt(gr),
                                     _opt(gz), int(force_span), int(G), used))
    assert gy.bands_intact()
    return (gr.result() if gr else None, gz.result() if gz else None, used[0], used[1])


def max_blocks():
    return int(lib().emu_features_max_blocks())


def _zi(zi, B):
    if zi is None:
        return None
    return Guarded.of(np.broadcast_to(np.asarray(zi, np.float32).reshape(-1), (B,)))


def preemphasis(y, *, coef=0.97, zi=None, want_zf=True, off_in=0, off_out=0, grid=0):
    """(out (B, L), zf (B) or None, four-samples kernel?)."""
    y = np.ascontiguousarray(np.atleast_2d(y), np.float32)
    B, L = y.shape
    gy, go, gzi = Guarded.of(y, off_in), Guarded.out((B, L), off_out), _zi(zi, B)
    gzf = Guarded.out((B,)) if want_zf else None
    used = (ctypes.c_int * 1)()
    _check(lib().emu_preemphasis_f32(gy.ptr, B, L, coef, _opt(gzi), go.ptr, _opt(gzf), grid, used))
    assert gy.bands_intact()
    return go.result(), (gzf.result() if gzf else None), bool(used[0])


def deemphasis(y, *, coef=0.97, zi=None, want_zf=True, off_in=0, off_out=0, force=0, workspace=True):
    """(out (B, L), zf (B) or None, chunked?).  force: 0 product's route, 1 one workgroup per clip, 2 chunked, 3 chunked
    with the second pass's workgroups in descending order."""
    y = np.ascontiguousarray(np.atleast_2d(y), np.float32)
    B, L = y.shape
    gy, go, gzi = Guarded.of(y, off_in), Guarded.out((B, L), off_out), _zi(zi, B)
    gzf = Guarded.out((B,)) if want_zf else None
    nws = int(lib().emu_deemphasis_workspace_floats(B, L))
    gws = Guarded.out((nws,)) if workspace else None
    used = (ctypes.c_int * 1)()
    _check(lib().emu_deemphasis_f32(gy.ptr, B, L, coef, _opt(gzi), go.ptr, _opt(gzf), _opt(gws), force, used))
    assert gy.bands_intact()
    if gws is not None:
        assert gws.bands_intact()
        if used[0]:
            gws.result()                                         # every chunk left its end state
    return go.result(), (gzf.result() if gzf else None), bool(used[0])


def savgol(x, taps, edge, *, mode="interp", cval=0.0, force_generic=False, grid=0, off=0):
    """x (outer, n, inner) filtered along the middle axis.  Returns (out, rows kernel?)."""
    x = np.ascontiguousarray(x, np.float32)
    outer, n, inner = x.shape
    taps = np.ascontiguousarray(taps, np.float32)
    # (a band as wide as a workgroup's chunk of the rows kernel: a last chunk that ran past the row would land in it)
    gx, gt, go = Guarded.of(x, off), Guarded.of(taps), Guarded.out(x.shape, off, guard=1100)
    ge = None if edge is None else Guarded.of(edge)
    used = (ctypes.c_int * 1)()
    _check(lib().emu_savgol_f32(gx.ptr, outer, n, inner, gt.ptr, len(taps), SG_MODES[mode], cval, _opt(ge), go.ptr,
                                int(force_generic), grid, used))
    assert gx.bands_intact() and gt.bands_intact()
    return go.result(), bool(used[0])


def extend(x, n_ext, mode, *, grid=0):
    x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
    B, L = x.shape
    gx, go = Guarded.of(x), Guarded.out((B, L + 2 * n_ext))
    _check(lib().emu_extend_f32(gx.ptr, B, L, n_ext, EXT_MODES[mode], go.ptr, grid))
    assert gx.bands_intact()
    return go.result()


def spectral_contrast(S, bands, *, linear=False):
    """S (B, F, T), bands (n, 3) int32 rows (lo, hi, k).  Returns (B, n, T)."""
    S = np.ascontiguousarray(S, np.float32)
    B, F, T = S.shape
    bands = np.ascontiguousarray(bands, np.int32)
    gS, gb = Guarded.of(S), Guarded.of(bands, dtype=np.int32)
    go = Guarded.out((B, bands.shape[0], T))
    _check(lib().emu_spectral_contrast_f32(gS.ptr, B, F, T, gb.ptr, bands.shape[0], int(linear), go.ptr))
    assert gS.bands_intact()
    assert go.bands_intact()
    return go.view.copy()                                        # NaN columns give NaN: no "never written" check here


def acf_peaks(r, *, min_lag, max_lag, threshold, sr, want=("f0", "voiced", "periodicity")):
    r = np.ascontiguousarray(np.atleast_2d(r), np.float32)
    rows, n_lag = r.shape
    gr = Guarded.of(r)
    gf = Guarded.out((rows,)) if "f0" in want else None
    gv = Guarded.out((rows,), dtype=np.uint8, fill=77) if "voiced" in want else None
    gp = Guarded.out((rows,)) if "periodicity" in want else None
    _check(lib().emu_acf_peaks_f32(gr.ptr, rows, n_lag, min_lag, max_lag, threshold, sr, _opt(gf), _opt(gv), _opt(gp)))
    assert gr.bands_intact()
    return {k: g.result() for k, g in (("f0", gf), ("voiced", gv), ("periodicity", gp)) if g is not None}


def pcm16(x, *, scale=1.0 / 32768.0, off_in=0, off_out=0, grid=0):
    x = np.ascontiguousarray(x, np.int16).reshape(-1)
    gx, go = Guarded.of(x, off_in, np.int16), Guarded.out((len(x),), off_out)
    _check(lib().emu_pcm16_to_f32(gx.ptr, len(x), scale, go.ptr, grid))
    assert gx.bands_intact()
    return go.result()


# ---- autocorrelation glue -------------------------------------------------------------------------------------------
def row_mean(y):
    y = np.ascontiguousarray(np.atleast_2d(y), np.float32)
    gy, go = Guarded.of(y, 1), Guarded.out((y.shape[0],))
    _check(lib().emu_row_mean_f32(gy.ptr, y.shape[0], y.shape[1], go.ptr))
    return go.result()


def autocorr_pad(y, N, mean=None, *, grid=0):
    y = np.ascontiguousarray(np.atleast_2d(y), np.float32)
    B, n = y.shape
    gy, go = Guarded.of(y, 1), Guarded.out((B, N))
    gm = None if mean is None else Guarded.of(mean)
    _check(lib().emu_autocorr_pad_f32(gy.ptr, B, n, N, _opt(gm), go.ptr, grid))
    return go.result()


def power_spectrum(X, *, grid=0):
    """X (..., 2) float32 pairs, in place on a copy."""
    X = np.ascontiguousarray(X, np.float32)
    g = Guarded.of(X)
    _check(lib().emu_power_spectrum_f32(g.ptr, X.size // 2, grid))
    assert g.bands_intact()
    return g.view.copy()


def autocorr_finish(r, max_lag, normalize, *, grid=0):
    r = np.ascontiguousarray(np.atleast_2d(r), np.float32)
    B, N = r.shape
    gr, go = Guarded.of(r), Guarded.out((B, max_lag))
    _check(lib().emu_autocorr_finish_f32(gr.ptr, B, N, max_lag, int(normalize), go.ptr, grid))
    return go.result()


def twiddles(n):
    tw = np.empty(2 * n, np.float32)
    _check(lib().ap_twiddle_table_host(n, tw.ctypes.data))
    return tw


def autocorrelation(y, max_lag, *, normalize=True, center=True):
    y = np.ascontiguousarray(np.atleast_2d(y), np.float32)
    B, n = y.shape
    N = int(lib().emu_autocorrelation_nfft(n))
    a, b = ctypes.c_int(), ctypes.c_int()
    if lib().emu_features_cfft_split(N, ctypes.byref(a), ctypes.byref(b)) != 0:
        raise ValueError("n_fft does not split")
    tw1, tw2 = twiddles(a.value), twiddles(b.value)
    gy, go = Guarded.of(y), Guarded.out((B, max_lag))
    gws = Guarded.out((4 * B * N + B,))
    _check(lib().emu_autocorrelation_f32(gy.ptr, B, n, max_lag, int(normalize), int(center), tw1.ctypes.data,
                                         tw2.ctypes.data, gws.ptr, go.ptr))
    assert gy.bands_intact() and gws.bands_intact()
    return go.result()


def lds_overruns():
    return int(lib().emu_features_lds_overruns())


def guard_selftest():
    return int(lib().emu_features_guard_selftest())
