"""CPU: the PCEN kernel source (kernels_pcen.h) on the SIMT emulator of tests/emu against the float64 definition in
tests/pcen_ref.py (scipy.signal.lfilter, scipy.ndimage.maximum_filter1d).

Every buffer lies between NaN bands and, in the padded-row variants, has NaN pad columns: emu_pcen_bind asserts that
none of them was written, that every payload value was, and that no NaN comes out (a read of a band or a pad column
would surface as one: the window maximum, the scan and the chain keep a NaN).

The bound is derived in pcen_ref's docstring from the roundings of the kernel's own scan (21 + 3 per tile crossed, in
units of 2^-24, relative to the non-negative smoother) propagated through the chain, with 2 ulp assumed per native
log2 / exp2 / rcp instruction.  Every accuracy test prints its worst error / bound with -s.  Worst seen: 0.21 on the
emulator (glibc's log2f / exp2f and a division in the instructions' place), 0.27 on an MI355X (test_gpu_pcen.py) for
the values, 0.15 / 0.15 for zf.  The yardsticks of pcen_ref.self_check(), same bound: SciPy's float32 lfilter with a
NumPy float32 log1p / expm1 chain 0.40 at b = 1e-3 (its smoother alone is at 1.22 of the smoother's share K u after 431
frames and keeps growing with T: 1 - b is rounded once and compounded); the textbook subtraction on quiet input 4.2e5,
a relative error of 170 %.

Mutations of kernels_pcen.h tried, and the first test of this file each one fails:
  carry power off by one (a^lane in every tile)             test_emu_pcen[1x65x65] (the first shape with T > 64)
  zf taken at lane 63 of the last tile                      test_emu_pcen[1x1x1]
  default state 1 instead of 1 - b                          test_emu_pcen[1x1x1]
  reflect off by one in the bin window (m - lo + 1)         test_emu_pcen_max_size[3x2x2]
  reflect with period 2 M - 1 (p - m for p - 1 - m)         test_emu_pcen_max_size[1x1x1]
  the textbook subtraction (x + bias)^power - bias^power    test_emu_pcen[1x1x1] (and test_emu_pcen_quiet_input)
  log1p as ln(fl(1 + u)), without Kahan's quotient          test_emu_pcen[1x1x1]
"""

import os
import sys

import numpy as np
import pytest

import pcen_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_pcen_bind as eb  # noqa: E402

IDS = ["x".join(map(str, s)) for s in R.SHAPES]
SMALL_IDS = ["x".join(map(str, s)) for s in R.SMALL]


def run(S, name, **kw):
    """(out, zf, parameters) through the emulator for a named parameter set; b = 0 gets the per-row state."""
    p = R.params(name)
    zi = kw.pop("zi", R.zi_for(S.shape) if p["b"] == 0.0 else None)
    got, zf = eb.pcen(S, zi=None if zi is None else np.asarray(zi)[..., 0], **p, **kw)
    return got, zf, p, zi


def test_reference_self_check():
    ratios = R.self_check()
    for k, v in ratios.items():
        print(f"pcen yardstick: {k}: {v:.3g}")
    assert ratios["textbook subtraction, quiet input, relative error"] > 1.0          # what the quiet case is there for


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_emu_pcen(shape):
    """Every parameter set on the small shapes, the defaults and b = 1e-3 on the long ones; dense and padded rows and
    one workgroup walking all rows in turn."""
    S = R.cases()["wide"][shape]
    worst = worst_zf = 0.0
    for k, name in enumerate(R.PARAMS if shape in R.SMALL else ("defaults", "b=1e-3")):
        pads = ((0, 0), (3, 5))[k % 2]
        got, zf, p, zi = run(S, name, pad_in=pads[0], pad_out=pads[1], grid=(k % 3 == 0))
        assert eb.geometry()["chain"] == (1 if p["power"] == 0 else 2 if p["bias"] == 0 else 0)
        r, rz, _ = R.check(got, zf, S, p, (shape, name), zi=zi)
        worst, worst_zf = max(worst, r), max(worst_zf, rz)
        if p["b"] == 0.0:                                   # the smoother stays at its state
            assert np.array_equal(zf, zi[..., 0])
    print(f"pcen {shape}: worst error / bound {worst:.3f}, zf {worst_zf:.3f}")


@pytest.mark.parametrize("kind", ["quiet", "zeros"])
def test_emu_pcen_quiet_input(kind):
    """S <= 1e-3, where (x + bias)^power - bias^power has no correct digit left in float32 (pcen_ref.textbook32 is at
    4e5 times this bound), and a third of the values exactly 0 with a silent row and silent leading tiles."""
    shape = R.QUIET_SHAPE
    S = R.cases()[kind][shape]
    worst = 0.0
    for name in ("defaults", "b=1e-3", "power=2", "bias=0", "power=0", "speech"):
        got, zf, p, zi = run(S, name, pad_in=1, pad_out=2)
        worst = max(worst, R.check(got, zf, S, p, (kind, name))[0])
        assert np.all((got == 0.0) == (S == 0.0))
    print(f"pcen {kind} input: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("shape", R.SMALL, ids=SMALL_IDS)
def test_emu_pcen_max_size(shape):
    """The running maximum over the reflected bin window, up to a window that wraps the whole axis twice."""
    S = R.cases()["wide"][shape]
    M = shape[1]
    worst = 0.0
    for k, ms in enumerate(R.max_sizes(M)):
        for name in ("defaults", "b=1"):                    # b = 1: Msm is the maximum itself
            p = R.params(name)
            got, zf = eb.pcen(S, max_size=ms, pad_in=(k % 2) * 3, pad_out=(k % 2) * 2, grid=k % 2, **p)
            worst = max(worst, R.check(got, zf, S, dict(p, max_size=ms), (shape, ms, name))[0])
    print(f"pcen max_size {shape}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("shape", [(3, 5, 64), (3, 3, 129)], ids=["3x5x64", "3x3x129"])
def test_emu_pcen_ref_and_zi(shape):
    """ref= replaces the running maximum whatever max_size says, dense and padded; a state that differs per row."""
    S = R.cases()["wide"][shape]
    ref = R.cases()["zeros"][shape]
    zi = R.zi_for(shape)
    worst = 0.0
    for pad_ref in (0, 4):
        for ms in (1, 3):
            p = R.params("defaults")
            got, zf = eb.pcen(S, ref=ref, max_size=ms, zi=zi[..., 0], pad_ref=pad_ref, pad_in=1, **p)
            worst = max(worst, R.check(got, zf, S, p, (shape, "ref", pad_ref, ms), zi=zi, ref=ref)[0])
    got, zf, p, _ = run(S, "b=1e-3", zi=zi)
    worst = max(worst, R.check(got, zf, S, p, (shape, "zi"), zi=zi)[0])
    assert not np.array_equal(got, run(S, "b=1e-3")[0])
    got, none = eb.pcen(S, want_zf=False, **p)                # zf not wanted
    assert none is None and np.array_equal(got, run(S, "b=1e-3")[0])
    print(f"pcen ref / zi {shape}: worst error / bound {worst:.3f}")


def test_emu_pcen_row_bits_depend_on_the_row_only():
    """A row's bits do not depend on the batch, on its position among the bands (max_size = 1), on the grid or on dense
    versus padded rows."""
    for shape in ((3, 5, 64), (3, 3, 129)):
        S = R.cases()["wide"][shape]
        B, M, T = shape
        for name in ("defaults", "bias=0"):
            base, zf, p, _ = run(S, name)
            for grid in (1, 2, 5):
                g, z = eb.pcen(S, grid=grid, pad_in=2, pad_out=7, **p)
                assert np.array_equal(g, base) and np.array_equal(z, zf)
            for b in range(B):
                g, z = eb.pcen(S[b:b + 1], **p)
                assert np.array_equal(g[0], base[b]) and np.array_equal(z[0], zf[b])
            perm = np.arange(M)[::-1]
            g, z = eb.pcen(S[:, perm], **p)
            assert np.array_equal(g[:, perm], base) and np.array_equal(z[:, perm], zf)
            g, z = eb.pcen(S.reshape(1, B * M, T), **p)
            assert np.array_equal(g.reshape(shape), base)
        base, zf = eb.pcen(S, max_size=3, **R.params("defaults"))
        for b in range(B):
            g, z = eb.pcen(S[b:b + 1], max_size=3, grid=1, pad_in=1, **R.params("defaults"))
            assert np.array_equal(g[0], base[b]) and np.array_equal(z[0], zf[b])


def test_emu_pcen_nan_reaches_later_frames_of_the_window_only():
    """A NaN at one (row, frame) changes the frames from its own on, in the rows whose bin window holds it; every
    other value keeps its bits."""
    for shape, (b0, m0, t0) in (((3, 5, 64), (1, 2, 17)), ((3, 3, 129), (2, 0, 64)), ((3, 3, 129), (0, 2, 128))):
        S = R.cases()["wide"][shape]
        bad = S.copy()
        bad[b0, m0, t0] = np.nan
        for ms in (1, 2, 3):
            p = R.params("defaults")
            clean, zf = eb.pcen(S, max_size=ms, **p)
            got, zf_bad = eb.pcen(bad, max_size=ms, allow_nan=True, **p)
            # row m sees rows m - ms // 2 .. m + (ms - 1) // 2
            rows = [m for m in range(shape[1]) if m - ms // 2 <= m0 <= m + (ms - 1) // 2]
            hit = np.zeros(shape, bool)
            hit[b0, rows, t0:] = True
            assert np.array_equal(np.isnan(got), hit), (shape, ms)
            assert np.array_equal(got[~hit], clean[~hit])
            zhit = np.zeros(shape[:2], bool)
            zhit[b0, rows] = True
            assert np.array_equal(np.isnan(zf_bad), zhit) and np.array_equal(zf_bad[~zhit], zf[~zhit])


@pytest.mark.parametrize("name", ["defaults", "b=1e-3", "power=0"])
def test_emu_pcen_chunks(name):
    """pcen(S[..., :k], return_zf) then pcen(S[..., k:], zi=zf): each piece within its bound of the offline float64
    reference (the second piece's state carries the first piece's error, k_in = K + 2), the last state included; the
    first piece has the bits of the offline call's first k frames.  (A cut at a multiple of the tile is not bit-identical:
    the state crosses a call as a Msm, rounded, and a tile as Msm.)"""
    shape = R.CHUNK_SHAPE
    S = R.cases()["wide"][shape]
    T = shape[2]
    p = R.params(name)
    want, zf64, _ = R.pcen(S, **p)
    whole, zf_whole = eb.pcen(S, **p)
    worst = 0.0
    for k in (1, 63, 64, 65, T - 1):
        head, zf_h = eb.pcen(S[..., :k], pad_in=1, **p)
        r0, _, k_zf = R.check(head, zf_h, S[..., :k], p, (name, k, "head"))
        tail, zf_t = eb.pcen(S[..., k:], zi=zf_h, pad_out=3, **p)
        # against the offline reference: the reference's own state at the cut, the bound with the incoming error
        zi64 = R.pcen(S[..., :k], **p)[1]
        r1, rz, _ = R.check(tail, zf_t, S[..., k:], p, (name, k, "tail"), zi=zi64, k_in=k_zf)
        np.testing.assert_allclose(R.pcen(S[..., k:], zi=zi64, **p)[0], want[..., k:], rtol=1e-12)
        assert np.array_equal(head, whole[..., :k])
        worst = max(worst, r0, r1, rz)
    print(f"pcen chunks {name}: worst error / bound {worst:.3f}")


def test_emu_pcen_rejects_before_launching():
    buf = np.zeros(4096, np.float32)
    s, o, z = buf.ctypes.data, buf.ctypes.data + 8192, buf.ctypes.data + 12288
    INVALID, UNSUPPORTED = -1, -2

    def rc(*a):
        return eb.pcen_raw(*a), eb.last_error()

    #          S  B  M  T rs ref rsr ms  b   gain bias power eps   zi  out rso zf
    assert rc(s, 1, 4, 8, 8, None, 0, 1, 0.5, 0.98, 2.0, 0.5, 1e-6, None, o, 8, None)[0] == 0
    assert rc(None, 1, 4, 8, 8, None, 0, 1, 0.5, 0.98, 2.0, 0.5, 1e-6, None, o, 8, None)[0] == INVALID
    assert rc(s, 1, 4, 8, 8, None, 0, 1, 0.5, 0.98, 2.0, 0.5, 1e-6, None, None, 8, None)[0] == INVALID
    for bad in ((0, 4, 8), (1, 0, 8), (1, 4, 0)):
        assert "non-empty" in rc(s, *bad, 8, None, 0, 1, 0.5, 0.98, 2.0, 0.5, 1e-6, None, o, 8, None)[1]
    for b in (-0.1, 1.5, float("nan")):
        assert "b must lie in [0, 1]" in rc(s, 1, 4, 8, 8, None, 0, 1, b, 0.98, 2.0, 0.5, 1e-6, None, o, 8, None)[1]
    assert "b = 0 needs zi" in rc(s, 1, 4, 8, 8, None, 0, 1, 0.0, 0.98, 2.0, 0.5, 1e-6, None, o, 8, None)[1]
    assert rc(s, 1, 4, 8, 8, None, 0, 1, 0.0, 0.98, 2.0, 0.5, 1e-6, z, o, 8, None)[0] == 0
    assert "gain must be" in rc(s, 1, 4, 8, 8, None, 0, 1, 0.5, -1.0, 2.0, 0.5, 1e-6, None, o, 8, None)[1]
    assert "bias must be" in rc(s, 1, 4, 8, 8, None, 0, 1, 0.5, 0.98, -2.0, 0.5, 1e-6, None, o, 8, None)[1]
    assert "power must be" in rc(s, 1, 4, 8, 8, None, 0, 1, 0.5, 0.98, 2.0, -0.5, 1e-6, None, o, 8, None)[1]
    for eps in (0.0, -1e-6, 1e-40):
        assert "eps must be" in rc(s, 1, 4, 8, 8, None, 0, 1, 0.5, 0.98, 2.0, 0.5, eps, None, o, 8, None)[1]
    for ms in (0, 256, -1):
        assert "max_size must be an integer in 1 .. 255" in rc(s, 1, 4, 8, 8, None, 0, ms, 0.5, 0.98, 2.0, 0.5, 1e-6, None, o, 8, None)[1]
    assert "row strides" in rc(s, 1, 4, 8, 7, None, 0, 1, 0.5, 0.98, 2.0, 0.5, 1e-6, None, o, 8, None)[1]
    assert "row strides" in rc(s, 1, 4, 8, 8, None, 0, 1, 0.5, 0.98, 2.0, 0.5, 1e-6, None, o, 7, None)[1]
    assert "row strides" in rc(s, 1, 4, 8, 8, s, 7, 1, 0.5, 0.98, 2.0, 0.5, 1e-6, None, o, 8, None)[1]
    assert "overlaps" in rc(s, 1, 4, 8, 8, None, 0, 1, 0.5, 0.98, 2.0, 0.5, 1e-6, None, s + 64, 8, None)[1]
    assert "zf overlaps" in rc(s, 1, 4, 8, 8, None, 0, 1, 0.5, 0.98, 2.0, 0.5, 1e-6, None, o, 8, o + 8)[1]
    # the padding behind the last row is not part of an input: an output right behind the last value is no overlap
    assert rc(s, 1, 4, 6, 8, None, 0, 1, 0.5, 0.98, 2.0, 0.5, 1e-6, None, s + 4 * 30, 8, None)[0] == 0
    assert "overlaps" in rc(s, 1, 4, 6, 8, None, 0, 1, 0.5, 0.98, 2.0, 0.5, 1e-6, None, s + 4 * 29, 8, None)[1]
    r, msg = rc(s, 1, (1 << 28) + 1, 8, 8, None, 0, 1, 0.5, 0.98, 2.0, 0.5, 1e-6, None, s + (1 << 50), 8, None)
    assert r == UNSUPPORTED and "2^28" in msg
