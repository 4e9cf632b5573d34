"""CPU: the YIN kernel source (kernels_yin.h) on the SIMT emulator of tests/emu, against the definition in
tests/yin_ref.py with the tolerances of test_gpu_yin.py.

A few frames per signal: the head of the clip (centred: the first frames are padded on the left), eight frames
from the middle (not centred) and the tail (centred: the last frames are padded on the right).  The grid is forced
small so that the frames of one call are spread over several waves and workgroups."""

import os
import sys

import numpy as np
import pytest

import yin_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_yin_bind as eb  # noqa: E402

SIGNALS = ["vibrato", "bursts", "noise"]
_signals = {}


def pieces(name, fl, hop):
    """(sub-clip, center) triples: head, middle eight frames, tail of the 2 s signal."""
    if not _signals:
        _signals.update(R.signals(R.SR, 2 * R.SR))
    y = _signals[name].astype(np.float32)
    mid = len(y) // 2
    return [(y[:fl + 3 * hop], True), (y[mid:mid + fl + 7 * hop], False), (y[-(fl + 3 * hop) - 5:], True)]


def check(name, shape, general, expect_wave):
    fl, hop, fmin, fmax = shape
    n_dec = n_all = 0
    for k, (y, center) in enumerate(pieces(name, fl, hop)):
        kw = dict(fmin=fmin, fmax=fmax, sr=R.SR, frame_length=fl, hop_length=hop, center=center, general=general,
                  grid=3)
        curve, wave_c = eb.yin_cmnd(y, **kw)
        f0, aper, wave_f = eb.yin(y, trough_threshold=R.THRESHOLD, **kw)
        assert wave_c == wave_f == expect_wave
        c = R.Case(y, fl, hop, fmin, fmax, center)
        c.compare(curve[0], f0[0], aper[0], f"{name} n={fl} piece {k} general={general}")
        n_dec += int(c.dec.sum())
        n_all += c.dec.size
    assert 2 * n_dec >= n_all, (name, n_dec, n_all)
    assert eb.lds_overruns() == 0


@pytest.mark.parametrize("shape", R.SHAPES[:2], ids=["n2048", "n1024"])
@pytest.mark.parametrize("name", SIGNALS)
def test_emu_wave_kernel(name, shape):
    check(name, shape, general=False, expect_wave=True)


def test_emu_other_shapes_take_the_general_kernel():
    for shape in R.SHAPES[2:]:
        check("vibrato", shape, general=False, expect_wave=False)
    check("vibrato", (2048, 511, 65.0, 2093.0), general=False, expect_wave=False)      # odd hop


@pytest.mark.parametrize("shape", R.SHAPES, ids=[f"n{s[0]}" for s in R.SHAPES])
@pytest.mark.parametrize("name", SIGNALS)
def test_emu_general_kernel(name, shape):
    check(name, shape, general=True, expect_wave=False)


def test_emu_batch_equals_single_and_scaling():
    """A clip alone and inside a batch give identical bits on both kernels (frames land on other waves and
    workgroups); d' of the wave kernel does not see an absolute scale (no floor on small magnitudes)."""
    for shape in R.SHAPES[:2]:
        batch_equals_single_and_scaling(shape)


def batch_equals_single_and_scaling(shape):
    fl, hop, fmin, fmax = shape
    ys = np.stack([pieces(n, fl, hop)[0][0] for n in SIGNALS])
    for general in (False, True):
        kw = dict(fmin=fmin, fmax=fmax, sr=R.SR, frame_length=fl, hop_length=hop, general=general)
        fb, ab, _ = eb.yin(ys, grid=2, **kw)
        cb, _ = eb.yin_cmnd(ys, grid=2, **kw)
        for i in range(len(SIGNALS)):
            f1, a1, _ = eb.yin(ys[i], grid=3, **kw)
            c1, _ = eb.yin_cmnd(ys[i], grid=1, **kw)
            assert np.array_equal(f1[0], fb[i]) and np.array_equal(a1[0], ab[i]) and np.array_equal(c1[0], cb[i])
    for scale in (1000.0, 1e-3):
        y = (scale * ys[0].astype(np.float64)).astype(np.float32)
        c = R.Case(y, fl, hop, fmin, fmax, True)
        curve, _ = eb.yin_cmnd(y, fmin=fmin, fmax=fmax, sr=R.SR, frame_length=fl, hop_length=hop)
        f0, aper, wave = eb.yin(y, fmin=fmin, fmax=fmax, sr=R.SR, frame_length=fl, hop_length=hop)
        assert wave
        c.compare(curve[0], f0[0], aper[0], f"vibrato x {scale}")
    assert eb.lds_overruns() == 0


@pytest.mark.parametrize("shape", R.SHAPES[:2], ids=["n2048", "n1024"])
@pytest.mark.parametrize("general", [False, True], ids=["wave", "general"])
def test_emu_all_zero_clip(general, shape):
    fl, hop, fmin, fmax = shape
    lo, hi, _ = R.periods(R.SR, fmin, fmax, fl)
    y = np.zeros((1, fl + 2 * hop + 1), np.float32)
    kw = dict(fmin=fmin, fmax=fmax, sr=R.SR, frame_length=fl, hop_length=hop, general=general)
    f0, aper, _ = eb.yin(y, **kw)
    curve, _ = eb.yin_cmnd(y, **kw)
    assert np.all(curve == 1.0) and np.all(aper == 1.0)
    assert np.all(f0 == np.float32(R.SR) / np.float32(lo))


@pytest.mark.parametrize("shape", R.SHAPES[:2], ids=["n2048", "n1024"])
def test_emu_center_equals_zero_padded_clip_and_kernels_agree(shape):
    fl, hop, fmin, fmax = shape
    y = pieces("bursts", fl, hop)[0][0]
    yp = np.pad(y, (fl // 2, fl // 2))
    kw = dict(fmin=fmin, fmax=fmax, sr=R.SR, frame_length=fl, hop_length=hop)
    got = {}
    for general in (False, True):
        ca, _ = eb.yin_cmnd(y, center=True, general=general, grid=2, **kw)
        cb, _ = eb.yin_cmnd(yp, center=False, general=general, grid=3, **kw)
        fa, aa, _ = eb.yin(y, center=True, general=general, grid=2, **kw)
        fb, ab, _ = eb.yin(yp, center=False, general=general, grid=3, **kw)
        assert np.array_equal(ca, cb) and np.array_equal(fa, fb) and np.array_equal(aa, ab)
        got[general] = ca
    atol = R.Case(y, fl, hop, fmin, fmax, True).atol
    err = float(np.abs(got[False] - got[True]).max())
    print(f"n={fl}: wave vs general curve {err:.3e} (atol {atol:.3e})")
    assert not np.array_equal(got[False], got[True]) and err <= atol


def test_emu_argument_checks():
    y = np.zeros((1, 4096), np.float32)
    with pytest.raises(ValueError, match="frame_length must be even"):
        eb.yin(y, fmin=65.0, fmax=2093.0, frame_length=2046 + 1, hop_length=512)
    with pytest.raises(ValueError, match="lag range"):
        eb.yin(y, fmin=100.0, fmax=700.0, frame_length=64, hop_length=16)
    with pytest.raises(ValueError, match="Signal length"):
        eb.yin(y[:, :100], fmin=65.0, fmax=2093.0, center=False)
