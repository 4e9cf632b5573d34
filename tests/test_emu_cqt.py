"""CPU: the constant-Q kernel source (kernels_cqt.h) on the SIMT emulator of tests/emu, through the kernel's C ABI,
against the float64 definition in tests/cqt_ref.py.

Hand-built banks: random complex taps of equal magnitude 1 / L (every tap counts the same), lengths 1, 2, 63, 64, 65,
128, 277 and 4103 mixed so that a group of four bins holds unequal lengths, m0 centred and deliberately off-centre,
n_bins in {1, 5, 17} x T in {1, 33, 65} x hop in {1, 64, 100, 512} (and the hops beyond 520, where a tile of the kernel
holds fewer than 32 frames), two clips, NaN behind every padded output row and
around every input (emu_cqt_bind asserts that nothing outside the payload was written and no NaN was read).  Real
banks: the product's own packed bank (cqt.py) for sr = 8000, fmin = 500, 17 bins with hann / boxcar / hamming windows
and the vqt configuration, against the definition's float64 bank.

The bound is cqt_ref's, (d_k + 3) 2^-24 s_k sum |ypad| |g_k|, with d_k from the tile constants the twin reports
(d_k <= 104 for every case here); every accuracy test prints its worst error / bound with -s.  Worst seen on the
emulator: 0.056 on the hand-built banks, 0.036 on the real ones; on an MI355X (test_gpu_cqt.py) the hand-built banks
give the emulator's bits (0.046 on its cases), the defaults on a cosine 0.062.  Each test asserts cqt_ref.sharp():
1 / L_k >= 2 (d_k + 3) 2^-24, so one lost or doubled tap of an equal-magnitude bank leaves the bound
(test_emu_cqt_bound_sees_one_tap shows it).

Mutations of kernels_cqt.h tried, and the first test of this file each one fails:
  tap index off by one (j = m - m0 + 1)                      test_emu_cqt_hand[bins1-T1-hop100]
  chunk seam (the ring advances by samples one place late)   test_emu_cqt_hand[bins1-T33-hop512] (the first bank with L > 256)
  m0 sign (the tile's first sample at t0 hop - lo)           test_emu_cqt_hand[bins1-T1-hop64]
  reflect period 2 L - 1 (SciPy's "reflect", not NumPy's)    test_emu_cqt_hand[bins1-T33-hop100] (the first reflect case that pads)
  scale applied twice                                        test_emu_cqt_hand[bins1-T1-hop100]
  a lane left out of the reduction (31 of 32)                test_emu_cqt_hand[bins1-T1-hop512]
  the conjugate dropped                                      test_emu_cqt_hand[bins1-T1-hop100]
  edge padding takes y[L - 2] on the right                   test_emu_cqt_hand[bins1-T33-hop64]
  the ring's mirrored head not written                       test_emu_cqt_hops_beyond_the_ring[520-32]
  the ring's first fill one sample short                     test_emu_cqt_hand[bins1-T33-hop512]
"""

import importlib
import os
import sys

import numpy as np
import pytest

import cqt_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_cqt_bind as eb  # noqa: E402

# (T = 1 needs L < hop: there is no such clip at hop = 1)
FULL = [(n, T, hop) for n in (1, 5, 17) for T in (1, 33, 65) for hop in (1, 64, 100, 512) if (T, hop) != (1, 1)]
FULL_IDS = ["bins%d-T%d-hop%d" % c for c in FULL]


def run(y, hop, mode, bank, **kw):
    """(got, worst error / bound) of one emulated call against the definition; asserts the bound and its sharpness."""
    taps, m0, s = bank
    flat, off = R.pack(taps)
    got = eb.cqt(y, hop, mode, flat, off, m0, s, **kw)
    want, A = R.transform(y, hop, mode, taps, m0, s)
    d = R.chain(m0, np.diff(off), eb.constants())
    assert R.sharp(np.diff(off), d), (np.diff(off), d)
    return got, R.check(got, want, A, d, (hop, mode))


@pytest.mark.parametrize("case", FULL, ids=FULL_IDS)
def test_emu_cqt_hand(case):
    """Every (n_bins, T, hop): the pad mode, centred / off-centre m0 and dense / padded output rows rotate with the case."""
    n_bins, T, hop = case
    i = FULL.index(case)
    y = R.signal(2, R.hand_length(T, hop), seed=i)
    assert 1 + y.shape[1] // hop == T
    got, ratio = run(y, hop, R.PAD_MODES[i % 3], R.hand_bank(n_bins, i, centred=(i // 3) % 2 == 0), pad_out=(0, 3)[i % 2])
    assert got.shape == (2, n_bins, T)
    g = eb.geometry()
    assert g["n_groups"] == -(-n_bins // g["bins_per_group"]) and g["n_tt"] == -(-T // g["frames_per_tile"])
    assert g["grid"] == 2 * g["n_groups"] * g["n_tt"]
    print(f"cqt hand {case}: worst error / bound {ratio:.4f}")


@pytest.mark.parametrize("hop, frames", [(520, 32), (521, 31), (1024, 16), (16128, 2), (16129, 1), (20000, 1)])
def test_emu_cqt_hops_beyond_the_ring(hop, frames):
    """The signal ring holds 32 frames of a tile up to hop 520; beyond, a tile has as many frames as fit, down to one."""
    T = 2 * frames + 1
    y = R.signal(2, (T - 1) * hop + 5, seed=hop)
    got, ratio = run(y, hop, R.PAD_MODES[hop % 3], R.hand_bank(5, hop % 8, centred=hop % 2 == 0), pad_out=1)
    g = eb.geometry()
    assert got.shape == (2, 5, T) and g["frames_per_tile"] == frames and g["n_tt"] == 3
    print(f"cqt hop {hop}: worst error / bound {ratio:.4f}")


@pytest.mark.parametrize("mode", R.PAD_MODES)
def test_emu_cqt_short_clip_every_pad_mode(mode):
    """L = 1500 < L_0 / 2 = 2051: the padding reaches both ends of every frame of the longest filter, reflect more than
    once (the C entry reflects at any distance; the length precondition is the Python layer's).  Centred and off-centre."""
    worst = 0.0
    for centred in (True, False):
        bank = R.hand_bank(5, 7, centred)
        assert max(len(g) for g in bank[0]) == 4103
        y = R.signal(2, 1500, seed=11)
        got, ratio = run(y, 100, mode, bank, pad_out=1)
        assert got.shape == (2, 5, 16)
        worst = max(worst, ratio)
    print(f"cqt short clip {mode}: worst error / bound {worst:.4f}")


def test_emu_cqt_pad_modes_differ_only_where_the_padding_is_met():
    """The three modes give the same bits on frames whose taps all lie inside the clip, and differ elsewhere."""
    bank = R.hand_bank(5, 2, True)                              # longest: 277 taps
    y = R.signal(1, 2000, seed=3)
    outs = [run(y, 64, m, bank)[0] for m in R.PAD_MODES]
    reach = max(len(g) for g in bank[0]) // 2 + 1
    t = np.arange(outs[0].shape[-1]) * 64
    inside = (t - reach >= 0) & (t + reach <= 2000)
    assert inside.sum() > 10
    for o in outs[1:]:
        assert np.array_equal(o[..., inside], outs[0][..., inside])
        assert not np.array_equal(o[..., 0], outs[0][..., 0])


def test_emu_cqt_grid_override_and_batch_position():
    """Any number of workgroups gives the default grid's bits; a clip's bits do not depend on its place in the batch."""
    bank = R.hand_bank(17, 4, False)
    flat, off = R.pack(bank[0])
    y = R.signal(2, R.hand_length(33, 100), seed=5)
    base = eb.cqt(y, 100, "reflect", flat, off, bank[1], bank[2])
    default_grid = eb.geometry()["grid"]
    assert default_grid == 2 * 5 * 2
    for grid in (1, 3, 7, default_grid + 5):
        got = eb.cqt(y, 100, "reflect", flat, off, bank[1], bank[2], grid=grid, pad_out=2)
        assert eb.geometry()["grid"] == grid and np.array_equal(got.view(np.uint32), base.view(np.uint32))
    for b in range(2):
        got = eb.cqt(y[b:b + 1], 100, "reflect", flat, off, bank[1], bank[2])
        assert np.array_equal(got[0].view(np.uint32), base[b].view(np.uint32))
    # a band's bits do not depend on the bands that share its group only through the group's tap range:
    # the same band alone gives the definition too (checked by the bound), not necessarily the same bits
    k = 3
    alone = ([bank[0][k]], bank[1][k:k + 1], bank[2][k:k + 1])
    run(y, 100, "reflect", alone)


def test_emu_cqt_bound_sees_one_tap():
    """A signal of +-1 against equal-magnitude taps: the result with one tap of the longest filter zeroed, or one
    doubled, is outside the bound of the definition, the intact bank's far inside."""
    taps, m0, s = R.hand_bank(5, 7, True)
    rng = np.random.default_rng(9)
    y = np.where(rng.random((1, 6000)) < 0.5, -1.0, 1.0).astype(np.float32)
    want, A = R.transform(y, 512, "edge", taps, m0, s)
    flat, off = R.pack(taps)
    d = R.chain(m0, np.diff(off), eb.constants())
    R.check(eb.cqt(y, 512, "edge", flat, off, m0, s), want, A, d)
    for factor in (0.0, 2.0):
        for where in (0, 2051, 4102):
            broken = flat.copy()
            broken[off[0] + where] *= factor
            with pytest.raises(AssertionError):
                R.check(eb.cqt(y, 512, "edge", broken, off, m0, s), want, A, d)


@pytest.mark.parametrize("case", R.REAL_CASES, ids=R.REAL_IDS)
def test_emu_cqt_real_banks(case):
    """The product's packed bank through the kernel against the definition's own float64 bank: all three pad modes,
    hop below and above the filter lengths, norm / scale variants on the first window."""
    C = importlib.import_module("mlx_audio_primitives_amd.cqt")
    name, func, kw = case
    y = R.signal(2, 1100, seed=21)
    worst = 0.0
    variants = [dict()] + ([dict(norm=2, scale=False), dict(norm=None), dict(norm=np.inf, filter_scale=0.5), dict(tuning=0.3, bins_per_octave=24)]
                           if name == "hann" else [])
    for v, extra in enumerate(variants):
        full = dict(kw, **extra)
        gamma = None if func == "vqt" else 0.0
        args, _ = C._parameters(full["sr"], 512, full["fmin"], full["n_bins"], full.get("bins_per_octave", 12), full.get("tuning", 0.0),
                                full.get("filter_scale", 1), full.get("norm", 1), 0.01, full["window"], full.get("scale", True),
                                "constant", None, gamma, "equal")
        taps, off, m0, s, _ = C._bank(*args)
        ref_taps, ref_m0, ref_s = R.real_bank(func, full)
        assert np.array_equal(m0, ref_m0) and np.array_equal(np.diff(off), [len(g) for g in ref_taps])
        d = R.chain(m0, np.diff(off), eb.constants())
        for i, (hop, mode) in enumerate(((64, "constant"), (100, "reflect"), (512, "edge"))):
            if (v + i) % 3 and v:
                continue                                          # the variants take one mode each
            got = eb.cqt(y, hop, mode, taps, off, m0, s, pad_out=i)
            want, A = R.transform(y, hop, mode, ref_taps, ref_m0, ref_s)
            worst = max(worst, R.check(got, want, A, d, (name, extra, hop, mode)))
    print(f"cqt real bank {name}: worst error / bound {worst:.4f}")


def test_emu_cqt_rejects_before_launching():
    buf = np.zeros(4096, np.float32)
    y, o = buf.ctypes.data, buf.ctypes.data + 8192
    taps = np.ones(4, np.complex64)
    off = np.array([0, 2, 4], np.int64)
    m0 = np.zeros(2, np.int32)
    s = np.ones(2, np.float32)
    t, f, m, sc = taps.ctypes.data, off.ctypes.data, m0.ctypes.data, s.ctypes.data
    INVALID, UNSUPPORTED = -1, -2

    def rc(*a):
        return eb.cqt_raw(*a), eb.last_error()

    #          y  B   L  hop pad taps off m0 scale bins T out rs
    assert rc(y, 1, 64, 16, 0, t, f, m, sc, 2, 5, o, 5)[0] == 0
    for k in (0, 5, 6, 7, 8, 11):
        a = [y, 1, 64, 16, 0, t, f, m, sc, 2, 5, o, 5]
        a[k] = None
        assert rc(*a) == (INVALID, "cqt: NULL buffer")
    assert "non-empty" in rc(y, 0, 64, 16, 0, t, f, m, sc, 2, 5, o, 5)[1]
    assert "non-empty" in rc(y, 1, 0, 16, 0, t, f, m, sc, 2, 1, o, 5)[1]
    assert "hop_length must be positive" in rc(y, 1, 64, 0, 0, t, f, m, sc, 2, 5, o, 5)[1]
    assert "n_bins must be positive" in rc(y, 1, 64, 16, 0, t, f, m, sc, 0, 5, o, 5)[1]
    for pad in (-1, 3):
        assert "Unknown pad_mode" in rc(y, 1, 64, 16, pad, t, f, m, sc, 2, 5, o, 5)[1]
    for T in (4, 6):
        assert "n_frames mismatch" in rc(y, 1, 64, 16, 0, t, f, m, sc, 2, T, o, 6)[1]
    assert "out_row_stride" in rc(y, 1, 64, 16, 0, t, f, m, sc, 2, 5, o, 4)[1]
    r, msg = rc(y, 1, (1 << 30) + 1, 1 << 30, 0, t, f, m, sc, 2, 2, o, 2)
    assert r == UNSUPPORTED and "2^30" in msg
