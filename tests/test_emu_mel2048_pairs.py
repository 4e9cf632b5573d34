"""CPU emulator: the pair contraction of ap_mel2048_run_kernel (hop 512: two frames per filterbank contraction,
the first frame's |X|^p plane parked behind the wave's exchange buffer, 8-byte partial-sum slots).

The emulator launches one workgroup of 8 waves, so a batch of N = B T frames is cut into 8 stretches that start
at frames N w / 8: the stretches enter at different rotations, and clips end on either frame of a pair.  Frames
at an odd entry rotation, before a clip end or a stretch end on the first frame of a pair take the single-frame
body; every frame must get the same bits on either path, which the replica tests check with identical clips."""

import os
import sys

import numpy as np
import pytest

from oracle import audio_oracle as ao

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import emu_bind as eb  # noqa: E402
import mel2048_pair_cases as pc  # noqa: E402
import mel2048_round_cases as rc  # noqa: E402

HOP = 512
LENGTHS = (9000, 600, 5000)          # T = 18, 2 and 10
WAVES = 8                            # stretches of an emulator launch


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("power", rc.POWERS)
@pytest.mark.parametrize("passes", [1, 2, 3, 4])
def test_emu_pair_contraction_against_oracle(monkeypatch, passes, power, L):
    fb, sr, kw, hand_made = rc.bank(passes)
    plan, desc = eb.mel_plan(fb)
    rc.check_plan(desc, fb.shape[0], passes)
    y = rc.signal(passes, HOP, L)
    win = ao.padded_window("hann", 2048, 2048)
    T = eb.n_frames(L, 2048, HOP, True)
    assert T == {9000: 18, 600: 2, 5000: 10}[L]
    R = rc.reference(monkeypatch, y, fb, sr, HOP, power, kw, hand_made)
    A = eb.melspec(y, 2048, HOP, win, fb, power=power)
    assert A.shape == R.shape == (rc.B, fb.shape[0], T)
    np.testing.assert_allclose(A, R, rtol=1e-4, atol=1e-4)


def _replicas(passes, power, L, n):
    fb, _, _, _ = rc.bank(passes)
    y1 = rc.signal(passes, HOP, L)[:1]
    y = np.ascontiguousarray(np.repeat(y1, n, axis=0))
    win = ao.padded_window("hann", 2048, 2048)
    A, amax = eb.melspec(y, 2048, HOP, win, fb, power=power, return_max=True)
    return A, amax


@pytest.mark.parametrize("power", rc.POWERS)
@pytest.mark.parametrize("passes", [3, 4])
def test_emu_pair_and_single_frame_paths_give_the_same_bits(passes, power):
    """7 identical clips of T = 18 frames: 126 frames in stretches that start at frames 0, 15, 31, 47, 63, 78,
    94 and 110 of the batch, which are frames 0, 15, 13, 11, 9, 6, 4 and 2 of their clips: entry rotations 0, 3,
    1, 3, 1, 2, 0 and 2.  By the loop's rules 8 of the 18 frames run on the pair path in one replica and on the
    single-frame path in another."""
    n, L, T = 7, 9000, 18
    assert len(pc.on_both_paths(n, T, WAVES)) >= 8, "the shape no longer puts the same frames on both paths"
    A, amax = _replicas(passes, power, L, n)
    assert A.shape[2] == T
    for b in range(1, n):
        np.testing.assert_array_equal(A[b], A[0])
    assert amax == A.max()


@pytest.mark.parametrize("power", rc.POWERS)
def test_emu_clip_end_on_the_first_frame_of_a_pair(monkeypatch, power):
    """T = 11: the first clip's last frame (t = 10) is the first frame of a pair and takes the single-frame body;
    the following clips then start at other rotations.  Against the oracle, and replicas bit for bit."""
    passes, L, T, n = 3, 5200, 11, 5
    assert "single" in pc.paths(n, T, WAVES)[T - 1] and pc.on_both_paths(n, T, WAVES)
    fb, sr, kw, hand_made = rc.bank(passes)
    A, amax = _replicas(passes, power, L, n)
    assert A.shape == (n, fb.shape[0], T)
    y1 = rc.signal(passes, HOP, L)[:1]
    R = rc.reference(monkeypatch, y1, fb, sr, HOP, power, kw, hand_made)
    np.testing.assert_allclose(A[:1], R, rtol=1e-4, atol=1e-4)
    for b in range(1, n):
        np.testing.assert_array_equal(A[b], A[0])
    assert amax == A.max()


def test_emu_parking_areas_stay_inside_the_lds():
    """4 passes carry the largest weight table: exchange buffers, parking planes and tables must fit lds_bytes."""
    fb, _, _, _ = rc.bank(4)
    win = ao.padded_window("hann", 2048, 2048)
    y = rc.signal(4, HOP, 9000)
    before = eb.lds_overruns()
    eb.melspec(y, 2048, HOP, win, fb, power=2.0)
    assert eb.lds_overruns() == before == 0


def _poison_lds():
    """Every byte of the emulator's LDS array 0xFF (NaN as float32): what an earlier kernel may have left behind."""
    import ctypes
    buf = (ctypes.c_ubyte * (160 * 1024)).in_dll(eb.lib(), "ap_smem")
    ctypes.memset(buf, 0xFF, 160 * 1024)


@pytest.mark.parametrize("power", rc.POWERS)
def test_emu_reads_behind_the_parked_plane_are_zero(monkeypatch, power):
    """A bank with weight at bin 1024: its entries read the groups up to 259 with zero weights, floats 1025 to 1039
    behind the plane.  In the exchange buffer those are the wave's own (finite) exchange data; behind the parked
    plane nobody writes them in the frame loop, so the kernel has to zero them and the parking area has to hold
    them.  LDS full of NaN before the launch, and non-finite clips between identical finite ones (whose waves
    work next door in LDS): the finite clips come out finite, identical bit for bit on both paths, and right."""
    fb = pc.high_bin_bank()
    plan, desc = eb.mel_plan(fb)
    assert desc[12] <= 256 and desc[15] <= 4 and fb.shape[0] <= 128          # the run kernel takes it
    assert pc.reads_behind_the_plane(plan, desc) >= 257
    L, T, n = 5200, 11, 7
    assert "single" in pc.paths(n, T, WAVES)[T - 1] and pc.on_both_paths(n, T, WAVES)
    x = rc.signal(3, HOP, L)[0]
    y = np.stack([x, np.full(L, np.nan, np.float32), x, np.full(L, np.inf, np.float32), x,
                  np.full(L, -np.inf, np.float32), x])
    win = ao.padded_window("hann", 2048, 2048)
    _poison_lds()
    A = eb.melspec(y, 2048, HOP, win, fb, power=power)
    assert np.isfinite(A[0::2]).all()
    for b in (2, 4, 6):
        np.testing.assert_array_equal(A[b], A[0])
    monkeypatch.setattr(ao, "mel_filterbank", lambda *a, **k: fb)
    R = ao.melspectrogram(x[None], sr=22050, n_fft=2048, hop_length=HOP, power=power, n_mels=128)
    np.testing.assert_allclose(A[:1], R, rtol=1e-4, atol=1e-4)
