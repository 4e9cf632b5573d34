"""CPU emulator: ap_mel2048_run_kernel with every contraction pass count the launcher instantiates (1 to 4)
and the run kernels' 18-complex twiddle rows, against the oracle.  Clip ends inside a
wave's stretch, T no multiple of 8, a clip shorter than a frame, both frame-loop shapes (hop 512: four
rotations; hop 256: one), power 2 and 1."""

import os
import sys

import numpy as np
import pytest

from oracle import audio_oracle as ao

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import emu_bind as eb  # noqa: E402
import mel2048_round_cases as rc  # noqa: E402


@pytest.mark.parametrize("L", rc.LENGTHS)
@pytest.mark.parametrize("hop", rc.HOPS)
@pytest.mark.parametrize("power", rc.POWERS)
@pytest.mark.parametrize("passes", [1, 2, 3, 4])
def test_emu_run_kernel_contraction_passes(monkeypatch, passes, power, hop, L):
    fb, sr, kw, hand_made = rc.bank(passes)
    plan, desc = eb.mel_plan(fb)
    assert (desc[12] + 63) // 64 == passes          # the pass count the launcher derives: no fallback unnoticed
    rc.check_plan(desc, fb.shape[0], passes)
    y = rc.signal(passes, hop, L)
    win = ao.padded_window("hann", 2048, 2048)
    T = eb.n_frames(L, 2048, hop, True)
    assert T % 8 != 0
    R = rc.reference(monkeypatch, y, fb, sr, hop, power, kw, hand_made)
    A = eb.melspec(y, 2048, hop, win, fb, power=power)
    assert A.shape == R.shape == (rc.B, fb.shape[0], T)
    np.testing.assert_allclose(A, R, rtol=1e-4, atol=1e-4)
    A2, amax = eb.melspec(y, 2048, hop, win, fb, power=power, return_max=True)
    np.testing.assert_array_equal(A2, A)
    assert amax == A.max()


def test_emu_spec_run_kernel_shares_the_twiddle_rows():
    """ap_spec2048_run_kernel takes the same apm_forward and table layout: once at hop 512."""
    L, Bn = 9000, 3
    rng = np.random.default_rng(5)
    t = np.arange(L) / 22050.0
    y = (0.5 * np.sin(2 * np.pi * 440.0 * t)[None] + 0.05 * rng.standard_normal((Bn, L))).astype(np.float32)
    win = ao.padded_window("hann", 2048, 2048)
    kw = dict(sr=22050, n_fft=2048, hop_length=512, center=True)
    got = eb.spectral_from_audio(y, 22050, 512, win, center=True)
    for b in range(Bn):
        # tolerances of test_emu_spectral_statistics_from_audio
        np.testing.assert_allclose(got["centroid"][b], ao.spectral_centroid(y[b], **kw)[0], rtol=2e-4, atol=1e-2)
        np.testing.assert_allclose(got["bandwidth"][b], ao.spectral_bandwidth(y[b], **kw)[0], rtol=2e-4, atol=1e-2)
        off = np.abs(got["rolloff"][b] - ao.spectral_rolloff(y[b], **kw)[0]) / (22050 / 2048)
        assert off.max() <= 1.001 and (off > 0.5).mean() < 0.02


def test_emu_run_kernels_stay_inside_their_lds():
    """The tables grew: the launch code's lds_bytes must cover them (emulator LDS guard).  The counter
    accumulates from the moment the library is loaded, so this test launches both run kernels itself, the
    mel one with the largest weight table (4 passes)."""
    fb, _, _, _ = rc.bank(4)
    win = ao.padded_window("hann", 2048, 2048)
    y = rc.signal(4, 512, 9000)
    before = eb.lds_overruns()
    eb.melspec(y, 2048, 512, win, fb, power=2.0)
    eb.spectral_from_audio(y, 22050, 512, win, center=True)
    assert eb.lds_overruns() == before == 0
