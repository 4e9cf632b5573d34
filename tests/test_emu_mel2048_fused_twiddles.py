"""CPU emulator: the n_fft = 2048 run kernels with every twiddle folded into the butterfly level that consumes
it (fft_lds.h "twiddles folded into the butterfly", kernels_mel2048.h apm_forward / apm_split).

* The scalar twins of the new primitives against complex128 arithmetic.
* Pure tones on the bins whose radix-4 groups sit where the read-side W_64 twiddle changes (c = g >> 4), on the
  mirrored groups and on the L = 0 lane, each alone in a clip and all mixed, through the box filterbank,
  against the oracle at rtol = atol = 1e-4.
* The accuracy bound: worst error of a frame against a float64 mel spectrogram, relative to the frame's largest
  mel value, over the cases of mel2048_round_cases.py, at most twice the parent commit's figure.  Each fused
  difference 2 a' - s carries one rounding more than a' - w b, of the size of the sum's own, so the error
  bound of a butterfly stage can at most double.
  Measured on the emulator: parent commit 3.2977e-07, this kernel 3.1659e-07 (profiles/README.md, round 6)."""

import os
import sys

import numpy as np
import pytest

from oracle import audio_oracle as ao

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import emu_bind as eb  # noqa: E402
import emu_fused_twiddles_bind as eft  # noqa: E402
import mel2048_fused_cases as fc  # noqa: E402
import mel2048_round_cases as rc  # noqa: E402

# worst_frame_error of the parent commit's run kernel (twiddles as complex multiplies of their own) on the
# emulator, over passes 1-4 x hops x powers x LENGTHS of mel2048_round_cases.py
PARENT_WORST_FRAME_ERROR = 3.2977e-07


def _c(a):
    return a[..., 0].astype(np.complex128) + 1j * a[..., 1].astype(np.complex128)


def test_fused_twiddle_primitives_against_complex128():
    """Every new primitive's scalar twin: a fixed chain of float32 FMAs, so a few float32 roundings of the
    largest intermediate (|a| + |w b| <= 2.7 here with |t| <= 2.42: bound 8 eps x 8)."""
    rng = np.random.default_rng(11)
    n = 4096
    rec = rng.uniform(-1.0, 1.0, (n, 6, 2)).astype(np.float32)
    ang = rng.uniform(0, 2 * np.pi, (n, 2))
    rec[:, 4, 0], rec[:, 4, 1] = np.cos(ang[:, 0]), np.sin(ang[:, 0])       # table form (c, s): w = c - i s
    rec[:, 5, 0], rec[:, 5, 1] = np.cos(ang[:, 1]), np.sin(ang[:, 1])
    a, b, x2, x3 = (_c(rec[:, i]) for i in range(4))
    wa, wb = np.conj(_c(rec[:, 4])), np.conj(_c(rec[:, 5]))
    tol = 64 * np.finfo(np.float32).eps
    # the W16 constants of finish_fused: (c, t) with w = c (1 - i t)
    consts = [(0.92387953251128675613, 0.41421356237309504880, 0.38268343236508977173, 2.41421356237309504880),
              (0.70710678118654752440, 1.0, -0.70710678118654752440, -1.0),
              (0.38268343236508977173, 2.41421356237309504880, -0.92387953251128675613, 0.41421356237309504880)]
    for ca, ta, cb, tb in consts:
        o = _c(eft.prims(rec, ca, ta, cb, tb))
        ka, kb = ca * (1 - 1j * ta), cb * (1 - 1j * tb)

        def fft4(v0, v1, v2, v3):
            return [v0 + v1 + v2 + v3, v0 - 1j * v1 - v2 + 1j * v3, v0 - v1 + v2 - v3, v0 + 1j * v1 - v2 - 1j * v3]

        want = [a + kb * b, a - kb * b, ka * a + kb * b, ka * a - kb * b,
                a + wb * b, a - wb * b, wa * a + wb * b, wa * a - wb * b]
        want += fft4(wa * a, wb * b, wb * x2, wa * x3)
        want += fft4(a, wb * b, wa * x2, wb * x3)
        want += fft4(a, ka * b, kb * x2, ca * (1 - 1j * tb) * x3)
        want += fft4(a, ka * b, -1j * x2, kb * x3)
        for i, w in enumerate(want):
            np.testing.assert_allclose(o[:, i], w, rtol=0, atol=tol, err_msg=f"output {i}, constants {ca, ta, cb, tb}")


@pytest.mark.parametrize("power", fc.POWERS)
@pytest.mark.parametrize("hop", fc.HOPS)
@pytest.mark.parametrize("which", list(range(len(fc.ALONE))) + ["mixed"])
def test_emu_run_kernel_tones_on_twiddle_groups(which, hop, power):
    y = fc.mixed() if which == "mixed" else fc.alone(which)
    win = ao.padded_window("hann", fc.N_FFT, fc.N_FFT)
    A = eb.melspec(y, fc.N_FFT, hop, win, fc.box_filterbank(), power=power)
    R = fc.box_reference(y, hop, power)
    assert A.shape == R.shape == (fc.B, 128, 1 + fc.L // hop)
    np.testing.assert_allclose(A, R, rtol=1e-4, atol=1e-4,
                               err_msg=f"bins {fc.TONE_BINS if which == 'mixed' else fc.ALONE[which]}")


def test_emu_run_kernel_accuracy_against_float64(monkeypatch):
    win = ao.padded_window("hann", 2048, 2048)
    worst = 0.0
    for passes in (1, 2, 3, 4):
        fb = rc.bank(passes)[0]
        plan, desc = eb.mel_plan(fb)
        rc.check_plan(desc, fb.shape[0], passes)                 # the run kernel serves it
        for hop in rc.HOPS:
            for power in rc.POWERS:
                for L in rc.LENGTHS:
                    y = rc.signal(passes, hop, L)
                    A = eb.melspec(y, 2048, hop, win, fb, power=power)
                    e = fc.worst_frame_error(A, fc.mel_f64(y, win, fb, hop, power))
                    print(f"passes {passes} hop {hop} power {power} L {L}: {e:.4e}")
                    worst = max(worst, e)
    print(f"worst frame error {worst:.4e}, parent {PARENT_WORST_FRAME_ERROR:.4e}")
    assert worst <= 2 * PARENT_WORST_FRAME_ERROR
