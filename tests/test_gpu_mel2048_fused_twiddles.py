"""GPU twin of test_emu_mel2048_fused_twiddles.py: ap_mel2048_run_kernel with the twiddles folded into the
butterflies, through ap_melspec_rows_f32.  Pure tones on the radix-4 groups where the read-side W_64 twiddle
changes, on the mirrored groups and on the L = 0 lane (each alone in a clip, and all mixed) through the box
filterbank, and the noise signal of the three-pass mel bank, against the oracle at rtol = atol = 1e-4; dense
rows against line-padded rows bit for bit."""

import os
import sys

import numpy as np
import pytest

from oracle import audio_oracle as ao

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import mlx_audio_primitives_amd as ap  # noqa: E402
from mlx_audio_primitives_amd import _extension as ext  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mel2048_fused_cases as fc  # noqa: E402
import mel2048_round_cases as rc  # noqa: E402


def _rows(y, fb, plan, desc, hop, power, T, Ts):
    """ap_melspec_rows_f32 into a (B, M, Ts) buffer pre-filled with a marker."""
    from mlx_audio_primitives_amd.stft import _get_padded_window, _get_twiddles
    dev = y.device
    B, L = y.shape
    M = fb.shape[0]
    win = _get_padded_window("hann", 2048, 2048, dev)
    tw = _get_twiddles(2048, dev)
    out = torch.full((B, M, Ts), -777.0, dtype=torch.float32, device=dev)
    key = torch.zeros(1, dtype=torch.int32, device=dev)
    ext.check(ext.dlib(dev).ap_melspec_rows_f32(
        ext.ptr(y), B, L, 2048, hop, ext.ptr(win), ext.ptr(tw), 1, ext.PAD_MODES["constant"], T, Ts,
        ext.ptr(fb), ext.ptr(plan), desc.ctypes.data, M, float(power), ext.ptr(out), key.data_ptr(),
        ext.stream_ptr(dev)))
    return out.cpu().numpy()


def _check(y_np, fb_np, R, hop, power, what):
    assert torch.cuda.is_available() and ap.HAS_HIP_EXT
    plan_np, desc = ext.mel_plan_host(fb_np)
    M = fb_np.shape[0]
    assert ext.lib().ap_melspec_rows_fused(2048, hop, 1, ext.PAD_MODES["constant"], M, float(power),
                                           ext.ptr(torch.from_numpy(plan_np).cuda()), desc.ctypes.data)
    y = torch.from_numpy(y_np).cuda()
    fb = torch.from_numpy(fb_np.copy()).cuda()
    plan = torch.from_numpy(plan_np).cuda()
    T = 1 + y_np.shape[1] // hop
    Tp = -(-T // 8) * 8
    assert T % 8 != 0
    dense = _rows(y, fb, plan, desc, hop, power, T, T)
    padded = _rows(y, fb, plan, desc, hop, power, T, Tp)
    assert dense.shape == R.shape
    np.testing.assert_allclose(dense, R, rtol=1e-4, atol=1e-4, err_msg=what)
    np.testing.assert_array_equal(padded[:, :, :T], dense)
    assert np.all(padded[:, :, T:] == -777.0)


@pytest.mark.parametrize("power", fc.POWERS)
@pytest.mark.parametrize("hop", fc.HOPS)
def test_run_kernel_tones_on_twiddle_groups(hop, power):
    fb = fc.box_filterbank()
    for i in range(len(fc.ALONE)):
        y = fc.alone(i)
        _check(y, fb, fc.box_reference(y, hop, power), hop, power, f"bins {fc.ALONE[i]}")
    y = fc.mixed()
    _check(y, fb, fc.box_reference(y, hop, power), hop, power, "all tones mixed")


@pytest.mark.parametrize("power", fc.POWERS)
@pytest.mark.parametrize("hop", fc.HOPS)
def test_run_kernel_noise(monkeypatch, hop, power):
    fb, sr, kw, hand_made = rc.bank(3)
    y = rc.signal(3, hop, 9000)
    _check(y, fb, rc.reference(monkeypatch, y, fb, sr, hop, power, kw, hand_made), hop, power, "noise")
