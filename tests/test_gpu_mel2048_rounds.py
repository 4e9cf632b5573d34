"""GPU twin of test_emu_mel2048_rounds.py: ap_mel2048_run_kernel with 1 to 4 contraction passes, both
frame-loop shapes, power 2 and 1, clips that end inside a wave's stretch and a clip shorter than a frame -
against the oracle at the mel tolerance of test_gpu_parity.py (rtol = atol = 1e-4), dense rows against
line-padded rows bit for bit, and the public melspectrogram() on the banks it can build."""

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
import mel2048_round_cases as rc  # noqa: E402


def _rows(y, fb, plan, desc, hop, power, T, Ts):
    """ap_melspec_rows_f32: (B, M, Ts) buffer pre-filled with a marker, and max(out) from the kernel's key."""
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
    k = int(key.cpu().numpy().view(np.uint32)[0])
    u = (k & 0x7FFFFFFF) if (k & 0x80000000) else (~k & 0xFFFFFFFF)          # ap_fkey_inv
    return out.cpu().numpy(), np.array([u], np.uint32).view(np.float32)[0]


@pytest.mark.parametrize("L", rc.LENGTHS)
@pytest.mark.parametrize("hop", rc.HOPS)
@pytest.mark.parametrize("power", rc.POWERS)
@pytest.mark.parametrize("passes", [1, 2, 3, 4])
def test_run_kernel_contraction_passes(monkeypatch, passes, power, hop, L):
    assert torch.cuda.is_available() and ap.HAS_HIP_EXT
    fb_np, sr, kw, hand_made = rc.bank(passes)
    plan_np, desc = ext.mel_plan_host(fb_np)
    assert (desc[12] + 63) // 64 == passes          # the pass count the launcher derives: no fallback unnoticed
    rc.check_plan(desc, fb_np.shape[0], passes)
    M = fb_np.shape[0]
    y_np = rc.signal(passes, hop, L)
    y = torch.from_numpy(y_np).cuda()
    fb = torch.from_numpy(fb_np.copy()).cuda()
    plan = torch.from_numpy(plan_np).cuda()
    T = 1 + L // hop
    Tp = -(-T // 8) * 8
    assert T % 8 != 0
    assert ext.lib().ap_melspec_rows_fused(2048, hop, 1, ext.PAD_MODES["constant"], M, float(power),
                                           ext.ptr(plan), desc.ctypes.data)      # the run kernel serves it
    R = rc.reference(monkeypatch, y_np, fb_np, sr, hop, power, kw, hand_made)
    dense, dmax = _rows(y, fb, plan, desc, hop, power, T, T)
    padded, pmax = _rows(y, fb, plan, desc, hop, power, T, Tp)
    assert dense.shape == R.shape
    np.testing.assert_allclose(dense, R, rtol=1e-4, atol=1e-4)
    np.testing.assert_array_equal(padded[:, :, :T], dense)
    assert np.all(padded[:, :, T:] == -777.0)       # nothing written between the rows
    assert dmax == dense.max() and pmax == dense.max()
    if not hand_made:
        pub = ap.melspectrogram(y, sr=sr, n_fft=2048, hop_length=hop, power=power, **kw)
        np.testing.assert_array_equal(pub.cpu().numpy(), dense)
