"""GPU twin of test_emu_mel2048_pairs.py: the pair contraction of ap_mel2048_run_kernel (hop 512).  Identical
clips through ap_melspec_rows_f32 must come out bit for bit identical although the waves' stretches start at
different rotations and clips end on either frame of a pair (the same frame runs on the pair path in one replica
and in the single-frame body in another); dense rows against line-padded rows; the oracle at the mel tolerance of
test_gpu_parity.py (rtol = atol = 1e-4); and a hand-made 4-pass bank through filterbank_spectrogram(), the
largest LDS carve-up ap_prepare_mel_run has to fit the parking planes into."""

import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import mlx_audio_primitives_amd as ap  # noqa: E402
from mlx_audio_primitives_amd import _extension as ext  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mel2048_pair_cases as pc  # noqa: E402
import mel2048_round_cases as rc  # noqa: E402

HOP = 512


def _rows(y, fb, plan, desc, power, T, Ts):
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
        ext.ptr(y), B, L, 2048, HOP, ext.ptr(win), ext.ptr(tw), 1, ext.PAD_MODES["constant"], T, Ts,
        ext.ptr(fb), ext.ptr(plan), desc.ctypes.data, M, float(power), ext.ptr(out), key.data_ptr(),
        ext.stream_ptr(dev)))
    k = int(key.cpu().numpy().view(np.uint32)[0])
    u = (k & 0x7FFFFFFF) if (k & 0x80000000) else (~k & 0xFFFFFFFF)          # ap_fkey_inv
    return out.cpu().numpy(), np.array([u], np.uint32).view(np.float32)[0]


def _bank_on_device(passes):
    fb_np, sr, kw, hand_made = rc.bank(passes)
    plan_np, desc = ext.mel_plan_host(fb_np)
    rc.check_plan(desc, fb_np.shape[0], passes)
    return fb_np, sr, kw, hand_made, torch.from_numpy(fb_np.copy()).cuda(), torch.from_numpy(plan_np).cuda(), desc


@pytest.mark.parametrize("L,n", [(9000, 7), (5200, 5)])
@pytest.mark.parametrize("power", rc.POWERS)
@pytest.mark.parametrize("passes", [3, 4])
def test_identical_clips_give_identical_bits(passes, power, L, n):
    """T = 18 (clips end on the second frame of a pair or on a single frame) and T = 11 (the first clip ends on
    the first frame of a pair); 126 frames in 16 stretches of about 8, 55 frames in 8 stretches of about 7."""
    assert torch.cuda.is_available() and ap.HAS_HIP_EXT
    fb_np, _, _, _, fb, plan, desc = _bank_on_device(passes)
    M = fb_np.shape[0]
    y1 = rc.signal(passes, HOP, L)[:1]
    y = torch.from_numpy(np.ascontiguousarray(np.repeat(y1, n, axis=0))).cuda()
    T = 1 + L // HOP
    Tp = -(-T // 8) * 8
    assert T % 8 != 0
    # the launcher's partition of this batch puts frames on the pair path in one replica, the single-frame one in another
    assert len(pc.on_both_paths(n, T, pc.gpu_workers(n * T))) >= 4
    assert ext.lib().ap_melspec_rows_fused(2048, HOP, 1, ext.PAD_MODES["constant"], M, float(power),
                                           ext.ptr(plan), desc.ctypes.data)      # the run kernel serves it
    dense, dmax = _rows(y, fb, plan, desc, power, T, T)
    padded, pmax = _rows(y, fb, plan, desc, power, T, Tp)
    for b in range(1, n):
        np.testing.assert_array_equal(dense[b], dense[0])
    np.testing.assert_array_equal(padded[:, :, :T], dense)
    assert np.all(padded[:, :, T:] == -777.0)       # nothing written between the rows
    assert dmax == dense.max() and pmax == dense.max()


@pytest.mark.parametrize("power", rc.POWERS)
def test_pair_contraction_against_oracle(monkeypatch, power):
    passes, L = 3, 9000
    fb_np, sr, kw, hand_made, fb, plan, desc = _bank_on_device(passes)
    y_np = rc.signal(passes, HOP, L)
    T = 1 + L // HOP
    R = rc.reference(monkeypatch, y_np, fb_np, sr, HOP, power, kw, hand_made)
    dense, dmax = _rows(torch.from_numpy(y_np).cuda(), fb, plan, desc, power, T, T)
    assert dense.shape == R.shape
    np.testing.assert_allclose(dense, R, rtol=1e-4, atol=1e-4)
    assert dmax == dense.max()
    pub = ap.melspectrogram(torch.from_numpy(y_np).cuda(), sr=sr, n_fft=2048, hop_length=HOP, power=power, **kw)
    np.testing.assert_array_equal(pub.cpu().numpy(), dense)


def test_four_pass_bank_through_filterbank_spectrogram(monkeypatch):
    """The largest weight table: exchange buffers + parking planes + tables have to fit the LDS of a CU."""
    fb_np, sr, kw, hand_made = rc.bank(4)
    _, desc = ext.mel_plan_host(fb_np)
    rc.check_plan(desc, fb_np.shape[0], 4)
    y_np = rc.signal(4, HOP, 9000)
    R = rc.reference(monkeypatch, y_np, fb_np, sr, HOP, 2.0, kw, hand_made)
    got = ap.filterbank_spectrogram(torch.from_numpy(y_np).cuda(), fb_np, n_fft=2048, hop_length=HOP, power=2.0)
    assert tuple(got.shape) == R.shape
    np.testing.assert_allclose(got.cpu().numpy(), R, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("power", rc.POWERS)
def test_reads_behind_the_parked_plane_are_zero(monkeypatch, power):
    """GPU twin of test_emu_reads_behind_the_parked_plane_are_zero: a bank with weight at bin 1024 (entries that read
    up to group 259 of the plane with zero weights).  First the hop-256 kernel runs on clips of NaN, enough frames
    for every CU, so that the exchange buffers it leaves in LDS are NaN where the hop-512 carve-up has its parking
    areas; then identical finite clips alternate with non-finite ones.  The finite clips come out finite, identical
    bit for bit, and right."""
    from oracle import audio_oracle as ao
    fb_np = pc.high_bin_bank()
    plan_np, desc = ext.mel_plan_host(fb_np)
    assert desc[12] <= 256 and desc[15] <= 4
    assert pc.reads_behind_the_plane(plan_np, desc) >= 257
    fb = torch.from_numpy(fb_np.copy()).cuda()
    plan = torch.from_numpy(plan_np).cuda()
    L, T, n = 5200, 11, 7
    assert "single" in pc.paths(n, T, pc.gpu_workers(n * T))[T - 1] and pc.on_both_paths(n, T, pc.gpu_workers(n * T))
    nan_clips = torch.full((2048, 2048), float("nan"), dtype=torch.float32, device="cuda")     # 9 frames each at hop 256
    ap.filterbank_spectrogram(nan_clips, fb_np, n_fft=2048, hop_length=256, power=power)
    torch.cuda.synchronize()
    x = rc.signal(3, HOP, L)[0]
    y_np = np.stack([x, np.full(L, np.nan, np.float32), x, np.full(L, np.inf, np.float32), x,
                     np.full(L, -np.inf, np.float32), x])
    dense, _ = _rows(torch.from_numpy(y_np).cuda(), fb, plan, desc, power, T, T)
    assert np.isfinite(dense[0::2]).all()
    for b in (2, 4, 6):
        np.testing.assert_array_equal(dense[b], dense[0])
    monkeypatch.setattr(ao, "mel_filterbank", lambda *a, **k: fb_np)
    R = ao.melspectrogram(x[None], sr=22050, n_fft=2048, hop_length=HOP, power=power, n_mels=128)
    np.testing.assert_allclose(dense[:1], R, rtol=1e-4, atol=1e-4)
