"""GPU: cqt / vqt on the device against the float64 definition in tests/cqt_ref.py, with the bound of test_emu_cqt.py:
(d_k + 3) 2^-24 s_k sum |ypad| |g_k|, d_k from the tile constants of kernels_cqt.h (the emulator twin reports them).

The hand-built banks of test_emu_cqt.py go through the C entry on the device and must give the emulator's bits; the
real banks go through ap.cqt / ap.vqt.  What only the device shows: 1D / 2D / int16 input, a non-default stream, the
default configuration (84 bands, 97 to 11 685 taps) on one second of audio.  Worst error / bound seen on an MI355X:
0.046 on the hand-built banks (the emulator's bits), 0.036 on the real banks, 0.062 at the defaults (printed per case
with -s)."""

import os
import sys

import numpy as np
import pytest
import torch

import cqt_ref as R

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _extension as _x

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_cqt_bind as eb  # noqa: E402

pytestmark = pytest.mark.gpu

# every n_bins, T, hop and pad mode of the emulator's sweep at least once; the rest of the sweep is the emulator's
# and the hops at which a tile holds fewer than 32 frames (the signal ring: 31 at hop 521, 16 at 1024, 1 beyond 16128)
HAND = ((1, 33, 1), (5, 1, 512), (17, 65, 100), (17, 33, 64), (5, 65, 512), (1, 1, 64), (17, 65, 1), (5, 65, 521), (5, 33, 1024),
        (5, 3, 20000))
HAND_IDS = ["bins%d-T%d-hop%d" % c for c in HAND]


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def device_cqt(y, hop, mode, flat, off, m0, s, pad_out=0, stream=None):
    """ap_cqt_f32 on the device with a hand-built bank; the padded output rows start as NaN."""
    B, L = y.shape
    T = 1 + L // hop
    yd, td, od, md, sd = dev(y), dev(flat.view(np.float32)), dev(off), dev(m0), dev(s)
    out = torch.full((B, len(m0), T + pad_out), complex("nan+nanj"), dtype=torch.complex64, device="cuda")
    _x.check(_x.dlib(yd.device).ap_cqt_f32(_x.ptr(yd), B, L, hop, eb.PAD_MODES[mode], _x.ptr(td), _x.ptr(od), _x.ptr(md), _x.ptr(sd),
                                           len(m0), T, _x.ptr(out), T + pad_out, _x.stream_ptr(yd.device)))
    got = out.cpu().numpy()
    assert np.isnan(got[..., T:].view(np.float32)).all(), "a pad column was written"
    return np.ascontiguousarray(got[..., :T])


@pytest.mark.parametrize("case", HAND, ids=HAND_IDS)
def test_gpu_cqt_hand_banks_equal_the_emulator(case):
    n_bins, T, hop = case
    i = HAND.index(case)
    mode = R.PAD_MODES[i % 3]
    taps, m0, s = R.hand_bank(n_bins, 50 + i, centred=i % 2 == 0)
    flat, off = R.pack(taps)
    y = R.signal(2, R.hand_length(T, hop), seed=100 + i)
    got = device_cqt(y, hop, mode, flat, off, m0, s, pad_out=i % 3)
    emu = eb.cqt(y, hop, mode, flat, off, m0, s)
    want, A = R.transform(y, hop, mode, taps, m0, s)
    d = R.chain(m0, np.diff(off), eb.constants())
    assert R.sharp(np.diff(off), d)
    ratio = R.check(got, want, A, d, case)
    assert np.array_equal(got.view(np.uint32), emu.view(np.uint32)), "the device and the emulator differ in some bit"
    print(f"cqt hand {case} {mode}: worst error / bound {ratio:.4f}")


@pytest.mark.parametrize("mode", R.PAD_MODES)
def test_gpu_cqt_short_clip_every_pad_mode(mode):
    """L = 1500 < L_0 / 2: the padding reaches both ends of every frame of the 4103-tap filter."""
    taps, m0, s = R.hand_bank(5, 7, mode != "edge")
    flat, off = R.pack(taps)
    y = R.signal(2, 1500, seed=11)
    got = device_cqt(y, 100, mode, flat, off, m0, s, pad_out=1)
    want, A = R.transform(y, 100, mode, taps, m0, s)
    ratio = R.check(got, want, A, R.chain(m0, np.diff(off), eb.constants()), mode)
    assert np.array_equal(got.view(np.uint32), eb.cqt(y, 100, mode, flat, off, m0, s).view(np.uint32))
    print(f"cqt short clip {mode}: worst error / bound {ratio:.4f}")


@pytest.mark.parametrize("case", R.REAL_CASES, ids=R.REAL_IDS)
def test_gpu_cqt_real_banks(case):
    """ap.cqt / ap.vqt against the definition: three pad modes and hops, norm / scale variants on the first window."""
    name, func, kw = case
    f = getattr(ap, func)
    y = R.signal(2, 1100, seed=21)
    yd = dev(y)
    worst = 0.0
    variants = [dict()] + ([dict(norm=2, scale=False), dict(norm=None), dict(norm=np.inf, filter_scale=0.5), dict(tuning=0.3, bins_per_octave=24)]
                           if name == "hann" else [])
    for v, extra in enumerate(variants):
        full = dict(kw, **extra)
        ref_taps, ref_m0, ref_s = R.real_bank(func, full)
        d = R.chain(ref_m0, [len(g) for g in ref_taps], eb.constants())
        for i, (hop, mode) in enumerate(((64, "constant"), (100, "reflect"), (512, "edge"))):
            if (v + i) % 3 and v:
                continue
            got = f(yd, hop_length=hop, pad_mode=mode, **full)
            assert got.dtype == torch.complex64 and got.shape == (2, full["n_bins"], 1 + 1100 // hop) and got.is_cuda
            want, A = R.transform(y, hop, mode, ref_taps, ref_m0, ref_s)
            worst = max(worst, R.check(got.cpu().numpy(), want, A, d, (name, extra, hop, mode)))
    print(f"cqt real bank {name}: worst error / bound {worst:.4f}")


def test_gpu_cqt_input_kinds_and_streams():
    """1D input is row 0 of the batch; a host array; int16 PCM is its float32 value; a non-default stream."""
    kw = dict(sr=8000, fmin=500.0, n_bins=17, hop_length=100)
    y = R.signal(2, 3000, seed=4)
    base = ap.cqt(dev(y), **kw)
    assert base.shape == (2, 17, 31)
    for b in range(2):
        one = ap.cqt(dev(y[b]), **kw)
        assert one.shape == (17, 31) and torch.equal(one, base[b])
    assert torch.equal(ap.cqt(y, **kw), base) and torch.equal(ap.cqt(torch.from_numpy(y.copy()), **kw), base)
    assert torch.equal(ap.vqt(dev(y), gamma=0, **kw), base)
    assert not torch.equal(ap.vqt(dev(y), **kw), base)
    p16 = np.clip(np.round(y * 8000.0), -32768, 32767).astype(np.int16)
    want = ap.cqt(dev(p16.astype(np.float32) / 32768.0), **kw)
    for arr in (p16, dev(p16), p16[0]):
        got = ap.cqt(arr, **kw)
        assert torch.equal(got, want if arr.ndim == 2 else want[0])
    side = torch.cuda.Stream()
    yd = dev(y)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = ap.cqt(yd, **kw)
        twice = ap.cqt(yd, pad_mode="edge", **kw)
    side.synchronize()
    assert torch.equal(got, base) and torch.equal(twice, ap.cqt(yd, pad_mode="edge", **kw))


def test_gpu_cqt_defaults_on_cosines():
    """The default configuration, B = 1, L = 22050, T = 44, on unit cosines at f_0, f_24, f_83: on frames whose window
    lies inside the clip | |C[k, t]| - sqrt(N_k) / 2 | <= 1e-5 sqrt(N_k) / 2 + bound (the float64 definition itself
    deviates by up to 7e-6: the image at -f_k and the window's discreteness), and the bound on every element."""
    f, N, m0, Ls = R.lengths(22050, R.C1, 84)
    taps, m0, s = R.bank(22050, R.C1, 84)
    d = R.chain(m0, Ls, eb.constants())
    n = np.arange(22050, dtype=np.float64)
    worst = 0.0
    for k in (0, 24, 83):
        y = np.cos(2.0 * np.pi * f[k] * n / 22050.0).astype(np.float32)[None]
        got = ap.cqt(dev(y)).cpu().numpy()
        assert got.shape == (1, 84, 44)
        want, A = R.transform(y, 512, "constant", taps, m0, s)
        worst = max(worst, R.check(got, want, A, d, ("defaults", k)))
        t = np.arange(44) * 512
        inside = (t + m0[k] >= 0) & (t + m0[k] + Ls[k] <= 22050)
        assert inside.sum() >= 20
        peak = np.sqrt(N[k]) / 2.0
        bound = (d[k] + 3.0) * R.U * A[0, k, inside]
        assert np.all(np.abs(np.abs(got[0, k, inside].astype(np.complex128)) - peak) <= 1e-5 * peak + bound), (k, np.abs(got[0, k, inside]), peak)
        assert np.all(np.abs(got[0, k, inside]) > 1.8 * np.abs(got[0, k + 1 if k < 83 else k - 1, inside]))     # the neighbour reads about half
    print(f"cqt defaults on cosines: worst error / bound {worst:.4f}")


def test_gpu_cqt_scale_is_applied_last():
    """scale=False equals scale=True times sqrt(N_k) to 1 ulp: both scale the same sum S, fl(S fl(N_k)) against
    fl(S fl(sqrt N_k)); dividing the latter by its float32 scale in float64 leaves S (1 + e), |e| <= 2^-24, so the two
    differ by at most 2 2^-24 = one float32 epsilon, per component."""
    kw = dict(sr=8000, fmin=500.0, n_bins=17, hop_length=64)
    y = dev(R.signal(2, 2000, seed=8))
    a = ap.cqt(y, scale=True, **kw).cpu().numpy().view(np.float32).astype(np.float64)
    b = ap.cqt(y, scale=False, **kw).cpu().numpy().view(np.float32).astype(np.float64)
    _, N, _, _ = R.lengths(8000, 500.0, 17)
    s_true = np.sqrt(N).astype(np.float32).astype(np.float64)[None, :, None]
    s_false = N.astype(np.float32).astype(np.float64)[None, :, None]
    want = a / s_true * s_false
    assert np.all(np.abs(b - want) <= np.finfo(np.float32).eps * np.abs(want))
    assert np.abs(b).max() > 0
