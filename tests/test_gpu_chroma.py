"""GPU: the chroma kernels on the device against the float64 definitions and the derived bound of tests/chroma_ref.py.

The sweeps of test_emu_chroma.py go through the C entries on the device (they are tiny: every value of every parameter
is met).  Real input with norm = 0 and no pre_l1 involves no sqrt and no division and must give the emulator's bits;
for the other paths the test prints whether the bits matched and asserts the bound only (whether the device's sqrt
and division give the host's bits is printed, not assumed).  Then the public functions: 1D / 2D / int16 input, a
non-default stream, the spectrum read in place (complex, line-padded rows), and a 440 Hz cosine through all four.
Every accuracy test prints its worst error / bound (-s).  Seen on an MI355X: every case of both sweeps gave the
emulator's bits; worst error / bound 0.28 (CENS, 3 taps, no norm), 0.135 for the fold, 0.073 through the public
functions."""

import importlib
import os
import sys

import numpy as np
import pytest
import torch

import chroma_ref as R
import test_emu_chroma as E

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _extension as _x

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_chroma_bind as eb  # noqa: E402

M = importlib.import_module("mlx_audio_primitives_amd.chroma")

pytestmark = pytest.mark.gpu
CONSTS = E.CONSTS
INF = np.inf


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def padded(x, pad):
    """x (B, K, T) on the device with `pad` NaN columns behind every row: (tensor that owns the memory, row stride)."""
    B, K, T = x.shape
    fill = complex("nan+nanj") if np.iscomplexobj(x) else float("nan")
    buf = torch.full((B, K, T + pad), fill, dtype=torch.complex64 if np.iscomplexobj(x) else torch.float32, device="cuda")
    buf[:, :, :T] = dev(x)
    return buf, T + pad


def device_fold(x, w, in_kind, *, pre_l1=False, threshold=None, norm=None, pad_in=0, pad_out=0):
    B, K, T = x.shape
    xd, in_rs = padded(x, pad_in)
    wd = None if w is None else dev(w)
    n_out = K if w is None else w.shape[0]
    out = torch.full((B, n_out, T + pad_out), float("nan"), dtype=torch.float32, device="cuda")
    _x.check(_x.dlib(xd.device).ap_chroma_fold_f32(_x.ptr(xd), in_kind, B, K, T, in_rs, None if wd is None else _x.ptr(wd), n_out,
                                                   int(pre_l1), int(threshold is not None), float(threshold or 0.0), eb.NORMS[norm],
                                                   _x.ptr(out), T + pad_out, _x.stream_ptr(xd.device)))
    got = out.cpu().numpy()
    assert np.isnan(got[..., T:]).all(), "a pad column was written"
    return np.ascontiguousarray(got[..., :T])


def device_cens(x, taps, norm, pad_in=0, pad_out=0):
    B, n, T = x.shape
    xd, in_rs = padded(x, pad_in)
    td = None if taps is None else dev(taps)
    out = torch.full((B, n, T + pad_out), float("nan"), dtype=torch.float32, device="cuda")
    _x.check(_x.dlib(xd.device).ap_chroma_cens_f32(_x.ptr(xd), B, n, T, in_rs, None if td is None else _x.ptr(td),
                                                   0 if taps is None else len(taps), eb.NORMS[norm], _x.ptr(out), T + pad_out,
                                                   _x.stream_ptr(xd.device)))
    got = out.cpu().numpy()
    assert np.isnan(got[..., T:]).all(), "a pad column was written"
    return np.ascontiguousarray(got[..., :T])


@pytest.mark.parametrize("case", E.FOLD_CASES, ids=E.FOLD_IDS)
def test_gpu_fold_sweep(case):
    K, n_out, T, B, kind, has_w, norm, pre_l1, thr, pad_in, pad_out = case
    x, w, kw, lay = E.fold_case(case)
    got = device_fold(x, w, kind, pad_in=pad_in, pad_out=pad_out, **kw)
    want, bound, keep = R.fold(x, kind, w, CONSTS, **kw)
    ratio = R.check(got, want, bound, keep, case)
    emu = eb.fold(x, w, **kw, **lay)
    same = np.array_equal(got.view(np.uint32), emu.view(np.uint32))
    if kind == 0 and norm is None and not pre_l1:
        assert same, "no sqrt and no division on this path: the device and the emulator must agree in every bit"
    print(f"fold {E.FOLD_IDS[E.FOLD_CASES.index(case)]}: worst error / bound {ratio:.4f}; the emulator's bits: {same}")


@pytest.mark.parametrize("case", E.CENS_CASES, ids=E.CENS_IDS)
def test_gpu_cens_sweep(case):
    n, T, n_taps, norm, B, pad_in, pad_out = case
    i = E.CENS_CASES.index(case)
    x = R.chroma_input(B, n, T, seed=i)
    taps = E.cens_taps(n_taps, i)
    got = device_cens(x, taps, norm, pad_in, pad_out)
    want, bound, keep = R.cens(x, taps, norm)
    ratio = R.check(got, want, bound, keep, case)
    same = np.array_equal(got.view(np.uint32), eb.cens(x, taps, norm=norm).view(np.uint32))
    print(f"cens {E.CENS_IDS[i]}: worst error / bound {ratio:.4f}; the emulator's bits: {same}")


def test_gpu_n_chroma_above_the_cap_is_named():
    with pytest.raises(ValueError, match="n_chroma"):
        ap.chroma_cqt(C=dev(np.ones((98, 4), np.float32)), n_chroma=49, bins_per_octave=49)
    with pytest.raises(ValueError, match="n_chroma"):
        ap.chroma_stft(S=dev(np.ones((65, 4), np.float32)), n_chroma=49)


# ---------------------------------------------------------------------------------------------------------------------
# the public functions
# ---------------------------------------------------------------------------------------------------------------------
CQ = dict(sr=22050, fmin=110.0, n_octaves=3)            # 108 bands from A2: the longest filter has about 10 400 taps


def signal(B, L, seed):
    rng = np.random.default_rng(seed)
    n = np.arange(L) / 22050.0
    y = sum(a * np.cos(2 * np.pi * f * n + p) for a, f, p in ((0.5, 220.0, 0.3), (0.3, 554.4, 1.0), (0.2, 329.6, 2.0)))
    y = y[None] * (0.5 + rng.uniform(0.0, 1.0, (B, 1))) + 0.01 * rng.standard_normal((B, L))
    return y.astype(np.float32)


def test_gpu_chroma_input_kinds_and_streams():
    """1D input is row 0 of the batch; a host array; int16 PCM is its float32 value; a non-default stream."""
    y = signal(2, 12000, 1)
    p16 = np.clip(np.round(y * 16000.0), -32768, 32767).astype(np.int16)
    yf = p16.astype(np.float32) / 32768.0
    funcs = (("chroma_stft", lambda v: ap.chroma_stft(y=v, n_fft=512, hop_length=128), 12),
             ("chroma_cqt", lambda v: ap.chroma_cqt(y=v, **CQ), 12),
             ("chroma_cens", lambda v: ap.chroma_cens(y=v, **CQ), 12),
             ("tonnetz", lambda v: ap.tonnetz(y=v, **CQ), 6))
    side = torch.cuda.Stream()
    for name, f, rows in funcs:
        base = f(dev(y))
        T = base.shape[-1]
        assert base.shape == (2, rows, T) and base.dtype == torch.float32 and base.is_cuda, name
        assert torch.isfinite(base).all() and base.abs().max() > 0
        for b in range(2):
            one = f(dev(y[b]))
            assert one.shape == (rows, T) and torch.equal(one, base[b]), name
        assert torch.equal(f(y), base) and torch.equal(f(torch.from_numpy(y.copy())), base), name
        want = f(dev(yf))
        for arr in (p16, dev(p16), p16[0]):
            got = f(arr)
            assert torch.equal(got, want if arr.ndim == 2 else want[0]), name
        yd = dev(y)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            got = f(yd)
        side.synchronize()
        assert torch.equal(got, base), name


def test_gpu_chroma_cqt_reads_the_complex_spectrum_in_place():
    """chroma_cqt(y=y) is chroma_cqt(C=cqt(y)) bit for bit (|C| is taken in the kernel), and both it and the fold of a
    stored magnitude lie within the bound of the definition applied to the device's complex spectrum."""
    y = dev(signal(2, 12000, 2))
    C = ap.cqt(y, sr=22050, fmin=110.0, n_bins=108, bins_per_octave=36)
    w = ap.cq_to_chroma(108, bins_per_octave=36, fmin=110.0)
    for kw in (dict(), dict(norm=2, threshold=None), dict(norm=None, threshold=0.05), dict(norm=1, window=np.array([0.25, 0.5, 0.25]))):
        from_y = ap.chroma_cqt(y=y, **CQ, **kw)
        from_c = ap.chroma_cqt(C=C, fmin=110.0, **kw)
        assert torch.equal(from_y, from_c), kw
        from_mag = ap.chroma_cqt(C=ap.magnitude(C), fmin=110.0, **kw)
        wk = ap.cq_to_chroma(108, bins_per_octave=36, fmin=110.0, window=kw["window"]) if "window" in kw else w
        rk = dict(norm=kw.get("norm", INF), threshold=kw.get("threshold", 0.0))
        want, bound, keep = R.fold(C.cpu().numpy(), 1, wk, CONSTS, **rk)
        r1 = R.check(from_y.cpu().numpy(), want, bound, keep, ("y", kw))
        r2 = R.check(from_mag.cpu().numpy(), want, bound, keep, ("magnitude", kw))
        print(f"chroma_cqt {kw}: worst error / bound {r1:.4f} from y, {r2:.4f} from a stored magnitude")
    one = ap.chroma_cqt(C=C[0], fmin=110.0)
    assert one.shape == (12, C.shape[-1]) and torch.equal(one, ap.chroma_cqt(C=C, fmin=110.0)[0])


def test_gpu_chroma_stft_reads_line_padded_rows():
    """B = 2, T = 259: stft hands back rows padded to 272 frames, which chroma_stft reads in place."""
    L = 258 * 512
    y = dev(signal(2, L, 3))
    X = ap.stft(y)
    assert X.shape == (2, 1025, 259) and not X.is_contiguous() and X.stride(1) == 272
    got = ap.chroma_stft(y=y)
    assert got.shape == (2, 12, 259)
    Xh = X.cpu().numpy()
    S = dev((Xh.real.astype(np.float64) ** 2 + Xh.imag.astype(np.float64) ** 2).astype(np.float32))
    assert S.is_contiguous()
    from_s = ap.chroma_stft(S=S)
    w = ap.chroma_filterbank(sr=22050, n_fft=2048)
    want, bound, keep = R.fold(Xh, 2, w, CONSTS, norm=INF)
    r1 = R.check(got.cpu().numpy(), want, bound, keep, "y")
    r2 = R.check(from_s.cpu().numpy(), want, bound, keep, "S")
    assert torch.equal(ap.chroma_stft(S=S[1]), from_s[1])
    for kw in (dict(norm=2, n_chroma=24, tuning=0.2), dict(norm=None, octwidth=None, base_c=False)):
        wk = ap.chroma_filterbank(sr=22050, n_fft=2048, **{k: v for k, v in kw.items() if k != "norm"})
        want, bound, keep = R.fold(Xh, 2, wk, CONSTS, norm=kw["norm"])
        R.check(ap.chroma_stft(y=y, **kw).cpu().numpy(), want, bound, keep, kw)
    print(f"chroma_stft on padded rows: worst error / bound {r1:.4f} from y, {r2:.4f} from S")


def cosine():
    return np.cos(2.0 * np.pi * 440.0 * np.arange(22050) / 22050.0).astype(np.float32)


def test_gpu_a_440_hz_cosine_is_an_a():
    y = dev(cosine())
    c = ap.chroma_stft(y=y).cpu().numpy()
    assert c.shape == (12, 44)
    assert np.all(c[9, 2:-2] == 1.0) and np.all(c[:, 2:-2].argmax(axis=0) == 9), c[:, 2:-2].argmax(axis=0)
    c = ap.chroma_cqt(y=y, **CQ).cpu().numpy()
    assert c.shape == (12, 44)
    t = np.arange(44) * 512
    inside = (t >= 5300) & (t <= 22050 - 5300)           # the longest filter (10 412 taps) lies inside the clip
    assert inside.sum() >= 20
    assert np.all(c[9, inside] == 1.0) and np.all(c[:, inside].argmax(axis=0) == 9)
    assert np.all(np.delete(c[:, inside], 9, axis=0) < 0.5)


def test_gpu_chroma_cqt_at_its_defaults():
    """252 bands from C1 (the longest filter has 35 031 taps, longer than the clip): within the bound of the definition
    applied to the device's own cqt, and an A where the 440 Hz band's window lies inside the clip."""
    y = dev(cosine())
    got = ap.chroma_cqt(y=y)
    assert got.shape == (12, 44) and got.dtype == torch.float32
    C = ap.cqt(y, n_bins=252, bins_per_octave=36)
    want, bound, keep = R.fold(C.cpu().numpy()[None], 1, ap.cq_to_chroma(252, bins_per_octave=36), CONSTS, norm=INF, threshold=0.0)
    ratio = R.check(got.cpu().numpy()[None], want, bound, keep, "defaults")
    c = got.cpu().numpy()
    assert np.all(c[:, 10:34].argmax(axis=0) == 9) and np.all(c[9, 10:34] == 1.0)
    print(f"chroma_cqt at its defaults: worst error / bound {ratio:.4f}")


def test_gpu_tonnetz_of_uniform_and_one_hot_chroma():
    uniform = np.full((2, 12, 70), 0.37, np.float32)
    got = ap.tonnetz(chroma=dev(uniform)).cpu().numpy()
    want, bound, keep = R.fold(uniform, 0, M._phi64(12).astype(np.float32), CONSTS, pre_l1=True)
    assert got.shape == (2, 6, 70)
    ratio = R.check(got, want, bound, keep, "uniform")
    assert np.all(np.abs(want) <= 1e-7) and np.all(np.abs(got) <= bound + 1e-7)       # phi rounded to float32 sums to ~1e-8, not 0
    onehot = np.zeros((12, 12), np.float32)
    onehot[np.arange(12), np.arange(12)] = 3.0
    got = ap.tonnetz(chroma=dev(onehot)).cpu().numpy().astype(np.float64)
    assert got.shape == (6, 12)
    r = np.sqrt(got[0::2] ** 2 + got[1::2] ** 2)
    np.testing.assert_allclose(r, np.array([1.0, 1.0, 0.5])[:, None] * np.ones((1, 12)), rtol=0, atol=8 * R.U)
    want, bound, keep = R.fold(onehot[None], 0, M._phi64(12).astype(np.float32), CONSTS, pre_l1=True)
    R.check(got[None], want, bound, keep, "one-hot")
    print(f"tonnetz of a uniform chroma: worst error / bound {ratio:.4f}")


def test_gpu_chroma_cens_at_its_defaults():
    y = dev(cosine())
    got = ap.chroma_cens(y=y).cpu().numpy()
    assert got.shape == (12, 44)
    chroma = ap.chroma_cqt(y=y, norm=None).cpu().numpy()
    taps = M._smoothing_taps(41, "hann")
    want, bound, keep = R.cens(chroma[None], taps, 2)
    ratio = R.check(got[None], want, bound, keep, "cens defaults", max_left_out=0.01)
    n = np.sqrt((got.astype(np.float64) ** 2).sum(axis=0))
    live = np.abs(want[0]).max(axis=0) > 0
    assert live.sum() >= 40
    np.testing.assert_allclose(n[live], 1.0, rtol=0, atol=(12 + 4) * R.U)
    assert torch.equal(ap.chroma_cens(C=ap.cqt(y, n_bins=252, bins_per_octave=36)), dev(got))
    plain = ap.chroma_cens(y=y, win_len_smooth=None, norm=None).cpu().numpy()
    assert set(np.unique(plain)) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    print(f"chroma_cens at its defaults: worst error / bound {ratio:.4f}, left out {100 * (1 - keep.mean()):.2f} %")
