"""GPU: yin / yin_cmnd against their definition in float64 (tests/yin_ref.py).

Measured on an MI355X (worst over every case below; the bounds come from yin_ref.Case, i.e. from the float32
NumPy route's own error, never from these figures): see DESIGN.md, "YIN".

Inputs: six 2 s signals (fixed seed), five shapes (2048 / 1024 on the wave kernel and on the general one, 512 / 1536 / 400 on the general kernel),
centred and not, two lengths (the second not a multiple of the hop), as one batch and each clip alone."""

import functools

import numpy as np
import pytest
import torch

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _extension as ext

import yin_ref as R

pytestmark = pytest.mark.gpu

LENGTHS = {"2s": 2 * R.SR, "2s+37": 2 * R.SR + 37}


@functools.lru_cache(maxsize=None)
def clips(L):
    s = R.signals(R.SR, L)
    return np.stack([s[k] for k in R.NAMES]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name, L, shape, center):
    fl, hop, fmin, fmax = shape
    return R.Case(clips(L)[R.NAMES.index(name)], fl, hop, fmin, fmax, center)


def served_by_wave_kernel(fl, hop, L):
    return bool(ext.lib().ap_yin_fused(fl, hop, L))


def run(y, shape, center, **kw):
    fl, hop, fmin, fmax = shape
    curve = ap.yin_cmnd(y, fmin=fmin, fmax=fmax, sr=R.SR, frame_length=fl, hop_length=hop, center=center, **kw)
    f0, aper = ap.yin(y, fmin=fmin, fmax=fmax, sr=R.SR, frame_length=fl, hop_length=hop, center=center,
                      return_aperiodicity=True, **kw)
    torch.cuda.synchronize()
    return curve.cpu().numpy(), f0.cpu().numpy(), aper.cpu().numpy()


# every shape as dispatched, plus the general kernel forced on the shapes the wave kernel serves
ROUTES = [(s, False) for s in R.SHAPES] + [(s, True) for s in R.SHAPES[:2]]


@pytest.mark.parametrize("Lname", list(LENGTHS))
@pytest.mark.parametrize("center", [True, False], ids=["center", "nocenter"])
@pytest.mark.parametrize("shape,general", ROUTES, ids=[f"n{s[0]}{'-general' if g else ''}" for s, g in ROUTES])
def test_yin_matches_definition(shape, general, center, Lname, monkeypatch):
    """Curve, f0 on the decisive frames and aperiodicity for every signal (`loud` and `quiet` against their own
    float64 curves: a hidden absolute floor fails `quiet`), the batch and every clip alone bit for bit, and the
    cap on the frames left out.  general: the same through AP_YIN_GENERAL=1 (only differs where the wave kernel
    serves the shape)."""
    L = LENGTHS[Lname]
    fl, hop = shape[0], shape[1]
    if general:
        monkeypatch.setenv("AP_YIN_GENERAL", "1")
    assert served_by_wave_kernel(fl, hop, L) == (fl in (2048, 1024))
    y = torch.from_numpy(clips(L)).cuda()
    curve, f0, aper = run(y, shape, center)
    for i, name in enumerate(R.NAMES):
        c = case(name, L, shape, center)
        left_out = c.compare(curve[i], f0[i], aper[i], f"{name} n={fl} center={center} L={L} general={general}")
        assert left_out <= R.CAPS[name], (name, left_out)
        c1, f1, a1 = run(y[i], shape, center)
        assert np.array_equal(c1, curve[i]) and np.array_equal(f1, f0[i]) and np.array_equal(a1, aper[i]), name


@pytest.mark.parametrize("shape", R.SHAPES[:2], ids=["n2048", "n1024"])
def test_wave_kernel_agrees_with_general_kernel(shape, monkeypatch):
    L = LENGTHS["2s+37"]
    assert served_by_wave_kernel(shape[0], shape[1], L)
    y = torch.from_numpy(clips(L)).cuda()
    cw, fw, aw = run(y, shape, True)
    monkeypatch.setenv("AP_YIN_GENERAL", "1")
    cg, fg, ag = run(y, shape, True)
    assert not np.array_equal(cw, cg)                  # two kernels did run
    for i, name in enumerate(R.NAMES):
        c = case(name, L, shape, True)
        err = float(np.abs(cw[i] - cg[i]).max())
        print(f"{name}: wave vs general curve {err:.3e} (atol {c.atol:.3e})")
        assert err <= c.atol


@pytest.mark.parametrize("shape", R.SHAPES, ids=[f"n{s[0]}" for s in R.SHAPES])
def test_all_zero_clip(shape):
    fl, hop, fmin, fmax = shape
    lo, hi, _ = R.periods(R.SR, fmin, fmax, fl)
    y = torch.zeros((2, 3 * fl + 11), device="cuda")
    curve, f0, aper = run(y, shape, True)
    assert np.isfinite(curve).all() and np.all(curve == 1.0)
    assert np.all(f0 == np.float32(R.SR) / np.float32(lo)) and np.all(aper == 1.0)


@pytest.mark.parametrize("shape", R.SHAPES, ids=[f"n{s[0]}" for s in R.SHAPES])
def test_center_equals_zero_padded_clip(shape):
    fl = shape[0]
    y = clips(LENGTHS["2s+37"])[:3]
    yp = np.pad(y, ((0, 0), (fl // 2, fl // 2)))
    a = run(torch.from_numpy(y).cuda(), shape, True)
    b = run(torch.from_numpy(yp).cuda(), shape, False)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_sine_440_is_resolved_between_integer_lags():
    t = np.arange(R.SR) / R.SR
    y = np.sin(2 * np.pi * 440.0 * t).astype(np.float32)
    for shape in R.SHAPES:
        fl, hop, fmin, fmax = shape
        f0 = ap.yin(y, fmin=fmin, fmax=fmax, sr=R.SR, frame_length=fl, hop_length=hop).cpu().numpy()
        k = fl // hop
        inner = f0[k:-k]
        print(f"n={fl}: {inner.min():.4f} .. {inner.max():.4f} Hz")
        assert np.all(np.abs(inner - 440.0) < 0.5)


def test_host_noncontiguous_inputs_and_defaults():
    shape = R.SHAPES[0]
    y = clips(LENGTHS["2s"])
    want = run(torch.from_numpy(y).cuda(), shape, True)
    wide = torch.from_numpy(np.repeat(y, 2, axis=1)).cuda()[:, ::2]         # strided view
    assert not wide.is_contiguous()
    for u, v in zip(run(wide, shape, True), want):
        assert np.array_equal(u, v)
    for u, v in zip(run(y, shape, True), want):                              # host array
        assert np.array_equal(u, v)
    f0 = ap.yin(y[0], fmin=65.0, fmax=2093.0)                                # librosa's defaults: 2048 / 512
    assert f0.shape == (1 + y.shape[1] // 512,) and np.array_equal(f0.cpu().numpy(), want[1][0])
    f0w = ap.yin(y[0], fmin=65.0, fmax=2093.0, win_length=1024)
    assert torch.equal(f0, f0w)


@pytest.mark.parametrize("mode", ["edge", "reflect"])
def test_edge_and_reflect_padding(mode):
    for shape in (R.SHAPES[0], R.SHAPES[1], R.SHAPES[4]):
        fl = shape[0]
        y = clips(LENGTHS["2s+37"])[:2]
        yp = np.pad(y, ((0, 0), (fl // 2, fl // 2)), mode=mode)
        a = run(torch.from_numpy(y).cuda(), shape, True, pad_mode=mode)
        b = run(torch.from_numpy(yp).cuda(), shape, False)
        for u, v in zip(a, b):
            assert np.array_equal(u, v)


def test_caller_stream():
    y = torch.from_numpy(clips(LENGTHS["2s"])).cuda()
    for shape in R.SHAPES[:3]:
        want = run(y, shape, True)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = run(y, shape, True)
        for u, v in zip(got, want):
            assert np.array_equal(u, v)


def test_odd_hop_takes_the_general_kernel():
    assert not served_by_wave_kernel(2048, 511, 44100)
    fl, hop, fmin, fmax = 2048, 511, 65.0, 2093.0
    y = clips(LENGTHS["2s"])[0]
    c = R.Case(y, fl, hop, fmin, fmax, True)
    curve, f0, aper = run(torch.from_numpy(y).cuda(), (fl, hop, fmin, fmax), True)
    c.compare(curve, f0, aper, "vibrato hop=511")
