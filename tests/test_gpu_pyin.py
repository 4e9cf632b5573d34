"""GPU: pyin's two kernels against the definition in tests/pyin_ref.py, then the public function.  The observation kernel
is fed the device's own yin_cmnd curves (and synthetic curves through the C entry) and held to the derived bounds; the
banded decode is fed emissions the device made and must equal the float32 model in every bit."""

import math

import numpy as np
import pytest
import torch

import pyin_ref as R
import yin_ref as Y

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _extension as _x
from mlx_audio_primitives_amd import pitch

pytestmark = pytest.mark.gpu
TABLES = lambda n_lags, **kw: pitch._pyin_tables(fmin=65.40639132514966, fmax=2093.004522404789, sr=22050, hop=512, n_lags=n_lags, **kw)  # noqa: E731
SR, C2, C7 = 22050, 65.40639132514966, 2093.004522404789
FLOOR = math.log(R.TINY) + 1e-4         # an emission above this holds a probability: p > tiny (e^1e-4 - 1)


dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731


def observe(curve, lo, fmin, bps, n_bins, tabs):
    """ap_pyin_observe_f32 on curve (B, n_lags, T): (E (B, T, n_bins + 1), voiced_prob (B, T)) as host arrays."""
    c = curve if isinstance(curve, torch.Tensor) else dev(curve)
    B, n_lags, T = c.shape
    t = [dev(tabs[k]) for k in ("thr", "beta", "ea", "nz")]
    E, vp = torch.full((B, T, n_bins + 1), float("nan"), device="cuda"), torch.full((B, T), float("nan"), device="cuda")
    _x.check(_x.dlib(c.device).ap_pyin_observe_f32(_x.ptr(c), B, n_lags, T, lo, float(SR), float(fmin), bps, n_bins, _x.ptr(t[0]), _x.ptr(t[1]),
                                                   100, _x.ptr(t[2]), _x.ptr(t[3]), len(tabs["ea"]), 0.01, _x.ptr(E), _x.ptr(vp),
                                                   _x.stream_ptr(c.device)))
    return E.cpu().numpy(), vp.cpu().numpy()


def check_observation(curve, E, vp, lo, fmin, bps, n_bins, tabs, label):
    """One clip against observe64; returns the share of frames left out."""
    P, vsum, dec = R.observe64(curve, lo, SR, fmin, bps, n_bins, tabs, 0.01)
    L, bE, v, bv = R.expected(P, vsum, 100, curve.shape[0])
    assert np.isfinite(E).all() and np.isfinite(vp).all(), label
    errE, errv = np.abs(E - L)[dec], np.abs(vp - v)[dec]
    print(f"{label}: E err / bound {float((errE / bE[dec]).max()):.3f}  voiced_prob err / bound {float((errv / bv[dec]).max()):.3f}  "
          f"non-decisive {1 - dec.mean():.4f}  occupied bins {int((P > 0).sum())}")
    assert ((E[:, :n_bins] > FLOOR) == (L[:, :n_bins] > FLOOR))[dec].all(), label
    assert (errE <= bE[dec]).all() and (errv <= bv[dec]).all(), label
    return 1.0 - float(dec.mean())


@pytest.mark.parametrize("fl,hop,fmin,fmax", [(2048, 512, C2, C7), (512, 128, 200.0, 2000.0)])
def test_observation_on_device_curves(fl, hop, fmin, fmax):
    sig, names = Y.signals(SR, 11025), ["vibrato", "glide", "bursts", "noise"]
    lo, hi, _ = Y.periods(SR, fmin, fmax, fl)
    bps, n_bins, tabs = 10, int(math.floor(120 * math.log2(fmax / fmin))) + 1, TABLES(hi - lo + 1)
    kw = dict(fmin=fmin, fmax=fmax, sr=SR, frame_length=fl, hop_length=hop)
    batch = ap.yin_cmnd(np.stack([sig[k] for k in names[:3]]).astype(np.float32), **kw)
    alone = ap.yin_cmnd(sig["noise"].astype(np.float32), **kw)[None]
    (Eb, vb), (Ea, va) = observe(batch, lo, fmin, bps, n_bins, tabs), observe(alone, lo, fmin, bps, n_bins, tabs)
    E1, v1 = observe(batch[1:2].contiguous(), lo, fmin, bps, n_bins, tabs)
    assert E1.tobytes() == Eb[1:2].tobytes() and v1.tobytes() == vb[1:2].tobytes(), "a clip alone differs from the clip in a batch"
    curves = list(batch.cpu().numpy()) + [alone[0].cpu().numpy()]
    for name, c, E, v in zip(names, curves, list(Eb) + [Ea[0]], list(vb) + [va[0]]):
        assert check_observation(c, E, v, lo, fmin, bps, n_bins, tabs, f"{fl} {name}") <= 0.005


# name: (values set in a curve of ones over the lags 10 .. 339 (None: a ramp), occupied bins, fmin, n_bins at 12 bins per octave)
SYNTHETIC = {"no trough": ({}, 0, 65.0, 64), "trough at 0": (None, 1, 65.0, 64), "trough at the last lag": (None, 1, 65.0, 64),
             "two candidates in one bin": ({296: 0.05, 298: 0.07, 120: 0.3}, 2, 65.0, 64),       # lags 306 / 308: 1.79 / 1.67 bins
             "candidate at n_bins": ({0: 0.02, 200: 0.2}, 1, SR / 10 / 2.0 ** (20.2 / 12), 20)}  # lag 10: bin 20.2, clipped, dropped


@pytest.mark.parametrize("case", list(SYNTHETIC))
def test_observation_on_synthetic_curves(case):
    values, occupied, fmin, n_bins = SYNTHETIC[case]
    c = np.ones(330, np.float32)
    if values is None:
        c = np.linspace(0.05, 1.5, 330).astype(np.float32)[::1 if case == "trough at 0" else -1]
    for x, v in (values or {}).items():
        c[x] = v
    curve, tabs = np.stack([c, (0.5 * c).astype(np.float32)], axis=1), TABLES(330)     # the second frame passes other thresholds
    E, vp = observe(curve[None], 10, fmin, 1, n_bins, tabs)
    assert check_observation(curve, E[0], vp[0], 10, fmin, 1, n_bins, tabs, case) == 0.0
    assert (E[0, :, :n_bins] > FLOOR).sum(axis=1).tolist() == [occupied, occupied]


def decode(E, lw, lz, ls, li, h, max_blocks=0):
    """ap_pyin_decode_f32 on device emissions E (B, T, nb + 1) with freq[j] = j and fill -1: host arrays."""
    B, T, nb = E.shape[0], E.shape[1], E.shape[2] - 1
    t = [dev(np.asarray(a, np.float32)) for a in (lw, lz, np.reshape(ls, 4), np.arange(nb))]
    full = lambda shape, fill, dtype: torch.full(shape, fill, dtype=dtype, device="cuda")      # noqa: E731
    ptr, st, f0 = full((B, T, 2 * nb), -4370, torch.int16), full((B, T), -7, torch.int32), full((B, T), -7.0, torch.float32)
    vo, lp = full((B, T), 9, torch.uint8), full((B,), float("nan"), torch.float64)
    _x.check(_x.dlib(E.device).ap_pyin_decode_f32(_x.ptr(E), B, nb, T, _x.ptr(t[0]), h, _x.ptr(t[1]), _x.ptr(t[2]), float(li), _x.ptr(t[3]), 1, -1.0,
                                                  _x.ptr(ptr), _x.ptr(st), _x.ptr(f0), _x.ptr(vo), _x.ptr(lp), max_blocks,
                                                  _x.stream_ptr(E.device)))
    return ptr.cpu().numpy().view(np.uint16), st.cpu().numpy(), lp.cpu().numpy(), f0.cpu().numpy(), vo.cpu().numpy()


def sparse_emissions(nb, T, B, rng):
    """Mostly-zero observation rows through the device's own emission kernel: E (B, T, nb + 1) on the device."""
    prob = np.zeros((B, nb + 1, T), np.float32)
    for b, t in np.ndindex(B, T):
        k = rng.integers(0, 4)
        prob[b, rng.integers(0, nb, k), t] = rng.uniform(0.0, 1.0 / 3, k).astype(np.float32)
    prob[:, nb] = (1.0 - prob[:, :nb].sum(axis=1)) / nb
    p, E, flags = dev(prob), torch.empty((B, T, nb + 1), device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda")
    _x.check(_x.dlib(p.device).ap_viterbi_emission_f32(_x.ptr(p), B, nb + 1, T, T, 0, None, _x.ptr(E), _x.ptr(flags), _x.stream_ptr(p.device)))
    return E


def check_decode(E, lw, lz, ls, li, h, max_blocks, label):
    ptr, st, lp, f0, vo = decode(E, lw, lz, ls, li, h, max_blocks)
    Eh, nb = E.cpu().numpy(), E.shape[2] - 1
    for b in range(Eh.shape[0]):
        mp, ms, ml = R.decode_f32(Eh[b], lw, lz, ls, li, h)
        assert ptr[b, 1:].tobytes() == mp[1:].tobytes() and not ptr[b, 0].any(), (label, b, "back-pointers")
        assert st[b].tobytes() == ms.tobytes() and lp[b].tobytes() == ml.tobytes(), (label, b, lp[b], ml)
        assert (vo[b] == (ms < nb)).all() and (f0[b] == np.where(ms < nb, ms % nb, -1)).all(), (label, b, "gather")


@pytest.mark.parametrize("nb", [2, 3, 63, 64, 65, 255, 256, 257, 601, 1024])
def test_decode_equals_the_model(nb):
    assert _x.lib().ap_pyin_max_bins() == 1024
    rng, STEPS = np.random.default_rng(nb), (1, 2, 16, 17, 18, 40)        # the backtrack stages 16 rows: T - 1 below, at, above it
    for n, W in enumerate(w for w in (1, 2, 3, 101, nb) if w <= nb):      # a grid of 2 under 3 sequences
        T, B, switch = STEPS[(n + nb) % len(STEPS)], (1, 3)[(n + nb) % 2], (0.01, 0.0, 1.0, 0.3, 0.01)[n]
        check_decode(sparse_emissions(nb, T, B, rng), *pitch._pyin_band(nb, W, switch), np.float32(math.log(1 / (2 * nb))), W // 2, 2,
                     f"nb {nb} W {W} T {T} B {B} switch {switch}")
    for T in STEPS:                                                         # every step count at one band
        check_decode(sparse_emissions(nb, T, 2, rng), *pitch._pyin_band(nb, min(nb, 5), 0.01), -1.0, min(nb, 5) // 2, 0, f"nb {nb} T {T}")
    h = min(nb - 1, 3)                                                      # integer scores: ties everywhere, every sum exact
    E = dev(rng.integers(-6, 1, (3, 18, nb + 1)).astype(np.float32))
    check_decode(E, -np.abs(np.arange(-h, h + 1.0)), np.zeros(nb), np.float32([[0, -2], [-2, 0]]), -1.0, h, 2, f"nb {nb} integers")


def test_pyin_end_to_end():
    host = lambda out: [a.cpu().numpy() for a in out]                       # noqa: E731
    sine = np.sin(2 * np.pi * 220.0 * np.arange(SR) / SR).astype(np.float32)
    f0, voiced, prob = host(ap.pyin(sine, fmin=C2, fmax=C7, sr=SR))
    assert f0.shape == voiced.shape == prob.shape == (1 + SR // 512,) and voiced.dtype == bool
    assert voiced[2:-2].all() and (np.abs(np.log2(f0[2:-2] / 220.0)) <= 1 / 120 + 1e-6).all() and (prob[2:-2] > 0.5).all()
    z0, zv, zp = host(ap.pyin(np.zeros(8192, np.float32), fmin=C2, fmax=C7, sr=SR))
    assert not zv.any() and np.isnan(z0).all() and (zp == 0).all()
    n0, nv, _ = host(ap.pyin(np.zeros(8192, np.float32), fmin=C2, fmax=C7, sr=SR, fill_na=None))
    assert not nv.any() and np.isfinite(n0).all() and (n0 >= np.float32(C2)).all()
    bursts = Y.signals(SR, SR)["bursts"].astype(np.float32)
    batch = host(ap.pyin(torch.from_numpy(np.stack([bursts, sine])).cuda(), fmin=C2, fmax=C7, sr=SR))
    for a, b, c in zip(batch, host(ap.pyin(bursts, fmin=C2, fmax=C7, sr=SR)), (f0, voiced, prob)):
        assert a[0].tobytes() == b.tobytes(), "a clip alone differs from the clip in a batch"
        assert a[1].tobytes() == c.tobytes(), "host and device input differ"
