"""GPU: reassigned_spectrogram against the float64 NumPy reference of tests/reassign_ref.py, within the per-element bound stated
there, at the smallest shapes at which each kernel can go wrong.  (The T = 1 case keeps only its first 100 samples at zero: a clip
shorter than a hop whose first n_fft samples are zero is all zero.)"""

import numpy as np
import pytest
import torch

import reassign_ref as R

import mlx_audio_primitives_amd as ap

pytestmark = pytest.mark.gpu

W = dict(n_fft=2048, L=5300, batch=2)                       # wave kernel: T = 11, a partial last group, a clip boundary in a stretch
TILE = dict(n_fft=400, hop=160, L=2000, batch=2)            # tile kernel: T = 13, G = 8
OPTIONS = [dict(rf=False), dict(rt=False), dict(fill_nan=True), dict(clip=False), dict(ref_power=0.0)]
CASES = [dict(n_fft=2048, L=500, head=100), W, dict(W, hop=441, batch=1), dict(W, center=False, L=4113, batch=1),
         dict(W, pad_mode="reflect", batch=1), dict(W, pad_mode="edge", batch=1), dict(W, win_length=1200, batch=1),
         dict(W, window="hamming", batch=1), TILE, dict(n_fft=512, hop=128, win_length=300, L=2500),
         dict(n_fft=27, hop=5, L=300, batch=2), dict(n_fft=77, hop=19, L=700),
         dict(TILE, pad_mode="reflect", center=True, batch=1),
         dict(TILE, center=False, batch=1)] + [dict(W, **o) for o in OPTIONS] + [dict(TILE, **o) for o in OPTIONS]


def split(case):
    """(signal, keyword arguments of R.reference) of a case."""
    c = dict(case)
    n_fft, L, batch, head = c.pop("n_fft"), c.pop("L"), c.pop("batch", 1), c.pop("head", None)
    hop = c.get("hop") or (c.get("win_length") or n_fft) // 4
    return R.signal(L, n_fft, hop, head=head, batch=batch, ref_power=c.get("ref_power", 1e-6)), dict(c, n_fft=n_fft, hop=hop)


def run(y, kw):
    kw = dict(kw)
    names = dict(hop="hop_length", rf="reassign_frequencies", rt="reassign_times")
    return ap.reassigned_spectrogram(torch.from_numpy(y).cuda(), **{names.get(k, k): v for k, v in kw.items()})


def ulp32(x):
    return np.spacing(np.abs(np.nan_to_num(x, posinf=0.0)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_matches_float64_reference(case):
    y, kw = split(case)
    r = R.reference(y, **kw)
    out = run(y, kw)
    for o in out:
        assert o.dtype == torch.float32 and o.is_cuda and tuple(o.shape) == r["mags"].shape
    freqs, times, mags = (o.cpu().numpy().astype(np.float64) for o in out)
    assert np.all(np.abs(mags - r["mags"]) <= 4 * r["E_h"])
    bf, bt, excluded = R.quotient_bounds(r)
    print("excluded", excluded.mean())
    assert excluded.mean() <= 0.01
    n, sr = kw["n_fft"], 22050
    for name, got, bound, m, scale, on, grid in (("freqs", freqs, bf, R.M_FREQ[n], sr / (2 * np.pi), kw.get("rf", True), r["bin_f"]),
                                                 ("times", times, bt, R.M_TIME[n], 1 / sr, kw.get("rt", True), r["frame_t"])):
        want = r[name]
        if not on:                                         # the broadcast grid, exactly
            assert np.array_equal(got.astype(np.float32), np.broadcast_to(grid, got.shape).astype(np.float32)), name
            continue
        keep = ~excluded
        assert np.array_equal(np.isnan(got)[keep], np.isnan(want)[keep]), name
        keep &= ~np.isnan(want)
        tol = np.where(r["bad"], 0.0, m * bound * scale)     # a filled value carries no quotient
        hi = r["lim"][0 if name == "freqs" else 1]
        lo_w, hi_w = np.clip(want - tol, 0 if np.isfinite(hi) else -np.inf, hi), np.clip(want + tol, 0 if np.isfinite(hi) else -np.inf, hi)
        err = np.maximum(lo_w - got, got - hi_w)[keep] / ulp32(want)[keep]
        print(name, "worst excess in ulp of the value", err.max(initial=-np.inf))
        assert np.all(err <= 1.0), name


@pytest.mark.parametrize("case", [W, TILE, dict(W, pad_mode="reflect")], ids=["wave", "tile", "wave-reflect"])
def test_bit_identical_runs_batch_and_flags(case):
    y, kw = split(case)
    a = [o.cpu().numpy() for o in run(y, kw)]
    again = [o.cpu().numpy() for o in run(y, kw)]
    alone = [o.cpu().numpy() for o in run(y[1], kw)]
    only_f = [o.cpu().numpy() for o in run(y, dict(kw, rt=False))]
    only_t = [o.cpu().numpy() for o in run(y, dict(kw, rf=False))]
    for i in range(3):
        assert np.array_equal(a[i], again[i], equal_nan=True)
        assert np.array_equal(a[i][1], alone[i], equal_nan=True)
    for i in (0, 2):                                       # a plane that is off leaves the others as they were, bit for bit
        assert np.array_equal(a[i], only_f[i], equal_nan=True)
    for i in (1, 2):
        assert np.array_equal(a[i], only_t[i], equal_nan=True)
