"""GPU: the piptrack kernels on the device against the NumPy model of tests/piptrack_ref.py and against the emulator, every
float32 bit and every count equal (the sweeps of test_emu_piptrack.py through the C entries), then the public functions.
The one test that is not an exact comparison is the end-to-end property at the bottom."""

import importlib
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import piptrack_ref as R
import test_emu_piptrack as E

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _extension as _x

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_piptrack_bind as eb  # noqa: E402

M = importlib.import_module("mlx_audio_primitives_amd.pitch")

pytestmark = pytest.mark.gpu
bits = E.bits
SR = E.SR


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def padded(x, pad):
    B, F, T = x.shape
    cplx = np.iscomplexobj(x)
    buf = torch.full((B, F, T + pad), complex("nan+nanj") if cplx else float("nan"), dtype=torch.complex64 if cplx else torch.float32,
                     device="cuda")
    buf[:, :, :T] = dev(x)
    return buf, T + pad, int(cplx)


def device_dense(x, k_lo, k_hi, bin_hz, threshold, ref, pad_in, pad_out):
    B, F, T = x.shape
    xd, in_rs, kind = padded(x, pad_in)
    mode, value, _, _ = eb.ref_args(ref, B, T)
    rd = dev(np.broadcast_to(np.asarray(ref, np.float32), (B, T))) if mode == 2 else None
    outs = [torch.full((B, F, T + pad_out), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    _x.check(_x.dlib(xd.device).ap_piptrack_f32(_x.ptr(xd), kind, B, F, T, in_rs, k_lo, k_hi, float(threshold), mode, value,
                                                None if rd is None else _x.ptr(rd), float(bin_hz), _x.ptr(outs[0]), _x.ptr(outs[1]),
                                                T + pad_out, _x.stream_ptr(xd.device)))
    got = [o.cpu().numpy() for o in outs]
    assert all(np.isnan(g[..., T:]).all() for g in got), "a pad column was written"
    return [np.ascontiguousarray(g[..., :T]) for g in got]


def device_records(x, k_lo, k_hi, bin_hz, capacity, per_clip, threshold=0.1):
    B, F, T = x.shape
    xd, in_rs, kind = padded(x, 3)
    G = B if per_clip else 1
    rec = torch.full((G, capacity, 2), float("nan"), dtype=torch.float32, device="cuda")
    cnt = torch.full((G,), -1, dtype=torch.int64, device="cuda")
    _x.check(_x.dlib(xd.device).ap_piptrack_records_f32(_x.ptr(xd), kind, B, F, T, in_rs, k_lo, k_hi, float(threshold), 0, 0.0, None,
                                                        float(bin_hz), int(per_clip), _x.ptr(rec), capacity, _x.ptr(cnt), _x.stream_ptr(xd.device)))
    return cnt, rec


def device_tuning(rec, cnt, edges, bpo):
    G, capacity, _ = rec.shape
    n_bins = len(edges) - 1
    thr = torch.full((G,), float("nan"), dtype=torch.float32, device="cuda")
    counts = torch.full((G, n_bins), -1, dtype=torch.int64, device="cuda")
    _x.check(_x.dlib(rec.device).ap_piptrack_tuning_f32(_x.ptr(rec), _x.ptr(cnt), G, capacity, float(bpo), _x.ptr(dev(edges)), n_bins,
                                                        _x.ptr(thr), _x.ptr(counts), _x.stream_ptr(rec.device)))
    return thr.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("case", E.DENSE_CASES, ids=E.DENSE_IDS)
def test_gpu_dense_sweep(case):
    x, S, k_lo, k_hi, bin_hz, ref, kw = E.dense_case(case)
    want_p, want_m = R.piptrack(S, **kw)
    got_p, got_m = device_dense(x, k_lo, k_hi, bin_hz, kw["threshold"], ref, case[7], case[8])
    np.testing.assert_array_equal(bits(got_p), bits(want_p))
    np.testing.assert_array_equal(bits(got_m), bits(want_m))
    emu_p, emu_m = eb.dense(x, k_lo, k_hi, bin_hz, threshold=kw["threshold"], ref=ref)
    np.testing.assert_array_equal(bits(got_p), bits(emu_p))
    np.testing.assert_array_equal(bits(got_m), bits(emu_m))


def test_gpu_equal_to_the_threshold_and_subnormal_den():
    S, calls = E.edge_columns()
    for kw in calls:
        want_p, want_m = R.piptrack(S, k_range=(0, 6), sr=10, **kw)
        got_p, got_m = device_dense(S, 0, 6, np.float32(1.0), kw.get("threshold", 0.1), kw.get("ref"), 0, 0)
        np.testing.assert_array_equal(bits(got_p), bits(want_p))
        np.testing.assert_array_equal(bits(got_m), bits(want_m))


def test_gpu_histogram_below_27_5_hz_and_of_junk():
    f = E.low_frequencies()
    ok = f[np.isfinite(f)]
    for res, bpo in ((0.01, 12), (0.3, 36)):
        edges = R.edges(res)
        counts = torch.full((len(edges) - 1,), -1, dtype=torch.int64, device="cuda")
        fd = dev(f)
        _x.check(_x.dlib(fd.device).ap_pitch_hist_f32(_x.ptr(fd), fd.numel(), float(bpo), _x.ptr(dev(edges)), len(edges) - 1,
                                                      _x.ptr(counts), _x.stream_ptr(fd.device)))
        np.testing.assert_array_equal(counts.cpu().numpy(), R.counts(ok, res, bpo))
        assert ap.pitch_tuning(fd, resolution=res, bins_per_octave=bpo) == R.pitch_tuning(ok, res, bpo)


@pytest.mark.parametrize("per_clip", [False, True])
@pytest.mark.parametrize("cplx", [False, True])
def test_gpu_records_selection_and_histogram(per_clip, cplx):
    X, S, p, m, k_lo, k_hi, bin_hz = E.tonal()
    cnt, rec = device_records(X if cplx else S, k_lo, k_hi, bin_hz, 4096, per_clip)
    groups = [(p[b], m[b]) for b in range(3)] if per_clip else [(p, m)]
    n_host, rec_host = cnt.cpu().numpy(), rec.cpu().numpy()
    for g, (pg, mg) in enumerate(groups):
        want = E.dense_pairs(pg, mg)
        assert int(n_host[g]) == len(want)
        np.testing.assert_array_equal(E.as_words(rec_host[g, :len(want)]), E.as_words(want))
        assert np.isnan(rec_host[g, len(want):]).all()
    for resolution, bpo in ((0.01, 12), (0.3, 12), (0.01, 36), (0.3, 36)):
        assert R.nearest_edge_distance(p, resolution, bpo) > 1e-9
        thr, counts = device_tuning(rec, cnt, R.edges(resolution), bpo)
        for g, (pg, mg) in enumerate(groups):
            n, wthr, wc = R.tuning_parts(pg, mg, resolution, bpo)
            np.testing.assert_array_equal(bits(thr[g]), bits(wthr))
            np.testing.assert_array_equal(counts[g], wc)
    # too small a buffer: the counter counts on, the group is left alone
    cnt2, rec2 = device_records(X, k_lo, k_hi, bin_hz, 64, per_clip)
    np.testing.assert_array_equal(cnt2.cpu().numpy(), n_host)
    thr, counts = device_tuning(rec2, cnt2, R.edges(0.01), 12)
    assert np.isnan(thr).all() and (counts == -1).all()


@pytest.mark.parametrize("cplx", [False, True])
def test_gpu_peak_dense_records_flush_mid_tile(cplx):
    """threshold 0 on independent magnitudes: a third of the bins are peaks, so every wave fills and hands over its LDS
    stage several times inside a tile (E.dense_fixture asserts that of the fixture).  The records must equal the dense
    peaks as a multiset with a capacity above the count, and the counter must count on with one below it."""
    x, S, p, m, per_wave_tile = E.dense_fixture(cplx)
    for per_clip in (False, True):
        groups = [(p[b], m[b]) for b in range(p.shape[0])] if per_clip else [(p, m)]
        want = [E.dense_pairs(pg, mg) for pg, mg in groups]
        big = max(len(w) for w in want) + 7
        for capacity in (big, 1000):
            cnt, rec = device_records(x, 0, S.shape[1], np.float32(1.0), capacity, per_clip, threshold=0.0)
            n_host, rec_host = cnt.cpu().numpy(), rec.cpu().numpy()
            for g, w in enumerate(want):
                assert int(n_host[g]) == len(w) > 1000
                if capacity == big:
                    np.testing.assert_array_equal(E.as_words(rec_host[g, :len(w)]), E.as_words(w))
                    assert np.isnan(rec_host[g, len(w):]).all()
                else:                           # every slot holds one of the peaks, none twice
                    got = E.as_words(rec_host[g])
                    assert len(np.unique(got)) == capacity and np.isin(got, E.as_words(w)).all()
    emu_cnt, emu_rec = eb.records(x, 0, S.shape[1], np.float32(1.0), big, threshold=0.0, per_clip=True)
    np.testing.assert_array_equal(emu_cnt.astype(np.int64), n_host)


@pytest.mark.parametrize("n", E.MEDIAN_NS)
def test_gpu_median_of_hand_made_records(n):
    rng = np.random.default_rng(n)
    for flavour in ("random", "equal", "two-valued"):
        mags = {"random": rng.gamma(1.0, 3.0, n), "equal": np.full(n, 2.5),
                "two-valued": np.where(np.arange(n) < n // 2, 1.25, 7.0)}[flavour].astype(np.float32)
        rng.shuffle(mags)
        pit = (440.0 * 2.0 ** rng.uniform(-2, 2, n)).astype(np.float32)
        rec = np.full((1, max(n, 1) + 5, 2), np.nan, np.float32)
        rec[0, :n, 0], rec[0, :n, 1] = mags, pit
        thr, counts = device_tuning(dev(rec), dev(np.array([n], np.int64)), R.edges(0.01), 12)
        want = R.median(mags)
        np.testing.assert_array_equal(bits(thr[0]), bits(want))
        assert R.nearest_edge_distance(pit) > 1e-9
        np.testing.assert_array_equal(counts[0], R.counts(pit[mags >= want]))


# ---------------------------------------------------------------------------------------------------------------------
# the public functions
# ---------------------------------------------------------------------------------------------------------------------
_sig = {}


def signal():
    if "y" not in _sig:
        _sig["y"] = R.tones(3, 173 * 128, 5, detune=0.2)
    return _sig["y"]


def test_gpu_piptrack_of_a_model_spectrum_is_the_model():
    X, S, p, m, k_lo, k_hi, bin_hz = E.tonal()
    for arg in (S, X):
        gp, gm = ap.piptrack(S=dev(arg), sr=SR)
        assert gp.shape == S.shape == (3, 257, 174) and gp.dtype == torch.float32 and gp.is_cuda
        np.testing.assert_array_equal(bits(gp.cpu().numpy()), bits(p))
        np.testing.assert_array_equal(bits(gm.cpu().numpy()), bits(m))
    one_p, one_m = ap.piptrack(S=S[1], sr=SR)
    assert one_p.shape == (257, 174)
    np.testing.assert_array_equal(bits(one_p.cpu().numpy()), bits(p[1]))
    ref = np.float32(3.0)
    wp, wm = R.piptrack(S, sr=SR, ref=ref, fmin=0.0, fmax=1e6)
    gp, gm = ap.piptrack(S=dev(S), sr=SR, ref=-3.0, fmin=0.0, fmax=1e6)
    np.testing.assert_array_equal(bits(gp.cpu().numpy()), bits(wp))
    rt = np.random.default_rng(3).uniform(0.5, 5.0, (3, 174)).astype(np.float32)
    wp, wm = R.piptrack(S, sr=SR, ref=rt)
    gp, gm = ap.piptrack(S=dev(S), sr=SR, ref=dev(rt))
    np.testing.assert_array_equal(bits(gm.cpu().numpy()), bits(wm))
    gp2, _ = ap.piptrack(S=dev(S), sr=SR, ref=np.max)
    np.testing.assert_array_equal(bits(gp2.cpu().numpy()), bits(p))


@pytest.mark.parametrize("layout", ["lines", "dense"])
def test_gpu_piptrack_from_audio_reads_the_spectrum_in_place(layout):
    """piptrack(y=y) is piptrack(S=stft(y)) in every bit under both spectrum layouts (B T >= 512 and T % 16 != 0: stft's
    rows are padded under "lines"), and the model applied to the device's own spectrum."""
    y = dev(signal())
    prev = ap.set_spectrum_layout(layout)
    try:
        Xd = ap.stft(y, n_fft=512, hop_length=128)
        assert Xd.shape == (3, 257, 174) and (Xd.is_contiguous() == (layout == "dense"))
        from_y = ap.piptrack(y=y, sr=SR, n_fft=512)
        from_s = ap.piptrack(S=Xd, sr=SR)
        from_mag = ap.piptrack(S=ap.magnitude(Xd), sr=SR)
    finally:
        ap.set_spectrum_layout(prev)
    for a, b in zip(from_y, from_s):
        assert torch.equal(a, b)
    S, wrong = R.magnitude(Xd.cpu().numpy())
    keep = ~wrong.any(axis=1)                                   # frames without a double-rounding tie in the model
    wp, wm = R.piptrack(S, sr=SR)
    np.testing.assert_array_equal(bits(from_y[0].cpu().numpy().transpose(0, 2, 1)[keep]), bits(wp.transpose(0, 2, 1)[keep]))
    np.testing.assert_array_equal(bits(from_y[1].cpu().numpy().transpose(0, 2, 1)[keep]), bits(wm.transpose(0, 2, 1)[keep]))
    assert keep.mean() > 0.99
    print(f"piptrack(y) [{layout}]: peaks {(wp > 0).mean():.4f} of the bins; magnitude(X) gave the same peaks: "
          f"{torch.equal(from_mag[0], from_y[0])}")


def test_gpu_estimate_tuning_paths_agree():
    y = dev(signal())
    Xd = ap.stft(y, n_fft=512, hop_length=128)
    S, wrong = R.magnitude(Xd.cpu().numpy())
    assert not wrong.any()
    kw = dict(sr=SR, n_fft=512, hop_length=128)
    for res, bpo in ((0.01, 12), (0.3, 36)):
        want = R.estimate_tuning(S, sr=SR, resolution=res, bins_per_octave=bpo)
        want_clip = R.estimate_tuning(S, sr=SR, resolution=res, bins_per_octave=bpo, per_clip=True)
        p, m = R.piptrack(S, sr=SR)
        assert R.nearest_edge_distance(p, res, bpo) > 1e-9
        a = ap.estimate_tuning(y=y, resolution=res, bins_per_octave=bpo, **kw)
        assert isinstance(a, float) and a == want
        assert ap.estimate_tuning(S=dev(S), sr=SR, resolution=res, bins_per_octave=bpo) == want
        assert ap.estimate_tuning(S=Xd, sr=SR, resolution=res, bins_per_octave=bpo) == want
        c = ap.estimate_tuning(y=y, resolution=res, bins_per_octave=bpo, per_clip=True, **kw)
        assert c.dtype == np.float64 and c.shape == (3,)
        np.testing.assert_array_equal(c, want_clip)
        # every clip alone, and in another order: independent of its neighbours
        for b in range(3):
            assert ap.estimate_tuning(y=y[b], resolution=res, bins_per_octave=bpo, **kw) == want_clip[b]
        np.testing.assert_array_equal(ap.estimate_tuning(y=y.flip(0), resolution=res, bins_per_octave=bpo, per_clip=True, **kw), want_clip[::-1])
        # pitch_tuning of the dense peaks above the median, on the device tensor and on the host
        gp, gm = ap.piptrack(S=dev(S), sr=SR)
        thr = float(R.median(m[p > 0]))
        sel = gp[(gm >= thr) & (gp > 0)]
        assert ap.pitch_tuning(sel, resolution=res, bins_per_octave=bpo) == want
        assert ap.pitch_tuning(sel.cpu().numpy(), resolution=res, bins_per_octave=bpo) == want
        assert ap.pitch_tuning(gp, resolution=res, bins_per_octave=bpo) == R.pitch_tuning(p, res, bpo)
    # the rerun with the exact capacity
    assert ap.estimate_tuning(y=y, _capacity=50, **kw) == R.estimate_tuning(S, sr=SR)
    k_lo, k_hi = R.bin_range(SR, 512, 150.0, 4000.0, 257)
    n_bins, edges = M._tuning_bins(0.01, 12)
    n_want, thr_want, counts_want = R.tuning_parts(*R.piptrack(S, sr=SR))
    for capacity, runs_want in ((50, 2), (n_want - 1, 2), (n_want, 1), (None, 1)):
        n, thr, counts, runs = M._tuning_records(dev(S), k_lo, k_hi, 0.1, 0, 0.0, None, float(np.float32(SR / 512)), False, n_bins,
                                                 edges, 12, capacity)
        assert runs == runs_want and int(n[0]) == n_want, capacity
        np.testing.assert_array_equal(bits(thr[0]), bits(thr_want))
        np.testing.assert_array_equal(counts[0], counts_want)
    # a non-default stream
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s1 = ap.estimate_tuning(y=y, **kw)
        sp, sm = ap.piptrack(y=y, **kw)
    side.synchronize()
    bp, bm = ap.piptrack(y=y, **kw)
    assert s1 == R.estimate_tuning(S, sr=SR) and torch.equal(sp, bp) and torch.equal(sm, bm)
    # nothing to estimate from
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert ap.estimate_tuning(S=dev(np.zeros((9, 5), np.float32)), sr=SR) == 0.0
        assert ap.pitch_tuning(dev(np.zeros(7, np.float32))) == 0.0
    assert len(w) == 2 and all(issubclass(i.category, UserWarning) for i in w)


# The NumPy model on this fixture (a float64 STFT rounded to complex64; tests/test_piptrack_api.py asserts these on the
# CPU): -0.32 for d = -0.3, -0.01 for d = 0.0, 0.21 for d = 0.23, so |estimate - d| is 0.02, 0.01, 0.02: the result is the
# LEFT edge of the fullest bin and the parabola on a Hann main lobe pulls towards the bin centre.  The margin of two
# histogram bins (0.02) holds for the model and is not widened.  Top pitch class share of the model, tuned against
# tuning 0: 0.4208 / 0.3694, 0.41882 / 0.41881, 0.4241 / 0.3893.
@pytest.mark.parametrize("d", [-0.3, 0.0, 0.23])
def test_gpu_detuned_harmonics_end_to_end(d):
    y = dev(R.harmonics(d))
    est = ap.estimate_tuning(y=y, sr=SR)
    print(f"d = {d}: estimate_tuning {est:+.2f}")
    assert abs(est - d) <= 0.02 + 1e-12
    tuned = ap.chroma_stft(y=y, sr=SR, tuning=est, norm=1).amax(dim=0)
    plain = ap.chroma_stft(y=y, sr=SR, tuning=0.0, norm=1).amax(dim=0)
    print(f"   top pitch class share per frame: {float(tuned.mean()):.4f} tuned, {float(plain.mean()):.4f} at tuning 0")
    assert float(tuned.mean()) >= float(plain.mean())
