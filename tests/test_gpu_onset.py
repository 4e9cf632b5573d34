"""GPU: onset_strength / peak_pick / onset_detect through the public API against the float64 definitions in
tests/onset_ref.py: the shapes, parameters and bounds of test_emu_onset.py (its docstring derives them), then what only
the device can show - both routes to the envelope in identical bits, layouts, batch independence, a click train."""

import numpy as np
import pytest
import torch

import onset_ref as R
from onset_ref import DELTAS, PEAK_T, PEAK_WINDOWS, SHAPES, SHIFT_KINDS, lags, max_sizes, rows_for, spectrum
from onset_ref import strength_check as check

import mlx_audio_primitives_amd as ap

pytestmark = pytest.mark.gpu

IDS = ["x".join(map(str, s)) for s in SHAPES]


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the shared cases are read-only)


def padded(a, pad):
    """A device view of `a` whose rows are `pad` (NaN) columns apart from dense."""
    buf = torch.full(a.shape[:-1] + (a.shape[-1] + pad,), float("nan"), dtype=torch.float32, device="cuda")
    buf[..., :a.shape[-1]] = dev(a)
    return buf[..., :a.shape[-1]]


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gpu_onset_strength(shape):
    """Every lag x max_size of the shape, centre on and off at (2048, 512) and (512, 128) in turn, dense and padded S."""
    S = spectrum(shape)
    B, M, T = shape
    Sd, Sp = dev(S), padded(S, 3)
    worst, k = 0.0, 0
    for lag in lags(T):
        for ms in max_sizes(M):
            for center, n_fft, hop in (SHIFT_KINDS if (lag, ms) in ((1, 1), (2, 3)) else [SHIFT_KINDS[k % 4]]):
                want = R.onset_strength(S, lag, ms, shift=R.shift_of(lag, center, n_fft, hop))
                got = ap.onset_strength(S=(Sd, Sp)[k % 2], lag=lag, max_size=ms, center=center, n_fft=n_fft, hop_length=hop)
                assert got.shape == (B, T) and got.dtype == torch.float32 and got.is_contiguous()
                got = host(got)
                assert not np.isnan(got).any()
                worst = max(worst, check(got, want, M, (lag, ms, center, n_fft, hop)))
                if lag >= T:
                    assert not got.any()
                k += 1
    one = ap.onset_strength(S=Sd[0], lag=1, max_size=3)                               # (M, T) -> (T,)
    assert one.shape == (T,) and torch.equal(one, ap.onset_strength(S=Sd, lag=1, max_size=3)[0])
    print(f"onset strength {shape}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gpu_onset_strength_ref_route(shape):
    S = spectrum(shape)
    B, M, T = shape
    ref = (S + np.random.default_rng(3).standard_normal(shape).astype(np.float32) * 10).astype(np.float32)
    Sd, refd, refp = dev(S), dev(ref), padded(ref, 4)
    worst = 0.0
    for i, lag in enumerate(lags(T)):
        for ms in (1, 5):
            want = R.onset_strength(S, lag, ms, ref=ref, shift=lag + 2)
            got = host(ap.onset_strength(S=Sd, lag=lag, max_size=ms, ref=(refd, refp)[i % 2]))
            worst = max(worst, check(got, want, M, (lag, ms)))
    with pytest.raises(ValueError, match="ref must have the shape of S"):
        ap.onset_strength(S=Sd, ref=torch.zeros((B, M + 1, T), device="cuda"))
    print(f"onset strength ref route {shape}: worst error / bound {worst:.3f}")


_audio = {}


def clips():
    """2 x 132096 samples (T = 259: a padded-row mel view, B T >= 512 and T % 8 != 0); the second half of clip 1 is
    digital silence, so that top_db = 80 clips a good part of the array."""
    if not _audio:
        rng = np.random.default_rng(42)
        y = (rng.standard_normal((2, 132096)) * np.linspace(1.0, 0.01, 132096)).astype(np.float32)
        y[1] *= 0.5                                     # clip 0 holds the maximum the whole batch is clipped against
        y[1, 66048:] = 0.0
        yd = dev(y)
        mel = ap.melspectrogram(yd)
        _audio.update(y=yd, mel=mel, db=ap.power_to_db(mel), env=ap.onset_strength(y=yd))
    return _audio


def test_gpu_routes_agree_bit_for_bit():
    """onset_strength(y=y) == onset_strength(S=power_to_db(melspectrogram(y))) in every bit, for the default and for a
    running maximum; and both are the definition applied to the device's own dB values."""
    a = clips()
    mel, db, env = a["mel"], a["db"], a["env"]
    assert mel.shape == (2, 128, 259) and not mel.is_contiguous() and mel.stride(1) == 264
    assert env.shape == (2, 259) and env.dtype == torch.float32
    dbh = host(db)
    floor = dbh.min()
    assert floor == np.float32(dbh.max() - np.float32(80.0)) and 0.2 < np.mean(dbh == floor) < 0.8       # top_db clips
    assert torch.equal(env, ap.onset_strength(S=db))
    for lag, ms in ((2, 3), (1, 4)):
        assert torch.equal(ap.onset_strength(y=a["y"], lag=lag, max_size=ms), ap.onset_strength(S=db, lag=lag, max_size=ms))
    check(host(env), R.onset_strength(dbh, 1, 1, shift=3), 128, "y route")
    assert host(env)[:, 3:].max() > 1.0
    # kwargs reach the mel spectrogram: 64 bands at hop 256 -> T = 517, shift = 1 + 2048 // 512
    e2 = ap.onset_strength(y=a["y"], n_mels=64, hop_length=256)
    d2 = ap.power_to_db(ap.melspectrogram(a["y"], n_mels=64, hop_length=256))
    assert e2.shape == (2, 517) and torch.equal(e2, ap.onset_strength(S=d2, hop_length=256))
    assert not host(e2)[:, :5].any()


def test_gpu_layouts_agree_bit_for_bit():
    """A padded-row S view and its contiguous copy; a non-contiguous S that is no padded-row view is copied."""
    mel = clips()["mel"]
    assert not mel.is_contiguous()
    S = ap.power_to_db(mel)
    view = torch.full((2, 128, 264), float("nan"), device="cuda")[:, :, :259]
    view.copy_(S)
    for lag, ms in ((1, 1), (3, 5)):
        want = ap.onset_strength(S=S, lag=lag, max_size=ms)
        assert torch.equal(ap.onset_strength(S=view, lag=lag, max_size=ms), want)
        assert torch.equal(ap.onset_strength(S=view.contiguous(), lag=lag, max_size=ms), want)
        assert torch.equal(ap.onset_strength(S=S.transpose(1, 2).contiguous().transpose(1, 2), lag=lag, max_size=ms), want)
        assert torch.equal(ap.onset_strength(S=host(S), lag=lag, max_size=ms), want)             # NumPy in
    # a column-offset view: the padding behind its last row is nobody's, whatever the allocator put there
    big = torch.full((2, 128, 270), float("nan"), device="cuda")
    off = big[:, :, 5:264]
    off.copy_(S)
    assert torch.equal(ap.onset_strength(S=off, max_size=3), ap.onset_strength(S=S, max_size=3))
    assert torch.equal(ap.onset_detect(onset_envelope=off[:, 0, :], sparse=False), ap.onset_detect(onset_envelope=S[:, 0, :], sparse=False))


def test_gpu_clip_alone_equals_clip_in_batch():
    a = clips()
    for b in range(2):
        for ms in (1, 3):
            assert torch.equal(ap.onset_strength(S=a["db"][b], max_size=ms), ap.onset_strength(S=a["db"], max_size=ms)[b])
    # from audio, top_db clips against the maximum of the whole batch, which clip 0 holds: alone it sees the same floor
    assert torch.equal(ap.onset_strength(y=a["y"][0]), a["env"][0])
    assert torch.equal(ap.onset_strength(y=a["y"][:1])[0], a["env"][0])
    env = a["env"]
    kw = dict(onset_envelope=env, sparse=False, backtrack=True)
    batch = ap.onset_detect(**kw)
    for b in range(2):
        assert torch.equal(ap.onset_detect(**dict(kw, onset_envelope=env[b])), batch[b])


@pytest.mark.parametrize("windows", PEAK_WINDOWS, ids=["-".join(map(str, w)) for w in PEAK_WINDOWS])
@pytest.mark.parametrize("T", PEAK_T)
def test_gpu_peak_pick(T, windows):
    """wait x delta x normalize x backtrack on the rows of test_emu_onset.py, all rows of a case in one launch:
    peak_pick (no normalisation, the NaN row picked as NumPy's max and mean say) and onset_detect (normalize on and off;
    the NaN and the all-zero row yield nothing)."""
    rows = rows_for(T, windows)
    names = list(rows)
    x = np.stack([rows[k] for k in names])
    xd = dev(x)
    energy = np.random.default_rng(T).random(x.shape).astype(np.float32)
    ed = dev(energy)
    wk = dict(zip(("pre_max", "post_max", "pre_avg", "post_avg"), windows))
    n_picked = 0
    for delta in DELTAS:
        raw = {k: rows[k].astype(np.float64) for k in names}
        seen = {norm: {k: R.seen(rows[k], norm) for k in names} for norm in (False, True)}
        cand = {}
        for tag, vals in (("pick", raw), (False, seen[False]), (True, seen[True])):
            for k, v in vals.items():
                if v is not None:
                    assert R.decisive(v, windows, delta, on_grid=tag is not True), (k, tag, delta)   # the precondition
                    cand[tag, k] = R.candidates(v, *windows, delta)[0]
        for wait in sorted({0, 1, 10, T}):
            got = host(ap.peak_pick(xd, delta=delta, wait=wait, sparse=False, **wk))
            assert got.dtype == np.bool_ and got.shape == x.shape
            for i, k in enumerate(names):
                want = R.greedy(cand["pick", k], wait)
                assert np.array_equal(got[i], want), ("peak_pick", k, delta, wait)
                n_picked += int(want.sum())
            one = ap.peak_pick(xd[0], delta=delta, wait=wait, **wk)                       # sparse: int64 indices
            assert one.dtype == torch.int64 and one.is_cuda and np.array_equal(host(one), np.flatnonzero(got[0]))
            for norm in (False, True):
                for bt in (False, True):
                    for en in ((None, energy) if bt and wait == 1 else (None,)):
                        got = host(ap.onset_detect(onset_envelope=xd, normalize=norm, backtrack=bt, sparse=False, delta=delta,
                                                   wait=wait, energy=None if en is None else ed, **wk))
                        for i, k in enumerate(names):
                            v = seen[norm][k]
                            if v is None:
                                want = np.zeros(T, bool)
                            else:
                                want = R.greedy(cand[norm, k], wait)
                                if bt:
                                    want = R.backtrack(want, v if en is None else en[i])
                            assert np.array_equal(got[i], want), ("onset_detect", k, norm, delta, wait, bt, en is not None)
    assert n_picked > 0


def test_gpu_click_train():
    """Clicks every 0.25 s over low noise, 2 s at 22050 Hz: one onset per click, within 2 frames of click // 512;
    backtracking only moves them earlier; samples and time are the frames converted; a batch needs sparse=False."""
    sr, hop = 22050, 512
    rng = np.random.default_rng(0)
    y = (1e-4 * rng.standard_normal(2 * sr)).astype(np.float32)
    starts = [int(round(0.25 * sr * i)) for i in range(1, 8)]
    burst = (np.exp(-np.arange(600) / 100.0) * rng.standard_normal(600)).astype(np.float32)
    for s in starts:
        y[s:s + 600] += burst
    yd = dev(y)
    frames = ap.onset_detect(y=yd, sr=sr)
    assert frames.dtype == torch.int64 and frames.is_cuda
    f = host(frames)
    expect = np.array([s // hop for s in starts])
    assert len(f) == len(expect) and np.all(np.abs(f - expect) <= 2), (f, expect)
    back = host(ap.onset_detect(y=yd, sr=sr, backtrack=True))
    assert len(back) == len(f) and np.all(back <= f), (back, f)
    env = ap.onset_strength(y=yd, sr=sr)
    assert torch.equal(ap.onset_detect(onset_envelope=env, sr=sr), frames)
    samples = ap.onset_detect(y=yd, sr=sr, units="samples")
    assert samples.dtype == torch.int64 and np.array_equal(host(samples), f * hop)
    times = ap.onset_detect(y=yd, sr=sr, units="time")
    assert times.dtype == torch.float64 and np.array_equal(host(times), f * hop / float(sr))
    mask = ap.onset_detect(y=yd, sr=sr, sparse=False)
    assert mask.dtype == torch.bool and mask.shape == env.shape and np.array_equal(np.flatnonzero(host(mask)), f)
    both = torch.stack([yd, 0.5 * yd])
    with pytest.raises(ValueError, match="sparse=True needs 1D input"):
        ap.onset_detect(y=both, sr=sr)
    with pytest.raises(ValueError, match="sparse=True needs 1D input"):
        ap.peak_pick(torch.stack([env, env]), pre_max=1, post_max=1, pre_avg=4, post_avg=5, delta=0.07, wait=1)
    mb = ap.onset_detect(y=both, sr=sr, sparse=False)
    assert mb.shape == (2, env.shape[0]) and np.array_equal(np.flatnonzero(host(mb[0])), f)


def test_gpu_degenerate_inputs():
    z = torch.zeros(50, device="cuda")
    assert ap.onset_detect(onset_envelope=z).numel() == 0
    bad = torch.rand(50, device="cuda")
    bad[7] = float("inf")
    assert ap.onset_detect(onset_envelope=bad).numel() == 0
    assert ap.onset_detect(onset_envelope=torch.zeros(0, device="cuda")).numel() == 0
    assert ap.peak_pick(torch.zeros((2, 0), device="cuda"), pre_max=1, post_max=1, pre_avg=1, post_avg=1, delta=0.0, wait=0,
                        sparse=False).shape == (2, 0)
    assert ap.onset_strength(S=torch.zeros((2, 0, 9), device="cuda")).shape == (2, 9)
    e = ap.onset_strength(y=torch.zeros((2, 0), device="cuda"))                  # no samples: one centred frame of zeros
    assert e.shape == (2, 1) and not host(e).any()
    e = ap.onset_strength(y=torch.zeros((2, 4096), device="cuda"), lag=1, center=False)
    assert e.shape == (2, 9) and not host(e).any()
    limit = 16384
    assert ap.onset_detect(onset_envelope=torch.rand(limit, device="cuda"), sparse=False).shape == (limit,)
    with pytest.raises(ValueError, match=str(limit)):
        ap.onset_detect(onset_envelope=torch.rand(limit + 1, device="cuda"))
