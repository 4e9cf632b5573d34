"""GPU: tempogram / tempo / beat_track through the public API (and once through the C ABI, for the guard bands and the
intermediates) against the float64 definitions in tests/rhythm_ref.py: the cases and bounds of test_emu_rhythm.py (its
docstring and rhythm_ref state them), then what only the device can show - the chain from audio, batch independence
with the period left on the device."""

import numpy as np
import pytest
import torch

import rhythm_ref as R

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _extension as _x

pytestmark = pytest.mark.gpu

FPS = 22050 / 512


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the shared cases are read-only)


def padded(a, pad):
    """A device view of `a` whose rows are `pad` (NaN) columns apart from dense."""
    buf = torch.full(a.shape[:-1] + (a.shape[-1] + pad,), float("nan"), dtype=torch.float32, device="cuda")
    buf[..., :a.shape[-1]] = dev(a)
    return buf[..., :a.shape[-1]]


def host(t):
    return t.cpu().numpy()


def banded(shape, dtype=torch.float32, fill=float("nan"), band=64):
    """(whole buffer, payload view): a flat device buffer of prod(shape) elements between two bands of `fill`."""
    n = int(np.prod(shape))
    raw = torch.full((n + 2 * band,), fill, dtype=dtype, device="cuda")
    return raw, raw[band:band + n].view(shape)


def bands_intact(raw, fill, band=64):
    edge = torch.cat([raw[:band], raw[-band:]])
    return bool(torch.isnan(edge).all()) if isinstance(fill, float) and np.isnan(fill) else bool((edge == fill).all())


def _tg_variants(n, W):
    out = [(True, True, "hann", 0), (True, False, "hann", 3), (True, True, "array", 5)]
    if n >= W:
        out += [(False, True, "hann", 2), (False, False, "array", 0)]
    return out


@pytest.mark.parametrize("shape", R.TG_SHAPES, ids=["x".join(map(str, s)) for s in R.TG_SHAPES])
def test_gpu_tempogram(shape, monkeypatch):
    """W <= 512 on the wave kernel and, with AP_TEMPOGRAM_GENERAL=1, on the general one (each against the reference, and
    against each other within the same atol); 513 and 600 fall back to the general kernel."""
    worst = {"wave": 0.0, "general": 0.0}
    for W in R.TG_WAVE_W + R.TG_GENERAL_W:
        for center, norm_inf, kind, pad in _tg_variants(shape[1], W):
            e, want, atol, window = R.tg_case(shape, W, center, norm_inf, kind)
            got = {}
            for route in (("wave", "general") if W in R.TG_WAVE_W else ("general",)):
                monkeypatch.setenv("AP_TEMPOGRAM_GENERAL", "1" if route == "general" else "0")
                g = ap.tempogram(onset_envelope=padded(e, pad) if pad else dev(e), win_length=W, center=center,
                                 window=window if kind == "hann" else dev(window), norm=np.inf if norm_inf else None)
                assert g.shape == want.shape and g.dtype == torch.float32 and g.is_contiguous()
                got[route] = host(g)
                assert not np.isnan(got[route]).any()
                ratio = float(np.max(np.abs(got[route] - want) / atol))
                worst[route] = max(worst[route], ratio)
                assert ratio <= 1.0, (route, shape, W, center, norm_inf, kind, ratio)
            if "wave" in got:
                assert float(np.max(np.abs(got["wave"] - got["general"]) / atol)) <= 1.0, (shape, W, center, norm_inf, kind)
    monkeypatch.setenv("AP_TEMPOGRAM_GENERAL", "0")
    e = R.tg_envelope(shape)
    one = ap.tempogram(onset_envelope=dev(e[0]), win_length=8)                           # (n,) -> (W, T)
    assert one.shape == (8, shape[1]) and torch.equal(one, ap.tempogram(onset_envelope=dev(e), win_length=8)[0])
    print(f"tempogram {shape}: worst error / atol, wave {worst['wave']:.3f}, general {worst['general']:.3f}")


@pytest.mark.parametrize("route", ["wave", "general"])
def test_gpu_tempogram_abi_bands_and_tile_sums(route):
    """Through the C ABI: the envelope rows strided between NaN bands, the tempogram and the tile sums between NaN bands
    that stay unwritten; the tile sums are the stored values added in frame order.  The wave route refuses W = 513."""
    from mlx_audio_primitives_amd.stft import _get_twiddles

    B, n, W = 3, 130, 344
    e = R.tg_envelope((B, n))
    src_raw, src = banded((B, n + 6))
    src[:, :n] = dev(e)
    w = dev(R.window_of("hann", W).astype(np.float32))
    lib = _x.lib()
    assert lib.ap_tempogram_fused(512) == 1 and lib.ap_tempogram_fused(513) == 0
    tw = _get_twiddles(1024, src.device).data_ptr() if route == "wave" else None
    n_agg = int(lib.ap_tempogram_agg_floats(B, n, W, 1))
    out_raw, out = banded((B, W, n))
    agg_raw, agg = banded((B, n_agg // (B * W), W))
    _x.check(_x.dlib(out.device).ap_tempogram_f32(src.data_ptr(), B, n, n + 6, w.data_ptr(), W, 1, 1, tw, out.data_ptr(),
                                                   agg.data_ptr(), _x.stream_ptr(out.device)))
    torch.cuda.synchronize()
    assert bands_intact(out_raw, float("nan")) and bands_intact(agg_raw, float("nan")) and bands_intact(src_raw, float("nan"))
    assert bool(torch.isnan(src[:, n:]).all()) and not bool(torch.isnan(out).any()) and not bool(torch.isnan(agg).any())
    got, tiles = host(out), host(agg)
    e_, want, atol, _ = R.tg_case((B, n), W, True, True, "hann")
    assert np.max(np.abs(got - want)) <= atol
    for tile in range(tiles.shape[1]):
        seq = np.zeros((B, W), np.float32)
        for t in range(64 * tile, min(64 * tile + 64, n)):
            seq = seq + got[:, :, t]
        assert np.array_equal(tiles[:, tile], seq)
    if route == "wave":
        w513 = torch.ones(513, device="cuda")
        big = torch.empty((1, 513, 600), device="cuda")
        rc = _x.dlib(out.device).ap_tempogram_f32(torch.ones(600, device="cuda").data_ptr(), 1, 600, 600, w513.data_ptr(), 513, 1, 1,
                                                  tw, big.data_ptr(), None, _x.stream_ptr(out.device))
        assert rc == _x.AP_ERR_UNSUPPORTED


@pytest.mark.parametrize("route", ["wave", "general"])
def test_gpu_tempogram_clip_alone_equals_clip_in_batch_and_zero_row(route, monkeypatch):
    monkeypatch.setenv("AP_TEMPOGRAM_GENERAL", "1" if route == "general" else "0")
    for shape, W in (((3, 130), 64), ((3, 130), 384), ((2, 5), 3)):
        e = R.tg_envelope(shape).copy()
        e[-1] = 0.0
        batch = ap.tempogram(onset_envelope=dev(e), win_length=W)
        for b in range(shape[0]):
            assert torch.equal(ap.tempogram(onset_envelope=dev(e[b]), win_length=W), batch[b])
        assert not bool(batch[-1].any()) and bool(batch[0].any())                      # zeros, not NaN
        assert not bool(ap.tempogram(onset_envelope=dev(e), win_length=W, norm=None)[-1].any())


# ---- tempo ------------------------------------------------------------------------------------------------------------
class _LogNormal:
    def logpdf(self, bpm):
        with np.errstate(divide="ignore", invalid="ignore"):
            return -0.5 * ((np.log(bpm) - np.log(100.0)) / 0.4) ** 2 - np.log(bpm)


def _index_of(bpm_value, W):
    k = np.flatnonzero(R.tempo_frequencies(W) == float(bpm_value))
    assert len(k) == 1
    return int(k[0])


@pytest.mark.parametrize("period,n", R.TEMPO_CASES)
def test_gpu_tempo(period, n, monkeypatch):
    W = R.tempo_window()
    e = R.click_train(n, period, seed=1)
    tg = R.tempogram(e[None], W)
    g = tg.mean(axis=-1, keepdims=True)
    ed = dev(e)
    tgd = ap.tempogram(onset_envelope=ed, win_length=W)
    for kw in (dict(), dict(max_tempo=None), dict(prior=_LogNormal()), dict(start_bpm=90.0, std_bpm=0.5)):
        want, ok = R.tempo_pick(g, R.log_prior(W, **kw))
        assert ok, (period, n, kw)                                   # the precondition
        got = ap.tempo(onset_envelope=ed, **kw)
        assert got.shape == (1,) and got.dtype == torch.float64
        assert _index_of(got[0], W) == int(want[0, 0]), (period, n, kw)
        monkeypatch.setenv("AP_TEMPOGRAM_GENERAL", "1")
        assert _index_of(ap.tempo(onset_envelope=ed, **kw)[0], W) == int(want[0, 0]), (period, n, kw)
        monkeypatch.setenv("AP_TEMPOGRAM_GENERAL", "0")
        assert _index_of(ap.tempo(tg=tgd, **kw)[0], W) == int(want[0, 0])             # tg= given against the envelope route
    both = ap.tempo(onset_envelope=torch.stack([ed, ed * 0.5]))
    assert both.shape == (2, 1) and both[0, 0] == ap.tempo(onset_envelope=ed)[0]


def test_gpu_tempo_per_frame():
    W = R.tempo_window()
    e = R.click_train(130, 11, seed=1)
    s = R.tempo_scores(R.tempogram(e[None], W), R.log_prior(W))[0]
    want = np.argmax(s, axis=0)
    srt = np.sort(np.where(np.isfinite(s), s, -np.inf), axis=0)
    ok = srt[-1] - srt[-2] > 64 * R.EPS * np.max(np.abs(np.where(np.isfinite(s), s, 0.0)), axis=0)
    assert ok.mean() > 0.9
    got = host(ap.tempo(onset_envelope=dev(e), aggregate=None))
    assert got.shape == (130,)
    assert np.array_equal(got[ok], R.tempo_frequencies(W)[want][ok])
    print(f"per-frame tempo: {int((~ok).sum())} of {len(ok)} columns not compared (no decisive reference): {np.flatnonzero(~ok).tolist()}")


# ---- beat tracking -----------------------------------------------------------------------------------------------------
BEAT_SETTINGS = [(100.0, True), (100.0, False), (400.0, True), (400.0, False)]


@pytest.mark.parametrize("T", R.BEAT_T)
def test_gpu_beat_track(T):
    n_beats = 0
    for P in R.BEAT_P:
        bpm = 60.0 * FPS / P
        for tightness, trim in BEAT_SETTINGS:
            cases = [(kind,) + R.beat_case(kind, T, P, tightness, trim) for kind in R.BEAT_KINDS]
            x = np.stack([c[1] for c in cases])
            tempo, mask = ap.beat_track(onset_envelope=padded(x, 3) if P % 2 else dev(x), bpm=bpm, tightness=tightness, trim=trim,
                                        sparse=False)
            assert mask.shape == x.shape and mask.dtype == torch.bool and tempo.shape == (len(cases),) and tempo.dtype == torch.float64
            tempo, mask = host(tempo), host(mask)
            for i, (kind, o, st, redraws) in enumerate(cases):
                assert redraws <= 8
                want = np.zeros(T, bool) if st is None else st["mask"]
                if st is not None:
                    R.check_rule(kind, T, P, st)                      # the precondition (and which rule it is)
                assert np.array_equal(mask[i], want), (kind, T, P, tightness, trim, np.flatnonzero(mask[i]), np.flatnonzero(want))
                assert tempo[i] == (bpm if want.any() else 0.0)
                n_beats += int(want.sum())
    assert n_beats > 0 or T < 3
    # 1D input, the units
    o, st, _ = R.beat_case("clicks", T, 8)
    tempo, frames = ap.beat_track(onset_envelope=dev(o), bpm=60.0 * FPS / 8)
    want = np.flatnonzero(st["mask"]) if st is not None else np.zeros(0, int)
    assert tempo.shape == () and frames.dtype == torch.int64 and np.array_equal(host(frames), want)
    assert np.array_equal(host(ap.beat_track(onset_envelope=dev(o), bpm=60.0 * FPS / 8, units="samples")[1]), want * 512)
    np.testing.assert_allclose(host(ap.beat_track(onset_envelope=dev(o), bpm=60.0 * FPS / 8, units="time")[1]), want * 512 / 22050)


def test_gpu_beat_track_abi_intermediates():
    """L, C and link through the C ABI, every buffer between guard bands."""
    T = 130
    lib = _x.lib()
    for P, tightness in ((8, 100.0), (3, 400.0), (64, 100.0)):
        kinds = ["clicks", "random", "spike", "zero"]
        cases = [R.beat_case(k, T, P, tightness, True) for k in kinds]
        B = len(cases)
        src_raw, src = banded((B, T + 5))
        src[:, :T] = dev(np.stack([c[0] for c in cases]))
        per = torch.full((B,), P, dtype=torch.int32, device="cuda")
        mask_raw, mask = banded((B, T), torch.uint8, 0xFF)
        cnt_raw, cnt = banded((B,), torch.int32, -7)
        L_raw, L = banded((B, T))
        C_raw, C = banded((B, T))
        link_raw, link = banded((B, T), torch.int32, -2 ** 31)
        _x.check(_x.dlib(src.device).ap_beat_track_f32(src.data_ptr(), B, T, T + 5, per.data_ptr(), tightness, 1, mask.data_ptr(),
                                                       cnt.data_ptr(), L.data_ptr(), C.data_ptr(), link.data_ptr(),
                                                       _x.stream_ptr(src.device)))
        torch.cuda.synchronize()
        assert bands_intact(mask_raw, 0xFF) and bands_intact(cnt_raw, -7) and bands_intact(link_raw, -2 ** 31)
        assert bands_intact(L_raw, float("nan")) and bands_intact(C_raw, float("nan")) and bands_intact(src_raw, float("nan"))
        assert bool(torch.isnan(src[:, T:]).all())
        mask, cnt, L, C, link = host(mask), host(cnt), host(L), host(C), host(link)
        for i, (o, st, _) in enumerate(cases):
            if st is None:
                assert not mask[i].any() and cnt[i] == 0 and not L[i].any() and not C[i].any() and (link[i] == -1).all()
                continue
            rl = float(np.max(np.abs(L[i] - st["L"]) / R.L_bound(st, P)))
            rc = float(np.max(np.abs(C[i] - st["C"]) / R.C_bound(st, P, tightness)))
            print(f"beat_track P = {P}, {kinds[i]}: L error / bound {rl:.3f}, C {rc:.3f}")
            assert rl <= 1.0 and rc <= 1.0
            R.check_rule(kinds[i], T, P, st, C[i])
            chain = st["all_beats"]
            assert np.array_equal(link[i][chain], st["link"][chain]) and np.array_equal(link[i] < 0, st["link"] < 0)
            assert np.array_equal(mask[i].astype(bool), st["mask"]) and cnt[i] == len(st["beats"])


def test_gpu_beat_track_bare_spike_pins_the_tie_break():
    """One onset among exact zeros: exact ties in the DP go to the largest d.  L, C and the links equal the float32
    restatement rhythm_ref.beat_dp_f32 in every bit (see test_emu_rhythm.py)."""
    for T, P, tightness in ((65, 8, 100.0), (130, 22, 100.0), (63, 2, 400.0), (64, 3, 100.0), (431, 64, 100.0)):
        o = R.beat_row("bare_spike", T, P, seed=T)
        L32, C32, link32 = R.beat_dp_f32(o, P, tightness)
        src = dev(o[None])
        per = torch.full((1,), P, dtype=torch.int32, device="cuda")
        mask = torch.empty((1, T), dtype=torch.uint8, device="cuda")
        cnt = torch.empty(1, dtype=torch.int32, device="cuda")
        L, C = torch.empty((1, T), device="cuda"), torch.empty((1, T), device="cuda")
        link = torch.empty((1, T), dtype=torch.int32, device="cuda")
        _x.check(_x.dlib(src.device).ap_beat_track_f32(src.data_ptr(), 1, T, T, per.data_ptr(), tightness, 1, mask.data_ptr(),
                                                       cnt.data_ptr(), L.data_ptr(), C.data_ptr(), link.data_ptr(),
                                                       _x.stream_ptr(src.device)))
        assert np.array_equal(host(L)[0], L32) and np.array_equal(host(C)[0], C32), (T, P)
        assert np.array_equal(host(link)[0], link32), (T, P)


def test_gpu_beat_track_longest_row():
    T = 16384
    o, st, redraws = R.beat_case("clicks", T, 64, 400.0)
    assert st is not None and redraws <= 8
    R.check_rule("clicks", T, 64, st)
    tempo, frames = ap.beat_track(onset_envelope=dev(o), bpm=60.0 * FPS / 64, tightness=400.0)
    assert np.array_equal(host(frames), np.flatnonzero(st["mask"])) and len(frames) > 200
    with pytest.raises(ValueError, match="16384"):
        ap.beat_track(onset_envelope=torch.ones(T + 1, device="cuda"), bpm=120.0)


def _click_track(seconds=10.0, sr=22050, bpm=120.0):
    rng = np.random.default_rng(3)
    y = 1e-3 * rng.standard_normal(int(seconds * sr))
    starts = np.arange(0.25, seconds - 0.1, 60.0 / bpm)
    burst = np.exp(-np.arange(400) / 80.0) * np.sin(2 * np.pi * 1000.0 * np.arange(400) / sr)
    for s in starts:
        i = int(round(s * sr))
        y[i:i + 400] += burst
    return y.astype(np.float32), starts * sr / 512


def test_gpu_beat_track_from_audio_recovers_a_click_track():
    """The whole chain on the device: onset_strength -> tempogram tile sums -> pick -> beat tracker, nothing read back in
    between.  120 bpm clicks: the tempo lag equals the float64 reference's on the same envelope (decisive: asserted), the
    beats lie within one frame of the clicks."""
    y, click_frames = _click_track()
    yd = dev(y)
    env = ap.onset_strength(y=yd)
    W = R.tempo_window()
    g = R.tempogram(host(env)[None].astype(np.float64), W).mean(axis=-1, keepdims=True)
    want, ok = R.tempo_pick(g, R.log_prior(W))
    assert ok
    tempo, beats = ap.beat_track(y=yd)
    assert _index_of(tempo, W) == int(want[0, 0]) and abs(float(tempo) - 120.0) < 4.0
    beats = host(beats)
    assert len(beats) >= len(click_frames) - 3
    # a beat is a frame index: compare with the frame a click falls in (centred frames: the nearest t to sample / hop)
    assert all(np.min(np.abs(np.round(click_frames) - b)) <= 1 for b in beats), (beats, click_frames)
    # the same through the envelope, the mask and the other units
    tempo2, mask = ap.beat_track(onset_envelope=env, sparse=False)
    assert tempo2 == tempo and np.array_equal(np.flatnonzero(host(mask)), beats)
    assert np.array_equal(host(ap.beat_track(y=yd, units="samples")[1]), beats * 512)


def test_gpu_beat_track_row_alone_equals_row_in_batch():
    """Without bpm=: every row's period comes from its own tempo pick on the device."""
    rows = np.stack([R.click_train(431, p, seed=2) for p in (11, 22, 43)] + [np.zeros(431, np.float32)])
    tempo, mask = ap.beat_track(onset_envelope=dev(rows), sparse=False)
    assert float(tempo[3]) == 0.0 and not bool(mask[3].any()) and bool(mask[:3].any(dim=1).all())
    assert len(set(host(tempo[:3]))) > 1
    for b in range(4):
        t1, m1 = ap.beat_track(onset_envelope=dev(rows[b]), sparse=False)
        assert t1 == tempo[b] and torch.equal(m1, mask[b])
