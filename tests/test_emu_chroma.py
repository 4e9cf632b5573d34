"""CPU: the chroma kernels (csrc/kernels_chroma.h) on the SIMT emulator, through the C entries' twins, against the
float64 definitions and the derived bound of tests/chroma_ref.py.  Every buffer lies between NaN bands and every row
has NaN pad columns behind it (tests/emu/emu_chroma_bind.py): a read outside a row puts a NaN into a sum, a write
outside is seen directly.  Every accuracy test prints its worst error / bound (-s)."""

import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

import chroma_ref as R

import mlx_audio_primitives_amd as ap

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_chroma_bind as eb  # noqa: E402

M = importlib.import_module("mlx_audio_primitives_amd.chroma")

CONSTS = eb.constants()
CAP = CONSTS["max_out"]
TILE = CONSTS["cens_tile"]
SMOOTH = CONSTS["max_smooth"]
INF = np.inf

# (K, n_out, T, B, in_kind, w given, norm, pre_l1, threshold: None / 0 / "mid", pad_in, pad_out).  Every K of
# {1, 3, 4, 5, 84, 252, 257, 1025}, n_out of {1, 6, 12, 13, 36, cap}, T of {1, 63, 64, 65, 129}, B of {1, 3}, in_kind,
# norm, pre_l1 and threshold setting occurs, each with dense signed w; w = NULL (K = n_out) with every in_kind.
FOLD_CASES = (
    (1, 1, 1, 1, 0, True, None, False, None, 0, 0),
    (3, 6, 63, 3, 1, True, 1, True, None, 1, 0),
    (4, 12, 64, 1, 2, True, 2, False, 0.0, 0, 2),
    (5, 13, 65, 3, 0, True, INF, False, "mid", 3, 1),
    (84, 36, 129, 1, 1, True, INF, False, 0.0, 0, 0),
    (252, 12, 65, 3, 1, True, 2, False, "mid", 5, 3),
    (257, CAP, 63, 1, 2, True, 2, True, "mid", 1, 1),
    (1025, 12, 129, 1, 2, True, INF, False, None, 2, 0),
    (1025, CAP, 64, 1, 0, True, None, False, None, 0, 0),
    (84, 6, 129, 3, 0, True, None, True, None, 1, 2),
    (252, 36, 1, 3, 1, True, 1, True, 0.0, 0, 1),
    (257, 1, 65, 1, 1, True, INF, False, None, 0, 0),
    (12, 12, 65, 3, 0, False, 2, False, None, 2, 1),
    (1, 1, 1, 1, 2, False, None, True, None, 0, 0),
    (CAP, CAP, 63, 1, 1, False, 1, False, "mid", 1, 0),
    (13, 13, 64, 3, 2, False, INF, True, 0.0, 0, 3),
)
FOLD_IDS = ["K%d-n%d-T%d-B%d-kind%d-%s-norm%s-l1%d-thr%s" % (c[0], c[1], c[2], c[3], c[4], "w" if c[5] else "eye", c[6], c[7], c[8])
            for c in FOLD_CASES]


def fold_case(case):
    """(x, w, keyword arguments of eb.fold and R.fold) of a sweep case; the mid-range threshold is the median of the
    float64 values it is compared with."""
    K, n_out, T, B, kind, has_w, norm, pre_l1, thr, pad_in, pad_out = case
    i = FOLD_CASES.index(case) if case in FOLD_CASES else 99
    x = R.spectrum(B, K, T, kind, seed=i)
    w = R.matrix(n_out, K, seed=i) if has_w else None
    if thr == "mid":
        before, _, _ = R.fold(x, kind, w, CONSTS, pre_l1=pre_l1)
        thr = float(np.float32(np.median(before)))
    return x, w, dict(pre_l1=pre_l1, threshold=thr, norm=norm), dict(pad_in=pad_in, pad_out=pad_out, in_kind=kind)


def test_the_sweeps_cover_what_they_claim():
    col = lambda i, cases: {c[i] for c in cases}                 # noqa: E731
    with_w = [c for c in FOLD_CASES if c[5]]
    assert col(0, with_w) == {1, 3, 4, 5, 84, 252, 257, 1025} and col(1, with_w) == {1, 6, 12, 13, 36, CAP}
    assert col(2, FOLD_CASES) == {1, 63, 64, 65, 129} and col(3, FOLD_CASES) == {1, 3}
    assert col(4, with_w) == {0, 1, 2} and col(4, [c for c in FOLD_CASES if not c[5]]) == {0, 1, 2}
    assert col(6, FOLD_CASES) == {None, 1, 2, INF} and col(7, FOLD_CASES) == {False, True} and col(8, FOLD_CASES) == {None, 0.0, "mid"}
    assert any(c[9] for c in FOLD_CASES) and any(c[10] for c in FOLD_CASES)
    assert col(0, CENS_CASES) == {1, 12, 36} and col(2, CENS_CASES) == {0, 1, 3, 43, SMOOTH} and col(3, CENS_CASES) == {None, 1, 2, INF}
    assert col(1, CENS_CASES) == {1, 2, 20, 21, 41, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3}
    assert CAP >= 36 and SMOOTH >= 129


@pytest.mark.parametrize("case", FOLD_CASES, ids=FOLD_IDS)
def test_emu_fold_sweep(case):
    x, w, kw, lay = fold_case(case)
    got = eb.fold(x, w, **kw, **lay)
    want, bound, keep = R.fold(x, case[4], w, CONSTS, **kw)
    ratio = R.check(got, want, bound, keep, case)
    assert eb.geometry()["accumulators"] >= case[1]
    print(f"fold {FOLD_IDS[FOLD_CASES.index(case)]}: worst error / bound {ratio:.4f}, left out {100 * (1 - keep.mean()):.3f} %")


@pytest.mark.parametrize("case", [FOLD_CASES[i] for i in (5, 6, 12, 15)], ids=[FOLD_IDS[i] for i in (5, 6, 12, 15)])
def test_emu_fold_a_clip_alone_equals_the_clip_in_a_batch_and_the_grid_changes_no_bit(case):
    K, n_out, T, B, kind = case[:5]
    x, w, kw, lay = fold_case(case)
    x = R.spectrum(3, K, 129, kind, seed=77) if T < 129 or B < 3 else x
    base = eb.fold(x, w, **kw, **lay)
    for b in range(x.shape[0]):
        alone = eb.fold(x[b:b + 1], w, **kw, **lay)
        assert np.array_equal(alone.view(np.uint32), base[b:b + 1].view(np.uint32)), f"clip {b} alone differs from the batch"
    for grid in (1, 2, 5):
        again = eb.fold(x, w, grid=grid, **kw, **lay)
        assert eb.geometry()["grid"] == grid
        assert np.array_equal(again.view(np.uint32), base.view(np.uint32)), f"grid {grid} changed a bit"


@pytest.mark.parametrize("norm", R.NORMS, ids=lambda n: f"norm{n}")
def test_emu_fold_zero_frames_stay_zero_and_the_largest_entry_is_one(norm):
    x = np.array(R.spectrum(2, 84, 70, 1, seed=5))
    x[0, :, 3] = 0
    x[1, :, 64:] = 0
    w = R.matrix(12, 84, seed=5)
    for pre_l1 in (False, True):
        got = eb.fold(x, w, norm=norm, pre_l1=pre_l1, threshold=0.0)
        assert not got[0, :, 3].any() and not got[1, :, 64:].any(), "an all-zero frame is not all zero"
        assert not np.signbit(got[0, :, 3]).any()
        if norm == INF:
            live = np.abs(got).max(axis=1)
            want, _, _ = R.fold(x, 1, w, CONSTS, norm=norm, pre_l1=pre_l1, threshold=0.0)
            nonzero = np.abs(want).max(axis=1) > 0
            assert np.all(live[nonzero] == 1.0), "the largest entry of a frame is not exactly 1"
            assert np.all(live[~nonzero] == 0.0)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_emu_fold_a_nan_stays_in_its_frame(kind):
    x = np.array(R.spectrum(2, 37, 130, kind, seed=6))
    w = R.matrix(12, 37, seed=6)
    clean = eb.fold(x, w, in_kind=kind, norm=2, pre_l1=True, threshold=0.0)
    x[0, 5, 17] = np.nan
    x[1, 36, 64] = np.nan
    got = eb.fold(x, w, in_kind=kind, norm=2, pre_l1=True, threshold=0.0, allow_nan=True)
    assert np.isnan(got[0, :, 17]).all() and np.isnan(got[1, :, 64]).all()
    mask = np.ones(got.shape, bool)
    mask[0, :, 17] = False
    mask[1, :, 64] = False
    assert np.array_equal(got[mask].view(np.uint32), clean[mask].view(np.uint32)), "a NaN reached another frame"


def test_emu_fold_threshold_keeps_the_value_at_the_threshold():
    """a_c < threshold -> 0 is strict: with the identity and a real input the sums are the inputs themselves, so an
    element equal to the threshold stays and the next float32 below it goes."""
    thr = np.float32(0.3)
    x = np.array(R.spectrum(2, 12, 70, 0, seed=8))
    x[0, 3, 5] = thr
    x[0, 4, 5] = np.nextafter(thr, np.float32(0))
    x[1, 0, 69] = thr
    got = eb.fold(x, None, threshold=float(thr))
    assert np.array_equal(got, np.where(x < thr, np.float32(0), x))
    assert got[0, 3, 5] == thr and got[0, 4, 5] == 0 and got[1, 0, 69] == thr


def test_emu_fold_pre_l1_divides_by_the_sum_of_magnitudes():
    """A signed real input (tonnetz accepts any real chroma): p = sum |v|, not sum v."""
    rng = np.random.default_rng(12)
    x = rng.standard_normal((2, 12, 70)).astype(np.float32)
    w = M._phi64(12).astype(np.float32)
    got = eb.fold(x, w, pre_l1=True, pad_in=1)
    want, bound, keep = R.fold(x, 0, w, CONSTS, pre_l1=True)
    ratio = R.check(got, want, bound, keep, "signed")
    print(f"fold signed input, pre_l1: worst error / bound {ratio:.4f}")


REAL_BANKS = (
    ("chroma_filterbank", lambda: ap.chroma_filterbank(sr=22050, n_fft=2048), lambda: R.chroma_filterbank(22050, 2048), 2, dict(norm=INF)),
    ("cq_to_chroma-36", lambda: ap.cq_to_chroma(252, bins_per_octave=36), lambda: R.cq_to_chroma(252, 36), 1, dict(norm=INF, threshold=0.0)),
    ("cq_to_chroma-12", lambda: ap.cq_to_chroma(84, bins_per_octave=12, fmin=55.0), lambda: R.cq_to_chroma(84, 12, fmin=55.0), 1, dict(norm=None, threshold=0.0)),
    ("phi", lambda: M._phi64(12).astype(np.float32), lambda: R.phi(12), 0, dict(pre_l1=True)),
)


@pytest.mark.parametrize("case", REAL_BANKS, ids=[c[0] for c in REAL_BANKS])
def test_emu_fold_real_banks(case):
    """The package's own matrices: equal to the float64 definition rounded once, and the fold through them within the
    bound of the definition fed the same float32 matrix."""
    name, mine, ref, kind, kw = case
    w = np.asarray(mine(), np.float32)
    w64 = ref()
    assert w.shape == w64.shape and np.all(np.abs(w - w64) <= R.U * np.abs(w64) + 1e-12 * np.abs(w64).max())
    x = R.spectrum(2, w.shape[1], 70, kind, seed=9)
    got = eb.fold(x, w, in_kind=kind, pad_in=1, **kw)
    want, bound, keep = R.fold(x, kind, w, CONSTS, **kw)
    ratio = R.check(got, want, bound, keep, name)
    print(f"fold {name}: worst error / bound {ratio:.4f}")


# (n, T, n_taps, norm, B, pad_in, pad_out)
CENS_CASES = (
    (1, 1, 0, None, 1, 0, 0), (12, 2, 1, 1, 2, 1, 0), (36, 20, 3, 2, 1, 0, 2), (12, 21, 43, INF, 2, 0, 0), (12, 41, 43, 2, 1, 3, 1),
    (12, 64, SMOOTH, 2, 2, 0, 0), (36, 65, 43, 1, 1, 1, 1), (12, TILE - 1, 3, None, 2, 0, 0), (1, TILE, 43, 2, 1, 0, 0),
    (12, TILE + 1, SMOOTH, INF, 2, 2, 0), (12, 2 * TILE + 3, 43, 2, 2, 0, 1), (36, 2 * TILE + 3, SMOOTH, None, 1, 0, 0),
    (12, 2 * TILE + 3, 0, 2, 2, 1, 1), (12, 1, 43, 2, 1, 0, 0), (1, 65, 1, INF, 2, 0, 0),
)
CENS_IDS = ["n%d-T%d-taps%d-norm%s-B%d" % c[:5] for c in CENS_CASES]


def cens_taps(n_taps, seed):
    if n_taps == 0:
        return None
    return R.hann_taps(n_taps - 2) if n_taps == 43 else R.random_taps(n_taps, seed)


@pytest.mark.parametrize("case", CENS_CASES, ids=CENS_IDS)
def test_emu_cens_sweep(case):
    n, T, n_taps, norm, B, pad_in, pad_out = case
    i = CENS_CASES.index(case)
    x = R.chroma_input(B, n, T, seed=i)
    taps = cens_taps(n_taps, i)
    got = eb.cens(x, taps, norm=norm, pad_in=pad_in, pad_out=pad_out)
    want, bound, keep = R.cens(x, taps, norm)
    ratio = R.check(got, want, bound, keep, case)
    again = eb.cens(x, taps, norm=norm, grid=1)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32)), "a grid override changed a bit"
    print(f"cens {CENS_IDS[i]}: worst error / bound {ratio:.4f}, left out {100 * (1 - keep.mean()):.3f} %")


@pytest.mark.parametrize("n_taps", [2, 4])
def test_emu_cens_even_number_of_taps_and_signed_input(n_taps):
    """An even window is centred at (n_taps - 1) // 2, and the L1 norm takes magnitudes: a signed input whose frames
    stay clear of the quantiser's steps."""
    x = np.array(R.chroma_input(2, 12, TILE + 9, seed=50 + n_taps))
    x[:, 1::3, :] *= np.float32(-1.0)
    taps = R.random_taps(n_taps, 7)
    got = eb.cens(x, taps, norm=2, pad_out=1)
    want, bound, keep = R.cens(x, taps, 2)
    ratio = R.check(got, want, bound, keep, n_taps)
    assert (want < 0).sum() == 0 and np.abs(want).max() > 0
    print(f"cens {n_taps} taps, signed input: worst error / bound {ratio:.4f}")


def test_emu_cens_quantiser_exact():
    """Frames that are permutations of [8, 4, 2, 1, 1, 0, ...] have L1-normalised values 1/2, 1/4, 1/8, 1/16, 1/16, 0:
    all exact and none at a step, so the output is exactly [1, .75, .5, .25, .25, 0, ...] in the same places."""
    rng = np.random.default_rng(3)
    base = np.zeros(12, np.float32)
    base[:5] = (8, 4, 2, 1, 1)
    lev = np.zeros(12, np.float32)
    lev[:5] = (1.0, 0.75, 0.5, 0.25, 0.25)
    T = 2 * TILE + 5
    x = np.empty((2, 12, T), np.float32)
    want = np.empty((2, 12, T), np.float32)
    for b in range(2):
        for t in range(T):
            p = rng.permutation(12)
            x[b, :, t] = base[p] * np.float32(2.0 ** rng.integers(-20, 20))
            want[b, :, t] = lev[p]
    got = eb.cens(x, None, norm=None, pad_in=1, pad_out=1)
    assert np.array_equal(got, want)


def test_emu_cens_one_frame_against_all_the_others():
    """Every frame holds column A except a few that hold column B: with 43 non-zero taps the output differs from the
    all-A output on exactly the 43 frames around each odd one, clipped at the clip's ends (h = 21 on both sides), and the
    other clip does not change at all: the smoothing crosses the tile seams and stops at the ends of a clip."""
    T = 3 * TILE + 7
    A = np.array([8, 4, 2, 1, 1, 0, 0, 0, 0, 0, 0, 0], np.float32)
    Bc = A[::-1].copy()
    taps = R.random_taps(43, 1)
    taps = np.where(np.abs(taps) < 1e-3, np.float32(0.5), taps)
    plain = np.repeat(np.repeat(A[None, :, None], T, axis=2), 2, axis=0)
    base = eb.cens(plain, taps, norm=None)
    for odd in ((TILE - 1,), (TILE,), (0,), (T - 1,), (2 * TILE + 10,)):
        x = plain.copy()
        for t in odd:
            x[0, :, t] = Bc
        got = eb.cens(x, taps, norm=None, pad_in=2)
        want, bound, keep = R.cens(x, taps, None)
        R.check(got, want, bound, keep, odd)
        changed = (got != base).any(axis=1)
        expect = np.zeros((2, T), bool)
        for t in odd:
            expect[0, max(0, t - 21):min(T, t + 22)] = True
        assert np.array_equal(changed, expect), (odd, np.flatnonzero(changed[0]), np.flatnonzero(changed[1]))


def test_emu_prepare_rejections():
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data
    ok = dict(x_ptr=p, in_kind=0, B=1, K=4, T=8, in_rs=8, w_ptr=p, n_out=2, norm=0, out_ptr=p, out_rs=8)
    assert eb.fold_raw(**ok) == 0
    for change, word in ((dict(x_ptr=None), "NULL"), (dict(out_ptr=None), "NULL"), (dict(n_out=CAP + 1), "n_out"), (dict(n_out=0), "n_out"),
                         (dict(in_rs=7), "in_row_stride"), (dict(out_rs=7), "out_row_stride"), (dict(in_kind=3), "in_kind"),
                         (dict(in_kind=-1), "in_kind"), (dict(norm=4), "norm"), (dict(norm=-1), "norm"),
                         (dict(w_ptr=None), "identity"), (dict(B=0), "non-empty"), (dict(K=0), "non-empty"), (dict(T=0), "non-empty")):
        rc = eb.fold_raw(**dict(ok, **change))
        assert rc == -1 and word in eb.last_error(), (change, rc, eb.last_error())
    assert eb.fold_raw(**dict(ok, w_ptr=None, K=2, in_rs=8)) == 0
    ok = dict(x_ptr=p, B=1, n=12, T=8, in_rs=8, taps_ptr=p, n_taps=3, norm=2, out_ptr=p + 4 * 2048, out_rs=8)
    assert eb.cens_raw(**ok) == 0
    for change, word in ((dict(x_ptr=None), "NULL"), (dict(out_ptr=None), "NULL"), (dict(taps_ptr=None), "NULL taps"), (dict(n=0), "n must"),
                         (dict(n=CAP + 1), "n must"), (dict(n_taps=SMOOTH + 1), "n_taps"), (dict(n_taps=-1), "n_taps"), (dict(norm=4), "norm"),
                         (dict(in_rs=7), "in_row_stride"), (dict(out_rs=7), "out_row_stride"), (dict(B=0), "non-empty"), (dict(T=0), "non-empty")):
        rc = eb.cens_raw(**dict(ok, **change))
        assert rc == -1 and word in eb.last_error(), (change, rc, eb.last_error())
    assert eb.cens_raw(**dict(ok, taps_ptr=None, n_taps=0)) == 0
    assert ctypes.sizeof(ctypes.c_void_p) == 8
