"""GPU: the DTW kernels on the device against the definition in tests/dtw_ref.py and against the emulator.

The sweeps of test_emu_dtw.py go through the C entries on the device: D, the step codes and the paths must equal the
model and the emulator in every bit; the cost kernel lies within its bound and, for sqeuclidean and cityblock (no sqrt,
no division), gives the emulator's bits, while for euclidean and cosine the match is printed, not assumed.  Then the
public functions: 2-D, batched and host input, a non-default stream, padded rows read in place, and the properties a
user of DTW relies on.  Seen on an MI355X: every cost case gave the emulator's bits, euclidean and cosine included;
worst error / bound 0.82 (sqeuclidean, d = 2); the CENS alignment of 130 x 143 frames stays 4.9 frames from j = 1.1 i
on average.  The weighted step tables are what pins the compiler's contraction of mul * c + add, which the emulator
cannot see."""

import os
import sys

import numpy as np
import pytest
import torch

import dtw_ref as R
import test_emu_dtw as E

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _extension as _x

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_dtw_bind as eb  # noqa: E402

pytestmark = pytest.mark.gpu
TW, TH = E.TW, E.TH


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def padded(x, pad, fill=float("nan")):
    """x (B, R, T) on the device with `pad` columns of `fill` behind every row: (tensor that owns the memory, row stride)."""
    B, R_, T = x.shape
    buf = torch.full((B, R_, T + pad), fill, dtype=torch.float32, device="cuda")
    buf[:, :, :T] = dev(x)
    return buf, T + pad


def device_cost(X, Y, metric, pad_x=0, pad_y=0, pad_out=0):
    B, d, N = X.shape
    M = Y.shape[2]
    xd, x_rs = padded(X, pad_x)
    yd, y_rs = padded(Y, pad_y)
    out = torch.full((B, N, M + pad_out), float("nan"), dtype=torch.float32, device="cuda")
    _x.check(_x.dlib(xd.device).ap_dtw_cost_f32(_x.ptr(xd), _x.ptr(yd), B, d, N, M, x_rs, y_rs, eb.METRICS[metric], _x.ptr(out),
                                                M + pad_out, _x.stream_ptr(xd.device)))
    got = out.cpu().numpy()
    assert np.isnan(got[..., M:]).all(), "a pad column was written"
    return np.ascontiguousarray(got[..., :M])


def device_accumulate(C, steps=None, add=None, mul=None, *, subseq=False, band_r=None, pad_in=0, pad_out=0):
    """(D, codes, the device tensors with their padded rows) through ap_dtw_accumulate_f32; -inf behind the rows of C."""
    B, N, M = C.shape
    ab, add, mul, n = eb._table(eb.DEFAULT_STEPS if steps is None else steps, add, mul)
    cd, c_rs = padded(C, pad_in, float("-inf"))
    rs = M + pad_out
    Dd = torch.full((B, N, rs), float("nan"), dtype=torch.float32, device="cuda")
    Sd = torch.full((B, N, rs), eb.BYTE_POISON, dtype=torch.uint8, device="cuda")
    _x.check(_x.dlib(cd.device).ap_dtw_accumulate_f32(_x.ptr(cd), B, N, M, c_rs, n, ab.ctypes.data, add.ctypes.data, mul.ctypes.data,
                                                      int(bool(subseq)), int(band_r is not None), int(band_r or 0), _x.ptr(Dd), rs,
                                                      _x.ptr(Sd), rs, _x.stream_ptr(cd.device)))
    D, S = Dd.cpu().numpy(), Sd.cpu().numpy()
    assert np.isnan(D[..., M:]).all() and (S[..., M:] == eb.BYTE_POISON).all(), "a pad column was written"
    return np.ascontiguousarray(D[..., :M]), np.ascontiguousarray(S[..., :M]), Dd, Sd


def device_backtrack(Sd, Dd, N, M, steps=None, *, subseq=False, start=None):
    """The list of paths (None: no path) through ap_dtw_backtrack_i32 on device tensors with padded rows."""
    B, rs = Sd.shape[0], Sd.shape[2]
    ab = eb._table(eb.DEFAULT_STEPS if steps is None else steps, None, None)[0]
    L = N + M - 1
    path = torch.full((B, L, 2), -7, dtype=torch.int32, device="cuda")
    lens = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    st = None if start is None else dev(np.asarray(start, np.int32))
    _x.check(_x.dlib(Sd.device).ap_dtw_backtrack_i32(None if Dd is None else _x.ptr(Dd), _x.ptr(Sd), None if st is None else _x.ptr(st),
                                                     B, N, M, rs, rs, ab.shape[0], ab.ctypes.data, int(bool(subseq)), _x.ptr(path),
                                                     _x.ptr(lens), _x.stream_ptr(Sd.device)))
    path, lens = path.cpu().numpy(), lens.cpu().numpy()
    out = []
    for b in range(B):
        n = int(lens[b])
        assert n == -1 or 1 <= n <= L
        assert n < 0 or (path[b, n:] == -7).all(), "the path was written beyond its length"
        out.append(None if n < 0 else path[b, :n].copy())
    return out


def same_paths(a, b):
    return len(a) == len(b) and all((p is None and q is None) or (p is not None and q is not None and np.array_equal(p, q))
                                    for p, q in zip(a, b))


@pytest.mark.parametrize("case", E.ACC_CASES, ids=E.ACC_IDS)
def test_gpu_accumulate_and_backtrack_sweep(case):
    N, M = case[0], case[1]
    C, kw, lay = E.acc_case(case)
    D, S, Dd, Sd = device_accumulate(C, **kw, **lay)
    Dr, Sr = E.reference(C, kw)
    E.assert_same(D, S, Dr, Sr, case)
    De, Se = eb.accumulate(C, **kw, **lay)
    E.assert_same(D, S, De, Se, f"{case} against the emulator")
    paths = device_backtrack(Sd, Dd, N, M, kw["steps"], subseq=kw["subseq"])
    E.assert_paths(paths, S, D, kw["steps"], kw["subseq"], case)
    assert same_paths(paths, eb.backtrack(S, kw["steps"], D=D, subseq=kw["subseq"]))


@pytest.mark.parametrize("kind", ["ties", "signed"])
def test_gpu_ties_negative_costs_and_non_finite_costs(kind):
    for tab in sorted(E.TABLES):
        steps, add, mul = E.TABLES[tab]
        C = R.cost_matrix(2, TW + 3, TH + 7, 7, kind)
        if kind == "signed":
            C[0, 3, 10:] = np.inf
            C[1, 10:20, TW - 1:TW + 2] = np.nan
            C[1, 30, 40] = -np.inf
        kw = dict(steps=steps, add=add, mul=mul, subseq=kind == "ties", band_r=None)
        D, S, Dd, Sd = device_accumulate(C, **kw, pad_in=1)
        E.assert_same(D, S, *E.reference(C, kw), (tab, kind))
        assert not np.isnan(D).any() and (S[np.isnan(C)] == R.NONE).all()
        paths = device_backtrack(Sd, Dd, TW + 3, TH + 7, steps, subseq=kw["subseq"])
        E.assert_paths(paths, S, D, steps, kw["subseq"], (tab, kind))


def test_gpu_backtrack_windows_starts_and_dead_ends():
    WIN = E.WIN
    N, M = 2 * WIN + 5, 2 * WIN + 9
    S = np.full((1, N, M), 1, np.uint8)
    S[0, 1:, WIN + 3] = 2
    S[0, 0, 0] = R.START
    path, = device_backtrack(dev(S), None, N, M)
    np.testing.assert_array_equal(path, R.backtrack(S[0]))
    assert len(path) == N + M - 1
    S = np.zeros((2, 3 * WIN + 1, 3 * WIN + 1), np.uint8)
    S[:, 0, 0] = R.START
    S[1, WIN + 7, WIN + 7] = R.NONE
    paths = device_backtrack(dev(S), None, 3 * WIN + 1, 3 * WIN + 1)
    np.testing.assert_array_equal(paths[0], np.repeat(np.arange(3 * WIN, -1, -1), 2).reshape(-1, 2))
    assert paths[1] is None
    S = np.zeros((1, 3, 5), np.uint8)
    assert device_backtrack(dev(S), None, 3, 5) == [None]
    # the subseq start: the first minimum of a tied last row, -inf behind the rows of D
    C = R.cost_matrix(2, 5, 3 * WIN + 2, 19)
    D, S, Dd, Sd = device_accumulate(C, subseq=True, pad_out=3)
    Dd[:, :, 3 * WIN + 2:] = float("-inf")
    Dd[:, -1, :3 * WIN + 2] = 5.0
    for c in (70, 2 * WIN + 1, 7, 64):
        Dd[0, -1, c] = 1.0
    Dd[1, -1, WIN + 1] = float("-inf")
    Dd[1, -1, WIN + 65] = float("-inf")
    paths = device_backtrack(Sd, Dd, 5, 3 * WIN + 2, subseq=True)
    assert paths[0][0].tolist() == [4, 7] and paths[1][0].tolist() == [4, WIN + 1]
    Dh = Dd.cpu().numpy()[..., :3 * WIN + 2]
    assert same_paths(paths, eb.backtrack(S, D=Dh, subseq=True))
    given = device_backtrack(Sd, None, 5, 3 * WIN + 2, start=[9, 3 * WIN + 1])
    np.testing.assert_array_equal(given[0], R.backtrack(S[0], start=9))
    assert given[1][0].tolist() == [4, 3 * WIN + 1]


@pytest.mark.parametrize("case", E.COST_CASES, ids=E.COST_IDS)
def test_gpu_cost_sweep(case):
    X, Y, lay = E.cost_case(case)
    metric = case[3]
    got = device_cost(X, Y, metric, **lay)
    want, bound = R.cost(X, Y, metric)
    ratio = R.check_cost(got, want, bound, case)
    same = E.same_bits(got, eb.cost(X, Y, metric, **lay))
    if metric in ("sqeuclidean", "cityblock"):
        assert same, "no sqrt and no division on this path: the device and the emulator must agree in every bit"
    print(f"cost {E.COST_IDS[E.COST_CASES.index(case)]}: worst error / bound {ratio:.4f}; the emulator's bits: {same}")


def test_gpu_cost_special_values():
    X = R.features(2, 13, E.CT + 3, 31)
    for metric in ("euclidean", "sqeuclidean", "cityblock"):
        got = device_cost(X, X, metric)
        assert (np.diagonal(got, axis1=1, axis2=2) == 0.0).all(), f"{metric}: x == y gives exactly 0"
    Y = X.copy()
    Y[:, :, 5] = 0.0
    got = device_cost(X, Y, "cosine")
    assert (got[:, :, 5] == 1.0).all()
    R.check_cost(got, *R.cost(X, Y, "cosine"), "zero column")


# ---------------------------------------------------------------------------------------------------------------------
# the public functions
# ---------------------------------------------------------------------------------------------------------------------
def seq(d, T, seed):
    return R.features(1, d, T, seed)[0]


def test_gpu_dtw_shapes_inputs_and_the_tuple():
    X, Y = R.features(3, 12, TW + 9, 41), R.features(3, 12, TH + 30, 42)
    N, M = X.shape[2], Y.shape[2]
    D, wp, steps = ap.dtw(dev(X), dev(Y), return_steps=True)
    assert D.shape == (3, N, M) and D.dtype == torch.float32 and D.is_cuda
    assert steps.shape == (3, N, M) and steps.dtype == torch.uint8 and steps.is_cuda
    assert isinstance(wp, list) and len(wp) == 3 and all(p.dtype == torch.int32 and p.is_cuda and p.shape[1] == 2 for p in wp)
    C = device_cost(X, Y, "euclidean")
    Dr, Sr = E.reference(C, dict(steps=None, add=None, mul=None, subseq=False, band_r=None))
    E.assert_same(D.cpu().numpy(), steps.cpu().numpy(), Dr, Sr, "dtw(X, Y)")
    for b in range(3):
        np.testing.assert_array_equal(wp[b].cpu().numpy(), R.backtrack(Sr[b]))
        D1, wp1, s1 = ap.dtw(dev(X[b]), dev(Y[b]), return_steps=True)            # 2-D: row b of the batch
        assert D1.shape == (N, M) and torch.equal(D1, D[b]) and torch.equal(s1, steps[b]) and torch.equal(wp1, wp[b])
    Dh, wph = ap.dtw(X, Y)                                                       # host arrays
    assert Dh.is_cuda and torch.equal(Dh, D) and all(torch.equal(a, b) for a, b in zip(wph, wp))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Ds, wps = ap.dtw(dev(X), dev(Y))
    side.synchronize()
    assert torch.equal(Ds, D) and all(torch.equal(a, b) for a, b in zip(wps, wp))
    # the tuple: D [, wp] [, steps], D alone when nothing else is asked for
    only = ap.dtw(dev(X), dev(Y), backtrack=False)
    assert isinstance(only, torch.Tensor) and torch.equal(only, D)
    two = ap.dtw(dev(X), dev(Y), backtrack=False, return_steps=True)
    assert isinstance(two, tuple) and len(two) == 2 and torch.equal(two[0], D) and torch.equal(two[1], steps)
    # dtw_backtracking reproduces wp, batched, 2-D and from the host
    again = ap.dtw_backtracking(steps)
    assert all(torch.equal(a, b) for a, b in zip(again, wp))
    assert torch.equal(ap.dtw_backtracking(steps[1]), wp[1]) and torch.equal(ap.dtw_backtracking(steps[1].cpu().numpy()), wp[1])
    assert torch.equal(ap.dtw_backtracking(steps[1], start=M - 1), wp[1])
    assert ap.dtw_backtracking(steps, start=[3, 4, 5])[2][0].tolist() == [N - 1, 5]


def test_gpu_dtw_cost_matrix_in_place_and_every_metric():
    X, Y = R.features(2, 7, TW + 1, 43), R.features(2, 7, TW + 30, 44)        # (1, 2) steps reach the end: M - 1 <= 2 (N - 1)
    N, M = X.shape[2], Y.shape[2]
    for metric in R.METRICS:
        D, wp = ap.dtw(dev(X), dev(Y), metric=metric)
        C = dev(device_cost(X, Y, metric))
        D2, wp2 = ap.dtw(C=C)
        assert torch.equal(D, D2) and all(torch.equal(a, b) for a, b in zip(wp, wp2)), metric
        buf, rs = padded(C.cpu().numpy(), 5, float("-inf"))                     # padded rows are read in place
        D3 = ap.dtw(C=buf[:, :, :M], backtrack=False)
        assert torch.equal(D, D3), metric
        D4 = ap.dtw(C=C.cpu().numpy().astype(np.float64)[0], backtrack=False)   # a host float64 matrix, 2-D
        assert torch.equal(D4, D[0])
    kw = dict(step_sizes_sigma=[[1, 1], [1, 2], [2, 1]], weights_add=[0.0, 0.5, 0.5], weights_mul=[1.0, 2.0, 2.0],
              global_constraints=True, band_rad=0.5)
    Cn = device_cost(X, Y, "euclidean")
    D, wp, steps = ap.dtw(C=dev(Cn), return_steps=True, **kw)
    Dr, Sr = E.reference(Cn, dict(steps=((1, 1), (1, 2), (2, 1)), add=(0.0, 0.5, 0.5), mul=(1.0, 2.0, 2.0), subseq=False,
                                  band_r=R.band_radius(0.5, N, M)))
    E.assert_same(D.cpu().numpy(), steps.cpu().numpy(), Dr, Sr, "weights and band")
    with pytest.raises(ValueError, match="pair 0"):
        ap.dtw(C=dev(R.cost_matrix(2, 5, 40, 1)), step_sizes_sigma=[[1, 1], [1, 2], [2, 1]])
    with pytest.raises(ValueError, match="pair 1"):
        bad = np.zeros((2, 4, 4), np.uint8)
        bad[0, 0, 0] = R.START
        bad[1, 2, 2] = R.NONE
        ap.dtw_backtracking(dev(bad))


def test_gpu_dtw_properties():
    X = seq(12, 2 * TW + 7, 45)
    N = X.shape[1]
    D, wp = ap.dtw(dev(X), dev(X))
    assert D[-1, -1].item() == 0.0
    np.testing.assert_array_equal(wp.cpu().numpy(), np.repeat(np.arange(N - 1, -1, -1), 2).reshape(-1, 2))
    # symmetry: D of (X, Y) is the transpose of D of (Y, X) in every bit.  (x - y)^2 == (y - x)^2, and swapping the steps
    # (0, 1) and (1, 0) changes the order of the candidates, which decides the code of a tie but not the minimum's value
    Y = seq(12, TH + 20, 46)
    Dxy = ap.dtw(dev(X), dev(Y), backtrack=False)
    Dyx = ap.dtw(dev(Y), dev(X), backtrack=False)
    assert torch.equal(Dxy, Dyx.T), "D(X, Y) == D(Y, X)^T at the default table"
    # every column repeated twice: the path runs along j = 2 i, 2 i + 1
    Y2 = np.repeat(X, 2, axis=1)
    D, wp = ap.dtw(dev(X), dev(Y2))
    assert D[-1, -1].item() == 0.0
    p = wp.cpu().numpy()
    assert (p[:, 1] // 2 == p[:, 0]).all() and len(p) == 2 * N
    # subseq: X embedded in a longer random Y at offset o is found at the columns o .. o + N - 1 with cost 0
    o = TW + 11
    Yl = seq(12, 3 * TW + N, 47)
    Yl[:, o:o + N] = X
    D, wp = ap.dtw(dev(X), dev(Yl), subseq=True)
    p = wp.cpu().numpy()
    np.testing.assert_array_equal(p, np.stack([np.arange(N - 1, -1, -1), np.arange(o + N - 1, o - 1, -1)], axis=1))
    assert D[-1, o + N - 1].item() == 0.0 and D[-1].min().item() == 0.0


def test_gpu_dtw_aligns_cens_of_a_clip_and_its_slower_copy():
    sr = 22050
    rng = np.random.default_rng(48)
    notes = 110.0 * 2.0 ** (rng.integers(0, 24, 12) / 12.0)
    t = np.arange(int(0.25 * sr)) / sr
    y = np.concatenate([np.sin(2 * np.pi * f * t) * np.hanning(len(t)) for f in notes]).astype(np.float32)
    slow = ap.resample(dev(y), sr, 24255)                                       # the same clip, 10 % longer
    kw = dict(sr=sr, fmin=110.0, n_octaves=3, hop_length=512)
    a, b = ap.chroma_cens(y=dev(y), **kw), ap.chroma_cens(y=slow, **kw)
    N, M = a.shape[1], b.shape[1]
    assert abs(M - 1.1 * N) <= 2
    D, wp = ap.dtw(a, b, global_constraints=True, band_rad=0.25)
    p = wp.cpu().numpy()
    assert p[0].tolist() == [N - 1, M - 1] and p[-1].tolist() == [0, 0]
    assert (np.diff(p[:, 0]) <= 0).all() and (np.diff(p[:, 1]) <= 0).all() and (np.diff(p.sum(axis=1)) < 0).all()
    assert R.in_band(p[:, 0], p[:, 1], N, M, R.band_radius(0.25, N, M)).all()
    print(f"cens alignment: {N} x {M} frames, mean |j - 1.1 i| = {np.abs(p[:, 1] - 1.1 * p[:, 0]).mean():.2f} frames")
