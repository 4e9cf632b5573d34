"""GPU: the recurrence / cross-similarity kernels on the device against the definition in tests/segment_ref.py and
against the emulator.

The sweeps of test_emu_segment.py go through the C entries on the device (the `Device` engine below has the emulator
binding's interface): the records, connectivity, distance, med_k_scalar and the lag arrays must equal the model, whose D
is the emulated cost kernel's, in every bit; affinity and the mean bandwidths lie within the derived bounds.
cross_similarity(mode="distance", k=n_ref) must equal the device's own ap_dtw_cost_f32 in every bit: that pins the
compiler's contraction, which the emulator cannot see.  Then the public functions: 2-D, batched,
host, float64 and padded-view input, a non-default stream, and the properties a user relies on.  Seen on an MI355X:
every case gave the model's and the emulator's bits, euclidean and cosine included; worst error / bound 0.96 (a mean
bandwidth of two values: the one rounding to float32); the CENS clip of 259 frames repeated at frame 129 puts 105 mutual
nearest neighbours on lag 129 and a median of 0 on the other lags."""

import os
import sys

import numpy as np
import pytest
import torch

import dtw_ref
import segment_ref as R
import test_emu_segment as E

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _extension as _x

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_segment_bind as sb  # noqa: E402

pytestmark = pytest.mark.gpu
TI = E.TI


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def padded(x, pad, fill=float("nan")):
    """x (B, R, T) on the device with `pad` columns of `fill` behind every row: (tensor that owns the memory, row stride)."""
    B, R_, T = x.shape
    buf = torch.full((B, R_, T + pad), fill, dtype=torch.float32, device="cuda")
    buf[:, :, :T] = dev(x)
    return buf, T + pad


class Device:
    """The C entries on the device, with the interface of emu_segment_bind."""

    class Pair:
        def __init__(self, ref, data, pad_ref=0, pad_data=0):
            self.data = np.asarray(data, np.float32)
            self.B, self.d, self.n = self.data.shape
            self.yd, self.y_rs = padded(self.data, pad_data)
            if ref is None:
                self.n_ref, self.xd, self.x_rs = self.n, self.yd, self.y_rs
            else:
                self.n_ref = ref.shape[2]
                self.xd, self.x_rs = padded(np.asarray(ref, np.float32), pad_ref)

    @staticmethod
    def _lib():
        return _x.dlib(torch.device("cuda", torch.cuda.current_device()))

    @staticmethod
    def _stream():
        return _x.stream_ptr(torch.device("cuda", torch.cuda.current_device()))

    @classmethod
    def threshold(cls, p, metric, k, width=0):
        rec = torch.full((p.B, p.n, 2), -286331154, dtype=torch.int32, device="cuda")       # 0xEEEEEEEE
        _x.check(cls._lib().ap_segment_threshold_f32(_x.ptr(p.xd), _x.ptr(p.yd), p.B, p.d, p.n_ref, p.n, p.x_rs, p.y_rs, sb.METRICS[metric],
                                                     int(k), int(width), _x.ptr(rec), cls._stream()))
        rec = rec.cpu().numpy()
        return np.ascontiguousarray(rec[..., 0]).view(np.float32), np.ascontiguousarray(rec[..., 1])

    @staticmethod
    def _records(tau, t):
        return dev(np.stack([np.ascontiguousarray(tau, np.float32).view(np.int32), np.ascontiguousarray(t, np.int32)], axis=-1))

    @classmethod
    def bandwidth(cls, tau, t, kind):
        B, n = tau.shape
        rec = cls._records(tau, t)
        bw = torch.full((B,), -7.0, dtype=torch.float32, device="cuda")
        _x.check(cls._lib().ap_segment_bandwidth_f32(_x.ptr(rec), B, n, sb.KINDS[kind], _x.ptr(bw), cls._stream()))
        return bw.cpu().numpy()

    @classmethod
    def write(cls, p, metric, mode, tau, t, *, width=0, full=False, sym=False, self_diag=False, bw=None, bandwidth_value=1.0, pad_out=0):
        rec = cls._records(tau, t)
        rs = p.n + pad_out
        is_byte = mode == "connectivity"
        out = torch.full((p.B, p.n_ref, rs), sb.BYTE_POISON if is_byte else float("nan"), dtype=torch.uint8 if is_byte else torch.float32,
                         device="cuda")
        bwd = None if bw is None else dev(np.asarray(bw, np.float32))
        _x.check(cls._lib().ap_segment_write_f32(_x.ptr(p.xd), _x.ptr(p.yd), p.B, p.d, p.n_ref, p.n, p.x_rs, p.y_rs, sb.METRICS[metric],
                                                 sb.MODES[mode], int(width), int(full), int(sym), int(self_diag), _x.ptr(rec),
                                                 None if bwd is None else _x.ptr(bwd), float(bandwidth_value), _x.ptr(out), rs, cls._stream()))
        got = out.cpu().numpy()
        if is_byte:
            assert (got[..., p.n:] == sb.BYTE_POISON).all(), "a pad column was written"
            got = got[..., :p.n]
            assert ((got == 0) | (got == 1)).all(), "a cell is neither 0 nor 1, or was not written"
            return got.astype(bool)
        assert np.isnan(got[..., p.n:]).all(), "a pad column was written"
        got = np.ascontiguousarray(got[..., :p.n])
        assert not np.isnan(got).any(), "a cell is NaN or was not written"
        return got

    @classmethod
    def lag(cls, a, to_lag, pad=True, *, pad_in=0, pad_out=0):
        a = np.asarray(a)
        is_bool = a.dtype == np.bool_
        src = a.view(np.uint8) if is_bool else a.view(np.int32)
        B, rows_in, n = src.shape
        tp = (2 * n if pad else n) if to_lag else rows_in
        rows_out = tp if to_lag else n
        poison = sb.BYTE_POISON if is_bool else -286331154
        ind = torch.full((B, rows_in, n + pad_in), poison, dtype=torch.uint8 if is_bool else torch.int32, device="cuda")
        ind[:, :, :n] = dev(src)
        out = torch.full((B, rows_out, n + pad_out), poison, dtype=ind.dtype, device="cuda")
        _x.check(cls._lib().ap_segment_lag(_x.ptr(ind), B, n, tp, src.itemsize, int(bool(to_lag)), n + pad_in, _x.ptr(out), n + pad_out,
                                           cls._stream()))
        got = out.cpu().numpy()
        assert (got[..., n:] == poison).all(), "a pad column was written"
        got = np.ascontiguousarray(got[..., :n])
        assert (got != poison).all(), "a cell was not written"
        return got.view(np.bool_) if is_bool else got.view(a.dtype)


@pytest.mark.parametrize("case", E.CROSS_CASES, ids=E.CROSS_IDS)
def test_gpu_cross_similarity_sweep(case):
    X, Y, metric, k, kw = E.cross_inputs(case)
    print(f"worst error / bound {E.check_case(Device, X, Y, metric, k, what=str(case), **kw):.4f}")
    pair_e, pair_d = sb.Pair(X, Y), Device.Pair(X, Y)
    for a, b in zip(sb.threshold(pair_e, metric, k), Device.threshold(pair_d, metric, k)):
        assert E.same_bits(a, b), "the records differ from the emulator's"


@pytest.mark.parametrize("case", E.REC_CASES, ids=E.REC_IDS)
def test_gpu_recurrence_sweep(case):
    Y, metric, k, kw = E.rec_inputs(case)
    print(f"worst error / bound {E.check_case(Device, None, Y, metric, k, what=str(case), **kw):.4f}")
    pair_e, pair_d = sb.Pair(None, Y), Device.Pair(None, Y)
    te, td = sb.threshold(pair_e, metric, k, kw["width"]), Device.threshold(pair_d, metric, k, kw["width"])
    assert E.same_bits(te[0], td[0]) and E.same_bits(te[1], td[1]), "the records differ from the emulator's"
    args = dict(width=kw["width"], sym=kw["sym"], self_diag=kw["self_diag"], full=kw["full"])
    assert E.same_bits(sb.write(pair_e, metric, "distance", *te, **args), Device.write(pair_d, metric, "distance", *td, **args))


@pytest.mark.parametrize("kind, metric", E.TIE_CASES)
def test_gpu_ties_go_to_the_smaller_index(kind, metric):
    E.check_ties(Device, kind, metric)


@pytest.mark.parametrize("metric", E.METRICS)
@pytest.mark.parametrize("d, n_ref, n", [(12, 2 * TI + 3, TI + 5), (128, TI + 1, 2 * TI + 3), (13, TI - 1, TI - 1), (1, 3, TI)])
def test_gpu_distances_are_the_cost_kernels_in_every_bit(metric, d, n_ref, n):
    """cross_similarity(mode="distance", k=n_ref) against the device's own ap_dtw_cost_f32: the one comparison that sees
    whether the compiler contracted an operation of the restated arithmetic differently."""
    X, Y = dtw_ref.features(2, d, n_ref, 7 * d), dtw_ref.features(2, d, n, 7 * d + 1)
    xd, yd = dev(X), dev(Y)
    C = torch.empty((2, n_ref, n), dtype=torch.float32, device="cuda")
    _x.check(_x.dlib(xd.device).ap_dtw_cost_f32(_x.ptr(xd), _x.ptr(yd), 2, d, n_ref, n, n_ref, n, sb.METRICS[metric], _x.ptr(C), n,
                                                _x.stream_ptr(xd.device)))
    got = ap.cross_similarity(yd, xd, k=n_ref, metric=metric, mode="distance")
    assert got.dtype == torch.float32 and got.shape == (2, n_ref, n)
    assert E.same_bits(got.cpu().numpy(), C.cpu().numpy())
    # and the thresholds are distances of that matrix: the largest of every column
    tau, _ = Device.threshold(Device.Pair(X, Y), metric, n_ref)
    assert E.same_bits(tau, C.max(dim=1).values.cpu().numpy() + np.float32(0.0))


def model_matrix(X, Y, metric, k, **kw):
    D = E.cost(Y if X is None else X, Y, metric)
    return np.stack([R.matrix(D[b], k, **kw)[0] for b in range(Y.shape[0])])


def test_gpu_public_functions_take_every_kind_of_input():
    Y = dtw_ref.features(3, 12, TI + 9, 60)
    X = dtw_ref.features(3, 12, TI - 5, 61)
    n, n_ref = Y.shape[2], X.shape[2]
    k = R.default_k_recurrence(n, 1)
    want = model_matrix(None, Y, "euclidean", k, width=1)
    got = ap.recurrence_matrix(dev(Y))
    assert got.dtype == torch.bool and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(ap.recurrence_matrix(dev(Y[0])).cpu().numpy(), want[0])                    # 2-D
    assert np.array_equal(ap.recurrence_matrix(Y).cpu().numpy(), want)                               # host
    assert np.array_equal(ap.recurrence_matrix(torch.from_numpy(Y[1])).cpu().numpy(), want[1])
    assert np.array_equal(ap.recurrence_matrix(Y.astype(np.float64)).cpu().numpy(), want)            # float64: cast
    buf, rs = padded(Y, 7)                                                                            # padded rows, read in place
    view = buf[:, :, :n]
    assert not view.is_contiguous()
    assert np.array_equal(ap.recurrence_matrix(view).cpu().numpy(), want)
    assert np.isnan(buf[:, :, n:].cpu().numpy()).all()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        on_s = ap.recurrence_matrix(dev(Y), mode="distance", sym=True, width=3, k=5)
    s.synchronize()
    assert E.same_bits(on_s.cpu().numpy(), model_matrix(None, Y, "euclidean", 5, width=3, sym=True, mode="distance"))
    kc = R.default_k_cross(n_ref)
    got = ap.cross_similarity(dev(Y), X, metric="cityblock")                                          # device and host mixed
    assert got.shape == (3, n_ref, n) and np.array_equal(got.cpu().numpy(), model_matrix(X, Y, "cityblock", kc))
    got = ap.cross_similarity(Y[2], X[2], metric="cosine", mode="distance", full=True)
    assert got.shape == (n_ref, n) and E.same_bits(got.cpu().numpy(), model_matrix(X[2:], Y[2:], "cosine", kc, full=True, mode="distance")[0])


def test_gpu_affinity_bandwidths_and_the_error_for_an_unusable_estimate():
    Y = dtw_ref.features(2, 12, TI + 9, 62)
    n = Y.shape[2]
    k = R.default_k_recurrence(n, 1)
    D = E.cost(Y, Y, "euclidean")
    for bandwidth in (None, "med_k_scalar", "mean_k", "gmean_k", 0.8):
        got = ap.recurrence_matrix(Y, mode="affinity", bandwidth=bandwidth, self=True).cpu().numpy()
        for b in range(2):
            _, tau, t = R.neighbours(D[b], k, 1)
            bw = bandwidth if isinstance(bandwidth, float) else R.bandwidth(tau, t, bandwidth or "med_k_scalar")[0]
            (want, bound), _, _ = R.matrix(D[b], k, width=1, mode="affinity", self_diag=True, bw=bw)
            if bandwidth in ("mean_k", "gmean_k"):              # the estimate itself is within its bound: widen by its effect
                rel = R.bandwidth(tau, t, bandwidth)[1] / bw
                bound = bound + want * np.abs(np.log(np.maximum(want, R.TINY))) * rel * 2
            R.check_affinity(got[b], want, bound, f"{bandwidth} pair {b}")
            assert (np.diag(got[b]) == 1.0).all()
    const = np.full((3, 20), 0.5, np.float32)                   # every distance 0: the median is 0
    with pytest.raises(ValueError, match="estimated bandwidth"):
        ap.recurrence_matrix(const, mode="affinity")
    assert ap.recurrence_matrix(const, mode="affinity", bandwidth=1.0).shape == (20, 20)
    assert ap.recurrence_matrix(const).dtype == torch.bool      # connectivity asks for no bandwidth


def test_gpu_properties_of_the_matrices():
    Y = dtw_ref.features(2, 12, 2 * TI + 3, 63)
    n = Y.shape[2]
    for metric in E.METRICS:
        for width, k in ((1, None), (4, 7), (R.max_width(n), 3)):
            Rm = ap.recurrence_matrix(Y, metric=metric, width=width, k=k)
            eligible = np.array([sum(abs(i - j) >= width for i in range(n)) for j in range(n)])
            k_eff = R.default_k_recurrence(n, width) if k is None else k
            np.testing.assert_array_equal(Rm.sum(dim=1).cpu().numpy(), np.broadcast_to(np.minimum(k_eff, eligible), (2, n)))
            S = ap.recurrence_matrix(Y, metric=metric, width=width, k=k, sym=True, mode="distance")
            assert torch.equal(S, S.transpose(1, 2)) and (~(S != 0) | Rm).all()
            for M in (Rm, S):
                for pad in (True, False):
                    lag = ap.recurrence_to_lag(M, pad=pad)
                    assert lag.shape == (2, 2 * n if pad else n, n) and lag.dtype == M.dtype
                    assert torch.equal(ap.lag_to_recurrence(lag), M)
            assert torch.equal(ap.lag_to_recurrence(ap.recurrence_to_lag(Rm[0])), Rm[0])
    C = ap.cross_similarity(Y[:, :, :50], Y, k=9)
    np.testing.assert_array_equal(C.sum(dim=1).cpu().numpy(), np.full((2, 50), 9))
    assert E.same_bits(ap.recurrence_to_lag(Rm.cpu().numpy()).cpu().numpy(), R.to_lag(Rm.cpu().numpy()))      # host input


def test_gpu_a_clip_repeated_twice_shows_the_diagonal_at_half_its_length():
    sr, hop = 22050, 512
    rng = np.random.default_rng(5)
    t = np.arange(sr * 3) / sr
    notes = rng.choice([220.0, 246.9, 277.2, 293.7, 329.6, 370.0, 415.3, 440.0], 12)
    clip = np.concatenate([np.sin(2 * np.pi * f * t[:len(t) // 12]) * np.hanning(len(t) // 12) for f in notes]).astype(np.float32)
    clip = clip[:(len(clip) // hop) * hop]
    cens = ap.chroma_cens(y=np.concatenate([clip, clip]), sr=sr, hop_length=hop)
    cens = cens.reshape(-1, cens.shape[-2], cens.shape[-1])[0]
    n = cens.shape[-1]
    Rm = ap.recurrence_matrix(cens, k=1, width=3, mode="connectivity", sym=True)     # the nearest frame outside +-2: the copy
    lag = ap.recurrence_to_lag(Rm, pad=False).float().sum(dim=-1).cpu().numpy()
    half = len(clip) // hop
    lo = 3
    best = lo + int(np.argmax(lag[lo:n - lo]))
    print(f"n = {n}, half = {half}, strongest lag {best}, its count {lag[best]:.0f}, the median count {np.median(lag):.0f}")
    # n - half frames have a copy `half` frames later.  The copy's features differ only near a seam (the start, the
    # middle, the end): within the 20 frames the 41-frame smoothing reaches plus the 12 frames (11 685 taps / 512) of the
    # longest constant-Q filter, on either end of that stretch.  Everywhere else the copy is the mutual nearest frame.
    assert min(abs(best - half), abs(best - (n - half))) <= 1 and lag[best] >= (n - half) - 2 * (20 + 12)
