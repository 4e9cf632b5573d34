"""GPU: nmf / decompose.decompose against the float64 definition of tests/nmf_ref.py, on its four shapes and both
losses.  test_one_iteration is what pins the MFMA lane layout of kernels_nmf.h on the hardware: the CPU twin runs the
same kernel against a model of the instruction, which a kernel written to that model would agree with either way.
Every case prints its figures before it asserts; the bounds come from nmf_ref, never from such figures."""

import numpy as np
import pytest
import torch

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _extension as ext

import nmf_ref as R

pytestmark = pytest.mark.gpu

CASES = [(s, l) for s in R.SHAPES for l in R.LOSSES]
CASE_IDS = [f"{i}-{l}" for i in R.IDS for l in R.LOSSES]
both = pytest.mark.parametrize("shape,loss", CASES, ids=CASE_IDS)


def padded(V, pad=5):
    """V on the device as a view of rows with `pad` NaN columns behind them."""
    buf = torch.full(V.shape[:-1] + (V.shape[-1] + pad,), float("nan"), device="cuda")
    buf[..., :V.shape[-1]] = torch.from_numpy(V).cuda()
    return buf[..., :V.shape[-1]]


def run(V, W, H, loss, n, **kw):
    W, H = ap.nmf(V, W.shape[-1], beta_loss=loss, init="custom", W=W, H=H, max_iter=n, tol=0, **kw)
    return W.cpu().numpy(), H.cpu().numpy()


@both
def test_one_iteration(shape, loss):
    B, F, T, K = shape
    V, W0, H0 = R.case(shape)
    W, H = run(padded(V), W0, H0, loss, 1)
    assert W.shape == (B, F, K) and H.shape == (B, K, T)
    Wr, Hr = R.iterate(V, W0, H0, loss)
    e_h, e_w = R.one_step_bounds(F, T, K, loss)
    errs = R.rel_err(H, Hr), R.rel_err(W, Wr)
    print(f"H {errs[0]:.3e} of {e_h:.3e}, W {errs[1]:.3e} of {e_w:.3e}")
    assert errs[0] <= e_h and errs[1] <= e_w
    W2, H2 = run(V, W0, H0, loss, 1)                                   # dense rows, a second call: the same bits
    assert np.array_equal(W2, W) and np.array_equal(H2, H)


@both
def test_five_iterations(shape, loss):
    B, F, T, K = shape
    V, W0, H0 = R.case(shape)
    ref = R.iterate(V, W0, H0, loss, 5)
    f32 = R.iterate(V, W0, H0, loss, 5, dtype=np.float32)
    got = run(V, W0, H0, loss, 5)
    for name, x, x32, r, floor in zip("WH", got, f32, ref, reversed(R.one_step_bounds(F, T, K, loss))):
        err, err32 = np.abs(x - r).max() / r.max(), np.abs(x32 - r).max() / r.max()
        bound = max(4 * err32, floor)
        print(f"{name}: {err:.3e}, float32 numpy {err32:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
        assert err <= bound


@both
def test_objective(shape, loss):
    B, F, T, K = shape
    V, W0, H0 = R.case(shape)
    Vd, Wd, Hd = (torch.from_numpy(a).cuda() for a in (V, W0, H0))
    L = ext.dlib(Vd.device)
    code = R.LOSSES.index(loss)
    ws = torch.empty(int(L.ap_nmf_workspace_bytes(B, F, T, K, code)) // 8 + 1, dtype=torch.float64, device="cuda")
    out = torch.empty(B, dtype=torch.float64, device="cuda")
    ext.check(L.ap_nmf_objective_f32(ext.ptr(Vd), B, F, T, T, K, ext.ptr(Wd), ext.ptr(Hd), code, 1e-10, ext.ptr(out), ext.ptr(ws),
                                     ext.stream_ptr(Vd.device)))
    got, want = out.cpu().numpy(), R.objective(V, W0, H0, loss)
    print(np.abs(got - want) / want, R.g(K + F * T))
    assert (np.abs(got - want) <= R.g(K + F * T) * want).all()


@both
def test_objective_never_rises(shape, loss):
    V, W, H = R.case(shape)
    Vd = torch.from_numpy(V).cuda()
    before = R.objective(V, W, H, loss)
    for it in range(30):
        W, H = run(Vd, W, H, loss, 1)
        after = R.objective(V, W, H, loss)
        assert (after <= before * (1 + 1e-6)).all(), (it, before, after)
        before = after


def test_fixed_dictionary_sort_and_stopping():
    V, W0, H0 = R.case(R.SHAPES[1])
    W, H = ap.nmf(V, 17, update_components=False, W=W0[0], max_iter=3, tol=0, random_state=1)
    assert np.array_equal(W.cpu().numpy(), np.broadcast_to(W0[0], W0.shape))
    assert H.shape == H0.shape and bool((H >= 0).all())
    Ws, Hs = ap.decompose.decompose(V, 17, sort=True, max_iter=20, tol=0, random_state=2)
    Wu, Hu = ap.decompose.decompose(V, 17, max_iter=20, tol=0, random_state=2)
    peaks = Ws.argmax(dim=-2).cpu().numpy()
    assert (np.diff(peaks, axis=-1) >= 0).all()
    order = np.argsort(Wu.argmax(dim=-2).cpu().numpy(), axis=-1, kind="stable")
    assert np.array_equal(Ws.cpu().numpy(), np.take_along_axis(Wu.cpu().numpy(), order[:, None, :], -1))
    assert np.array_equal(Hs.cpu().numpy(), np.take_along_axis(Hu.cpu().numpy(), order[:, :, None], -2))
    W, H, n = ap.nmf(V, 17, max_iter=200, tol=1e-2, random_state=3, return_n_iter=True)
    assert n % 10 == 0 and 10 <= n < 200
    assert ap.nmf(V, 17, max_iter=7, tol=0, return_n_iter=True)[2] == 7
