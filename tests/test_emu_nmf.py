"""CPU emulator: the NMF kernels (kernels_nmf.h, with the MFMA model of tests/emu/emu_mfma.h) against float64
(tests/nmf_ref.py), to the derived per-element bound of nmf_ref.one_step_bounds with no factor on top.  The binding
checks the poisoned bands, the NaN pad of V and the LDS limit on every call; the outputs have exactly K components, so
nothing of the zero padding to 16 / 32 / 64 can show."""

import os
import sys

import numpy as np
import pytest

import nmf_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_nmf_bind as E  # noqa: E402

CASES = [(s, l) for s in R.SHAPES for l in R.LOSSES]
CASE_IDS = [f"{i}-{l}" for i in R.IDS for l in R.LOSSES]


@pytest.mark.parametrize("shape,loss", CASES, ids=CASE_IDS)
def test_one_iteration_within_the_derived_bound(shape, loss):
    B, F, T, K = shape
    V, W0, H0 = R.case(shape)
    e_h, e_w = R.one_step_bounds(F, T, K, loss)
    # H alone: W must come back in every bit
    W, H = E.mu(V, W0, H0, loss, update_w=False)
    _, Hr = R.iterate(V, W0, H0, loss, update_components=False)
    assert np.array_equal(W, W0)
    err = R.rel_err(H, Hr)
    print(f"H alone: {err:.3e} of {e_h:.3e}")
    assert err <= e_h
    # the full iteration, on another grid: the same H bits, W within the compounded bound
    W, H2 = E.mu(V, W0, H0, loss, grid=2)
    Wr, Hr = R.iterate(V, W0, H0, loss)
    assert np.array_equal(H2, H)
    errs = R.rel_err(H2, Hr), R.rel_err(W, Wr)
    print(f"iteration: H {errs[0]:.3e} of {e_h:.3e}, W {errs[1]:.3e} of {e_w:.3e}")
    assert errs[0] <= e_h and errs[1] <= e_w
    assert all(np.array_equal(a, b) for a, b in zip(E.mu(V, W0, H0, loss), (W, H2)))          # the same bits again


@pytest.mark.parametrize("loss", R.LOSSES)
def test_objective(loss):
    shape = R.SHAPES[1]
    B, F, T, K = shape
    V, W0, H0 = R.case(shape)
    want = R.objective(V, W0, H0, loss)
    got = E.objective(V, W0, H0, loss)
    assert (np.abs(got - want) <= R.g(K + F * T) * np.abs(want)).all(), (got, want)
