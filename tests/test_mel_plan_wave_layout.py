"""Host plan builder (ap_mel_plan_host): the wave layout of a filterbank plan, with and without the exchange of
entries that frees the plane reads of ap_mel2048_run_kernel from bank conflicts.

The exchange runs only for plans that kernel can take (1025 bins, at most 4 passes); it is quadratic in the
positions of a layout, so wide and dense banks - which filterbank_spectrogram accepts as well - must not get it.
Whatever the layout, it has to hold the filterbank: every weight exactly once, under the slot of its row."""

import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mel2048_round_cases as rc  # noqa: E402

from mlx_audio_primitives_amd import _extension as _x  # noqa: E402


def rebuild(plan, desc):
    """The dense filterbank that the wave layout of a plan computes: entry e reads weight row i at quad
    256 (e // 64) + 64 i + e % 64; rows 0-1 weigh groups gA, gA + 1 into slot A, rows 2-3 groups gB, gB + 1 into
    slot B (-1: slot A).  Slots belong to rows through rowstart; the slot past the last one is the dump."""
    M, F, n_slots = int(desc[1]), int(desc[2]), int(desc[7])
    n_ent, n_quads = int(desc[12]), int(desc[14])
    assert n_ent % 64 == 0 and n_quads == 4 * n_ent
    rowstart = plan[desc[10]:desc[10] + M + 1]
    assert rowstart[M] == n_slots
    row_of = np.repeat(np.arange(M), np.diff(rowstart))
    ent = plan[desc[11]:desc[11] + 4 * n_ent].reshape(n_ent, 4)
    wq = plan[desc[13]:desc[13] + 4 * n_quads].view(np.float32).reshape(n_quads, 4)
    fb = np.zeros((M, 4 * ((F + 3) // 4) + 16), np.float32)
    for e, (sa, ga, sb, gb) in enumerate(ent):
        col = 256 * (e // 64) + e % 64
        for i in range(4):
            slot, g = (sa, ga + i) if i < 2 else (sa if sb < 0 else sb, gb + i - 2)
            w = wq[col + 64 * i]
            if slot == n_slots:
                assert not w.any(), "weights that end in the dump slot"
                continue
            assert 0 <= slot < n_slots
            assert not fb[row_of[slot], 4 * g:4 * g + 4][w != 0].any(), "a weight twice"
            fb[row_of[slot], 4 * g:4 * g + 4] += w
    assert not fb[:, F:].any()
    return fb[:, :F]


def dense_bank(M, F, seed):
    return (np.random.default_rng(seed).random((M, F)) + 0.5).astype(np.float32)


BANKS = {
    "headline": lambda: _x.mel_filterbank_host(22050, 2048, 128),           # 3 passes: entries exchanged
    "four_pass": lambda: rc.bank(4)[0],                                     # 4 passes: entries exchanged
    "one_pass": lambda: rc.bank(1)[0],
    "n_fft_512": lambda: _x.mel_filterbank_host(22050, 512, 40),            # another n_fft: dealing alone
    "n_fft_4096": lambda: _x.mel_filterbank_host(22050, 4096, 128),         # 5 passes, 2049 bins
    "dense_12x1025": lambda: dense_bank(12, 1025, 1),                       # 1025 bins, 13 passes: dealing alone
    "dense_40x1025": lambda: dense_bank(40, 1025, 2),                       # 41 passes
    "dense_3x257": lambda: dense_bank(3, 257, 3),
}


@pytest.mark.parametrize("name", sorted(BANKS))
def test_wave_layout_holds_the_filterbank(name):
    fb = np.ascontiguousarray(BANKS[name](), np.float32)
    plan, desc = _x.mel_plan_host(fb)
    assert int(desc[3]) == plan.size
    np.testing.assert_array_equal(rebuild(plan, desc), fb)


def test_headline_plan_got_the_exchange():
    """Bank cycles of the 12 plane reads of the headline plan (tools/lds_banks.py; ideal 48).  Dealing the entries
    of a pass to the lane groups alone cannot go below 64: one pass holds one residue modulo 16 eight times, two
    per lane group at best, which is 32 cycles for that pass and at least 16 for each of the other two.  Fewer
    than 64 therefore shows that entries moved between passes.  The weight reads stay at their ideal."""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import lds_banks
    plan, desc = _x.mel_plan_host(np.ascontiguousarray(BANKS["headline"](), np.float32))
    rc.check_plan(desc, 128, 3)
    per_pass = lds_banks.mel_plan_reads(plan, desc, slot_bytes=8)
    print("plane reads per pass:", [p[0] for p in per_pass])
    assert sum(p[0] for p in per_pass) < 64 and all(p[1] == 16 for p in per_pass)
