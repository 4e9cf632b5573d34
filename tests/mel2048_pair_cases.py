"""Shared by test_emu_mel2048_pairs.py and test_gpu_mel2048_pairs.py.  Not a test module.

paths(): which body of ap_mel2048_run_kernel's hop-512 frame loop computes each frame, for a launch cut into
`workers` stretches (the emulator launches one workgroup: 8; the GPU launcher ceil(frames / 64) workgroups of 8
waves, at most 256).  It restates the loop's rule (rotation r0 = t mod 4 at the stretch's start, one step a frame; a
frame at an even rotation pairs with its successor when that is in the same clip and stretch) and is used only to
assert that a shape covers what its test claims, never to predict a value.

high_bin_bank(): a filterbank with weight up to bin 1024, whose plan has entries that start at the |X|^2 groups
253 to 256 and so read up to group 259 - floats 1025 to 1039, behind the plane."""

import numpy as np


def gpu_workers(n_frames):
    return 8 * max(1, min(256, -(-n_frames // 64)))


def paths(B, T, workers=8):
    """{frame of a clip: set of 'pair' / 'single'} over the B clips."""
    seen = {}
    N = B * T
    for w in range(workers):
        f, hi = N * w // workers, N * (w + 1) // workers
        if f >= hi:
            continue
        rot = (f % T) & 3
        while f < hi:
            t = f % T
            if rot % 2 == 0 and t + 1 != T and f + 1 < hi:
                seen.setdefault(t, set()).add("pair")
                seen.setdefault(t + 1, set()).add("pair")
                f += 2
                rot = (rot + 2) & 3
            else:
                seen.setdefault(t, set()).add("single")
                f += 1
                rot = (rot + 1) & 3
    return seen


def on_both_paths(B, T, workers=8):
    return [t for t, s in paths(B, T, workers).items() if s == {"pair", "single"}]


def high_bin_bank():
    """128 triangles of 16 bins on a linear grid, 8 bins apart, cut off at bin 1024: row 126 covers bins 1009 to 1024,
    row 127 bins 1017 to 1024."""
    fb = np.zeros((128, 1025), np.float32)
    k = np.arange(16)
    tri = ((1.0 - np.abs((k + 0.5) / 8.0 - 1.0)) / 8.0).astype(np.float32)
    for m in range(128):
        a = 1 + 8 * m
        b = min(a + 16, 1025)
        fb[m, a:b] = tri[:b - a]
    return fb


def reads_behind_the_plane(plan, desc):
    """Largest |X|^2 group an entry of the wave layout reads (half A: gA, gA + 1; half B: gB, gB + 1)."""
    n = int(desc[12])
    parts = np.asarray(plan[desc[11]:desc[11] + 4 * n]).reshape(n, 4)
    return int(max(parts[:, 1].max(), parts[:, 3].max())) + 1
