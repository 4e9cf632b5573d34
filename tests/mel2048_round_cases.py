"""Shapes shared by test_emu_mel2048_rounds.py (CPU emulator) and test_gpu_mel2048_rounds.py (GPU): one
filterbank per contraction pass count of ap_mel2048_run_kernel (1 to 4), the hop of the four-rotation frame
loop and one of the single-rotation loop, and clips whose ends fall inside a wave's stretch.  Not a test
module."""

import numpy as np

from oracle import audio_oracle as ao

HOPS = (512, 256)            # hop 512: registers shared between frames, four loop bodies; 256: one body
POWERS = (2.0, 1.0)
# B = 3 clips; hop 512 / 256: T = 18 / 36 (no multiple of 8, clip ends inside the 8 waves' stretches) and,
# for a clip shorter than a frame, T = 2 / 3 (fewer frames than waves: some waves have nothing to do)
LENGTHS = (9000, 600)
B = 3


def four_pass_bank():
    """128 triangular filters on a linear grid that need 4 contraction passes: ao.mel_filterbank has no
    parameters that reach more than 3 with n_mels <= 128 (a mel bank over 1025 bins has about
    128 + n_mels / 2 plan entries).  Rows 0..98 span 28 bins (two parts of more than 2 groups: two whole
    entries each), row 99 spans 60 bins (4 parts), rows 100..127 span 6 bins (short parts, paired)."""
    fb = np.zeros((128, 1025), np.float32)
    for m in range(128):
        if m < 99:
            a, w = 7 * m, 28
        elif m == 99:
            a, w = 700, 60
        else:
            a, w = 770 + 8 * (m - 100), 6
        k = np.arange(w)
        fb[m, a:a + w] = (1.0 - np.abs((k + 0.5) / (w / 2.0) - 1.0)) * (2.0 / w)
    return fb


# passes -> (sr, n_mels, mel_filterbank keywords) or None for four_pass_bank()
BANKS = {
    1: (22050, 20, dict(fmax=2000.0)),
    2: (22050, 128, dict(fmax=8000.0)),
    3: (22050, 128, {}),
    4: None,
}


def bank(passes):
    """(filterbank (M, 1025), sr, keywords for ao.melspectrogram, hand-made)"""
    if BANKS[passes] is None:
        return four_pass_bank(), 22050, dict(n_mels=128), True
    sr, M, kw = BANKS[passes]
    return ao.mel_filterbank(sr, 2048, M, **kw), sr, dict(n_mels=M, **kw), False


def check_plan(desc, M, passes):
    """The plan is one the run kernel takes (ap_prepare_mel_run) and needs exactly `passes` passes."""
    assert desc[0] & 2, "no part descriptors"
    assert M <= 128 and desc[12] <= 256 and desc[15] <= 4
    assert (desc[12] + 63) // 64 == passes


def signal(passes, hop, L):
    return np.random.default_rng(1000 * passes + hop + L).standard_normal((B, L)).astype(np.float32)


def reference(monkeypatch, y, fb, sr, hop, power, kw, hand_made):
    """ao.melspectrogram; for the hand-made bank its filterbank builder hands back that bank."""
    if hand_made:
        monkeypatch.setattr(ao, "mel_filterbank", lambda *a, **k: fb)
    return ao.melspectrogram(y, sr=sr, n_fft=2048, hop_length=hop, power=power, **kw)
