"""Timings of pyin: the observation kernel, the banded decode and the whole call at 256 clips x 220 500
samples with the defaults, and the banded decode against the dense decode of the same model at 512 bins x 2 (the dense
kernel's largest).  Device events, median of 7 after 2 warm-up calls.  Usage: python tools/pyin_bench.py [out.txt]"""

import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mlx_audio_primitives_amd as ap  # noqa: E402
from mlx_audio_primitives_amd import _extension as _x  # noqa: E402
from mlx_audio_primitives_amd import pitch  # noqa: E402


def timed(fn, warmup=2, reps=7):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def decode_call(E, tab, nb):
    B, T = E.shape[0], E.shape[1]
    t = {k: dev(tab[k]) for k in ("lw", "lz", "ls", "freq")}
    ptr = torch.empty((B, T, 2 * nb), dtype=torch.int16, device="cuda")
    st = torch.empty((B, T), dtype=torch.int32, device="cuda")
    f0 = torch.empty((B, T), device="cuda")
    vo = torch.empty((B, T), dtype=torch.uint8, device="cuda")
    lp = torch.empty((B,), dtype=torch.float64, device="cuda")
    d, s = _x.dlib(E.device), _x.stream_ptr(E.device)
    return lambda: _x.check(d.ap_pyin_decode_f32(_x.ptr(E), B, nb, T, _x.ptr(t["lw"]), tab["h"], _x.ptr(t["lz"]), _x.ptr(t["ls"]), tab["li"],
                                                 _x.ptr(t["freq"]), 1, float("nan"), _x.ptr(ptr), _x.ptr(st), _x.ptr(f0), _x.ptr(vo), _x.ptr(lp), 0, s))


def main():
    out = []
    B, L, sr, fl, hop = 256, 220500, 22050, 2048, 512
    fmin, fmax = 65.40639132514966, 2093.004522404789
    rng = np.random.default_rng(0)
    t = np.arange(L) / sr
    f = 220.0 * 2.0 ** (rng.uniform(-1, 1, (B, 1)) + 0.02 * np.sin(2 * np.pi * 5 * t)[None])
    y = dev((np.sin(2 * np.pi * np.cumsum(f, axis=1) / sr) + 0.1 * rng.standard_normal((B, L))).astype(np.float32))
    curve = ap.yin_cmnd(y, fmin=fmin, fmax=fmax, sr=sr, frame_length=fl, hop_length=hop)
    n_lags, T = curve.shape[1], curve.shape[2]
    lo = max(int(math.floor(sr / fmax)), 1)
    tab = pitch._pyin_tables(fmin=fmin, fmax=fmax, sr=sr, hop=hop, n_lags=n_lags, n_thresholds=100, beta_parameters=(2, 18),
                             boltzmann_parameter=2, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01)
    nb = tab["n_bins"]
    tt = {k: dev(tab[k]) for k in ("thr", "beta", "ea", "nz")}
    E = torch.empty((B, T, nb + 1), device="cuda")
    vp = torch.empty((B, T), device="cuda")
    d, s = _x.dlib(E.device), _x.stream_ptr(E.device)
    observe = lambda: _x.check(d.ap_pyin_observe_f32(_x.ptr(curve), B, n_lags, T, lo, float(sr), fmin, tab["bps"], nb, _x.ptr(tt["thr"]),  # noqa: E731
                                                     _x.ptr(tt["beta"]), 100, _x.ptr(tt["ea"]), _x.ptr(tt["nz"]), int(tt["ea"].numel()), 0.01,
                                                     _x.ptr(E), _x.ptr(vp), s))
    out.append(f"pyin defaults, {B} clips x {L} samples: {T} frames, {n_lags} lags, {nb} bins x 2, W = {tab['W']}")
    out.append(f"  yin_cmnd            {timed(lambda: ap.yin_cmnd(y, fmin=fmin, fmax=fmax, sr=sr, frame_length=fl, hop_length=hop)):9.3f} ms")
    out.append(f"  observation kernel  {timed(observe):9.3f} ms")
    out.append(f"  banded decode       {timed(decode_call(E, tab, nb)):9.3f} ms")
    out.append(f"  pyin, whole call    {timed(lambda: ap.pyin(y, fmin=fmin, fmax=fmax, sr=sr)):9.3f} ms")
    # banded against dense at 512 bins: the same model as a (1024, 1024) transition matrix
    nb, W, Td = 512, 101, 431
    lw, lz, ls = pitch._pyin_band(nb, W, 0.01)
    tab2 = dict(lw=lw, lz=lz, ls=ls, freq=np.arange(nb, dtype=np.float32), h=W // 2, li=float(np.float32(math.log(1 / (2 * nb)))))
    prob = np.where(rng.uniform(size=(1, nb + 1, Td)) < 0.01, rng.uniform(size=(1, nb + 1, Td)), 0.0).astype(np.float32)
    for Bd in (1, 256):
        p = dev(np.repeat(prob, Bd, axis=0))
        E2 = torch.empty((Bd, Td, nb + 1), device="cuda")
        flags = torch.empty((Bd,), dtype=torch.int32, device="cuda")
        _x.check(d.ap_viterbi_emission_f32(_x.ptr(p), Bd, nb + 1, Td, Td, 0, None, _x.ptr(E2), _x.ptr(flags), s))
        banded = timed(decode_call(E2, tab2, nb))
        Ed = torch.cat([E2[:, :, :nb], E2[:, :, nb:].expand(Bd, Td, nb)], dim=2).contiguous()
        with np.errstate(divide="ignore"):
            lt = np.kron(np.exp(ls.astype(np.float64)).reshape(2, 2), ap.transition_local(nb, W))
        ltd, lid = dev(np.log(lt + np.finfo(np.float32).tiny).astype(np.float32)), dev(np.full(2 * nb, tab2["li"], np.float32))
        ptr = torch.empty((Bd, Td, 2 * nb), dtype=torch.int16, device="cuda")
        st = torch.empty((Bd, Td), dtype=torch.int32, device="cuda")
        lp = torch.empty((Bd,), dtype=torch.float64, device="cuda")
        dense = timed(lambda: _x.check(d.ap_viterbi_decode_f32(_x.ptr(Ed), Bd, 2 * nb, Td, _x.ptr(ltd), _x.ptr(lid), _x.ptr(ptr), _x.ptr(st),
                                                               _x.ptr(lp), s)))
        out.append(f"decode, {nb} bins x 2, W = {W}, T = {Td}, B = {Bd}: banded {banded:9.3f} ms   dense (1024 states) {dense:9.3f} ms")
    text = "\n".join(out)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
