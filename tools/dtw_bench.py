"""Steady-state times of the DTW kernels: the accumulated-cost recursion and the backtracking at one long pair
(B = 1, 7 750 x 7 750: two three-minute chroma sequences at hop 512), at B = 64, 1 000 x 1 000 and at B = 256, 431 x 431
(the batch of tools/chroma_bench.py), and the cost kernel at d = 12.

Protocol of tools/bench_configs.py (`steady`), as tools/chroma_bench.py: inputs resident in HBM, three rotating input
buffers, ramp-up with the operator itself, 5 back-to-back streams timed with HIP events; reported: the median stream and
the spread of the five.  Yardsticks.  Large batches: memory traffic, 9 bytes per cell (C once, D once, one step byte) at
the rate `preemphasis` reaches on 256 x 220 500 samples in the same session.  B = 1: the dependency chain, N + M - 1
dependent cells and one launch per tile-anti-diagonal: cells per second and the time per launch are reported.  The cost
kernel is compared with torch.cdist on the same tensors; the recursion with the numpy model of tests/dtw_ref.py on the
host (one pair of 1 000 x 1 000), the only other implementation there is.

  python tools/dtw_bench.py                      # every step, each in a child process under its own time limit;
                                                 # writes profiles/dtw_timings.txt (--out to choose another file)
  python tools/dtw_bench.py --only acc_b64       # one step in this process, one JSON line (for a kernel trace of it)
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pcen_bench import streams  # noqa: E402

SHAPES = {"b1": (1, 7750, 7750), "b64": (64, 1000, 1000), "b256": (256, 431, 431)}
# step -> time limit in seconds
STEPS = {"preemphasis": 120, "acc_b1": 240, "bt_b1": 240, "acc_b64": 180, "bt_b64": 180, "acc_b256": 180, "bt_b256": 180,
         "cost_d12": 120, "torch_cdist_d12": 120, "numpy_ref": 180}


def run_step(name, a):
    rep = {"step": name}
    if name == "numpy_ref":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import dtw_ref as R

        C = R.cost_matrix(1, 1000, 1000, 0)[0]
        R.accumulate(C[:100, :100])
        t0 = time.perf_counter()
        R.accumulate(C)
        ms = 1e3 * (time.perf_counter() - t0)
        rep.update(batch=1, N=1000, M=1000, cells=1.0e6, ms=ms, ms_min=ms, ms_max=ms, launches=0)
        return rep

    import torch

    import mlx_audio_primitives_amd as ap
    from mlx_audio_primitives_amd import _extension as _x
    from tools.bench_configs import N_ROT

    M = importlib.import_module("mlx_audio_primitives_amd.dtw")
    g = torch.Generator(device="cuda").manual_seed(42)

    def rand(*shape):
        return torch.rand(shape, device="cuda", generator=g)

    table = M._step_table(None, None, None)
    if name == "preemphasis":
        ys = [rand(256, 220500) for _ in range(N_ROT)]
        fn = lambda i: ap.preemphasis(ys[i % N_ROT])                                       # noqa: E731
        rep.update(batch=256, N=220500, M=1, cells=0.0, bytes=8.0 * 256 * 220500, launches=1)
    elif name.startswith(("acc_", "bt_")):
        B, N, Mm = SHAPES[name.split("_")[1]]
        rep.update(batch=B, N=N, M=Mm, cells=float(B) * N * Mm)
        n_diag = -(-N // 64) + -(-Mm // 64) - 1
        if name.startswith("acc_"):
            Cs = [rand(B, N, Mm) for _ in range(N_ROT)]
            fn = lambda i: M._accumulate(Cs[i % N_ROT], table, False, None)                # noqa: E731
            rep.update(bytes=9.0 * B * N * Mm, launches=n_diag)
        else:
            Ss = [M._accumulate(rand(B, N, Mm), table, False, None)[1] for _ in range(N_ROT)]
            path = torch.empty((B, N + Mm - 1, 2), dtype=torch.int32, device="cuda")
            lens = torch.empty((B,), dtype=torch.int32, device="cuda")
            ab = table[0]
            lib = _x.dlib(path.device)

            def fn(i):
                S = Ss[i % N_ROT]
                _x.check(lib.ap_dtw_backtrack_i32(None, _x.ptr(S), None, B, N, Mm, Mm, Mm, 3, ab.ctypes.data, 0, _x.ptr(path), _x.ptr(lens),
                                                  _x.stream_ptr(path.device)))
            fn(0)
            n_path = float(lens.sum().item())
            rep.update(bytes=n_path * 9.0, launches=1, path_cells=n_path)                  # a code read and two ints written per path cell
    else:
        B, N, Mm, d = 64, 1000, 1000, 12
        Xs = [rand(B, d, N) for _ in range(N_ROT)]
        Ys = [rand(B, d, Mm) for _ in range(N_ROT)]
        rep.update(batch=B, N=N, M=Mm, cells=float(B) * N * Mm, bytes=4.0 * B * N * Mm + 4.0 * B * d * (N + Mm), launches=1)
        if name == "cost_d12":
            fn = lambda i: M._cost(Xs[i % N_ROT], Ys[i % N_ROT], 0)                        # noqa: E731
        else:
            fn = lambda i: torch.cdist(Xs[i % N_ROT].transpose(1, 2), Ys[i % N_ROT].transpose(1, 2))   # noqa: E731
    ts = streams(fn, a.ramp)
    rep.update(ms=ts[len(ts) // 2], ms_min=ts[0], ms_max=ts[-1])
    return rep


def report(rows):
    """The text of profiles/dtw_timings.txt for {step: row of run_step}."""
    lines = ["dtw timings (tools/dtw_bench.py): ms per call, steady state, HIP events, three rotating inputs;",
             "median of 5 back-to-back streams, spread = (max - min) / median of the five",
             "acc_*: ap_dtw_accumulate_f32 (default steps), 9 bytes per cell; bt_*: ap_dtw_backtrack_i32, 9 bytes per path cell;",
             "GB/s = bytes / time; stream = share of the rate preemphasis reaches in the same session;",
             "us/launch = time / launches (one launch per tile-anti-diagonal); numpy_ref: tests/dtw_ref.py on the host", ""]
    rate = rows["preemphasis"]["bytes"] / rows["preemphasis"]["ms"] / 1e6 if "preemphasis" in rows else None
    lines.append(f"{'step':<18}{'batch':>6}{'N':>8}{'M':>6}{'ms':>11}{'min':>11}{'max':>11}{'spread':>8}{'Gcell/s':>9}{'GB/s':>9}{'stream':>8}"
                 f"{'launches':>9}{'us/launch':>10}")
    for name, r in rows.items():
        gbs = r["bytes"] / r["ms"] / 1e6 if "bytes" in r else None
        share = f"{gbs / rate:>8.1%}" if rate and gbs is not None and not name.startswith("torch") else f"{'':>8}"
        per = f"{1e3 * r['ms'] / r['launches']:>10.2f}" if r.get("launches") else f"{'':>10}"
        lines.append(f"{name:<18}{r['batch']:>6}{r['N']:>8}{r['M']:>6}{r['ms']:>11.4f}{r['ms_min']:>11.4f}{r['ms_max']:>11.4f}"
                     f"{(r['ms_max'] - r['ms_min']) / r['ms']:>8.1%}{r['cells'] / r['ms'] / 1e6:>9.3f}"
                     + (f"{gbs:>9.1f}" if gbs is not None else f"{'':>9}") + share + f"{r.get('launches', 0):>9}" + per)
    lines.append("")
    if "torch_cdist_d12" in rows and "cost_d12" in rows:
        lines.append(f"torch_cdist_d12 / cost_d12 = {rows['torch_cdist_d12']['ms'] / rows['cost_d12']['ms']:.2f}")
    if "numpy_ref" in rows:
        ref = rows["numpy_ref"]["cells"] / rows["numpy_ref"]["ms"]
        for k in ("acc_b1", "acc_b64", "acc_b256"):
            if k in rows:
                lines.append(f"{k} / numpy_ref, cells per second = {rows[k]['cells'] / rows[k]['ms'] / ref:.0f}")
    return "\n".join(lines) + "\n"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ramp", type=float, default=0.5)
    p.add_argument("--only", choices=list(STEPS))
    p.add_argument("--skip", choices=list(STEPS), action="append", default=[])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw_timings.txt"))
    a = p.parse_args()
    if a.only:
        print(json.dumps(run_step(a.only, a)))
        return 0
    rows = {}
    for name, limit in STEPS.items():
        if name in a.skip:
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--only", name, "--ramp", str(a.ramp)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:           # a fault, an abort or the time limit: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            print(f"step {name} ended with status {r.returncode}; stopping", file=sys.stderr)
            return 1
        rows[name] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(rows[name]), flush=True)
    text = report(rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
