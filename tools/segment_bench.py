"""Steady-state times of the recurrence-matrix kernels: every pass (threshold, bandwidth, write) and the whole call of
recurrence_matrix, for connectivity and for affinity with sym, at one five-minute clip (1 x 12 x 12 920: chroma at the
default hop), at 64 x 12 x 1 000 and at 256 x 128 x 431 (the batch of tools/chroma_bench.py with mel-sized features);
width 1 and the default k.

Protocol of tools/bench_configs.py (`steady`), as tools/dtw_bench.py: inputs resident in HBM, three rotating input
buffers, ramp-up with the operator itself, 5 back-to-back streams timed with HIP events; reported: the median stream and
the spread of the five.  Yardsticks, all measured in the same session: the output bytes written once (1 byte per cell
for connectivity, 4 for affinity) at the rate `preemphasis` reaches on 256 x 220 500 samples; and the torch composition
on the same tensors: dtw's cost launch, the diagonal set to +inf, torch.topk, a scatter into a zeroed matrix.

  python tools/segment_bench.py                  # every group, each in a child process under its own time limit;
                                                 # writes profiles/segment_timings.txt (--out to choose another file)
  python tools/segment_bench.py --only b64       # one group in this process, one JSON line per step
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pcen_bench import streams  # noqa: E402

SHAPES = {"b1": (1, 12, 12920), "b64": (64, 12, 1000), "b256": (256, 128, 431)}
# group -> time limit in seconds
GROUPS = {"preemphasis": 120, "b1": 300, "b64": 240, "b256": 240}
STEPS = ("thr", "bw", "write_conn", "write_aff_sym", "call_conn", "call_aff_sym", "torch_conn")


def run_group(name, a):
    import torch

    import mlx_audio_primitives_amd as ap
    from mlx_audio_primitives_amd import _extension as _x
    from tools.bench_configs import N_ROT

    g = torch.Generator(device="cuda").manual_seed(42)
    rows = []

    def timed(step, fn, **kw):
        ts = streams(fn, a.ramp)
        rows.append(dict(step=step, ms=ts[len(ts) // 2], ms_min=ts[0], ms_max=ts[-1], **kw))
        print(json.dumps(rows[-1]), flush=True)

    if name == "preemphasis":
        ys = [torch.rand((256, 220500), device="cuda", generator=g) for _ in range(N_ROT)]
        timed("preemphasis", lambda i: ap.preemphasis(ys[i % N_ROT]), batch=256, d=1, n=220500, k=0, bytes=8.0 * 256 * 220500)
        return rows

    S = importlib.import_module("mlx_audio_primitives_amd.segment")
    D = importlib.import_module("mlx_audio_primitives_amd.dtw")
    B, d, n = SHAPES[name]
    k = S._default_k(n - 1)
    xs = [torch.rand((B, d, n), device="cuda", generator=g) for _ in range(N_ROT)]
    dev = xs[0].device
    lib = _x.dlib(dev)
    sp = _x.stream_ptr(dev)
    rec = torch.empty((B, n, 2), dtype=torch.int32, device=dev)
    bw = torch.empty((B,), dtype=torch.float32, device=dev)
    out8 = torch.empty((B, n, n), dtype=torch.uint8, device=dev)
    out32 = torch.empty((B, n, n), dtype=torch.float32, device=dev)
    cells = float(B) * n * n
    common = dict(batch=B, d=d, n=n, k=k)

    def thr(i):
        x = xs[i % N_ROT]
        _x.check(lib.ap_segment_threshold_f32(_x.ptr(x), _x.ptr(x), B, d, n, n, n, n, 0, k, 1, _x.ptr(rec), sp))

    def write(i, mode, sym, out):
        x = xs[i % N_ROT]
        _x.check(lib.ap_segment_write_f32(_x.ptr(x), _x.ptr(x), B, d, n, n, n, n, 0, mode, 1, 0, sym, 0, _x.ptr(rec), _x.ptr(bw), 1.0, _x.ptr(out), n, sp))

    def torch_conn(i):
        x = xs[i % N_ROT]
        C = D._cost(x, x, 0)                                    # C[i, j]: rows are the reference frames
        C.diagonal(dim1=1, dim2=2).fill_(float("inf"))
        idx = torch.topk(C, k, dim=1, largest=False).indices    # the k nearest i of every query j
        return torch.zeros((B, n, n), dtype=torch.bool, device=dev).scatter_(1, idx, True)

    timed("thr", thr, bytes=8.0 * B * n, **common)
    thr(0)                                                      # the records of xs[0]: what the later steps read
    timed("bw", lambda i: _x.check(lib.ap_segment_bandwidth_f32(_x.ptr(rec), B, n, 0, _x.ptr(bw), sp)), bytes=8.0 * B * n, **common)
    timed("write_conn", lambda i: write(0, 0, 0, out8), bytes=cells, **common)
    timed("write_aff_sym", lambda i: write(0, 2, 1, out32), bytes=4.0 * cells, **common)
    timed("call_conn", lambda i: ap.recurrence_matrix(xs[i % N_ROT]), bytes=cells, **common)
    timed("call_aff_sym", lambda i: ap.recurrence_matrix(xs[i % N_ROT], mode="affinity", sym=True), bytes=4.0 * cells, **common)
    same = bool(torch.equal(torch_conn(0), ap.recurrence_matrix(xs[0])))
    timed("torch_conn", torch_conn, bytes=cells, same_as_call_conn=same, **common)
    return rows


def report(groups):
    """The text of profiles/segment_timings.txt for {group: rows of run_group}."""
    lines = ["segment timings (tools/segment_bench.py): ms per call, steady state, HIP events, three rotating inputs;",
             "median of 5 back-to-back streams, spread = (max - min) / median of the five; euclidean, width 1, default k",
             "thr / bw / write_*: the C entries on preallocated buffers; call_*: recurrence_matrix as a user calls it (call_aff_sym",
             "includes the 4-byte copy of the estimated bandwidth); torch_conn: cost launch + diagonal + topk + scatter;",
             "GB/s = output bytes / time; stream = share of the rate preemphasis reaches in the same session;",
             "share = the pass's time over thr + write (connectivity) or thr + bw + write (affinity)", ""]
    pre = groups.get("preemphasis", [None])[0]
    rate = pre["bytes"] / pre["ms"] / 1e6 if pre else None
    lines.append(f"{'group':<12}{'step':<16}{'batch':>6}{'d':>5}{'n':>7}{'k':>5}{'ms':>11}{'min':>11}{'max':>11}{'spread':>8}{'GB/s':>9}{'stream':>8}{'share':>16}")
    for gname, rows in groups.items():
        by = {r["step"]: r for r in rows}
        for r in rows:
            gbs = r["bytes"] / r["ms"] / 1e6
            stream = f"{gbs / rate:>8.1%}" if rate and r["step"] not in ("thr", "bw") else f"{'':>8}"
            share = ""
            if r["step"] in ("thr", "bw", "write_conn", "write_aff_sym") and "write_conn" in by:
                conn, aff = by["thr"]["ms"] + by["write_conn"]["ms"], by["thr"]["ms"] + by["bw"]["ms"] + by["write_aff_sym"]["ms"]
                share = {"thr": f"{r['ms'] / conn:.0%} / {r['ms'] / aff:.0%}", "bw": f"- / {r['ms'] / aff:.0%}",
                         "write_conn": f"{r['ms'] / conn:.0%} / -", "write_aff_sym": f"- / {r['ms'] / aff:.0%}"}[r["step"]]
            lines.append(f"{gname:<12}{r['step']:<16}{r['batch']:>6}{r['d']:>5}{r['n']:>7}{r['k']:>5}{r['ms']:>11.4f}{r['ms_min']:>11.4f}{r['ms_max']:>11.4f}"
                         f"{(r['ms_max'] - r['ms_min']) / r['ms']:>8.1%}{gbs:>9.1f}{stream}{share:>16}")
        if "torch_conn" in by:
            lines.append(f"{gname}: torch_conn / call_conn = {by['torch_conn']['ms'] / by['call_conn']['ms']:.2f}; the two give the same matrix: "
                         f"{by['torch_conn']['same_as_call_conn']} (random data has no ties)")
        lines.append("")
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ramp", type=float, default=0.5)
    p.add_argument("--only", choices=list(GROUPS))
    p.add_argument("--skip", choices=list(GROUPS), action="append", default=[])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_timings.txt"))
    a = p.parse_args()
    if a.only:
        run_group(a.only, a)
        return 0
    groups = {}
    for name, limit in GROUPS.items():
        if name in a.skip:
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--only", name, "--ramp", str(a.ramp)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:           # a fault, an abort or the time limit: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            print(f"group {name} ended with status {r.returncode}; stopping", file=sys.stderr)
            return 1
        groups[name] = [json.loads(line) for line in r.stdout.strip().splitlines() if line.startswith("{")]
        print(r.stdout, flush=True)
    text = report(groups)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
