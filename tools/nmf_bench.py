"""Per-iteration times of nmf's multiplicative updates at F = 1025, T = 2000, K = 32 for B = 1, 16, 64, both losses,
and for scale the same iteration composed from torch.matmul at equal shapes.

One launch is ap_nmf_mu_f32 with --iters iterations (one C call, no readback); V, W and H stay in HBM.  After a ramp-up
with the operator itself, 5 back-to-back streams of launches are timed with device events; a row is the median and the
range of the 5, per iteration.  Floor: V read twice per iteration (4 B x 2 per element) at 6 TB/s.  Frobenius runs on the
Gram route (kernels_nmf.h); the fused W^T (W H) route was not built, so there is no second Frobenius column.

  python tools/nmf_bench.py                    # every step in a child process under its own time limit; writes
                                               # profiles/nmf_timings.txt (--out to choose another file)
  python tools/nmf_bench.py --only mu_frobenius_b16     # one step in this process, one JSON line
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOSSES = ("frobenius", "kullback-leibler")
BATCHES = (1, 16, 64)
STEPS = {f"{kind}_{loss}_b{B}": 150 for kind in ("mu", "torch") for loss in LOSSES for B in BATCHES}     # step -> seconds
HBM = 6e12


def torch_iteration(V, W, H, loss, eps):
    import torch

    Wt = W.transpose(1, 2)
    if loss == 0:
        H = H * torch.matmul(Wt, V) / (torch.matmul(torch.matmul(Wt, W), H) + eps)
        Ht = H.transpose(1, 2)
        W = W * torch.matmul(V, Ht) / (torch.matmul(W, torch.matmul(H, Ht)) + eps)
    else:
        H = H * torch.matmul(Wt, V / (torch.matmul(W, H) + eps)) / (W.sum(1)[:, :, None] + eps)
        W = W * torch.matmul(V / (torch.matmul(W, H) + eps), H.transpose(1, 2)) / (H.sum(2)[:, None, :] + eps)
    return W, H


def run_step(name, a):
    import torch

    from mlx_audio_primitives_amd import _extension as ext

    kind, loss_name, b = name.split("_")
    loss, B, F, T, K = LOSSES.index(loss_name), int(b[1:]), a.bins, a.frames, a.components
    g = torch.Generator(device="cuda").manual_seed(42)
    V = torch.rand((B, F, K), device="cuda", generator=g) ** 4 @ torch.rand((B, K, T), device="cuda", generator=g) ** 2
    V += 0.01 * torch.rand((B, F, T), device="cuda", generator=g)
    s = float(torch.sqrt(V.mean() / K))
    state = [s * torch.randn((B, F, K), device="cuda", generator=g).abs(), s * torch.randn((B, K, T), device="cuda", generator=g).abs()]
    L = ext.dlib(V.device)
    ws = torch.empty(int(L.ap_nmf_workspace_bytes(B, F, T, K, loss)) // 8 + 1, dtype=torch.float64, device="cuda")
    stream = ext.stream_ptr(V.device)

    def launch():
        if kind == "mu":
            ext.check(L.ap_nmf_mu_f32(ext.ptr(V), B, F, T, T, K, ext.ptr(state[0]), ext.ptr(state[1]), a.iters, loss, 1, 1e-10,
                                      ext.ptr(ws), stream))
        else:
            for _ in range(a.iters):
                state[0], state[1] = torch_iteration(V, state[0], state[1], loss, 1e-10)

    launch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    launch()
    torch.cuda.synchronize()
    n = max(1, min(50, int(0.2 / max(time.perf_counter() - t0, 1e-5))))            # ~0.2 s per stream
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.ramp:
        launch()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            launch()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / (n * a.iters))
    ts.sort()
    assert bool(torch.isfinite(state[1]).all())
    return {"step": name, "batch": B, "F": F, "T": T, "K": K, "ms": ts[2], "ms_min": ts[0], "ms_max": ts[-1], "launches": n,
            "floor_ms": B * F * T * 8 / HBM * 1e3}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--bins", type=int, default=1025)
    p.add_argument("--frames", type=int, default=2000)
    p.add_argument("--components", type=int, default=32)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--ramp", type=float, default=0.5)
    p.add_argument("--only", choices=list(STEPS))
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "nmf_timings.txt"))
    a = p.parse_args()
    if a.only:
        print(json.dumps(run_step(a.only, a)))
        return 0
    rows = {}
    for name, limit in STEPS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--only", name, "--bins", str(a.bins),
               "--frames", str(a.frames), "--components", str(a.components), "--iters", str(a.iters), "--ramp", str(a.ramp)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:           # a fault, an abort or the time limit: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            print(f"step {name} ended with status {r.returncode}; stopping", file=sys.stderr)
            return 1
        rows[name] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(rows[name]), flush=True)
    lines = [f"nmf timings (tools/nmf_bench.py): ms per iteration (update H, then W), F = {a.bins}, T = {a.frames}, K = {a.components}",
             f"{a.iters} iterations per launch, median [min .. max] of 5 streams of launches, device events; floor = V read twice at 6 TB/s",
             "mu = ap_nmf_mu_f32 (Frobenius on the Gram route; the fused route was not built), torch = the same iteration from torch.matmul", ""]
    lines.append(f"{'loss':<18}{'batch':>6}{'mu ms':>10}{'[min .. max]':>22}{'x floor':>9}{'torch ms':>10}{'[min .. max]':>22}{'torch / mu':>11}")
    for loss in LOSSES:
        for B in BATCHES:
            m, t = rows[f"mu_{loss}_b{B}"], rows[f"torch_{loss}_b{B}"]
            lines.append(f"{loss:<18}{B:>6}{m['ms']:>10.4f}{'[%.4f .. %.4f]' % (m['ms_min'], m['ms_max']):>22}{m['ms'] / m['floor_ms']:>9.1f}"
                         f"{t['ms']:>10.4f}{'[%.4f .. %.4f]' % (t['ms_min'], t['ms_max']):>22}{t['ms'] / m['ms']:>11.2f}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
