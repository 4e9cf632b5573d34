"""Steady-state times of pcen on the headline batch (256 clips x 220 500 samples @22.05 kHz, n_fft 2048, hop 512: a
256 x 128 x 431 mel spectrogram in `melspectrogram`'s line-padded layout, times 2^31).

Protocol of tools/bench_configs.py (`steady`): inputs resident in HBM, three rotating input buffers, ramp-up with the
operator itself, 5 back-to-back streams timed with HIP events; reported: the median stream and the spread (min .. max)
of the five.  The kernel moves 8 bytes per element (S read once, out written once).  It is compared with things that
are not itself:
  preemphasis        the package's other 8-byte-per-element filter on the same machine in the same session, on a
                     signal of as many elements: the bandwidth a streaming kernel reaches here
  torch_chain        the pointwise chain alone in torch on a smoother that is already there (exp, log, log1p, expm1 as
                     torch composes them): a lower bound on what a torch user pays, since torch has no IIR

  python tools/pcen_bench.py                        # every step, each in a child process under its own time limit;
                                                    # writes profiles/pcen_timings.txt (--out to choose another file)
  python tools/pcen_bench.py --only pcen_kernel     # one step in this process, one JSON line (for a kernel trace of it)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# step -> time limit in seconds
STEPS = {"pcen": 120, "pcen_kernel": 120, "pcen_kernel_dense": 120, "pcen_max3": 120, "pcen_power0": 120, "pcen_bias0": 120,
         "pcen_gain0": 120, "preemphasis": 120, "torch_chain": 120}
BYTES = 8


def streams(fn, ramp_s, n_streams=5):
    """tools/bench_configs.steady, returning every stream: sorted ms per launch."""
    import torch

    fn(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(1)
    torch.cuda.synchronize()
    one = max(time.perf_counter() - t0, 1e-5)
    n_launch = max(3, min(200, int(0.03 / one)))
    t0 = time.perf_counter()
    i = 0
    while time.perf_counter() - t0 < ramp_s:
        for _ in range(n_launch):
            fn(i)
            i += 1
        torch.cuda.synchronize()
    ts = []
    for _ in range(n_streams):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_launch):
            fn(i)
            i += 1
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / n_launch)
    return sorted(ts)


def run_step(name, a):
    import torch

    import mlx_audio_primitives_amd as ap
    from mlx_audio_primitives_amd import _extension as _x
    from mlx_audio_primitives_amd.pcen import smoothing_coefficient
    from tools.bench_configs import N_ROT

    g = torch.Generator(device="cuda").manual_seed(42)
    B, L = a.batch, a.samples
    rep = {"step": name, "batch": B, "samples": L}
    ys = [torch.randn((B, L), device="cuda", generator=g) * 0.1 for _ in range(N_ROT)]
    mels = []
    for y in ys:
        mel = ap.melspectrogram(y)
        S = torch.empty_strided(mel.shape, mel.stride(), dtype=torch.float32, device="cuda")
        torch.mul(mel, 2.0 ** 31, out=S)
        mels.append(S)
    _, M, T = mels[0].shape
    n = B * M * T
    rep.update(M=M, T=T, row_stride=int(mels[0].stride(1)), elements=n)
    if name == "preemphasis":
        del mels
        x = [torch.randn((B * M, T), device="cuda", generator=g) for _ in range(N_ROT)]
        ts = streams(lambda i: ap.preemphasis(x[i % N_ROT]), a.ramp)
    elif name == "torch_chain":
        del ys
        b = smoothing_coefficient(0.4, 22050, 512)
        sm = [m.contiguous() * b + 1.0 for m in mels]             # some smoother: its values do not matter to the time
        Sc = [m.contiguous() for m in mels]

        def chain(i):
            S, Ms = Sc[i % N_ROT], sm[i % N_ROT]
            smooth = torch.exp(-0.98 * torch.log(1e-6 + Ms))
            return (2.0 ** 0.5) * torch.expm1(0.5 * torch.log1p(S * smooth / 2.0))
        ts = streams(chain, a.ramp)
    elif name in ("pcen_kernel", "pcen_kernel_dense"):
        del ys
        if name.endswith("dense"):
            mels = [m.contiguous() for m in mels]
        outs = [torch.empty((B, M, T), device="cuda") for _ in range(N_ROT)]
        b = smoothing_coefficient(0.4, 22050, 512)

        def kernel(i):
            m = mels[i % N_ROT]
            _x.check(_x.dlib(m.device).ap_pcen_f32(_x.ptr(m), B, M, T, int(m.stride(1)), None, 0, 1, b, 0.98, 2.0, 0.5, 1e-6,
                                                   None, _x.ptr(outs[i % N_ROT]), T, None, _x.stream_ptr(m.device)))
        ts = streams(kernel, a.ramp)
    else:
        del ys
        kw = {"pcen": {}, "pcen_max3": dict(max_size=3), "pcen_power0": dict(power=0.0), "pcen_bias0": dict(bias=0.0),
              "pcen_gain0": dict(gain=0.0)}[name]
        ts = streams(lambda i: ap.pcen(mels[i % N_ROT], **kw), a.ramp)
    rep.update(ms=ts[len(ts) // 2], ms_min=ts[0], ms_max=ts[-1])
    return rep


def report(rows):
    """The text of profiles/pcen_timings.txt for {step: row of run_step}."""
    lines = ["pcen timings (tools/pcen_bench.py): ms per call, steady state, HIP events, three rotating inputs;",
             "median of 5 back-to-back streams, spread = (max - min) / median of the five",
             f"GB/s = {BYTES} B per element (one read, one write) / time", ""]
    lines.append(f"{'step':<22}{'batch':>6}{'ms':>10}{'min':>10}{'max':>10}{'spread':>8}{'ns/elem':>10}{'GB/s':>9}")
    for name, r in rows.items():
        lines.append(f"{name:<22}{r['batch']:>6}{r['ms']:>10.4f}{r['ms_min']:>10.4f}{r['ms_max']:>10.4f}"
                     f"{(r['ms_max'] - r['ms_min']) / r['ms']:>8.1%}{r['ms'] * 1e6 / r['elements']:>10.4f}"
                     + ("" if name == "torch_chain" else f"{r['elements'] * BYTES / r['ms'] / 1e6:>9.0f}"))
    lines.append("")
    if "preemphasis" in rows:
        lines.append("bandwidth against preemphasis's (same bytes per element; preemphasis is a public call, whose output the")
        lines.append("allocator recycles, as pcen's is; pcen_kernel writes three rotating outputs):")
        for k in ("pcen", "pcen_kernel"):
            if k in rows:
                lines.append(f"  {k} {rows['preemphasis']['ms'] / rows[k]['ms']:.2f}")
    if "pcen" in rows and "torch_chain" in rows:
        lines.append(f"torch_chain / pcen = {rows['torch_chain']['ms'] / rows['pcen']['ms']:.2f} (the chain alone, no smoother)")
    return "\n".join(lines) + "\n"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--samples", type=int, default=220500)
    p.add_argument("--ramp", type=float, default=0.5)
    p.add_argument("--only", choices=list(STEPS))
    p.add_argument("--skip", choices=list(STEPS), action="append", default=[])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcen_timings.txt"))
    a = p.parse_args()
    if a.only:
        print(json.dumps(run_step(a.only, a)))
        return 0
    rows = {}
    for name, limit in STEPS.items():
        if name in a.skip:
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--only", name,
               "--batch", str(a.batch), "--samples", str(a.samples), "--ramp", str(a.ramp)]
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
