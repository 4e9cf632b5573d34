"""StreamingISTFT timings.

  python tools/time_istft_stream.py calls
      (a) ms per process() call (device events, median of 5 runs of 64 calls after a 1 s ramp) for 256 streams:
          n_fft 512 / hop 128 with 8 frames per call and n_fft 2048 / hop 512 with 16 frames per call.
  python tools/time_istft_stream.py trace OUT_DIR
      the workload of (b) / (c), meant to run under its own `rocprofv3 --kernel-trace --stats -d OUT_DIR -- ...`:
      for both shapes, 200 process() calls of 64 frames on 256 streams, then 200 offline istft calls of the same
      64 frames; writes OUT_DIR/istft_stream_calls.json with the call counts.
  python tools/time_istft_stream.py report OUT_DIR
      (b) kernel time per frame, streaming against offline, and (c) launches per process() call, out of the trace.
"""
import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(512, 128, 8), (2048, 512, 16)]        # n_fft, hop, frames per call of (a)
B = 256
TRACE_FRAMES, TRACE_CALLS = 64, 200


def _spectra(n_fft, T, count):
    import torch

    g = torch.Generator(device="cuda").manual_seed(n_fft)
    F = n_fft // 2 + 1
    return [torch.complex(torch.randn((B, F, T), device="cuda", generator=g),
                          torch.randn((B, F, T), device="cuda", generator=g)) for _ in range(count)]


def calls():
    import torch
    import mlx_audio_primitives_amd as ap

    for n_fft, hop, T in SHAPES:
        Ss = _spectra(n_fft, T, 4)
        st = ap.StreamingISTFT(n_fft=n_fft, hop_length=hop)
        i, t0 = 0, time.time()
        while time.time() - t0 < 1.0:
            for _ in range(16):
                st.process(Ss[i % 4]); i += 1
            torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(64):
                st.process(Ss[i % 4]); i += 1
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 64)
        ts.sort()
        print(f"calls n_fft {n_fft} hop {hop}: {B} streams x {T} frames per call: {ts[2] * 1e3:.1f} us per "
              f"process() call (min {ts[0] * 1e3:.1f}), {ts[2] * 1e6 / (B * T):.2f} ns per frame")


def trace(out_dir):
    import torch
    import mlx_audio_primitives_amd as ap

    counts = {}
    for n_fft, hop, _ in SHAPES:
        Ss = _spectra(n_fft, TRACE_FRAMES, 4)
        st = ap.StreamingISTFT(n_fft=n_fft, hop_length=hop)
        for i in range(TRACE_CALLS):
            st.process(Ss[i % 4])
        torch.cuda.synchronize()
        for i in range(TRACE_CALLS):
            ap.istft(Ss[i % 4], hop_length=hop, n_fft=n_fft, center=False)
        torch.cuda.synchronize()
        counts[str(n_fft)] = {"hop": hop, "process_calls": TRACE_CALLS, "istft_calls": TRACE_CALLS,
                              "frames_per_call": B * TRACE_FRAMES}
    os.makedirs(out_dir, exist_ok=True)
    json.dump(counts, open(os.path.join(out_dir, "istft_stream_calls.json"), "w"), indent=1)


def report(out_dir):
    counts = json.load(open(glob.glob(os.path.join(out_dir, "**", "istft_stream_calls.json"), recursive=True)[0]))
    rows = list(csv.DictReader(open(glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)[0])))
    for key, c in counts.items():
        n_fft = int(key)
        stream = [r for r in rows if "ap_istft_stream_kernel<" + key + ">" in r["Kernel_Name"]
                  or f"ap_istft_stream_kernelILi{key}E" in r["Kernel_Name"]]
        dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        # the offline calls come after the stream calls of the same shape: the istft kernels between this shape's
        # last stream launch and the next shape's first
        t_end = max(int(r["End_Timestamp"]) for r in stream)
        later = [int(r["Start_Timestamp"]) for r in rows if "ap_istft_stream" in r["Kernel_Name"]
                 and int(r["Start_Timestamp"]) > t_end]
        t_stop = min(later) if later else float("inf")
        offline = [r for r in rows if "istft" in r["Kernel_Name"] and "stream" not in r["Kernel_Name"]
                   and t_end < int(r["Start_Timestamp"]) < t_stop]
        s_ns = sorted(dur(r) for r in stream)
        o_ns = sorted(dur(r) for r in offline)
        frames = c["frames_per_call"]
        s_med, o_med = s_ns[len(s_ns) // 2], o_ns[len(o_ns) // 2]
        print(f"n_fft {n_fft} hop {c['hop']}: {B} streams x {TRACE_FRAMES} frames per call")
        print(f"  (c) launches per process() call: {len(stream) / c['process_calls']:.2f} "
              f"({len(stream)} ap_istft_stream_kernel launches for {c['process_calls']} calls)")
        print(f"  (b) streaming kernel {s_med / 1e3:.1f} us per call = {s_med / frames:.2f} ns per frame; "
              f"offline istft kernel {o_med / 1e3:.1f} us = {o_med / frames:.2f} ns per frame "
              f"({sorted(set(r['Kernel_Name'][:60] for r in offline))}); ratio {s_med / o_med:.2f}")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "calls"
    if mode == "calls":
        calls()
    elif mode == "trace":
        trace(sys.argv[2])
    else:
        report(sys.argv[2])
