"""Zero-phase FIR band-pass of continuous recordings (eegnet_fir, one workgroup per row and chunk) against its
two bounds -- the memory floor and the fp64 rate -- and against the step behind it.  Writes
profiles/fir_bench.json.

    python tools/bench_fir.py [--reps 5] [--window-ms 100] [--out profiles/fir_bench.json]

Shapes: 22 rows x 76,800 samples (ten minutes at 128 Hz), 22 x 345,600 (a whole BCI IV-2a session file) and
18 x 22 x 345,600 (all of them), float32 input, the 213-tap 4-38 Hz design at 128 Hz.  Timed alternately in one
process after warming up every leg:
    (a) bandpass_filter into a preallocated output, device taps
    (b) y.copy_(x) on the same tensors: one read and one write of the recording, the memory floor
    (c) exponential_moving_standardize of the same recording into the same output (eegnet_ems)
    (d) 22 x 345,600 only: the chain filter -> standardise in place -> epoch_logits for 288 cues
        (EEGNet-8,2 at 22 x 257, the reference's epochs)
Device events around windows of repeated calls (as many calls as fill --window-ms), median and min-max over
--reps windows, in ms per call.  One row is also convolved on the host in float64 (np.convolve, the oracle's
sum) and the time scaled to the shape's rows; at 22 x 76,800 the GPU result is checked against the oracle on
three rows.  Needs a HIP device: there is no fallback."""

from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from eegnetreplication_amd import (EEGNet, bandpass_filter, design_bandpass, epoch_logits, epoch_starts,  # noqa: E402
                                   exponential_moving_standardize, ops)

SHAPES = ((1, 22, 76800), (1, 22, 345600), (18, 22, 345600))
N_CUES = 288


def event_window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls                              # ms per call


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 5), "min_ms": round(min(xs), 5), "max_ms": round(max(xs), 5)}


def run_shape(shape, taps_np, reps, window_ms, dev):
    R, C, N = shape
    L = len(taps_np)
    torch.manual_seed(2)
    x = torch.randn(shape, device=dev) * 7.0 + 40.0
    y = torch.empty_like(x)
    taps = torch.from_numpy(taps_np).to(dev)
    legs = {
        "a_fir": lambda: bandpass_filter(x, taps, out=y),
        "b_copy": lambda: y.copy_(x),
        "c_ems": lambda: exponential_moving_standardize(x, out=y),
    }
    if shape == SHAPES[1]:
        model = EEGNet(C, 257).to(dev).eval()
        onsets = torch.linspace(0, N - 257 - 64 - 1, N_CUES).long()
        starts = epoch_starts(onsets).to(dev)
        z = torch.empty_like(x[0])

        def chain():
            bandpass_filter(x[0], taps, out=z)
            exponential_moving_standardize(z, out=z)
            return epoch_logits(model, z, starts)

        legs["d_chain_288_cues"] = chain
    for fn in legs.values():                                      # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    calls = {k: max(5, min(2000, math.ceil(window_ms / max(event_window(fn, 3), 1e-4)))) for k, fn in legs.items()}
    t = {k: [] for k in legs}
    for _ in range(reps):                                         # the legs alternate
        for k, fn in legs.items():
            t[k].append(event_window(fn, calls[k]))
    s = {k: stats(v) for k, v in t.items()}
    nbytes = x.numel() * 4
    a_ms = s["a_fir"]["median_ms"]
    flop = 2.0 * L * x.numel()
    res = {"rows": R * C, "n_samples": N, "n_taps": L, "chunks_per_row": (N - 1) // ops.fir_chunk() + 1,
           "recording_bytes": nbytes, "calls_per_window": calls, **s,
           "a_over_b": round(a_ms / s["b_copy"]["median_ms"], 3),
           "a_over_c": round(a_ms / s["c_ems"]["median_ms"], 3),
           "samples_per_s_a": int(x.numel() / (a_ms * 1e-3)),
           # what the launch moves (x read once plus the chunks' halos, y written once) and what it computes
           "gb_per_s_a": round(2 * nbytes / (a_ms * 1e-3) / 1e9, 1),
           "gb_per_s_b": round(2 * nbytes / (s["b_copy"]["median_ms"] * 1e-3) / 1e9, 1),
           "fp64_gflop": round(flop / 1e9, 2),
           "fp64_tflops_a": round(flop / (a_ms * 1e-3) / 1e12, 2)}
    # the float64 host convolution of one row, scaled to the shape's rows
    from fir_cases import assert_fir_close, extend, oracle_fir
    row = x[0, :1].cpu().numpy()
    u = extend(row, L)[0]
    t0 = time.perf_counter()
    np.convolve(u, taps_np, "valid")
    one = time.perf_counter() - t0
    res["host_convolve_one_row_s"] = round(one, 4)
    res["host_convolve_all_rows_s"] = round(one * R * C, 2)
    res["host_over_a"] = round(one * R * C * 1e3 / a_ms, 1)
    if shape == SHAPES[0]:
        xn = x[0, :3].cpu().numpy()
        ref = oracle_fir(xn, taps_np)
        got = bandpass_filter(x[0, :3], taps).cpu().numpy()
        assert_fir_close(got, ref, xn, taps_np, name="bench_fir 22 x 76,800, three rows")
        res["max_abs_err_vs_oracle"] = float(np.abs(got - ref).max())
        res["within_tolerance"] = True
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fir_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fir needs a HIP device")
    dev = torch.device("cuda:0")
    taps = design_bandpass()
    out = {"tool": "bench_fir", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "design": "one launch: k_fir, a workgroup per (row, chunk), the chunk and its halo staged in LDS as fp64, "
                     "8 outputs per thread over a sliding register window, one fp64 FMA per tap and output",
           "chunk": ops.fir_chunk(), "n_taps": len(taps),
           "timing": "device events around windows of repeated calls, 5 windows per leg, the legs alternating; "
                     "ms per call",
           "configs": [run_shape(s, taps, args.reps, args.window_ms, dev) for s in SHAPES]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
