"""Rational polyphase resampling of continuous recordings (eegnet_resample, one workgroup per row and chunk of
outputs) against its two floors -- the memory floor and the band-pass that follows it -- and against the host.
Writes profiles/resample_bench.json.

    python tools/bench_resample.py [--reps 5] [--window-ms 100] [--out profiles/resample_bench.json]

Shapes: 22 rows x 150,000 samples (ten minutes at 250 Hz), 22 x 672,000 (a whole BCI IV-2a session file at 250 Hz)
and 18 x 22 x 672,000 (all of them), float32 input, 250 -> 128 Hz (64/125), the default 2501-tap Kaiser design.
Timed alternately in one process after warming up every leg:
    (a) resample into a preallocated output, device taps
    (b) y.copy_(x) on the input: one read and one write of the recording at 250 Hz, the memory floor
    (c) bandpass_filter (eegnet_fir, the 213-tap design) of the resampled recording: the step behind it
Device events around windows of repeated calls (as many calls as fill --window-ms), median and min-max over
--reps windows, in ms per call.  One row is also resampled on the host in float64 (scipy.signal.resample_poly,
when scipy is there) and the time scaled to the shape's rows; at 22 x 150,000 the GPU result is checked against
the oracle on three rows.  Needs a HIP device: there is no fallback."""

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

from eegnetreplication_amd import bandpass_filter, design_bandpass, design_resampler, ops, resample  # noqa: E402

SHAPES = ((1, 22, 150000), (1, 22, 672000), (18, 22, 672000))
UP, DOWN = 64, 125


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


def run_shape(shape, taps_np, bp_np, reps, window_ms, dev):
    R, C, N = shape
    L = len(taps_np)
    K = -(-L // UP)
    torch.manual_seed(2)
    x = torch.randn(shape, device=dev) * 7.0 + 40.0
    xc = torch.empty_like(x)
    taps, bp = torch.from_numpy(taps_np).to(dev), torch.from_numpy(bp_np).to(dev)
    y = resample(x, UP, DOWN, taps)
    z = torch.empty_like(y)
    legs = {
        "a_resample": lambda: resample(x, UP, DOWN, taps, out=y),
        "b_copy": lambda: xc.copy_(x),
        "c_fir": lambda: bandpass_filter(y, bp, out=z),
    }
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
    in_bytes, out_bytes = x.numel() * 4, y.numel() * 4
    a_ms, b_ms, c_ms = (s[k]["median_ms"] for k in ("a_resample", "b_copy", "c_fir"))
    flop = 2.0 * K * y.numel()
    ch = ops.resample_chunk(L, UP, DOWN)
    res = {"rows": R * C, "n_samples": N, "n_out": int(y.shape[-1]), "n_taps": L, "terms_per_output": K,
           "chunk_outputs": ch, "chunks_per_row": (int(y.shape[-1]) - 1) // ch + 1,
           "input_bytes": in_bytes, "output_bytes": out_bytes, "calls_per_window": calls, **s,
           "a_over_b": round(a_ms / b_ms, 3), "a_over_c": round(a_ms / c_ms, 3),
           "nearer_floor": "b_copy" if abs(math.log(a_ms / b_ms)) < abs(math.log(a_ms / c_ms)) else "c_fir",
           "input_samples_per_s_a": int(x.numel() / (a_ms * 1e-3)),
           # what the launch moves (x read once plus the chunks' halos, y written once) and what it computes
           "gb_per_s_a": round((in_bytes + out_bytes) / (a_ms * 1e-3) / 1e9, 1),
           "gb_per_s_b": round(2 * in_bytes / (b_ms * 1e-3) / 1e9, 1),
           "fp64_gflop": round(flop / 1e9, 2),
           "fp64_tflops_a": round(flop / (a_ms * 1e-3) / 1e12, 2)}
    try:                                                          # the float64 host resampling of one row, for scale
        from scipy.signal import resample_poly
        row = x[0, 0].double().cpu().numpy()
        t0 = time.perf_counter()
        resample_poly(row, UP, DOWN)
        one = time.perf_counter() - t0
        res["host_resample_poly_one_row_s"] = round(one, 4)
        res["host_resample_poly_all_rows_s"] = round(one * R * C, 2)
        res["host_over_a"] = round(one * R * C * 1e3 / a_ms, 1)
    except ImportError:
        res["host_resample_poly_one_row_s"] = None
    if shape == SHAPES[0]:
        from resample_cases import assert_resample_close, oracle_resample
        xn = x[0, :3].cpu().numpy()
        ref = oracle_resample(xn, taps_np, UP, DOWN, "reflect_limited")
        got = resample(x[0, :3], UP, DOWN, taps).cpu().numpy()
        assert_resample_close(got, ref, xn, taps_np, UP, DOWN, "reflect_limited", name="bench_resample 22 x 150,000, three rows")
        res["max_abs_err_vs_oracle"] = float(np.abs(got - ref).max())
        res["within_tolerance"] = True
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample needs a HIP device")
    dev = torch.device("cuda:0")
    taps, bp = design_resampler(UP, DOWN), design_bandpass()
    out = {"tool": "bench_resample", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "design": "one launch: k_resample, a workgroup per (row, chunk of outputs), the zero-padded prototype as the "
                     "phase table and the chunk's input span staged in LDS as fp64, 4 outputs per thread 256 apart "
                     "(one phase), one fp64 FMA per term and output",
           "ratio": f"{UP}/{DOWN}", "n_taps": len(taps), "ends": "reflect_limited",
           "timing": "device events around windows of repeated calls, the legs alternating; median and min-max over "
                     "the windows of a leg, ms per call",
           "windows_per_leg": args.reps, "window_ms": args.window_ms,
           "configs": [run_shape(s, taps, bp, args.reps, args.window_ms, dev) for s in SHAPES]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
