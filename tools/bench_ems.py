"""Exponential moving standardisation of continuous recordings (eegnet_ems, the three-launch blocked scan)
against its memory floor and its consumer.  Writes profiles/ems_bench.json.

    python tools/bench_ems.py [--reps 5] [--window-ms 100] [--out profiles/ems_bench.json]

Shapes: 22 rows x 76,800 samples (ten minutes at 128 Hz, the recording of profiles/windows_bench.json),
22 x 345,600 (a whole BCI IV-2a session file) and 18 x 22 x 345,600 (all of them), float32 input.  Timed
alternately in one process after warming up every leg:
    (a) exponential_moving_standardize into a preallocated output
    (b) the same in place (y is x)
    (c) y.copy_(x) on the same tensors: one read and one write of the recording, the memory floor
    (d) sliding_logits at hop 4 on the standardised recording, the call that consumes it (EEGNet-8,2 at
        22 x 256; first shape only: the others exceed what a user slides over in one call)
Device events around windows of repeated calls (as many calls as fill --window-ms), median and min-max over
--reps windows, in ms per call.  At 22 x 76,800 the serial float64 oracle (tests/ems_cases.oracle_ems, the
reference's loop) is timed once on the CPU and the GPU result is checked against it.  Needs a HIP device:
there is no fallback."""

from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from eegnetreplication_amd import EEGNet, exponential_moving_standardize, ops, sliding_logits  # noqa: E402

SHAPES = ((1, 22, 76800), (1, 22, 345600), (18, 22, 345600))
HOP = 4


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


def run_shape(shape, reps, window_ms, dev):
    R, C, N = shape
    torch.manual_seed(2)
    x = torch.randn(shape, device=dev) * 7.0 + 40.0
    y = torch.empty_like(x)
    z = x.clone()
    legs = {
        "a_ems": lambda: exponential_moving_standardize(x, out=y),
        "b_ems_in_place": lambda: exponential_moving_standardize(z, out=z),
        "c_copy": lambda: y.copy_(x),
    }
    if R == 1:
        model = EEGNet(C, 256).to(dev).eval()
        rec = exponential_moving_standardize(x[0])
        legs["d_sliding_logits_hop4"] = lambda: sliding_logits(model, rec, HOP)
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
    res = {"rows": R * C, "n_samples": N, "chunks_per_row": (N - 1) // ops.ems_chunk() + 1,
           "recording_bytes": nbytes, "calls_per_window": calls, **s,
           "a_over_c": round(s["a_ems"]["median_ms"] / s["c_copy"]["median_ms"], 3),
           "samples_per_s_a": int(x.numel() / (s["a_ems"]["median_ms"] * 1e-3)),
           # what the three launches move: x read by k_ems_agg and k_ems_out, y written once
           "gb_per_s_a": round(3 * nbytes / (s["a_ems"]["median_ms"] * 1e-3) / 1e9, 1),
           "gb_per_s_c": round(2 * nbytes / (s["c_copy"]["median_ms"] * 1e-3) / 1e9, 1)}
    if R == 1:
        res["a_over_d"] = round(s["a_ems"]["median_ms"] / s["d_sliding_logits_hop4"]["median_ms"], 3)
    if shape == SHAPES[0]:
        from ems_cases import ABS_TOL, REL_TOL, oracle_ems
        xn = x[0].cpu().numpy()
        t0 = time.perf_counter()
        ref, _ = oracle_ems(xn)
        res["oracle_cpu_s"] = round(time.perf_counter() - t0, 3)
        err = (exponential_moving_standardize(x[0]).double().cpu() - torch.from_numpy(ref)).abs()
        res["max_abs_err_vs_oracle"] = float(err.max())
        res["within_tolerance"] = bool((err <= REL_TOL * torch.from_numpy(ref).abs() + ABS_TOL).all())
        res["oracle_cpu_over_a"] = round(res["oracle_cpu_s"] * 1e3 / s["a_ems"]["median_ms"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ems_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ems needs a HIP device")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_ems", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "design": "three launches: k_ems_agg (chunk aggregates), k_ems_carry (carries), k_ems_out",
           "chunk": ops.ems_chunk(),
           "timing": "device events around windows of repeated calls, 5 windows per leg, the legs alternating; "
                     "ms per call",
           "configs": [run_shape(s, args.reps, args.window_ms, dev) for s in SHAPES]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
