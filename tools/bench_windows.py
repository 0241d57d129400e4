"""Sliding-window inference over a continuous recording: the unfolded copy a caller had to make before
(rec.unfold -> contiguous -> ops.forward_eval) against ops.forward_eval_windows reading the recording
in place.  Writes profiles/windows_bench.json.

    python tools/bench_windows.py [--reps 5] [--window-ms 100] [--out profiles/windows_bench.json]

Inputs: EEGNet-8,2 at 22 x 256 and 22 x 257, one recording of 76,800 samples (10 min at 128 Hz), hops 4,
8, 32 and 128.  Timed alternately in one process after warming up every leg:
    (a) rec.unfold(-1, T, hop) made contiguous as [W, C, T], then ops.forward_eval
    (b) ops.forward_eval_windows
    (c) (b) with reduce=True (the second kernel: crop-averaged probabilities and prediction)
    (d) ops.forward_eval alone on the W windows already unfolded (k_infer on as many trials: what (b)
        would cost if the loader were free)
    (e) ops.forward_eval_windows on that unfolded batch taken as W recordings of one window each: (d)'s
        memory layout through (b)'s kernel, which splits (b) - (d) into the kernel's share, (e) - (d),
        and the share of reading 1 KB rows a recording apart, (b) - (e)
Device events around windows of repeated calls (as many calls as fill --window-ms, measured once per
config), median and min-max over --reps windows, in ms per call.  Also the peak extra device memory of
one call of (a) and of (b), and a check that (a) and (b) give the same bits on the timed inputs.  Needs a
HIP device: there is no fallback."""

from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eegnetreplication_amd import EEGNet, ops  # noqa: E402

C = 22
N_SAMPLES = 76800
SHAPES = (256, 257)
HOPS = (4, 8, 32, 128)


def unfolded(rec, T, hop):
    """[C, N] -> the windows as the contiguous [W, C, T] batch forward_eval takes."""
    return rec.unfold(-1, T, hop).permute(1, 0, 2).contiguous()


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


def peak_extra_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def run_config(T, hop, reps, window_ms, dev):
    torch.manual_seed(1)
    model = EEGNet(C, T).to(dev).eval()
    shape, flat, bn = model.shape, model.flat_parameters(), model.flat_bn_buffers()
    rec = torch.randn((C, N_SAMPLES), device=dev)
    W = ops.window_count(shape, N_SAMPLES, hop)
    x_pre = unfolded(rec, T, hop)

    legs = {
        "a_unfold_forward_eval": lambda: ops.forward_eval(shape, flat, bn, unfolded(rec, T, hop)),
        "b_windows": lambda: ops.forward_eval_windows(shape, flat, bn, rec, hop),
        "c_windows_reduce": lambda: ops.forward_eval_windows(shape, flat, bn, rec, hop, reduce=True),
        "d_forward_eval_only": lambda: ops.forward_eval(shape, flat, bn, x_pre),
        "e_windows_on_unfolded": lambda: ops.forward_eval_windows(shape, flat, bn, x_pre, 1),
    }
    for fn in legs.values():                                      # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ref = legs["a_unfold_forward_eval"]()
    bit_equal = bool(torch.equal(ref, legs["b_windows"]()) and torch.equal(ref, legs["e_windows_on_unfolded"]()[:, 0]))
    del ref
    mem_a = peak_extra_bytes(legs["a_unfold_forward_eval"])
    mem_b = peak_extra_bytes(legs["b_windows"])
    calls = {k: max(10, min(2000, math.ceil(window_ms / max(event_window(fn, 5), 1e-4)))) for k, fn in legs.items()}
    t = {k: [] for k in legs}
    for _ in range(reps):                                         # the legs alternate
        for k, fn in legs.items():
            t[k].append(event_window(fn, calls[k]))
    s = {k: stats(v) for k, v in t.items()}
    a, b, c, d, e = (s[k] for k in legs)
    res = {"C": C, "T": T, "n_samples": N_SAMPLES, "hop": hop, "windows": W, "calls_per_window": calls, **s,
           "b_over_a": round(b["median_ms"] / a["median_ms"], 4),
           "c_over_b": round(c["median_ms"] / b["median_ms"], 4),
           "b_over_d": round(b["median_ms"] / d["median_ms"], 4),
           "e_over_d": round(e["median_ms"] / d["median_ms"], 4),
           "windows_per_s_b": int(W / (b["median_ms"] * 1e-3)),
           "trials_per_s_d": int(W / (d["median_ms"] * 1e-3)),
           "peak_extra_bytes_a": mem_a, "peak_extra_bytes_b": mem_b,
           "unfolded_copy_bytes": int(x_pre.numel() * 4), "recording_bytes": int(rec.numel() * 4),
           "logits_bit_equal": bit_equal,
           "b_not_slower_than_a": bool(b["median_ms"] <= a["median_ms"]),
           # (b) against k_infer on as many trials: inside the larger of the two legs' min-max spreads
           "b_within_spread_of_d": bool(abs(b["median_ms"] - d["median_ms"]) <=
                                        max(b["max_ms"] - b["min_ms"], d["max_ms"] - d["min_ms"]))}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_windows needs a HIP device (there is no fallback)")
    if args.reps < 5 or args.window_ms < 100:
        print("note: fewer than 5 windows of 100 ms: not a measurement to quote", flush=True)
    dev = torch.device("cuda:0")
    out = {"tool": "bench_windows", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "timing": f"device events around windows of repeated calls (about {args.window_ms:g} ms each), "
                     f"{args.reps} windows per leg, the legs alternating; ms per call",
           "configs": []}
    for T in SHAPES:
        for hop in HOPS:
            out["configs"].append(run_config(T, hop, args.reps, args.window_ms, dev))
            torch.cuda.empty_cache()
    out["logits_bit_equal"] = bool(all(c["logits_bit_equal"] for c in out["configs"]))
    out["b_not_slower_than_a_everywhere"] = bool(all(c["b_not_slower_than_a"] for c in out["configs"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print("wrote", args.out, "bit-equal =", out["logits_bit_equal"], "(b) <= (a) everywhere =",
          out["b_not_slower_than_a_everywhere"])


if __name__ == "__main__":
    main()
