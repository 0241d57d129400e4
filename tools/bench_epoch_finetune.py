"""Frozen-BatchNorm fine-tuning on the cue epochs of a continuous recording: the gather a caller had to make
before (the epochs cut out once into [N, C, T], every shuffled batch gathered out of that, ops.frozen_step)
against ops.frozen_step_windows reading the recording in place.  Writes profiles/epoch_finetune_bench.json.

    python tools/bench_epoch_finetune.py [--reps 5] [--window-ms 100] [--out profiles/epoch_finetune_bench.json]

Inputs: EEGNet-8,2 at 22 x 256 and 22 x 257 with p = 0.25, one session of 22 x 345,600 samples (45 min at
128 Hz) with 288 cues at random starts, batches of B = 64 and B = 288 drawn as a slice of one permutation,
train_from 0 (everything trains) and "block_2".  Timed alternately in one process after warming up every leg:
    (a) x_all[sel], y_all[sel] gathered into contiguous tensors, then ops.frozen_step
    (b) ops.frozen_step_windows with sel on the recording
    (c) ops.frozen_step alone on an already gathered batch: the kernel floor, what (b) would cost if the
        windowed loader were free
Every leg runs the whole step (k_frozen, the reduction, Adam) at lr = 0, so the parameters stay where they
are over the thousands of timed calls and every call does the same work.  Also one whole epoch of
finetune_on_recording at batch 64 (5 steps, the last one of 32) against the same loop over gathered batches
through FusedTrainer.step.  Device events around windows of repeated calls (as many calls as fill
--window-ms, measured once per config), median and min-max over --reps windows, in ms per call.  Also a check
that (a) and (b) give the same bits on the timed inputs.  Needs a HIP device: there is no fallback."""

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

from eegnetreplication_amd import EEGNet, FusedTrainer, finetune_on_recording, ops  # noqa: E402
from eegnetreplication_amd.model import batch_slices  # noqa: E402

C = 22
N_SAMPLES = 345600
N_CUES = 288
P_DROP = 0.25
SHAPES = (256, 257)
BATCHES = (64, 288)
STAGES = (0, "block_2")


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


def time_legs(legs, reps, window_ms, warm=3):
    for fn in legs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    calls = {k: max(5, min(2000, math.ceil(window_ms / max(event_window(fn, 3), 1e-4)))) for k, fn in legs.items()}
    t = {k: [] for k in legs}
    for _ in range(reps):                                         # the legs alternate
        for k, fn in legs.items():
            t[k].append(event_window(fn, calls[k]))
    return calls, {k: stats(v) for k, v in t.items()}


def session(T, dev):
    g = torch.Generator().manual_seed(2)
    rec = torch.randn((C, N_SAMPLES), generator=g).to(dev)
    starts = torch.randint(0, N_SAMPLES - T + 1, (N_CUES,), generator=g).sort().values.to(dev)
    labels = torch.randint(0, 4, (N_CUES,), generator=g).to(dev)
    x_all = torch.stack([rec[:, s:s + T] for s in starts.tolist()]).contiguous()
    return rec, starts, labels, x_all


def spread(s):
    return s["max_ms"] - s["min_ms"]


def run_config(T, B, stage, reps, window_ms, dev):
    torch.manual_seed(1)
    model = EEGNet(C, T, p=P_DROP).to(dev).train()
    shape, flat, bn = model.shape, model.flat_parameters().detach().clone(), model.flat_bn_buffers()
    rec, starts, labels, x_all = session(T, dev)
    sel = torch.randperm(N_CUES, generator=torch.Generator().manual_seed(3))[:B].to(dev)
    x_pre, y_pre = x_all[sel].contiguous(), labels[sel].contiguous()
    n = flat.numel()
    ws = ops.new_frozen_workspace(shape, B, dev)

    def state():
        return dict(adam_state=torch.zeros(2 * n, device=dev), step_i32=torch.zeros(1, dtype=torch.int32, device=dev),
                    loss=torch.zeros(1, device=dev), logits=torch.zeros((B, 4), device=dev), lr=0.0, train_from=stage)

    sa, sb, sc = state(), state(), state()
    ga, gb, gc = (torch.zeros(n, device=dev) for _ in range(3))
    legs = {
        "a_gather_frozen_step": lambda: ops.frozen_step(shape, flat, bn, x_all[sel], 7, 1, ga, ws, labels=labels[sel], **sa),
        "b_frozen_step_windows": lambda: ops.frozen_step_windows(shape, flat, bn, rec, starts, labels, 7, 1, gb, ws,
                                                                 sel=sel, **sb),
        "c_frozen_step_only": lambda: ops.frozen_step(shape, flat, bn, x_pre, 7, 1, gc, ws, labels=y_pre, **sc),
    }
    legs["a_gather_frozen_step"]()                                # one call each from the same state: the same bits
    legs["b_frozen_step_windows"]()
    torch.cuda.synchronize()
    bit_equal = bool(torch.equal(ga, gb) and torch.equal(sa["loss"], sb["loss"]) and
                     torch.equal(sa["logits"], sb["logits"]) and torch.equal(sa["adam_state"], sb["adam_state"]))
    calls, s = time_legs(legs, reps, window_ms)
    a, b, c = (s[k] for k in legs)
    res = {"C": C, "T": T, "B": B, "train_from": stage, "calls_per_window": calls, **s,
           "b_over_a": round(b["median_ms"] / a["median_ms"], 4),
           "b_over_c": round(b["median_ms"] / c["median_ms"], 4),
           "a_over_c": round(a["median_ms"] / c["median_ms"], 4),
           "windows_per_s_b": int(B / (b["median_ms"] * 1e-3)),
           "outputs_bit_equal": bit_equal,
           "b_not_slower_than_a": bool(b["median_ms"] <= a["median_ms"]),
           "b_within_spread_of_c": bool(abs(b["median_ms"] - c["median_ms"]) <= max(spread(b), spread(c)))}
    print(json.dumps(res), flush=True)
    return res


def run_epoch(T, reps, window_ms, dev, batch=64):
    rec, starts, labels, x_all = session(T, dev)
    torch.manual_seed(1)
    ma = EEGNet(C, T, p=P_DROP).to(dev).freeze_bn().train()
    mb = EEGNet(C, T, p=P_DROP).to(dev).freeze_bn().train()
    ta, tb = FusedTrainer(ma, lr=0.0), FusedTrainer(mb, lr=0.0)
    gen_a, gen_b = torch.Generator(device=dev).manual_seed(4), torch.Generator(device=dev).manual_seed(4)
    slices = batch_slices(N_CUES, batch)
    losses_b = torch.zeros((1, len(slices)), device=dev)

    def gather_loop():
        perm = torch.randperm(N_CUES, device=dev, generator=gen_b)
        for k, (i, j) in enumerate(slices):
            s = perm[i:j]
            losses_b[0, k:k + 1].copy_(tb.step(x_all[s], labels[s]))

    legs = {
        "gather_loop_epoch": gather_loop,
        "finetune_on_recording_epoch": lambda: finetune_on_recording(ma, rec, starts, labels, epochs=1, batch_size=batch,
                                                                     trainer=ta, generator=gen_a),
    }
    calls, s = time_legs(legs, reps, window_ms, warm=2)
    g, f = (s[k] for k in legs)
    res = {"C": C, "T": T, "cues": N_CUES, "batch": batch, "steps": len(slices), "calls_per_window": calls, **s,
           "finetune_over_gather": round(f["median_ms"] / g["median_ms"], 4),
           "finetune_not_slower": bool(f["median_ms"] <= g["median_ms"])}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epoch_finetune_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_epoch_finetune needs a HIP device (there is no fallback)")
    if args.reps < 5 or args.window_ms < 100:
        print("note: fewer than 5 windows of 100 ms: not a measurement to quote", flush=True)
    dev = torch.device("cuda:0")
    out = {"tool": "bench_epoch_finetune", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "timing": f"device events around windows of repeated calls (about {args.window_ms:g} ms each), "
                     f"{args.reps} windows per leg, the legs alternating; ms per call (per epoch for the epochs)",
           "session": {"C": C, "n_samples": N_SAMPLES, "cues": N_CUES, "p_drop": P_DROP},
           "configs": [], "epochs": []}
    for T in SHAPES:
        for B in BATCHES:
            for stage in STAGES:
                out["configs"].append(run_config(T, B, stage, args.reps, args.window_ms, dev))
                torch.cuda.empty_cache()
    for T in SHAPES:
        out["epochs"].append(run_epoch(T, args.reps, args.window_ms, dev))
        torch.cuda.empty_cache()
    out["outputs_bit_equal"] = bool(all(c["outputs_bit_equal"] for c in out["configs"]))
    out["b_not_slower_than_a_everywhere"] = bool(all(c["b_not_slower_than_a"] for c in out["configs"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print("wrote", args.out, "bit-equal =", out["outputs_bit_equal"], "(b) <= (a) everywhere =",
          out["b_not_slower_than_a_everywhere"])


if __name__ == "__main__":
    main()
