"""Fine-tuning epochs of K frozen-BatchNorm models at batch 64: the fold-indexed launches
(FrozenFoldBatch, fused: eegnet_frozen_step_folds, four launches per batch for all K models) against the
per-fold path (fused=False: one eegnet_frozen_step per fold and batch on the fold's own stream -- all
there was before the fold-indexed call), both replaying captured hipGraphs.  Writes
profiles/frozen_folds_bench.json.

    python tools/bench_frozen_folds.py [--reps 5] [--window-s 0.3] [--out profiles/frozen_folds_bench.json]

Set-up: 22 x 257, batch 64, p = 0.25, 864 trials per fold (14 steps per epoch), K in {12, 36, 90}.  The two
paths alternate in one process after warm-up epochs (the eager epoch, the capture, replays); a window is a
host clock around as many epochs as span about --window-s seconds, ending in a device synchronise, the
same number of epochs for both paths; median and min-max over --reps windows, and trials/s.  Both paths
train copies of the same models on the same shuffles, so their parameters are compared bit for bit at the
end.  Needs a HIP device: there is no fallback."""

from __future__ import annotations

import argparse
import copy
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eegnetreplication_amd import EEGNet, FrozenFoldBatch  # noqa: E402

BATCH_SIZE = 64
C, T, P_DROP, N_TRIALS = 22, 257, 0.25, 864
FOLDS = (12, 36, 90)
WARMUP = 4            # the eager epoch (graph capture at its end) and three replays


def window(fn, epochs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / epochs * 1e3          # ms per epoch


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def run_folds(K, reps, window_s, dev):
    torch.manual_seed(1)
    base = [EEGNet(C, T, p=P_DROP).freeze_bn() for _ in range(K)]
    seeds = list(range(100, 100 + K))
    sets = [(torch.randn((N_TRIALS, C, T), device=dev), torch.randint(0, 4, (N_TRIALS,), device=dev, dtype=torch.int64))
            for _ in range(K)]
    legs = {}
    for name, fused in (("fused", True), ("per_fold", False)):
        models = [copy.deepcopy(m).to(dev).train() for m in base]
        legs[name] = {"models": models, "fb": FrozenFoldBatch(models, seeds, graphs=True, fused=fused),
                      "gens": [torch.Generator().manual_seed(s) for s in seeds], "t": []}

    def epoch(leg):
        leg["fb"].epoch(sets, BATCH_SIZE, leg["gens"])

    for leg in legs.values():
        for _ in range(WARMUP):
            epoch(leg)
    torch.cuda.synchronize()
    # epochs per window: about window_s seconds of the slower path, the same count for both
    probe = max(window(lambda leg=leg: epoch(leg), 3) for leg in legs.values())
    epochs = max(5, math.ceil(window_s * 1e3 / probe))
    for _ in range(reps):
        for leg in legs.values():
            leg["t"].append(window(lambda leg=leg: epoch(leg), epochs))
    same = all(torch.equal(a.flat_parameters(), b.flat_parameters())
               for a, b in zip(legs["fused"]["models"], legs["per_fold"]["models"]))
    f, p = stats(legs["fused"]["t"]), stats(legs["per_fold"]["t"])
    steps = (N_TRIALS + BATCH_SIZE - 1) // BATCH_SIZE
    res = {"folds": K, "C": C, "T": T, "batch": BATCH_SIZE, "p": P_DROP, "trials_per_fold": N_TRIALS,
           "steps_per_epoch": steps, "epochs_per_window": epochs, "windows": reps,
           "fused": f, "per_fold": p,
           "fused_ms_per_step": round(f["median_ms"] / steps, 4), "per_fold_ms_per_step": round(p["median_ms"] / steps, 4),
           "fused_trials_per_s": int(K * N_TRIALS / (f["median_ms"] * 1e-3)),
           "per_fold_trials_per_s": int(K * N_TRIALS / (p["median_ms"] * 1e-3)),
           "speedup": round(p["median_ms"] / f["median_ms"], 2),
           "fused_no_slower": bool(f["median_ms"] <= p["median_ms"]),
           "parameters_bit_equal": bool(same)}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--folds", type=int, nargs="*", default=list(FOLDS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_folds_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frozen_folds needs a HIP device (there is no fallback)")
    if args.reps < 5 or args.window_s < 0.3:
        print("note: fewer than 5 windows of 0.3 s: not a measurement to quote", flush=True)
    dev = torch.device("cuda:0")
    out = {"tool": "bench_frozen_folds", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "timing": f"host clock around windows of about {args.window_s} s of epochs ending in a device synchronise, "
                     f"{args.reps} windows per path, fused and per-fold alternating, both replaying hipGraphs after "
                     f"{WARMUP} warm-up epochs",
           "fused_min_folds": FrozenFoldBatch.FUSED_MIN_FOLDS, "configs": []}
    for K in args.folds:
        out["configs"].append(run_folds(K, args.reps, args.window_s, dev))
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
