"""Time partial fine-tuning: the frozen-BatchNorm step that trains a suffix of the layers
(eegnet_frozen_step_from / eegnet_frozen_step_folds_from) against the full frozen step, in one process.

Single model, 22 x 256 and 22 x 257 at B = 64 and B = 4096, per iteration with the fused Adam and
device-generated masks:
    full          ops.frozen_step, every layer trained (train_from = 0: the code path before the stages)
    aggregation / block_2 / classifier
                  the same call with train_from set: the backward stops at the frozen prefix
    forward       ops.forward_frozen, the forward alone: the floor of every stage
Device events around `inner` back-to-back iterations, inputs rotated over several buffers, the legs
alternating window by window after a warm-up of each, the median over the windows with min / max.

Folds, 90 models x 864 trials of 22 x 257 at batch 64 (FrozenFoldBatch, fused launches, captured graphs
replayed): the full step against block_2 and classifier, a host clock around windows of whole epochs that
end in a device synchronise, the legs alternating.

Every cut stage is compared with the full step of the same run, never with another stage.  The gate: at
B = 4096 and in the 90-fold epoch a cut stage is not slower than the full step beyond the min-max spread
recorded for the full step in that run; the exit status is 1 when one is.  B = 64 is recorded, not gated:
three launches' fixed cost dominates there.  Needs a HIP device; there is no CPU path.

    python tools/bench_partial_finetune.py [--repeats 15] [--out profiles/partial_finetune_bench.json]
"""

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

from eegnetreplication_amd import EEGNet, FrozenFoldBatch, ops  # noqa: E402

NBUF = 4
CUT = ("aggregation", "block_2", "classifier")
FOLDS, N_TRIALS, BATCH_SIZE, P_FOLDS = 90, 864, 64, 0.25
FOLD_WARMUP = 4           # the eager epoch (graph capture at its end) and three replays


def new_model(dev, C, T, p=0.5):
    torch.manual_seed(0)
    model = EEGNet(C, T, p=p)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                      # BN off identity, as a trained model's is
        for bn in model._bns():
            bn.weight.copy_(0.5 + torch.rand(bn.weight.shape, generator=g))
            bn.bias.copy_(0.2 * torch.randn(bn.bias.shape, generator=g))
            bn.running_mean.copy_(0.1 * torch.randn(bn.running_mean.shape, generator=g))
            bn.running_var.copy_(0.3 + torch.rand(bn.running_var.shape, generator=g))
    return model.to(dev).train()


def stats(ms, n=5):
    return {"median_ms": round(statistics.median(ms), n), "min_ms": round(min(ms), n), "max_ms": round(max(ms), n)}


def bench_single(dev, B, C, T, warmup, repeats):
    gen = lambda s: torch.Generator(device=dev).manual_seed(s)
    xs = [torch.randn((B, C, T), device=dev, generator=gen(10 + i)) for i in range(NBUF)]
    y = torch.randint(0, 4, (B,), device=dev, generator=gen(5))
    inner = 100 if B <= 256 else 20
    legs, checks = {}, []

    def step_leg(stage):
        m = new_model(dev, C, T)
        shape, flat, bnf = m.shape, m.flat_parameters(), m.flat_bn_buffers()
        n = flat.numel()
        grads, adam = torch.zeros(n, device=dev), torch.zeros(2 * n, device=dev)
        step, loss = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, device=dev)
        ws = ops.new_frozen_workspace(shape, B, dev)
        checks.append((flat, step))
        return lambda x: ops.frozen_step(shape, flat, bnf, x, 7, 0, grads, ws, labels=y, adam_state=adam,
                                         step_i32=step, loss=loss, key_from_step=True, train_from=stage)

    legs["full"] = step_leg(0)
    for s in CUT:
        legs[s] = step_leg(s)
    mf = new_model(dev, C, T)
    legs["forward"] = lambda x: ops.forward_frozen(mf.shape, mf.flat_parameters(), mf.flat_bn_buffers(), x, 7, 0)

    k = 0
    for fn in legs.values():
        for _ in range(warmup):
            fn(xs[k % NBUF])
            k += 1
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn(xs[k % NBUF])
                k += 1
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / inner)
    torch.cuda.synchronize()
    for flat, step in checks:
        if not bool(torch.isfinite(flat).all()) or int(step.item()) <= 0:
            raise SystemExit(f"{C}x{T} B={B}: a timed step left non-finite parameters")
    res = {"C": C, "T": T, "B": B, "inner": inner, "windows": repeats}
    for name in legs:
        res[name] = stats(ms[name])
    full, floor = res["full"], res["forward"]["median_ms"]
    spread = full["max_ms"] - full["min_ms"]
    res["full_spread_ms"] = round(spread, 5)
    res["full_over_forward"] = round(full["median_ms"] / floor, 3)
    for s in CUT:
        res[s]["over_full"] = round(res[s]["median_ms"] / full["median_ms"], 3)
        res[s]["over_forward"] = round(res[s]["median_ms"] / floor, 3)
        res[s]["not_slower_than_full"] = bool(res[s]["median_ms"] <= full["median_ms"] + spread)
    print(json.dumps(res), flush=True)
    return res


def window(fn, epochs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / epochs * 1e3          # ms per epoch


def bench_folds(dev, K, reps, window_s):
    C, T = 22, 257
    torch.manual_seed(1)
    base = [EEGNet(C, T, p=P_FOLDS).freeze_bn() for _ in range(K)]
    seeds = list(range(100, 100 + K))
    sets = [(torch.randn((N_TRIALS, C, T), device=dev), torch.randint(0, 4, (N_TRIALS,), device=dev, dtype=torch.int64))
            for _ in range(K)]
    legs = {}
    for name in ("full", "block_2", "classifier"):
        models = [copy.deepcopy(m).to(dev).train_from("temporal" if name == "full" else name).train() for m in base]
        legs[name] = {"models": models, "fb": FrozenFoldBatch(models, seeds, graphs=True, fused=True),
                      "gens": [torch.Generator().manual_seed(s) for s in seeds], "t": []}

    def epoch(leg):
        leg["fb"].epoch(sets, BATCH_SIZE, leg["gens"])

    for leg in legs.values():
        for _ in range(FOLD_WARMUP):
            epoch(leg)
    torch.cuda.synchronize()
    probe = max(window(lambda leg=leg: epoch(leg), 3) for leg in legs.values())
    epochs = max(5, math.ceil(window_s * 1e3 / probe))
    for _ in range(reps):
        for leg in legs.values():
            leg["t"].append(window(lambda leg=leg: epoch(leg), epochs))
    for name, leg in legs.items():
        if not all(bool(torch.isfinite(m.flat_parameters()).all()) for m in leg["models"]):
            raise SystemExit(f"folds, {name}: a timed epoch left non-finite parameters")
    steps = (N_TRIALS + BATCH_SIZE - 1) // BATCH_SIZE
    res = {"folds": K, "C": C, "T": T, "batch": BATCH_SIZE, "p": P_FOLDS, "trials_per_fold": N_TRIALS,
           "steps_per_epoch": steps, "epochs_per_window": epochs, "windows": reps}
    for name, leg in legs.items():
        res[name] = stats(leg["t"], 4)
        res[name]["trials_per_s"] = int(K * N_TRIALS / (res[name]["median_ms"] * 1e-3))
    full = res["full"]
    spread = full["max_ms"] - full["min_ms"]
    res["full_spread_ms"] = round(spread, 4)
    for s in ("block_2", "classifier"):
        res[s]["over_full"] = round(res[s]["median_ms"] / full["median_ms"], 3)
        res[s]["not_slower_than_full"] = bool(res[s]["median_ms"] <= full["median_ms"] + spread)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=15, help="windows per leg of the single-model legs")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--fold-reps", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.3, help="seconds of epochs per window of the fold legs")
    ap.add_argument("--folds", type=int, default=FOLDS, help="0 skips the fold legs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partial_finetune_bench.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        raise SystemExit("--repeats must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this benchmark runs on the GPU only")
    dev = torch.device("cuda", 0)
    res = {"tool": "bench_partial_finetune", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
           "timing": f"single: device events, median of {args.repeats} windows per leg, legs alternating, {NBUF} rotated "
                     f"input buffers; folds: host clock around windows of about {args.window_s} s of graph-replayed "
                     f"epochs ending in a device synchronise, {args.fold_reps} windows per leg, legs alternating",
           "single": [bench_single(dev, B, 22, T, args.warmup, args.repeats) for B in (64, 4096) for T in (256, 257)]}
    gated = [s[c]["not_slower_than_full"] for s in res["single"] if s["B"] == 4096 for c in CUT]
    if args.folds:
        res["folds"] = bench_folds(dev, args.folds, args.fold_reps, args.window_s)
        gated += [res["folds"][c]["not_slower_than_full"] for c in ("block_2", "classifier")]
    res["gate_cut_stages_not_slower_than_full"] = all(gated)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print("wrote", args.out)
    return 0 if res["gate_cut_stages_not_slower_than_full"] else 1


if __name__ == "__main__":
    sys.exit(main())
