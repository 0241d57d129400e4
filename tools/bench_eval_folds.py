"""Per-epoch validation of the batch-64 protocols: the per-fold loop train.py's _run_folds ran before
fold-indexed validation (kept here verbatim as the baseline) against one evaluate_folds call, on the
protocols' own sizes.  Writes profiles/eval_folds_bench.json.

    python tools/bench_eval_folds.py [--reps 5] [--epochs 50] [--out profiles/eval_folds_bench.json]

Timed, both ways, alternating in one process after warming up every shape: the validation block alone
and the whole epoch (FoldBatch.epoch + validation), as a host clock around windows of --epochs epochs
that end in a device synchronise; median and min-max over --reps windows.  Also the device-event time of
the two validation kernels (k_eval_folds + k_eval_folds_reduce) with the implied trials/s beside
k_infer's on the same number of trials, and a check of (b)'s loss, correct counts and logits against
(a)'s on the timed inputs.  Needs a HIP device: there is no fallback."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eegnetreplication_amd import EEGNet, FoldBatch, evaluate_folds, ops  # noqa: E402

BATCH_SIZE = 64
C, T = 22, 257
CONFIGS = [  # protocol, folds, validation trials, training trials, dropout p (train.py:50-140, 182-290)
    ("cross-subject", 90, 864, 1440, 0.25),
    ("within-subject", 36, 86, 346, 0.5),
]
LOSS_RTOL = 1e-4


def baseline_groups(val_sets, device):
    """_run_folds' size groups as of the parent commit (train.py lines 95-105)."""
    groups = {}
    for k, (_, yv) in enumerate(val_sets):
        groups.setdefault(len(yv), []).append(k)
    vgroups = []
    for nv, ks in groups.items():
        nb = (nv + BATCH_SIZE - 1) // BATCH_SIZE
        seg = torch.arange(nv, device=device) // BATCH_SIZE
        vgroups.append((ks, nb, seg, torch.bincount(seg, minlength=nb).double(),
                        torch.stack([val_sets[k][1] for k in ks])))
    return vgroups


def baseline_validation(models, val_sets, vgroups, val_loss, val_acc, keep_logits=None):
    """The parent commit's validation block (train.py lines 108-123), verbatim."""
    with torch.no_grad():
        logits = []
        for m, (Xv, _) in zip(models, val_sets):
            m.eval()
            logits.append(m(Xv))                # eval BN: batch-size independent
            m.train()
        for ks, nb, seg, cnt, Y in vgroups:
            L = torch.stack([logits[k] for k in ks])                      # [G, nv, classes]
            ce = F.cross_entropy(L.flatten(0, 1), Y.flatten(), reduction="none").view(Y.shape)
            means = torch.zeros((len(ks), nb), dtype=torch.float64, device=ce.device).index_add_(
                1, seg, ce.double()) / cnt
            vl = means.mean(1)
            va = (L.argmax(2) == Y).sum(1)
            for j, k in enumerate(ks):
                val_loss[k].append(vl[j])
                val_acc[k].append(va[j])
    if keep_logits is not None:
        keep_logits[:] = logits


def window(fn, epochs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / epochs * 1e3          # ms per epoch


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def event_ms(fn, reps=30):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def run_config(name, K, nv, ntr, p, reps, epochs, dev):
    torch.manual_seed(1)
    models = [EEGNet(C, T, p=p).to(dev) for _ in range(K)]
    seeds = list(range(100, 100 + K))
    gens = [torch.Generator().manual_seed(s) for s in seeds]

    def rand_set(n):
        return (torch.randn((n, C, T), device=dev), torch.randint(0, 4, (n,), device=dev, dtype=torch.int64))
    train_sets = [rand_set(ntr) for _ in range(K)]
    val_sets = [rand_set(nv) for _ in range(K)]
    fb = FoldBatch(models, seeds, graphs=True)
    vgroups = baseline_groups(val_sets, dev)
    shape = models[0].shape
    vloss = torch.zeros((2, K), dtype=torch.float64, device=dev)
    vcorr = torch.zeros((2, K), dtype=torch.int64, device=dev)

    def val_a():
        baseline_validation(models, val_sets, vgroups, [[] for _ in range(K)], [[] for _ in range(K)])

    def val_b():
        evaluate_folds(models, val_sets, BATCH_SIZE, out=(vloss[0], vcorr[0]))

    def train():
        fb.epoch(train_sets, BATCH_SIZE, gens)

    # warm-up: the eager epoch, the captured one and a replay; both validations
    for _ in range(3):
        train()
    val_a()
    val_b()
    torch.cuda.synchronize()

    # ---- results of (a) against (b) on the timed inputs ----
    la, ca, logits_a = [[] for _ in range(K)], [[] for _ in range(K)], []
    baseline_validation(models, val_sets, vgroups, la, ca, keep_logits=logits_a)
    val_b()
    # (b)'s logits: the same call with a logits pointer per fold (evaluate_folds itself keeps none)
    logits_b = [torch.empty((nv, 4), dtype=torch.float32, device=dev) for _ in range(K)]
    ents = [dict(params=m.flat_parameters(), bn_buffers=m.flat_bn_buffers(), x=X, labels=None, n=nv,
                 logits=logits_b[k]) for k, (m, (X, _)) in enumerate(zip(models, val_sets))]
    ops.eval_folds(shape, ops.eval_fold_table(ents, dev), K, nv, batch=BATCH_SIZE)
    torch.cuda.synchronize()
    loss_a = torch.stack([v[0] for v in la]).cpu().numpy()
    corr_a = torch.stack([v[0] for v in ca]).cpu().numpy()
    loss_b, corr_b = vloss[0].cpu().numpy(), vcorr[0].cpu().numpy()
    loss_err = float(np.max(np.abs(loss_b - loss_a) / np.maximum(1.0, np.abs(loss_a))))
    check = {"loss_max_rel_err": loss_err, "loss_within_1e-4": bool(loss_err <= LOSS_RTOL),
             "correct_equal": bool(np.array_equal(corr_a, corr_b)),
             "logits_bit_equal": bool(all(torch.equal(a, b) for a, b in zip(logits_a, logits_b)))}

    # ---- host-clock windows, (a) and (b) alternating ----
    t = {"val_a": [], "val_b": [], "epoch_a": [], "epoch_b": []}
    for _ in range(reps):
        t["val_a"].append(window(val_a, epochs))
        t["val_b"].append(window(val_b, epochs))
        t["epoch_a"].append(window(lambda: (train(), val_a()), epochs))
        t["epoch_b"].append(window(lambda: (train(), val_b()), epochs))
    t["train_only"] = [window(train, epochs) for _ in range(reps)]

    # ---- device events: the two validation kernels, and k_infer on as many trials of one model ----
    ces = torch.empty((K, nv), dtype=torch.float32, device=dev)
    preds = torch.empty((K, nv), dtype=torch.int32, device=dev)
    st_table = ops.eval_fold_table(
        [dict(params=m.flat_parameters(), bn_buffers=m.flat_bn_buffers(), x=X, labels=y, n=nv, ce=ces[k],
              pred=preds[k], loss=vloss[1, k:], correct=vcorr[1, k:])
         for k, (m, (X, y)) in enumerate(zip(models, val_sets))], dev)
    kern = event_ms(lambda: ops.eval_folds(shape, st_table, K, nv, batch=BATCH_SIZE))
    Xall = torch.randn((K * nv, C, T), device=dev)
    flat, bn = models[0].flat_parameters(), models[0].flat_bn_buffers()
    ops.forward_eval(shape, flat, bn, Xall)
    infer = event_ms(lambda: ops.forward_eval(shape, flat, bn, Xall))
    kmed, imed = statistics.median(kern), statistics.median(infer)

    a, b = stats(t["val_a"]), stats(t["val_b"])
    ea, eb = stats(t["epoch_a"]), stats(t["epoch_b"])
    spread_a = a["max_ms"] - a["min_ms"]
    res = {"protocol": name, "folds": K, "C": C, "T": T, "val_n": nv, "train_n": ntr, "batch": BATCH_SIZE,
           "validation_baseline": a, "validation_eval_folds": b, "epoch_baseline": ea, "epoch_eval_folds": eb,
           "train_only": stats(t["train_only"]),
           "validation_speedup": round(a["median_ms"] / b["median_ms"], 2),
           "validation_share_of_epoch_baseline": round(a["median_ms"] / ea["median_ms"], 3),
           "validation_share_of_epoch_eval_folds": round(b["median_ms"] / eb["median_ms"], 3),
           "kernels_event_ms": {"median": round(kmed, 4), "min": round(min(kern), 4), "max": round(max(kern), 4)},
           "kernels_trials_per_s": int(K * nv / (kmed * 1e-3)),
           "k_infer_event_ms": {"median": round(imed, 4), "min": round(min(infer), 4), "max": round(max(infer), 4)},
           "k_infer_trials_per_s": int(K * nv / (imed * 1e-3)),
           "check": check,
           "accept_validation": bool(a["median_ms"] - b["median_ms"] > spread_a),
           "accept_epoch": bool(eb["median_ms"] <= ea["median_ms"])}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_folds_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_folds needs a HIP device (there is no fallback)")
    if args.reps < 5 or args.epochs < 50:
        print("note: fewer than 5 repetitions of 50 epochs: not a measurement to quote", flush=True)
    dev = torch.device("cuda:0")
    out = {"tool": "bench_eval_folds", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "timing": f"host clock around windows of {args.epochs} epochs ending in a device synchronise, "
                     f"{args.reps} windows per leg, baseline and eval_folds alternating; kernels by device events",
           "configs": []}
    for name, K, nv, ntr, p in CONFIGS:
        out["configs"].append(run_config(name, K, nv, ntr, p, args.reps, args.epochs, dev))
        torch.cuda.empty_cache()
    out["accept"] = bool(all(c["accept_validation"] and c["accept_epoch"] and all(
        v is True for k, v in c["check"].items() if k != "loss_max_rel_err") for c in out["configs"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print("wrote", args.out, "accept =", out["accept"])


if __name__ == "__main__":
    main()
