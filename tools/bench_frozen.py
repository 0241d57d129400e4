"""Time the fused frozen-BatchNorm fine-tuning step (eegnet_frozen_step: k_frozen + k_frozen_reduce + Adam).

For 22 x 256 and 22 x 257 at B = 64 (the fine-tuning regime) and B = 4096 it times, per iteration:
  (a) frozen_step_ms   ops.frozen_step with labels and the fused Adam (device-generated dropout masks)
  (b) train_step_ms    ops.train_step, the existing five-pass train-mode step with batch statistics and
                       its fused Adam, x at the row pitch its kernels load fastest (eegnet_x_pitch)
  (c) torch_stock_ms   a stock-PyTorch fp32 module with the same layer stack built here, its BatchNorm
                       modules in eval(), nn.Dropout, autograd and torch.optim.Adam(lr=1e-3, eps=1e-7)
and prints ONE JSON line.  Device events around `inner` back-to-back iterations, inputs rotated over
several buffers, warm-up first, the median over the repeats with min / max recorded.  The gate: at B = 64
(a) is not slower than (b) beyond the recorded run-to-run spread (the larger of the two min-max ranges);
the exit status is 1 when it is.  The B = 4096 figures and (c) / (a) are reported, not gated.  Needs a HIP
device; there is no CPU path.

    python tools/bench_frozen.py [--repeats 15] [--out profiles/frozen_bench.json]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eegnetreplication_amd import EEGNet, ops  # noqa: E402

NBUF = 4


def timed(fn, bufs, warmup, repeats, inner):
    """Median / min / max ms per call of fn(buf) over `repeats` windows of `inner` calls (device events)."""
    k = 0
    for _ in range(warmup):
        fn(bufs[k % len(bufs)])
        k += 1
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn(bufs[k % len(bufs)])
            k += 1
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return statistics.median(ms), min(ms), max(ms)


def stock_module(C, T, F1=8, D=2, K1=32, p=0.5):
    """The EEGNet-8,2 layer stack as plain torch.nn modules (input [B, 1, C, T])."""
    F2 = F1 * D
    return nn.Sequential(
        nn.Conv2d(1, F1, kernel_size=(1, K1), padding="same", bias=False), nn.BatchNorm2d(F1),
        nn.Conv2d(F1, F2, kernel_size=(C, 1), padding="valid", groups=F1, bias=False),
        nn.BatchNorm2d(F2), nn.ELU(), nn.AvgPool2d(kernel_size=(1, 4)), nn.Dropout(p=p),
        nn.Conv2d(F2, F2, kernel_size=(1, 16), padding="same", groups=F2, bias=False),
        nn.Conv2d(F2, F2, kernel_size=(1, 1), padding="same", bias=False),
        nn.BatchNorm2d(F2), nn.ELU(), nn.AvgPool2d(kernel_size=(1, 8)), nn.Dropout(p=p), nn.Flatten(),
        nn.Linear(F2 * (T // 32), 4, bias=True))


def new_model(dev, C, T):
    torch.manual_seed(0)
    model = EEGNet(C, T)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                      # BN off identity, as a trained model's is
        for bn in model._bns():
            bn.weight.copy_(0.5 + torch.rand(bn.weight.shape, generator=g))
            bn.bias.copy_(0.2 * torch.randn(bn.bias.shape, generator=g))
            bn.running_mean.copy_(0.1 * torch.randn(bn.running_mean.shape, generator=g))
            bn.running_var.copy_(0.3 + torch.rand(bn.running_var.shape, generator=g))
    return model.to(dev).train()


def bench_shape(dev, B, C, T, warmup, repeats):
    gen = lambda s: torch.Generator(device=dev).manual_seed(s)
    xs = [torch.randn((B, C, T), device=dev, generator=gen(10 + i)) for i in range(NBUF)]
    y = torch.randint(0, 4, (B,), device=dev, generator=gen(5))
    inner = 20 if B <= 256 else 5

    def adam_bufs(model):
        n = model.flat_parameters().numel()
        return (torch.zeros(n, device=dev), torch.zeros(2 * n, device=dev),
                torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, device=dev))

    # (a) the fused frozen step
    mf = new_model(dev, C, T)
    shape, flat, bnf = mf.shape, mf.flat_parameters(), mf.flat_bn_buffers()
    grads, adam, step, loss = adam_bufs(mf)
    ws = ops.new_frozen_workspace(shape, B, dev)
    frozen = lambda x: ops.frozen_step(shape, flat, bnf, x, 7, 0, grads, ws, labels=y, adam_state=adam,
                                       step_i32=step, loss=loss, key_from_step=True)
    a = timed(frozen, xs, warmup, repeats, inner)

    # (b) the train-mode step (batch statistics), x at its fastest pitch
    mt = new_model(dev, C, T)
    flat_t, bn_t, nbt_t = mt.flat_views()
    grads_t, adam_t, step_t, loss_t = adam_bufs(mt)
    ws_t = ops.new_workspace(shape, B, dev)
    xts = [ops.pad_x_rows(x, shape.x_pitch()) for x in xs]
    train = lambda x: ops.train_step(shape, flat_t, bn_t, x, y, 7, 0, grads_t, adam_t, step_t, ws_t, loss_t,
                                     nbt=nbt_t, key_from_step=True)
    b = timed(train, xts, warmup, repeats, inner)

    # (c) stock PyTorch: the same stack, BatchNorm modules in eval(), autograd, torch.optim.Adam
    stock = stock_module(C, T).to(dev).train()
    for mod in stock.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.eval()
    opt = torch.optim.Adam(stock.parameters(), lr=1e-3, eps=1e-7)

    def stock_step(x):
        lo = nn.functional.cross_entropy(stock(x.unsqueeze(1)), y)
        opt.zero_grad()
        lo.backward()
        opt.step()

    c = timed(stock_step, xs, max(3, warmup // 2), max(5, repeats // 2), inner=3)
    torch.cuda.synchronize()
    if not (bool(torch.isfinite(flat).all()) and bool(torch.isfinite(flat_t).all()) and int(step.item()) > 0):
        raise SystemExit(f"{C}x{T} B={B}: a timed step left non-finite parameters")
    r = lambda v, n=5: round(v, n)
    spread = max(a[2] - a[1], b[2] - b[1])
    return {
        "C": C, "T": T, "B": B,
        "frozen_step_ms": r(a[0]), "frozen_step_ms_min_max": [r(a[1]), r(a[2])],
        "train_step_ms": r(b[0]), "train_step_ms_min_max": [r(b[1]), r(b[2])],
        "torch_stock_ms": r(c[0], 4), "torch_stock_ms_min_max": [r(c[1], 4), r(c[2], 4)],
        "spread_ms": r(spread),
        "frozen_over_train": r(a[0] / b[0], 3),
        "stock_over_frozen": r(c[0] / a[0], 1),
        "frozen_trials_per_s": round(B / (a[0] * 1e-3)),
        "frozen_not_slower_than_train": bool(a[0] <= b[0] + spread),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.repeats < 5:
        raise SystemExit("--repeats must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this benchmark runs on the GPU only")
    dev = torch.device("cuda", 0)
    res = {"tool": "bench_frozen", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
           "timing": f"device events, median of {args.repeats} windows, {NBUF} rotated input buffers",
           "shapes": [bench_shape(dev, B, 22, T, args.warmup, args.repeats) for B in (64, 4096) for T in (256, 257)]}
    res["gate_b64_frozen_not_slower_than_train"] = all(s["frozen_not_slower_than_train"] for s in res["shapes"]
                                                       if s["B"] == 64)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["gate_b64_frozen_not_slower_than_train"] else 1


if __name__ == "__main__":
    sys.exit(main())
