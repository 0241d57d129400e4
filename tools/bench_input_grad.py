"""Time the eval-mode input gradient (eegnet_input_grad_eval, k_infer_dx) on the GPU.

At B = 4096 for 22 x 256 and 22 x 257 it times, per launch over a whole batch:
  (a) forward_eval_ms     ops.forward_eval (k_infer): the yardstick, one spatial GEMM + one FIR sweep
  (b) input_grad_ms       ops.input_grad_eval (CE seed): forward + transposed chain in one kernel
  (c) torch_autograd_ms   fp32 autograd of oracle.torch_ref.TorchRefEEGNet(device="cuda") in eval mode
                          for the same dx (torch.autograd.grad of the summed CE with respect to x only)
and prints ONE JSON line.  Device events around `inner` back-to-back launches, inputs rotated over
several buffers, warm-up first, the median over the repeats.  (b) must beat (c): the exit status is 1
when it does not.  (b) / (a) is reported, not gated.  Needs a HIP device; there is no CPU path.

    python tools/bench_input_grad.py [--batch 4096] [--repeats 15] [--out profiles/input_grad_bench.json]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eegnetreplication_amd import EEGNet, ops  # noqa: E402
from oracle.torch_ref import TorchRefEEGNet  # noqa: E402

NBUF = 4


def timed(fn, bufs, warmup, repeats, inner):
    """Median ms per call of fn(buf) over `repeats` windows of `inner` calls (device events)."""
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


def bench_shape(dev, B, C, T, warmup, repeats):
    torch.manual_seed(0)
    model = EEGNet(C, T)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                      # BN off identity, as a trained model's is
        for bn in model._bns():
            bn.weight.copy_(0.5 + torch.rand(bn.weight.shape, generator=g))
            bn.bias.copy_(0.2 * torch.randn(bn.bias.shape, generator=g))
            bn.running_mean.copy_(0.1 * torch.randn(bn.running_mean.shape, generator=g))
            bn.running_var.copy_(0.3 + torch.rand(bn.running_var.shape, generator=g))
    model = model.to(dev).eval()
    shape, flat, bnf = model.shape, model.flat_parameters(), model.flat_bn_buffers()
    xs = [torch.randn((B, C, T), device=dev, generator=torch.Generator(device=dev).manual_seed(10 + i))
          for i in range(NBUF)]
    y = torch.randint(0, 4, (B,), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    dx_out = torch.empty_like(xs[0])

    ref = TorchRefEEGNet({k: v.detach() for k, v in model.state_dict().items()}, p=0.0, device=dev)
    ref.training = False

    def autograd_dx(x):
        xr = x.detach().requires_grad_()
        loss = torch.nn.functional.cross_entropy(ref(xr), y, reduction="sum")
        return torch.autograd.grad(loss, xr)[0]

    fwd = lambda x: ops.forward_eval(shape, flat, bnf, x)
    dxf = lambda x: ops.input_grad_eval(shape, flat, bnf, x, kind="ce", targets=y, out=dx_out)

    # same dx from both routes before anything is timed (fp32 against fp32: summation order only)
    want = autograd_dx(xs[0])
    got, _ = dxf(xs[0])
    torch.cuda.synchronize()
    rel = float((got - want).abs().max() / want.abs().max())
    if not rel < 1e-3:
        raise SystemExit(f"{C}x{T}: input_grad_eval and fp32 autograd disagree (max|diff|/max|dx| = {rel:.3g})")

    a = timed(fwd, xs, warmup, repeats, inner=20)
    b = timed(dxf, xs, warmup, repeats, inner=20)
    c = timed(autograd_dx, xs, max(3, warmup // 2), max(5, repeats // 2), inner=3)
    nbytes = 2 * B * C * T * 4 + B * 16
    return {
        "C": C, "T": T, "B": B,
        "forward_eval_ms": round(a[0], 5), "forward_eval_ms_min_max": [round(a[1], 5), round(a[2], 5)],
        "input_grad_ms": round(b[0], 5), "input_grad_ms_min_max": [round(b[1], 5), round(b[2], 5)],
        "torch_autograd_ms": round(c[0], 4), "torch_autograd_ms_min_max": [round(c[1], 4), round(c[2], 4)],
        "input_grad_over_forward": round(b[0] / a[0], 3),
        "autograd_over_input_grad": round(c[0] / b[0], 1),
        "input_grad_trials_per_s": round(B / (b[0] * 1e-3)),
        "input_grad_hbm_gb_per_s": round(nbytes / (b[0] * 1e-3) / 1e9, 1),
        "max_rel_diff_vs_fp32_autograd": float(f"{rel:.3g}"),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this benchmark runs on the GPU only")
    dev = torch.device("cuda", 0)
    res = {"tool": "bench_input_grad", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
           "timing": f"device events, median of {args.repeats} windows, {NBUF} rotated input buffers",
           "shapes": [bench_shape(dev, args.batch, 22, T, args.warmup, args.repeats) for T in (256, 257)]}
    res["input_grad_beats_autograd"] = all(s["input_grad_ms"] < s["torch_autograd_ms"] for s in res["shapes"])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["input_grad_beats_autograd"] else 1


if __name__ == "__main__":
    sys.exit(main())
