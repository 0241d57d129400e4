"""GPU tests of the eval-mode input gradients (k_infer_dx behind eegnet_input_grad_eval): parity with
the float64 oracle (tests/dx_cases.py, pinned to the reference by tests/golden/dx/DX1.npz) for the three
seed kinds over the compile-time shapes, K1 = 64, the reference's test shapes, F2 = 4 and a batch larger
than the launch grid; the argmax seed; trial independence, determinism and non-finite isolation; the
bounds of the dx writes; the autograd path of EEGNet.forward; relevance_maps; saliency on a wide model.

Tolerance: the project's (golden_util.assert_close: rtol 1e-4, atol 1e-5 * max|ref|)."""

from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dx_cases import model_state, oracle_dx
from golden_util import assert_close, make_inputs
from hip_cases import random_model

pytestmark = pytest.mark.gpu

KINDS = ("dlogits", "logit", "ce")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _case(C, T, B, F1=8, D=2, K1=32, seed=0):
    """(model on the device in eval mode, oracle state, x, y, dlogits) -- numpy inputs."""
    m = random_model(C, T, F1=F1, D=D, K1=K1, seed=3 * C + T + F1 + K1 + seed)
    state = model_state(m)
    x, y = make_inputs(B, C, T, 1200 + T + C + seed)
    dl = np.random.default_rng(77 + B + seed).standard_normal((B, 4)).astype(np.float32)
    return m.to(_dev()).eval(), state, x, y, dl


def _run(model, x, kind, dlogits=None, targets=None, out=None):
    from eegnetreplication_amd import ops
    dev = _dev()
    t = lambda a, dt: None if a is None else torch.as_tensor(np.asarray(a), dtype=dt).to(dev)
    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return ops.input_grad_eval(model.shape, model.flat_parameters(), model.flat_bn_buffers(), xd, kind=kind,
                               dlogits=t(dlogits, torch.float32), targets=t(targets, torch.int64), out=out)


def _seed_args(kind, y, dl):
    return dict(dlogits=dl) if kind == "dlogits" else dict(targets=y)


def _check_parity(model, state, x, y, dl, what):
    for kind in KINDS:
        kw = _seed_args(kind, y, dl)
        dx_ref, lg_ref = oracle_dx(state, x, kind, **kw)
        dx, lg = _run(model, x, kind, **kw)
        torch.cuda.synchronize()
        assert_close(lg.cpu().numpy(), lg_ref, name=f"{what} {kind} logits")
        assert_close(dx.cpu().numpy(), dx_ref, name=f"{what} {kind} dx")


SHAPES = [
    # C, T, B, F1, D, K1
    (22, 256, 3, 8, 2, 32),      # compile-time shape
    (22, 257, 5, 8, 2, 32),      # pool truncation, unaligned rows, odd B
    (22, 257, 2, 8, 2, 64),      # K1 = 64
    (8, 64, 4, 8, 2, 32),        # reference test shape
    (64, 128, 2, 8, 2, 32),      # reference test shape
    (32, 512, 2, 8, 2, 32),      # reference test shape
    (5, 96, 3, 4, 1, 32),        # F2 = 4, C not a multiple of 4
    (22, 256, 2, 2, 2, 32),      # F2 = 4 with D = 2
]


@pytest.mark.parametrize("C,T,B,F1,D,K1", SHAPES)
def test_dx_matches_float64_oracle(C, T, B, F1, D, K1):
    model, state, x, y, dl = _case(C, T, B, F1, D, K1)
    _check_parity(model, state, x, y, dl, f"EEGNet-{F1},{D} K1={K1} {C}x{T} B={B}")


@pytest.mark.parametrize("C,T,B,F1,D,K1", [(22, 257, 5, 8, 2, 32), (5, 96, 3, 4, 1, 32), (22, 257, 2, 8, 2, 64)])
def test_dx_logits_equal_the_eval_forward(C, T, B, F1, D, K1):
    """k_infer_dx's forward half is k_infer's arithmetic on k_infer's operands: the logits input_grad_eval
    returns are forward_eval's, bit for bit."""
    from eegnetreplication_amd import ops
    model, _, x, y, _ = _case(C, T, B, F1, D, K1)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(_dev())
    want = ops.forward_eval(model.shape, model.flat_parameters(), model.flat_bn_buffers(), xd)
    _, lg = _run(model, xd, "ce", targets=y)
    assert torch.equal(lg, want)


def test_dx_with_more_trials_than_the_launch_grid():
    """8 x 64 with B = 2 * grid + 3 (the host launches min(B, CUs) workgroups): the strided trial loop
    and the reuse of the x rows (as dx staging, then for the prefetched next trial) run."""
    dev = _dev()
    grid = torch.cuda.get_device_properties(dev).multi_processor_count
    B = 2 * grid + 3
    model, state, x, y, dl = _case(8, 64, B)
    _check_parity(model, state, x, y, dl, f"8x64 B={B}")


def test_argmax_seed_equals_explicit_argmax_targets():
    model, _, x, _, _ = _case(22, 257, 6, seed=1)
    dx_a, lg = _run(model, x, "logit")
    dx_b, lg_b = _run(model, x, "logit", targets=lg.argmax(1).cpu().numpy())
    assert torch.equal(lg, lg_b)
    assert torch.equal(dx_a, dx_b)
    assert float(dx_a.abs().max()) > 0


def test_trials_are_independent_and_runs_deterministic():
    model, _, x, y, dl = _case(22, 257, 5, seed=2)
    for kind in KINDS:
        kw = _seed_args(kind, y, dl)
        dx, lg = _run(model, x, kind, **kw)
        dx2, lg2 = _run(model, x, kind, **kw)
        assert torch.equal(dx, dx2) and torch.equal(lg, lg2), kind
        for b in range(5):
            kb = {k: v[b:b + 1] for k, v in kw.items()}
            dx1, lg1 = _run(model, x[b:b + 1], kind, **kb)
            assert torch.equal(dx1[0], dx[b]) and torch.equal(lg1[0], lg[b]), (kind, b)


def test_non_finite_trial_does_not_leak_into_the_others():
    """One trial of five poisoned with NaN / Inf samples: the other four come back bit-identical to
    the clean run.  What this catches is stale LDS carried between trials, and at B = 5 every trial has a
    workgroup of its own, so the same is run at B = 2 * CUs + 5 with the poisoned trial in the middle of
    a workgroup's three (trials b, b + CUs, b + 2 CUs share one)."""
    dev = _dev()
    grid = torch.cuda.get_device_properties(dev).multi_processor_count
    for B, bad in ((5, 2), (2 * grid + 5, grid + 1)):
        model, _, x, y, dl = _case(22, 257, B, seed=3)
        clean_dx, clean_lg = _run(model, x, "ce", targets=y)
        xp = x.copy()
        xp[bad, 3, 10] = np.nan
        xp[bad, 7, 100] = np.inf
        xp[bad, 0, 256] = -np.inf
        xp[bad, 21, 0] = np.nan
        dx, lg = _run(model, xp, "ce", targets=y)
        keep = torch.ones(B, dtype=torch.bool, device=dev)
        keep[bad] = False
        assert torch.equal(dx[keep], clean_dx[keep]), B
        assert torch.equal(lg[keep], clean_lg[keep]), B
        assert not bool(torch.isfinite(dx[bad]).all())


@pytest.mark.parametrize("C,T,F1,D", [(22, 257, 8, 2), (5, 96, 4, 1)])
@pytest.mark.parametrize("guard", [1024, 1031])
def test_dx_writes_stay_inside_dx_and_cover_it(C, T, F1, D, guard):
    """dx as a slice of a larger buffer with sentinel bands on both sides (guard 1031: a dx that is
    only 4-byte aligned, so 5 x 96 takes the scalar stores): the bands come back untouched and every
    element of dx is written (a second run on another sentinel gives the same bits)."""
    dev = _dev()
    B = 3
    model, _, x, y, _ = _case(C, T, B, F1, D, seed=4)
    n = B * C * T
    want, _ = _run(model, x, "ce", targets=y)
    outs = []
    for sentinel in (777.25, -3.5e8):
        buf = torch.full((guard + n + guard,), sentinel, dtype=torch.float32, device=dev)
        dx = buf[guard:guard + n].view(B, C, T)
        got, _ = _run(model, x, "ce", targets=y, out=dx)
        torch.cuda.synchronize()
        assert got.data_ptr() == dx.data_ptr()
        assert bool((buf[:guard] == sentinel).all()) and bool((buf[guard + n:] == sentinel).all())
        outs.append(dx.clone())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], want)


def test_autograd_path_through_eval_forward():
    dev = _dev()
    model, state, x_np, y_np, dl = _case(22, 257, 4, seed=5)
    y = torch.from_numpy(y_np).to(dev)
    x = torch.from_numpy(x_np).to(dev).requires_grad_()
    logits = model(x)
    F.cross_entropy(logits, y, reduction="sum").backward()
    dx_ref, lg_ref = oracle_dx(state, x_np, "ce", targets=y_np)
    assert_close(logits.detach().cpu().numpy(), lg_ref, name="autograd logits")
    assert_close(x.grad.cpu().numpy(), dx_ref, name="x.grad (CE, sum)")
    assert all(p.grad is None for p in model.parameters())
    # an explicit seed through torch.autograd.grad
    x2 = torch.from_numpy(x_np).to(dev).requires_grad_()
    (g,) = torch.autograd.grad(model(x2), x2, torch.from_numpy(dl).to(dev))
    dx_ref, _ = oracle_dx(state, x_np, "dlogits", dlogits=dl)
    assert_close(g.cpu().numpy(), dx_ref, name="autograd.grad (dlogits)")
    # train mode keeps refusing input gradients
    model.train()
    with pytest.raises(NotImplementedError, match="gradients with respect to the EEG input"):
        model(torch.from_numpy(x_np).to(dev).requires_grad_())
    # eval mode without x.requires_grad: the parameter path still has no backward
    model.eval()
    out = model(torch.from_numpy(x_np).to(dev))
    assert out.requires_grad
    with pytest.raises(NotImplementedError, match="eval-mode EEGNet forward"):
        out.sum().backward()


def test_saliency_uses_eval_semantics_and_leaves_the_mode():
    from eegnetreplication_amd import saliency
    dev = _dev()
    model, state, x_np, y_np, _ = _case(22, 256, 3, seed=6)
    x = torch.from_numpy(x_np).to(dev)
    model.train()
    dx, lg = saliency(model, x, targets=torch.from_numpy(y_np), kind="ce")
    assert model.training and not dx.requires_grad
    dx_ref, lg_ref = oracle_dx(state, x_np, "ce", targets=y_np)
    assert_close(dx.cpu().numpy(), dx_ref, name="saliency ce dx")
    assert_close(lg.cpu().numpy(), lg_ref, name="saliency logits")
    dx, lg = saliency(model, x)                       # the predicted class
    dx_ref, _ = oracle_dx(state, x_np, "logit", targets=lg.argmax(1).cpu().numpy())
    assert_close(dx.cpu().numpy(), dx_ref, name="saliency logit dx")
    with pytest.raises(ValueError):
        saliency(model, x, kind="ce")


@pytest.mark.parametrize("method", ["gradxinput", "grad"])
def test_relevance_maps_match_oracle(method):
    from eegnetreplication_amd import relevance_maps
    _dev()
    C, T, sizes = 22, 257, (4, 3, 5)
    N = sum(sizes)
    model, state, x_np, _, _ = _case(C, T, N, seed=7)
    y_np = (np.arange(N) % 4).astype(np.int64)
    loader, o = [], 0
    for s in sizes:
        loader.append((torch.from_numpy(x_np[o:o + s]), torch.from_numpy(y_np[o:o + s])))
        o += s
    got = relevance_maps(model, loader, method=method)
    assert tuple(got.shape) == (4, C, T) and got.dtype == torch.float32
    dx, _ = oracle_dx(state, x_np, "logit", targets=y_np)
    rel = np.abs(dx * x_np.astype(np.float64)) if method == "gradxinput" else np.abs(dx)
    want = np.stack([rel[y_np == k].mean(0) for k in range(4)])
    assert_close(got.cpu().numpy(), want, name=f"relevance_maps {method}")


def test_saliency_on_a_wide_model_raises():
    from eegnetreplication_amd import saliency
    dev = _dev()
    m = random_model(64, 512, F1=16, D=4, seed=9).to(dev).eval()
    x = torch.zeros((1, 64, 512), device=dev)
    with pytest.raises(NotImplementedError, match=r"input gradients: F1\*D = 64 > 16 is not supported"):
        saliency(m, x)
    with pytest.raises(NotImplementedError, match="gradients with respect to the EEG input"):
        m(x.clone().requires_grad_())
