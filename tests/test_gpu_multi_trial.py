"""Several trials per workgroup at the runtime shapes: the train step and the eval forward at batches
large enough that every workgroup of every pass runs its trial loop more than once.

The streaming passes split a batch over min(B, 2 CUs) workgroups, passes C / D and the eval forward
over min(B, CUs), the F2 > 16 streaming passes over about CUs / ceil(F2 / 16) trial ranges
(eegnet_host.hip make_geo).  Every other test of a shape that is not one of the
compile-time ones (22 x 256 / 257 EEGNet-8,2, EEGNet-16,4 at 64 x 512) has B <= 40, so there each
`for (b = b0; b < b1; ++b)` runs once: the register-staged prefetch of the next trial's x (k_pass_a,
k_pass_e, k_infer, k_wpass_a / _e, k_winfer), of its v / d2 / r planes (k_pass_b, k_pass_dr, k_wpass_b,
the whole-trial block-2 passes) and the uneven trial split are first exercised here.

B comes from the library's own answer (ops.launch_grids): the smallest batch at which every pass's
every trial range holds at least two trials and no pass divides the batch evenly.  Pass C of the
F2 <= 16 step (k_pass_c) deals its trials to the waves of its workgroups, and the query counts those
per-wave streams (workgroups x 8 waves at the runtime shapes), so that every wave runs its trial loop
twice -- carrying wacc / sdz / bacc across trials and reusing its Hs row: B = 4097 for the F2 <= 16
shapes and 513 for the wide ones on 256 CUs.  Each test asserts that premise.

Per shape: the module path (forward_train + backward kernels) with injected masks, the fused step
(on-device masks, CE, backward, clamps, Adam) and the eval forward of the same batch, against the
float64 oracle.  The wide shapes (B = 513) use oracle/numpy_ref.py.  At B = 4097 a numpy_ref step
takes 5 to 11 s even for the small F2 <= 16 shapes (more for (4, 800) and (22, 257, 6, 2)), so these
use the reference layer stack in float64 on the device (oracle/torch_ref.py, as tests/test_gpu_wide.py
test_cfg5_full_batch_against_float64).  Tolerance: rtol 1e-4, atol 1e-5 max|ref| with the
near-zero-gradient rules (tests/golden_util.py).  The library's dims validation accepts every shape
below as listed; the library refuses to train (5, 72, 8, 4) with K1 = 64 (F1*D > 16 with 64 taps), so
that shape runs its eval forward only (EVAL_SHAPES)."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from golden_util import (PARAM_NAMES, assert_close, assert_grads_close, assert_params_close, make_inputs,
                         make_masks)
from hip_cases import (device_masks, flat_to_dict, grads_of, module_step, oracle_eval, random_model,
                       state_np)

pytestmark = pytest.mark.gpu

NARROW = [
    # C, T, F1, D, K1, p, float64 reference on the device
    (8, 64, 8, 2, 32, 0.25, True),
    (16, 200, 2, 2, 32, 0.25, True),
    (8, 100, 4, 1, 32, 0.5, True),
    (3, 64, 8, 2, 64, 0.25, True),
    (4, 800, 8, 2, 32, 0.25, True),
    (22, 257, 6, 2, 32, 0.5, True),
    # C in 33..48: three c-tiles in pass E's dws GEMM, two waves on each, waves 6 and 7 idle in it
    (40, 64, 8, 2, 32, 0.25, True),
]
WIDE = [
    (8, 64, 12, 2, 32, 0.5, False),     # F2 = 24: a partial o-chunk
    (6, 100, 16, 4, 32, 0.25, False),   # F2 = 64, T % 8 != 0, T1 = 25 odd: k_wpass_b's per-sample stores
    (10, 128, 12, 4, 32, 0.5, False),   # F2 = 48
]
SHAPES = NARROW + WIDE
# F2 = 32 with K1 = 64: the eval forward only.  The library refuses the train step of F1*D > 16 with
# 64 taps (eegnet_host.hip check_wide_train: it ended in a GPU memory fault at this shape, cause not
# known; tests/test_abi.py checks the refusal).
EVAL_SHAPES = SHAPES + [(5, 72, 8, 4, 64, 0.25, False)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def multi_trial_batch(shape):
    """The smallest B at which every pass gives each of its trial ranges (for k_pass_c: each wave's
    stream) >= 2 trials (B // n >= 2) and splits unevenly (B % n != 0), and the grids at that B."""
    from eegnetreplication_amd import ops
    for B in range(2, 1 << 16):
        grids = ops.launch_grids(shape, B)
        if all(B // n >= 2 and B % n for n in grids.values()):
            return B, grids
    raise AssertionError("no batch below 65536 gives every pass two trials per workgroup")


def _setup(C, T, F1, D, K1, p):
    """Model and batch of one shape (the same for its three tests), with the premise asserted."""
    _dev()
    m = random_model(C, T, F1=F1, D=D, K1=K1, p=p, seed=13 * C + T + F1 + D)
    B, grids = multi_trial_batch(m.shape)
    assert set(grids) == {"A", "B", "C", "D", "E", "eval"}
    for name, n in grids.items():
        assert n >= 1 and B // n >= 2 and B % n != 0, (name, n, B)
    x_np, y_np = make_inputs(B, C, T, 1200 + T + C)
    return m, B, x_np, y_np


def _torch_step(m, x_np, y_np, p, masks, dev):
    """float64 reference step on the device: logits, loss, clamped grads, updated running statistics."""
    from oracle import torch_ref as tr
    state = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    ref = tr.TorchRefEEGNet(state, p=p, device=dev, dtype=torch.float64)
    x = torch.from_numpy(x_np).to(dev).double()
    mk = None if masks is None else tuple(torch.from_numpy(a).to(dev) for a in masks)
    rl = ref(x, mk)
    rloss = torch.nn.functional.cross_entropy(rl, torch.from_numpy(y_np).to(dev))
    rloss.backward()
    return (rl.detach().cpu().numpy(), float(rloss), {k: ref.params[k].grad.cpu().numpy() for k in PARAM_NAMES},
            {k: v.cpu().numpy() for k, v in ref.buffers.items()})


def _check_buffers(m, ref_nb, what):
    bufs = {k: b.detach().cpu().numpy() for k, b in m.named_buffers()}
    for k, v in ref_nb.items():
        if "running_mean" in k:
            assert_close(bufs[k], v, atol_abs=1e-5 * max(1.0, float(np.abs(v).max())), name=f"{what} {k}")
        elif "running_var" in k:
            assert_close(bufs[k], v, name=f"{what} {k}")
        else:
            assert int(bufs[k]) == int(v), f"{what} {k}"


@pytest.mark.parametrize("C,T,F1,D,K1,p,big", SHAPES)
def test_multi_trial_module_step_matches_oracle(C, T, F1, D, K1, p, big):
    m, B, x_np, y_np = _setup(C, T, F1, D, K1, p)
    masks = make_masks(B, F1 * D, T, 1210 + C, p)
    what = f"EEGNet-{F1},{D} K1={K1} {C}x{T} B={B}"
    if not big:
        module_step(m, x_np, y_np, p, masks, what, _dev())      # test_gpu_wide._step's body
        return
    dev = _dev()
    ref_logits, ref_loss, ref_grads, ref_nb = _torch_step(m, x_np, y_np, p, masks, dev)
    m = m.to(dev).train()
    m.set_dropout_masks(torch.from_numpy(masks[0]).to(dev), torch.from_numpy(masks[1]).to(dev))
    logits = m(torch.from_numpy(x_np).to(dev))
    loss = torch.nn.functional.cross_entropy(logits, torch.from_numpy(y_np).to(dev))
    loss.backward()
    assert_close(logits.detach().cpu().numpy(), ref_logits, name=f"{what} logits")
    assert abs(float(loss) - ref_loss) <= 1e-4 * max(1.0, abs(ref_loss)), f"{what} loss"
    assert_grads_close(grads_of(m), ref_grads, prefix=f"{what} grad.")
    _check_buffers(m, ref_nb, what)


@pytest.mark.parametrize("C,T,F1,D,K1,p,big", SHAPES)
def test_multi_trial_fused_step_matches_oracle(C, T, F1, D, K1, p, big):
    from eegnetreplication_amd import FusedTrainer
    from oracle import numpy_ref as nr
    dev = _dev()
    m, B, x_np, y_np = _setup(C, T, F1, D, K1, p)
    seed, offset = 0x51DE_5EED, 5
    masks = device_masks(B, F1 * D, T, seed, offset, p)
    params, bufs = state_np(m)
    params = {k: v.astype(np.float64) for k, v in params.items()}
    if big:
        logits_ref, loss_ref, grads_ref, nb_ref = _torch_step(m, x_np, y_np, p, masks, dev)
        ref = dict(logits=logits_ref, loss=loss_ref, grads=grads_ref, buffers=nb_ref,
                   params=nr.adam_step(params, grads_ref, nr.adam_init(params), lr=1e-3, eps=1e-7))
    else:
        ref = nr.train_step(params, bufs, x_np, y_np, nr.adam_init(params), p=p, masks=masks)
    model = m.to(dev).train()
    model.next_dropout_key = lambda: (seed, offset)
    tr = FusedTrainer(model, lr=1e-3, eps=1e-7)
    logits = torch.empty((B, 4), device=dev)
    loss = tr.step(torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev), logits=logits)
    torch.cuda.synchronize()
    what = f"fused EEGNet-{F1},{D} K1={K1} {C}x{T} B={B}"
    assert_close(logits.cpu().numpy(), ref["logits"], name=f"{what} logits")
    assert abs(float(loss) - float(ref["loss"])) <= 1e-4 * max(1.0, abs(float(ref["loss"]))), what
    assert_grads_close(flat_to_dict(model, tr.adam.grads), ref["grads"], prefix=f"{what} grad.")
    _check_buffers(model, ref["buffers"], what)
    assert_params_close({k: q.detach().cpu().numpy() for k, q in model.named_parameters()}, ref["params"],
                        prefix=f"{what} step1.")


@pytest.mark.parametrize("C,T,F1,D,K1,p,big", EVAL_SHAPES)
def test_multi_trial_eval_matches_oracle(C, T, F1, D, K1, p, big):
    dev = _dev()
    m, B, x_np, _ = _setup(C, T, F1, D, K1, p)
    if big:
        from oracle import torch_ref as tr
        ref = tr.TorchRefEEGNet({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, p=p,
                                device=dev, dtype=torch.float64)
        ref.training = False
        with torch.no_grad():
            want = ref(torch.from_numpy(x_np).to(dev).double()).cpu().numpy()
    else:
        want = oracle_eval(m, x_np)
    m = m.to(dev).eval()
    with torch.no_grad():
        out = m(torch.from_numpy(x_np).to(dev)).cpu().numpy()
    assert_close(out, want, name=f"eval EEGNet-{F1},{D} K1={K1} {C}x{T} B={B}")
