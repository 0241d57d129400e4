"""Test-side helpers of the frozen-BatchNorm tests: the float64 oracle (oracle.torch_ref's ATen layer
stack with every BatchNorm normalising by its running statistics and dropout on, under plain autograd;
pinned to the reference by tests/golden/frozen/FZ1.npz) and the fixture loader."""

from __future__ import annotations

import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from golden_util import CLAMPED_GRADS, GOLDEN_DIR, PARAM_NAMES, assert_close, make_inputs
from oracle.numpy_ref import BN_EPS, BN_MOMENTUM
from oracle.torch_ref import TorchRefEEGNet

FZ_DIR = os.path.join(GOLDEN_DIR, "frozen")
CLAMPS = {"spatial.weight": 1.0, "classifier.weight": 0.25}      # model.py:44, model.py:84


class FrozenRefEEGNet(TorchRefEEGNet):
    """The reference layer stack in train mode with its three BatchNorm layers in eval(): running
    statistics used, no buffer touched; ``_drop`` (inherited) follows ``p`` and the injected masks."""

    def __init__(self, state: dict, p: float = 0.5, dtype=torch.float64):
        super().__init__(state, p=p, dtype=dtype)
        self.training = True

    def _bn(self, pre, a):
        b = self.buffers
        return F.batch_norm(a, b[f"{pre}.running_mean"], b[f"{pre}.running_var"],
                            self.params[f"{pre}.weight"], self.params[f"{pre}.bias"],
                            training=False, momentum=BN_MOMENTUM, eps=BN_EPS)


def load_fz_fixture(name="FZ1"):
    z = np.load(os.path.join(FZ_DIR, name + ".npz"), allow_pickle=False)
    z = {k: z[k] for k in z.files}
    meta = json.loads(str(z["meta"]))
    x, y = make_inputs(meta["B"], meta["C"], meta["T"], meta["seed"])
    state = {k[5:]: v for k, v in z.items() if k.startswith("init.")}
    return z, meta, state, x, y


def oracle_frozen(state: dict, x, p, masks=None, labels=None, dlogits=None, loss_scale=1.0):
    """float64 frozen-BatchNorm step.  Seed: mean cross-entropy against ``labels`` times ``loss_scale``,
    or ``dlogits``.  Returns dict(logits, loss, grads (clamped by the reference's hooks), raw (the same
    gradients before the hooks), buffers (after the step), model)."""
    assert (labels is None) != (dlogits is None)
    assert p == 0.0 or masks is not None
    m = FrozenRefEEGNet(state, p=p)
    xt = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    logits = m(xt, masks if p > 0 else None)
    loss = None
    if labels is not None:
        loss = F.cross_entropy(logits, torch.as_tensor(np.asarray(labels), dtype=torch.int64))
        (loss * loss_scale).backward()
    else:
        logits.backward(torch.as_tensor(np.asarray(dlogits), dtype=torch.float64))
    grads = {k: m.params[k].grad.numpy().copy() for k in PARAM_NAMES}
    # the same gradients before the two hooks
    raw = raw_grads(state, x, p, masks, labels=labels, dlogits=dlogits, loss_scale=loss_scale)
    return dict(logits=logits.detach().numpy(), loss=None if loss is None else float(loss.detach()), grads=grads, raw=raw,
                buffers={k: v.numpy().copy() for k, v in m.buffers.items()}, model=m)


def raw_grads(state, x, p, masks, labels=None, dlogits=None, loss_scale=1.0):
    """The 12 gradients before the clamps of model.py:44/84 (the hooks removed from the leaves)."""
    m = FrozenRefEEGNet(state, p=p)
    for k in CLAMPED_GRADS:
        m.params[k] = m.params[k].detach().clone().requires_grad_(True)      # a leaf without the hook
    logits = m(torch.as_tensor(np.asarray(x), dtype=torch.float64), masks if p > 0 else None)
    if labels is not None:
        out = F.cross_entropy(logits, torch.as_tensor(np.asarray(labels), dtype=torch.int64)) * loss_scale
        gs = torch.autograd.grad(out, m.parameters())
    else:
        gs = torch.autograd.grad(logits, m.parameters(), torch.as_tensor(np.asarray(dlogits), dtype=torch.float64))
    return {k: g.numpy().copy() for k, g in zip(PARAM_NAMES, gs)}


def assert_frozen_grads_close(actual: dict, expected: dict, raw: dict | None = None, prefix="", rtol=1e-4,
                              atol_frac=1e-5):
    """Every tensor, gamma1 / beta1 included, to plain assert_close (rtol 1e-4, atol 1e-5 * max|ref|);
    the two clamped tensors judged at their unclamped scale (``raw``), as assert_grads_close does."""
    for k in PARAM_NAMES:
        if raw is not None and k in CLAMPED_GRADS:
            scale = max(float(np.max(np.abs(raw[k]))), float(np.max(np.abs(expected[k]))))
            assert_close(actual[k], expected[k], rtol=rtol, atol_abs=atol_frac * scale, name=prefix + k)
        else:
            assert_close(actual[k], expected[k], rtol=rtol, atol_frac=atol_frac, name=prefix + k)


def model_state(m) -> dict:
    """state_dict of a product EEGNet as CPU numpy arrays (the oracle's input)."""
    return {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
