"""Test-side helpers of the input-gradient tests: the float64 dx oracle (oracle.torch_ref's ATen layer
stack in eval mode under plain autograd, pinned to the reference by tests/golden/dx/DX1.npz) and the
fixture loader."""

from __future__ import annotations

import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from golden_util import GOLDEN_DIR, make_inputs
from oracle.torch_ref import TorchRefEEGNet

DX_DIR = os.path.join(GOLDEN_DIR, "dx")


def load_dx_fixture(name="DX1"):
    z = np.load(os.path.join(DX_DIR, name + ".npz"), allow_pickle=False)
    z = {k: z[k] for k in z.files}
    meta = json.loads(str(z["meta"]))
    x, y = make_inputs(meta["B"], meta["C"], meta["T"], meta["seed"])
    state = {k[5:]: v for k, v in z.items() if k.startswith("init.")}
    return z, meta, state, x, y


def oracle_dx(state: dict, x, kind: str, dlogits=None, targets=None):
    """float64 (dx, logits) of the eval-mode stack.  kind: "dlogits" (seed ``dlogits``), "logit"
    (onehot(targets); the argmax of the float64 logits when targets is None) or "ce"
    (softmax - onehot(targets): cross-entropy with reduction "sum")."""
    m = TorchRefEEGNet(state, p=0.0, dtype=torch.float64)
    m.training = False
    xt = torch.as_tensor(np.asarray(x), dtype=torch.float64).clone().requires_grad_()
    logits = m(xt)
    if kind == "dlogits":
        seed = torch.as_tensor(np.asarray(dlogits), dtype=torch.float64)
        (dx,) = torch.autograd.grad(logits, xt, seed)
    elif kind == "logit":
        t = logits.argmax(1) if targets is None else torch.as_tensor(np.asarray(targets), dtype=torch.int64)
        (dx,) = torch.autograd.grad(logits.gather(1, t.view(-1, 1)).sum(), xt)
    elif kind == "ce":
        t = torch.as_tensor(np.asarray(targets), dtype=torch.int64)
        (dx,) = torch.autograd.grad(F.cross_entropy(logits, t, reduction="sum"), xt)
    else:
        raise ValueError(kind)
    return dx.numpy(), logits.detach().numpy()


def model_state(m) -> dict:
    """state_dict of a product EEGNet as CPU numpy arrays (the oracle's input)."""
    return {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
