"""Generate the input-gradient fixture tests/golden/dx/DX1.npz from the REFERENCE implementation.

Runs on the development machine only, where the reference imports (torch CPU), like make_golden.py:
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_dx.py

The reference ``EEGNet(22, 257)`` (model.py:12-99) in ``.eval()``, BatchNorm affine parameters and
running statistics moved off identity, B = 2; ``x.grad`` by plain autograd for two seeds:
  dx_ce       d/dx of F.cross_entropy(logits, y, reduction="sum")
  dx_dlogits  d/dx of (logits * dlogits).sum() for the stored ``dlogits``
Inputs x / labels are regenerated from ``inputs.make_inputs`` by seed and are not stored.  The
fixture lives in the ``dx/`` subdirectory: every ``tests/golden/*.npz`` is a training fixture.
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference/src")

from inputs import make_inputs  # noqa: E402
from eegnet_repl.model import EEGNet  # noqa: E402  (the reference)

import logging  # noqa: E402
logging.getLogger().setLevel(logging.WARNING)

torch.set_num_threads(8)

C, T, B, SEED = 22, 257, 2, 91


def main():
    torch.manual_seed(1000 + SEED)
    model = EEGNet(C=C, T=T)
    g = torch.Generator().manual_seed(77 + SEED)
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.3)
                mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
                mod.weight.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
    model.eval()
    out = {"init." + k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    x, y = make_inputs(B, C, T, SEED)
    dlogits = torch.randn(B, 4, generator=g)
    yt = torch.from_numpy(y)

    xt = torch.from_numpy(x).requires_grad_()
    logits = model(xt)
    F.cross_entropy(logits, yt, reduction="sum").backward()
    out["logits"] = logits.detach().numpy().copy()
    out["dx_ce"] = xt.grad.numpy().copy()

    xt = torch.from_numpy(x).requires_grad_()
    (dx,) = torch.autograd.grad(model(xt), xt, dlogits)
    out["dx_dlogits"] = dx.numpy().copy()
    out["dlogits"] = dlogits.numpy().copy()

    meta = dict(name="DX1", C=C, T=T, B=B, F1=8, D=2, seed=SEED, torch=torch.__version__,
                reference="PraKesEy/EEGNetReplication src/eegnet_repl/model.py")
    out["meta"] = np.array(json.dumps(meta))
    os.makedirs(os.path.join(HERE, "dx"), exist_ok=True)
    path = os.path.join(HERE, "dx", "DX1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
