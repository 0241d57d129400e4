"""Generate the frozen-BatchNorm fixture tests/golden/frozen/FZ1.npz from the REFERENCE implementation.

Runs on the development machine only, where the reference imports (torch CPU), like make_golden.py:
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_frozen.py

The reference ``EEGNet(22, 257)`` (model.py:12-99) in train mode with its three BatchNorm2d modules in
``.eval()`` (the stock way to fine-tune with frozen statistics), BatchNorm affine parameters and running
statistics moved off identity, p = 0.5 with the dropout keep-masks injected through forward hooks as
make_golden.py does, B = 3.  Stored: the initial state, the masks, logits, the mean cross-entropy, the 12
parameter gradients of ``loss * scale`` for scale 1 (``grad1.*``) and 64 (``grad64.*``: both clamps of
model.py:44/84 active) and the BatchNorm buffers after the step (``buf1.*``, equal to the initial ones).
Inputs x / labels are regenerated from ``inputs.make_inputs`` by seed and are not stored.  The fixture
lives in the ``frozen/`` subdirectory: every ``tests/golden/*.npz`` is a training fixture.
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

from inputs import make_inputs, make_masks  # noqa: E402
from eegnet_repl.model import EEGNet  # noqa: E402  (the reference)

import logging  # noqa: E402
logging.getLogger().setLevel(logging.WARNING)

torch.set_num_threads(8)

C, T, B, P, SEED = 22, 257, 3, 0.5, 93
SCALES = (1, 64)


def install_masks(model, p, masks):
    """Replace nn.Dropout's random draw with the given keep-masks (1 = keep), as make_golden.py."""
    drops = [m for m in model.modules() if isinstance(m, nn.Dropout)]
    assert len(drops) == 2
    for mod, mk in zip(drops, masks):
        def hook(module, inp, out, mk=mk):
            assert module.training
            m = torch.as_tensor(mk, dtype=torch.float32).reshape(out.shape)
            return inp[0] * (m / (1.0 - p))
        mod.register_forward_hook(hook)


def main():
    torch.manual_seed(1000 + SEED)
    model = EEGNet(C=C, T=T, p=P)
    g = torch.Generator().manual_seed(77 + SEED)
    bns = [m for m in model.modules() if isinstance(m, nn.BatchNorm2d)]
    with torch.no_grad():
        for mod in bns:
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.3)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
            mod.weight.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
            mod.bias.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
    model.train()
    for mod in bns:
        mod.eval()
    out = {"init." + k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    x, y = make_inputs(B, C, T, SEED)
    masks = make_masks(B, 16, T, SEED * 100, P)
    install_masks(model, P, masks)
    out["mask2"], out["mask3"] = masks
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    for scale in SCALES:
        model.zero_grad()
        logits = model(xt)
        loss = F.cross_entropy(logits, yt)
        (loss * scale).backward()
        for k, prm in model.named_parameters():
            out[f"grad{scale}." + k] = prm.grad.detach().numpy().copy()
    out["logits"] = logits.detach().numpy().copy()
    out["loss"] = np.array(loss.item())
    for k, v in model.state_dict().items():
        if "running" in k or "num_batches" in k:
            out["buf1." + k] = v.detach().cpu().numpy().copy()
    meta = dict(name="FZ1", C=C, T=T, B=B, F1=8, D=2, p=P, seed=SEED, scales=list(SCALES),
                torch=torch.__version__, reference="PraKesEy/EEGNetReplication src/eegnet_repl/model.py")
    out["meta"] = np.array(json.dumps(meta))
    os.makedirs(os.path.join(HERE, "frozen"), exist_ok=True)
    path = os.path.join(HERE, "frozen", "FZ1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
