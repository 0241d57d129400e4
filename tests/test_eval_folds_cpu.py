"""Fold-indexed validation (eegnet_eval_folds), the checks that need no GPU: the C-ABI declares and the
binding mirrors the call and its record, the validation rejects what the kernels do not cover before
any device call, and the float64 metric helper the GPU tests use as their oracle (tests/eval_cases.py)
is the reference's own validation loop (model.py:151-172)."""

from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from eval_cases import val_metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "eegnet_abi.h")


def _lib_or_skip():
    from eegnetreplication_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libeegnet_hip.so not built (run __graft_entry__.build())")
    return _lib, _lib.load()


def test_header_declares_and_binding_has_eval_folds():
    from eegnetreplication_amd import _lib
    txt = open(HEADER).read()
    for name in ("eegnet_eval_folds", "eegnet_eval_fold_bytes"):
        assert re.search(r"^\s*(?:int|size_t)\s+" + name + r"\s*\(", txt, re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
    assert len(_lib._SIGS["eegnet_eval_folds"][1]) == 7
    assert re.search(r"#define EEGNET_ABI_VERSION 5\b", txt)      # no field of dims / fold moved


def test_eval_fold_mirror_matches_header():
    from eegnetreplication_amd import _lib
    txt = open(HEADER).read()
    body = re.search(r"typedef struct eegnet_eval_fold \{(.*?)\} eegnet_eval_fold;", txt, re.S).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\**(\w+);", body, re.M)
    assert fields == [n for n, _ in _lib.EvalFold._fields_]
    assert len(fields) == 10
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    snippet = re.search(r"class EvalFold\(ctypes\.Structure\):(.*?)\nassert", doc, re.S).group(1)
    assert re.findall(r'"(\w+)"', snippet) == fields


def test_eval_fold_bytes_matches_mirror():
    _lib, lib = _lib_or_skip()
    assert lib.eegnet_eval_fold_bytes() == ctypes.sizeof(_lib.EvalFold) == 80


def _call(lib, d, nfolds=2, table=256, max_n=8, batch=64, slot=0):
    # the table pointer is a dummy that is never dereferenced: every call here fails on its arguments
    return lib.eegnet_eval_folds(ctypes.byref(d), nfolds, ctypes.c_void_p(table) if table else None, max_n,
                                 batch, slot, None)


def test_wide_dims_are_rejected():
    _lib, lib = _lib_or_skip()
    assert _call(lib, _lib.dims(1, 64, 512, F1=16, D=4)) == -1
    assert b"F1*D" in lib.eegnet_last_error()


def test_argument_validation_without_a_gpu():
    _lib, lib = _lib_or_skip()
    d = _lib.dims(1, 22, 257)
    for kw, word in ((dict(nfolds=0), b"nfolds"), (dict(table=0), b"folds is NULL"), (dict(batch=0), b"batch"),
                     (dict(max_n=-1), b"max_n"), (dict(max_n=2 ** 40), b"max_n"), (dict(slot=-1), b"slot")):
        assert _call(lib, d, **kw) == -1, kw
        assert word in lib.eegnet_last_error(), kw
    assert _call(lib, _lib.dims(1, 22, 257, x_pitch=260)) == -1
    assert b"x_pitch" in lib.eegnet_last_error()
    assert _call(lib, _lib.dims(0, 22, 257, K1=48)) == -1          # invalid dims (dims->B itself is ignored)
    assert b"K1" in lib.eegnet_last_error()


def _reference_loop(logits, labels, batch):
    """model.py:151-172 literally: per DataLoader batch F.cross_entropy (a mean), summed, divided by
    len(loader); correct trials counted by argmax.  float64."""
    z, y = torch.from_numpy(logits).double(), torch.from_numpy(labels)
    running, correct, nb = 0.0, 0, 0
    for i in range(0, len(y), batch):
        zb, yb = z[i:i + batch], y[i:i + batch]
        running += torch.nn.functional.cross_entropy(zb, yb).item()
        correct += int((zb.argmax(1) == yb).sum())
        nb += 1
    return running / nb, correct


@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_metric_helper_is_the_reference_loop(n):
    rng = np.random.default_rng(n)
    logits = (3.0 * rng.standard_normal((n, 4))).astype(np.float32)
    labels = rng.integers(0, 4, n).astype(np.int64)
    ce, loss, correct = val_metrics(logits, labels, 64)
    ref_loss, ref_correct = _reference_loop(logits, labels, 64)
    assert ce.shape == (n,) and ce.dtype == np.float64
    assert abs(loss - ref_loss) <= 1e-12 * max(1.0, abs(ref_loss))
    assert correct == ref_correct
    if n == 130:                     # a short last batch weighs as much as a full one: not the plain mean
        assert abs(loss - ce.mean()) > 1e-6
        assert abs(val_metrics(logits, labels, 130)[1] - ce.mean()) <= 1e-12
        assert abs(val_metrics(logits, labels, 1)[1] - ce.mean()) <= 1e-12


def test_metric_helper_edges():
    assert val_metrics(np.zeros((0, 4), np.float32), np.zeros(0, np.int64))[1:] == (0.0, 0)
    ce, loss, correct = val_metrics(np.zeros((3, 4), np.float32), np.array([0, 1, 0]))
    assert np.allclose(ce, np.log(4.0)) and correct == 2           # ties: the lowest index


def test_metric_helper_on_golden_eval_logits():
    """The helper on the oracle's eval-mode logits of golden G2, against the literal loop."""
    from golden_util import Golden
    from oracle import numpy_ref as nr
    g = Golden("G2")
    logits, _, _ = nr.forward(g.init_params(), g.init_buffers(), g.x, train=False)
    logits = np.asarray(logits, dtype=np.float32)
    for batch in (64, 5):
        _, loss, correct = val_metrics(logits, g.y, batch)
        ref_loss, ref_correct = _reference_loop(logits, np.asarray(g.y, dtype=np.int64), batch)
        assert abs(loss - ref_loss) <= 1e-12 * max(1.0, abs(ref_loss))
        assert correct == ref_correct


def test_evaluate_folds_refuses_wide_and_mixed_shapes():
    """One common shape with F1*D <= 16, or a ValueError that says what to do instead (raised before
    anything touches a device)."""
    from eegnetreplication_amd import EEGNet, FoldBatch, evaluate_folds
    assert callable(FoldBatch.validate)
    x, y = torch.zeros(2, 64, 512), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="one at a time"):
        evaluate_folds([EEGNet(64, 512, F1=16, D=4)], [(x, y)])
    with pytest.raises(ValueError, match="one at a time"):
        evaluate_folds([EEGNet(22, 256), EEGNet(22, 257)], [(x, y), (x, y)])
    with pytest.raises(ValueError, match="per model"):
        evaluate_folds([EEGNet(22, 256)], [])
