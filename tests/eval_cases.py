"""The validation metrics of the reference's epoch loop (model.py:151-172) in float64 numpy: the oracle of
the fold-indexed validation call (eegnet_eval_folds), shared by its CPU and GPU tests."""

from __future__ import annotations

import numpy as np

LOSS_RTOL = 1e-4      # the project's bar for the fused CE loss (tests/test_gpu_parity.py)


def trial_ce(logits, labels):
    """Per-trial cross-entropy logsumexp(logits) - logits[label], float64 [n]."""
    z = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    mx = z.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(z - mx).sum(axis=1))
    return lse - z[np.arange(len(y)), y]


def val_metrics(logits, labels, batch=64):
    """``(ce [n], loss, correct)``: the per-trial CE; the validation loss -- the mean over the batches of
    ``batch`` consecutive trials (the last one short) of each batch's mean CE, i.e.
    running_val_loss / len(val_loader) -- and the number of trials whose argmax (lowest index on a
    tie) is the label.  No trials: loss 0, correct 0."""
    z = np.asarray(logits, dtype=np.float64).reshape(-1, 4)
    y = np.asarray(labels, dtype=np.int64)
    n = len(y)
    ce = trial_ce(z, y)
    means = [ce[i:i + batch].mean() for i in range(0, n, batch)]
    loss = float(np.sum(means) / len(means)) if means else 0.0
    correct = int((z.argmax(axis=1) == y).sum()) if n else 0
    return ce, loss, correct


def loss_tol(ref):
    """|got - ref| bound of a loss / CE value: 1e-4 * max(1, |ref|)."""
    return LOSS_RTOL * np.maximum(1.0, np.abs(ref))
