"""Preprocessing of continuous recordings on the device: exponential moving standardisation, the step the
reference applies to every recording before it cuts trials out of it (``raw_exponential_moving_standardize``,
dataset.py:45-70).  ``raw recording -> exponential_moving_standardize -> sliding_logits`` runs without a host
step; ``StreamStandardizer`` is the same call fed block by block with the state carried along.
"""

from __future__ import annotations

import torch

from . import ops
from .ops import require_device


def _as_rows(rec, what):
    """``rec`` [C, N] or [R, C, N] on the device, float32 or float64 -> ([R, C, N] view, was 2-D)."""
    if rec.dim() not in (2, 3):
        raise RuntimeError(f"expected a recording [C, N] or [R, C, N], got {list(rec.shape)}")
    require_device(rec, what)
    if rec.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"exponential moving standardisation expects a float32 or float64 recording "
                           f"(got {rec.dtype})")
    return (rec.unsqueeze(0), True) if rec.dim() == 2 else (rec, False)


def _standardize(rec, out, **kw):
    if out is not None and out.shape != rec.shape:
        raise ValueError(f"out must have the recording's shape {list(rec.shape)} (got {list(out.shape)})")
    r3, squeeze = _as_rows(rec, "EEGNet recording")
    o3 = None
    if out is not None:
        require_device(out, "out")
        o3 = out.unsqueeze(0) if squeeze else out
    with torch.no_grad():
        y = ops.ems(r3.detach(), o3, **kw)
    if out is not None:
        return out
    return y[0] if squeeze else y


def exponential_moving_standardize(rec, factor_new=1e-3, init_block_size=1000, eps=1e-10, out=None):
    """Exponential moving standardisation of continuous recordings, per channel row:

        m_t = (1 - factor_new) m_{t-1} + factor_new x_t
        v_t = (1 - factor_new) v_{t-1} + factor_new (x_t - m_t)^2
        y_t = (x_t - m_t) / sqrt(v_t + eps)

    with (m, v) started at the mean and the population variance of the row's first
    min(init_block_size, N) samples.  ``rec`` is [C, N] or [R, C, N], float32 or float64, on the device, and
    is read in place when its last stride is 1 and its rows lie at one pitch (a contiguous tensor, or a
    time slice of a larger buffer, passed as it lies).  Returns float32 of the same shape; all arithmetic is
    float64 on the device and the result is rounded once.  ``out``: a float32 tensor of that shape to
    receive the result -- ``rec`` itself for an in-place call on a float32 recording.  The result goes
    straight into ``sliding_logits`` / ``cropped_predict``, a time slice of it included.  The same inputs
    give the same bits."""
    return _standardize(rec, out, factor_new=float(factor_new), init_block=int(init_block_size), eps=float(eps))


class StreamStandardizer:
    """``exponential_moving_standardize`` fed block by block: the standardiser of a pseudo-online decoder.

    ``n_rows_or_shape``: the number of channel rows C, or the leading shape of every block -- ``(C,)`` for
    blocks [C, n], ``(R, C)`` for blocks [R, C, n].  ``push(block)`` returns the standardised block
    (float32) and carries the running (mean, var) of every row to the next push; ``state`` is that float64
    [rows, 2] tensor on the device (None before the first push), ``reset()`` forgets it.

    The first push starts from the mean and variance of its own first min(init_block_size, n) samples.
    The concatenated output therefore equals ``exponential_moving_standardize`` of the whole recording
    only when the first block holds at least ``init_block_size`` samples; with a shorter first block the
    start values come from fewer samples and the outputs differ until the moving statistics forget them."""

    def __init__(self, n_rows_or_shape, factor_new=1e-3, init_block_size=1000, eps=1e-10):
        lead = (int(n_rows_or_shape),) if isinstance(n_rows_or_shape, int) else tuple(int(s) for s in n_rows_or_shape)
        if len(lead) not in (1, 2) or min(lead) < 1:
            raise ValueError(f"expected a row count or a leading shape (C,) or (R, C), got {n_rows_or_shape!r}")
        self.lead = lead
        self.factor_new, self.init_block_size, self.eps = float(factor_new), int(init_block_size), float(eps)
        self.state = None

    def reset(self):
        self.state = None

    def push(self, block):
        if tuple(block.shape[:-1]) != self.lead:
            raise RuntimeError(f"expected a block {list(self.lead)} + [n], got {list(block.shape)}")
        resume = self.state is not None
        if not resume:
            require_device(block, "EEGNet recording block")
            rows = 1
            for s in self.lead:
                rows *= s
            state = torch.empty((rows, 2), dtype=torch.float64, device=block.device)
        else:
            state = self.state
        y = _standardize(block, None, factor_new=self.factor_new, init_block=self.init_block_size, eps=self.eps,
                         state=state, resume=resume)
        if block.shape[-1] > 0:
            self.state = state
        return y
