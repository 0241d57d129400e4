"""Torch-facing wrappers of the HIP C-ABI: train/eval forward, backward, Adam, fused train step.

Every function here runs the HIP kernels of ``csrc/eegnet_kernels.hip`` through
``libeegnet_hip.so``; tensors must live on a HIP device.  There is no CPU or eager-PyTorch path.
"""

from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import torch

from . import _lib

NCLS = 4


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_device(t: torch.Tensor, what: str):
    if t.device.type != "cuda":
        raise RuntimeError(
            f"{what} is on '{t.device}': the MI355X EEGNet path runs on a HIP device only "
            f"(move the model and the inputs to 'cuda').")


@dataclass(frozen=True)
class Shape:
    """Static dims of one EEGNet instance (model.py:13)."""
    C: int
    T: int
    F1: int = 8
    D: int = 2
    K1: int = 32
    p: float = 0.5
    eps: float = 1e-5
    momentum: float = 0.1

    @property
    def F2(self):
        return self.F1 * self.D

    @property
    def T1(self):
        return self.T // 4

    @property
    def T2(self):
        return self.T1 // 8

    def dims(self, B: int, p: float | None = None, x_pitch: int = 0) -> _lib.Dims:
        if p is None:                 # per-(B, pitch) cache (the struct is only read by the library)
            cache = self.__dict__.setdefault("_dims_cache", {})
            d = cache.get((B, x_pitch))
            if d is None:
                d = cache[(B, x_pitch)] = _lib.dims(B, self.C, self.T, self.F1, self.D, self.K1, self.p,
                                                    self.eps, self.momentum, x_pitch)
            return d
        return _lib.dims(B, self.C, self.T, self.F1, self.D, self.K1, p, self.eps, self.momentum, x_pitch)

    def x_pitch(self) -> int:
        """The x row pitch the training kernels load fastest (eegnet_x_pitch): T rounded up to 4
        floats for 22 x 257, else T."""
        return int(_lib.load().eegnet_x_pitch(ctypes.byref(self.dims(1))))

    def param_shapes(self):
        """(name, shape) in nn.Module.named_parameters() order (model.py:22-84)."""
        F1, F2, C, K1 = self.F1, self.F2, self.C, self.K1
        nf = F2 * (self.T // 32)
        return [
            ("temporal.0.weight", (F1, 1, 1, K1)), ("temporal.1.weight", (F1,)),
            ("temporal.1.bias", (F1,)), ("spatial.weight", (F2, 1, C, 1)),
            ("aggregation.0.weight", (F2,)), ("aggregation.0.bias", (F2,)),
            ("block_2.0.weight", (F2, 1, 1, 16)), ("block_2.1.weight", (F2, F2, 1, 1)),
            ("block_2.2.weight", (F2,)), ("block_2.2.bias", (F2,)),
            ("classifier.weight", (NCLS, nf)), ("classifier.bias", (NCLS,)),
        ]

    def n_params(self):
        n = 0
        for _, s in self.param_shapes():
            k = 1
            for d in s:
                k *= d
            n += k
        return n

    def bn_layout(self):
        """Flat bn_buffers order of the ABI: rm1, rv1, rm2, rv2, rm3, rv3."""
        F1, F2 = self.F1, self.F2
        return [("temporal.1.running_mean", F1), ("temporal.1.running_var", F1),
                ("aggregation.0.running_mean", F2), ("aggregation.0.running_var", F2),
                ("block_2.2.running_mean", F2), ("block_2.2.running_var", F2)]


PASSES = ("A", "B", "C", "D", "E", "eval")


def launch_grids(shape: Shape, B: int, fold_launch: bool = False) -> dict:
    """eegnet_launch_grids: {pass: number of trial ranges a batch of B is split into} for the train
    step's passes A to E and the eval forward ("eval"; 0 for a fold launch).  Every range -- the
    trials one workgroup (pass C for F1*D <= 16: one wave) runs in turn -- holds B // n or B // n + 1
    trials.  ``fold_launch``: the
    per-fold grids of ``train_step_folds``.  Host-side geometry only: nothing is launched."""
    out = (ctypes.c_int * len(PASSES))()
    _lib.check(_lib.load().eegnet_launch_grids(ctypes.byref(shape.dims(B)), ctypes.c_int(1 if fold_launch else 0),
                                               out), "eegnet_launch_grids")
    return dict(zip(PASSES, (int(v) for v in out)))


def new_workspace(shape: Shape, B: int, device) -> torch.Tensor:
    nbytes = _lib.workspace_bytes(shape.dims(B))
    return torch.zeros(nbytes, dtype=torch.uint8, device=device)   # zero-filled once (tickets)


def forward_train(shape: Shape, flat_params, bn_flat, x, ws, seed: int, offset: int,
                  masks=None, p: float | None = None, nbt=None) -> torch.Tensor:
    """Train-mode forward: BN batch stats (+ running-stat update in bn_flat), dropout."""
    B = x.shape[0]
    logits = torch.empty((B, NCLS), dtype=torch.float32, device=x.device)
    m2, m3 = masks if masks is not None else (None, None)
    d = shape.dims(B, p, x_pitch_of(x))
    _lib.check(_lib.load().eegnet_forward_train(
        ctypes.byref(d), _ptr(flat_params), _ptr(bn_flat), _ptr(x), _ptr(m2), _ptr(m3),
        ctypes.c_uint64(seed), ctypes.c_uint64(offset), _ptr(logits), _ptr(ws), _stream(),
        _ptr(nbt)), "eegnet_forward_train")
    return logits


NO_CLAMP = 1
KEY_FROM_STEP = 2      # include/eegnet_abi.h: dropout key follows the device Adam step (graphs)


def backward(shape: Shape, flat_params, x, ws, seed: int, offset: int, dlogits=None, labels=None,
             masks=None, p: float | None = None, grads=None, loss=None, clamp=True) -> torch.Tensor:
    B = x.shape[0]
    if grads is None:
        grads = torch.empty_like(flat_params)
    m2, m3 = masks if masks is not None else (None, None)
    d = shape.dims(B, p, x_pitch_of(x))
    _lib.check(_lib.load().eegnet_backward(
        ctypes.byref(d), _ptr(flat_params), _ptr(x), _ptr(dlogits), _ptr(labels), _ptr(m2),
        _ptr(m3), ctypes.c_uint64(seed), ctypes.c_uint64(offset), _ptr(grads), _ptr(loss), _ptr(ws),
        _stream(), 0 if clamp else NO_CLAMP), "eegnet_backward")
    return grads


def clamp_grads(shape: Shape, grads):
    """model.py:44/84 gradient clamps on a flat grad buffer (after a data-parallel all-reduce)."""
    _lib.check(_lib.load().eegnet_clamp_grads(ctypes.byref(shape.dims(1)), _ptr(grads), _stream()),
               "eegnet_clamp_grads")


def forward_eval(shape: Shape, flat_params, bn_flat, x) -> torch.Tensor:
    x = x.contiguous()                # the eval kernels read [B][C][T] rows (no pitch)
    B = x.shape[0]
    logits = torch.empty((B, NCLS), dtype=torch.float32, device=x.device)
    d = shape.dims(B)
    _lib.check(_lib.load().eegnet_forward_eval(
        ctypes.byref(d), _ptr(flat_params), _ptr(bn_flat), _ptr(x), _ptr(logits), _stream()),
        "eegnet_forward_eval")
    return logits


def window_count(shape: Shape, n_samples: int, hop: int) -> int:
    """eegnet_window_count: the T-sample windows, ``hop`` samples apart, of a recording of ``n_samples``
    samples -- (n_samples - T) // hop + 1.  Host-side only."""
    out = ctypes.c_int64(0)
    _lib.check(_lib.load().eegnet_window_count(ctypes.byref(shape.dims(1)), ctypes.c_int64(n_samples),
                                               ctypes.c_int64(hop), ctypes.byref(out)), "eegnet_window_count")
    return int(out.value)


def forward_eval_windows(shape: Shape, flat_params, bn_flat, rec, hop: int, *, reduce=False):
    """Eval-mode forward of every T-sample window of continuous recordings (eegnet_forward_eval_windows):
    window w of a recording is its samples [w hop, w hop + T).  ``rec`` is [C, N] or [R, C, N] float32 on
    the device and is read in place -- no unfolded copy -- when its last stride is 1 and its channel and
    recording strides are ``pitch`` and ``C * pitch`` (a contiguous tensor, or a time slice of one);
    anything else is made contiguous first.  Returns logits [R, W, 4] ([W, 4] for a 2-D ``rec``), each
    row bit-identical to ``forward_eval`` on that window; with ``reduce=True`` ``(logits, probs, pred)``,
    probs [R, 4] = the mean over a recording's windows of softmax(logits) (accumulated in float64) and
    pred [R] int32 its argmax (``[4]`` and a 0-d tensor for a 2-D ``rec``)."""
    require_device(rec, "rec")
    if rec.dtype != torch.float32:
        raise RuntimeError(f"forward_eval_windows expects float32 input (got {rec.dtype})")
    if rec.dim() not in (2, 3) or rec.shape[-2] != shape.C:
        raise RuntimeError(f"expected a recording [{shape.C}, N] or [R, {shape.C}, N], got {list(rec.shape)}")
    squeeze = rec.dim() == 2
    r3 = rec.unsqueeze(0) if squeeze else rec
    R, C, N = r3.shape
    pitch = r3.stride(1) if C > 1 else r3.stride(0) if R > 1 else N      # (a size-1 dim's stride says nothing)
    in_place = r3.stride(2) == 1 and pitch >= N and (R <= 1 or r3.stride(0) == C * pitch)
    if not in_place:
        r3 = r3.contiguous()
        pitch = N
    W = window_count(shape, N, hop)                       # (raises on hop < 1 or N < T)
    logits = torch.empty((R, W, NCLS), dtype=torch.float32, device=rec.device)
    probs = torch.empty((R, NCLS), dtype=torch.float32, device=rec.device) if reduce else None
    pred = torch.empty((R,), dtype=torch.int32, device=rec.device) if reduce else None
    if R:
        _lib.check(_lib.load().eegnet_forward_eval_windows(
            ctypes.byref(shape.dims(1)), _ptr(flat_params), _ptr(bn_flat), _ptr(r3), ctypes.c_int64(R),
            ctypes.c_int64(N), ctypes.c_int64(pitch), ctypes.c_int64(hop), _ptr(logits), _ptr(probs), _ptr(pred),
            _stream()), "eegnet_forward_eval_windows")
    if squeeze:
        logits = logits[0]
        if reduce:
            probs, pred = probs[0], pred[0]
    return (logits, probs, pred) if reduce else logits


def ems_chunk() -> int:
    """eegnet_ems_chunk: the samples of one chunk of the standardisation's scan.  Host-side only."""
    return int(_lib.load().eegnet_ems_chunk())


def _row_pitch(t: torch.Tensor):
    """The element pitch of the rows of ``t`` [R, C, N] when they lie at one pitch (last stride 1, pitch >= N,
    recording stride C * pitch), else None.  A size-1 dimension's stride says nothing."""
    R, C, N = t.shape
    pitch = t.stride(1) if C > 1 else t.stride(0) if R > 1 else N
    if N > 1 and t.stride(2) != 1:
        return None
    if pitch < N or (C > 1 and R > 1 and t.stride(0) != C * pitch):
        return None
    return int(pitch)


def ems(x, out=None, *, factor_new=1e-3, init_block=1000, eps=1e-10, state=None, resume=False):
    """Exponential moving standardisation of continuous recordings (eegnet_ems): per row
    m_t = (1-a) m_{t-1} + a x_t, v_t = (1-a) v_{t-1} + a (x_t - m_t)^2, y_t = (x_t - m_t) / sqrt(v_t + eps),
    a = ``factor_new``, in float64 on the device, rounded to float32 once.  ``x`` is [R, C, N] float32 or
    float64 on the device and is read in place when its rows lie at one pitch (a contiguous tensor or a time
    slice of one); anything else is made contiguous first.  ``out``: a float32 [R, C, N] device tensor whose
    rows lie at one pitch, to receive y -- ``x`` itself for an in-place call (float32) -- else a new
    contiguous one.  ``state``: float64 [R * C, 2] = (mean, var) per row; it receives the final state, and
    with ``resume`` the rows start from it instead of from their first ``init_block`` samples."""
    require_device(x, "x")
    if x.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"ems expects float32 or float64 input (got {x.dtype})")
    if x.dim() != 3:
        raise RuntimeError(f"expected recordings [R, C, N], got {list(x.shape)}")
    R, C, N = x.shape
    in_place = out is not None and out.data_ptr() == x.data_ptr()
    xp = _row_pitch(x)
    if xp is None:
        if in_place:
            raise ValueError("an in-place call needs rows at one pitch with a last stride of 1")
        x, xp = x.contiguous(), N
    if out is None:
        out = torch.empty((R, C, N), dtype=torch.float32, device=x.device)
    elif out.shape != x.shape or out.dtype != torch.float32 or out.device != x.device or _row_pitch(out) is None:
        raise ValueError(f"out must be a float32 {list(x.shape)} tensor on {x.device} whose rows lie at one pitch "
                         f"(last stride 1)")
    if state is not None and (state.dtype != torch.float64 or tuple(state.shape) != (R * C, 2)
                              or not state.is_contiguous() or state.device != x.device):
        raise ValueError(f"state must be a contiguous float64 [{R * C}, 2] tensor on {x.device}")
    if R * C == 0 or N == 0:
        return out
    lib = _lib.load()
    nbytes = ctypes.c_size_t(0)
    _lib.check(lib.eegnet_ems_scratch_bytes(ctypes.c_int64(R * C), ctypes.c_int64(N), ctypes.byref(nbytes)),
               "eegnet_ems_scratch_bytes")
    scratch = torch.empty(int(nbytes.value), dtype=torch.uint8, device=x.device)
    _lib.check(lib.eegnet_ems(
        _ptr(x), ctypes.c_int(x.dtype == torch.float64), ctypes.c_int64(R * C), ctypes.c_int64(N), ctypes.c_int64(xp),
        _ptr(out), ctypes.c_int64(_row_pitch(out)), ctypes.c_double(factor_new), ctypes.c_int64(init_block),
        ctypes.c_double(eps), _ptr(state), ctypes.c_int(1 if resume else 0), _ptr(scratch), _stream()), "eegnet_ems")
    return out


FIR_WHOLE, FIR_FIRST, FIR_NEXT, FIR_TAIL = 0, 1, 2, 3     # include/eegnet_abi.h EEGNET_FIR_*


def fir_chunk() -> int:
    """eegnet_fir_chunk: the outputs of one workgroup of the FIR kernel.  Host-side only."""
    return int(_lib.load().eegnet_fir_chunk())


def fir_max_taps() -> int:
    """eegnet_fir_max_taps: the longest filter eegnet_fir takes.  Host-side only."""
    return int(_lib.load().eegnet_fir_max_taps())


def fir(x, taps, out=None, *, mode=FIR_WHOLE, hist_in=None, hist_out=None, lead=None):
    """FIR filtering of continuous recordings (eegnet_fir): per row y[t] = sum_k taps[k] u[t + M - k],
    M = (L - 1) // 2, in float64 on the device, rounded to float32 once.  ``x`` is [R, C, N] float32 or float64
    on the device and is read in place when its rows lie at one pitch (a contiguous tensor or a time slice of
    one); anything else is made contiguous first.  ``taps``: a contiguous float64 [L] device tensor.
    ``mode``: FIR_WHOLE, the zero-phase call with both ends reflected (N outputs); FIR_FIRST, a stream's
    first block (N >= L, N - M outputs, ``hist_out`` written); FIR_NEXT, a continuation (``hist_in`` read,
    ``hist_out`` written, N outputs); FIR_TAIL, the stream's last M outputs from ``hist_in`` (``x`` is None
    and ``lead`` = (R, C)).  The histories are contiguous float64 [R * C, L - 1] device tensors, two different
    ones.  ``out``: a float32 [R, C, outputs] device tensor whose rows lie at one pitch and that does not
    overlap ``x`` (ValueError), else a new contiguous one."""
    require_device(taps, "taps")
    if taps.dtype != torch.float64 or taps.dim() != 1 or not taps.is_contiguous():
        raise ValueError("taps must be a contiguous float64 [L] tensor on the device")
    L = int(taps.shape[0])
    M = (L - 1) // 2
    if mode == FIR_TAIL:
        if x is not None or lead is None:
            raise ValueError("the tail call takes no samples: x is None and lead = (R, C)")
        R, C = (int(v) for v in lead)
        N, xp, is64, dev = 0, 0, False, taps.device
    else:
        require_device(x, "x")
        if x.dtype not in (torch.float32, torch.float64):
            raise RuntimeError(f"fir expects float32 or float64 input (got {x.dtype})")
        if x.dim() != 3:
            raise RuntimeError(f"expected recordings [R, C, N], got {list(x.shape)}")
        R, C, N = x.shape
        xp = _row_pitch(x)
        if xp is None:
            x, xp = x.contiguous(), N
        is64, dev = x.dtype == torch.float64, x.device
    n_out = {FIR_WHOLE: N, FIR_FIRST: max(N - M, 0), FIR_NEXT: N, FIR_TAIL: M}[mode]
    if out is None:
        out = torch.empty((R, C, n_out), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (R, C, n_out) or out.dtype != torch.float32 or out.device != dev or _row_pitch(out) is None:
        raise ValueError(f"out must be a float32 {[R, C, n_out]} tensor on {dev} whose rows lie at one pitch "
                         f"(last stride 1)")
    for name, h in (("hist_in", hist_in), ("hist_out", hist_out)):
        if h is not None and (h.dtype != torch.float64 or tuple(h.shape) != (R * C, L - 1) or not h.is_contiguous()
                              or h.device != dev):
            raise ValueError(f"{name} must be a contiguous float64 [{R * C}, {L - 1}] tensor on {dev}")
    if R * C == 0 or (N == 0 and mode != FIR_TAIL):
        return out
    op = _row_pitch(out)
    if mode != FIR_TAIL and n_out > 0:
        # the library rejects it too (EEGNET_EINVAL): said here as the ValueError the Python surface promises
        x0, x1 = x.data_ptr(), x.data_ptr() + ((R * C - 1) * xp + N) * x.element_size()
        y0, y1 = out.data_ptr(), out.data_ptr() + ((R * C - 1) * op + n_out) * 4
        if x0 < y1 and y0 < x1:
            raise ValueError("out overlaps x: filtering in place is not supported (a workgroup's outputs would "
                             "overwrite inputs its neighbours still read)")
    _lib.check(_lib.load().eegnet_fir(
        _ptr(x), ctypes.c_int(is64), ctypes.c_int64(R * C), ctypes.c_int64(N), ctypes.c_int64(xp), _ptr(taps),
        ctypes.c_int(L), _ptr(out), ctypes.c_int64(op), _ptr(hist_in), _ptr(hist_out), ctypes.c_int(mode), _stream()),
        "eegnet_fir")
    return out


RESAMPLE_WHOLE, RESAMPLE_FIRST, RESAMPLE_NEXT, RESAMPLE_TAIL = 0, 1, 2, 3    # include/eegnet_abi.h EEGNET_RESAMPLE_*
RESAMPLE_ENDS = {"zero": 0, "reflect_limited": 1}                             # EEGNET_RESAMPLE_ENDS_*


def resample_max_taps() -> int:
    """eegnet_resample_max_taps: the longest prototype filter eegnet_resample takes.  Host-side only."""
    return int(_lib.load().eegnet_resample_max_taps())


def resample_max_up() -> int:
    """eegnet_resample_max_up: the largest reduced ``up`` eegnet_resample takes.  Host-side only."""
    return int(_lib.load().eegnet_resample_max_up())


def resample_chunk(n_taps: int, up: int, down: int) -> int:
    """eegnet_resample_chunk: the outputs of one workgroup of the resampling kernel for this prototype and ratio
    (sized to the LDS; the outputs' bits do not depend on it).  Host-side only."""
    ch = int(_lib.load().eegnet_resample_chunk(ctypes.c_int(n_taps), ctypes.c_int(up), ctypes.c_int(down)))
    if ch < 0:
        _lib.check(ch, "eegnet_resample_chunk")
    return ch


def resample_count(n_samples: int, n_taps: int, up: int, down: int, *, mode=RESAMPLE_WHOLE, n_before=0) -> int:
    """eegnet_resample_count: the outputs per row that a call with these integers writes.  Host-side only."""
    out = ctypes.c_int64(0)
    _lib.check(_lib.load().eegnet_resample_count(ctypes.c_int64(n_samples), ctypes.c_int64(n_before), ctypes.c_int(n_taps),
                                                 ctypes.c_int(up), ctypes.c_int(down), ctypes.c_int(mode),
                                                 ctypes.byref(out)), "eegnet_resample_count")
    return int(out.value)


def resample(x, taps, up, down, out=None, *, ends="reflect_limited", mode=RESAMPLE_WHOLE, n_before=0, hist_in=None,
             hist_out=None, lead=None):
    """Rational polyphase resampling of continuous recordings (eegnet_resample; scipy's ``resample_poly``, not the
    FFT method the reference's ``raw.resample`` defaults to): per row, with c = m down + half,
    y[m] = sum_n taps[c - n up] u[n], in float64 on the device, rounded to float32 once.  ``x`` is [R, C, N]
    float32 or float64 on the device and is read in place when its rows lie at one pitch; anything else is made
    contiguous first.  ``taps``: a contiguous float64 [L] device tensor, L odd.  ``ends``: "zero" or
    "reflect_limited".  ``mode``: RESAMPLE_WHOLE; RESAMPLE_FIRST, a stream's first block (``hist_out`` written);
    RESAMPLE_NEXT, a continuation after ``n_before`` samples (``hist_in`` read, ``hist_out`` written);
    RESAMPLE_TAIL, the stream's last outputs from ``hist_in`` after ``n_before`` samples (``x`` is None and
    ``lead`` = (R, C)).  The histories are contiguous float64 [R * C, 2 (L // 2 // up) + 2] device tensors (``up``
    reduced), two different ones.  The output count is ``resample_count`` of the same integers.  ``out``: a
    float32 [R, C, outputs] device tensor whose rows lie at one pitch and that does not overlap ``x``
    (ValueError), else a new contiguous one."""
    require_device(taps, "taps")
    if taps.dtype != torch.float64 or taps.dim() != 1 or not taps.is_contiguous():
        raise ValueError("taps must be a contiguous float64 [L] tensor on the device")
    if ends not in RESAMPLE_ENDS:
        raise ValueError(f"ends must be one of {sorted(RESAMPLE_ENDS)} (got {ends!r})")
    L, up, down = int(taps.shape[0]), int(up), int(down)
    if mode == RESAMPLE_TAIL:
        if x is not None or lead is None:
            raise ValueError("the tail call takes no samples: x is None and lead = (R, C)")
        R, C = (int(v) for v in lead)
        N, xp, is64, dev = 0, 0, False, taps.device
    else:
        require_device(x, "x")
        if x.dtype not in (torch.float32, torch.float64):
            raise RuntimeError(f"resample expects float32 or float64 input (got {x.dtype})")
        if x.dim() != 3:
            raise RuntimeError(f"expected recordings [R, C, N], got {list(x.shape)}")
        R, C, N = x.shape
        xp = _row_pitch(x)
        if xp is None:
            x, xp = x.contiguous(), N
        is64, dev = x.dtype == torch.float64, x.device
    if R * C == 0 or (N == 0 and mode != RESAMPLE_TAIL):
        raise ValueError(f"an empty recording cannot be resampled (got {[R, C, N]})")
    n_out = resample_count(N, L, up, down, mode=mode, n_before=n_before)
    if out is None:
        out = torch.empty((R, C, n_out), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (R, C, n_out) or out.dtype != torch.float32 or out.device != dev or _row_pitch(out) is None:
        raise ValueError(f"out must be a float32 {[R, C, n_out]} tensor on {dev} whose rows lie at one pitch "
                         f"(last stride 1)")
    g = math.gcd(up, down)
    H = 2 * ((L // 2) // (up // g)) + 2
    for name, h in (("hist_in", hist_in), ("hist_out", hist_out)):
        if h is not None and (h.dtype != torch.float64 or tuple(h.shape) != (R * C, H) or not h.is_contiguous()
                              or h.device != dev):
            raise ValueError(f"{name} must be a contiguous float64 [{R * C}, {H}] tensor on {dev}")
    op = _row_pitch(out)
    if mode != RESAMPLE_TAIL and n_out > 0:
        # the library rejects it too (EEGNET_EINVAL): said here as the ValueError the Python surface promises
        x0, x1 = x.data_ptr(), x.data_ptr() + ((R * C - 1) * xp + N) * x.element_size()
        y0, y1 = out.data_ptr(), out.data_ptr() + ((R * C - 1) * op + n_out) * 4
        if x0 < y1 and y0 < x1:
            raise ValueError("out overlaps x: resampling in place is not supported (a workgroup's outputs would "
                             "overwrite inputs its neighbours still read)")
    _lib.check(_lib.load().eegnet_resample(
        _ptr(x), ctypes.c_int(is64), ctypes.c_int64(R * C), ctypes.c_int64(N), ctypes.c_int64(xp), _ptr(taps),
        ctypes.c_int(L), ctypes.c_int(up), ctypes.c_int(down), ctypes.c_int(RESAMPLE_ENDS[ends]), _ptr(out),
        ctypes.c_int64(op), ctypes.c_int64(n_before), _ptr(hist_in), _ptr(hist_out), ctypes.c_int(mode), _stream()),
        "eegnet_resample")
    return out


def forward_eval_windows_at(shape: Shape, flat_params, bn_flat, rec, starts, rec_index=None):
    """Eval-mode forward of the T-sample windows a table places (eegnet_forward_eval_windows_at): window w is
    samples [starts[w], starts[w] + T) of recording rec_index[w] (None: recording 0).  ``rec`` as
    ``forward_eval_windows`` takes it; ``starts`` int64 [W] and ``rec_index`` int32 [W] are contiguous device
    tensors the host never reads -- the kernel clamps an entry into the recordings.  Returns logits [W, 4],
    each row bit-identical to ``forward_eval`` on that window."""
    require_device(rec, "rec")
    if rec.dtype != torch.float32:
        raise RuntimeError(f"forward_eval_windows_at expects float32 input (got {rec.dtype})")
    if rec.dim() not in (2, 3) or rec.shape[-2] != shape.C:
        raise RuntimeError(f"expected a recording [{shape.C}, N] or [R, {shape.C}, N], got {list(rec.shape)}")
    r3 = rec.unsqueeze(0) if rec.dim() == 2 else rec
    R, C, N = r3.shape
    pitch = _row_pitch(r3)
    if pitch is None:
        r3, pitch = r3.contiguous(), N
    for name, t, dt in (("starts", starts, torch.int64), ("rec_index", rec_index, torch.int32)):
        if t is None and name == "rec_index":
            continue
        require_device(t, name)
        if t.dtype != dt or t.dim() != 1 or not t.is_contiguous() or t.device != rec.device:
            raise ValueError(f"{name} must be a contiguous {dt} [W] tensor on {rec.device}")
    W = int(starts.shape[0])
    if rec_index is not None and int(rec_index.shape[0]) != W:
        raise ValueError(f"rec_index holds {int(rec_index.shape[0])} entries, starts {W}")
    logits = torch.empty((W, NCLS), dtype=torch.float32, device=rec.device)
    if W == 0:
        return logits
    _lib.check(_lib.load().eegnet_forward_eval_windows_at(
        ctypes.byref(shape.dims(1)), _ptr(flat_params), _ptr(bn_flat), _ptr(r3), ctypes.c_int64(R), ctypes.c_int64(N),
        ctypes.c_int64(pitch), _ptr(starts), _ptr(rec_index), ctypes.c_int64(W), _ptr(logits), _stream()),
        "eegnet_forward_eval_windows_at")
    return logits


SEED_DLOGITS, SEED_LOGIT, SEED_CE = 0, 1, 2     # include/eegnet_abi.h EEGNET_SEED_*
_SEED_KINDS = {"dlogits": SEED_DLOGITS, "logit": SEED_LOGIT, "ce": SEED_CE}


def input_grad_eval(shape: Shape, flat_params, bn_flat, x, *, kind, dlogits=None, targets=None, out=None):
    """Eval-mode input gradient (eegnet_input_grad_eval, one fused launch): ``(dx, logits)`` with
    dx[b] = d(g[b] . logits[b]) / dx[b].  ``kind``: "dlogits" (g = ``dlogits`` [B, 4]), "logit"
    (g = onehot(``targets``), the trial's own argmax when ``targets`` is None) or "ce"
    (g = softmax(logits) - onehot(``targets``)).  ``out``: a contiguous float32 [B, C, T] tensor to
    receive dx (any 4-byte alignment) instead of a new one."""
    if kind not in _SEED_KINDS:
        raise ValueError(f"kind must be one of {sorted(_SEED_KINDS)} (got {kind!r})")
    require_device(x, "x")
    x = x.contiguous()                # the eval kernels read [B][C][T] rows (no pitch)
    B = x.shape[0]
    if dlogits is not None:
        dlogits = dlogits.to(device=x.device, dtype=torch.float32).contiguous()
        if tuple(dlogits.shape) != (B, NCLS):
            raise ValueError(f"dlogits must be [{B}, {NCLS}] (got {list(dlogits.shape)})")
    if targets is not None:
        targets = targets.to(device=x.device, dtype=torch.int64).contiguous()
        if tuple(targets.shape) != (B,):
            raise ValueError(f"targets must be [{B}] (got {list(targets.shape)})")
    if out is None:
        out = torch.empty_like(x)
    elif (out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous()
          or out.device != x.device):
        raise ValueError(f"out must be a contiguous float32 {list(x.shape)} tensor on {x.device}")
    logits = torch.empty((B, NCLS), dtype=torch.float32, device=x.device)
    if B == 0:
        return out, logits
    d = shape.dims(B)
    _lib.check(_lib.load().eegnet_input_grad_eval(
        ctypes.byref(d), _ptr(flat_params), _ptr(bn_flat), _ptr(x), ctypes.c_int(_SEED_KINDS[kind]),
        _ptr(dlogits), _ptr(targets), _ptr(out), _ptr(logits), _stream()), "eegnet_input_grad_eval")
    return out, logits


def new_frozen_workspace(shape: Shape, B: int, device) -> torch.Tensor:
    """Workspace of ``frozen_step`` for batches of B trials (eegnet_frozen_workspace_bytes)."""
    out = ctypes.c_size_t(0)
    _lib.check(_lib.load().eegnet_frozen_workspace_bytes(ctypes.byref(shape.dims(B)), ctypes.byref(out)),
               "eegnet_frozen_workspace_bytes")
    return torch.zeros(int(out.value), dtype=torch.uint8, device=device)


def forward_frozen(shape: Shape, flat_params, bn_flat, x, seed: int, offset: int, masks=None,
                   p: float | None = None) -> torch.Tensor:
    """Train-mode forward with the BatchNorm layers frozen (eegnet_forward_frozen): running statistics
    used and not written, dropout from ``masks`` or the (seed, offset) generator."""
    x = x.contiguous()
    B = x.shape[0]
    logits = torch.empty((B, NCLS), dtype=torch.float32, device=x.device)
    m2, m3 = masks if masks is not None else (None, None)
    _lib.check(_lib.load().eegnet_forward_frozen(
        ctypes.byref(shape.dims(B, p)), _ptr(flat_params), _ptr(bn_flat), _ptr(x), _ptr(m2), _ptr(m3),
        ctypes.c_uint64(seed), ctypes.c_uint64(offset), _ptr(logits), _stream()), "eegnet_forward_frozen")
    return logits


# include/eegnet_abi.h EEGNET_TRAIN_*: the first trainable module of a partial fine-tuning step, by name
STAGES = ("temporal", "aggregation", "block_2", "classifier")


def stage_index(stage) -> int:
    """0..3 for a stage given as its index or its name in ``STAGES``."""
    if isinstance(stage, str):
        if stage not in STAGES:
            raise ValueError(f"stage must be one of {list(STAGES)} (got {stage!r})")
        return STAGES.index(stage)
    return int(stage)


def trainable_offset(shape: Shape, stage) -> int:
    """eegnet_trainable_offset: the first element of the flat parameters that a frozen-BatchNorm step
    with ``train_from=stage`` trains (everything from that module on; 0 for "temporal").  Host-side
    geometry only."""
    out = ctypes.c_int64(0)
    _lib.check(_lib.load().eegnet_trainable_offset(ctypes.byref(shape.dims(1)), ctypes.c_int(stage_index(stage)),
                                                   ctypes.byref(out)), "eegnet_trainable_offset")
    return int(out.value)


def frozen_step(shape: Shape, flat_params, bn_flat, x, seed: int, offset: int, grads, ws, *, dlogits=None,
                labels=None, masks=None, adam_state=None, step_i32=None, loss=None, logits=None, lr=1e-3,
                betas=(0.9, 0.999), eps=1e-7, p: float | None = None, clamp=True, key_from_step=False,
                train_from=0):
    """One frozen-BatchNorm iteration (eegnet_frozen_step) on the device, no host sync: forward, the
    seed (``dlogits`` [B, 4], or mean cross-entropy against ``labels`` with the loss written to
    ``loss``), backward and all 12 parameter gradients into ``grads``; with ``adam_state`` the Adam
    update follows on the same stream.  ``x`` must be contiguous [B, C, T]; ``ws`` from
    ``new_frozen_workspace``.  ``train_from`` (a stage of ``STAGES``, by index or name) other than 0
    trains the modules from that one on (eegnet_frozen_step_from): the backward stops there, and
    ``grads``, the parameters and the Adam moments below ``trainable_offset`` are not written."""
    if not x.is_contiguous():
        raise ValueError("frozen_step takes a contiguous [B, C, T] x")
    m2, m3 = masks if masks is not None else (None, None)
    stage = stage_index(train_from)
    args = (ctypes.byref(shape.dims(x.shape[0], p)), _ptr(flat_params), _ptr(bn_flat), _ptr(x), _ptr(dlogits),
            _ptr(labels), _ptr(m2), _ptr(m3), ctypes.c_uint64(seed), ctypes.c_uint64(offset), _ptr(grads),
            _ptr(adam_state), _ptr(step_i32), ctypes.c_float(lr), ctypes.c_float(betas[0]),
            ctypes.c_float(betas[1]), ctypes.c_float(eps), _ptr(loss), _ptr(logits), _ptr(ws), _stream(),
            (0 if clamp else NO_CLAMP) | (KEY_FROM_STEP if key_from_step else 0))
    if stage == 0:
        _lib.check(_lib.load().eegnet_frozen_step(*args), "eegnet_frozen_step")
    else:
        _lib.check(_lib.load().eegnet_frozen_step_from(*args, ctypes.c_int(stage)), "eegnet_frozen_step_from")
    return grads


def host_table(t, what, dtype, lo, hi, why):
    """A host table (list, numpy array, CPU tensor) as a CPU tensor of ``dtype``, every entry in [lo, hi]."""
    t = torch.as_tensor(t)
    if t.numel() == 0 and t.dim() == 1:
        t = t.to(torch.int64)                                   # (an empty list comes as float32)
    if t.is_floating_point() or t.dtype == torch.bool or t.dim() != 1:
        raise ValueError(f"{what} must be a 1-D table of integers (got {t.dtype} {list(t.shape)})")
    t = t.to(torch.int64)
    if t.numel() and (int(t.min()) < lo or int(t.max()) > hi):
        bad = int(((t < lo) | (t > hi)).nonzero()[0])
        raise ValueError(f"{what}[{bad}] = {int(t[bad])} is outside [{lo}, {hi}] ({why})")
    return t.to(dtype).contiguous()


def _table(t, what, dtype, device, lo, hi, why):
    """A table of ``frozen_step_windows``: a device tensor (contiguous, of ``dtype``, on ``device``) as it
    lies and unread; a host table checked by ``host_table`` and uploaded."""
    if isinstance(t, torch.Tensor) and t.device.type == "cuda":
        if t.dtype != dtype or t.dim() != 1 or not t.is_contiguous() or t.device != device:
            raise ValueError(f"{what} must be a contiguous {dtype} 1-D tensor on {device}")
        return t
    return host_table(t, what, dtype, lo, hi, why).to(device)


def frozen_step_windows(shape: Shape, flat_params, bn_flat, rec, starts, labels, seed: int, offset: int, grads, ws,
                        *, rec_index=None, sel=None, dlogits=None, masks=None, adam_state=None, step_i32=None,
                        loss=None, logits=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-7, p: float | None = None,
                        clamp=True, key_from_step=False, train_from=0):
    """``frozen_step`` on windows of continuous recordings read in place (eegnet_frozen_step_windows): batch
    row b is table entry e = ``sel[b]`` (b when ``sel`` is None), its x samples [starts[e], starts[e] + T) of
    recording ``rec_index[e]`` (None: recording 0) and its label ``labels[e]``; ``dlogits`` [B, 4] (instead
    of ``labels``), ``logits`` [B, 4] and the ``masks`` are indexed by the batch row.  B = len(sel), else
    len(starts); ``ws`` from ``new_frozen_workspace`` for B.

    ``rec`` [C, N] or [R, C, N] float32 is read where it lies when its last stride is 1 and the recording
    stride is C times the channel stride (a contiguous tensor or a time slice of one, at any 4-byte
    alignment), else through one contiguous copy; it is never written.  A device table (``starts`` /
    ``labels`` / ``sel`` int64, ``rec_index`` int32) is used as it lies and never read by the host, and the
    kernel clamps its entries: a start into [0, N - T], a recording into [0, R), a ``sel`` entry into the
    table.  A host table (list, numpy array, CPU tensor) is checked against those ranges (ValueError) and
    uploaded.

    ``grads`` on the trainable suffix, ``loss``, ``logits``, the parameters and both Adam moments after the
    update and the step counter are bit-identical to ``frozen_step`` on the batch's windows copied out into a
    contiguous [B, C, T] with the labels gathered, for the same (seed, offset) or masks, flags and
    ``train_from``."""
    require_device(rec, "rec")
    if rec.dtype != torch.float32:
        raise RuntimeError(f"frozen_step_windows expects a float32 recording (got {rec.dtype})")
    if rec.dim() not in (2, 3) or rec.shape[-2] != shape.C:
        raise RuntimeError(f"expected a recording [{shape.C}, N] or [R, {shape.C}, N], got {list(rec.shape)}")
    r3 = rec.unsqueeze(0) if rec.dim() == 2 else rec
    R, C, N = r3.shape
    pitch = _row_pitch(r3)
    if pitch is None:
        r3, pitch = r3.contiguous(), N
    dev = rec.device
    starts = _table(starts, "starts", torch.int64, dev, 0, N - shape.T,
                    f"a window of T = {shape.T} samples in a recording of {N}")
    n = int(starts.shape[0])
    if rec_index is not None:
        rec_index = _table(rec_index, "rec_index", torch.int32, dev, 0, R - 1, f"{R} recordings")
    if labels is not None:
        labels = _table(labels, "labels", torch.int64, dev, 0, NCLS - 1, f"{NCLS} classes")
    for name, t in (("rec_index", rec_index), ("labels", labels)):
        if t is not None and int(t.shape[0]) != n:
            raise ValueError(f"{name} holds {int(t.shape[0])} entries, starts {n}")
    if sel is not None:
        sel = _table(sel, "sel", torch.int64, dev, 0, n - 1, f"a table of {n} entries")
    B = n if sel is None else int(sel.shape[0])
    m2, m3 = masks if masks is not None else (None, None)
    _lib.check(_lib.load().eegnet_frozen_step_windows(
        ctypes.byref(shape.dims(B, p)), _ptr(flat_params), _ptr(bn_flat), _ptr(r3), ctypes.c_int64(R),
        ctypes.c_int64(N), ctypes.c_int64(pitch), _ptr(starts), _ptr(rec_index), _ptr(labels), ctypes.c_int64(n),
        _ptr(sel), _ptr(dlogits), _ptr(m2), _ptr(m3), ctypes.c_uint64(seed), ctypes.c_uint64(offset), _ptr(grads),
        _ptr(adam_state), _ptr(step_i32), ctypes.c_float(lr), ctypes.c_float(betas[0]), ctypes.c_float(betas[1]),
        ctypes.c_float(eps), _ptr(loss), _ptr(logits), _ptr(ws), _stream(),
        (0 if clamp else NO_CLAMP) | (KEY_FROM_STEP if key_from_step else 0), ctypes.c_int(stage_index(train_from))),
        "eegnet_frozen_step_windows")
    return grads


def forward_eval_bf16(shape: Shape, flat_params, bn_flat, x) -> torch.Tensor:
    """Eval-mode forward on bf16 input (bf16 MFMA operands, fp32 accumulation, fp32 logits)."""
    if x.dtype != torch.bfloat16:
        raise RuntimeError(f"forward_eval_bf16 expects bfloat16 input (got {x.dtype})")
    x = x.contiguous()
    B = x.shape[0]
    logits = torch.empty((B, NCLS), dtype=torch.float32, device=x.device)
    d = shape.dims(B)
    _lib.check(_lib.load().eegnet_forward_eval_bf16(
        ctypes.byref(d), _ptr(flat_params), _ptr(bn_flat), _ptr(x), _ptr(logits), _stream()),
        "eegnet_forward_eval_bf16")
    return logits


def adam_step(params, grads, exp_avg, exp_avg_sq, step_i32, lr=1e-3, betas=(0.9, 0.999), eps=1e-7):
    _lib.check(_lib.load().eegnet_adam_step(
        ctypes.c_int64(params.numel()), _ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq),
        _ptr(step_i32), ctypes.c_float(lr), ctypes.c_float(betas[0]), ctypes.c_float(betas[1]),
        ctypes.c_float(eps), _stream()), "eegnet_adam_step")


def x_pitch_of(x: torch.Tensor) -> int:
    """eegnet_dims.x_pitch for x: 0 for a contiguous [B, C, T] tensor, the channel-row pitch for a
    [B, C, T] view of [B, C, pitch] rows (``pad_x_rows``)."""
    if x.is_contiguous():
        return 0
    B, C, T = x.shape
    if x.stride(2) != 1 or x.stride(0) != C * x.stride(1) or x.stride(1) < T:
        raise ValueError("x must be a contiguous [B, C, T] tensor or a [B, C, T] view of [B, C, pitch] rows")
    if x.data_ptr() % 16:
        # pitched rows go to LDS in 16-byte DMA units: every row must start 16-byte aligned
        raise ValueError("a pitched x view must start 16-byte aligned")
    return int(x.stride(1))


def pad_x_rows(x: torch.Tensor, pitch: int) -> torch.Tensor:
    """A copy of x [N, C, T] with its rows at ``pitch`` floats (zeros after T), returned as the
    [N, C, T] view the training entry points take (x_pitch_of): 22 x 257 trials then load in 16-byte
    units."""
    N, C, T = x.shape
    if pitch == T:
        return x.contiguous()
    xp = torch.zeros((N, C, pitch), dtype=x.dtype, device=x.device)
    xp[:, :, :T] = x
    return xp[:, :, :T]


def train_step(shape: Shape, flat_params, bn_flat, x, labels, seed: int, offset: int, grads,
               adam_state, step_i32, ws, loss, logits=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-7,
               p: float | None = None, clamp=True, nbt=None, key_from_step=False):
    """One fused hot-loop iteration (model.py:141-148) on the device, no host sync.
    ``adam_state=None`` stops after the gradients (data-parallel)."""
    d = shape.dims(x.shape[0], p, x_pitch_of(x))
    _lib.check(_lib.load().eegnet_train_step(
        ctypes.byref(d), _ptr(flat_params), _ptr(bn_flat), _ptr(x), _ptr(labels),
        ctypes.c_uint64(seed), ctypes.c_uint64(offset), _ptr(grads), _ptr(adam_state),
        _ptr(step_i32), ctypes.c_float(lr), ctypes.c_float(betas[0]), ctypes.c_float(betas[1]),
        ctypes.c_float(eps), _ptr(loss), _ptr(logits), _ptr(ws), _stream(),
        (0 if clamp else NO_CLAMP) | (KEY_FROM_STEP if key_from_step else 0),
        _ptr(nbt)), "eegnet_train_step")


def train_stage(shape: Shape, stage: int, norm_batch: int, flat_params, bn_flat, x, labels, seed: int,
                offset: int, grads, adam_state, step_i32, ws, loss, lr=1e-3, betas=(0.9, 0.999), eps=1e-7,
                p: float | None = None, nbt=None):
    """eegnet_train_stage: stage 2k = pass k with its finalize deferred (sums left in ``ws``),
    stage 2k + 1 = pass k's finalize on the (all-reduced) sums; statistics normalised by
    ``norm_batch`` (the global batch of a synchronised-BatchNorm data-parallel step)."""
    d = shape.dims(x.shape[0], p, x_pitch_of(x))
    _lib.check(_lib.load().eegnet_train_stage(
        ctypes.byref(d), ctypes.c_int(stage), ctypes.c_int64(norm_batch), _ptr(flat_params), _ptr(bn_flat),
        _ptr(x), _ptr(labels), ctypes.c_uint64(seed), ctypes.c_uint64(offset), _ptr(grads), _ptr(adam_state),
        _ptr(step_i32), ctypes.c_float(lr), ctypes.c_float(betas[0]), ctypes.c_float(betas[1]),
        ctypes.c_float(eps), _ptr(loss), _ptr(ws), _stream(), 0, _ptr(nbt)), "eegnet_train_stage")


def stage_sums(shape: Shape, B: int, ws: torch.Tensor, p: float | None = None) -> list[torch.Tensor]:
    """The five float64 views of ``ws`` (a uint8 workspace tensor) that stages 0, 2, 4, 6, 8 leave
    their sums in (one buffer, reused by every pass: view k holds pass k's sums after stage 2k)."""
    d = shape.dims(B, p)
    lib = _lib.load()
    out = []
    for k in range(5):
        off, n = ctypes.c_size_t(0), ctypes.c_int(0)
        _lib.check(lib.eegnet_stage_sums(ctypes.byref(d), ctypes.c_int(k), ctypes.byref(off), ctypes.byref(n)),
                   "eegnet_stage_sums")
        out.append(ws[off.value:off.value + 8 * n.value].view(torch.float64))
    return out


def x_stats(shape: Shape, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """eegnet_x_stats: the per-trial, parameter-free BN1 statistics of x [N, C, T] (contiguous or a
    pad_x_rows view) as a [N, width] float32 device tensor -- the lag sums of each trial's zero-padded
    rows over the channels, its window-0 sample sum and the 'same' padding's edge products / sums.
    A fold whose training set is fixed reads a batch's rows of it instead of recomputing them."""
    require_device(x, "x")
    lib = _lib.load()
    N = x.shape[0]
    d = shape.dims(1, None, x_pitch_of(x))
    width = int(lib.eegnet_x_stats_width(ctypes.byref(d)))
    if width <= 0:
        _lib.check(width, "eegnet_x_stats_width")
    if out is None:
        out = torch.empty((N, width), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (N, width) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 [{N}, {width}] tensor")
    if N:
        _lib.check(lib.eegnet_x_stats(ctypes.byref(d), ctypes.c_int64(N), _ptr(x), _ptr(out), _stream()),
                   "eegnet_x_stats")
    return out


def fold_table(entries, device) -> torch.Tensor:
    """Device array of ``eegnet_fold`` entries (a uint8 tensor holding the packed structs).
    ``entries``: dicts with the eegnet_fold fields as tensors (or None) and ``seed`` as an int."""
    n = len(entries)
    arr = (_lib.Fold * n)()
    for i, e in enumerate(entries):
        for name, _ in _lib.Fold._fields_:
            if name == "seed":
                continue
            t = e.get(name)
            setattr(arr[i], name, 0 if t is None else t.data_ptr())
        arr[i].seed = int(e["seed"]) & ((1 << 64) - 1)
    raw = bytes(arr)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


def train_step_folds(shape: Shape, B: int, table: torch.Tensor, nfolds: int, row0: int, slot: int,
                     offset: int = 0, lr=1e-3, betas=(0.9, 0.999), eps=1e-7, p: float | None = None,
                     x_pitch: int = 0):
    """eegnet_train_step_folds: one fused step of ``nfolds`` independent models in one launch per
    pass (fold index = grid y).  ``table`` from fold_table(); every fold trains on rows
    [row0, row0 + B) of its own x / labels and writes its loss to losses[slot].  ``x_pitch``: the
    row pitch of every fold's x (0: contiguous [N, C, T]; pad_x_rows)."""
    d = shape.dims(B, p, x_pitch)
    _lib.check(_lib.load().eegnet_train_step_folds(
        ctypes.byref(d), ctypes.c_int(nfolds), _ptr(table), ctypes.c_int64(row0), ctypes.c_int64(slot),
        ctypes.c_uint64(offset), ctypes.c_float(lr), ctypes.c_float(betas[0]), ctypes.c_float(betas[1]),
        ctypes.c_float(eps), _stream()), "eegnet_train_step_folds")


def frozen_step_folds(shape: Shape, B: int, table: torch.Tensor, nfolds: int, row0: int, slot: int,
                      offset: int = 0, lr=1e-3, betas=(0.9, 0.999), eps=1e-7, p: float | None = None,
                      clamp=True, train_from=0):
    """eegnet_frozen_step_folds: one frozen-BatchNorm iteration (``frozen_step`` with labels and
    ``key_from_step``) of ``nfolds`` independent models in four launches, the fold index in the grid's
    y.  ``table`` from fold_table(); every fold trains on rows perm[row0 : row0 + B] (rows
    [row0, row0 + B) without a perm) of its own contiguous x / labels, writes its loss to
    losses[slot] and keeps its partial rows in its own ``ws`` (``new_frozen_workspace``); a fold
    without ``adam_state`` stops after its gradients.  BN buffers are read only.  ``train_from`` other
    than 0: every fold trains the modules from that stage on (eegnet_frozen_step_folds_from)."""
    stage = stage_index(train_from)
    args = (ctypes.byref(shape.dims(B, p)), ctypes.c_int(nfolds), _ptr(table), ctypes.c_int64(row0),
            ctypes.c_int64(slot), ctypes.c_uint64(offset), ctypes.c_float(lr), ctypes.c_float(betas[0]),
            ctypes.c_float(betas[1]), ctypes.c_float(eps), ctypes.c_int(0 if clamp else NO_CLAMP), _stream())
    if stage == 0:
        _lib.check(_lib.load().eegnet_frozen_step_folds(*args), "eegnet_frozen_step_folds")
    else:
        _lib.check(_lib.load().eegnet_frozen_step_folds_from(*args, ctypes.c_int(stage)),
                   "eegnet_frozen_step_folds_from")


def eval_fold_table(entries, device) -> torch.Tensor:
    """Device array of ``eegnet_eval_fold`` entries (a uint8 tensor holding the packed structs).
    ``entries``: dicts with the eegnet_eval_fold pointer fields as tensors (or None) and ``n`` as an
    int."""
    arr = (_lib.EvalFold * len(entries))()
    for i, e in enumerate(entries):
        for name, _ in _lib.EvalFold._fields_:
            if name == "n":
                continue
            t = e.get(name)
            setattr(arr[i], name, 0 if t is None else t.data_ptr())
        arr[i].n = int(e["n"])
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


def eval_folds(shape: Shape, table: torch.Tensor, nfolds: int, max_n: int, batch: int = 64, slot: int = 0):
    """eegnet_eval_folds: the eval forward, per-trial cross-entropy and argmax of ``nfolds`` models on
    their own held-out sets in one launch, then each fold's validation loss (the mean of the per-batch CE
    means over batches of ``batch`` trials, float64) and correct count into loss[slot] / correct[slot].
    ``table`` from eval_fold_table(); ``max_n`` the largest ``n`` in it.  No host synchronisation."""
    _lib.check(_lib.load().eegnet_eval_folds(
        ctypes.byref(shape.dims(1)), ctypes.c_int(nfolds), _ptr(table), ctypes.c_int64(max_n),
        ctypes.c_int(batch), ctypes.c_int64(slot), _stream()), "eegnet_eval_folds")
