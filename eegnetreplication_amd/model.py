"""Drop-in for ``eegnet_repl.model`` (PraKesEy/EEGNetReplication src/eegnet_repl/model.py).

``EEGNet`` keeps the reference's submodule tree, parameter/buffer names and shapes
(model.py:22-84) so ``state_dict`` round-trips with reference checkpoints and any ``torch.optim``
optimizer can step it; the grad-clamp hooks of model.py:44 and model.py:84 are registered the same
way.  ``forward`` never runs those submodules: it runs the MI355X HIP kernels through
``libeegnet_hip.so`` (train mode: 5-pass fused step; eval mode: one fused inference kernel).

``train`` / ``evaluate_model`` mirror model.py:101-189 / 191-227 (same arguments, returns, logging
cadence and the F4 "best model aliases the live weights" behaviour), with the epoch loss and
accuracy accumulated on the device (one host sync per epoch instead of one per batch).  When the
optimizer is ``torch.optim.Adam`` and the loss is a default ``nn.CrossEntropyLoss`` the whole step
(forward, CE, backward, clamps, Adam) runs as one fused device sequence.

``model.freeze_bn()`` switches the train-mode forward / backward and the fused step to frozen
BatchNorm (running statistics used and left untouched, dropout on) for fine-tuning a trained model
on a few calibration trials: one fused trial-parallel launch instead of the five passes.
"""

from __future__ import annotations

import logging

import torch
import torch.nn as nn

from . import ops
from .ops import Shape, require_device

logger = logging.getLogger("eegnet_repl")


class EEGNet(nn.Module):
    """EEGNet-F1,D (Lawhern et al. 2018) with the reference's module layout (model.py:12-99).

    C, T: channels and samples per trial; F1 temporal filters; D depth multiplier; p dropout.
    ``K1`` (temporal kernel length) defaults to the reference's 32 (model.py:26).
    """

    def __init__(self, C, T, F1=8, D=2, p=0.5, K1=32):
        super().__init__()
        F2 = F1 * D
        self.temporal = nn.Sequential(
            nn.Conv2d(1, F1, kernel_size=(1, K1), padding="same", bias=False),
            nn.BatchNorm2d(F1))
        self.spatial = nn.Conv2d(F1, D * F1, kernel_size=(C, 1), padding="valid", groups=F1,
                                 bias=False)
        self.spatial.weight.register_hook(lambda g: torch.clamp(g, min=-1.0, max=1.0))
        self.aggregation = nn.Sequential(nn.BatchNorm2d(D * F1), nn.ELU(),
                                         nn.AvgPool2d(kernel_size=(1, 4)), nn.Dropout(p=p))
        self.block_2 = nn.Sequential(
            nn.Conv2d(D * F1, D * F1, kernel_size=(1, 16), padding="same", groups=D * F1,
                      bias=False),
            nn.Conv2d(D * F1, F2, kernel_size=(1, 1), padding="same", bias=False),
            nn.BatchNorm2d(F2), nn.ELU(), nn.AvgPool2d(kernel_size=(1, 8)), nn.Dropout(p=p),
            nn.Flatten())
        self.classifier = nn.Linear(F2 * (T // 32), 4, bias=True)
        self.classifier.weight.register_hook(lambda g: torch.clamp(g, min=-0.25, max=0.25))
        self.C, self.T, self.F1, self.D, self.K1 = C, T, F1, D, K1
        self._masks = None
        self._rng_offset = 0
        self.bn_frozen = False
        self._flatten()

    # -- flat device layout -----------------------------------------------------------------
    def _bns(self):
        return (self.temporal[1], self.aggregation[0], self.block_2[2])

    def _flatten(self):
        """Re-home every parameter (and BN running stat) as a view of one flat fp32 buffer, in
        named_parameters() order -- the layout of include/eegnet_abi.h.  Parameter identity is
        kept (``.data`` is rebound), so optimizers built before ``.to()`` keep working."""
        # (module, attribute) of every parameter, in named_parameters() order: _flat_ok checks that
        # each slot still holds the Parameter re-homed here (a caller may assign a new one)
        self._pslots = [(mod, name) for mod in self.modules() for name, q in mod._parameters.items()
                        if q is not None]
        params = [mod._parameters[name] for mod, name in self._pslots]
        assert len(params) == len(list(self.parameters()))
        dev = params[0].device
        n = sum(p.numel() for p in params)
        flat = torch.empty(n, dtype=torch.float32, device=dev)
        o = 0
        for p in params:
            k = p.numel()
            flat[o:o + k].copy_(p.data.reshape(-1))
            p.data = flat[o:o + k].view(p.shape)
            o += k
        self._flat = flat
        bufs = []
        for bn in self._bns():
            bufs += [bn.running_mean, bn.running_var]
        nb = sum(b.numel() for b in bufs)
        bflat = torch.empty(nb, dtype=torch.float32, device=dev)
        o = 0
        views = []
        for b in bufs:
            k = b.numel()
            bflat[o:o + k].copy_(b.reshape(-1))
            views.append(bflat[o:o + k])
            o += k
        for bn, (rm, rv) in zip(self._bns(), zip(views[0::2], views[1::2])):
            bn.running_mean = rm
            bn.running_var = rv
        self._bn_flat = bflat
        # the three num_batches_tracked counters as views of one int64[3] buffer: the HIP forward
        # increments them in-kernel (no per-step host-side add_ launches)
        nflat = torch.zeros(3, dtype=torch.int64, device=dev)
        for i, bn in enumerate(self._bns()):
            if bn.num_batches_tracked is not None:
                nflat[i:i + 1].copy_(bn.num_batches_tracked.reshape(1))
                bn.num_batches_tracked = nflat[i:i + 1].view(())
        self._nbt_flat = nflat
        # the tensors _flat_ok checks, gathered once (a module-tree walk per call costs ~25 us of
        # host time, the whole budget of a batch-64 step)
        self._plist = params
        self._blist = [t for bn in self._bns() for t in (bn.running_mean, bn.running_var)]
        self._nlist = [bn.num_batches_tracked for bn in self._bns()]
        # every view's expected address, computed once: _flat_ok compares data_ptr() only
        base, o, ptrs = flat.data_ptr(), 0, []
        for q in params:
            ptrs.append(base + 4 * o)
            o += q.numel()
        b = bflat.data_ptr()
        bptrs, o = [], 0
        for t in self._blist:
            bptrs.append(b + 4 * o)
            o += t.numel()
        self._pexpect = list(zip(params, ptrs))
        self._bexpect = list(zip(self._blist, bptrs))
        self._nexpect = [(t, nflat.data_ptr() + 8 * i) for i, t in enumerate(self._nlist) if t is not None]
        self._shape_cache = None

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        if all(p.dtype == torch.float32 for p in self.parameters()):
            self._flatten()
        return self

    def _flat_ok(self) -> bool:
        """Every parameter / BN buffer still a view of the flat buffers (a caller may rebind
        ``p.data``, assign a new Parameter or replace a buffer)."""
        for (mod, name), p in zip(self._pslots, self._plist):
            if mod._parameters.get(name) is not p:
                return False
        bns = self._bns()
        for i, bn in enumerate(bns):
            if bn.running_mean is not self._blist[2 * i] or bn.running_var is not self._blist[2 * i + 1] \
                    or bn.num_batches_tracked is not self._nlist[i]:
                return False
        for p, ptr in self._pexpect:
            if p.data_ptr() != ptr or not p.is_contiguous():
                return False
        for t, ptr in self._bexpect:
            if t.data_ptr() != ptr:
                return False
        for t, ptr in self._nexpect:
            if t.data_ptr() != ptr:
                return False
        return True

    def flat_views(self):
        """(flat parameters, flat BN buffers, num_batches_tracked buffer) after ONE layout check (a
        fused step needs all three; the check is the larger part of its host time)."""
        if not self._flat_ok():
            self._flatten()
        return self._flat, self._bn_flat, self._nbt_flat

    def flat_parameters(self) -> torch.Tensor:
        if not self._flat_ok():
            self._flatten()
        return self._flat

    def flat_bn_buffers(self) -> torch.Tensor:
        if not self._flat_ok():
            self._flatten()
        return self._bn_flat

    def flat_num_batches_tracked(self) -> torch.Tensor:
        """int64[3] device buffer behind the three BatchNorm2d.num_batches_tracked counters."""
        if not self._flat_ok():
            self._flatten()
        return self._nbt_flat

    @property
    def shape(self) -> Shape:
        bn = self.temporal[1]
        if bn.momentum is None:
            raise NotImplementedError("BatchNorm momentum=None (cumulative average) is not supported")
        key = (float(self.aggregation[3].p), float(bn.eps), float(bn.momentum))
        if self._shape_cache is None or self._shape_cache[0] != key:
            self._shape_cache = (key, Shape(C=self.C, T=self.T, F1=self.F1, D=self.D, K1=self.K1,
                                            p=key[0], eps=key[1], momentum=key[2]))
        return self._shape_cache[1]

    # -- frozen BatchNorm (fine-tuning) ---------------------------------------------------------
    def freeze_bn(self, mode: bool = True):
        """Freeze (or release) the three BatchNorm layers for fine-tuning, as ``bn.eval()`` on a stock
        module: while set and the model is in train mode, the forward normalises with the running
        statistics and writes neither them nor ``num_batches_tracked``; dropout stays on and
        ``backward()`` fills all 12 ``param.grad`` (one fused launch, F1*D <= 16).  A plain attribute
        (``bn_frozen``), not a buffer: ``train()`` / ``eval()`` / ``to()`` leave it alone, it is not in
        ``state_dict``, and it has no effect in eval mode.  Returns self."""
        self.bn_frozen = bool(mode)
        return self

    # -- partial fine-tuning: a frozen prefix of the layers ----------------------------------------
    # the first parameter (named_parameters() order) of each stage of ops.STAGES
    _STAGE_FIRST = {"temporal": "temporal.0.weight", "aggregation": "aggregation.0.weight",
                    "block_2": "block_2.0.weight", "classifier": "classifier.weight"}

    def train_from(self, stage):
        """Train the modules from ``stage`` on and freeze every module before it: ``"temporal"``
        (everything trains), ``"aggregation"`` (the temporal block and the spatial filters are kept),
        ``"block_2"`` (and the second BatchNorm's affine pair) or ``"classifier"`` (the classifier
        alone).  Sets ``requires_grad`` False on the prefix and True on the suffix, as a caller would on
        a stock module.  With ``freeze_bn()`` set, the train-mode backward, ``FusedTrainer`` / ``train()``
        and ``FrozenFoldBatch`` then run a backward that stops where the trainable layers stop, leave
        ``grad`` of the frozen parameters ``None`` and never write them or their Adam state.  Without
        ``freeze_bn()`` nothing changes: the five-pass train step ignores ``requires_grad`` (it computes
        and, fused, applies all 12 gradients), as it always has.  Returns self."""
        s = ops.stage_index(stage)
        if not 0 <= s < len(ops.STAGES):
            raise ValueError(f"stage must be one of {list(ops.STAGES)} (got {stage!r})")
        first = self._STAGE_FIRST[ops.STAGES[s]]
        on = False
        for name, p in self.named_parameters():
            on = on or name == first
            p.requires_grad_(on)
        return self

    def trainable_stage(self) -> int:
        """The stage (index into ``ops.STAGES``) the parameters' ``requires_grad`` flags spell: 0 when
        every parameter trains, else the first trainable module of a frozen-prefix pattern as
        ``train_from`` sets it.  Any other pattern raises NotImplementedError."""
        named = list(self.named_parameters())
        flags = [p.requires_grad for _, p in named]
        if all(flags):
            return 0
        starts = {name: i for i, name in enumerate(self._STAGE_FIRST.values())}
        first = flags.index(True) if any(flags) else None
        if first is None:
            bad, why = named[-1][0], "no parameter is trainable"
        elif named[first][0] not in starts:
            bad, why = named[first][0], "it is trainable while the parameters before it are frozen, and no stage begins there"
        elif not all(flags[first:]):
            bad = named[first + flags[first:].index(False)][0]
            why = f"it is frozen behind the trainable {named[first][0]}"
        else:
            return starts[named[first][0]]
        raise NotImplementedError(
            f"partial fine-tuning trains a suffix of the layers: {bad} does not fit ({why}); the supported "
            f"stages are {', '.join(ops.STAGES)} (EEGNet.train_from)")

    def _stage_checked(self) -> int:
        """``trainable_stage()`` for a caller that has just made the layout check (``flat_views``): the
        usual case, every parameter trainable, without walking the module tree."""
        for p in self._plist:
            if not p.requires_grad:
                return self.trainable_stage()
        return 0

    # -- dropout control (test hook) ------------------------------------------------------------
    def set_dropout_masks(self, m2, m3):
        """Inject keep-masks ([B,F2,T//4], [B,F2,T//128] uint8, 1 = keep) for the train-mode
        forward/backward, or ``None`` to return to the on-device generator."""
        self._masks = None if m2 is None else (m2.to(torch.uint8).contiguous(),
                                               m3.to(torch.uint8).contiguous())

    def next_dropout_key(self):
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self._rng_offset += 1
        return seed, self._rng_offset

    # -- forward -------------------------------------------------------------------------------
    def forward(self, x):
        """Logits [B, 4] of x [B, C, T] on the HIP kernels.

        In eval mode an input with ``requires_grad`` (grad enabled, F1*D <= 16) gets a differentiable
        forward: ``backward()`` fills ``x.grad`` with one fused eval-mode input-gradient launch.  That
        node is differentiable with respect to x ONLY -- the parameters are not its inputs, so every
        ``param.grad`` stays ``None``; parameter gradients come from the train-mode forward.  Train
        mode does not provide input gradients (they need the batch-global BatchNorm backward)."""
        require_device(x, "EEGNet input")
        if x.dtype == torch.bfloat16 and not self.training:
            # bf16 batched inference: bf16 MFMA operands, fp32 accumulation
            if x.dim() != 3 or x.shape[1] != self.C or x.shape[2] != self.T:
                raise RuntimeError(f"expected input [B,{self.C},{self.T}], got {list(x.shape)}")
            with torch.no_grad():
                return ops.forward_eval_bf16(self.shape, self.flat_parameters(), self._bn_flat, x)
        if x.dtype != torch.float32:
            raise RuntimeError(f"EEGNet expects float32 input (got {x.dtype}; bfloat16 is accepted in "
                               f"eval mode); the reference casts with signals.float() (model.py:137)")
        if x.dim() != 3 or x.shape[1] != self.C or x.shape[2] != self.T:
            raise RuntimeError(f"expected input [B,{self.C},{self.T}], got {list(x.shape)}")
        if x.requires_grad:
            if self.training or not torch.is_grad_enabled() or self.F1 * self.D > 16:
                raise NotImplementedError("gradients with respect to the EEG input are not provided")
            flat = self.flat_parameters()
            require_device(flat, "EEGNet parameters")
            return _EvalInputGradFn.apply(x, self, self.shape)
        x = x.contiguous()
        flat = self.flat_parameters()
        require_device(flat, "EEGNet parameters")
        shape = self.shape
        params = list(self.parameters())
        if self.training:
            seed, offset = self.next_dropout_key()
            masks = self._masks
            if masks is not None and masks[0].shape[0] != x.shape[0]:
                raise RuntimeError("injected dropout masks do not match the batch size")
            if getattr(self, "bn_frozen", False):
                # the stage the backward will run at (an unsupported pattern raises here: nothing ran); 0
                # when nothing will be differentiated
                diff = torch.is_grad_enabled() and any(p.requires_grad for p in params)
                stage = self._stage_checked() if diff else 0
                return _FrozenTrainFn.apply(x, self, shape, seed, offset, masks, stage, *params)
            return _TrainFn.apply(x, self, shape, seed, offset, masks, *params)
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _EvalFn.apply(x, self, shape, *params)
        return ops.forward_eval(shape, flat, self._bn_flat, x)


class _TrainFn(torch.autograd.Function):
    """Train-mode EEGNet step as one autograd node: forward = passes A,B,C of the HIP pipeline,
    backward(dlogits) = passes C,D,E + finalizes (grads already clamped as model.py:44,84)."""

    @staticmethod
    def forward(ctx, x, mod, shape, seed, offset, masks, *params):
        ws = ops.new_workspace(shape, x.shape[0], x.device)
        flat = mod.flat_parameters().clone()
        logits = ops.forward_train(shape, flat, mod.flat_bn_buffers(), x, ws, seed, offset,
                                   masks=masks, nbt=mod.flat_num_batches_tracked())
        ctx.shape, ctx.seed, ctx.offset, ctx.masks = shape, seed, offset, masks
        ctx.param_shapes = [p.shape for p in params]
        ctx.save_for_backward(x, ws, flat)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        x, ws, flat = ctx.saved_tensors
        g = ops.backward(ctx.shape, flat, x, ws, ctx.seed, ctx.offset,
                         dlogits=dlogits.contiguous().float(), masks=ctx.masks)
        out, o = [], 0
        for s in ctx.param_shapes:
            k = 1
            for d in s:
                k *= d
            out.append(g[o:o + k].view(s))
            o += k
        return (None, None, None, None, None, None, *out)


def _not_supported(e: RuntimeError):
    """The library's "... is not supported" rejections (wide dims) as NotImplementedError."""
    if "is not supported" in str(e):
        raise NotImplementedError(str(e)) from None
    raise e


class _FrozenTrainFn(torch.autograd.Function):
    """Train-mode step with the BatchNorm layers frozen (EEGNet.freeze_bn) as one autograd node:
    forward = the forward-only variant of the fused frozen kernel, backward(dlogits) = one
    eegnet_frozen_step (gradients clamped as model.py:44,84, no Adam).  The backward differentiates the
    forward that ran: parameters, running statistics, masks and dropout key are those of forward time."""

    @staticmethod
    def forward(ctx, x, mod, shape, seed, offset, masks, stage, *params):
        flat = mod.flat_parameters().clone()
        bn_flat = mod.flat_bn_buffers().clone()
        try:
            logits = ops.forward_frozen(shape, flat, bn_flat, x, seed, offset, masks=masks)
        except RuntimeError as e:
            _not_supported(e)
        ctx.shape, ctx.seed, ctx.offset, ctx.masks = shape, seed, offset, masks
        ctx.param_shapes = [p.shape for p in params]
        ctx.stage = stage
        ctx.save_for_backward(x, flat, bn_flat)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        x, flat, bn_flat = ctx.saved_tensors
        ws = ops.new_frozen_workspace(ctx.shape, x.shape[0], x.device)
        g = ops.frozen_step(ctx.shape, flat, bn_flat, x, ctx.seed, ctx.offset, torch.empty_like(flat), ws,
                            dlogits=dlogits.contiguous().float(), masks=ctx.masks, train_from=ctx.stage)
        # the cut step leaves g below the trainable suffix unwritten: None for the frozen parameters
        off = ops.trainable_offset(ctx.shape, ctx.stage) if ctx.stage else 0
        out, o = [], 0
        for s in ctx.param_shapes:
            k = 1
            for d in s:
                k *= d
            out.append(g[o:o + k].view(s) if o >= off else None)
            o += k
        return (None, None, None, None, None, None, None, *out)


class _EvalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mod, shape, *params):
        return ops.forward_eval(shape, mod.flat_parameters(), mod.flat_bn_buffers(), x)

    @staticmethod
    def backward(ctx, dlogits):
        raise NotImplementedError(
            "backward through an eval-mode EEGNet forward is not provided; call model.train() "
            "for a differentiable forward")


class _EvalInputGradFn(torch.autograd.Function):
    """Eval-mode forward that is differentiable with respect to x only: forward = the fused inference
    kernel, backward(dlogits) = one eegnet_input_grad_eval launch (EEGNET_SEED_DLOGITS).  The
    parameters are not inputs of the node, so they receive no gradient.  The backward runs on the
    parameters and running statistics as they are at that moment."""

    @staticmethod
    def forward(ctx, x, mod, shape):
        xc = x.detach().contiguous()
        ctx.mod, ctx.shape = mod, shape
        ctx.save_for_backward(xc)
        return ops.forward_eval(shape, mod.flat_parameters(), mod.flat_bn_buffers(), xc)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogits):
        (x,) = ctx.saved_tensors
        mod = ctx.mod
        dx, _ = ops.input_grad_eval(ctx.shape, mod.flat_parameters(), mod.flat_bn_buffers(), x,
                                    kind="dlogits", dlogits=dlogits)
        return dx, None, None


def saliency(model, x, targets=None, kind="logit"):
    """Input gradient of an EEGNet decision: ``(dx, logits)`` for x [B, C, T], in one fused launch and
    with no autograd graph.  ``kind="logit"``: dx[b] = d logits[b, targets[b]] / dx[b], the predicted
    class when ``targets`` is None; ``kind="ce"``: the gradient of the trial's cross-entropy against
    ``targets``.  Always eval semantics (running statistics, no dropout), whatever ``model.training``
    is, and that mode is left untouched.  F1*D > 16 models raise NotImplementedError."""
    if kind not in ("logit", "ce"):
        raise ValueError(f"kind must be 'logit' or 'ce' (got {kind!r})")
    if kind == "ce" and targets is None:
        raise ValueError("kind='ce' needs targets")
    require_device(x, "EEGNet input")
    if x.dtype != torch.float32:
        raise RuntimeError(f"saliency expects float32 input (got {x.dtype})")
    if x.dim() != 3 or x.shape[1] != model.C or x.shape[2] != model.T:
        raise RuntimeError(f"expected input [B,{model.C},{model.T}], got {list(x.shape)}")
    flat = model.flat_parameters()
    require_device(flat, "EEGNet parameters")
    with torch.no_grad():
        try:
            return ops.input_grad_eval(model.shape, flat, model.flat_bn_buffers(), x.detach(), kind=kind,
                                       targets=targets)
        except RuntimeError as e:
            if "is not supported" in str(e):
                raise NotImplementedError(str(e)) from None
            raise


def relevance_maps(model, loader, method="gradxinput"):
    """Per-class input-relevance maps [4, C, T]: the mean over the trials of each TRUE class of
    |dx * x| (``method="gradxinput"``) or |dx| (``"grad"``), dx being the saliency of the true-class
    logit, over a loader of (signals, labels).  Accumulated on the device in float64 with one host
    sync at the end; a class without trials gets a zero map."""
    if method not in ("gradxinput", "grad"):
        raise ValueError(f"method must be 'gradxinput' or 'grad' (got {method!r})")
    device = _device()
    model = model.to(device)
    acc = torch.zeros((ops.NCLS, model.C, model.T), dtype=torch.float64, device=device)
    cnt = torch.zeros(ops.NCLS, dtype=torch.float64, device=device)
    for signals, labels in loader:
        signals = signals.float().to(device, non_blocking=True)
        labels = labels.to(device, non_blocking=True).long()
        dx, _ = saliency(model, signals, targets=labels, kind="logit")
        rel = (dx * signals if method == "gradxinput" else dx).abs().double()
        acc.index_add_(0, labels, rel)
        cnt += torch.bincount(labels, minlength=ops.NCLS)[:ops.NCLS]
    out = (acc / cnt.clamp(min=1.0).view(-1, 1, 1)).float()
    return out.cpu()


# ----------------------------------------------------------------------------------------------
# sliding windows over continuous recordings (pseudo-online decoding, cropped evaluation)
# ----------------------------------------------------------------------------------------------
def window_starts(N, T, hop) -> torch.Tensor:
    """Start sample of every T-sample window, ``hop`` samples apart, of a recording of N samples:
    window w is samples [w hop, w hop + T); there are (N - T) // hop + 1 of them."""
    N, T, hop = int(N), int(T), int(hop)
    if hop < 1:
        raise ValueError(f"hop must be >= 1 (got {hop})")
    if N < T:
        raise ValueError(f"a recording of {N} samples is shorter than one window (T = {T})")
    return torch.arange(0, N - T + 1, hop, dtype=torch.int64)


def _windows(model, rec, hop, reduce):
    """ops.forward_eval_windows on a model: eval semantics whatever ``model.training`` is."""
    require_device(rec, "EEGNet recording")
    if rec.dtype != torch.float32:
        raise RuntimeError(f"sliding windows expect a float32 recording (got {rec.dtype})")
    if rec.dim() not in (2, 3) or rec.shape[-2] != model.C or rec.shape[-1] < model.T:
        raise RuntimeError(f"expected a recording [{model.C}, N] or [R, {model.C}, N] with N >= {model.T}, "
                           f"got {list(rec.shape)}")
    flat = model.flat_parameters()
    require_device(flat, "EEGNet parameters")
    with torch.no_grad():
        try:
            return ops.forward_eval_windows(model.shape, flat, model.flat_bn_buffers(), rec.detach(), int(hop),
                                            reduce=reduce)
        except RuntimeError as e:
            _not_supported(e)


def sliding_logits(model, rec, hop):
    """Logits of every T-sample window of continuous recordings, a decision every ``hop`` samples:
    [R, W, 4] for ``rec`` [R, C, N] ([W, 4] for [C, N]), W = (N - T) // hop + 1, window w being samples
    [w hop, w hop + T) (``window_starts``).  The recording is read in place (a contiguous tensor or a
    time slice of one; no unfolded copy), and every row is bit-identical to ``model.eval()(window)``.
    Always eval semantics (running statistics, no dropout), whatever ``model.training`` is, and that
    mode is left untouched.  F1*D > 16 models raise NotImplementedError."""
    return _windows(model, rec, hop, False)


def cropped_predict(model, rec, hop):
    """Cropped decoding of long trials: ``(probs, pred, logits)`` with logits as ``sliding_logits``,
    probs [R, 4] the mean over a recording's crops of softmax(logits) (accumulated in float64 on the
    device, in window order) and pred [R] int32 its argmax, the lowest class on a tie ([4] and a 0-d
    tensor for a 2-D ``rec``).  Eval semantics; the mode is left untouched."""
    logits, probs, pred = _windows(model, rec, hop, True)
    return probs, pred, logits


def epoch_starts(onsets, sfreq=128.0, tmin=0.5):
    """Start sample of the epoch of every cue: ``onsets + round(tmin * sfreq)``, an int64 tensor.  With the
    defaults and T = 257 these are the reference's epochs, ``mne.Epochs(tmin=0.5, tmax=2.5)`` at 128 Hz: 257
    samples starting 64 samples after the cue."""
    onsets = torch.as_tensor(onsets)
    if onsets.is_floating_point() or onsets.dtype == torch.bool:
        raise ValueError(f"cue onsets are sample indices: expected integers (got {onsets.dtype})")
    return onsets.to(torch.int64) + int(round(float(tmin) * float(sfreq)))


_host_table = ops.host_table


def epoch_logits(model, rec, starts, rec_index=None):
    """Logits [W, 4] of the T-sample windows a table places in continuous recordings -- cue epoching in
    place: window w is samples [starts[w], starts[w] + T) of recording ``rec_index[w]`` of ``rec`` [R, C, N]
    (recording 0 when ``rec_index`` is None, and for a 2-D ``rec`` [C, N]), read where it lies, and row w is
    bit-identical to ``model.eval()`` on that window copied out (``epoch_starts`` gives the reference's
    starts from the cue onsets).  A table given on the host -- a list, a numpy array or a CPU tensor -- is
    checked there (ValueError for a start outside [0, N - T] or a recording outside [0, R)) and uploaded; a
    device table (``starts`` int64, ``rec_index`` int32) is used as it lies and never read by the host, so
    the call can be captured in a graph -- the kernel then clamps an out-of-range entry into the recordings
    instead of reading outside them.  Always eval semantics, whatever ``model.training`` is, and that mode
    is left untouched.  F1*D > 16 models raise NotImplementedError."""
    if rec.dim() not in (2, 3) or rec.shape[-2] != model.C or rec.shape[-1] < model.T:
        raise RuntimeError(f"expected a recording [{model.C}, N] or [R, {model.C}, N] with N >= {model.T}, "
                           f"got {list(rec.shape)}")
    R, N = (1 if rec.dim() == 2 else int(rec.shape[0])), int(rec.shape[-1])
    # host tables first: their check needs no device
    if not (isinstance(starts, torch.Tensor) and starts.device.type == "cuda"):
        starts = _host_table(starts, "starts", torch.int64, 0, N - model.T,
                             f"a window of T = {model.T} samples in a recording of {N}")
    if rec_index is not None and not (isinstance(rec_index, torch.Tensor) and rec_index.device.type == "cuda"):
        rec_index = _host_table(rec_index, "rec_index", torch.int32, 0, R - 1, f"{R} recordings")
        if rec_index.numel() != starts.numel():
            raise ValueError(f"rec_index holds {rec_index.numel()} entries, starts {starts.numel()}")
    require_device(rec, "EEGNet recording")
    if rec.dtype != torch.float32:
        raise RuntimeError(f"epoch_logits expects a float32 recording (got {rec.dtype})")
    starts = starts.to(rec.device)
    rec_index = None if rec_index is None else rec_index.to(rec.device)
    flat = model.flat_parameters()
    require_device(flat, "EEGNet parameters")
    with torch.no_grad():
        try:
            return ops.forward_eval_windows_at(model.shape, flat, model.flat_bn_buffers(), rec.detach(), starts,
                                               rec_index)
        except RuntimeError as e:
            _not_supported(e)


def evaluate_cropped(model, loader, hop) -> float:
    """Accuracy in percent of the crop-averaged prediction (``cropped_predict``) over a loader of
    ``([b, C, N], labels)`` batches of long trials: ``evaluate_model`` for cropped evaluation, with the
    count kept on the device and one host sync at the end."""
    device = _device()
    model = model.to(device)
    correct = torch.zeros((), dtype=torch.int64, device=device)
    total = 0
    for signals, labels in loader:
        signals = signals.float().to(device, non_blocking=True)
        labels = labels.to(device, non_blocking=True)
        _, pred, _ = cropped_predict(model, signals, hop)
        correct += (pred.long() == labels).sum()
        total += labels.size(0)
    return 100 * int(correct.item()) / total


# ----------------------------------------------------------------------------------------------
# train / evaluate_model  (model.py:101-227)
# ----------------------------------------------------------------------------------------------
def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device: the MI355X EEGNet build runs on an AMD GPU only")
    return "cuda"


def _fusable(model, optimizer, loss_fn) -> bool:
    if not isinstance(model, EEGNet) or type(optimizer) is not torch.optim.Adam:
        return False
    if type(loss_fn) is not nn.CrossEntropyLoss:
        return False
    if loss_fn.weight is not None or loss_fn.reduction != "mean" or loss_fn.label_smoothing != 0.0:
        return False
    if len(optimizer.param_groups) != 1:
        return False
    grp = optimizer.param_groups[0]
    ids, want = [id(p) for p in grp["params"]], [id(p) for p in model.parameters()]
    if ids != want:
        # partial fine-tuning with frozen BatchNorm: an optimizer over exactly the trainable suffix
        # (Adam(filter(lambda p: p.requires_grad, model.parameters())) after EEGNet.train_from)
        if not getattr(model, "bn_frozen", False):
            return False
        try:
            stage = model.trainable_stage()
        except NotImplementedError:
            return False                    # (the autograd path raises it at the first forward)
        if stage == 0 or ids != [id(p) for p in model.parameters() if p.requires_grad]:
            return False
    if grp["weight_decay"] != 0 or grp["amsgrad"] or grp.get("maximize", False):
        return False
    if isinstance(grp["lr"], torch.Tensor) or grp.get("differentiable", False):
        return False
    return True


class FusedAdamState:
    """Device-side Adam state for the fused step, synchronised with a torch.optim.Adam."""

    def __init__(self, model: EEGNet, optimizer=None):
        flat = model.flat_parameters()
        n = flat.numel()
        self.state = torch.zeros(2 * n, dtype=torch.float32, device=flat.device)
        self.step = torch.zeros(1, dtype=torch.int32, device=flat.device)
        self.grads = torch.zeros(n, dtype=torch.float32, device=flat.device)
        if optimizer is not None:
            self.load_from(model, optimizer)

    @staticmethod
    def _skips(model, p) -> bool:
        """A parameter the fused frozen-BatchNorm step never touches (EEGNet.train_from): stock Adam
        keeps no state for a parameter whose grad stays None, and neither does the synchronisation."""
        return getattr(model, "bn_frozen", False) and not p.requires_grad

    def load_from(self, model, optimizer):
        n = model.flat_parameters().numel()
        o = 0
        steps = set()
        for p in model.parameters():
            st = {} if self._skips(model, p) else optimizer.state.get(p, {})
            k = p.numel()
            if "exp_avg" in st:
                self.state[o:o + k].copy_(st["exp_avg"].reshape(-1))
                self.state[n + o:n + o + k].copy_(st["exp_avg_sq"].reshape(-1))
                steps.add(int(st["step"]))
            o += k
        if len(steps) > 1:
            raise RuntimeError("inconsistent Adam step counts across parameters")
        self.step.fill_(steps.pop() if steps else 0)

    def store_to(self, model, optimizer):
        n = model.flat_parameters().numel()
        step = int(self.step.item())
        o = 0
        for p in model.parameters():
            k = p.numel()
            if self._skips(model, p):
                o += k
                continue
            st = optimizer.state[p]
            st["step"] = torch.tensor(float(step))
            st["exp_avg"] = self.state[o:o + k].view(p.shape).clone()
            st["exp_avg_sq"] = self.state[n + o:n + o + k].view(p.shape).clone()
            p.grad = self.grads[o:o + k].view(p.shape).clone()
            o += k


class FusedTrainer:
    """Whole hot-loop iteration (model.py:141-148) as one device sequence per batch."""

    def __init__(self, model: EEGNet, lr=1e-3, betas=(0.9, 0.999), eps=1e-7, optimizer=None):
        self.model = model
        self.lr, self.betas, self.eps = lr, betas, eps
        self.adam = FusedAdamState(model, optimizer)
        dev = model.flat_parameters().device
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self._ws = {}
        self._fws = {}

    def workspace(self, B):
        ws = self._ws.get(B)
        if ws is None:
            ws = ops.new_workspace(self.model.shape, B, self.model.flat_parameters().device)
            self._ws[B] = ws
        return ws

    def frozen_workspace(self, B):
        ws = self._fws.get(B)
        if ws is None:
            ws = ops.new_frozen_workspace(self.model.shape, B, self.model.flat_parameters().device)
            self._fws[B] = ws
        return ws

    def step(self, x, y, logits=None):
        m = self.model
        seed, offset = m.next_dropout_key()
        flat, bn_flat, nbt = m.flat_views()
        if getattr(m, "bn_frozen", False):
            # frozen BatchNorm (EEGNet.freeze_bn): one trial-parallel launch, the reduction and Adam; the
            # running statistics and num_batches_tracked are not touched
            masks = m._masks
            if masks is not None and masks[0].shape[0] != x.shape[0]:
                raise RuntimeError("injected dropout masks do not match the batch size")
            stage = m._stage_checked()      # EEGNet.train_from: the backward and Adam stop at the frozen prefix
            try:
                ops.frozen_step(m.shape, flat, bn_flat, x.contiguous(), seed, offset, self.adam.grads,
                                self.frozen_workspace(x.shape[0]), labels=y, masks=masks,
                                adam_state=self.adam.state, step_i32=self.adam.step, loss=self.loss,
                                logits=logits, lr=self.lr, betas=self.betas, eps=self.eps, train_from=stage)
            except RuntimeError as e:
                _not_supported(e)
            return self.loss
        ops.train_step(m.shape, flat, bn_flat, x, y, seed, offset,
                       self.adam.grads, self.adam.state, self.adam.step, self.workspace(x.shape[0]),
                       self.loss, logits=logits, lr=self.lr, betas=self.betas, eps=self.eps,
                       nbt=nbt)
        return self.loss

    def step_epochs(self, rec, starts, y, rec_index=None, sel=None, logits=None):
        """The frozen-BatchNorm branch of ``step`` on windows of continuous recordings read in place
        (``ops.frozen_step_windows``): batch row b is table entry ``sel[b]`` (b when ``sel`` is None), samples
        [starts[e], starts[e] + T) of recording ``rec_index[e]`` of ``rec`` with label ``y[e]``.  The dropout
        key sequence (``next_dropout_key``), the injected masks, the ``train_from`` stage and the Adam state
        are ``step``'s, so the parameters, the moments, the step counter and the loss come out bit-identical
        to ``step`` on the windows copied out.  Device tables are clamped by the kernel, host tables checked
        (``ops.frozen_step_windows``).  RuntimeError unless the model is ``freeze_bn()``-ed: the five-pass
        train step reads contiguous trials."""
        m = self.model
        if not getattr(m, "bn_frozen", False):
            raise RuntimeError("step_epochs is the frozen-BatchNorm step on windows: call model.freeze_bn() first "
                               "(the train-mode step with batch statistics takes contiguous trials, FusedTrainer.step)")
        seed, offset = m.next_dropout_key()
        flat, bn_flat, _ = m.flat_views()
        B = len(sel) if sel is not None else len(starts)
        masks = m._masks
        if masks is not None and masks[0].shape[0] != B:
            raise RuntimeError("injected dropout masks do not match the batch size")
        stage = m._stage_checked()
        try:
            ops.frozen_step_windows(m.shape, flat, bn_flat, rec, starts, y, seed, offset, self.adam.grads,
                                    self.frozen_workspace(B), rec_index=rec_index, sel=sel, masks=masks,
                                    adam_state=self.adam.state, step_i32=self.adam.step, loss=self.loss,
                                    logits=logits, lr=self.lr, betas=self.betas, eps=self.eps, train_from=stage)
        except RuntimeError as e:
            _not_supported(e)
        return self.loss


def batch_slices(n, batch_size):
    """The (begin, end) slices of a permutation of n entries a loop at ``batch_size`` takes: ceil(n / batch_size)
    of them, the last one short (``DataLoader(shuffle=True)`` without ``drop_last``)."""
    n, batch_size = int(n), int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1 (got {batch_size})")
    return [(i, min(i + batch_size, n)) for i in range(0, n, batch_size)]


def finetune_on_recording(model, rec, starts, labels, rec_index=None, *, epochs=1, batch_size=64, lr=1e-3,
                          betas=(0.9, 0.999), eps=1e-7, optimizer=None, generator=None, trainer=None):
    """Fine-tune a ``freeze_bn()``-ed model on the cue epochs of continuous recordings as they lie in memory:
    epoch e of the table is samples [starts[e], starts[e] + T) of recording ``rec_index[e]`` of ``rec``
    [R, C, N] (recording 0 when ``rec_index`` is None, and for [C, N]) with label ``labels[e]``
    (``epoch_starts`` gives the reference's starts from the cue onsets).  No epoch is copied out and no batch
    gathered: per epoch one ``torch.randperm(n, device=..., generator=...)`` is drawn and ceil(n / batch_size)
    ``FusedTrainer.step_epochs`` calls run, each on ``sel = perm[i : i + batch_size]``, the last one short.
    Host tables are checked once (ValueError for a start outside [0, N - T], a recording outside [0, R) or a
    label outside the classes) and uploaded; device tables are used as they lie, clamped by the kernel.  What
    trains is what ``EEGNet.train_from`` left trainable.

    Every step is bit-identical to ``FusedTrainer.step`` on the batch's windows gathered into a contiguous
    [B, C, T] tensor.  Returns ``(losses, trainer)``: the per-step mean cross-entropies as a device tensor
    [epochs, steps], written on the stream without a host read, and the trainer (``trainer`` when given, else a
    new one over ``lr`` / ``betas`` / ``eps`` -- or the single parameter group of ``optimizer``, a
    ``torch.optim.Adam`` whose state is loaded first and stored back at the end, as ``train`` does)."""
    if not getattr(model, "bn_frozen", False):
        raise RuntimeError("finetune_on_recording fine-tunes with frozen BatchNorm: call model.freeze_bn() first")
    require_device(rec, "EEGNet recording")
    if rec.dim() not in (2, 3) or rec.shape[-2] != model.C or rec.shape[-1] < model.T:
        raise RuntimeError(f"expected a recording [{model.C}, N] or [R, {model.C}, N] with N >= {model.T}, "
                           f"got {list(rec.shape)}")
    dev = rec.device
    R, N = (1 if rec.dim() == 2 else int(rec.shape[0])), int(rec.shape[-1])
    # host tables are checked and uploaded once, here; step_epochs then sees device tables
    if not (isinstance(starts, torch.Tensor) and starts.device.type == "cuda"):
        starts = _host_table(starts, "starts", torch.int64, 0, N - model.T,
                             f"a window of T = {model.T} samples in a recording of {N}").to(dev)
    if rec_index is not None and not (isinstance(rec_index, torch.Tensor) and rec_index.device.type == "cuda"):
        rec_index = _host_table(rec_index, "rec_index", torch.int32, 0, R - 1, f"{R} recordings").to(dev)
    if not (isinstance(labels, torch.Tensor) and labels.device.type == "cuda"):
        labels = _host_table(labels, "labels", torch.int64, 0, ops.NCLS - 1, f"{ops.NCLS} classes").to(dev)
    n = int(starts.shape[0])
    if trainer is None:
        if optimizer is not None:
            grp = optimizer.param_groups[0]
            lr, betas, eps = grp["lr"], grp["betas"], grp["eps"]
        trainer = FusedTrainer(model, lr=lr, betas=betas, eps=eps, optimizer=optimizer)
    slices = batch_slices(n, batch_size)
    losses = torch.zeros((int(epochs), len(slices)), dtype=torch.float32, device=dev)
    for e in range(int(epochs)):
        perm = torch.randperm(n, device=dev, generator=generator)
        for k, (i, j) in enumerate(slices):
            losses[e, k:k + 1].copy_(trainer.step_epochs(rec, starts, labels, rec_index, sel=perm[i:j]))
    if optimizer is not None:
        trainer.adam.store_to(model, optimizer)
    return losses, trainer


def train(model, optimizer, loss_fn, train_loader, val_loader, nepochs=500, *, true_best=False,
          fused=None):
    """Train and validate every epoch (model.py:101-189).

    Returns (best_state_dict, train_losses, val_losses, val_accuracies).  As in the reference the
    "best" state dict is a shallow copy of the live state, i.e. the final weights;
    ``true_best=True`` snapshots the best-validation weights instead.
    """
    device = _device()
    logger.info(f"Training on {device} device")
    model = model.to(device)
    use_fused = _fusable(model, optimizer, loss_fn) if fused is None else fused
    trainer = None
    if use_fused:
        grp = optimizer.param_groups[0]
        trainer = FusedTrainer(model, lr=grp["lr"], betas=grp["betas"], eps=grp["eps"],
                               optimizer=optimizer)

    train_losses, val_losses, val_accuracies = [], [], []
    best_model = model.state_dict()
    best_val_acc = 0
    for e in range(1, nepochs + 1):
        model.train()
        run_loss = torch.zeros((), dtype=torch.float64, device=device)
        n_train = 0
        for signals, labels in train_loader:
            signals = signals.float().to(device, non_blocking=True)
            labels = labels.to(device, non_blocking=True)
            if trainer is not None:
                run_loss += trainer.step(signals, labels)[0]
            else:
                preds = model(signals)
                loss = loss_fn(preds, labels)
                run_loss += loss.detach()
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
            n_train += 1

        model.eval()
        run_val = torch.zeros((), dtype=torch.float64, device=device)
        correct = torch.zeros((), dtype=torch.int64, device=device)
        total = 0
        n_val = 0
        with torch.no_grad():
            for signals, labels in val_loader:
                signals = signals.float().to(device, non_blocking=True)
                labels = labels.to(device, non_blocking=True)
                preds = model(signals)
                run_val += loss_fn(preds, labels)
                correct += (torch.argmax(preds, dim=1) == labels).sum()
                total += labels.size(0)
                n_val += 1

        epoch_train_loss = float(run_loss.item()) / max(n_train, 1)
        epoch_val_loss = float(run_val.item()) / max(n_val, 1)
        epoch_val_acc = 100 * int(correct.item()) / total
        train_losses.append(epoch_train_loss)
        val_losses.append(epoch_val_loss)
        val_accuracies.append(epoch_val_acc)
        if epoch_val_acc > best_val_acc:
            best_val_acc = epoch_val_acc
            if true_best:
                best_model = {k: v.detach().clone() for k, v in model.state_dict().items()}
            else:
                best_model = model.state_dict().copy()
        if e == 1 or e % 50 == 0 or e == nepochs:
            logger.info(f"Epoch: {e}/{nepochs}.. Train Loss: {epoch_train_loss:.3f}.. "
                        f"Val Loss: {epoch_val_loss:.3f}.. Val Acc: {epoch_val_acc:.2f}%..")
    if trainer is not None:
        trainer.adam.store_to(model, optimizer)
    return best_model, train_losses, val_losses, val_accuracies


def evaluate_model(model, test_loader) -> float:
    """Test accuracy in percent (model.py:191-227).  Like the reference it does not call
    ``model.eval()``: the caller's mode is used."""
    device = _device()
    logger.info(f"Testing on {device} device")
    model = model.to(device)
    correct = torch.zeros((), dtype=torch.int64, device=device)
    total = 0
    with torch.no_grad():
        for signals, labels in test_loader:
            signals = signals.float().to(device, non_blocking=True)
            labels = labels.to(device, non_blocking=True)
            preds = model(signals)
            correct += (torch.argmax(preds, dim=1) == labels).sum()
            total += labels.size(0)
    return 100 * int(correct.item()) / total
