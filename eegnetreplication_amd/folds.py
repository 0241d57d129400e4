"""Fold-batched training: k independent EEGNet fold runs advanced in lock-step on one GPU
(SURVEY.md 8(f) row 1).

The real protocol trains at batch 64 (train.py:87,229): one fused step is a few microseconds of
work spread over a handful of small launches, so a single fold leaves most of the 256 CUs idle
and the host waits on every launch.  The within-subject protocol has 36 independent runs and the
cross-subject one 90 (train.py:50,73,182,194).  ``FoldBatch`` keeps k of them resident (own
parameters, BN buffers, Adam state and workspace each) and enqueues step j of every fold before
step j+1 of any, each fold on its own HIP stream, so the kernels of different folds overlap on
the device and no host synchronisation happens inside an epoch.

Per fold the arithmetic is ``FusedTrainer.step``'s (model.py:141-148 semantics: forward, CE,
backward with the two clamps, Adam); only the interleaving changes.  Dropout keys are
counter-based per fold -- (fold seed, step counter) -- and a fold-indexed launch splits each fold's
batch over workgroups by the batch size alone, so a fold's trajectory does not depend on how many
other folds run beside it or on which rank it was dealt to (tests/test_gpu_folds.py checks
bit-equality with the same fold run alone).

``FrozenFoldBatch`` is the same for fine-tuning with frozen BatchNorm (``EEGNet.freeze_bn()``): the
frozen step of every resident model in one fold-indexed call (eegnet_frozen_step_folds), each fold
bit-identical to ``ops.frozen_step`` on it alone (tests/test_gpu_frozen_folds.py).
"""

from __future__ import annotations

import weakref

import torch

from . import ops
from .dataset import epoch_permutation
from .model import EEGNet, FusedAdamState


class _FoldGraph:
    """One fold's captured epoch: the key it was captured under (every raw device pointer the graph
    holds), static permutation and per-step loss slots, and the graph."""

    def __init__(self, key, perm, losses, graph):
        self.key = key
        self.perm, self.losses, self.graph = perm, losses, graph


def _refuse_frozen(models):
    """Fold batching runs the batch-statistics step only: a model with frozen BatchNorm layers
    (EEGNet.freeze_bn) would silently train with batch statistics and move its running ones."""
    if any(getattr(m, "bn_frozen", False) for m in models):
        raise ValueError("FoldBatch does not support models with frozen BatchNorm (EEGNet.freeze_bn): "
                         "fine-tune them with FrozenFoldBatch, train() / FusedTrainer, or call freeze_bn(False)")


def _require_frozen(models):
    """Frozen fold batching runs the frozen-BatchNorm step only: a model in batch-statistics mode would
    silently train without moving its running statistics."""
    if not all(getattr(m, "bn_frozen", False) for m in models):
        raise ValueError("FrozenFoldBatch needs every model's BatchNorm layers frozen (EEGNet.freeze_bn()): "
                         "train batch-statistics models with FoldBatch")


def _epoch_buffers(K, n, nsteps, dev):
    """The per-epoch state of a fused fold launch.  The folds' permutations and loss slots are rows of
    one [K, n] / [K, nsteps] buffer each: an epoch refreshes every permutation with ONE asynchronous
    copy from a pinned host buffer (two, alternating: the host fills the next epoch's while the device
    runs this one) and sums every fold's losses with one kernel."""
    perm2 = torch.zeros((K, n), dtype=torch.int64, device=dev)
    loss2 = torch.zeros((K, nsteps), dtype=torch.float32, device=dev)
    return {"graph": None, "perm2": perm2, "perm": list(perm2.unbind(0)),
            "loss2": loss2, "losses": list(loss2.unbind(0)),
            "host": [torch.zeros((K, n), dtype=torch.int64).pin_memory() for _ in range(2)],
            "copied": [None, None], "epoch": 0}


def _stage_permutations(st, n, generators):
    """This epoch's permutation of every fold into ``st["perm2"]``: one pinned-host copy."""
    i = st["epoch"] & 1
    st["epoch"] += 1
    if st["copied"][i] is not None:     # this pinned buffer's copy (two epochs ago) has run
        st["copied"][i].synchronize()
    host = st["host"][i]
    for k in range(host.shape[0]):
        g = generators[k] if generators is not None else None
        host[k].copy_(epoch_permutation(n, g) if g is not None else torch.arange(n))
    st["perm2"].copy_(host, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    st["copied"][i] = ev


def _run_epoch(st, steps, graphs):
    """Replay the captured epoch, or enqueue it with ``steps()`` (and, with ``graphs``, capture it for
    the next epochs); returns the folds' loss sums."""
    if st["graph"] is not None:
        st["graph"].replay()
    else:
        steps()
        if graphs:                      # capture for the next epochs (tables / workspaces exist)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                steps()
            st["graph"] = gr
            # the capture recorded without executing: run this epoch's work once more is NOT
            # wanted -- the eager pass above already trained the epoch
    return list(st["loss2"].sum(dim=1, dtype=torch.float64).unbind(0))


class _At:
    """A raw device address where a table builder expects a tensor (``data_ptr()``)."""

    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


_eval_states: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()    # models[0] -> evaluate_folds state


def evaluate_folds(models, sets, batch_size: int = 64, *, out=None):
    """Validate every model on its own held-out set with one fold-indexed call (eegnet_eval_folds):
    the eval-mode forward (running statistics, no dropout, whatever mode the modules are in), the
    per-trial cross-entropy and the argmax of all folds in one launch, and per fold the reference's
    validation loss -- the mean over the batches of ``batch_size`` consecutive trials (the last one
    short) of each batch's mean CE, model.py:156-172 -- and the number of correct trials.

    ``sets[k] = (X_k [n_k, C, T] float32, y_k [n_k] int64)``: contiguous device tensors, sizes may
    differ, folds may share a set.  Returns ``(loss float64 [k], correct int64 [k])`` device tensors;
    nothing is synchronised and no torch kernel runs.  ``out``: a ``(loss, correct)`` pair of
    contiguous [k] tensors (float64, int64) to receive the results -- rows of two larger buffers, say
    -- instead of the call's own pair, which the next call on the same models and sets overwrites.

    The fold table, the per-trial scratch and the outputs are built once per (models, sets) identity
    and reused: training updates parameters and BN buffers in place, so the pointers stay valid.  They
    are rebuilt when a model's flat parameter / BN buffer or a set tensor is another object."""
    K = len(models)
    if K < 1 or len(sets) != K:
        raise ValueError("need at least one model and one (X, y) per model")
    if out is not None:
        lo, co = out
        if (tuple(lo.shape) != (K,) or tuple(co.shape) != (K,) or lo.dtype != torch.float64
                or co.dtype != torch.int64 or not lo.is_contiguous() or not co.is_contiguous()
                or lo.device != co.device):
            raise ValueError(f"out must be (float64 [{K}], int64 [{K}]) contiguous tensors on one device")
        # a row of a larger buffer is that buffer's table at another slot: no new table per row
        bases = (lo.untyped_storage().data_ptr(), co.untyped_storage().data_ptr())
        slot = lo.storage_offset()
        if co.storage_offset() != slot:
            bases, slot = (lo.data_ptr(), co.data_ptr()), 0
    else:
        bases, slot = None, 0
    # every raw device pointer the table holds, and the identity of what it was taken from (the state
    # keeps the set tensors alive, so an id cannot come back as another tensor); one flat-layout check
    # per model (flat_views), which re-flattens a model whose parameters were re-created
    views = [m.flat_views() for m in models]
    key = (bases, tuple((id(m), v[0].data_ptr(), v[1].data_ptr(), id(X), X.data_ptr(), X.shape[0], id(y),
                         y.data_ptr()) for m, v, (X, y) in zip(models, views, sets)))
    st = _eval_states.get(models[0])
    if st is None or st["key"] != key:
        shape = models[0].shape

        def geom(s):                  # what the eval forward reads of a Shape (not p, not the momentum)
            return (s.C, s.T, s.F1, s.D, s.K1, s.eps)
        if any(geom(m.shape) != geom(shape) for m in models) or shape.F2 > 16:
            raise ValueError("evaluate_folds needs one common EEGNet shape with F1*D <= 16 for every model: "
                             "evaluate other models one at a time (model.eval(); model(X), or evaluate_model())")
        dev = views[0][0].device
        if dev.type != "cuda":
            raise RuntimeError("evaluate_folds runs on a HIP device only")
        for X, y in sets:
            if (X.device != dev or y.device != dev or X.dtype != torch.float32 or y.dtype != torch.int64
                    or X.dim() != 3 or tuple(X.shape[1:]) != (shape.C, shape.T) or tuple(y.shape) != (X.shape[0],)):
                raise ValueError(f"every set must be (X [n, {shape.C}, {shape.T}] float32, y [n] int64) on {dev}")
            if not X.is_contiguous() or not y.is_contiguous():
                raise ValueError("evaluate_folds takes contiguous X and y (call .contiguous() once, outside "
                                 "the loop)")
            if shape.T % 4 == 0 and X.data_ptr() % 16:
                raise ValueError("X must be 16-byte aligned when T % 4 == 0")
        if out is not None and lo.device != dev:
            raise ValueError(f"out must be on {dev}")
        ns = [int(X.shape[0]) for X, _ in sets]
        ce = torch.empty(max(sum(ns), 1), dtype=torch.float32, device=dev)
        pred = torch.empty(max(sum(ns), 1), dtype=torch.int32, device=dev)
        st = {"key": key, "shape": shape, "src": list(sets), "ce": ce, "pred": pred, "max_n": max(ns)}
        if out is None:
            st["loss"] = torch.zeros(K, dtype=torch.float64, device=dev)
            st["correct"] = torch.zeros(K, dtype=torch.int64, device=dev)
            lp, cp = st["loss"].data_ptr(), st["correct"].data_ptr()
        else:
            st["hold"] = (lo.untyped_storage(), co.untyped_storage())
            lp, cp = bases
        ents, o = [], 0
        for k, (v, (X, y)) in enumerate(zip(views, sets)):
            ents.append(dict(params=v[0], bn_buffers=v[1], x=X, labels=y, n=ns[k],
                             logits=None, ce=_At(ce.data_ptr() + 4 * o), pred=_At(pred.data_ptr() + 4 * o),
                             loss=_At(lp + 8 * k), correct=_At(cp + 8 * k)))
            o += ns[k]
        st["table"] = ops.eval_fold_table(ents, dev)
        _eval_states[models[0]] = st
    shape = st["shape"]
    ops.eval_folds(shape, st["table"], K, st["max_n"], batch=int(batch_size), slot=slot)
    return (st["loss"], st["correct"]) if out is None else (lo, co)


class _FoldStreams:
    """What FoldBatch and FrozenFoldBatch share: the per-fold path of an epoch -- one HIP stream per
    fold, each fold's epoch enqueued by the class's ``_steps`` and, with ``graphs``, captured as that
    fold's hipGraph -- and the identity keys of what a captured epoch or a fold table baked in."""

    def __len__(self):
        return len(self.models)

    def validate(self, sets, batch_size: int = 64):
        """``evaluate_folds`` on this batch's models: per fold the validation loss (float64) and the
        number of correct trials (int64) on ``sets[k] = (X_k, y_k)``, as device tensors, unsynchronised."""
        return evaluate_folds(self.models, sets, batch_size)

    def _fold_key(self, k, X, y, batch_size):
        """What fold k's captured epoch baked in: its model / Adam buffers (re-created by ``.to()``,
        ``.float()`` or a re-flatten), its X and y, the batch size and workspace."""
        m, a = self.models[k], self.adam[k]
        return (X.shape[0], batch_size, id(X), X.data_ptr(), id(y), y.data_ptr(),
                m.flat_parameters().data_ptr(), m.flat_bn_buffers().data_ptr(),
                m.flat_num_batches_tracked().data_ptr(), a.state.data_ptr(), a.grads.data_ptr(),
                a.step.data_ptr())

    def _fused_key(self, data, batch_size):
        """Everything a fold table or the captured graph holds a raw device pointer to: each
        model's flat parameters, BN buffers, counters, Adam state and gradients, and the identity
        of every fold's X and y.  ``.to()`` / ``.cuda()`` / ``.float()`` or a re-flatten re-creates
        the model buffers; a caller may pass new y tensors with the same X."""
        ptrs = []
        for m, a in zip(self.models, self.adam):
            ptrs += [m.flat_parameters().data_ptr(), m.flat_bn_buffers().data_ptr(),
                     m.flat_num_batches_tracked().data_ptr(), a.state.data_ptr(), a.grads.data_ptr(),
                     a.step.data_ptr()]
        return (data[0][0].shape[0], batch_size, tuple(ptrs),
                tuple((id(X), X.data_ptr(), id(y), y.data_ptr()) for X, y in data))

    def _epoch_streams(self, data, batch_size, generators):
        cur = torch.cuda.current_stream()
        sums = []
        for k, (X, y) in enumerate(data):
            n = X.shape[0]
            nsteps = (n + batch_size - 1) // batch_size
            g = generators[k] if generators is not None else None
            perm = epoch_permutation(n, g) if g is not None else torch.arange(n)
            s = self.streams[k]
            s.wait_stream(cur)
            st = self._graph[k]
            with torch.cuda.stream(s):
                key = self._fold_key(k, X, y, batch_size)
                if st is not None and st.key == key:
                    st.perm.copy_(perm, non_blocking=True)
                    st.graph.replay()
                    sums.append(st.losses.sum(dtype=torch.float64))
                    continue
                perm_d = perm.to(X.device)
                losses = torch.zeros(nsteps, dtype=torch.float32, device=X.device)
                self._steps(k, X, y, perm_d, losses, batch_size)
                sums.append(losses.sum(dtype=torch.float64))
                if self.graphs:                 # capture for the next epochs (workspaces exist now)
                    gr = torch.cuda.CUDAGraph()
                    sperm = perm_d.clone()
                    slosses = torch.zeros_like(losses)
                    with torch.cuda.graph(gr, stream=s):
                        self._steps(k, X, y, sperm, slosses, batch_size)
                    self._graph[k] = _FoldGraph(key, sperm, slosses, gr)
        for s in self.streams:
            cur.wait_stream(s)
        for t in sums:
            t.record_stream(cur)
        return sums


class FoldBatch(_FoldStreams):
    """k independent fold runs on one GPU, one HIP stream each.

    ``graphs=True`` captures each fold's epoch (batch gathers + fused steps) as a hipGraph after
    its first, eager epoch and replays it afterwards: one host call per fold per epoch instead of
    ~10 launches per step.  Dropout keys follow the device Adam step (EEGNET_KEY_FROM_STEP) in both
    modes, so replays draw fresh masks each step and graph and eager runs are bit-identical."""

    def __init__(self, models: list[EEGNet], seeds: list[int], lr=1e-3, betas=(0.9, 0.999),
                 eps=1e-7, graphs=False, fused=None, xstats=True):
        """``fused``: advance all folds with ONE launch per pass (eegnet_train_step_folds, the fold
        index in the grid) instead of one stream per fold.  ``None`` picks it whenever it applies:
        same model shape for every fold, F1*D <= 16, and (per epoch) the same number of trials.
        ``xstats``: fused launches read each batch's parameter-free BN1 statistics from a per-trial
        table of every fold's X (ops.x_stats, computed once per X and refreshed when X changes in
        place) instead of recomputing the lag-Gram from x every step.

        Change detection is PyTorch's version counter (``X._version``), which tracked in-place ops
        bump.  Writes that bypass it -- through ``X.data``, DLPack or another library's view of the
        storage, a ctypes / HIP kernel -- must be followed by ``invalidate_x()``: without it the
        table (and, at 22 x 257, the padded copy the kernels read) keeps the old trials."""
        if len(models) != len(seeds) or not models:
            raise ValueError("need one seed per model and at least one model")
        _refuse_frozen(models)
        dev = models[0].flat_parameters().device
        if dev.type != "cuda":
            raise RuntimeError("FoldBatch runs on a HIP device only")
        self.models = models
        self.seeds = [int(s) for s in seeds]
        self.lr, self.betas, self.eps = lr, betas, eps
        self.graphs = graphs
        self.adam = [FusedAdamState(m) for m in models]
        self.streams = [torch.cuda.Stream(device=dev) for _ in models]
        self._ws: list[dict] = [{} for _ in models]
        self._graph: list[_FoldGraph | None] = [None] * len(models)
        same = all(m.shape == models[0].shape for m in models) and models[0].shape.F2 <= 16
        if fused and not same:
            raise ValueError("fused fold launches need the same EEGNet shape (F1*D <= 16) for every fold")
        self.fused = same if fused is None else bool(fused)
        self.xstats = bool(xstats)
        self._fz = None                     # fused-launch state: buffers, fold tables, graph

    def invalidate_x(self):
        """Recompute every fold's padded x copy and per-trial BN1 table from its X at the next epoch
        (for writes to X that PyTorch's version counter does not see: ``X.data``, DLPack, foreign
        kernels).  Same storage: the fold tables and the captured graph stay valid."""
        if self._fz is not None:
            for ent in self._fz["xsrc"].values():
                ent["ver"] = None

    def _workspace(self, k, B):
        ws = self._ws[k].get(B)
        if ws is None:
            ws = ops.new_workspace(self.models[k].shape, B, self.models[k].flat_parameters().device)
            self._ws[k][B] = ws
        return ws

    def _steps(self, k, X, y, perm, losses, batch_size):
        """Enqueue one epoch of fold k on the current stream: the epoch's shuffled copy of X is
        gathered once (one launch, not two per step), batch j is its rows [jB, (j+1)B), and its
        loss lands in losses[j] (no accumulation kernel)."""
        m = self.models[k]
        a = self.adam[k]
        Xp, yp = X.index_select(0, perm), y.index_select(0, perm)
        flat, bn, nbt = m.flat_views()
        for j, i in enumerate(range(0, perm.shape[0], batch_size)):
            xb, yb = Xp[i:i + batch_size], yp[i:i + batch_size]
            ops.train_step(m.shape, flat, bn, xb, yb, self.seeds[k],
                           0, a.grads, a.state, a.step, self._workspace(k, xb.shape[0]),
                           losses[j:j + 1], lr=self.lr, betas=self.betas, eps=self.eps,
                           nbt=nbt, key_from_step=True)

    # -- fused launches: all folds in one grid --------------------------------------------------
    def _fused_state(self, data, batch_size):
        X0, _ = data[0]
        n = X0.shape[0]
        key = self._fused_key(data, batch_size)
        st = self._fz
        if st is not None and st["key"] == key:
            return st
        dev = X0.device
        K = len(self.models)
        nsteps = (n + batch_size - 1) // batch_size
        # any change: new tables, and the graph (which baked the old pointers in) is dropped
        st = {"key": key, "src": [d for d in data], "tables": {}, "steps": [],
              **_epoch_buffers(K, n, nsteps, dev)}
        # x rows at the pitch the kernels load fastest (22 x 257: 260 floats, 16-byte DMA units):
        # one padded copy per distinct X, kept for the life of this state and refreshed in place
        # (same storage: the tables and the graph stay valid) whenever X changes in place
        # (X._version: a caller refilling a preallocated augmentation buffer)
        shape = self.models[0].shape
        xp = shape.x_pitch()
        st["x_pitch"] = 0 if xp == shape.T else xp
        st["xsrc"] = {}

        def xrows(X):
            """(the rows the kernels read, the per-trial BN1 table or None) of X, made once per X"""
            ent = st["xsrc"].get(id(X))
            if ent is None:
                rows = X if ops.x_pitch_of(X) == st["x_pitch"] else ops.pad_x_rows(X, xp)
                stat = ops.x_stats(shape, rows) if self.xstats else None
                ent = st["xsrc"][id(X)] = {"X": X, "rows": rows, "stat": stat, "ver": X._version}
            return ent["rows"], ent["stat"]
        for j, i in enumerate(range(0, n, batch_size)):
            B = min(batch_size, n - i)
            st["steps"].append((i, j, B))
            if B not in st["tables"]:
                ents = []
                for k, m in enumerate(self.models):
                    a = self.adam[k]
                    # x / labels stay unshuffled: the kernels read batch row r as row perm[r]
                    X, y = data[k]
                    rows, stat = xrows(X)
                    ents.append(dict(params=m.flat_parameters(), bn_buffers=m.flat_bn_buffers(),
                                     num_batches_tracked=m.flat_num_batches_tracked(), x=rows, xstat=stat,
                                     labels=y,
                                     perm=st["perm"][k], grads=a.grads, adam_state=a.state, step=a.step,
                                     losses=st["losses"][k], ws=self._workspace(k, B), seed=self.seeds[k]))
                st["tables"][B] = ops.fold_table(ents, dev)
        self._fz = st
        return st

    def _fused_steps(self, st, data):
        shape = self.models[0].shape
        K = len(self.models)
        for i, j, B in st["steps"]:
            ops.train_step_folds(shape, B, st["tables"][B], K, row0=i, slot=j, offset=0, lr=self.lr,
                                 betas=self.betas, eps=self.eps, x_pitch=st["x_pitch"])

    def _refresh_padded(self, st):
        """Every X that changed in place since its padded copy / BN1 table were made: re-copy and
        recompute them in their own storage (the fold tables and the captured graph keep pointing
        there)."""
        shape = self.models[0].shape
        for ent in st["xsrc"].values():
            X = ent["X"]
            if X._version != ent["ver"]:
                with torch.no_grad():
                    if ent["rows"] is not X:
                        ent["rows"].copy_(X)
                    if ent["stat"] is not None:
                        ops.x_stats(shape, ent["rows"], out=ent["stat"])
                ent["ver"] = X._version

    def _epoch_fused(self, data, batch_size, generators):
        n = data[0][0].shape[0]
        st = self._fused_state(data, batch_size)
        self._refresh_padded(st)
        _stage_permutations(st, n, generators)
        return _run_epoch(st, lambda: self._fused_steps(st, data), self.graphs)

    def epoch(self, data: list[tuple[torch.Tensor, torch.Tensor]], batch_size: int = 64,
              generators: list[torch.Generator] | None = None) -> list[torch.Tensor]:
        """One training epoch of every fold.  ``data[k] = (X_k [N_k,C,T] fp32, y_k [N_k] int64)``,
        device-resident.  Each fold is shuffled by its own generator exactly as
        DataLoader(shuffle=True, generator=g) would (train.py:87; dataset.epoch_permutation) and cut into batches of ``batch_size`` with a short last batch
        (drop_last=False).  Returns per-fold float64 device scalars: the sum of the batch losses
        (the reference's running loss, model.py:150).  Nothing is synchronised."""
        if len(data) != len(self.models):
            raise ValueError("one (X, y) per fold")
        _refuse_frozen(self.models)
        if self.fused and all(X.shape[0] == data[0][0].shape[0] for X, _ in data):
            return self._epoch_fused(data, batch_size, generators)
        return self._epoch_streams(data, batch_size, generators)


class FrozenFoldBatch(_FoldStreams):
    """k independent frozen-BatchNorm fine-tuning runs on one GPU: ``FoldBatch`` for models whose
    BatchNorm layers are frozen (``EEGNet.freeze_bn()``) -- fine-tuning a cross-subject model per
    subject with k-fold validation, say.  Per fold the arithmetic is ``FusedTrainer.step``'s on a frozen
    model (forward with the running statistics and dropout, mean CE, backward with the two clamps,
    Adam); the running statistics and ``num_batches_tracked`` are never written.

    The fused path advances every fold with four launches per batch (eegnet_frozen_step_folds: the
    fold index in the grid, the epoch's shuffle read through per-fold permutations, x in place); the
    per-fold path runs ``ops.frozen_step`` on the epoch's gathered rows, one HIP stream per fold.  Both
    key the dropout masks by (fold seed, device Adam step) and split a fold's batch over workgroups by
    the batch size alone, so they agree bit for bit, with and without ``graphs``.

    Partial fine-tuning (``EEGNet.train_from``): every epoch derives each model's stage from its
    ``requires_grad`` flags; a fold's backward stops at its frozen prefix, whose parameters and Adam
    state are never written.  The fused launches take one stage for all folds: with mixed stages
    ``fused=True`` is a ValueError and ``fused=None`` runs the per-fold path, each fold at its own stage."""

    def __init__(self, models: list[EEGNet], seeds: list[int], lr=1e-3, betas=(0.9, 0.999),
                 eps=1e-7, graphs=False, fused=None):
        """``fused``: ``None`` picks the fused launches where they apply (one EEGNet shape with
        F1*D <= 16 for every fold and, per epoch, the same number of trials) and
        ``FUSED_MIN_FOLDS`` or more folds are resident.  ``graphs``: the first epoch runs eagerly,
        the epoch is captured as a hipGraph and later epochs replay it."""
        if len(models) != len(seeds) or not models:
            raise ValueError("need one seed per model and at least one model")
        _require_frozen(models)
        dev = models[0].flat_parameters().device
        if dev.type != "cuda":
            raise RuntimeError("FrozenFoldBatch runs on a HIP device only")
        self.models = models
        self.seeds = [int(s) for s in seeds]
        self.lr, self.betas, self.eps = lr, betas, eps
        self.graphs = graphs
        self.adam = [FusedAdamState(m) for m in models]
        self.streams = [torch.cuda.Stream(device=dev) for _ in models]
        self._ws: list[dict] = [{} for _ in models]
        self._graph: list[_FoldGraph | None] = [None] * len(models)
        same = all(m.shape == models[0].shape for m in models) and models[0].shape.F2 <= 16
        if fused and not same:
            raise ValueError("fused fold launches need the same EEGNet shape (F1*D <= 16) for every fold")
        self._auto = fused is None
        self.fused = (same and len(models) >= self.FUSED_MIN_FOLDS) if fused is None else bool(fused)
        self._fz = None                     # fused-launch state: buffers, fold tables, graph
        self._stages = None
        self._derive_stages()

    def _derive_stages(self):
        """Each model's stage from its ``requires_grad`` flags (NotImplementedError for a pattern that is
        no frozen prefix).  A change drops what was captured with the old stages; returns whether the
        fused launches apply (one stage for every fold)."""
        stages = tuple(m.trainable_stage() for m in self.models)
        if stages != self._stages:
            self._stages = stages
            self._fz = None
            self._graph = [None] * len(self.models)
        uniform = len(set(stages)) == 1
        if self.fused and not uniform and not self._auto:
            raise ValueError(f"fused fold launches need the same trainable stage for every fold (got "
                             f"{[ops.STAGES[s] for s in stages]}): pass fused=None or fused=False")
        return self.fused and uniform

    # fused=None takes the fused launches from this many folds on: profiles/frozen_folds_bench.json has
    # them no slower than the per-fold path at every K measured (12, 36, 90), and nothing below 12
    FUSED_MIN_FOLDS = 12

    def _workspace(self, k, B):
        ws = self._ws[k].get(B)
        if ws is None:
            ws = ops.new_frozen_workspace(self.models[k].shape, B, self.models[k].flat_parameters().device)
            self._ws[k][B] = ws
        return ws

    def _steps(self, k, X, y, perm, losses, batch_size):
        """Enqueue one epoch of fold k on the current stream, as FoldBatch._steps: the epoch's
        shuffled copy of X gathered once, batch j its rows [jB, (j+1)B), its loss in losses[j]."""
        m = self.models[k]
        a = self.adam[k]
        Xp, yp = X.index_select(0, perm), y.index_select(0, perm)
        flat, bn, _ = m.flat_views()
        for j, i in enumerate(range(0, perm.shape[0], batch_size)):
            xb, yb = Xp[i:i + batch_size], yp[i:i + batch_size]
            ops.frozen_step(m.shape, flat, bn, xb, self.seeds[k], 0, a.grads, self._workspace(k, xb.shape[0]),
                            labels=yb, adam_state=a.state, step_i32=a.step, loss=losses[j:j + 1],
                            lr=self.lr, betas=self.betas, eps=self.eps, key_from_step=True,
                            train_from=self._stages[k])

    def _fused_state(self, data, batch_size):
        X0, _ = data[0]
        n = X0.shape[0]
        key = self._fused_key(data, batch_size)
        st = self._fz
        if st is not None and st["key"] == key:
            return st
        dev = X0.device
        shape = self.models[0].shape
        for X, y in data:
            if (X.device != dev or y.device != dev or X.dtype != torch.float32 or y.dtype != torch.int64
                    or X.dim() != 3 or tuple(X.shape[1:]) != (shape.C, shape.T) or tuple(y.shape) != (n,)):
                raise ValueError(f"every fold's data must be (X [n, {shape.C}, {shape.T}] float32, y [n] int64) on {dev}")
            # the frozen kernels read x in place at pitch T: no padded copy, no BN1 table
            if not X.is_contiguous() or not y.is_contiguous():
                raise ValueError("FrozenFoldBatch takes contiguous X and y (call .contiguous() once, outside "
                                 "the loop)")
            if shape.T % 4 == 0 and X.data_ptr() % 16:
                raise ValueError("X must be 16-byte aligned when T % 4 == 0")
        K = len(self.models)
        nsteps = (n + batch_size - 1) // batch_size
        # any change: new tables, and the graph (which baked the old pointers in) is dropped
        st = {"key": key, "src": [d for d in data], "tables": {}, "steps": [],
              **_epoch_buffers(K, n, nsteps, dev)}
        for j, i in enumerate(range(0, n, batch_size)):
            B = min(batch_size, n - i)
            st["steps"].append((i, j, B))
            if B not in st["tables"]:       # one table per distinct batch size (the short last batch)
                ents = []
                for k, m in enumerate(self.models):
                    a = self.adam[k]
                    X, y = data[k]
                    ents.append(dict(params=m.flat_parameters(), bn_buffers=m.flat_bn_buffers(), x=X, labels=y,
                                     perm=st["perm"][k], grads=a.grads, adam_state=a.state, step=a.step,
                                     losses=st["losses"][k], ws=self._workspace(k, B), seed=self.seeds[k]))
                st["tables"][B] = ops.fold_table(ents, dev)
        self._fz = st
        return st

    def _fused_steps(self, st):
        shape = self.models[0].shape
        K = len(self.models)
        for i, j, B in st["steps"]:
            ops.frozen_step_folds(shape, B, st["tables"][B], K, row0=i, slot=j, offset=0, lr=self.lr,
                                  betas=self.betas, eps=self.eps, train_from=self._stages[0])

    def epoch(self, data: list[tuple[torch.Tensor, torch.Tensor]], batch_size: int = 64,
              generators: list[torch.Generator] | None = None) -> list[torch.Tensor]:
        """One fine-tuning epoch of every fold, as ``FoldBatch.epoch``: ``data[k] = (X_k [N_k,C,T]
        fp32, y_k [N_k] int64)``, device-resident and contiguous; each fold shuffled by its own
        generator as DataLoader(shuffle=True, generator=g) would and cut into batches of
        ``batch_size`` with a short last batch.  Returns per-fold float64 device scalars: the sum of
        the batch losses.  Nothing is synchronised."""
        _require_frozen(self.models)
        if len(data) != len(self.models):
            raise ValueError("one (X, y) per fold")
        if self._derive_stages() and all(X.shape[0] == data[0][0].shape[0] for X, _ in data):
            st = self._fused_state(data, batch_size)
            _stage_permutations(st, data[0][0].shape[0], generators)
            return _run_epoch(st, lambda: self._fused_steps(st), self.graphs)
        return self._epoch_streams(data, batch_size, generators)
