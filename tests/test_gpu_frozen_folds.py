"""GPU tests of fold-indexed frozen-BatchNorm fine-tuning (eegnet_frozen_step_folds behind
``ops.frozen_step_folds`` and ``FrozenFoldBatch``).

The contract of the call is bit-identity: every output of a fold -- gradients, loss, parameters, Adam
state, step -- equals ``ops.frozen_step(key_from_step=True)`` on that fold alone with the batch's rows
gathered, whatever else shares the launch.  The tests check that with ``torch.equal``, and pin the
fold-indexed call to the float64 oracle (tests/frozen_cases.py) directly as well, at the tolerances of
tests/test_gpu_frozen.py."""

from __future__ import annotations

import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from frozen_cases import FrozenRefEEGNet, assert_frozen_grads_close, model_state, oracle_frozen
from golden_util import PARAM_NAMES, assert_close, make_inputs
from hip_cases import device_masks, flat_to_dict, random_model

pytestmark = pytest.mark.gpu

SENTINEL = 7.0          # what an unwritten loss slot holds


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _cus():
    return torch.cuda.get_device_properties(_dev()).multi_processor_count


@functools.lru_cache(maxsize=None)
def _model(C, T, F1=8, D=2, K1=32, p=0.5, seed=0):
    """A CPU model with every BN term off its identity value; shared, never modified."""
    return random_model(C, T, F1=F1, D=D, K1=K1, p=p, seed=17 * seed + C + T + K1)


@functools.lru_cache(maxsize=None)
def _data(n, C, T, seed):
    """(x [n, C, T] float32, y [n] int64) numpy; shared, never modified."""
    return make_inputs(n, C, T, 2100 + seed)


class _Fold:
    """One model's device state of a fold-indexed call: a device copy of the model, gradients, Adam
    state (non-zero), the device step, three loss slots and the partial-row workspace."""

    def __init__(self, m, X, y, perm, seed, step0, B, adam=True):
        from eegnetreplication_amd import ops
        dev = _dev()
        self.md = copy.deepcopy(m).to(dev).train()
        self.md.flat_num_batches_tracked().fill_(17)
        n = self.md.flat_parameters().numel()
        g = torch.Generator().manual_seed(seed)
        self.X, self.y, self.perm, self.seed, self.B = X, y, perm, seed, B
        self.grads = torch.full((n,), float("nan"), device=dev)
        self.adam = (1e-3 * torch.rand(2 * n, generator=g)).to(dev) if adam else None
        self.step = torch.full((1,), step0, dtype=torch.int32, device=dev)
        self.losses = torch.full((3,), SENTINEL, device=dev)
        self.ws = ops.new_frozen_workspace(self.md.shape, B, dev)

    def clone(self):
        c = copy.copy(self)
        c.md = copy.deepcopy(self.md)
        c.grads, c.step, c.losses, c.ws = self.grads.clone(), self.step.clone(), self.losses.clone(), self.ws.clone()
        c.adam = None if self.adam is None else self.adam.clone()
        return c

    def entry(self):
        return dict(params=self.md.flat_parameters(), bn_buffers=self.md.flat_bn_buffers(), x=self.X, labels=self.y,
                    perm=self.perm, grads=self.grads, adam_state=self.adam, step=self.step, losses=self.losses,
                    ws=self.ws, seed=self.seed)

    def outputs(self):
        z = torch.zeros(1, device=_dev())
        return (self.grads, self.losses, self.md.flat_parameters(), self.adam if self.adam is not None else z,
                self.step, self.md.flat_bn_buffers(), self.md.flat_num_batches_tracked())

    def rows(self, row0):
        idx = (self.perm[row0:row0 + self.B] if self.perm is not None
               else torch.arange(row0, row0 + self.B, device=_dev()))
        return self.X.index_select(0, idx).contiguous(), self.y.index_select(0, idx).contiguous()


def _run_folds(folds, row0, slot, offset, clamp=True):
    """One eegnet_frozen_step_folds over ``folds`` (in that table order), synchronised."""
    from eegnetreplication_amd import ops
    table = ops.fold_table([f.entry() for f in folds], _dev())
    ops.frozen_step_folds(folds[0].md.shape, folds[0].B, table, len(folds), row0, slot, offset=offset, clamp=clamp)
    torch.cuda.synchronize()


def _run_alone(f, row0, slot, offset, clamp=True):
    """The same iteration of one fold through eegnet_frozen_step on the batch's gathered rows."""
    from eegnetreplication_amd import ops
    xb, yb = f.rows(row0)
    ops.frozen_step(f.md.shape, f.md.flat_parameters(), f.md.flat_bn_buffers(), xb, f.seed, offset, f.grads, f.ws,
                    labels=yb, adam_state=f.adam, step_i32=f.step, loss=f.losses[slot:slot + 1], clamp=clamp,
                    key_from_step=True)
    torch.cuda.synchronize()


def _assert_same(a, b, what):
    for i, (u, v) in enumerate(zip(a.outputs(), b.outputs())):
        assert torch.equal(u, v), f"{what}: output {i} (grads, losses, params, adam, step, bn, nbt)"


def _make_folds(C, T, B, F1=8, D=2, K1=32, steps=(0, 3, 7), n=None, share_x=True, p=0.5):
    """len(steps) folds: own parameters, BN buffers, seeds and permutations; the first two share one x."""
    dev = _dev()
    n = n if n is not None else B + 6
    sets = {}
    folds = []
    for k, s in enumerate(steps):
        xi = 0 if (share_x and k < 2) else k
        if xi not in sets:
            x, y = _data(n, C, T, xi)
            sets[xi] = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(50 + k)).to(dev)
        folds.append(_Fold(_model(C, T, F1, D, K1, p, seed=k), *sets[xi], perm, seed=1000 + 37 * k, step0=s, B=B))
    return folds


# ---- 1. a fold equals itself alone ----
@pytest.mark.parametrize("C,T,B,F1,D,K1", [(22, 257, 5, 8, 2, 32), (22, 256, 3, 8, 2, 32), (5, 96, 3, 4, 1, 32),
                                           (22, 257, 2, 8, 2, 64)])
def test_a_fold_equals_itself_alone(C, T, B, F1, D, K1):
    folds = _make_folds(C, T, B, F1, D, K1)
    assert folds[0].X is folds[1].X and folds[2].X is not folds[0].X
    alone = [f.clone() for f in folds]
    before = [f.clone() for f in folds]
    _run_folds(folds, row0=2, slot=1, offset=9)
    for k, (f, a, b) in enumerate(zip(folds, alone, before)):
        _run_alone(a, row0=2, slot=1, offset=9)
        _assert_same(f, a, f"fold {k}")
        assert float(f.losses[0]) == SENTINEL == float(f.losses[2]) and np.isfinite(float(f.losses[1]))
        assert torch.equal(f.md.flat_bn_buffers(), b.md.flat_bn_buffers())
        assert torch.equal(f.md.flat_num_batches_tracked(), b.md.flat_num_batches_tracked())
        assert int(f.step) == int(b.step) + 1
        assert not torch.equal(f.md.flat_parameters(), b.md.flat_parameters())
        assert bool(torch.isfinite(f.grads).all())


# ---- 2. more trials than the per-fold grid ----
def test_more_trials_than_the_per_fold_grid():
    """8 x 64 at B = 2 * CUs + 3: every workgroup of a fold accumulates several trials, the last round is
    partial; bit-identical to the single call, and fold 0 on the float64 oracle under its own masks."""
    B, T, offset = 2 * _cus() + 3, 64, 4
    folds = _make_folds(8, T, B, steps=(2, 5), n=B + 2)
    alone = [f.clone() for f in folds]
    state = model_state(folds[0].md)
    _run_folds(folds, row0=1, slot=0, offset=offset)
    for k, (f, a) in enumerate(zip(folds, alone)):
        _run_alone(a, row0=1, slot=0, offset=offset)
        _assert_same(f, a, f"fold {k}")
    f = folds[0]
    xb, yb = f.rows(1)
    ref = oracle_frozen(state, xb.cpu().numpy(), 0.5, device_masks(B, 16, T, f.seed, offset + 2, 0.5),
                        labels=yb.cpu().numpy())
    assert_frozen_grads_close(flat_to_dict(f.md, f.grads), ref["grads"], raw=ref["raw"], prefix=f"8x64 B={B} grad ")
    assert_close(f.losses.cpu().numpy()[0], ref["loss"], name="8x64 loss")


# ---- 3. the float64 oracle directly ----
def _oracle_adam(state, p, x, y, masks_per_step, step0):
    """float64 oracle fine-tuning on one batch: torch.optim.Adam(lr=1e-3, eps=1e-7) whose step count starts
    at ``step0`` with zero moments (the fold's device state), one ``masks`` pair per step."""
    ref = FrozenRefEEGNet(state, p=p)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3, eps=1e-7)
    for q in ref.parameters():
        opt.state[q] = dict(step=torch.tensor(float(step0)), exp_avg=torch.zeros_like(q), exp_avg_sq=torch.zeros_like(q))
    losses = []
    for masks in masks_per_step:
        loss = F.cross_entropy(ref(torch.as_tensor(x, dtype=torch.float64), masks), torch.as_tensor(y))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return {k: ref.params[k].detach().numpy() for k in PARAM_NAMES}, losses


def test_folds_match_the_float64_oracle_under_their_own_masks():
    C, T, B, p, offset, row0 = 22, 257, 5, 0.5, 42, 1
    steps = (0, 3, 7)
    folds = _make_folds(C, T, B, steps=steps)
    for f in folds:
        f.adam.zero_()
    states = [model_state(f.md) for f in folds]
    batches = [tuple(t.cpu().numpy() for t in f.rows(row0)) for f in folds]
    masks = [device_masks(B, 16, T, f.seed, offset + s, p) for f, s in zip(folds, steps)]
    _run_folds(folds, row0=row0, slot=0, offset=offset)
    refs = []
    for k, f in enumerate(folds):
        ref = oracle_frozen(states[k], batches[k][0], p, masks[k], labels=batches[k][1])
        refs.append(ref)
        assert_frozen_grads_close(flat_to_dict(f.md, f.grads), ref["grads"], raw=ref["raw"], prefix=f"fold {k} grad ")
        assert_close(f.losses.cpu().numpy()[0], ref["loss"], name=f"fold {k} loss")
    # the key is per fold: fold 1 under fold 0's masks is another function
    wrong = oracle_frozen(states[1], batches[1][0], p, masks[0], labels=batches[1][1])
    with pytest.raises(AssertionError):
        assert_frozen_grads_close(flat_to_dict(folds[1].md, folds[1].grads), wrong["grads"], raw=wrong["raw"])
    # two more calls: three Adam steps per fold, the masks following each fold's device step
    first = [float(f.losses[0]) for f in folds]
    _run_folds(folds, row0=row0, slot=1, offset=offset)
    _run_folds(folds, row0=row0, slot=2, offset=offset)
    for k, (f, s) in enumerate(zip(folds, steps)):
        mk = [device_masks(B, 16, T, f.seed, offset + s + i, p) for i in range(3)]
        want, ref_losses = _oracle_adam(states[k], p, batches[k][0], batches[k][1], mk, s)
        got = {n: v.detach().cpu().numpy() for n, v in f.md.named_parameters()}
        for n in PARAM_NAMES:              # the tolerance of test_three_fused_adam_steps_match_the_oracle
            assert_close(got[n], want[n], rtol=1e-5, atol_frac=1e-5, name=f"fold {k} Adam x3 {n}")
        assert int(f.step) == s + 3
        assert float(f.losses[0]) == first[k]
        assert_close(f.losses.cpu().numpy(), np.array(ref_losses), name=f"fold {k} Adam x3 losses")


# ---- 4. independence from nfolds and the table order ----
def test_a_fold_does_not_depend_on_nfolds_or_its_place_in_the_table():
    folds = _make_folds(22, 257, 3, steps=(0, 1, 2, 3, 4))
    single = [f.clone() for f in folds]
    _run_folds([folds[i] for i in (3, 0, 4, 1, 2)], row0=0, slot=2, offset=1)
    for k, s in enumerate(single):
        _run_folds([s], row0=0, slot=2, offset=1)
        _assert_same(folds[k], s, f"fold {k}")


# ---- 5. isolation ----
def test_a_non_finite_trial_stays_in_its_fold():
    B, row0 = 5, 2
    folds = _make_folds(22, 257, B, share_x=False)
    clean = [f.clone() for f in folds]
    _run_folds(clean, row0=row0, slot=0, offset=3)
    bad = folds[1]
    bad.X = bad.X.clone()
    bad.X[int(bad.perm[row0 + 2]), 3, 10] = float("nan")
    _run_folds(folds, row0=row0, slot=0, offset=3)
    for k in (0, 2):
        _assert_same(folds[k], clean[k], f"fold {k}")
    assert not bool(torch.isfinite(bad.grads).all())


# ---- 6. NO_CLAMP and gradients only ----
def test_no_clamp_and_a_fold_without_adam_state():
    from eegnetreplication_amd import ops
    folds = _make_folds(22, 257, 3)
    folds[1].adam = None
    start = [f.clone() for f in folds]
    raw, raw_alone = [f.clone() for f in start], [f.clone() for f in start]
    _run_folds(folds, row0=0, slot=0, offset=5)
    _run_folds(raw, row0=0, slot=0, offset=5, clamp=False)
    for k, (f, r, a, s) in enumerate(zip(folds, raw, raw_alone, start)):
        _run_alone(a, row0=0, slot=0, offset=5, clamp=False)
        _assert_same(r, a, f"NO_CLAMP fold {k}")
        # the clamped gradients are the clamp of the unclamped ones
        clamped = r.grads.clone()
        ops.clamp_grads(f.md.shape, clamped)
        assert torch.equal(clamped, f.grads), k
        if k == 1:                          # gradients only: parameters and step stay
            assert torch.equal(f.md.flat_parameters(), s.md.flat_parameters()) and int(f.step) == int(s.step)
            assert bool(torch.isfinite(f.grads).all())
        else:
            assert not torch.equal(f.md.flat_parameters(), s.md.flat_parameters()) and int(f.step) == int(s.step) + 1


# ---- 7. FrozenFoldBatch against loops ----
def _frozen_models(K, p, dev):
    return [copy.deepcopy(_model(22, 257, p=p, seed=k)).to(dev).freeze_bn().train() for k in range(K)]


def _epoch_sets(ns, dev):
    out = []
    for k, n in enumerate(ns):
        x, y = _data(n, 22, 257, 10 + k)
        out.append((torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)))
    return out


def _run_batch(p, sets, epochs, seeds, **kw):
    """(models, FrozenFoldBatch, per-epoch loss sums) after ``epochs`` epochs with per-fold generators."""
    from eegnetreplication_amd import FrozenFoldBatch
    models = _frozen_models(len(sets), p, _dev())
    fb = FrozenFoldBatch(models, seeds, **kw)
    gens = [torch.Generator().manual_seed(100 + k) for k in range(len(sets))]
    sums = [torch.stack(fb.epoch(sets, 64, gens)) for _ in range(epochs)]
    torch.cuda.synchronize()
    return models, fb, sums


def _assert_same_runs(a, b, what):
    (ma, fa, sa), (mb, fb, sb) = a, b
    for k in range(len(ma)):
        assert torch.equal(ma[k].flat_parameters(), mb[k].flat_parameters()), f"{what}: params {k}"
        assert torch.equal(fa.adam[k].state, fb.adam[k].state), f"{what}: Adam state {k}"
        assert torch.equal(fa.adam[k].step, fb.adam[k].step), f"{what}: step {k}"
    for e, (u, v) in enumerate(zip(sa, sb)):
        assert torch.equal(u, v), f"{what}: loss sums of epoch {e}"


def test_frozen_fold_batch_equals_the_loops():
    from eegnetreplication_amd import FusedTrainer, ops
    from eegnetreplication_amd.dataset import epoch_permutation
    dev = _dev()
    K, n, epochs, seeds = 3, 150, 2, [5, 6, 7]
    sets = _epoch_sets([n] * K, dev)
    fused = _run_batch(0.5, sets, epochs, seeds, fused=True)
    assert fused[1].fused and fused[1]._fz is not None and sorted(fused[1]._fz["tables"]) == [22, 64]
    loops = _run_batch(0.5, sets, epochs, seeds, fused=False)
    assert loops[1]._fz is None
    _assert_same_runs(fused, loops, "fused / per-fold")
    # a hand loop of frozen_step over the same shuffles
    ref = _frozen_models(K, 0.5, dev)
    bn0 = [(m.flat_bn_buffers().clone(), m.flat_num_batches_tracked().clone()) for m in ref]
    for k, (m, (X, y)) in enumerate(zip(ref, sets)):
        g = torch.Generator().manual_seed(100 + k)
        nprm = m.flat_parameters().numel()
        grads, adam = torch.zeros(nprm, device=dev), torch.zeros(2 * nprm, device=dev)
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        for e in range(epochs):
            perm = epoch_permutation(n, g).to(dev)
            Xp, yp = X[perm], y[perm]
            losses = torch.zeros(3, device=dev)
            for j, i in enumerate(range(0, n, 64)):
                xb, yb = Xp[i:i + 64].contiguous(), yp[i:i + 64].contiguous()
                ops.frozen_step(m.shape, m.flat_parameters(), m.flat_bn_buffers(), xb, seeds[k], 0, grads,
                                ops.new_frozen_workspace(m.shape, xb.shape[0], dev), labels=yb, adam_state=adam,
                                step_i32=step, loss=losses[j:j + 1], key_from_step=True)
            assert torch.equal(losses.sum(dtype=torch.float64), fused[2][e][k]), (k, e)
        assert torch.equal(m.flat_parameters(), fused[0][k].flat_parameters()), k
        assert torch.equal(adam, fused[1].adam[k].state) and int(step) == int(fused[1].adam[k].step) == 6
    for m, (bn, nbt) in zip(fused[0], bn0):
        assert torch.equal(m.flat_bn_buffers(), bn) and torch.equal(m.flat_num_batches_tracked(), nbt)
    # p = 0: no mask is drawn, so FusedTrainer on frozen clones is the same arithmetic
    fused0 = _run_batch(0.0, sets, epochs, seeds, fused=True)
    for k, (m, (X, y)) in enumerate(zip(_frozen_models(K, 0.0, dev), sets)):
        tr = FusedTrainer(m)
        g = torch.Generator().manual_seed(100 + k)
        for e in range(epochs):
            perm = epoch_permutation(n, g).to(dev)
            ls = []
            for i in range(0, n, 64):
                ls.append(tr.step(X[perm[i:i + 64]].contiguous(), y[perm[i:i + 64]].contiguous()).clone())
            tot = torch.cat(ls).sum(dtype=torch.float64)
            assert torch.equal(tot, fused0[2][e][k]), (k, e)
        assert torch.equal(m.flat_parameters(), fused0[0][k].flat_parameters()), k
        assert torch.equal(tr.adam.state, fused0[1].adam[k].state)


# ---- 8. graph replay ----
def test_graph_replays_equal_eager_epochs_and_draw_fresh_masks():
    dev = _dev()
    sets = _epoch_sets([150] * 3, dev)
    eager = _run_batch(0.5, sets, 3, [5, 6, 7], fused=True)
    graph = _run_batch(0.5, sets, 3, [5, 6, 7], fused=True, graphs=True)
    assert graph[1]._fz["graph"] is not None and eager[1]._fz["graph"] is None
    _assert_same_runs(eager, graph, "eager / graph")
    # lr = 0, no shuffle: the parameters and the batches stay, so two replays differ by their masks alone
    from eegnetreplication_amd import FrozenFoldBatch
    models = _frozen_models(3, 0.5, dev)
    p0 = [m.flat_parameters().clone() for m in models]
    fb = FrozenFoldBatch(models, [5, 6, 7], lr=0.0, fused=True, graphs=True)
    sums = [torch.stack(fb.epoch(sets, 64)).cpu() for _ in range(3)]
    assert all(torch.equal(m.flat_parameters(), q) for m, q in zip(models, p0))
    assert bool((sums[1] != sums[2]).all()) and bool(torch.isfinite(torch.stack(sums)).all())


# ---- 9. unequal n ----
def test_unequal_n_takes_the_per_fold_path():
    dev = _dev()
    sets = _epoch_sets([150, 100], dev)
    both = _run_batch(0.5, sets, 2, [5, 6], fused=True)
    assert both[1]._fz is None                        # never fused: the folds' epochs differ in length
    for k in range(2):
        from eegnetreplication_amd import FrozenFoldBatch
        m = _frozen_models(2, 0.5, dev)[k]
        fb = FrozenFoldBatch([m], [5 + k], fused=True)
        g = torch.Generator().manual_seed(100 + k)
        sums = [fb.epoch([sets[k]], 64, [g])[0] for _ in range(2)]
        torch.cuda.synchronize()
        assert fb._fz is not None
        assert torch.equal(m.flat_parameters(), both[0][k].flat_parameters()), k
        assert torch.equal(fb.adam[0].state, both[1].adam[k].state)
        assert all(torch.equal(s, both[2][e][k]) for e, s in enumerate(sums))
