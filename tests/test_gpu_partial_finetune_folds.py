"""GPU tests of partial fine-tuning over folds (eegnet_frozen_step_folds_from behind
``ops.frozen_step_folds(train_from=...)`` and ``FrozenFoldBatch`` on models cut by ``EEGNet.train_from``).

Three folds of n = 10 trials at batch 4 (the last batch has 2), at 22 x 257 and at 5 x 96 EEGNet-4,1.  The
contract is bit identity: each fold equals ``ops.frozen_step(train_from=s, key_from_step=True)`` on its own
gathered rows, the fused and the per-fold path agree, graph replays equal eager epochs, and the frozen
prefix of the parameters and of both Adam moments keeps its bits."""

from __future__ import annotations

import copy
import functools

import pytest
import torch

from golden_util import make_inputs
from hip_cases import random_model

pytestmark = pytest.mark.gpu

K, N, BATCH = 3, 10, 4
SEEDS = [5, 6, 7]
SENTINEL = -321.5           # what the Adam moments of a frozen parameter hold before and after
SHAPES = [(22, 257, 8, 2), (5, 96, 4, 1)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _model(C, T, F1, D, seed):
    """A CPU model with every BN term off its identity value; shared, never modified."""
    return random_model(C, T, F1=F1, D=D, p=0.5, seed=19 * seed + C + T)


@functools.lru_cache(maxsize=None)
def _data(C, T, seed):
    return make_inputs(N, C, T, 2300 + seed)


def _models(C, T, F1, D, stages):
    return [copy.deepcopy(_model(C, T, F1, D, k)).to(_dev()).freeze_bn().train_from(s).train()
            for k, s in enumerate(stages)]


def _sets(C, T):
    dev = _dev()
    return [tuple(torch.from_numpy(a).to(dev) for a in _data(C, T, k)) for k in range(K)]


def _mark_prefix(fb, models, stages):
    """The sentinel into both Adam moments of every fold's frozen prefix; returns the offsets."""
    from eegnetreplication_amd import ops
    offs = []
    for a, m, s in zip(fb.adam, models, stages):
        n, off = m.flat_parameters().numel(), ops.trainable_offset(m.shape, s)
        a.state[:off] = SENTINEL
        a.state[n:n + off] = SENTINEL
        offs.append(off)
    return offs


def _run_batch(C, T, F1, D, stages, epochs, cls=None, **kw):
    """(models, FrozenFoldBatch, per-epoch loss sums, initial parameters, offsets) after ``epochs`` epochs."""
    from eegnetreplication_amd import FrozenFoldBatch
    models = _models(C, T, F1, D, stages)
    before = [m.flat_parameters().clone() for m in models]
    fb = (cls or FrozenFoldBatch)(models, SEEDS, **kw)
    offs = _mark_prefix(fb, models, stages)
    gens = [torch.Generator().manual_seed(100 + k) for k in range(K)]
    sets = _sets(C, T)
    sums = [torch.stack(fb.epoch(sets, BATCH, gens)) for _ in range(epochs)]
    torch.cuda.synchronize()
    return models, fb, sums, before, offs


def _run_alone(C, T, F1, D, stages, epochs):
    """The same epochs fold by fold: ops.frozen_step(train_from=s, key_from_step=True) on each batch's
    gathered rows.  Returns per fold (parameters, Adam state, step, per-epoch loss sums)."""
    from eegnetreplication_amd import ops
    from eegnetreplication_amd.dataset import epoch_permutation
    dev = _dev()
    out = []
    for k, (m, (X, y)) in enumerate(zip(_models(C, T, F1, D, stages), _sets(C, T))):
        g = torch.Generator().manual_seed(100 + k)
        n, off = m.flat_parameters().numel(), ops.trainable_offset(m.shape, stages[k])
        grads, adam = torch.zeros(n, device=dev), torch.zeros(2 * n, device=dev)
        adam[:off] = SENTINEL
        adam[n:n + off] = SENTINEL
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        sums = []
        for _ in range(epochs):
            perm = epoch_permutation(N, g).to(dev)
            Xp, yp = X[perm], y[perm]
            losses = torch.zeros((N + BATCH - 1) // BATCH, device=dev)
            for j, i in enumerate(range(0, N, BATCH)):
                xb, yb = Xp[i:i + BATCH].contiguous(), yp[i:i + BATCH].contiguous()
                ops.frozen_step(m.shape, m.flat_parameters(), m.flat_bn_buffers(), xb, SEEDS[k], 0, grads,
                                ops.new_frozen_workspace(m.shape, xb.shape[0], dev), labels=yb, adam_state=adam,
                                step_i32=step, loss=losses[j:j + 1], key_from_step=True, train_from=stages[k])
            sums.append(losses.sum(dtype=torch.float64))
        torch.cuda.synchronize()
        out.append((m.flat_parameters().clone(), adam, int(step), sums))
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_equals_alone(run, alone, what):
    models, fb, sums, before, offs = run
    for k, (prm, adam, step, ls) in enumerate(alone):
        assert torch.equal(_bits(models[k].flat_parameters()), _bits(prm)), f"{what}: params of fold {k}"
        assert torch.equal(_bits(fb.adam[k].state), _bits(adam)), f"{what}: Adam state of fold {k}"
        assert int(fb.adam[k].step) == step
        for e, s in enumerate(ls):
            assert torch.equal(sums[e][k], s), f"{what}: loss sum of fold {k}, epoch {e}"


def _assert_prefix_untouched(run, what):
    models, fb, sums, before, offs = run
    for k, (m, off) in enumerate(zip(models, offs)):
        n = m.flat_parameters().numel()
        want = torch.full((off,), SENTINEL, device=_dev())
        assert torch.equal(_bits(m.flat_parameters()[:off]), _bits(before[k][:off])), f"{what}: frozen params {k}"
        assert torch.equal(_bits(fb.adam[k].state[:off]), _bits(want)), f"{what}: frozen exp_avg {k}"
        assert torch.equal(_bits(fb.adam[k].state[n:n + off]), _bits(want)), f"{what}: frozen exp_avg_sq {k}"
        assert off == 0 or not torch.equal(m.flat_parameters()[off:], before[k][off:]), f"{what}: fold {k} did not train"


@pytest.mark.parametrize("stage", ["block_2", "classifier"])
@pytest.mark.parametrize("C,T,F1,D", SHAPES)
def test_fused_folds_equal_the_single_model_step(C, T, F1, D, stage):
    run = _run_batch(C, T, F1, D, [stage] * K, 1, fused=True)
    assert run[1]._fz is not None and sorted(run[1]._fz["tables"]) == [2, 4]
    _assert_equals_alone(run, _run_alone(C, T, F1, D, [stage] * K, 1), f"fused {stage}")
    _assert_prefix_untouched(run, f"fused {stage}")
    # the per-fold path is the same arithmetic
    loops = _run_batch(C, T, F1, D, [stage] * K, 1, fused=False)
    assert loops[1]._fz is None
    for k in range(K):
        assert torch.equal(_bits(run[0][k].flat_parameters()), _bits(loops[0][k].flat_parameters()))
        assert torch.equal(_bits(run[1].adam[k].state), _bits(loops[1].adam[k].state))
    assert torch.equal(run[2][0], loops[2][0])


@pytest.mark.parametrize("stage", ["block_2", "classifier"])
@pytest.mark.parametrize("C,T,F1,D", SHAPES)
def test_graph_replay_equals_eager_epochs(C, T, F1, D, stage):
    eager = _run_batch(C, T, F1, D, [stage] * K, 2, fused=True)
    graph = _run_batch(C, T, F1, D, [stage] * K, 2, fused=True, graphs=True)
    assert graph[1]._fz["graph"] is not None and eager[1]._fz["graph"] is None
    for k in range(K):
        assert torch.equal(_bits(eager[0][k].flat_parameters()), _bits(graph[0][k].flat_parameters())), k
        assert torch.equal(_bits(eager[1].adam[k].state), _bits(graph[1].adam[k].state)), k
        assert int(eager[1].adam[k].step) == int(graph[1].adam[k].step) == 6
    for e in range(2):
        assert torch.equal(eager[2][e], graph[2][e]), e
    _assert_prefix_untouched(graph, f"graph {stage}")


def test_mixed_stages_with_fused_launches_raise():
    from eegnetreplication_amd import FrozenFoldBatch
    models = _models(22, 257, 8, 2, ["block_2", "classifier", "block_2"])
    with pytest.raises(ValueError, match="same trainable stage for every fold"):
        FrozenFoldBatch(models, SEEDS, fused=True)
    # mixed after construction: the epoch checks before any device work
    fb = FrozenFoldBatch(_models(22, 257, 8, 2, ["block_2"] * K), SEEDS, fused=True)
    fb.models[1].train_from("classifier")
    before = [m.flat_parameters().clone() for m in fb.models]
    with pytest.raises(ValueError, match="same trainable stage for every fold"):
        fb.epoch(_sets(22, 257), BATCH)
    torch.cuda.synchronize()
    assert all(torch.equal(m.flat_parameters(), b) for m, b in zip(fb.models, before))


@pytest.mark.parametrize("C,T,F1,D", SHAPES)
def test_mixed_stages_fall_back_to_the_per_fold_path(C, T, F1, D):
    from eegnetreplication_amd import FrozenFoldBatch

    class Eager(FrozenFoldBatch):
        FUSED_MIN_FOLDS = 1            # fused=None takes the fused launches whenever they apply

    stages = ["classifier", "temporal", "block_2"]
    run = _run_batch(C, T, F1, D, stages, 1, cls=Eager, fused=None)
    assert run[1]._fz is None                          # mixed stages: never fused
    _assert_equals_alone(run, _run_alone(C, T, F1, D, stages, 1), "mixed stages")
    _assert_prefix_untouched(run, "mixed stages")
    uniform = _run_batch(C, T, F1, D, ["block_2"] * K, 1, cls=Eager, fused=None)
    assert uniform[1]._fz is not None                  # one stage: the fused launches
