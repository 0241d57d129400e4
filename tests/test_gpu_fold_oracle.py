"""Fold-indexed train steps (eegnet_train_step_folds, what train.py --fold-batch runs for both
protocols) against the float64 oracle, launch by launch.

tests/test_gpu_folds.py and tests/test_gpu_sharding.py compare fold launches with themselves
(torch.equal) or post-Adam parameters after a few steps; Adam normalises each element's step, so a
gradient that is a few per cent off moves those parameters by less than their tolerance.  Here the
table is built and launched directly (ops.fold_table / ops.train_step_folds, as FoldBatch._fused_state
and _fused_steps do) and after EVERY launch each fold's loss slot, all 12 gradients, the six running
statistics, the three num_batches_tracked counters, the Adam step and the post-Adam parameters are
compared with oracle/numpy_ref.train_step on the rows the launch trained on.

One launch advances K = 3 folds: different parameters and BN state, own X of 150 trials, own seed,
own non-identity permutation (dataset.epoch_permutation).  The epoch's three batches are rows
[0, 64), [64, 128) and the short [128, 150).  The oracle carries parameters, BN buffers and Adam
moments in float64 from step to step; before launches 2 and 3 that state, rounded to fp32, is copied
into the device fold, so every launch starts where its reference step starts and parameter drift
stays out of the gradient comparison.

Dropout: the fold kernels draw the keep factor of batch row b from the index (b F2 + o) T1 + q and
b NF + i -- the row of the BATCH (the workspace row), not the permuted row perm[row0 + b] of x
(eegnet_stream.hip k_pass_b, eegnet_passes.hip k_pass_c / k_pass_dr: only x, xstat and the labels go
through fold_row) -- under the key mix(seed_k, offset + *step_k).  The reference masks are therefore
hip_cases.device_masks(B, F2, T, seed_k, offset + step_k, p) applied to the gathered batch.

Tolerances are the project's (tests/golden_util.py: rtol 1e-4, atol 1e-5 max|ref|, the near-zero
gradient rule; loss within 1e-4 max(1, |ref|); running statistics as test_gpu_coverage._check_step).

The epoch-level test drives FoldBatch.epoch itself (fused launches, eager and hipGraph replay, with
and without the x statistics table) for two epochs and compares with the float64 loop of
tests/test_gpu_protocols.py at that test's tolerances."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from golden_util import PARAM_NAMES, assert_close, assert_grads_close, assert_params_close
from hip_cases import device_masks, flat_to_dict, random_model, state_np

pytestmark = pytest.mark.gpu

N = 150                                     # trials per fold: batches of 64, 64 and 22
LAUNCHES = ((0, 64), (64, 64), (128, 22))   # (row0, B)
K = 3
OFFSET = 7                                  # eegnet_train_step_folds' key offset

SHAPES = [
    # C, T, F1, D, K1, p
    (22, 257, 8, 2, 32, 0.5),
    (22, 256, 8, 2, 32, 0.25),
    (8, 64, 8, 2, 32, 0.25),
    (16, 200, 2, 2, 32, 0.25),
    (8, 100, 4, 1, 32, 0.5),
    (3, 64, 8, 2, 64, 0.25),
    (4, 800, 8, 2, 32, 0.25),
    (22, 257, 8, 2, 32, 0.0),
]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _case(C, T, F1, D, K1, p, share=None):
    """The inputs of one case, host side: per fold the model, X, y, seed and permutation.
    ``share``: {fold: fold whose X it reads} (own labels, seed and permutation)."""
    from eegnetreplication_amd.dataset import epoch_permutation
    share = share or {}
    folds = []
    for k in range(K):
        rng = np.random.default_rng(1000 * C + T + 17 * k)
        X = rng.standard_normal((N, C, T), dtype=np.float32)
        y = rng.integers(0, 4, N).astype(np.int64)
        seed = 0x5EED_0000 + 977 * k + T
        perm = epoch_permutation(N, torch.Generator().manual_seed(50 + k)).numpy()
        folds.append(dict(model=random_model(C, T, F1=F1, D=D, K1=K1, p=p, seed=3 * C + T + 5 * k),
                          X=X, y=y, seed=seed, perm=perm))
    for k, src in share.items():
        folds[k]["X"] = folds[src]["X"]
    for f in folds:
        assert not np.array_equal(f["perm"], np.arange(N))
    return folds


_REF = {}


def _reference(key, folds, p, F2, T):
    """Per fold the three float64 oracle steps of the epoch (computed once per case and shared by its
    xstat / pitch variants): [{loss, grads, params, buffers, adam m / v} per launch]."""
    from oracle import numpy_ref as nr
    if key in _REF:
        return _REF[key]
    out = []
    for f in folds:
        params, bufs = state_np(f["model"])
        params = {k: v.astype(np.float64) for k, v in params.items()}
        st = nr.adam_init(params)
        steps = []
        for step, (row0, B) in enumerate(LAUNCHES):
            idx = f["perm"][row0:row0 + B]
            masks = device_masks(B, F2, T, f["seed"], OFFSET + step, p) if p > 0 else None
            r = nr.train_step(params, bufs, f["X"][idx].astype(np.float64), f["y"][idx], st, p=p, masks=masks)
            params, bufs = r["params"], r["buffers"]
            steps.append(dict(loss=r["loss"], grads=r["grads"], params=params, buffers=bufs,
                              m={k: v.copy() for k, v in st.m.items()}, v={k: v.copy() for k, v in st.v.items()}))
        out.append(steps)
    _REF[key] = out
    return out


def _flat32(d, names, dev):
    a = np.concatenate([np.asarray(d[k], dtype=np.float64).reshape(-1) for k in names])
    return torch.from_numpy(a.astype(np.float32)).to(dev)


def _run(C, T, F1, D, K1, p, *, xstat, pitched=False, use_perm=True, share=None, tag=""):
    from eegnetreplication_amd import ops
    from eegnetreplication_amd.model import FusedAdamState
    dev = _dev()
    folds = _case(C, T, F1, D, K1, p, share)
    F2 = F1 * D
    ref = _reference((C, T, F1, D, K1, p, tuple(sorted((share or {}).items()))), folds, p, F2, T)
    if not use_perm:
        # the table's perm is NULL and X / y are handed over in epoch order: the same batches, and
        # (the dropout index being the batch row) the same masks, so the same reference steps
        assert not share
        for f in folds:
            f["X"], f["y"], f["perm"] = f["X"][f["perm"]], f["y"][f["perm"]], None
    shape = folds[0]["model"].shape
    bn_names = [n for n, _ in shape.bn_layout()]
    # every workgroup of every pass of the full batches runs at least two trials of its fold.  Pass C
    # is counted in per-wave streams: its workgroups take 16 trials each, two per wave at the runtime
    # shapes (8 waves) and one per wave at the two compile-time shapes (16 waves)
    grids = ops.launch_grids(shape, 64, fold_launch=True)
    assert all(64 // grids[k] >= 2 for k in "ABDE"), grids
    spec = (C, F1, D, K1) == (22, 8, 2, 32) and T in (256, 257)
    assert 64 // grids["C"] == (1 if spec else 2), grids
    pitch = shape.x_pitch() if pitched else T
    assert pitch != T or not pitched
    xdev, dv = {}, []
    for f in folds:
        m = f["model"].to(dev).train()
        if id(f["X"]) not in xdev:          # one device copy (and one table) per distinct X
            rows = torch.from_numpy(f["X"]).to(dev)
            if pitched:
                rows = ops.pad_x_rows(rows, pitch)
            xdev[id(f["X"])] = (rows, ops.x_stats(shape, rows) if xstat else None)
        rows, stat = xdev[id(f["X"])]
        flat, bn, nbt = m.flat_views()
        dv.append(dict(m=m, flat=flat, bn=bn, nbt=nbt, adam=FusedAdamState(m), rows=rows, stat=stat,
                       y=torch.from_numpy(f["y"]).to(dev),
                       perm=torch.from_numpy(f["perm"]).to(dev) if f["perm"] is not None else None,
                       losses=torch.zeros(len(LAUNCHES), dtype=torch.float32, device=dev),
                       ws={B: ops.new_workspace(shape, B, dev) for B in {b for _, b in LAUNCHES}}))
    if share:
        assert len(xdev) < K
    tables = {}
    for B in {b for _, b in LAUNCHES}:
        tables[B] = ops.fold_table(
            [dict(params=d["flat"], bn_buffers=d["bn"], num_batches_tracked=d["nbt"], x=d["rows"], xstat=d["stat"],
                  labels=d["y"], perm=d["perm"], grads=d["adam"].grads, adam_state=d["adam"].state,
                  step=d["adam"].step, losses=d["losses"], ws=d["ws"][B], seed=f["seed"])
             for d, f in zip(dv, folds)], dev)
    for step, (row0, B) in enumerate(LAUNCHES):
        if step:                            # start from the reference's state (fp32-rounded)
            for k, d in enumerate(dv):
                prev = ref[k][step - 1]
                d["flat"].copy_(_flat32(prev["params"], PARAM_NAMES, dev))
                d["bn"].copy_(_flat32(prev["buffers"], bn_names, dev))
                d["adam"].state.copy_(torch.cat([_flat32(prev["m"], PARAM_NAMES, dev),
                                                 _flat32(prev["v"], PARAM_NAMES, dev)]))
        ops.train_step_folds(shape, B, tables[B], K, row0=row0, slot=step, offset=OFFSET,
                             x_pitch=pitch if pitched else 0)
        torch.cuda.synchronize()
        for k, d in enumerate(dv):
            r = ref[k][step]
            what = f"{tag}fold {k} launch {step + 1} (row0 {row0}, B {B}) "
            loss = float(d["losses"][step])
            assert abs(loss - r["loss"]) <= 1e-4 * max(1.0, abs(r["loss"])), f"{what}loss {loss} vs {r['loss']}"
            assert_grads_close(flat_to_dict(d["m"], d["adam"].grads), r["grads"], prefix=what + "grad.")
            bn = d["bn"].cpu().numpy()
            o = 0
            for name, n in shape.bn_layout():
                got, want = bn[o:o + n], np.asarray(r["buffers"][name], dtype=np.float64)
                o += n
                if name.endswith("running_mean"):
                    assert_close(got, want, atol_abs=1e-5 * max(1.0, float(np.abs(want).max())), name=what + name)
                else:
                    assert_close(got, want, name=what + name)
            assert d["nbt"].tolist() == [step + 1] * 3, f"{what}num_batches_tracked {d['nbt'].tolist()}"
            for name in ("temporal.1", "aggregation.0", "block_2.2"):
                assert int(r["buffers"][name + ".num_batches_tracked"]) == step + 1
            assert int(d["adam"].step.item()) == step + 1, what + "Adam step"
            assert_params_close(flat_to_dict(d["m"], d["flat"]), r["params"], steps=step + 1,
                                prefix=what + "param.")
        # the slots of later launches are untouched
        for d in dv:
            assert torch.count_nonzero(d["losses"][step + 1:]).item() == 0


@pytest.mark.parametrize("xstat", [True, False], ids=["xstat", "noxstat"])
@pytest.mark.parametrize("C,T,F1,D,K1,p", SHAPES)
def test_fold_launches_match_oracle(C, T, F1, D, K1, p, xstat):
    _run(C, T, F1, D, K1, p, xstat=xstat)


@pytest.mark.parametrize("xstat", [True, False], ids=["xstat", "noxstat"])
def test_fold_launches_match_oracle_pitched_x(xstat):
    """22 x 257 with x rows at the pitch the kernels load fastest (260 floats, ops.pad_x_rows): what
    FoldBatch hands the fold launches for the recordings' shape."""
    from eegnetreplication_amd.ops import Shape
    assert Shape(22, 257).x_pitch() == 260
    _run(22, 257, 8, 2, 32, 0.5, xstat=xstat, pitched=True, tag="pitch 260 ")


def test_fold_launches_without_perm_match_oracle():
    """perm = NULL: batch row r is row row0 + r of an X (and labels) already in epoch order."""
    _run(22, 257, 8, 2, 32, 0.5, xstat=True, pitched=True, use_perm=False, tag="no perm ")


def test_folds_sharing_one_x_match_oracle():
    """Folds 0 and 2 read the same X and the same statistics table through different permutations,
    labels, seeds and parameters (repeats of one cross-subject split share their training set)."""
    _run(8, 64, 8, 2, 32, 0.25, xstat=True, share={2: 0}, tag="shared X ")


# ---------------------------------------------------------------------------------------------
# FoldBatch.epoch over two epochs vs the float64 loop
# ---------------------------------------------------------------------------------------------
_EPOCH_REF = {}


def _epoch_reference(C, T, data, gen_seeds, models):
    from hip_cases import oracle_train_loop as _oracle_train    # test_gpu_protocols' float64 loop
    key = (C, T)
    if key not in _EPOCH_REF:
        out = []
        for (X, y, Xv, yv), gs, m in zip(data, gen_seeds, models):
            p0 = {k: v.detach().numpy().copy() for k, v in m.named_parameters()}
            b0 = {k: v.detach().numpy().copy() for k, v in m.named_buffers()}
            out.append(_oracle_train(p0, b0, X.astype(np.float64), y, Xv.astype(np.float64), yv, 2, gs))
        _EPOCH_REF[key] = out
    return _EPOCH_REF[key]


@pytest.mark.parametrize("xstats", [True, False], ids=["xstat", "noxstat"])
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("C,T", [(8, 64), (22, 257)])
def test_fold_batch_epochs_match_oracle(C, T, graphs, xstats):
    """2 epochs of FoldBatch.epoch (fused=True: fold-indexed launches; graphs=True replays epoch 2 from
    the captured graph) on 2 folds of 150 trials (p = 0, batch 64 with a short last batch, each fold
    shuffled by its own seeded generator) and FoldBatch.validate after every epoch: per-epoch train /
    validation losses, validation accuracies, final weights, BN running statistics and counters
    against the float64 loop over the same batches, compared as
    test_gpu_protocols.test_train_loop_matches_oracle_over_epochs compares FusedTrainer."""
    from eegnetreplication_amd import EEGNet, FoldBatch
    dev = _dev()
    nfold, epochs, steps = 2, 2, 6
    data, models, gen_seeds = [], [], [9, 10]
    for k in range(nfold):
        rng = np.random.default_rng(21 + k)
        data.append((rng.standard_normal((N, C, T), dtype=np.float32), rng.integers(0, 4, N).astype(np.int64),
                     rng.standard_normal((70, C, T), dtype=np.float32), rng.integers(0, 4, 70).astype(np.int64)))
        torch.manual_seed(4 + k)
        models.append(EEGNet(C, T, p=0.0))
    ref = _epoch_reference(C, T, data, gen_seeds, models)
    models = [m.to(dev) for m in models]
    fb = FoldBatch(models, [1, 2], graphs=graphs, fused=True, xstats=xstats)
    train = [(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)) for X, y, _, _ in data]
    val = [(torch.from_numpy(Xv).to(dev), torch.from_numpy(yv).to(dev)) for _, _, Xv, yv in data]
    gens = [torch.Generator().manual_seed(s) for s in gen_seeds]
    tl = [[] for _ in range(nfold)]
    vl = [[] for _ in range(nfold)]
    va = [[] for _ in range(nfold)]
    for _ in range(epochs):
        sums = fb.epoch(train, 64, gens)
        loss, correct = fb.validate(val, 64)
        torch.cuda.synchronize()
        for k in range(nfold):
            tl[k].append(float(sums[k]) / 3)
            vl[k].append(float(loss[k]))
            va[k].append(100 * int(correct[k]) / 70)
    if graphs:
        assert fb._fz["graph"] is not None
    for k, model in enumerate(models):
        params, bufs, otl, ovl, ova = ref[k]
        np.testing.assert_allclose(tl[k], otl, rtol=2e-4)
        np.testing.assert_allclose(vl[k], ovl, rtol=2e-4)
        assert va[k] == ova
        assert_params_close({n: q.detach().cpu().numpy() for n, q in model.named_parameters()}, params,
                            steps=steps, rtol=2e-4, atol_frac=2e-4, prefix=f"fold {k} ")
        # BN2's running statistics follow gamma1 / beta1, whose gradients are rounding residue
        # (test_gpu_protocols.test_train_loop_matches_oracle_over_epochs: the same bounds)
        hp = {n: q.detach().cpu().numpy().astype(np.float64) for n, q in model.named_parameters()}
        dbeta = float(np.abs(hp["temporal.1.bias"] - params["temporal.1.bias"]).max())
        dgam = float((np.abs(hp["temporal.1.weight"] - params["temporal.1.weight"])
                      / np.abs(params["temporal.1.weight"])).max())
        cap = 2 * 1e-3 * steps
        assert dbeta <= cap
        assert float(np.abs(hp["temporal.1.weight"] - params["temporal.1.weight"]).max()) <= cap
        W = float(np.abs(params["spatial.weight"].reshape(16, -1).sum(1)).max())
        for n, b in model.named_buffers():
            got = b.detach().cpu().numpy()
            if "num_batches_tracked" in n:
                assert int(b) == steps
            elif n == "aggregation.0.running_mean":
                assert_close(got, bufs[n], rtol=2e-4, atol_abs=1e-5 + 2 * dbeta * W, name=f"fold {k} {n}")
            elif n == "aggregation.0.running_var":
                assert_close(got, bufs[n], rtol=2e-4 + 4 * dgam, atol_abs=1e-5, name=f"fold {k} {n}")
            else:
                assert_close(got, bufs[n], rtol=2e-4, atol_abs=1e-5, name=f"fold {k} {n}")
        assert int(fb.adam[k].step.item()) == steps
