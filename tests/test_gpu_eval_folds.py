"""Fold-indexed validation (eegnet_eval_folds: k_eval_folds + k_eval_folds_reduce) on the GPU.

k_eval_folds runs k_infer's per-trial code with the model taken from a fold record, and no arithmetic
crosses trials, so the bar for the logits is bit-equality with ``ops.forward_eval`` on each fold alone;
``pred`` and ``correct`` are exact; the per-trial CE and the validation loss are compared with the
float64 helper of tests/eval_cases.py (pinned to the reference loop by tests/test_eval_folds_cpu.py)
applied to the kernel's own logits, to the project's loss tolerance 1e-4 * max(1, |ref|)."""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from eval_cases import loss_tol, val_metrics

pytestmark = pytest.mark.gpu

SENTINEL_L, SENTINEL_C = -12345.5, -777


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _shape(C, T):
    from eegnetreplication_amd.ops import Shape
    return Shape(C=C, T=T)


def _rand_model(shape, rng, dev):
    """Flat parameters and BN buffers of a random model, the running statistics randomised too."""
    prm = torch.from_numpy((0.3 * rng.standard_normal(shape.n_params())).astype(np.float32))
    bn = []
    for name, n in shape.bn_layout():
        bn.append(0.2 * rng.standard_normal(n) if name.endswith("mean") else rng.uniform(0.5, 1.5, n))
    return prm.to(dev), torch.from_numpy(np.concatenate(bn).astype(np.float32)).to(dev)


def _rand_set(shape, n, rng, dev):
    x = torch.from_numpy(rng.standard_normal((n, shape.C, shape.T), dtype=np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, 4, n).astype(np.int64)).to(dev)
    return x, y


def _folds(shape, sizes, seed, dev):
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        prm, bn = _rand_model(shape, rng, dev)
        x, y = _rand_set(shape, n, rng, dev)
        out.append(dict(prm=prm, bn=bn, x=x, y=y))
    return out


def _run(shape, folds, batch=64, slot=0, nslots=1, labels=True, logits=True, scratch=True, sums=True):
    """One eegnet_eval_folds call on freshly sentinel-filled outputs; returns them per fold."""
    from eegnetreplication_amd import ops
    dev = folds[0]["prm"].device
    K = len(folds)
    loss = torch.full((K, nslots), SENTINEL_L, dtype=torch.float64, device=dev)
    corr = torch.full((K, nslots), SENTINEL_C, dtype=torch.int64, device=dev)
    ents, outs = [], []
    for k, f in enumerate(folds):
        n = f["x"].shape[0]
        o = dict(logits=torch.full((n, 4), SENTINEL_L, dtype=torch.float32, device=dev),
                 ce=torch.full((n,), SENTINEL_L, dtype=torch.float32, device=dev),
                 pred=torch.full((n,), SENTINEL_C, dtype=torch.int32, device=dev))
        outs.append(o)
        ents.append(dict(params=f["prm"], bn_buffers=f["bn"], x=f["x"], labels=f["y"] if labels else None, n=n,
                         logits=o["logits"] if logits else None, ce=o["ce"] if scratch else None,
                         pred=o["pred"] if scratch else None, loss=loss[k] if sums else None,
                         correct=corr[k] if sums else None))
    table = ops.eval_fold_table(ents, dev)
    ops.eval_folds(shape, table, K, max(f["x"].shape[0] for f in folds), batch=batch, slot=slot)
    torch.cuda.synchronize()
    return outs, loss, corr


def _check(shape, folds, outs, loss, corr, batch, slot):
    from eegnetreplication_amd import ops
    for k, (f, o) in enumerate(zip(folds, outs)):
        n = f["x"].shape[0]
        if n:
            ref = ops.forward_eval(shape, f["prm"], f["bn"], f["x"])
            assert torch.equal(o["logits"], ref), f"fold {k}: logits differ from forward_eval"
            assert torch.equal(o["pred"].long(), torch.argmax(o["logits"], 1)), k
        want_correct = int((o["pred"].long() == f["y"]).sum())
        ce, ref_loss, ref_correct = val_metrics(o["logits"].cpu().numpy(), f["y"].cpu().numpy(), batch)
        got_ce, got_loss = o["ce"].double().cpu().numpy(), float(loss[k, slot])
        print(f"fold {k} n={n}: loss {got_loss!r} ref {ref_loss!r}; max |ce - ref| "
              f"{np.abs(got_ce - ce).max() if n else 0.0:.3e}; correct {int(corr[k, slot])}")
        assert int(corr[k, slot]) == want_correct == ref_correct, k
        assert np.all(np.abs(got_ce - ce) <= loss_tol(ce)), k
        assert abs(got_loss - ref_loss) <= loss_tol(ref_loss), k
        for s in range(loss.shape[1]):
            if s != slot:
                assert float(loss[k, s]) == SENTINEL_L and int(corr[k, s]) == SENTINEL_C, (k, s)


@pytest.mark.parametrize("C,T,sizes", [(8, 64, [1, 65, 130]), (22, 256, [1, 65, 130]), (22, 257, [3, 64])],
                         ids=["8x64-runtime", "22x256", "22x257"])
def test_per_fold_equality(C, T, sizes):
    dev = _dev()
    shape = _shape(C, T)
    folds = _folds(shape, sizes, 11, dev)
    outs, loss, corr = _run(shape, folds, batch=64, slot=1, nslots=3)
    _check(shape, folds, outs, loss, corr, 64, 1)


@pytest.mark.parametrize("batch", [1, 64, 1000])
def test_edge_sizes(batch):
    """An empty fold between two others; folds far smaller than the workgroups that cover their share
    of the grid (one trial beside 300: most workgroups of the small fold's range find nothing to do);
    batch = 1 and batch >= n (a plain mean)."""
    dev = _dev()
    shape = _shape(8, 64)
    folds = _folds(shape, [3, 0, 300, 1], 12, dev)
    outs, loss, corr = _run(shape, folds, batch=batch)
    _check(shape, folds, outs, loss, corr, batch, 0)
    assert float(loss[1, 0]) == 0.0 and int(corr[1, 0]) == 0
    if batch == 1000:
        for k in (0, 2, 3):
            mean = float(outs[k]["ce"].double().mean())
            assert abs(float(loss[k, 0]) - mean) <= 1e-12 * max(1.0, abs(mean))


def test_all_folds_empty():
    dev = _dev()
    shape = _shape(8, 64)
    folds = _folds(shape, [0, 0], 13, dev)
    _, loss, corr = _run(shape, folds)
    assert loss.flatten().tolist() == [0.0, 0.0] and corr.flatten().tolist() == [0, 0]


@pytest.mark.parametrize("C,T,n", [(22, 257, 70), (8, 64, 5)])
def test_one_fold(C, T, n):
    dev = _dev()
    shape = _shape(C, T)
    folds = _folds(shape, [n], 14, dev)
    outs, loss, corr = _run(shape, folds)
    _check(shape, folds, outs, loss, corr, 64, 0)


def test_more_folds_than_cus():
    """300 folds of two trials: every workgroup's range spans several folds, so it rebuilds the per-fold
    operands on the way."""
    from eegnetreplication_amd import ops
    dev = _dev()
    shape = _shape(8, 64)
    K, n = 300, 2
    rng = np.random.default_rng(15)
    P = torch.from_numpy((0.3 * rng.standard_normal((K, shape.n_params()))).astype(np.float32)).to(dev)
    nbn = sum(m for _, m in shape.bn_layout())
    Bn = torch.from_numpy(rng.uniform(0.5, 1.5, (K, nbn)).astype(np.float32)).to(dev)
    X, Y = _rand_set(shape, K * n, rng, dev)
    folds = [dict(prm=P[k], bn=Bn[k], x=X[n * k:n * k + n], y=Y[n * k:n * k + n]) for k in range(K)]
    outs, loss, corr = _run(shape, folds)
    # one reference launch per distinct model would be 300 tiny launches all the same: compare in bulk
    got = torch.cat([o["logits"] for o in outs])
    ref = torch.cat([ops.forward_eval(shape, f["prm"], f["bn"], f["x"]) for f in folds])
    assert torch.equal(got, ref)
    pred = torch.cat([o["pred"] for o in outs]).long()
    assert torch.equal(pred, ref.argmax(1))
    assert torch.equal(corr[:, 0], (pred == Y).view(K, n).sum(1))
    ce = torch.cat([o["ce"] for o in outs]).double().cpu().numpy()
    ref_ce, _, _ = val_metrics(ref.cpu().numpy(), Y.cpu().numpy(), 64)
    assert np.all(np.abs(ce - ref_ce) <= loss_tol(ref_ce))
    want = ref_ce.reshape(K, n).mean(1)
    assert np.all(np.abs(loss[:, 0].cpu().numpy() - want) <= loss_tol(want))


def test_ties_predict_class_zero():
    dev = _dev()
    shape = _shape(22, 257)
    folds = _folds(shape, [9], 16, dev)
    nf = 4 * shape.F2 * (shape.T // 32)
    folds[0]["prm"][-(nf + 4):] = 0.0              # classifier weight and bias: all logits equal
    outs, loss, corr = _run(shape, folds)
    assert torch.equal(outs[0]["logits"], torch.zeros_like(outs[0]["logits"]))
    assert torch.equal(outs[0]["pred"], torch.zeros_like(outs[0]["pred"]))       # as torch.argmax
    assert torch.equal(torch.argmax(outs[0]["logits"], 1).int(), outs[0]["pred"])
    ce = outs[0]["ce"].double().cpu().numpy()
    assert np.all(np.abs(ce - math.log(4.0)) <= loss_tol(math.log(4.0)))
    assert abs(float(loss[0, 0]) - math.log(4.0)) <= loss_tol(math.log(4.0))
    assert int(corr[0, 0]) == int((folds[0]["y"] == 0).sum())


def test_label_free_use_writes_logits_only():
    from eegnetreplication_amd import ops
    dev = _dev()
    shape = _shape(22, 256)
    folds = _folds(shape, [5, 67], 17, dev)
    outs, loss, corr = _run(shape, folds, labels=False)
    for f, o in zip(folds, outs):
        assert torch.equal(o["logits"], ops.forward_eval(shape, f["prm"], f["bn"], f["x"]))
        assert torch.all(o["ce"] == SENTINEL_L)                                  # no labels: no CE
        assert torch.equal(o["pred"].long(), torch.argmax(o["logits"], 1))       # pred needs none
    assert torch.all(loss == SENTINEL_L) and torch.all(corr == SENTINEL_C)
    # and with every optional output NULL but the logits
    outs, loss, corr = _run(shape, folds, labels=False, scratch=False, sums=False)
    for f, o in zip(folds, outs):
        assert torch.equal(o["logits"], ops.forward_eval(shape, f["prm"], f["bn"], f["x"]))
        assert torch.all(o["ce"] == SENTINEL_L) and torch.all(o["pred"] == SENTINEL_C)
    assert torch.all(loss == SENTINEL_L) and torch.all(corr == SENTINEL_C)


def test_shared_inputs():
    """Two folds on the same x / labels with different parameters: each as if evaluated alone."""
    dev = _dev()
    shape = _shape(22, 257)
    a, b = _folds(shape, [70, 1], 18, dev)
    b["x"], b["y"] = a["x"], a["y"]
    outs, loss, corr = _run(shape, [a, b])
    _check(shape, [a, b], outs, loss, corr, 64, 0)
    for k, f in enumerate((a, b)):
        o1, l1, c1 = _run(shape, [f])
        assert torch.equal(o1[0]["logits"], outs[k]["logits"]) and torch.equal(o1[0]["ce"], outs[k]["ce"])
        assert torch.equal(l1[0], loss[k]) and torch.equal(c1[0], corr[k])
    assert not torch.equal(outs[0]["logits"], outs[1]["logits"])


def test_reproducible_bits():
    dev = _dev()
    shape = _shape(22, 257)
    folds = _folds(shape, [130, 65, 7], 19, dev)
    o1, l1, c1 = _run(shape, folds)
    o2, l2, c2 = _run(shape, folds)
    assert torch.equal(l1, l2) and torch.equal(c1, c2)
    for a, b in zip(o1, o2):
        assert torch.equal(a["ce"], b["ce"]) and torch.equal(a["logits"], b["logits"])


# ---- the Python entry point -------------------------------------------------------------------------
def _modules(k, C, T, dev, seed=5):
    from eegnetreplication_amd import EEGNet
    torch.manual_seed(seed)
    models = [EEGNet(C, T, p=0.25 if i % 2 else 0.5).to(dev) for i in range(k)]
    rng = np.random.default_rng(seed)
    for m in models:                                   # running statistics away from (0, 1)
        _, bn = _rand_model(m.shape, rng, dev)
        m.flat_bn_buffers().copy_(bn)
    return models


def _plain_eval(m, X, y, batch=64):
    """(loss, correct) as the reference loop computes them, from the module's own eval forward."""
    was = m.training
    m.eval()
    with torch.no_grad():
        z = m(X)
    m.train(was)
    _, loss, correct = val_metrics(z.cpu().numpy(), y.cpu().numpy(), batch)
    return loss, correct


def test_evaluate_folds_entry_point():
    """evaluate_folds / FoldBatch.validate: sizes differ, modules stay in train mode, the state is reused
    across calls, rows of a larger buffer are written through the slot, and an in-place parameter
    change is seen without a rebuild."""
    from eegnetreplication_amd import FoldBatch, evaluate_folds, folds as F
    dev = _dev()
    C, T = 22, 257
    models = _modules(3, C, T, dev)
    rng = np.random.default_rng(20)
    sets = [_rand_set(models[0].shape, n, rng, dev) for n in (50, 70, 70)]
    loss, correct = evaluate_folds(models, sets, 64)
    assert loss.dtype == torch.float64 and correct.dtype == torch.int64 and loss.shape == correct.shape == (3,)
    assert all(m.training for m in models)
    for k, (m, (X, y)) in enumerate(zip(models, sets)):
        ref_loss, ref_correct = _plain_eval(m, X, y)
        assert int(correct[k]) == ref_correct
        assert abs(float(loss[k]) - ref_loss) <= loss_tol(ref_loss)
    table = F._eval_states[models[0]]["table"]
    L = torch.full((4, 3), SENTINEL_L, dtype=torch.float64, device=dev)
    Cn = torch.full((4, 3), SENTINEL_C, dtype=torch.int64, device=dev)
    evaluate_folds(models, sets, 64, out=(L[2], Cn[2]))
    table2 = F._eval_states[models[0]]["table"]
    assert table2 is not table                         # other outputs: a new table
    with torch.no_grad():
        models[1].flat_parameters().mul_(1.5)          # as a training step: in place
    evaluate_folds(models, sets, 64, out=(L[0], Cn[0]))
    assert F._eval_states[models[0]]["table"] is table2            # another row of the same buffers: reused
    torch.cuda.synchronize()
    assert torch.equal(L[2], loss) and torch.equal(Cn[2], correct)
    assert torch.all(L[1] == SENTINEL_L) and torch.all(L[3] == SENTINEL_L) and torch.all(Cn[3] == SENTINEL_C)
    assert float(L[0, 0]) == float(loss[0]) and float(L[0, 2]) == float(loss[2])
    ref_loss, ref_correct = _plain_eval(models[1], *sets[1])
    assert int(Cn[0, 1]) == ref_correct and abs(float(L[0, 1]) - ref_loss) <= loss_tol(ref_loss)
    fb = FoldBatch(models, [1, 2, 3])
    l2, c2 = fb.validate(sets)
    assert torch.equal(l2, L[0]) and torch.equal(c2, Cn[0])
    with pytest.raises(ValueError, match="contiguous"):
        evaluate_folds(models, [(X.transpose(1, 2).contiguous().transpose(1, 2), y) for X, y in sets])


def test_graph_capture_sees_in_place_parameter_changes():
    from eegnetreplication_amd import evaluate_folds
    dev = _dev()
    models = _modules(3, 22, 257, dev, seed=6)
    rng = np.random.default_rng(21)
    sets = [_rand_set(models[0].shape, n, rng, dev) for n in (65, 3, 130)]
    evaluate_folds(models, sets)                       # builds the table and the scratch (eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss, correct = evaluate_folds(models, sets)
    with torch.no_grad():
        for m in models:
            m.flat_parameters().add_(0.05 * torch.randn_like(m.flat_parameters()))
            m.flat_bn_buffers().mul_(1.1)
    g.replay()
    torch.cuda.synchronize()
    got = (loss.clone(), correct.clone())
    loss.fill_(SENTINEL_L)
    want = evaluate_folds(models, sets)                # eager, on the changed parameters
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for k, (m, (X, y)) in enumerate(zip(models, sets)):
        ref_loss, ref_correct = _plain_eval(m, X, y)
        assert int(got[1][k]) == ref_correct and abs(float(got[0][k]) - ref_loss) <= loss_tol(ref_loss)


def test_protocol_validation_matches_a_plain_recomputation():
    """train.py's _run_folds validates with evaluate_folds: per fold, the returned val / test metrics
    against a plain recomputation from the saved state -- a fresh EEGNet in .eval(), batches of 64,
    F.cross_entropy and argmax.  Accuracies exactly (bit-equal logits), the loss to the loss tolerance.
    Three epochs at p = 0: the metrics of every epoch are recomputed from a run stopped at that epoch
    (a fold batch is bit-reproducible, so the first e epochs of a longer run are the e-epoch run)."""
    import importlib
    import torch.nn.functional as Fn
    from eegnetreplication_amd import EEGNet
    T_ = importlib.import_module("eegnetreplication_amd.train")
    dev = _dev()
    C, T = 22, 257
    rng = np.random.default_rng(4)
    specs = []
    for u, nv in enumerate((50, 70, 70)):              # two validation-size groups
        X = rng.standard_normal((100 + nv, C, T)).astype(np.float64)
        y = rng.integers(0, 4, 100 + nv).astype(np.int64)
        ids = rng.permutation(100 + nv)
        te = (rng.standard_normal((40, C, T)), rng.integers(0, 4, 40).astype(np.int64))
        specs.append((X, y, ids[:100], ids[100:], te, 0.0, 10 + u))

    def plain(state, Xs, ys):
        m = EEGNet(C, T, p=0.0)
        m.load_state_dict(state)
        m = m.to(dev).eval()
        Xd = torch.as_tensor(np.asarray(Xs), dtype=torch.float32).to(dev)
        yd = torch.as_tensor(np.asarray(ys), dtype=torch.int64).to(dev)
        running, correct, nb = 0.0, 0, 0
        with torch.no_grad():
            for i in range(0, len(yd), 64):
                z = m(Xd[i:i + 64])
                running += Fn.cross_entropy(z.double(), yd[i:i + 64]).item()
                correct += int((z.argmax(1) == yd[i:i + 64]).sum())
                nb += 1
        return running / nb, correct

    runs = [T_._run_units(specs, e, dev, fold_batch=3) for e in (1, 2, 3)]
    for k, (X, y, tr, va, te, _, _) in enumerate(specs):
        per_epoch = [plain(runs[e][k]["state"], X[va], y[va]) for e in range(3)]
        want_loss = min(l for l, _ in per_epoch)
        want_acc = max(100.0 * c / len(va) for _, c in per_epoch)
        _, tcorrect = plain(runs[2][k]["state"], te[0], te[1])
        got = runs[2][k]
        print(f"unit {k}: val_loss {got['val_loss']!r} ref {want_loss!r}; val_acc {got['val_acc']} ref {want_acc}; "
              f"test_acc {got['test_acc']} ref {100 * tcorrect / 40}")
        assert got["val_acc"] == want_acc, k
        assert got["test_acc"] == 100 * tcorrect / 40, k
        assert abs(got["val_loss"] - want_loss) <= loss_tol(want_loss), k
