"""Consecutive train steps that alternate between two batches: the planes of step k are overwritten in
step k + 1 and must be read fresh.

The train passes load their streamed data -- x, the s / v planes of pass A, the block-2 planes of pass B and
dp2 of pass D -- under a cache policy (eegnet_common.h ld_pol, EEGNET_LD_X).  A policy may
change where a line is served from, never its value: every plane a pass reads was written
by an earlier launch of the same step, into the workspace the previous step filled with another batch's
planes.  A load served from a stale copy of the previous step's line would give step k + 1 the planes of
step k; with two different batches in alternation (batch 0, batch 1, batch 0) all three steps differ from
their neighbours in every plane.

Cases: B = 40 at the two compile-time shapes (22 x 256: the LDS-DMA pipelines; 22 x 257: the dword DMAs of
unaligned rows), B = 9 at a runtime shape (5 x 64, K1 = 32: the register-staged loads), one trainer and
one workspace per case; and a fold-indexed case (3 folds, batch 8, 22 x 257, one workspace per fold, the
launches at rows 0, 8, 0 of each fold's epoch).  All through the device dropout path with p = 0, so the
oracle needs no masks.  Each step is compared against oracle/numpy_ref.py (float64) at the tolerances of
tests/test_gpu_multi_trial.py: logits and gradients rtol 1e-4 / atol 1e-5 max|ref| with the
near-zero-gradient rules, the loss to 1e-4, running means to 1e-5 absolute, the parameters by
assert_params_close.  As in tests/test_gpu_fold_oracle.py every step starts from the reference's state
(fp32-rounded), so a step is judged on its own and not on the trajectory's drift."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from golden_util import PARAM_NAMES, assert_close, assert_grads_close, assert_params_close, make_inputs
from hip_cases import flat_to_dict, random_model, state_np

pytestmark = pytest.mark.gpu

CASES = [
    # B, C, T, K1
    (40, 22, 256, 32),
    (40, 22, 257, 32),
    (9, 5, 64, 32),
]
ORDER = (0, 1, 0)               # which of the two batches each step trains on


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _flat32(d, names, dev):
    a = np.concatenate([np.asarray(d[k], dtype=np.float64).reshape(-1) for k in names])
    return torch.from_numpy(a.astype(np.float32)).to(dev)


def _oracle_steps(m, batches):
    """The float64 oracle trajectory over ``batches`` [(x, y), ...]: per step what nr.train_step returns
    plus copies of the Adam moments after it."""
    from oracle import numpy_ref as nr
    params, bufs = state_np(m)
    params = {k: v.astype(np.float64) for k, v in params.items()}
    st = nr.adam_init(params)
    out = []
    for x, y in batches:
        r = nr.train_step(params, bufs, x.astype(np.float64), y, st, p=0.0)
        params, bufs = r["params"], r["buffers"]
        out.append(dict(r, m={k: v.copy() for k, v in st.m.items()}, v={k: v.copy() for k, v in st.v.items()}))
    return out


def _load_state(flat, bn, adam_state, bn_names, prev, dev):
    flat.copy_(_flat32(prev["params"], PARAM_NAMES, dev))
    bn.copy_(_flat32(prev["buffers"], bn_names, dev))
    adam_state.copy_(torch.cat([_flat32(prev["m"], PARAM_NAMES, dev), _flat32(prev["v"], PARAM_NAMES, dev)]))


def _check_buffers(bn, layout, ref_bufs, what):
    o = 0
    for name, n in layout:
        got, want = bn[o:o + n], np.asarray(ref_bufs[name], dtype=np.float64)
        o += n
        if name.endswith("running_mean"):
            assert_close(got, want, atol_abs=1e-5 * max(1.0, float(np.abs(want).max())), name=what + name)
        else:
            assert_close(got, want, name=what + name)


@pytest.mark.parametrize("B,C,T,K1", CASES)
def test_alternating_batches_match_oracle(B, C, T, K1):
    from eegnetreplication_amd import FusedTrainer
    dev = _dev()
    m = random_model(C, T, F1=8, D=2, K1=K1, p=0.0, seed=7 * C + T)
    two = [make_inputs(B, C, T, 4100 + T + i) for i in range(2)]
    assert not np.array_equal(two[0][0], two[1][0])
    ref = _oracle_steps(m, [two[i] for i in ORDER])
    model = m.to(dev).train()
    tr = FusedTrainer(model, lr=1e-3, eps=1e-7)
    flat, bn, nbt = model.flat_views()
    layout = model.shape.bn_layout()
    bn_names = [n for n, _ in layout]
    xs = [torch.from_numpy(x).to(dev) for x, _ in two]
    ys = [torch.from_numpy(y).to(dev) for _, y in two]
    logits = torch.empty((B, 4), device=dev)
    for step, i in enumerate(ORDER):
        if step:
            _load_state(flat, bn, tr.adam.state, bn_names, ref[step - 1], dev)
        loss = tr.step(xs[i], ys[i], logits=logits)
        torch.cuda.synchronize()
        r = ref[step]
        what = f"{C}x{T} B={B} step {step + 1} (batch {i}) "
        assert_close(logits.cpu().numpy(), r["logits"], name=what + "logits")
        assert abs(float(loss) - float(r["loss"])) <= 1e-4 * max(1.0, abs(float(r["loss"]))), what + "loss"
        assert_grads_close(flat_to_dict(model, tr.adam.grads), r["grads"], prefix=what + "grad.")
        _check_buffers(bn.cpu().numpy(), layout, r["buffers"], what)
        assert nbt.tolist() == [step + 1] * 3, what + "num_batches_tracked"
        assert int(tr.adam.step.item()) == step + 1, what + "Adam step"
        assert_params_close(flat_to_dict(model, flat), r["params"], prefix=what + "param.")
    assert len(tr._ws) == 1          # one workspace took all three steps' planes


def test_alternating_fold_launches_match_oracle():
    """3 folds, batch 8, 22 x 257: launches at rows 0, 8 and 0 of each fold's 16-trial epoch, each fold in
    its own workspace, which the next launch overwrites."""
    from eegnetreplication_amd import ops
    from eegnetreplication_amd.model import FusedAdamState
    dev = _dev()
    K, B, C, T, OFFSET = 3, 8, 22, 257, 3
    rows = [B * i for i in ORDER]
    folds = []
    for k in range(K):
        x, y = make_inputs(2 * B, C, T, 4300 + k)
        m = random_model(C, T, F1=8, D=2, K1=32, p=0.0, seed=90 + k)
        folds.append(dict(m=m, x=x, y=y, ref=_oracle_steps(m, [(x[r:r + B], y[r:r + B]) for r in rows])))
    shape = folds[0]["m"].shape
    layout = shape.bn_layout()
    bn_names = [n for n, _ in layout]
    dv = []
    for f in folds:
        m = f["m"].to(dev).train()
        flat, bn, nbt = m.flat_views()
        dv.append(dict(m=m, flat=flat, bn=bn, nbt=nbt, adam=FusedAdamState(m), x=torch.from_numpy(f["x"]).to(dev),
                       y=torch.from_numpy(f["y"]).to(dev),
                       losses=torch.zeros(len(ORDER), dtype=torch.float32, device=dev),
                       ws=ops.new_workspace(shape, B, dev)))
    table = ops.fold_table(
        [dict(params=d["flat"], bn_buffers=d["bn"], num_batches_tracked=d["nbt"], x=d["x"], xstat=None,
              labels=d["y"], perm=None, grads=d["adam"].grads, adam_state=d["adam"].state, step=d["adam"].step,
              losses=d["losses"], ws=d["ws"], seed=11 + k) for k, d in enumerate(dv)], dev)
    for step, row0 in enumerate(rows):
        if step:
            for f, d in zip(folds, dv):
                _load_state(d["flat"], d["bn"], d["adam"].state, bn_names, f["ref"][step - 1], dev)
        ops.train_step_folds(shape, B, table, K, row0=row0, slot=step, offset=OFFSET)
        torch.cuda.synchronize()
        for k, (f, d) in enumerate(zip(folds, dv)):
            r = f["ref"][step]
            what = f"fold {k} launch {step + 1} (row0 {row0}) "
            loss = float(d["losses"][step])
            assert abs(loss - float(r["loss"])) <= 1e-4 * max(1.0, abs(float(r["loss"]))), what + "loss"
            assert_grads_close(flat_to_dict(d["m"], d["adam"].grads), r["grads"], prefix=what + "grad.")
            _check_buffers(d["bn"].cpu().numpy(), layout, r["buffers"], what)
            assert d["nbt"].tolist() == [step + 1] * 3, what + "num_batches_tracked"
            assert_params_close(flat_to_dict(d["m"], d["flat"]), r["params"], prefix=what + "param.")
