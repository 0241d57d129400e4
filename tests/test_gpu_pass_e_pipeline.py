"""Pass E's look-ahead pipelines (k_pass_e at the compile-time EEGNet-8,2 shapes, K1 = 32) at the ends of a
workgroup's trial range.

The 22 x 256 kernel (eegnet_stream.hip pass_e_body, the PIPE loop) computes dy2 of trial b + 1 while the
dws GEMM of trial b runs, and stages dp2 and v two trials ahead.  What can go wrong sits at the range
ends: a range of one trial (prologue and last trial are the same trial, nothing is looked ahead), of two
(the look-ahead of the first trial is the last), of three (the first range with a trial that issues the
loads of trial b + 2), an empty range beside them never (B >= the grid).  The cases therefore are, with
G = the number of trial ranges pass E splits a large batch into (ops.launch_grids, so the CU count is
the library's answer, not this file's):

    B = 1              one workgroup, one trial
    B = G              every workgroup exactly one trial
    B = G + G // 2     ranges of 1 and 2 trials in one launch
    B = 2 G + G // 2   ranges of 2 and 3 trials in one launch

The 22 x 257 kernel (the DMA loop) has a trial loop of its own: s, dp2 and v go one trial ahead and
nothing further, so ranges of one and of two trials are the range ends that exist there.  Its cases are
t257_one_trial (B = 1) and t257_ranges_1_2 (B = G + G // 2, G from launch_grids at that shape).

Each case asserts its premise from launch_grids at that B (ranges of two and three trials need B > 2 G:
1280 trials, 29 MB of x, on a 256-CU device -- the oracle step of that case is what takes its 6 s, once;
the other cases take 0.4 to 4 s and every test that reuses a case's reference takes milliseconds).
Per case ONE float64 oracle step
(oracle/numpy_ref.train_step with the masks the device draws for (seed, offset)) is computed and shared:
the fused step (FusedTrainer: on-device masks, CE, backward, clamps, Adam) and the module path (model(x),
CE, backward through forward_train + backward, the same masks injected) are both compared with it --
loss, logits, all 12 gradients, the running statistics and counters, the post-Adam parameters -- at the
tolerances of tests/test_gpu_multi_trial.py (rtol 1e-4, atol 1e-5 max|ref|, the near-zero gradient rule,
loss within 1e-4 max(1, |ref|)).  The fused step run twice from the same state must agree bit for bit.

The fold launch (eegnet_train_step_folds: the same body through FOLD with a permutation) runs three folds
over batches of 64, 64 and 22 at 22 x 256 and is compared launch by launch as tests/test_gpu_fold_oracle.py
compares its cases (that file's _run, here with p = 0.5)."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from golden_util import assert_close, assert_grads_close, assert_params_close, make_inputs
from hip_cases import device_masks, flat_to_dict, grads_of, random_model, state_np

pytestmark = pytest.mark.gpu

C, T, F1, D, K1, P = 22, 256, 8, 2, 32, 0.5
SEED, OFFSET = 0x0E5E_ED01, 3
# case -> (T, the trial counts of its ranges)
CASES = {"one_trial": (256, "one_trial"), "one_each": (256, "one_each"), "ranges_1_2": (256, "ranges_1_2"),
         "ranges_2_3": (256, "ranges_2_3"),
         "t257_one_trial": (257, "one_trial"), "t257_ranges_1_2": (257, "ranges_1_2")}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _model(t):
    return random_model(C, t, F1=F1, D=D, K1=K1, p=P, seed=41)


def _batch(case):
    """B of the case and the trial counts its pass-E ranges hold, asserted from the library's grids."""
    from eegnetreplication_amd import ops
    t, kind = CASES[case]
    shape = _model(t).shape
    G = ops.launch_grids(shape, 1 << 16)["E"]
    assert G >= 2
    B = {"one_trial": 1, "one_each": G, "ranges_1_2": G + G // 2, "ranges_2_3": 2 * G + G // 2}[kind]
    n = ops.launch_grids(shape, B)["E"]
    sizes = {(w + 1) * B // n - w * B // n for w in range(n)}       # eegnet_common.h trial_range
    assert sizes == {"one_trial": {1}, "one_each": {1}, "ranges_1_2": {1, 2}, "ranges_2_3": {2, 3}}[kind], (B, n, sizes)
    assert n == (1 if kind == "one_trial" else G)
    return B


_CASE = {}


def _case(case):
    """Inputs and the float64 oracle step of a case, computed once and shared by its tests (read-only)."""
    if case not in _CASE:
        from oracle import numpy_ref as nr
        B, t = _batch(case), CASES[case][0]
        x_np, y_np = make_inputs(B, C, t, 7700 + B)
        masks = device_masks(B, F1 * D, t, SEED, OFFSET, P)
        params, bufs = state_np(_model(t))
        params = {k: v.astype(np.float64) for k, v in params.items()}
        ref = nr.train_step(params, bufs, x_np, y_np, nr.adam_init(params), p=P, masks=masks)
        for a in (x_np, y_np, *masks):
            a.setflags(write=False)
        _CASE[case] = dict(B=B, T=t, x=x_np, y=y_np, masks=masks, ref=ref)
    return _CASE[case]


def _check_buffers(m, ref_nb, what):
    bufs = {k: b.detach().cpu().numpy() for k, b in m.named_buffers()}
    for k, v in ref_nb.items():
        if "running_mean" in k:
            assert_close(bufs[k], v, atol_abs=1e-5 * max(1.0, float(np.abs(v).max())), name=f"{what} {k}")
        elif "running_var" in k:
            assert_close(bufs[k], v, name=f"{what} {k}")
        else:
            assert int(bufs[k]) == int(v), f"{what} {k}"


def _fused_step(c, dev):
    """One FusedTrainer step from the case's initial state: every output, on the host."""
    from eegnetreplication_amd import FusedTrainer
    model = _model(c["T"]).to(dev).train()
    model.next_dropout_key = lambda: (SEED, OFFSET)
    tr = FusedTrainer(model, lr=1e-3, eps=1e-7)
    logits = torch.empty((c["B"], 4), device=dev)
    loss = tr.step(torch.from_numpy(c["x"]).to(dev), torch.from_numpy(c["y"]).to(dev), logits=logits)
    torch.cuda.synchronize()
    return dict(model=model, logits=logits.cpu().numpy(), loss=float(loss),
                grads=flat_to_dict(model, tr.adam.grads),
                params={k: q.detach().cpu().numpy() for k, q in model.named_parameters()},
                buffers={k: b.detach().cpu().numpy() for k, b in model.named_buffers()})


@pytest.mark.parametrize("case", CASES)
def test_fused_step_matches_oracle(case):
    dev = _dev()
    c = _case(case)
    ref, what = c["ref"], f"fused 22x{c['T']} {case} B={c['B']}"
    out = _fused_step(c, dev)
    assert_close(out["logits"], ref["logits"], name=f"{what} logits")
    assert abs(out["loss"] - float(ref["loss"])) <= 1e-4 * max(1.0, abs(float(ref["loss"]))), what
    assert_grads_close(out["grads"], ref["grads"], prefix=f"{what} grad.")
    _check_buffers(out["model"], ref["buffers"], what)
    assert_params_close(out["params"], ref["params"], prefix=f"{what} step1.")


@pytest.mark.parametrize("case", CASES)
def test_module_step_matches_oracle(case):
    dev = _dev()
    c = _case(case)
    ref, what = c["ref"], f"module 22x{c['T']} {case} B={c['B']}"
    m = _model(c["T"]).to(dev).train()
    m.set_dropout_masks(torch.from_numpy(c["masks"][0]).to(dev), torch.from_numpy(c["masks"][1]).to(dev))
    y = torch.from_numpy(c["y"]).to(dev)
    logits = m(torch.from_numpy(c["x"]).to(dev))
    loss = torch.nn.functional.cross_entropy(logits, y)
    loss.backward()
    assert_close(logits.detach().cpu().numpy(), ref["logits"], name=f"{what} logits")
    assert abs(float(loss) - float(ref["loss"])) <= 1e-4 * max(1.0, abs(float(ref["loss"]))), what
    assert_grads_close(grads_of(m), ref["grads"], prefix=f"{what} grad.")
    _check_buffers(m, ref["buffers"], what)
    # the post-Adam parameters of this path: torch.optim.Adam on the kernels' gradients
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, eps=1e-7)
    opt.step()
    assert_params_close({k: q.detach().cpu().numpy() for k, q in m.named_parameters()}, ref["params"],
                        prefix=f"{what} step1.")


@pytest.mark.parametrize("case", CASES)
def test_fused_step_is_deterministic(case):
    dev = _dev()
    c = _case(case)
    a, b = _fused_step(c, dev), _fused_step(c, dev)
    assert a["loss"] == b["loss"]
    assert np.array_equal(a["logits"], b["logits"])
    for group in ("grads", "params", "buffers"):
        for k in a[group]:
            assert np.array_equal(a[group][k], b[group][k]), f"{case} {group} {k} differs between two runs"


def test_fold_launches_match_oracle():
    from test_gpu_fold_oracle import _run
    _run(C, T, F1, D, K1, P, xstat=False, tag="pass E pipeline ")
