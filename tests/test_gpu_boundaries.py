"""GPU tests of the A -> B pass boundary's finalize (eegnet_finalize.hip fin1_body) at shapes the other
files do not reach: both temporal kernel lengths, T = K1 = 64 (every sample an edge sample of some
window), one and three electrodes, B = 1 and 3, a five-sigma input offset, and the temporal taps
changed in place and by load_state_dict between steps.  Oracle: oracle/numpy_ref.py (float64).
Tolerance: rtol 1e-4, atol 1e-5 * max|ref| with the refinements of DESIGN 7 (tests/golden_util.py);
the two this file adds -- the spatial weight of a one-electrode model, BN2's running statistics after
the first step of a trajectory -- are refinements 1a and 1b there."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from golden_util import assert_close, make_inputs
from hip_cases import device_masks, random_model

pytestmark = pytest.mark.gpu

SEED = 0x51DE_5EED


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------
# The A -> B boundary's finalize (eegnet_finalize.hip fin1_body): BN1 moments from the lag-Gram of the
# padded rows, G w1 / S1 (the temporal weight gradient's inputs) for pass E's finalize -- at both
# kernel lengths, at T = K1 = 64 (every sample an edge sample of some window), one and three
# electrodes, B = 1 and 3.  One fused step against oracle/numpy_ref.py: logits, loss, all 12
# gradients, the parameters after Adam and the running statistics (running means on the absolute
# scale of DESIGN 7, refinement 3).  These cases fix what a shorter fin1 has to keep.
# ---------------------------------------------------------------------------------------------
FIN1_SHAPES = [
    # K1, C, T, F1, D
    (32, 22, 256, 8, 2),
    (32, 22, 257, 8, 2),
    (64, 22, 256, 8, 2),
    (32, 1, 64, 4, 1),
    (64, 3, 64, 8, 2),
]


def _np_state(m):
    params = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.named_parameters()}
    bufs = {k: v.detach().cpu().numpy() for k, v in m.named_buffers()}
    return params, bufs


def _worst(actual, expected):
    """max |a - e| / (1e-5 max|e| + 1e-4 |e|): the error as a fraction of the default tolerance."""
    a, e = np.asarray(actual, np.float64), np.asarray(expected, np.float64)
    return float(np.max(np.abs(a - e) / (1e-5 * max(float(np.max(np.abs(e))), 1e-30) + 1e-4 * np.abs(e))))


def _check_full_step(model, tr, loss, logits, ref, what, steps=1, skip_bufs=()):
    from golden_util import assert_grads_close, assert_params_close
    bn1 = {k: b.detach().cpu().numpy() for k, b in model.named_buffers() if k.startswith("temporal.1.running")}
    o = 0
    for k, prm in model.named_parameters():
        if k == "temporal.0.weight":
            gw1 = tr.adam.grads[o:o + prm.numel()].view(prm.shape).cpu().numpy()
        o += prm.numel()
    print(f"{what}: error / tolerance: dW1 {_worst(gw1, ref['grads']['temporal.0.weight']):.3f}, "
          f"BN1 running var {_worst(bn1['temporal.1.running_var'], ref['buffers']['temporal.1.running_var']):.3f}, "
          f"logits {_worst(logits.cpu().numpy(), ref['logits']):.3f}")
    assert_close(logits.cpu().numpy(), ref["logits"], name=f"{what} logits")
    assert abs(float(loss) - float(ref["loss"])) <= 1e-4 * max(1.0, abs(float(ref["loss"]))), what
    gr, n = {}, 0
    for k, prm in model.named_parameters():
        gr[k] = tr.adam.grads[n:n + prm.numel()].view(prm.shape).cpu().numpy()
        n += prm.numel()
    if model.shape.C == 1:
        # One electrode: the spatial "filter" is one scalar per output row, y2_o = ws_o * y1, and BN2
        # renormalises y2_o, so the loss does not see ws_o's scale: its gradient is O(bn_eps / var2), the
        # residue of two cancelling terms, exactly like gamma1's (refinement 1a).  It is judged
        # like the other structurally-zero gradients, on the model-wide gradient scale.
        gmax = max(float(np.max(np.abs(np.asarray(v)))) for v in ref["grads"].values())
        assert_close(gr["spatial.weight"], ref["grads"]["spatial.weight"], atol_abs=1e-5 * gmax,
                     name=f"{what} grad.spatial.weight")
        gr = dict(gr, **{"spatial.weight": np.asarray(ref["grads"]["spatial.weight"])})
    assert_grads_close(gr, ref["grads"], prefix=f"{what} grad.")
    pr = {k: prm.detach().cpu().numpy() for k, prm in model.named_parameters()}
    if model.shape.C == 1:            # ... and, as for gamma1 / beta1, Adam turns that residue into a move of up to lr
        assert_close(pr["spatial.weight"], ref["params"]["spatial.weight"], rtol=0.0, atol_abs=2.0 * 1e-3 * steps,
                     name=f"{what} params.spatial.weight")
        pr["spatial.weight"] = np.asarray(ref["params"]["spatial.weight"])
    assert_params_close(pr, ref["params"], steps=steps, prefix=f"{what} params.")
    bufs = {k: b.detach().cpu().numpy() for k, b in model.named_buffers()}
    for k, v in ref["buffers"].items():
        if k.startswith(tuple(skip_bufs)):
            continue
        if "running_mean" in k:
            assert_close(bufs[k], v, atol_abs=1e-5 * max(1.0, float(np.abs(v).max())), name=f"{what} {k}")
        elif "running_var" in k:
            assert_close(bufs[k], v, name=f"{what} {k}")
        else:
            assert int(bufs[k]) == int(v), f"{what} {k}"


def _fused_one_step(K1, Cc, Tt, F1, D, B, offset_x=0.0):
    from eegnetreplication_amd import FusedTrainer
    from oracle import numpy_ref as nr
    dev = _dev()
    p = 0.25
    m = random_model(Cc, Tt, F1=F1, D=D, K1=K1, p=p, seed=3 * K1 + Cc + Tt)
    x_np, y_np = make_inputs(B, Cc, Tt, 300 + Tt + B)
    x_np = np.ascontiguousarray(x_np + offset_x, dtype=np.float32)
    params, bufs = _np_state(m)
    seed, offset = SEED, 9
    masks = device_masks(B, F1 * D, Tt, seed, offset, p)
    ref = nr.train_step(params, bufs, x_np, y_np, nr.adam_init(params), p=p, masks=masks)
    model = m.to(dev).train()
    model.next_dropout_key = lambda: (seed, offset)
    tr = FusedTrainer(model, lr=1e-3, eps=1e-7)
    logits = torch.empty((B, 4), device=dev)
    loss = tr.step(torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev), logits=logits)
    torch.cuda.synchronize()
    _check_full_step(model, tr, loss, logits, ref, f"fin1 K1={K1} {Cc}x{Tt} EEGNet-{F1},{D} B={B} +{offset_x}")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K1,Cc,Tt,F1,D", FIN1_SHAPES)
def test_fin1_step_matches_oracle(K1, Cc, Tt, F1, D, B):
    _fused_one_step(K1, Cc, Tt, F1, D, B)


def test_fin1_step_with_input_offset():
    """x = 5 + N(0, 1): E[u^2] - mu^2 cancels five sigma's worth of mean."""
    _fused_one_step(32, 22, 256, 8, 2, 3, offset_x=5.0)


def test_fin1_follows_the_parameters_in_force():
    """Three fused steps against the oracle trajectory; the temporal taps are overwritten in place
    between steps 1 and 2 and load_state_dict is called between steps 2 and 3, so anything derived from
    the taps and kept from an earlier step would be stale.  From step 2 on BN2's running statistics are
    left out: they see gamma1 / beta1, whose Adam moves are +-lr noise in the oracle itself (DESIGN 7,
    refinement 1b); BN1's, which come straight from the taps, are compared at every step."""
    from eegnetreplication_amd import FusedTrainer
    from oracle import numpy_ref as nr
    dev = _dev()
    K1, Cc, Tt, F1, D, B, p = 32, 22, 256, 8, 2, 3, 0.25
    m = random_model(Cc, Tt, F1=F1, D=D, K1=K1, p=p, seed=41)
    params, bufs = _np_state(m)
    st = nr.adam_init(params)
    model = m.to(dev).train()
    steps = iter(range(1 << 20))
    model.next_dropout_key = lambda: (SEED, next(steps))
    tr = FusedTrainer(model, lr=1e-3, eps=1e-7)
    rng = np.random.default_rng(5)
    for s in range(3):
        if s > 0:
            taps = (rng.standard_normal((F1, 1, 1, K1)) * 0.2).astype(np.float32)
            if s == 1:                # in place, through the module's parameter
                with torch.no_grad():
                    model.get_parameter("temporal.0.weight").copy_(torch.from_numpy(taps))
            else:
                sd = {k: v.clone() for k, v in model.state_dict().items()}
                sd["temporal.0.weight"] = torch.from_numpy(taps)
                model.load_state_dict(sd)
            params = dict(params)
            params["temporal.0.weight"] = taps.astype(np.float64)
        x_np, y_np = make_inputs(B, Cc, Tt, 800 + s)
        masks = device_masks(B, F1 * D, Tt, SEED, s, p)
        ref = nr.train_step(params, bufs, x_np, y_np, st, p=p, masks=masks)
        logits = torch.empty((B, 4), device=dev)
        loss = tr.step(torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev), logits=logits)
        torch.cuda.synchronize()
        _check_full_step(model, tr, loss, logits, ref, f"changed-taps step {s + 1}", steps=s + 1,
                         skip_bufs=("aggregation.0.running",) if s > 0 else ())
        params, bufs = ref["params"], ref["buffers"]
