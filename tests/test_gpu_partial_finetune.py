"""GPU tests of partial fine-tuning on a single model (eegnet_frozen_step_from behind
``ops.frozen_step(train_from=...)``, ``EEGNet.train_from``): the suffix gradients against the float64 oracle
with the frozen prefix of ``grads`` left untouched; bit identity of the suffix, the loss and the logits
with the full step; independence of the workspace content; the fused Adam on the suffix; graph capture;
the module-level paths (autograd, train() with either optimizer form, the refusal of other patterns).

Shapes from test_gpu_input_grad.SHAPES, p = 0.5 with injected masks.  Tolerance: that of
frozen_cases.assert_frozen_grads_close (rtol 1e-4, atol 1e-5 * max|ref|, the clamped classifier weight at
its unclamped scale) on the suffix; Adam as test_gpu_frozen (rtol 1e-5, atol 1e-5 * max|ref|)."""

from __future__ import annotations

import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from frozen_cases import FrozenRefEEGNet, model_state, oracle_frozen
from golden_util import CLAMPED_GRADS, PARAM_NAMES, assert_close, make_inputs, make_masks
from hip_cases import device_masks, flat_to_dict, random_model
from test_gpu_input_grad import SHAPES

pytestmark = pytest.mark.gpu

STAGES = ("temporal", "aggregation", "block_2", "classifier")
FIRST = {"aggregation": "aggregation.0.weight", "block_2": "block_2.0.weight", "classifier": "classifier.weight"}
CUT = ("aggregation", "block_2", "classifier")
CASES = [(22, 256, 3, 8, 2, 32),       # the compile-time shape
         (22, 257, 5, 8, 2, 32),       # pitched rows, pool truncation
         (22, 257, 2, 8, 2, 64),       # K1 = 64
         (5, 96, 3, 4, 1, 32)]         # the run-time shape, F2 = 4
assert all(c in SHAPES for c in CASES)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _cus():
    return torch.cuda.get_device_properties(_dev()).multi_processor_count


def _t(a, dt, dev):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)


@functools.lru_cache(maxsize=None)
def _case(C, T, B, F1=8, D=2, K1=32, seed=0):
    """(model on the CPU, oracle state, x, y, masks) -- numpy inputs; shared, never modified."""
    m = random_model(C, T, F1=F1, D=D, K1=K1, p=0.5, seed=3 * C + T + F1 + K1 + seed)
    x, y = make_inputs(B, C, T, 1700 + T + C + seed)
    return m, model_state(m), x, y, make_masks(B, F1 * D, T, 900 + seed, 0.5)


@functools.lru_cache(maxsize=None)
def _ref(*case):
    """The float64 oracle of a case, computed once."""
    m, state, x, y, masks = _case(*case)
    return oracle_frozen(state, x, 0.5, masks, labels=y)


def _on_device(m):
    return copy.deepcopy(m).to(_dev()).train()


def _suffix(names, stage):
    return names[names.index(FIRST[stage]):]


def _step(md, x, stage, *, labels=None, dlogits=None, masks=None, seed=11, offset=5, ws=None, grads=None,
          key_from_step=False, step=None, adam_state=None):
    """ops.frozen_step(train_from=stage) on the device model ``md``: (flat grads, loss, logits)."""
    from eegnetreplication_amd import ops
    dev = _dev()
    B = x.shape[0]
    xd = x if isinstance(x, torch.Tensor) else _t(x, torch.float32, dev)
    flat = md.flat_parameters()
    if grads is None:
        grads = torch.full_like(flat, float("nan"))
    loss = torch.full((1,), float("nan"), device=dev)
    logits = torch.full((B, 4), float("nan"), device=dev)
    mk = None if masks is None else (_t(masks[0], torch.uint8, dev), _t(masks[1], torch.uint8, dev))
    ops.frozen_step(md.shape, flat, md.flat_bn_buffers(), xd, seed, offset, grads,
                    ops.new_frozen_workspace(md.shape, B, dev) if ws is None else ws,
                    dlogits=_t(dlogits, torch.float32, dev), labels=_t(labels, torch.int64, dev), masks=mk, loss=loss,
                    logits=logits, key_from_step=key_from_step, step_i32=step, adam_state=adam_state,
                    train_from=stage)
    torch.cuda.synchronize()
    return grads, loss, logits


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. parity of the suffix, the prefix untouched ----
@pytest.mark.parametrize("stage", CUT)
@pytest.mark.parametrize("C,T,B,F1,D,K1", CASES)
def test_suffix_gradients_match_the_float64_oracle(C, T, B, F1, D, K1, stage):
    from eegnetreplication_amd import ops
    m, state, x, y, masks = _case(C, T, B, F1, D, K1)
    ref = _ref(C, T, B, F1, D, K1)
    md = _on_device(m)
    off = ops.trainable_offset(md.shape, stage)
    fill = torch.full_like(md.flat_parameters(), float("nan"))
    grads, loss, logits = _step(md, x, stage, labels=y, masks=masks)
    what = f"{stage} EEGNet-{F1},{D} K1={K1} {C}x{T} B={B}"
    assert 0 < off < grads.numel()
    assert torch.equal(_bits(grads[:off]), _bits(fill[:off])), f"{what}: the frozen prefix of grads was written"
    assert bool(torch.isfinite(grads[off:]).all())
    assert_close(logits.cpu().numpy(), ref["logits"], name=f"{what} logits")
    assert_close(loss.cpu().numpy()[0], ref["loss"], name=f"{what} loss")
    got = flat_to_dict(md, grads)
    for k in _suffix(list(PARAM_NAMES), stage):
        if k in CLAMPED_GRADS:        # judged at its unclamped scale, as assert_frozen_grads_close does
            scale = max(float(np.max(np.abs(ref["raw"][k]))), float(np.max(np.abs(ref["grads"][k]))))
            assert_close(got[k], ref["grads"][k], rtol=1e-4, atol_abs=1e-5 * scale, name=f"{what} grad {k}")
        else:
            assert_close(got[k], ref["grads"][k], rtol=1e-4, atol_frac=1e-5, name=f"{what} grad {k}")


# ---- 2. bit identity with the full step ----
def _assert_same_suffix(md, x, stage, **kw):
    from eegnetreplication_amd import ops
    off = ops.trainable_offset(md.shape, stage)
    full = _step(md, x, 0, **kw)
    cut = _step(md, x, stage, **kw)
    assert torch.equal(_bits(cut[0][off:]), _bits(full[0][off:])), f"{stage}: suffix of grads"
    assert torch.equal(_bits(cut[1]), _bits(full[1])), f"{stage}: loss"
    assert torch.equal(_bits(cut[2]), _bits(full[2])), f"{stage}: logits"
    assert bool(torch.isnan(cut[0][:off]).all()) and bool(torch.isfinite(full[0]).all())


@pytest.mark.parametrize("stage", CUT)
@pytest.mark.parametrize("C,T,B,F1,D,K1", CASES)
def test_cut_step_is_bit_identical_to_the_full_step(C, T, B, F1, D, K1, stage):
    m, state, x, y, masks = _case(C, T, B, F1, D, K1)
    _assert_same_suffix(_on_device(m), x, stage, labels=y, masks=masks)


@pytest.mark.parametrize("stage", CUT)
def test_bit_identity_with_a_second_trial_per_workgroup(stage):
    """22 x 257 at B = CUs + 3: three workgroups take a second trial, so the read-modify-write of the
    partial row's correlation columns runs (device-generated masks)."""
    B = _cus() + 3
    m, state, x, y, _ = _case(22, 257, B, seed=1)
    _assert_same_suffix(_on_device(m), x, stage, labels=y, seed=5, offset=9)


def test_stage_names_and_indices_are_the_same_call():
    m, state, x, y, masks = _case(22, 257, 5)
    md = _on_device(m)
    for i, stage in enumerate(STAGES):
        a, b = _step(md, x, stage, labels=y, masks=masks), _step(md, x, i, labels=y, masks=masks)
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


# ---- 3. the workspace content does not matter ----
@pytest.mark.parametrize("stage", CUT)
@pytest.mark.parametrize("C,T,B,F1,D,K1", [CASES[1], CASES[3]])
def test_workspace_content_does_not_matter(C, T, B, F1, D, K1, stage):
    """0xFF bytes (NaN in every column) against zeros: a reduction that read a column of a frozen parameter,
    which the cut kernel never writes, would differ."""
    from eegnetreplication_amd import ops
    m, state, x, y, masks = _case(C, T, B, F1, D, K1)
    md = _on_device(m)
    out = []
    for byte in (0xFF, 0x00):
        ws = ops.new_frozen_workspace(md.shape, B, _dev()).fill_(byte)
        out.append(_step(md, x, stage, labels=y, masks=masks, ws=ws))
    off = ops.trainable_offset(md.shape, stage)
    assert bool(torch.isfinite(out[0][0][off:]).all())
    for a, b in zip(*out):
        assert torch.equal(_bits(a), _bits(b))


# ---- 4. the fused Adam on the suffix ----
def _oracle_adam_suffix(state, stage, batches):
    """float64 oracle fine-tuning with the prefix frozen: torch.optim.Adam(lr=1e-3, eps=1e-7) over the
    suffix parameters alone."""
    ref = FrozenRefEEGNet(state, p=0.5)
    names = _suffix(list(PARAM_NAMES), stage)
    opt = torch.optim.Adam([ref.params[k] for k in names], lr=1e-3, eps=1e-7)
    for x, y, masks in batches:
        loss = F.cross_entropy(ref(torch.as_tensor(x, dtype=torch.float64), masks), torch.as_tensor(y))
        for q in ref.parameters():
            q.grad = None
        loss.backward()
        opt.step()
    return {k: ref.params[k].detach().numpy() for k in PARAM_NAMES}


@pytest.mark.parametrize("stage", CUT)
def test_three_fused_adam_steps_on_the_suffix(stage):
    from eegnetreplication_amd import ops
    dev = _dev()
    C, T, B, seed, offset, sentinel = 22, 257, 4, 77, 3, -123.456
    m, state, x, y, _ = _case(C, T, B, seed=2)
    md = _on_device(m)
    flat = md.flat_parameters()
    n, off = flat.numel(), ops.trainable_offset(md.shape, stage)
    before = flat.clone()
    adam = torch.zeros(2 * n, device=dev)
    adam[:off] = sentinel
    adam[n:n + off] = sentinel
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    for _ in range(3):
        _step(md, x, stage, labels=y, seed=seed, offset=offset, key_from_step=True, step=step, adam_state=adam)
    assert int(step.item()) == 3
    assert torch.equal(_bits(flat[:off]), _bits(before[:off])), "frozen parameters were written"
    want = torch.full((off,), sentinel, device=dev)
    assert torch.equal(_bits(adam[:off]), _bits(want)) and torch.equal(_bits(adam[n:n + off]), _bits(want))
    assert not torch.equal(flat[off:], before[off:])
    batches = [(x, y, device_masks(B, 16, T, seed, offset + i, 0.5)) for i in range(3)]
    ref = _oracle_adam_suffix(state, stage, batches)
    got = {k: v.detach().cpu().numpy() for k, v in md.named_parameters()}
    for k in PARAM_NAMES:
        assert_close(got[k], ref[k], rtol=1e-5, atol_frac=1e-5, name=f"{stage} Adam x3 {k}")


# ---- 5. graph capture ----
@pytest.mark.parametrize("stage", CUT)
def test_cut_step_is_capturable_and_replays_draw_fresh_masks(stage):
    """The cut step with Adam and EEGNET_KEY_FROM_STEP captured once on one stream: two replays after one
    eager step leave the bits of three eager steps, so every replay keyed its masks by the device step."""
    from eegnetreplication_amd import ops
    dev = _dev()
    m, state, x, y, _ = _case(22, 257, 4, seed=2)
    xd, yd = _t(x, torch.float32, dev), _t(y, torch.int64, dev)
    out = []
    for graph in (False, True):
        md = _on_device(m)
        flat, bnf = md.flat_parameters(), md.flat_bn_buffers()
        n = flat.numel()
        grads, adam = torch.zeros(n, device=dev), torch.zeros(2 * n, device=dev)
        step, loss = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, device=dev)
        ws = ops.new_frozen_workspace(md.shape, 4, dev)
        losses = []

        def run():
            ops.frozen_step(md.shape, flat, bnf, xd, 9, 1, grads, ws, labels=yd, adam_state=adam, step_i32=step,
                            loss=loss, key_from_step=True, train_from=stage)
        run()
        if graph:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run()
            for _ in range(2):
                g.replay()
                losses.append(loss.clone())
        else:
            for _ in range(2):
                run()
                losses.append(loss.clone())
        torch.cuda.synchronize()
        out.append((flat.clone(), adam.clone(), grads.clone(), torch.cat(losses), int(step.item())))
    assert out[0][4] == out[1][4] == 3
    for a, b in zip(out[0][:4], out[1][:4]):
        assert torch.equal(_bits(a), _bits(b))


# ---- 6. module level ----
def _frozen_module(stage, seed, B=4):
    dev = _dev()
    m, state, x, y, masks = _case(22, 257, B, seed=seed)
    md = _on_device(m).freeze_bn().train_from(stage).train()
    md.set_dropout_masks(_t(masks[0], torch.uint8, dev), _t(masks[1], torch.uint8, dev))
    return md, state, x, y, masks, _t(x, torch.float32, dev), _t(y, torch.int64, dev)


@pytest.mark.parametrize("stage", CUT)
def test_autograd_leaves_frozen_grads_none(stage):
    md, state, x, y, masks, xd, yd = _frozen_module(stage, 3)
    logits = md(xd)
    logits.retain_grad()
    F.cross_entropy(logits, yd).backward()
    names = [k for k, _ in md.named_parameters()]
    suffix = _suffix(names, stage)
    want, _, _ = _step(md, x, stage, dlogits=logits.grad.cpu().numpy(), masks=masks)
    want = flat_to_dict(md, want)
    for k, p in md.named_parameters():
        if k in suffix:
            assert np.array_equal(p.grad.cpu().numpy().view(np.int32), want[k].view(np.int32)), k
        else:
            assert p.grad is None, k


def _train_once(stage, form):
    from eegnetreplication_amd.model import train
    dev = _dev()
    B, NB = 8, 3
    m, state, x, y, _ = _case(22, 257, B * NB, seed=4)
    md = _on_device(m).freeze_bn().train_from(stage)
    before = md.flat_parameters().clone()
    bn0, nbt0 = md.flat_bn_buffers().clone(), md.flat_num_batches_tracked().clone()
    loader = [(torch.from_numpy(x[i * B:(i + 1) * B]), torch.from_numpy(y[i * B:(i + 1) * B])) for i in range(NB)]
    ps = md.parameters() if form == "all" else filter(lambda p: p.requires_grad, md.parameters())
    opt = torch.optim.Adam(ps, lr=1e-3, eps=1e-7)
    torch.manual_seed(1234)                     # the dropout keys of the epoch
    train(md, opt, torch.nn.CrossEntropyLoss(), loader, loader[:1], nepochs=1)
    torch.cuda.synchronize()
    assert torch.equal(md.flat_bn_buffers(), bn0) and torch.equal(md.flat_num_batches_tracked(), nbt0)
    return md, opt, before


@pytest.mark.parametrize("stage", CUT)
def test_train_updates_the_suffix_alone_with_either_optimizer_form(stage):
    from eegnetreplication_amd import ops
    runs = [_train_once(stage, form) for form in ("all", "suffix")]
    off = ops.trainable_offset(runs[0][0].shape, stage)
    for md, opt, before in runs:
        flat = md.flat_parameters()
        assert torch.equal(_bits(flat[:off]), _bits(before[:off])), "frozen parameters moved"
        names = [k for k, _ in md.named_parameters()]
        suffix = _suffix(names, stage)
        o = 0
        for k, p in md.named_parameters():
            if k in suffix:
                assert int(opt.state[p]["step"]) == 3 and float(opt.state[p]["exp_avg_sq"].abs().max()) > 0, k
                assert not torch.equal(p.detach().reshape(-1), before[o:o + p.numel()]), f"{k} did not train"
            else:
                assert p not in opt.state and p.grad is None, k
            o += p.numel()
    assert torch.equal(_bits(runs[0][0].flat_parameters()), _bits(runs[1][0].flat_parameters()))
    for (ka, pa), (kb, pb) in zip(runs[0][0].named_parameters(), runs[1][0].named_parameters()):
        if pa in runs[0][1].state:
            for f in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(runs[0][1].state[pa][f], runs[1][1].state[pb][f]), (ka, f)


# ---- 7. refusals ----
def test_unsupported_pattern_raises_before_any_update():
    from eegnetreplication_amd.model import FusedTrainer, train
    md, state, x, y, masks, xd, yd = _frozen_module("block_2", 5)
    dict(md.named_parameters())["block_2.2.weight"].requires_grad_(False)       # a hole in the suffix
    before = md.flat_parameters().clone()
    loader = [(torch.from_numpy(x), torch.from_numpy(y))]
    with pytest.raises(NotImplementedError, match=r"block_2\.2\.weight.*temporal, aggregation, block_2, classifier"):
        md(xd)
    with pytest.raises(NotImplementedError, match=r"block_2\.2\.weight"):
        FusedTrainer(md).step(xd, yd)
    for ps in (list(md.parameters()), [p for p in md.parameters() if p.requires_grad]):
        with pytest.raises(NotImplementedError, match=r"block_2\.2\.weight"):
            train(md, torch.optim.Adam(ps, lr=1e-3), torch.nn.CrossEntropyLoss(), loader, loader, nepochs=1)
    torch.cuda.synchronize()
    assert torch.equal(_bits(md.flat_parameters()), _bits(before))
    assert all(p.grad is None for p in md.parameters())
