"""Fine-tuning on cue epochs read in place (eegnet_frozen_step_windows: k_frozen with the windowed loader)
on the GPU.

The kernel is k_frozen with another loader, and nothing behind the loader changes, so the bar for every output
of a call -- grads, loss, logits, the parameters and both Adam moments after the update, the step counter -- is
bit-equality with ``ops.frozen_step`` on the batch's windows copied out with torch indexing into a contiguous
[B, C, T] tensor (same model, same seed / offset or masks, same flags and ``train_from``).  One case per shape
is also held to the float64 oracle directly (frozen_cases.oracle_frozen at assert_frozen_grads_close's
tolerances: rtol 1e-4, atol 1e-5 * max|ref|)."""

from __future__ import annotations

import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"22x256": (22, 256), "22x257": (22, 257)}
OUTS = ("grads", "loss", "logits", "params", "moments", "step")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _cus():
    return torch.cuda.get_device_properties(_dev()).multi_processor_count


@functools.lru_cache(maxsize=None)
def _model(C, T, seed=3):
    """A train-mode model on the device (p = 0.5); shared, never modified (the calls update clones)."""
    from hip_cases import random_model
    return random_model(C, T, seed=seed).to(_dev()).train()


def _rec_np(R, C, N, seed):
    return np.random.default_rng(seed).standard_normal((R, C, N), dtype=np.float32)


def _table(T, N, R, seed):
    """tests/test_gpu_epochs.py::_table: starts covering 0, 1, 2, 3 mod 4, the last start N - T and its
    neighbours, and a shuffled rec_index."""
    last = N - T
    starts = [0, 1, 2, 3, 4, 5, 6, 7, T // 2, T // 2 + 1, T, T + 2, T + 3, last - 3, last - 2, last - 1, last, 0, last]
    rng = np.random.default_rng(seed)
    idx = rng.permutation(np.arange(len(starts)) % R)
    assert {s % 4 for s in starts} == {0, 1, 2, 3} and set(idx.tolist()) == set(range(R))
    return starts, idx.tolist()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, want, what=""):
    for k in OUTS:
        assert torch.equal(_bits(got[k]), _bits(want[k])), f"{what}: {k} differs"


def _start_state(m, fill=None):
    """Clones a call may update: the flat parameters, Adam moments off zero (the same for every call) and a
    step counter at 3; grads pre-filled with NaN (or ``fill``)."""
    flat = m.flat_parameters().detach().clone()
    g = torch.Generator(device="cpu").manual_seed(17)
    mom = (torch.rand(2 * flat.numel(), generator=g) * 1e-3).to(flat.device)
    step = torch.full((1,), 3, dtype=torch.int32, device=flat.device)
    grads = torch.full_like(flat, float("nan") if fill is None else fill)
    return flat, mom, step, grads


def _outs(flat, mom, step, grads, loss, logits):
    torch.cuda.synchronize()
    return dict(grads=grads, loss=loss, logits=logits, params=flat, moments=mom, step=step)


def _kw(m, B, masks, dlogits, clamp, stage, key_from_step, mom, step):
    dev = _dev()
    return dict(masks=masks, dlogits=dlogits, adam_state=mom, step_i32=step,
                loss=torch.full((1,), float("nan"), device=dev), logits=torch.full((B, 4), float("nan"), device=dev),
                clamp=clamp, key_from_step=key_from_step, train_from=stage)


def _windows(m, rec, starts, idx, labels, *, sel=None, masks=None, dlogits=None, clamp=True, stage=0, seed=11, offset=5,
             fill=None, key_from_step=False):
    """ops.frozen_step_windows from the start state; the tables as given (host or device)."""
    from eegnetreplication_amd import ops
    flat, mom, step, grads = _start_state(m, fill)
    B = len(sel) if sel is not None else len(starts)
    kw = _kw(m, B, masks, dlogits, clamp, stage, key_from_step, mom, step)
    ops.frozen_step_windows(m.shape, flat, m.flat_bn_buffers(), rec, starts, None if dlogits is not None else labels,
                            seed, offset, grads, ops.new_frozen_workspace(m.shape, B, _dev()), rec_index=idx, sel=sel,
                            **kw)
    return _outs(flat, mom, step, grads, kw["loss"], kw["logits"])


def _copied(m, rec, starts, idx, labels, *, sel=None, masks=None, dlogits=None, clamp=True, stage=0, seed=11, offset=5,
            fill=None, key_from_step=False):
    """The reference: ops.frozen_step on the batch's windows copied out with torch indexing (host tables)."""
    from eegnetreplication_amd import ops
    dev = _dev()
    flat, mom, step, grads = _start_state(m, fill)
    ent = list(range(len(starts))) if sel is None else list(sel)
    idx = [0] * len(starts) if idx is None else idx
    r3 = rec if rec.dim() == 3 else rec.unsqueeze(0)
    x = torch.stack([r3[idx[e], :, starts[e]:starts[e] + m.T] for e in ent]).contiguous()
    y = None if dlogits is not None else torch.tensor([labels[e] for e in ent], dtype=torch.int64, device=dev)
    B = len(ent)
    kw = _kw(m, B, masks, dlogits, clamp, stage, key_from_step, mom, step)
    ops.frozen_step(m.shape, flat, m.flat_bn_buffers(), x, seed, offset, grads, ops.new_frozen_workspace(m.shape, B, dev),
                    labels=y, **kw)
    return _outs(flat, mom, step, grads, kw["loss"], kw["logits"])


def _labels(n, seed):
    return np.random.default_rng(seed).integers(0, 4, n).tolist()


@functools.lru_cache(maxsize=None)
def _align_case(shape):
    """(model, rec, starts, idx, labels, the copied reference) of the alignment table; shared, never modified."""
    C, T = SHAPES[shape]
    m = _model(C, T)
    R, N = 3, 4 * T + 37
    rec = torch.from_numpy(_rec_np(R, C, N, 51)).to(_dev())
    starts, idx = _table(T, N, R, 52)
    labels = _labels(len(starts), 53)
    return m, rec, starts, idx, labels, _copied(m, rec, starts, idx, labels)


# ---- 1. alignments ----
@pytest.mark.parametrize("shape", list(SHAPES))
def test_alignments(shape):
    """R = 3 recordings of 4T + 37 samples and starts at every alignment: contiguous, as a slice one float into
    a NaN-filled buffer of odd pitch (a load outside the slice would make the loss NaN), and as an aligned
    slice at a pitch that is a multiple of 4 (16-byte loads where a start allows them)."""
    dev = _dev()
    m, rec, starts, idx, labels, ref = _align_case(shape)
    R, C, N = rec.shape
    keep = rec.clone()
    got = _windows(m, rec, starts, idx, labels)
    _same(got, ref, "contiguous")
    for k in OUTS:
        assert torch.isfinite(got[k].float()).all(), k
    assert got["step"].item() == 4 and not torch.equal(got["params"], m.flat_parameters())
    buf = torch.full((R, C, N + 7), float("nan"), dtype=torch.float32, device=dev)
    view = buf[:, :, 1:1 + N]
    view.copy_(rec)
    assert not view.is_contiguous() and view.data_ptr() % 16 == 4
    kept = buf.clone()
    got1 = _windows(m, view, starts, idx, labels)
    assert torch.isfinite(got1["loss"]).all() and torch.isfinite(got1["grads"]).all()
    _same(got1, ref, "one float into an odd pitch")
    assert torch.equal(_bits(buf), _bits(kept))
    buf4 = torch.full((R, C, N + 11), float("nan"), dtype=torch.float32, device=dev)
    assert (N + 11) % 4 == 0
    view4 = buf4[:, :, 4:4 + N]
    view4.copy_(rec)
    kept4 = buf4.clone()
    got4 = _windows(m, view4, starts, idx, labels)
    assert torch.isfinite(got4["loss"]).all() and torch.isfinite(got4["grads"]).all()
    _same(got4, ref, "aligned slice, pitch a multiple of 4")
    assert torch.equal(_bits(buf4), _bits(kept4))
    assert torch.equal(rec, keep)


# ---- 2. table forms ----
@pytest.mark.parametrize("shape", list(SHAPES))
def test_host_and_device_tables_give_the_same_bits(shape):
    dev = _dev()
    m, rec, starts, idx, labels, ref = _align_case(shape)
    _same(_windows(m, rec, np.array(starts), np.array(idx, dtype=np.int32), np.array(labels)), ref, "numpy")
    _same(_windows(m, rec, torch.tensor(starts), torch.tensor(idx), torch.tensor(labels)), ref, "CPU tensors")
    ds = torch.tensor(starts, dtype=torch.int64, device=dev)
    di = torch.tensor(idx, dtype=torch.int32, device=dev)
    dl = torch.tensor(labels, dtype=torch.int64, device=dev)
    _same(_windows(m, rec, ds, di, dl), ref, "device tensors")
    # recording 0 without a rec_index, and a 2-D recording
    ref0 = _copied(m, rec, starts, None, labels)
    _same(_windows(m, rec, starts, None, labels), ref0, "no rec_index")
    _same(_windows(m, rec[0], ds, None, dl), ref0, "2-D recording")
    with pytest.raises(ValueError, match=r"starts\[1\] = -1 is outside"):
        _windows(m, rec, [0, -1], None, [0, 1])
    with pytest.raises(ValueError, match=r"sel\[0\] = 2 is outside"):
        _windows(m, rec, [0, 1], None, [0, 1], sel=[2])


# ---- 3. the strided loop ----
@pytest.mark.parametrize("shape", list(SHAPES))
def test_more_windows_than_workgroups(shape):
    """B = 2 CUs + 3 windows of one recording: the next window's prefetch and a partial last round run."""
    C, T = SHAPES[shape]
    m = _model(C, T)
    N = T + 700
    rec = torch.from_numpy(_rec_np(1, C, N, 81)[0]).to(_dev())
    B = 2 * _cus() + 3
    rng = np.random.default_rng(82)
    starts = rng.integers(0, N - T + 1, B).tolist()
    labels = _labels(B, 83)
    _same(_windows(m, rec, starts, None, labels), _copied(m, rec, starts, None, labels), f"B = {B}")


def test_fewer_windows_than_workgroups():
    """B = 5: one window per workgroup, nothing is prefetched."""
    C, T = SHAPES["22x257"]
    m = _model(C, T)
    N = T + 700
    rec = torch.from_numpy(_rec_np(1, C, N, 84)[0]).to(_dev())
    starts = [3, 700, 0, 350, 1]
    _same(_windows(m, rec, starts, None, [0, 1, 2, 3, 0]), _copied(m, rec, starts, None, [0, 1, 2, 3, 0]), "B = 5")


# ---- 4. partial fine-tuning ----
@pytest.mark.parametrize("stage", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_partial_fine_tuning(shape, stage):
    """Every train_from at B = 7; grads, parameters and moments below the trainable offset keep their
    sentinel / start values."""
    from eegnetreplication_amd import ops
    m, rec, starts, idx, labels, _ = _align_case(shape)
    st, ix, lb = starts[2:9], idx[2:9], labels[2:9]
    got = _windows(m, rec, st, ix, lb, stage=stage, fill=-77.0)
    _same(got, _copied(m, rec, st, ix, lb, stage=stage, fill=-77.0), f"train_from {stage}")
    off = ops.trainable_offset(m.shape, stage)
    n = m.flat_parameters().numel()
    assert (off == 0) == (stage == 0) and off < n
    flat0, mom0, _, _ = _start_state(m)
    assert torch.isfinite(got["grads"][off:]).all() and not (got["grads"][off:] == -77.0).all()
    assert (got["grads"][:off] == -77.0).all()
    assert torch.equal(got["params"][:off], flat0[:off]) and not torch.equal(got["params"][off:], flat0[off:])
    assert torch.equal(got["moments"][:off], mom0[:off]) and torch.equal(got["moments"][n:n + off], mom0[n:n + off])


# ---- 5. sel ----
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sel_picks_table_entries_and_their_labels(shape):
    dev = _dev()
    m, rec, starts, idx, _, _ = _align_case(shape)
    labels = [e % 4 for e in range(len(starts))]
    sel = [17, 3, 11, 0, 6, 18, 9, 14]
    assert [labels[e] for e in sel] != labels[:len(sel)]           # a label taken by batch row would differ
    want = _windows(m, rec, [starts[e] for e in sel], [idx[e] for e in sel], [labels[e] for e in sel])
    _same(want, _copied(m, rec, starts, idx, labels, sel=sel), "gathered table")
    _same(_windows(m, rec, starts, idx, labels, sel=sel), want, "host sel")
    dsel = torch.tensor(sel, dtype=torch.int64, device=dev)
    _same(_windows(m, rec, starts, idx, labels, sel=dsel), want, "device sel")
    _same(_windows(m, rec, starts, idx, labels, sel=torch.tensor(sel + [0, 0], device=dev)[:8]), want, "a slice as sel")


# ---- 6. clamping ----
@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_tables_are_read_clamped(shape):
    """Device tables are never read by the host, so the kernel clamps them; the recordings sit in the middle of
    a NaN-filled buffer, and every output is finite and equal to the call on the clamped host tables."""
    dev = _dev()
    C, T = SHAPES[shape]
    m = _model(C, T)
    R, N = 3, 2 * T + 21
    buf = torch.full((R + 2, C, N + 8), float("nan"), dtype=torch.float32, device=dev)
    rec = buf[1:1 + R, :, 4:4 + N]
    rec.copy_(torch.from_numpy(_rec_np(R, C, N, 71)).to(dev))
    last = N - T
    ds = torch.tensor([-5, N, last + 1, -(1 << 40), 1 << 40, 7, 7], dtype=torch.int64, device=dev)
    di = torch.tensor([1, 1, 2, 0, 2, -1, R], dtype=torch.int32, device=dev)
    labels = [0, 1, 2, 3, 3, 2, 1]
    dl = torch.tensor(labels, dtype=torch.int64, device=dev)
    dsel = torch.tensor([-1, 7, 3, 6, 1, 5, 2, 4, 1 << 40], dtype=torch.int64, device=dev)
    got = _windows(m, rec, ds, di, dl, sel=dsel)
    for k in OUTS:
        assert torch.isfinite(got[k].float()).all(), k
    cs, ci, csel = [0, last, last, 0, last, 7, 7], [1, 1, 2, 0, 2, 0, R - 1], [0, 6, 3, 6, 1, 5, 2, 4, 6]
    want = _windows(m, rec, cs, ci, labels, sel=csel)
    _same(got, want, "clamped tables")
    _same(want, _copied(m, rec, cs, ci, labels, sel=csel), "copied")


# ---- 7. seeds and masks ----
@pytest.mark.parametrize("shape", list(SHAPES))
def test_masks_dlogits_and_no_clamp(shape):
    from golden_util import make_masks
    dev = _dev()
    m, rec, starts, idx, labels, ref = _align_case(shape)
    B = len(starts)
    m2, m3 = make_masks(B, m.F1 * m.D, m.T, 905, 0.5)
    masks = (torch.from_numpy(np.ascontiguousarray(m2)).to(dev, torch.uint8),
             torch.from_numpy(np.ascontiguousarray(m3)).to(dev, torch.uint8))
    got = _windows(m, rec, starts, idx, labels, masks=masks)
    _same(got, _copied(m, rec, starts, idx, labels, masks=masks), "injected masks")
    assert not torch.equal(got["logits"], ref["logits"])
    dlog = torch.from_numpy(np.random.default_rng(906).standard_normal((B, 4)).astype(np.float32)).to(dev)
    _same(_windows(m, rec, starts, idx, labels, dlogits=dlog), _copied(m, rec, starts, idx, labels, dlogits=dlog),
          "dlogits")
    raw = _windows(m, rec, starts, idx, labels, clamp=False, seed=5, offset=9)
    _same(raw, _copied(m, rec, starts, idx, labels, clamp=False, seed=5, offset=9), "clamp=False")


# ---- 8. graph capture ----
def test_graph_capture_with_device_tables():
    """One captured step with the dropout key from the device step counter; after new contents of rec, starts
    and sel and the start state restored, the replay equals the eager call on them at the same device step."""
    from eegnetreplication_amd import ops
    dev = _dev()
    C, T = SHAPES["22x257"]
    m = _model(C, T)
    R, N, n, B = 2, T + 300, 6, 4
    rec = torch.from_numpy(_rec_np(R, C, N, 91)).to(dev)
    ds = torch.tensor([0, 64, 300, 17, 5, 211], dtype=torch.int64, device=dev)
    di = torch.tensor([0, 1, 1, 0, 1, 0], dtype=torch.int32, device=dev)
    dl = torch.tensor([0, 1, 2, 3, 1, 2], dtype=torch.int64, device=dev)
    dsel = torch.tensor([5, 0, 3, 2], dtype=torch.int64, device=dev)
    flat, mom, step, grads = _start_state(m)
    flat0, mom0 = flat.clone(), mom.clone()
    loss = torch.zeros(1, device=dev)
    logits = torch.zeros((B, 4), device=dev)
    ws = ops.new_frozen_workspace(m.shape, B, dev)
    bn = m.flat_bn_buffers()

    def call():
        ops.frozen_step_windows(m.shape, flat, bn, rec, ds, dl, 21, 4, grads, ws, rec_index=di, sel=dsel, adam_state=mom,
                                step_i32=step, loss=loss, logits=logits, key_from_step=True)

    call()                                                           # eager once: the kernel's attributes are set
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    rec.copy_(torch.from_numpy(_rec_np(R, C, N, 92)).to(dev))
    ds.copy_(torch.tensor([5, 300, 1, 128, 77, 2], dtype=torch.int64))
    dsel.copy_(torch.tensor([1, 4, 4, 0], dtype=torch.int64))
    flat.copy_(flat0); mom.copy_(mom0); step.fill_(3)
    g.replay()
    torch.cuda.synchronize()
    got = {k: v.clone() for k, v in dict(grads=grads, loss=loss, logits=logits, params=flat, moments=mom, step=step).items()}
    want = _windows(m, rec, ds, di, dl, sel=dsel, seed=21, offset=4, key_from_step=True)
    _same(got, want, "replay")
    assert got["step"].item() == 4


# ---- 9. the float64 oracle ----
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_the_float64_oracle(shape):
    from frozen_cases import assert_frozen_grads_close, model_state, oracle_frozen
    from golden_util import assert_close, make_masks
    from hip_cases import flat_to_dict
    dev = _dev()
    m, rec, starts, idx, labels, _ = _align_case(shape)
    st, ix, lb = starts[1:16:3], idx[1:16:3], labels[1:16:3]
    B = len(st)
    m2, m3 = make_masks(B, m.F1 * m.D, m.T, 907, 0.5)
    masks = (torch.from_numpy(np.ascontiguousarray(m2)).to(dev, torch.uint8),
             torch.from_numpy(np.ascontiguousarray(m3)).to(dev, torch.uint8))
    got = _windows(m, rec, st, ix, lb, masks=masks)
    rec_np = rec.cpu().numpy()
    x = np.stack([rec_np[r, :, s:s + m.T] for s, r in zip(st, ix)])
    ref = oracle_frozen(model_state(m), x, 0.5, (m2, m3), labels=np.array(lb))
    assert_close(got["logits"].cpu().numpy(), ref["logits"], name=f"{shape} logits")
    assert_close(got["loss"].cpu().numpy()[0], ref["loss"], name=f"{shape} loss")
    assert_frozen_grads_close(flat_to_dict(m, got["grads"]), ref["grads"], raw=ref["raw"], prefix=f"{shape} grad ")


# ---- 10. the whole loop ----
def test_finetune_on_recording_equals_the_gather_loop():
    """n = 13 at batch 5, 2 epochs: the parameters, the moments, the step counter and the [2, 3] losses equal a
    hand loop that draws the same permutations and calls FusedTrainer.step on gathered copies."""
    from eegnetreplication_amd import FusedTrainer, finetune_on_recording
    dev = _dev()
    C, T = SHAPES["22x257"]
    R, N, n = 2, T + 500, 13
    rec = torch.from_numpy(_rec_np(R, C, N, 101)).to(dev)
    rng = np.random.default_rng(102)
    starts = rng.integers(0, N - T + 1, n).tolist()
    idx = rng.integers(0, R, n).tolist()
    labels = _labels(n, 103)
    ma = copy.deepcopy(_model(C, T)).freeze_bn().train_from("aggregation")
    mb = copy.deepcopy(ma)
    torch.manual_seed(1234)                                          # the dropout keys come from the global generator
    losses, ta = finetune_on_recording(ma, rec, starts, labels, idx, epochs=2, batch_size=5, lr=2e-3,
                                       generator=torch.Generator(device=dev).manual_seed(5))
    torch.cuda.synchronize()
    assert losses.shape == (2, 3) and losses.device.type == "cuda"
    torch.manual_seed(1234)
    tb = FusedTrainer(mb, lr=2e-3)
    gen = torch.Generator(device=dev).manual_seed(5)
    x_all = torch.stack([rec[r, :, s:s + T] for s, r in zip(starts, idx)])
    y_all = torch.tensor(labels, dtype=torch.int64, device=dev)
    want = []
    for _ in range(2):
        perm = torch.randperm(n, device=dev, generator=gen)
        for i in range(0, n, 5):
            sel = perm[i:i + 5]
            want.append(tb.step(x_all[sel].contiguous(), y_all[sel]).clone())
    torch.cuda.synchronize()
    assert torch.equal(_bits(losses), _bits(torch.cat(want).view(2, 3)))
    assert torch.equal(_bits(ma.flat_parameters()), _bits(mb.flat_parameters()))
    assert not torch.equal(ma.flat_parameters(), _model(C, T).flat_parameters())
    assert torch.equal(_bits(ta.adam.state), _bits(tb.adam.state))
    assert ta.adam.step.item() == tb.adam.step.item() == 6


# ---- 11. refusal ----
def test_wide_models_are_refused():
    from eegnetreplication_amd import EEGNet, FusedTrainer
    dev = _dev()
    wide = EEGNet(64, 512, F1=16, D=4).to(dev).freeze_bn().train()
    with pytest.raises(NotImplementedError, match="F1\\*D = 64 > 16 is not supported"):
        FusedTrainer(wide).step_epochs(torch.zeros((64, 1024), device=dev), [0, 5], [0, 1])
