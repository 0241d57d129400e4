"""Fine-tuning on cue epochs read in place (eegnet_frozen_step_windows): everything that needs no GPU -- every
host refusal of the C entry point with its message, through ctypes and with pointers that are never
dereferenced (the calls fail first), FusedTrainer.step_epochs on an unfrozen model, and the batch slicing of
finetune_on_recording."""

from __future__ import annotations

import ctypes
import os

import pytest


def _lib_or_skip():
    from eegnetreplication_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libeegnet_hip.so not built (run __graft_entry__.build())")
    return _lib, _lib.load()


def _p(v):
    return ctypes.c_void_p(v) if v else None      # never dereferenced: the calls fail first


def _step(lib, d, params=256, bn=256, rec=256, n_rec=2, n_samples=1000, pitch=1000, starts=256, rec_index=256,
          labels=256, n_table=8, sel=0, dlogits=0, grads=256, adam=0, step=0, loss=256, logits=256, ws=256, flags=0,
          train_from=0):
    return lib.eegnet_frozen_step_windows(
        ctypes.byref(d), _p(params), _p(bn), _p(rec), n_rec, n_samples, pitch, _p(starts), _p(rec_index), _p(labels),
        n_table, _p(sel), _p(dlogits), None, None, 1, 2, _p(grads), _p(adam), _p(step), 1e-3, 0.9, 0.999, 1e-7,
        _p(loss), _p(logits), _p(ws), None, flags, train_from)


def _refused(lib, d, msg, **kw):
    assert _step(lib, d, **kw) == -1, kw
    err = lib.eegnet_last_error()
    assert msg in err, (kw, err)


def test_library_exports_the_entry_point():
    _lib, lib = _lib_or_skip()
    assert "eegnet_frozen_step_windows" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "eegnet_frozen_step_windows")
    assert lib.eegnet_abi_version() == 5 == _lib.ABI_VERSION       # no struct changed


def test_null_pointers_are_rejected_by_name():
    _lib, lib = _lib_or_skip()
    d = _lib.dims(5, 22, 257)
    for name, said in (("params", b"params"), ("bn", b"bn_buffers"), ("rec", b"rec"), ("grads", b"grads"),
                       ("starts", b"starts"), ("ws", b"ws")):
        _refused(lib, d, said + b" is NULL", **{name: 0})
    _refused(lib, d, b"step is NULL", adam=256, step=0)
    assert lib.eegnet_frozen_step_windows(None, *([None] * 3), 1, 1000, 1000, *([None] * 3), 8, *([None] * 4), 1, 2,
                                          *([None] * 3), 1e-3, 0.9, 0.999, 1e-7, *([None] * 4), 0, 0) == -1


def test_exactly_one_of_labels_and_dlogits():
    _lib, lib = _lib_or_skip()
    d = _lib.dims(5, 22, 257)
    _refused(lib, d, b"frozen step on windows: need dlogits or labels", labels=0, dlogits=0)
    _refused(lib, d, b"frozen step on windows: dlogits and labels are exclusive", labels=256, dlogits=256)


def test_the_recordings_are_checked():
    _lib, lib = _lib_or_skip()
    d = _lib.dims(5, 22, 257)
    _refused(lib, d, b"n_samples = 256 is shorter than one window (T = 257)", n_samples=256, pitch=1000)
    _refused(lib, d, b"pitch = 999 is below n_samples = 1000", pitch=999)
    for n_rec in (0, -1, 1 << 31):
        _refused(lib, d, b"n_rec must be in [1, 2^31)", n_rec=n_rec)


@pytest.mark.parametrize("name,addr", [("rec", 258), ("starts", 260), ("rec_index", 258), ("labels", 260),
                                       ("sel", 260)])
def test_misaligned_pointers_are_rejected(name, addr):
    _lib, lib = _lib_or_skip()
    d = _lib.dims(5, 22, 256)
    _refused(lib, d, b"must be aligned to their element size", **{name: addr})


def test_no_16_byte_alignment_is_asked_of_rec():
    """A recording at any 4-byte alignment passes the alignment checks of a T % 4 == 0 shape (the contiguous
    step asks 16 bytes of x): with rec at 260 the call gets as far as the next refusal."""
    _lib, lib = _lib_or_skip()
    d = _lib.dims(5, 22, 256)
    _refused(lib, d, b"n_table must be in [1, 2^31)", rec=260, n_table=0)


def test_the_table_length_is_checked():
    _lib, lib = _lib_or_skip()
    d = _lib.dims(5, 22, 257)
    for n_table in (0, -3, 1 << 31):
        _refused(lib, d, b"n_table must be in [1, 2^31)", n_table=n_table, sel=256)
    _refused(lib, d, b"B = 5 windows exceed the table's 4 entries (no sel)", n_table=4)
    # with sel the batch may be longer than the table: the call gets past the table checks, to the flags'
    _refused(lib, d, b"EEGNET_KEY_FROM_STEP needs the device step counter", n_table=4, sel=256, flags=2)


def test_flags_and_train_from_are_validated():
    _lib, lib = _lib_or_skip()
    d = _lib.dims(5, 22, 257)
    for flags in (4, 8, 1 | 4, 1 << 20):
        _refused(lib, d, b"frozen step on windows: unknown flags", flags=flags)
    _refused(lib, d, b"EEGNET_KEY_FROM_STEP needs the device step counter", flags=2, step=0)
    for stage in (-1, 4, 17):
        _refused(lib, d, b"train_from must be EEGNET_TRAIN_ALL (0)", train_from=stage)


def test_wide_dims_pitch_and_geometry_are_rejected():
    _lib, lib = _lib_or_skip()
    for C, T in ((64, 512), (22, 256)):
        d = _lib.dims(1, C, T, F1=16, D=4)
        assert _step(lib, d) == -1
        assert lib.eegnet_last_error() == b"frozen BatchNorm: F1*D = 64 > 16 is not supported"
    _refused(lib, _lib.dims(5, 22, 257, x_pitch=260), b"x_pitch 0 or T")
    assert _step(lib, _lib.dims(5, 22, 257, x_pitch=257), flags=4) == -1      # x_pitch = T passes that check
    assert b"unknown flags" in lib.eegnet_last_error()
    assert _step(lib, _lib.dims(5, 22, 256, K1=48)) == -1         # the geometry's own checks come first
    assert _step(lib, _lib.dims(0, 22, 256)) == -1


def test_step_epochs_refuses_an_unfrozen_model():
    from eegnetreplication_amd import EEGNet, FusedTrainer
    m = EEGNet(22, 257)
    t = FusedTrainer(m)
    off = m._rng_offset
    with pytest.raises(RuntimeError, match="freeze_bn"):
        t.step_epochs(None, [0, 1], [0, 1])
    assert m._rng_offset == off                                   # refused before a dropout key is drawn


def test_finetune_on_recording_refuses_an_unfrozen_model_and_is_exported():
    import eegnetreplication_amd as pkg
    assert "finetune_on_recording" in pkg.__all__
    with pytest.raises(RuntimeError, match="freeze_bn"):
        pkg.finetune_on_recording(pkg.EEGNet(22, 257), None, [0], [0])


def test_batch_slicing():
    """n = 13 at batch 5: steps of 5, 5 and 3, the last one short (no drop_last)."""
    from eegnetreplication_amd.model import batch_slices
    assert batch_slices(13, 5) == [(0, 5), (5, 10), (10, 13)]
    assert [j - i for i, j in batch_slices(13, 5)] == [5, 5, 3]
    assert batch_slices(10, 5) == [(0, 5), (5, 10)]
    assert batch_slices(3, 64) == [(0, 3)]
    assert batch_slices(0, 5) == []
    with pytest.raises(ValueError, match="batch_size"):
        batch_slices(13, 0)


def test_finetune_on_recording_passes_the_slices_of_one_permutation_per_epoch(monkeypatch):
    """The device call stubbed out: per epoch one permutation of the table, cut into sel slices of 5, 5, 3."""
    import torch
    from eegnetreplication_amd import EEGNet, FusedTrainer, model as mod
    m = EEGNet(22, 257).freeze_bn()
    t = FusedTrainer(m)
    seen = []

    def fake_step(rec, starts, y, rec_index=None, sel=None, logits=None):
        seen.append(sel.clone())
        return torch.full((1,), float(len(seen)))

    monkeypatch.setattr(t, "step_epochs", fake_step)
    monkeypatch.setattr(mod, "require_device", lambda *a: None)
    monkeypatch.setattr(mod, "_host_table", lambda tab, *a: torch.as_tensor(tab))
    rec = torch.zeros((22, 2000))
    losses, got = mod.finetune_on_recording(m, rec, list(range(13)), [0] * 13, epochs=2, batch_size=5, trainer=t,
                                            generator=torch.Generator().manual_seed(7))
    assert got is t
    assert [len(s) for s in seen] == [5, 5, 3, 5, 5, 3]
    g = torch.Generator().manual_seed(7)
    for e in range(2):
        perm = torch.randperm(13, generator=g)
        assert torch.equal(torch.cat(seen[3 * e:3 * e + 3]), perm)
    assert torch.equal(losses, torch.tensor([[1., 2., 3.], [4., 5., 6.]]))
