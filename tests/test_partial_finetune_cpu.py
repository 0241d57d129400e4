"""Partial fine-tuning (EEGNet.train_from: the frozen-BatchNorm step trains a suffix of the layers), the
checks that need no GPU: eegnet_trainable_offset against the cumulative parameter sizes; the library's
validation of the two new entry points; ``train_from`` / ``trainable_stage`` on a CPU-constructed model
and the refusal of every requires_grad pattern that is no frozen prefix; which optimizers ``_fusable``
takes for a frozen-BatchNorm model."""

from __future__ import annotations

import ctypes
import os

import pytest

STAGES = ("temporal", "aggregation", "block_2", "classifier")
FIRST = {"temporal": "temporal.0.weight", "aggregation": "aggregation.0.weight",
         "block_2": "block_2.0.weight", "classifier": "classifier.weight"}
BAD_STAGE = b"train_from must be EEGNET_TRAIN_ALL (0), EEGNET_TRAIN_FROM_AGGREGATION (1), " \
            b"EEGNET_TRAIN_FROM_BLOCK2 (2) or EEGNET_TRAIN_FROM_CLASSIFIER (3)"


def _lib_or_skip():
    from eegnetreplication_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libeegnet_hip.so not built (run __graft_entry__.build())")
    return _lib, _lib.load()


def _p(v):
    return ctypes.c_void_p(v) if v else None      # never dereferenced: the calls fail first


def _step(lib, d, train_from, params=256, bn=256, x=256, dlogits=0, labels=256, grads=256, adam=0, step=0,
          loss=256, logits=256, ws=256, flags=0):
    return lib.eegnet_frozen_step_from(ctypes.byref(d), _p(params), _p(bn), _p(x), _p(dlogits), _p(labels), None,
                                       None, 1, 2, _p(grads), _p(adam), _p(step), 1e-3, 0.9, 0.999, 1e-7, _p(loss),
                                       _p(logits), _p(ws), None, flags, train_from)


def _folds(lib, d, train_from, nfolds=3, folds=256, row0=0, slot=0, flags=0):
    return lib.eegnet_frozen_step_folds_from(ctypes.byref(d), nfolds, _p(folds), row0, slot, 0, 1e-3, 0.9, 0.999,
                                             1e-7, flags, None, train_from)


# ---- the offsets ----
@pytest.mark.parametrize("C,T,F1,D,K1", [(22, 256, 8, 2, 32), (22, 257, 8, 2, 32), (22, 257, 8, 2, 64),
                                        (5, 96, 4, 1, 32), (8, 64, 8, 2, 32), (22, 256, 2, 2, 32)])
def test_trainable_offset_is_the_cumulative_parameter_size(C, T, F1, D, K1):
    _lib, lib = _lib_or_skip()
    from eegnetreplication_amd import ops
    shape = ops.Shape(C=C, T=T, F1=F1, D=D, K1=K1)
    start, o = {}, 0
    for name, s in shape.param_shapes():
        start[name] = o
        k = 1
        for n in s:
            k *= n
        o += k
    assert o == shape.n_params()
    out = ctypes.c_int64(-1)
    for i, stage in enumerate(STAGES):
        assert lib.eegnet_trainable_offset(ctypes.byref(shape.dims(7)), i, ctypes.byref(out)) == 0
        assert out.value == start[FIRST[stage]], stage
        assert ops.trainable_offset(shape, stage) == ops.trainable_offset(shape, i) == start[FIRST[stage]]
    assert ops.trainable_offset(shape, "temporal") == 0
    with pytest.raises(ValueError, match="stage must be one of"):
        ops.trainable_offset(shape, "spatial")


def test_library_exports_the_partial_entry_points():
    _lib, lib = _lib_or_skip()
    for name in ("eegnet_trainable_offset", "eegnet_frozen_step_from", "eegnet_frozen_step_folds_from"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.eegnet_abi_version() == 5 == _lib.ABI_VERSION


# ---- the library's validation ----
def test_a_bad_train_from_is_rejected_with_the_four_values_named():
    _lib, lib = _lib_or_skip()
    d = _lib.dims(5, 22, 257)
    out = ctypes.c_int64(0)
    for bad in (-1, 4, 7, 1 << 20):
        for rc in (_step(lib, d, bad), _folds(lib, d, bad),
                   lib.eegnet_trainable_offset(ctypes.byref(d), bad, ctypes.byref(out))):
            assert rc == -1, bad
            assert lib.eegnet_last_error().startswith(BAD_STAGE), bad
    assert lib.eegnet_trainable_offset(ctypes.byref(d), 1, None) == -1
    assert b"out is NULL" in lib.eegnet_last_error()


@pytest.mark.parametrize("stage", [0, 1, 2, 3])
def test_flags_and_pointers_are_checked_as_by_the_full_step(stage):
    _lib, lib = _lib_or_skip()
    d = _lib.dims(5, 22, 257)
    for name in ("params", "bn", "x", "grads", "ws"):
        assert _step(lib, d, stage, **{name: 0}) == -1, name
        assert b"is NULL" in lib.eegnet_last_error(), name
    assert _step(lib, d, stage, adam=256, step=0) == -1
    assert b"step is NULL" in lib.eegnet_last_error()
    assert _step(lib, d, stage, dlogits=0, labels=0) == -1
    assert b"dlogits or labels" in lib.eegnet_last_error()
    assert _step(lib, d, stage, dlogits=256, labels=256) == -1
    assert b"exclusive" in lib.eegnet_last_error()
    for flags in (4, 8, 1 | 4, 1 << 20):
        assert _step(lib, d, stage, flags=flags) == -1, flags
        assert b"frozen step: unknown flags" in lib.eegnet_last_error()
    assert _step(lib, d, stage, flags=2, step=0) == -1
    assert b"EEGNET_KEY_FROM_STEP needs the device step counter" in lib.eegnet_last_error()
    # the fold call: its own flag set (the keys always follow the device step), table and counts
    for flags in (2, 4, 1 | 2):
        assert _folds(lib, d, stage, flags=flags) == -1, flags
        assert b"frozen fold step: unknown flags" in lib.eegnet_last_error()
    assert _folds(lib, d, stage, folds=0) == -1
    assert b"folds is NULL" in lib.eegnet_last_error()
    for nf in (0, 65536):
        assert _folds(lib, d, stage, nfolds=nf) == -1
        assert b"nfolds must be in [1, 65535]" in lib.eegnet_last_error()
    assert _folds(lib, d, stage, row0=-1) == -1 and _folds(lib, d, stage, slot=-1) == -1


@pytest.mark.parametrize("stage", [1, 2, 3])
def test_wide_dims_and_pitch_are_rejected_as_by_the_full_step(stage):
    _lib, lib = _lib_or_skip()
    out = ctypes.c_int64(0)
    for C, T in ((64, 512), (22, 256)):
        d = _lib.dims(1, C, T, F1=16, D=4)
        for rc in (_step(lib, d, stage), _folds(lib, d, stage),
                   lib.eegnet_trainable_offset(ctypes.byref(d), stage, ctypes.byref(out))):
            assert rc == -1
            assert lib.eegnet_last_error() == b"frozen BatchNorm: F1*D = 64 > 16 is not supported"
    assert _step(lib, _lib.dims(5, 22, 257, x_pitch=260), stage) == -1
    assert b"x_pitch" in lib.eegnet_last_error()


# ---- the module ----
def _flags(m):
    return {k: p.requires_grad for k, p in m.named_parameters()}


def test_train_from_and_trainable_stage_round_trip():
    from eegnetreplication_amd import EEGNet
    m = EEGNet(22, 257)
    names = [k for k, _ in m.named_parameters()]
    assert m.trainable_stage() == 0
    for i, stage in enumerate(STAGES):
        for arg in (stage, i):
            assert m.train_from(arg) is m
            cut = names.index(FIRST[stage])
            assert _flags(m) == {k: j >= cut for j, k in enumerate(names)}, stage
            assert m.trainable_stage() == i
    assert m.train_from("temporal").trainable_stage() == 0 and all(_flags(m).values())
    for bad in ("spatial", "block_1", 4, -1):
        with pytest.raises(ValueError, match="stage must be one of"):
            m.train_from(bad)
    # not a buffer, not in the state dict; freeze_bn is independent of it
    assert m.train_from("block_2").bn_frozen is False
    assert list(m.state_dict().keys()) == list(EEGNet(22, 257).state_dict().keys())


@pytest.mark.parametrize("pattern,bad", [
    ("one tensor of a module frozen", "temporal.1.bias"),
    ("a frozen layer after a trainable one", "block_2.1.weight"),
    ("only the temporal block frozen", "spatial.weight"),
    ("one half of an affine pair frozen", "aggregation.0.bias"),
    ("a hole in the suffix", "block_2.2.weight"),
    ("nothing trainable", "classifier.bias"),
])
def test_unsupported_requires_grad_patterns_raise(pattern, bad):
    from eegnetreplication_amd import EEGNet
    m = EEGNet(22, 257)
    p = dict(m.named_parameters())
    if pattern == "one tensor of a module frozen":
        p["temporal.1.bias"].requires_grad_(False)
    elif pattern == "a frozen layer after a trainable one":
        p["block_2.1.weight"].requires_grad_(False)
    elif pattern == "only the temporal block frozen":
        for k in ("temporal.0.weight", "temporal.1.weight", "temporal.1.bias"):
            p[k].requires_grad_(False)
    elif pattern == "one half of an affine pair frozen":
        m.train_from("aggregation")
        p["aggregation.0.weight"].requires_grad_(False)
    elif pattern == "a hole in the suffix":
        m.train_from("block_2")
        p["block_2.2.weight"].requires_grad_(False)
    else:
        for q in p.values():
            q.requires_grad_(False)
    with pytest.raises(NotImplementedError) as e:
        m.trainable_stage()
    msg = str(e.value)
    assert bad in msg, msg
    for stage in STAGES:
        assert stage in msg, msg


# ---- which optimizers the fused step takes ----
def test_fusable_accepts_both_optimizer_forms_for_a_frozen_bn_model():
    import torch
    from eegnetreplication_amd import EEGNet
    from eegnetreplication_amd.model import _fusable
    loss = torch.nn.CrossEntropyLoss()
    for stage in STAGES:
        m = EEGNet(22, 257).freeze_bn().train_from(stage)
        assert _fusable(m, torch.optim.Adam(m.parameters(), lr=1e-3), loss), stage
        assert _fusable(m, torch.optim.Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=1e-3), loss), stage
    # a suffix optimizer whose stage does not match the flags
    m = EEGNet(22, 257).freeze_bn().train_from("block_2")
    opt = torch.optim.Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=1e-3)
    for other in ("aggregation", "classifier", "temporal"):
        assert not _fusable(m.train_from(other), opt, loss), other
    assert _fusable(m.train_from("block_2"), opt, loss)
    # a subset that is no suffix, a suffix in another order, an unsupported pattern
    ps = list(m.parameters())
    assert not _fusable(m, torch.optim.Adam(ps[6:9] + ps[10:], lr=1e-3), loss)
    assert not _fusable(m, torch.optim.Adam(ps[6:][::-1], lr=1e-3), loss)
    ps[8].requires_grad_(False)
    assert not _fusable(m, torch.optim.Adam([q for q in ps if q.requires_grad], lr=1e-3), loss)
    # without frozen BatchNorm nothing changes: the five-pass step has no suffix form
    m = EEGNet(22, 257).train_from("block_2")
    assert not _fusable(m, torch.optim.Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=1e-3), loss)
    assert _fusable(m, torch.optim.Adam(m.parameters(), lr=1e-3), loss)


def test_fused_adam_state_skips_frozen_parameters():
    """load_from / store_to of a frozen-BatchNorm model leave a frozen parameter as stock Adam leaves one
    whose grad is None: no optimizer.state entry, no grad."""
    import torch
    from eegnetreplication_amd import EEGNet
    from eegnetreplication_amd.model import FusedAdamState
    m = EEGNet(22, 257).freeze_bn().train_from("block_2")
    names = [k for k, _ in m.named_parameters()]
    for opt in (torch.optim.Adam(m.parameters(), lr=1e-3),
                torch.optim.Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=1e-3)):
        st = FusedAdamState(m, opt)
        st.step.fill_(2)
        st.state.fill_(0.5)
        st.grads.fill_(0.25)
        st.store_to(m, opt)
        for k, p in m.named_parameters():
            if names.index(k) < names.index("block_2.0.weight"):
                assert p not in opt.state and p.grad is None, k
            else:
                assert int(opt.state[p]["step"]) == 2 and p.grad is not None, k
                assert opt.state[p]["exp_avg"].shape == p.shape
        m.zero_grad()
