"""Fold-indexed frozen-BatchNorm fine-tuning, the checks that need no GPU: the header declares
eegnet_frozen_step_folds and the binding lists it, the eegnet_fold layout and the ABI version are the
ones the fold-indexed train step has, the library validates the call before any device call, and
``FrozenFoldBatch`` takes frozen models only (``FoldBatch`` keeps refusing them)."""

from __future__ import annotations

import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- header, binding and ABI ----
def test_header_declares_the_call_with_twelve_parameters():
    from eegnetreplication_amd import _lib
    txt = open(os.path.join(ROOT, "include", "eegnet_abi.h")).read()
    m = re.search(r"^\s*int\s+eegnet_frozen_step_folds\s*\((.*?)\);", txt, re.S | re.M)
    assert m is not None
    assert len(m.group(1).split(",")) == 12
    assert "eegnet_frozen_step_folds" in _lib.EXPORTED_SYMBOLS
    assert len(_lib._SIGS["eegnet_frozen_step_folds"][1]) == 12
    assert re.search(r"#define EEGNET_ABI_VERSION 5\b", txt)


def _lib_or_skip():
    from eegnetreplication_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libeegnet_hip.so not built (run __graft_entry__.build())")
    return _lib, _lib.load()


def test_library_exports_the_call_and_keeps_the_fold_layout():
    _lib, lib = _lib_or_skip()
    assert hasattr(lib, "eegnet_frozen_step_folds")
    assert lib.eegnet_abi_version() == 5 == _lib.ABI_VERSION
    assert lib.eegnet_fold_bytes() == ctypes.sizeof(_lib.Fold)


# ---- validation: dummy pointers, never dereferenced (every call fails first) ----
def _call(lib, d, nfolds=3, folds=256, row0=0, slot=0, flags=0):
    return lib.eegnet_frozen_step_folds(ctypes.byref(d), nfolds, ctypes.c_void_p(folds) if folds else None, row0,
                                        slot, 0, 1e-3, 0.9, 0.999, 1e-7, flags, None)


def test_wide_dims_are_rejected_naming_the_limit():
    _lib, lib = _lib_or_skip()
    assert _call(lib, _lib.dims(4, 64, 512, F1=16, D=4)) == -1
    assert b"F1*D" in lib.eegnet_last_error()


@pytest.mark.parametrize("kw", [dict(nfolds=0), dict(nfolds=65536), dict(folds=0), dict(row0=-1), dict(slot=-1),
                                dict(flags=2), dict(flags=4)], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_arguments_are_validated(kw):
    _lib, lib = _lib_or_skip()
    assert _call(lib, _lib.dims(5, 22, 257), **kw) == -1
    assert lib.eegnet_last_error() != b""


def test_a_row_pitch_is_rejected():
    _lib, lib = _lib_or_skip()
    assert _call(lib, _lib.dims(5, 22, 257, x_pitch=260)) == -1
    assert b"x_pitch" in lib.eegnet_last_error()


# ---- FrozenFoldBatch on CPU models ----
def test_frozen_fold_batch_takes_frozen_models_only():
    from eegnetreplication_amd import EEGNet, FrozenFoldBatch
    with pytest.raises(ValueError, match="freeze_bn"):
        FrozenFoldBatch([EEGNet(22, 257)], [1])
    with pytest.raises(ValueError, match="freeze_bn"):
        FrozenFoldBatch([EEGNet(22, 257).freeze_bn(), EEGNet(22, 257)], [1, 2])
    # unfrozen after construction: epoch() checks before any device work
    fb = FrozenFoldBatch.__new__(FrozenFoldBatch)
    fb.models = [EEGNet(22, 257).freeze_bn(), EEGNet(22, 257).freeze_bn()]
    fb.models[1].freeze_bn(False)
    with pytest.raises(ValueError, match="freeze_bn"):
        fb.epoch([(None, None), (None, None)])


def test_frozen_fold_batch_runs_on_a_hip_device_only():
    from eegnetreplication_amd import EEGNet, FrozenFoldBatch
    with pytest.raises(RuntimeError, match="HIP device only"):
        FrozenFoldBatch([EEGNet(22, 257).freeze_bn(), EEGNet(22, 257).freeze_bn()], [1, 2])
