"""Frozen-BatchNorm fine-tuning, the checks that need no GPU: the float64 oracle (tests/frozen_cases.py)
is pinned to the reference's own gradients with its BatchNorm modules in eval() (tests/golden/frozen/
FZ1.npz); ``EEGNet.freeze_bn`` is a plain flag that the module's mode changes leave alone and that the
batch-statistics trainers refuse; the library validates the frozen entry points before any device call."""

from __future__ import annotations

import copy
import ctypes
import os

import numpy as np
import pytest

from frozen_cases import (CLAMPS, FZ_DIR, assert_frozen_grads_close, load_fz_fixture, oracle_frozen)
from golden_util import PARAM_NAMES, assert_close


# ---- the oracle against the reference ----
@pytest.fixture(scope="module")
def fz1():
    z, meta, state, x, y = load_fz_fixture("FZ1")
    runs = {s: oracle_frozen(state, x, meta["p"], (z["mask2"], z["mask3"]), labels=y, loss_scale=float(s))
            for s in meta["scales"]}
    return z, meta, state, runs


def test_oracle_matches_reference_fixture(fz1):
    z, meta, state, runs = fz1
    assert (meta["C"], meta["T"], meta["B"], meta["p"]) == (22, 257, 3, 0.5)
    for s, r in runs.items():
        assert_close(r["logits"], z["logits"], name="FZ1 logits")
        assert_close(r["loss"], z["loss"], name="FZ1 loss")
        ref = {k: z[f"grad{s}.{k}"] for k in PARAM_NAMES}
        assert_frozen_grads_close(r["grads"], ref, raw=r["raw"], prefix=f"FZ1 x{s} grad ")
        # the hooks are exactly a clamp of the raw gradient
        for k in PARAM_NAMES:
            want = np.clip(r["raw"][k], -CLAMPS[k], CLAMPS[k]) if k in CLAMPS else r["raw"][k]
            assert np.array_equal(r["grads"][k], want), k


def test_fixture_exercises_bn1_gradients_and_both_clamps(fz1):
    z, meta, state, runs = fz1
    # gamma1 / beta1 are ordinary gradients here: nothing renormalises after BN1 when BN2 is frozen
    gmax = max(float(np.abs(z[f"grad1.{k}"]).max()) for k in PARAM_NAMES)
    for k in ("temporal.1.weight", "temporal.1.bias"):
        assert float(np.abs(z[f"grad1.{k}"]).max()) > 1e-2 * gmax, k
    raw = runs[64]["raw"]
    for k, c in CLAMPS.items():
        a = np.abs(raw[k])
        assert (a > c).any() and (a < c).any(), k


def test_frozen_step_leaves_the_buffers_alone(fz1):
    z, meta, state, runs = fz1
    for k, v in z.items():
        if k.startswith("buf1."):
            assert np.array_equal(v, state[k[5:]]), k                  # the reference's own
            assert np.array_equal(runs[1]["buffers"][k[5:]], state[k[5:]]), k
    assert any(k.startswith("buf1.") and k.endswith("num_batches_tracked") for k in z)


def test_fixture_is_no_larger_than_the_largest_training_fixture():
    from golden_util import GOLDEN_DIR, fixture_names
    assert "FZ1" not in fixture_names()           # tests/golden/*.npz are training fixtures
    size = os.path.getsize(os.path.join(FZ_DIR, "FZ1.npz"))
    largest = max(os.path.getsize(os.path.join(GOLDEN_DIR, f)) for f in os.listdir(GOLDEN_DIR)
                  if f.endswith(".npz"))
    assert size <= largest


# ---- the flag ----
def test_freeze_bn_is_a_plain_flag_outside_the_state_dict():
    import torch
    from eegnetreplication_amd import EEGNet
    m = EEGNet(22, 257)
    keys = list(m.state_dict().keys())
    assert m.bn_frozen is False
    assert m.freeze_bn() is m and m.bn_frozen is True
    assert list(m.state_dict().keys()) == keys
    assert "bn_frozen" not in dict(m.named_buffers())
    assert m.train().bn_frozen and m.eval().bn_frozen and m.train(False).bn_frozen
    assert m.to(torch.float32).bn_frozen and m.to("cpu").bn_frozen
    assert copy.deepcopy(m).bn_frozen
    # train() / eval() do what they always did to the submodules: the flag is not bn.eval()
    assert all(bn.training for bn in m.train()._bns())
    assert m.freeze_bn(False) is m and m.bn_frozen is False
    assert not copy.deepcopy(m).bn_frozen
    fresh = EEGNet(22, 257)
    fresh.load_state_dict(m.freeze_bn().state_dict())
    assert fresh.bn_frozen is False


def test_batch_statistics_trainers_refuse_a_frozen_model():
    from eegnetreplication_amd import EEGNet
    from eegnetreplication_amd.distributed import DataParallelTrainer
    from eegnetreplication_amd.folds import FoldBatch
    m = EEGNet(22, 257).freeze_bn()
    with pytest.raises(ValueError, match="freeze_bn"):
        FoldBatch([m], [1])
    with pytest.raises(ValueError, match="freeze_bn"):
        FoldBatch([EEGNet(22, 257), m], [1, 2])
    with pytest.raises(ValueError, match="freeze_bn"):
        DataParallelTrainer(m)
    with pytest.raises(ValueError, match="freeze_bn"):
        DataParallelTrainer(m, sync_bn=True)
    # frozen after construction: the steps check before any device work
    t = DataParallelTrainer.__new__(DataParallelTrainer)
    t.model, t.sync_bn, t._step = m, False, 0
    with pytest.raises(ValueError, match="freeze_bn"):
        t.step(None, None)
    t.sync_bn = True
    with pytest.raises(ValueError, match="freeze_bn"):
        t.step(None, None)
    assert t._step == 0
    fb = FoldBatch.__new__(FoldBatch)
    fb.models = [m]
    with pytest.raises(ValueError, match="freeze_bn"):
        fb.epoch([(None, None)])


# ---- the library's validation ----
def _lib_or_skip():
    from eegnetreplication_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libeegnet_hip.so not built (run __graft_entry__.build())")
    return _lib, _lib.load()


def _p(v):
    return ctypes.c_void_p(v) if v else None      # never dereferenced: the calls fail first


def _step(lib, d, params=256, bn=256, x=256, dlogits=0, labels=256, grads=256, adam=0, step=0, loss=256,
          logits=256, ws=256, flags=0):
    return lib.eegnet_frozen_step(ctypes.byref(d), _p(params), _p(bn), _p(x), _p(dlogits), _p(labels), None, None,
                                  1, 2, _p(grads), _p(adam), _p(step), 1e-3, 0.9, 0.999, 1e-7, _p(loss),
                                  _p(logits), _p(ws), None, flags)


def _fwd(lib, d, params=256, bn=256, x=256, logits=256):
    return lib.eegnet_forward_frozen(ctypes.byref(d), _p(params), _p(bn), _p(x), None, None, 1, 2, _p(logits), None)


def test_library_exports_the_frozen_entry_points():
    _lib, lib = _lib_or_skip()
    for name in ("eegnet_frozen_workspace_bytes", "eegnet_forward_frozen", "eegnet_frozen_step"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.eegnet_abi_version() == 5 == _lib.ABI_VERSION
    nb = ctypes.c_size_t(0)
    for B in (1, 64, 4096):
        assert lib.eegnet_frozen_workspace_bytes(ctypes.byref(_lib.dims(B, 22, 257)), ctypes.byref(nb)) == 0
        assert nb.value > 0
    assert lib.eegnet_frozen_workspace_bytes(ctypes.byref(_lib.dims(4, 22, 257)), None) == -1


def test_null_pointers_are_rejected_by_name():
    _lib, lib = _lib_or_skip()
    d = _lib.dims(5, 22, 257)
    for name in ("params", "bn", "x", "grads", "ws"):
        assert _step(lib, d, **{name: 0}) == -1, name
        assert b"is NULL" in lib.eegnet_last_error(), name
    for name in ("params", "bn", "x", "logits"):
        assert _fwd(lib, d, **{name: 0}) == -1, name
        assert b"is NULL" in lib.eegnet_last_error(), name
    assert _step(lib, d, adam=256, step=0) == -1
    assert b"step is NULL" in lib.eegnet_last_error()


def test_exactly_one_of_dlogits_and_labels():
    _lib, lib = _lib_or_skip()
    d = _lib.dims(5, 22, 257)
    assert _step(lib, d, dlogits=0, labels=0) == -1
    assert b"dlogits or labels" in lib.eegnet_last_error()
    assert _step(lib, d, dlogits=256, labels=256) == -1
    assert b"exclusive" in lib.eegnet_last_error()


def test_flags_are_validated():
    _lib, lib = _lib_or_skip()
    d = _lib.dims(5, 22, 257)
    for flags in (4, 8, 1 | 4, 1 << 20):
        assert _step(lib, d, flags=flags) == -1, flags
        assert b"unknown flags" in lib.eegnet_last_error()
    assert _step(lib, d, flags=2, step=0) == -1
    assert b"EEGNET_KEY_FROM_STEP needs the device step counter" in lib.eegnet_last_error()


def test_wide_dims_pitch_and_geometry_are_rejected():
    _lib, lib = _lib_or_skip()
    nb = ctypes.c_size_t(0)
    for C, T in ((64, 512), (22, 256)):
        d = _lib.dims(1, C, T, F1=16, D=4)
        for rc in (_step(lib, d), _fwd(lib, d), lib.eegnet_frozen_workspace_bytes(ctypes.byref(d), ctypes.byref(nb))):
            assert rc == -1
            assert lib.eegnet_last_error() == b"frozen BatchNorm: F1*D = 64 > 16 is not supported"
    d = _lib.dims(5, 22, 257, x_pitch=260)
    for rc in (_step(lib, d), _fwd(lib, d)):
        assert rc == -1
        assert b"x_pitch" in lib.eegnet_last_error()
    assert _step(lib, _lib.dims(5, 22, 256, K1=48)) == -1         # the geometry's own checks come first
    assert _step(lib, _lib.dims(0, 22, 256)) == -1


def test_lds_budget_is_checked_with_the_bytes_named():
    """A narrow shape the train step takes, but whose x, s, v and block-2 rows together do not fit one
    workgroup's LDS, is rejected with the bytes named."""
    _lib, lib = _lib_or_skip()
    d = _lib.dims(2, 1, 1024)
    nb = ctypes.c_size_t()
    assert lib.eegnet_workspace_bytes(ctypes.byref(d), ctypes.byref(nb)) == 0
    for rc in (_step(lib, d), _fwd(lib, d), lib.eegnet_frozen_workspace_bytes(ctypes.byref(d), ctypes.byref(nb))):
        assert rc == -1
        msg = lib.eegnet_last_error()
        assert msg.startswith(b"frozen BatchNorm: dims need ") and b" B of LDS" in msg
