"""Eval-mode input gradients, the checks that need no GPU: the float64 dx oracle is pinned to the
reference's own ``x.grad`` (tests/golden/dx/DX1.npz), the library exports eegnet_input_grad_eval and
its validation rejects what the kernel does not cover before any device call."""

from __future__ import annotations

import ctypes
import os

import pytest

from dx_cases import load_dx_fixture, oracle_dx
from golden_util import assert_close


def test_oracle_dx_matches_reference_fixture():
    z, meta, state, x, y = load_dx_fixture("DX1")
    assert (meta["C"], meta["T"], meta["B"]) == (22, 257, 2)
    dx, logits = oracle_dx(state, x, "ce", targets=y)
    assert_close(logits, z["logits"], name="DX1 logits")
    assert_close(dx, z["dx_ce"], name="DX1 dx (CE seed)")
    dx, logits = oracle_dx(state, x, "dlogits", dlogits=z["dlogits"])
    assert_close(logits, z["logits"], name="DX1 logits")
    assert_close(dx, z["dx_dlogits"], name="DX1 dx (dlogits seed)")
    # 22 x 257: the sample pool4 drops still gets a gradient through the temporal FIR
    assert abs(z["dx_ce"][:, :, 256]).max() > 0


def test_fixture_is_no_larger_than_the_largest_training_fixture():
    from dx_cases import DX_DIR
    from golden_util import GOLDEN_DIR, fixture_names
    assert "DX1" not in fixture_names()           # tests/golden/*.npz are training fixtures
    size = os.path.getsize(os.path.join(DX_DIR, "DX1.npz"))
    largest = max(os.path.getsize(os.path.join(GOLDEN_DIR, f)) for f in os.listdir(GOLDEN_DIR)
                  if f.endswith(".npz"))
    assert size <= largest


def _lib_or_skip():
    from eegnetreplication_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libeegnet_hip.so not built (run __graft_entry__.build())")
    return _lib, _lib.load()


def test_library_exports_input_grad_eval():
    _lib, lib = _lib_or_skip()
    assert "eegnet_input_grad_eval" in _lib.EXPORTED_SYMBOLS
    assert hasattr(lib, "eegnet_input_grad_eval")
    assert _lib.KERNEL_IDS[-1] == "k_infer_dx"


def _call(lib, d, kind=0, params=256, bn=256, x=256, dlogits=256, targets=256, dx=256, logits=256):
    p = lambda v: ctypes.c_void_p(v) if v else None      # never dereferenced: the call fails first
    return lib.eegnet_input_grad_eval(ctypes.byref(d), p(params), p(bn), p(x), kind, p(dlogits), p(targets),
                                      p(dx), p(logits), None)


def test_wide_dims_are_rejected_with_the_librarys_message():
    _lib, lib = _lib_or_skip()
    for C, T in ((64, 512), (22, 256)):
        assert _call(lib, _lib.dims(1, C, T, F1=16, D=4)) == -1
        assert lib.eegnet_last_error() == b"input gradients: F1*D = 64 > 16 is not supported"


def test_validation_without_a_gpu():
    _lib, lib = _lib_or_skip()
    d = _lib.dims(5, 22, 257)
    assert _call(lib, d, kind=3) == -1
    assert b"seed_kind" in lib.eegnet_last_error()
    assert _call(lib, d, kind=-1) == -1
    assert _call(lib, d, dx=0) == -1
    assert b"dx is NULL" in lib.eegnet_last_error()
    assert _call(lib, d, x=0) == -1
    assert _call(lib, d, params=0) == -1
    assert _call(lib, d, bn=0) == -1
    assert _call(lib, d, kind=2, targets=0) == -1
    assert b"targets" in lib.eegnet_last_error()
    assert _call(lib, d, kind=0, dlogits=0) == -1
    assert b"dlogits" in lib.eegnet_last_error()
    assert _call(lib, _lib.dims(5, 22, 257, x_pitch=260)) == -1
    assert b"x_pitch" in lib.eegnet_last_error()
    assert _call(lib, _lib.dims(5, 22, 256, K1=48)) == -1       # the geometry's own checks come first


def test_lds_budget_is_checked_with_the_bytes_named():
    """A narrow shape the eval forward takes, but whose x, s, ELU' and block-2 rows together do not fit
    one workgroup's LDS, is rejected with the bytes named, as the other paths do."""
    _lib, lib = _lib_or_skip()
    d = _lib.dims(2, 1, 1024)
    nb = ctypes.c_size_t()
    assert lib.eegnet_workspace_bytes(ctypes.byref(d), ctypes.byref(nb)) == 0
    assert _call(lib, d) == -1
    msg = lib.eegnet_last_error()
    assert msg.startswith(b"input gradients: dims need ") and b" B of LDS" in msg
