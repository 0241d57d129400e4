"""Host side of sliding-window inference (eegnet_window_count, eegnet_forward_eval_windows): the window
count, every rejection with its message, and ``window_starts``.  The validation precedes every device
call, so nothing here needs a GPU; the pointers handed in are never dereferenced."""

from __future__ import annotations

import ctypes

import pytest
import torch


def _lib():
    from eegnetreplication_amd import _lib
    return _lib, _lib.load()


def _count(lib, d, n, hop):
    out = ctypes.c_int64(-1)
    rc = lib.eegnet_window_count(ctypes.byref(d) if d is not None else None, n, hop, ctypes.byref(out))
    return rc, int(out.value), lib.eegnet_last_error().decode()


@pytest.mark.parametrize("T", [256, 257, 96])
def test_window_count_matches_the_definition(T):
    lib_mod, lib = _lib()
    d = lib_mod.dims(7, 22, T)           # B is ignored
    for n, hop in [(T, 1), (T, T), (T, T + 5), (T + 300, 1), (T + 300, 3), (T + 300, 4), (T + 300, 32),
                   (3 * T, T), (3 * T - 1, T), (3 * T + 7, T), (4 * T, T + 5), (T + 4, T + 5), (76800, 8)]:
        rc, W, msg = _count(lib, d, n, hop)
        assert rc == 0, msg
        assert W == (n - T) // hop + 1, (n, hop)
    # the wide dims have windows too: the count is geometry alone
    rc, W, msg = _count(lib, lib_mod.dims(1, 64, 512, F1=16, D=4), 1024, 128)
    assert rc == 0 and W == 5, msg


def test_window_count_rejections():
    lib_mod, lib = _lib()
    d = lib_mod.dims(1, 22, 256)
    rc, _, msg = _count(lib, None, 512, 1)
    assert rc == -1 and "dims is NULL" in msg
    assert lib.eegnet_window_count(ctypes.byref(d), 512, 1, None) == -1
    assert "out is NULL" in lib.eegnet_last_error().decode()
    for hop in (0, -3):
        rc, _, msg = _count(lib, d, 512, hop)
        assert rc == -1 and f"hop must be >= 1 (got {hop})" in msg
    rc, _, msg = _count(lib, d, 255, 1)
    assert rc == -1 and "n_samples = 255 is shorter than one window (T = 256)" in msg
    rc, _, msg = _count(lib, lib_mod.dims(1, 22, 256, K1=48), 512, 1)
    assert rc == -1 and "K1" in msg


def _call(lib, d, *, params=256, bn=256, rec=256, n_rec=1, n=512, pitch=None, hop=8, logits=256, probs=None,
          pred=None):
    """eegnet_forward_eval_windows with dummy non-NULL pointers (every call here fails before a launch)."""
    vp = lambda v: None if v is None else ctypes.c_void_p(v)
    rc = lib.eegnet_forward_eval_windows(ctypes.byref(d) if d is not None else None, vp(params), vp(bn), vp(rec),
                                         n_rec, n, n if pitch is None else pitch, hop, vp(logits), vp(probs),
                                         vp(pred), None)
    return rc, lib.eegnet_last_error().decode()


def test_forward_eval_windows_rejections():
    lib_mod, lib = _lib()
    d = lib_mod.dims(1, 22, 256)
    assert _call(lib, None) == (-1, "dims is NULL")
    for name, kw in [("params", dict(params=None)), ("bn_buffers", dict(bn=None)), ("rec", dict(rec=None)),
                     ("logits", dict(logits=None))]:
        assert _call(lib, d, **kw) == (-1, f"{name} is NULL"), name
    rc, msg = _call(lib, d, hop=0)
    assert rc == -1 and "hop must be >= 1 (got 0)" in msg
    rc, msg = _call(lib, d, n_rec=0)
    assert rc == -1 and "n_rec must be >= 1 (got 0)" in msg
    rc, msg = _call(lib, d, n=255)
    assert rc == -1 and "n_samples = 255 is shorter than one window (T = 256)" in msg
    rc, msg = _call(lib, d, n=512, pitch=511)
    assert rc == -1 and "pitch = 511 is below n_samples = 512" in msg
    rc, msg = _call(lib, lib_mod.dims(1, 22, 257, x_pitch=260))
    assert rc == -1 and "x_pitch must be 0 or T" in msg
    rc, msg = _call(lib, lib_mod.dims(1, 22, 256, x_pitch=256), hop=0)      # x_pitch = T passes that check
    assert rc == -1 and "hop must be" in msg


def test_forward_eval_windows_rejects_a_total_the_eval_forward_does_not_take():
    """n_rec * W is the batch of the eval forward: one above its limit (B * F2 * (T/4) < 2^32, so
    B < 2^22 at 22 x 256) is refused with the count, as eegnet_forward_eval refuses that B."""
    lib_mod, lib = _lib()
    d = lib_mod.dims(1, 22, 256)
    B = (1 << 32) // (16 * 64)                        # the first batch the eval forward refuses
    dB = lib_mod.dims(B, 22, 256)
    assert lib.eegnet_forward_eval(ctypes.byref(dB), ctypes.c_void_p(256), ctypes.c_void_p(256), None,
                                   ctypes.c_void_p(256), None) == -1
    assert "2^32" in lib.eegnet_last_error().decode()          # (refused on the dims, before the NULL x)
    rc, msg = _call(lib, d, n_rec=1, n=256 + B - 1, hop=1)
    assert rc == -1 and f"n_rec * W = {B} windows" in msg and "2^32" in msg
    rc, msg = _call(lib, d, n_rec=B, n=256, hop=1)
    assert rc == -1 and f"n_rec * W = {B} windows" in msg
    rc, msg = _call(lib, d, n_rec=1 << 40, n=1 << 30, hop=1)   # far beyond an int
    assert rc == -1 and "windows exceed the batch" in msg


def test_wide_dims_are_rejected_with_the_documented_message():
    lib_mod, lib = _lib()
    rc, msg = _call(lib, lib_mod.dims(1, 64, 512, F1=16, D=4), n=1024, hop=64)
    assert rc == -1
    assert msg == "sliding windows: F1*D = 64 > 16 is not supported"
    rc, msg = _call(lib, lib_mod.dims(1, 10, 128, F1=12, D=4), n=1024, hop=64)
    assert rc == -1 and msg == "sliding windows: F1*D = 48 > 16 is not supported"


def test_window_starts():
    from eegnetreplication_amd import window_starts
    from eegnetreplication_amd.ops import Shape, window_count
    for N, T, hop in [(256, 256, 1), (556, 256, 1), (556, 256, 3), (556, 256, 256), (1000, 257, 262),
                      (300, 96, 32), (260, 256, 261)]:
        s = window_starts(N, T, hop)
        assert s.dtype == torch.int64
        assert s.tolist() == list(range(0, N - T + 1, hop))
        assert len(s) == (N - T) // hop + 1 == window_count(Shape(C=22, T=T), N, hop)
        assert int(s[-1]) + T <= N
    with pytest.raises(ValueError, match="hop"):
        window_starts(512, 256, 0)
    with pytest.raises(ValueError, match="shorter"):
        window_starts(255, 256, 1)


def test_cpu_tensors_are_refused():
    from eegnetreplication_amd import EEGNet, cropped_predict, sliding_logits
    m = EEGNet(22, 256)
    rec = torch.zeros(22, 512)
    with pytest.raises(RuntimeError, match="HIP device"):
        sliding_logits(m, rec, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        cropped_predict(m, rec, 8)
