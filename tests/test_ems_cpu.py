"""Host side of the exponential moving standardisation (eegnet_ems, eegnet_ems_chunk,
eegnet_ems_scratch_bytes, ``exponential_moving_standardize``, ``StreamStandardizer``): the oracle against
the reference-generated fixture, the error of the blocked algorithm against the oracle, the geometry calls
and every rejection with its message.  The validation precedes every device call, so nothing here needs a
GPU; the pointers handed in are never dereferenced."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from ems_cases import EMS1, blocked_ems, ems1_input, make_recording, oracle_ems


def _lib():
    from eegnetreplication_amd import _lib
    return _lib.load()


def test_oracle_reproduces_the_reference_fixture_bit_for_bit():
    want = np.load(EMS1)["y"]
    x = ems1_input()
    got, state = oracle_ems(x)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape == (3, 2600)
    assert np.array_equal(got, want)
    assert state.shape == (3, 2) and abs(state[1, 0] - 100.0) < 1.0 and (state[:, 1] > 0).all()
    # the state is the recurrence's: a second half started from the first half's state continues it
    a, sa = oracle_ems(x[:, :1300])
    b, sb = oracle_ems(x[:, 1300:], state=sa)
    assert np.array_equal(np.concatenate([a, b], axis=1), want) and np.array_equal(sb, state)


def test_chunk_and_scratch_bytes():
    lib = _lib()
    L = lib.eegnet_ems_chunk()
    assert L >= 64
    from eegnetreplication_amd import ops
    assert ops.ems_chunk() == L

    def nbytes(rows, n):
        out = ctypes.c_size_t(0)
        assert lib.eegnet_ems_scratch_bytes(rows, n, ctypes.byref(out)) == 0, lib.eegnet_last_error().decode()
        return int(out.value)

    sizes = [1, 2, L - 1, L, L + 1, 3 * L + 5, 76800, 345600]
    for rows in (1, 3, 22, 45, 396):
        got = [nbytes(rows, n) for n in sizes]
        assert got[0] > 0 and got == sorted(got), (rows, got)
        assert nbytes(rows, L + 1) > nbytes(rows, L)                 # one more chunk
    for n in sizes:
        got = [nbytes(rows, n) for rows in (1, 2, 3, 22, 45, 396)]
        assert got == sorted(got) and len(set(got)) == len(got), (n, got)
    assert lib.eegnet_ems_scratch_bytes(3, 100, None) == -1
    assert "out is NULL" in lib.eegnet_last_error().decode()
    out = ctypes.c_size_t(0)
    for rows, n, msg in [(0, 100, "n_rows must be >= 1 (got 0)"), (3, 0, "n_samples must be >= 1 (got 0)"),
                         (1 << 31, L + 1, "exceed the grid limit of 2147483647 workgroups")]:
        assert lib.eegnet_ems_scratch_bytes(rows, n, ctypes.byref(out)) == -1
        assert msg in lib.eegnet_last_error().decode()


def _call(lib, *, x=256, f64=0, rows=3, n=512, x_pitch=None, y=1024, y_pitch=None, factor_new=1e-3, init_block=1000,
          eps=1e-10, state=None, resume=0, scratch=4096):
    """eegnet_ems with dummy non-NULL pointers (every call here fails before a launch)."""
    vp = lambda v: None if v is None else ctypes.c_void_p(v)
    rc = lib.eegnet_ems(vp(x), f64, rows, n, n if x_pitch is None else x_pitch, vp(y), n if y_pitch is None else y_pitch,
                        factor_new, init_block, eps, vp(state), resume, vp(scratch), None)
    return rc, lib.eegnet_last_error().decode()


def test_ems_rejections():
    lib = _lib()
    L = lib.eegnet_ems_chunk()
    for name, kw in [("x", dict(x=None)), ("y", dict(y=None)), ("scratch", dict(scratch=None))]:
        assert _call(lib, **kw) == (-1, f"{name} is NULL"), name
    cases = [
        (dict(rows=0), "eegnet_ems: n_rows must be >= 1 (got 0)"),
        (dict(rows=-2), "eegnet_ems: n_rows must be >= 1 (got -2)"),
        (dict(n=0), "eegnet_ems: n_samples must be >= 1 (got 0)"),
        (dict(n=512, x_pitch=511), "eegnet_ems: x_pitch = 511 is below n_samples = 512"),
        (dict(n=512, y_pitch=511), "eegnet_ems: y_pitch = 511 is below n_samples = 512"),
        (dict(factor_new=0.0), "eegnet_ems: factor_new must lie in (0, 1) (got 0)"),
        (dict(factor_new=1.0), "eegnet_ems: factor_new must lie in (0, 1) (got 1)"),
        (dict(factor_new=-0.5), "eegnet_ems: factor_new must lie in (0, 1) (got -0.5)"),
        (dict(factor_new=float("nan")), "eegnet_ems: factor_new must lie in (0, 1) (got nan)"),
        (dict(eps=-1e-10), "eegnet_ems: eps must be >= 0 (got -1e-10)"),
        (dict(init_block=0), "eegnet_ems: init_block must be >= 1 (got 0)"),
        (dict(resume=1), "eegnet_ems: resume needs state"),
        (dict(x=1024, y=1024, f64=1), "eegnet_ems: y may be x for fp32 input only"),
        (dict(x=1024, y=1024, x_pitch=520, y_pitch=512), "eegnet_ems: y is x but y_pitch = 512 is not x_pitch = 520"),
        (dict(x=258), "eegnet_ems: x, y, state and scratch must be aligned to their element size"),
        (dict(x=260, f64=1), "eegnet_ems: x, y, state and scratch must be aligned to their element size"),
    ]
    for kw, msg in cases:
        assert _call(lib, **kw) == (-1, msg), kw
    # the grid: n_rows * chunks workgroups, the limit named
    rc, msg = _call(lib, rows=1 << 31, n=L + 1, x_pitch=L + 1, y_pitch=L + 1)
    assert rc == -1 and "2 chunks" in msg and "exceed the grid limit of 2147483647 workgroups" in msg
    rc, msg = _call(lib, rows=3, n=1 << 62, x_pitch=1 << 62, y_pitch=1 << 62)
    assert rc == -1 and "exceed the grid limit of 2147483647 workgroups" in msg
    # resuming does not look at init_block
    rc, msg = _call(lib, resume=1, init_block=0, state=None)
    assert rc == -1 and msg == "eegnet_ems: resume needs state"


def test_python_refuses_cpu_tensors_wrong_ranks_and_dtypes():
    from eegnetreplication_amd import StreamStandardizer, exponential_moving_standardize
    with pytest.raises(RuntimeError, match="HIP device"):
        exponential_moving_standardize(torch.zeros(22, 512))
    with pytest.raises(RuntimeError, match="HIP device"):
        StreamStandardizer(22).push(torch.zeros(22, 512))
    with pytest.raises(RuntimeError, match="expected a block"):
        StreamStandardizer((2, 22)).push(torch.zeros(22, 512))
    with pytest.raises(ValueError, match="leading shape"):
        StreamStandardizer((2, 3, 4))
    s = StreamStandardizer(22)
    assert s.state is None
    s.reset()
    assert s.state is None
    # the rank is looked at first: no device needed to refuse it
    for shape in ((512,), (2, 3, 22, 512)):
        with pytest.raises(RuntimeError, match="expected a recording"):
            exponential_moving_standardize(torch.zeros(shape))
    with pytest.raises(ValueError, match="out must have the recording's shape"):
        exponential_moving_standardize(torch.zeros(22, 512), out=torch.zeros(22, 511))


def test_blocked_algorithm_against_the_oracle():
    """The reassociation error of the blocked form (chunk aggregates from a zero start, the three-term split
    of the variance scan, carries, output from the true carries) against the serial oracle, on the inputs
    of the GPU tests (the 45-row ones, same seeds): it must stay below the 2e-11 from which the GPU tests'
    1e-9 keeps a factor 50.  Measured: 6.1e-12 in y at N = 2, where the variance is still of eps's size and
    the rounding of the oracle's own mean of an offset row (a value of 100) is divided by 1e-5; 5.3e-13 from
    N = 999 on; 5.1e-13 relative in the final state (6.2e-14 on the three rows the GPU's state test uses).
    Most of it is the oracle's own rounding: it carries a mean of 100 through every step, the blocked form
    works on x less the chunk's first sample."""
    L = _lib().eegnet_ems_chunk()
    worst_y = worst_s = 0.0
    for rows, N, fn, dt in [(45, 1, 1e-3, np.float32), (45, 2, 1e-3, np.float32), (45, 2, 1e-3, np.float64),
                            (45, 999, 1e-3, np.float64), (45, 1001, 1e-3, np.float32),
                            (45, L - 1, 1e-3, np.float32), (45, L + 1, 1e-3, np.float64),
                            (45, 3 * L + 5, 1e-3, np.float64), (45, 3 * L + 5, 0.1, np.float32),
                            (3, 1007 + 3 * L, 1e-3, np.float32)]:
        x = make_recording(rows, N, 1000 * rows + N, dt)
        yo, so = oracle_ems(x, fn)
        yb, sb = blocked_ems(x, L, fn)
        worst_y = max(worst_y, float(np.abs(yo - yb).max()))
        if N > 2:                                         # (one or two samples leave a variance of ~0)
            worst_s = max(worst_s, float((np.abs(so - sb) / np.abs(so)).max()))
    yb, _ = blocked_ems(ems1_input(), L)
    worst_y = max(worst_y, float(np.abs(yb - np.load(EMS1)["y"]).max()))
    print(f"blocked vs oracle: max |dy| {worst_y:.3e}, max relative state error {worst_s:.3e}")
    assert worst_y <= 2e-11
    assert worst_s <= 1e-11                                # the bound the GPU's final state is held to
