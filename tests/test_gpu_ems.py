"""Exponential moving standardisation of continuous recordings on the GPU (eegnet_ems: k_ems_agg,
k_ems_carry, k_ems_out) against the serial float64 oracle ``ems_cases.oracle_ems``.

Tolerance everywhere: |gpu - oracle| <= 2^-23 |oracle| + 1e-9.  The kernels compute in fp64 and round to
fp32 once: the first term is one fp32 ulp, for a flip at that rounding's boundary; the second bounds the
fp64 reassociation error of the blocked scan, 50 times the 2e-11 below which the numpy restatement of the
blocked algorithm stays on these inputs (test_ems_cpu.py measures 6.1e-12 at N = 2 and 5.3e-13 from
N = 999 on).  The final state is compared to 1e-11 relative (the restatement: 6.2e-14 on the state test's
recording, 5.1e-13 at worst over the 45-row cases)."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from ems_cases import (EMS1, assert_ems_close, assert_state_close, ems1_input, make_recording, oracle_ems)

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 45]                      # 45 rows: not a multiple of anything the launch is shaped by
DTYPES = {"f32": np.float32, "f64": np.float64}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _L():
    from eegnetreplication_amd import ops
    return ops.ems_chunk()


def _sizes():
    L = _L()
    return [1, 2, 999, 1000, 1001, L - 1, L, L + 1, 3 * L + 5]


@functools.lru_cache(maxsize=None)
def _case(rows, N, dtype, factor_new=1e-3):
    """(input, oracle output, oracle final state), computed once per case and never written to."""
    x = make_recording(rows, N, 1000 * rows + N, DTYPES[dtype])
    y, s = oracle_ems(x, factor_new)
    for a in (x, y, s):
        a.setflags(write=False)
    return x, y, s


def _ems(x, **kw):
    from eegnetreplication_amd import exponential_moving_standardize
    return exponential_moving_standardize(x, **kw)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("ni", range(9), ids=["N1", "N2", "N999", "N1000", "N1001", "L-1", "L", "L+1", "3L+5"])
def test_parity_with_the_oracle(ni, rows):
    dev = _dev()
    N = _sizes()[ni]
    for dtype in DTYPES:
        x, ref, _ = _case(rows, N, dtype)
        got = _ems(torch.tensor(x, device=dev))
        assert got.dtype == torch.float32 and got.shape == (rows, N)
        assert_ems_close(got.cpu().numpy(), ref, name=f"{rows} x {N} {dtype}")


@pytest.mark.parametrize("rows", ROWS)
def test_a_fast_factor_makes_a_wrong_carry_power_loud(rows):
    """factor_new = 0.1 at 3L + 5 samples: p^k falls off within a few dozen samples, so a carry entering a
    chunk one power off moves the chunk's first outputs by a tenth of their size."""
    dev = _dev()
    N = 3 * _L() + 5
    for dtype in DTYPES:
        x, ref, _ = _case(rows, N, dtype, 0.1)
        got = _ems(torch.tensor(x, device=dev), factor_new=0.1)
        assert_ems_close(got.cpu().numpy(), ref, name=f"{rows} x {N} {dtype} a=0.1")


def test_the_reference_fixture():
    """The fixture the reference's own function wrote (3 x 2600 float64, two rows on DC offsets)."""
    dev = _dev()
    want = np.load(EMS1)["y"]
    got = _ems(torch.from_numpy(ems1_input()).to(dev))
    assert_ems_close(got.cpu().numpy(), want, name="EMS1")
    x3 = torch.from_numpy(ems1_input()).to(dev).view(1, 3, -1).expand(2, 3, -1).contiguous()      # [R, C, N]
    got3 = _ems(x3)
    assert got3.shape == (2, 3, 2600) and torch.equal(got3[0], got) and torch.equal(got3[1], got)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_a_time_slice_of_a_larger_buffer_and_a_pitched_output(dtype):
    """x is a time slice that starts at an odd element of a NaN-filled buffer: a load outside the slice
    would turn outputs into NaN.  y is a time slice of a poisoned buffer: nothing outside it is written."""
    from eegnetreplication_amd import ops
    dev = _dev()
    rows, N = 5, _L() + 77
    x, ref, _ = _case(rows, N, dtype)
    tdt = torch.float32 if dtype == "f32" else torch.float64
    for R, C in ((1, rows), (rows, 1)):
        buf = torch.full((R, C, N + 13), float("nan"), dtype=tdt, device=dev)
        view = buf[:, :, 3:3 + N]
        view.copy_(torch.tensor(x, device=dev).view(R, C, N))
        assert not view.is_contiguous() or R * C == 1
        assert view.data_ptr() % (2 * view.element_size()) == view.element_size()      # an odd element
        ybuf = torch.full((R, C, N + 9), -12345.5, dtype=torch.float32, device=dev)
        out = ybuf[:, :, 5:5 + N]
        got = ops.ems(view, out)
        assert got is out
        torch.cuda.synchronize()
        assert (ybuf[:, :, :5] == -12345.5).all() and (ybuf[:, :, 5 + N:] == -12345.5).all()
        assert_ems_close(out.reshape(rows, N).cpu().numpy(), ref, name=f"slice {R}x{C} {dtype}")
        assert torch.equal(out.reshape(rows, N), _ems(torch.tensor(x, device=dev)))
        assert torch.isnan(buf[:, :, :3]).all() and torch.isnan(buf[:, :, 3 + N:]).all()


def test_in_place_equals_out_of_place_bit_for_bit():
    dev = _dev()
    rows, N = 7, 2 * _L() + 301
    x, _, _ = _case(rows, N, "f32")
    xt = torch.tensor(x, device=dev)
    want = _ems(xt)
    a = xt.clone()
    assert _ems(a, out=a) is a
    assert torch.equal(a, want)
    buf = torch.full((rows, N + 6), float("nan"), dtype=torch.float32, device=dev)     # in place in a slice
    view = buf[:, 1:1 + N]
    view.copy_(xt)
    _ems(view, out=view)
    assert torch.equal(view, want)
    assert torch.isnan(buf[:, :1]).all() and torch.isnan(buf[:, 1 + N:]).all()
    from eegnetreplication_amd import ops
    x64 = xt.double().view(1, rows, N)
    with pytest.raises(RuntimeError, match="fp32 input only"):
        ops.ems(x64, x64.view(torch.float32)[:, :, :N])              # the same pointer, fp64 input


def test_stream_standardizer_carries_the_state():
    """1007 + 3L samples pushed as 1007, 1, 333 and the rest: the first block holds the 1000 samples the
    whole-recording call starts from, so the concatenation is that call's output."""
    from eegnetreplication_amd import StreamStandardizer
    dev = _dev()
    rows, N = 3, 1007 + 3 * _L()
    x, ref, ref_state = _case(rows, N, "f32")
    xt = torch.tensor(x, device=dev)
    s = StreamStandardizer(rows)
    parts, t = [], 0
    for n in (1007, 1, 333, N - 1341):
        parts.append(s.push(xt[:, t:t + n]))                        # a time slice, as it lies
        t += n
        assert s.state.dtype == torch.float64 and s.state.shape == (rows, 2)
    assert t == N
    assert_ems_close(torch.cat(parts, dim=1).cpu().numpy(), ref, name="stream")
    assert_state_close(s.state.cpu().numpy(), ref_state, name="stream")
    whole = _ems(xt)
    assert_ems_close(whole.cpu().numpy(), ref, name="whole")
    s.reset()
    assert s.state is None
    assert torch.equal(s.push(xt), whole)                           # one block: the whole-recording call
    assert_state_close(s.state.cpu().numpy(), ref_state, name="one block")
    s2 = StreamStandardizer((1, rows))                              # [R, C, n] blocks
    assert torch.equal(s2.push(xt.view(1, rows, N)), whole.view(1, rows, N))


def test_two_calls_give_the_same_bits():
    dev = _dev()
    x, _, _ = _case(45, 3 * _L() + 5, "f32")
    xt = torch.tensor(x, device=dev)
    assert torch.equal(_ems(xt), _ems(xt))


def test_graph_capture_with_sliding_logits_on_a_slice():
    """One capture of the standardisation followed by sliding_logits on a time slice of its output; the
    replay, on a recording changed in place since the capture, equals the eager calls bit for bit, and the
    slice read in place gives the logits of its contiguous copy."""
    from eegnetreplication_amd import sliding_logits
    from hip_cases import random_model
    dev = _dev()
    C, T, hop = 22, 256, 16
    m = random_model(C, T, seed=3).to(dev).eval()
    N = _L() + 900
    a, b = 300, 300 + T + 40 * hop + 3
    rec = torch.from_numpy(make_recording(C, N, 61)).to(dev)

    def run():
        y = _ems(rec)
        return y, sliding_logits(m, y[:, a:b], hop)

    run()                                                            # eager once: code objects loaded
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    rec.copy_(torch.from_numpy(make_recording(C, N, 62)).to(dev))
    g.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in out]
    want = run()
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    assert torch.isfinite(want[1]).all() and want[1].shape == (41, 4)
    assert torch.equal(want[1], sliding_logits(m, want[0][:, a:b].contiguous(), hop))
