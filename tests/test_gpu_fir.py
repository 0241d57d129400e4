"""Zero-phase FIR filtering of continuous recordings on the GPU (eegnet_fir: k_fir, k_fir_hist) against the
float64 oracle ``fir_cases.oracle_fir``.

Tolerance of every comparison with the oracle: |gpu - oracle| <= 2^-23 |oracle| + 2 L 2^-53 sum|h| max|u|
(fir_cases.fir_bound): one fp32 ulp for the single final rounding, plus the fp64 dot-product error bound of L
terms for the kernel and for the oracle.  Everything else here is bit-equality: an output is a fixed function
of the taps and of its L input values, so a delta filter reproduces the shifted, reflected input exactly, a
slice gives the bits of its contiguous copy, and a stream's blocks laid end to end are the whole-recording
call."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from fir_cases import asymmetric_taps, assert_fir_close, delta_taps, extend, make_recording, oracle_fir

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 45]                      # 45 rows: not a multiple of anything the launch is shaped by
DTYPES = {"f32": np.float32, "f64": np.float64}
TAPS = ["L1", "L3", "design213", "asym213", "cap"]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _chunk():
    from eegnetreplication_amd import ops
    return ops.fir_chunk()


@functools.lru_cache(maxsize=None)
def _taps(kind):
    from eegnetreplication_amd import design_bandpass, ops
    h = {"L1": lambda: np.array([0.75]), "L3": lambda: np.array([0.5, -0.25, 0.125]),
         "design213": design_bandpass, "asym213": lambda: asymmetric_taps(213),
         "cap": lambda: asymmetric_taps(ops.fir_max_taps(), seed=11)}[kind]()
    h = np.ascontiguousarray(h, dtype=np.float64)
    h.setflags(write=False)
    return h


def _sizes(L):
    """N in {1, 2, M, M+1, L-1, L, L+1, chunk-1, chunk, chunk+1, 3 chunk + 5}, those that are >= 1, once each."""
    M, ch = (L - 1) // 2, _chunk()
    return sorted({n for n in (1, 2, M, M + 1, L - 1, L, L + 1, ch - 1, ch, ch + 1, 3 * ch + 5) if n >= 1})


@functools.lru_cache(maxsize=None)
def _case(rows, N, dtype, kind):
    """(input, oracle output), computed once per case and never written to."""
    x = make_recording(rows, N, 1000 * rows + N, DTYPES[dtype])
    y = oracle_fir(x, _taps(kind))
    for a in (x, y):
        a.setflags(write=False)
    return x, y


def _filt(x, h, **kw):
    from eegnetreplication_amd import bandpass_filter
    return bandpass_filter(x, h, **kw)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("kind", TAPS)
def test_parity_with_the_oracle(kind, rows, dtype):
    dev = _dev()
    h = _taps(kind)
    ht = torch.from_numpy(h).to(dev)
    for N in _sizes(len(h)):
        x, ref = _case(rows, N, dtype, kind)
        got = _filt(torch.tensor(x, device=dev), ht)
        assert got.dtype == torch.float32 and got.shape == (rows, N)
        assert_fir_close(got.cpu().numpy(), ref, x, h, name=f"{kind} {rows} x {N} {dtype}")


@pytest.mark.parametrize("L", [3, 213])
def test_delta_taps_reproduce_the_shifted_reflected_input_exactly(L):
    """h[j] = 1 alone: y[t] = u[t + M - j], a pure shift.  j = 0 advances by M (the tail's reflection shows),
    j = L - 1 delays by M (the head's), j = M is the identity.  N = 50 < M at L = 213: the reflection runs out
    and zeros follow.  fp32 input: 2 x[0] - x[j] is computed in fp64 and rounded once, as the expectation is."""
    dev = _dev()
    M = (L - 1) // 2
    for N in (1, 2, 50, _chunk() + 77):
        x = make_recording(3, N, 70 + N)
        u = extend(x, L)
        xt = torch.tensor(x, device=dev)
        for j in (0, M, L - 1):
            want = u[:, 2 * M - j:2 * M - j + N].astype(np.float32)
            got = _filt(xt, delta_taps(L, j)).cpu().numpy()
            assert np.array_equal(got, want), (L, N, j, np.abs(got - want).max())


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_a_time_slice_of_a_larger_buffer_and_a_pitched_output(dtype):
    """x is a time slice that starts at an odd element of a NaN-filled buffer: a load outside the slice would
    turn outputs into NaN.  y is a time slice of a poisoned buffer: nothing outside it is written, and the
    result carries the bits of the contiguous call."""
    from eegnetreplication_amd import ops
    dev = _dev()
    h = _taps("design213")
    ht = torch.from_numpy(h).to(dev)
    rows, N = 5, _chunk() + 77
    x, ref = _case(rows, N, dtype, "design213")
    tdt = torch.float32 if dtype == "f32" else torch.float64
    want = _filt(torch.tensor(x, device=dev), ht)
    for R, C in ((1, rows), (rows, 1)):
        buf = torch.full((R, C, N + 13), float("nan"), dtype=tdt, device=dev)
        view = buf[:, :, 3:3 + N]
        view.copy_(torch.tensor(x, device=dev).view(R, C, N))
        assert view.data_ptr() % (2 * view.element_size()) == view.element_size()      # an odd element
        ybuf = torch.full((R, C, N + 9), -12345.5, dtype=torch.float32, device=dev)
        out = ybuf[:, :, 5:5 + N]
        got = ops.fir(view, ht, out)
        assert got is out
        torch.cuda.synchronize()
        assert (ybuf[:, :, :5] == -12345.5).all() and (ybuf[:, :, 5 + N:] == -12345.5).all()
        assert torch.equal(out.reshape(rows, N), want)
        assert_fir_close(out.reshape(rows, N).cpu().numpy(), ref, x, h, name=f"slice {R}x{C} {dtype}")
        assert torch.isnan(buf[:, :, :3]).all() and torch.isnan(buf[:, :, 3 + N:]).all()


def test_filtering_in_place_is_refused():
    dev = _dev()
    ht = torch.from_numpy(_taps("L3")).to(dev)
    x = torch.zeros((4, 600), device=dev)
    with pytest.raises(ValueError, match="in place is not supported"):
        _filt(x, ht, out=x)
    buf = torch.zeros((4, 1000), device=dev)
    with pytest.raises(ValueError, match="in place is not supported"):
        _filt(buf[:, :600], ht, out=buf[:, 300:900])
    x64 = torch.zeros((4, 600), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="in place is not supported"):
        _filt(x64, ht, out=x64.view(torch.float32)[:, 600:])
    with pytest.raises(ValueError, match="odd number of taps"):
        _filt(x, torch.zeros(4, dtype=torch.float64, device=dev))
    from eegnetreplication_amd import ops
    with pytest.raises(RuntimeError, match="n_taps must be in"):
        _filt(x, torch.zeros(ops.fir_max_taps() + 2, dtype=torch.float64, device=dev))


@pytest.mark.parametrize("kind", ["L3", "design213", "asym213"])
def test_stream_blocks_equal_the_whole_recording_bit_for_bit(kind):
    """Blocks of L, 1, 7, L-2 (shorter than the history: the new history is part old, part block), chunk + 3,
    1, 2 chunk + 1 and 5 samples, then flush(): the first push returns n - M samples, the others n, the flush
    the last M, and laid end to end they are the whole-recording call.  The same for [R, C, n] blocks."""
    from eegnetreplication_amd import StreamBandpass
    dev = _dev()
    h = _taps(kind)
    L, ch = len(h), _chunk()
    M = (L - 1) // 2
    blocks = [L, 1, 7, max(L - 2, 1), ch + 3, 1, 2 * ch + 1, 5]
    rows, N = 6, sum(blocks)
    x, ref = _case(rows, N, "f32", kind)
    xt = torch.tensor(x, device=dev)
    whole = _filt(xt, h)
    assert_fir_close(whole.cpu().numpy(), ref, x, h, name=f"whole {kind}")
    for lead, view in (((rows,), xt), ((2, 3), xt.view(2, 3, N))):
        s = StreamBandpass(lead if len(lead) > 1 else rows, h)
        parts, t = [], 0
        for i, n in enumerate(blocks):
            y = s.push(view[..., t:t + n])                           # a time slice, as it lies
            assert y.shape[-1] == (n - M if i == 0 else n) and y.dtype == torch.float32
            parts.append(y)
            t += n
        parts.append(s.flush())
        assert parts[-1].shape[-1] == M
        got = torch.cat(parts, dim=-1)
        assert got.shape == view.shape
        assert torch.equal(got.reshape(rows, N), whole), kind
        with pytest.raises(RuntimeError, match="flushed"):
            s.push(view[..., :5])
        s.reset()
        one = torch.cat([s.push(view), s.flush()], dim=-1)           # one block and the flush
        assert torch.equal(one.reshape(rows, N), whole)


def test_fp64_blocks_and_the_oracle():
    """An fp64 recording streamed in two blocks: the history carries its samples exactly."""
    from eegnetreplication_amd import StreamBandpass
    dev = _dev()
    h = _taps("asym213")
    rows, N = 3, 213 + 400
    x, ref = _case(rows, N, "f64", "asym213")
    xt = torch.tensor(x, device=dev)
    s = StreamBandpass(rows, h)
    got = torch.cat([s.push(xt[:, :213]), s.push(xt[:, 213:]), s.flush()], dim=1)
    assert torch.equal(got, _filt(xt, h))
    assert_fir_close(got.cpu().numpy(), ref, x, h, name="fp64 stream")


def test_two_calls_give_the_same_bits_and_recordings_do_not_mix():
    dev = _dev()
    h = torch.from_numpy(_taps("design213")).to(dev)
    N = 3 * _chunk() + 5
    x, _ = _case(45, N, "f32", "design213")
    xt = torch.tensor(x, device=dev)
    a = _filt(xt, h)
    assert torch.equal(a, _filt(xt, h))
    x3 = xt.view(5, 9, N)                                            # R = 5 recordings of 9 rows
    y3 = _filt(x3, h)
    assert y3.shape == (5, 9, N) and torch.equal(y3.view(45, N), a)
    for r in range(5):
        assert torch.equal(_filt(x3[r], h), y3[r])


def test_graph_capture_of_filter_and_standardisation():
    """One capture of bandpass_filter on device taps followed by the standardisation; the replay, on a
    recording changed in place since the capture, equals the eager calls bit for bit."""
    from eegnetreplication_amd import exponential_moving_standardize, preprocess_recording
    dev = _dev()
    h = torch.from_numpy(_taps("design213")).to(dev)
    C, N = 22, _chunk() + 900
    rec = torch.from_numpy(make_recording(C, N, 61)).to(dev)

    def run():
        y = _filt(rec, h)
        return y, exponential_moving_standardize(y)

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
    assert torch.isfinite(want[1]).all()
    assert torch.equal(preprocess_recording(rec, h), want[1])        # the composition is these two calls
