"""Rational polyphase resampling of continuous recordings on the GPU (eegnet_resample: k_resample,
k_resample_hist) against the float64 oracle ``resample_cases.oracle_resample``.

Tolerance of every comparison with the oracle:
|gpu - oracle| <= 2^-23 |oracle| + 2 K 2^-53 max_p sum_j |h[p + j up]| max|u|  (resample_cases.resample_bound): one
fp32 ulp for the single final rounding, plus the fp64 dot-product error bound of K terms for the kernel and for
the oracle.  Everything else here is bit-equality: an output is a fixed function of the taps and of the values of u
in its support, so a delta prototype reproduces the decimated, shifted, extended input exactly, a slice gives
the bits of its contiguous copy, and a stream's blocks laid end to end are the whole-recording call."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from resample_cases import (asymmetric_taps, assert_resample_close, delta_taps, extend, geometry, make_recording,
                            oracle_resample, out_length)

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 45]                      # 45 rows: not a multiple of anything the launch is shaped by
DTYPES = {"f32": np.float32, "f64": np.float64}
ENDS = ["reflect_limited", "zero"]
# name -> (up, down, taps): the default design (None), asymmetric random taps (a sum run the wrong way round
# shows), the longest prototype the kernel takes, and a prototype of one tap
KINDS = {"64/125": (64, 125, None), "2/5": (2, 5, None), "3/2": (3, 2, None), "1/3": (1, 3, None), "1/2": (1, 2, None),
         "64/125 asym2501": (64, 125, 2501), "64/125 asymcap": (64, 125, "cap"), "3/2 one tap": (3, 2, 1)}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _kind(kind):
    """(up, down, taps) of a kind, the taps read-only."""
    from eegnetreplication_amd import design_resampler, ops
    up, down, spec = KINDS[kind]
    if spec is None:
        h = design_resampler(up, down)
    elif spec == 1:
        h = np.array([0.75])
    else:
        h = asymmetric_taps(ops.resample_max_taps() if spec == "cap" else spec, up, seed=11)
    h = np.ascontiguousarray(h, dtype=np.float64)
    h.setflags(write=False)
    return up, down, h


def _chunk_inputs(kind, outputs=None):
    """The inputs that give ``outputs`` outputs (default: one chunk's), rounded down."""
    from eegnetreplication_amd import ops
    up, down, h = _kind(kind)
    ch = ops.resample_chunk(len(h), up, down)
    return (ch if outputs is None else outputs(ch)) * down // up


def _sizes(kind):
    """N in {1, 2, Q+1, Q+2, Q+3, down, down+1, a chunk's inputs -1 / +0 / +1, three chunks' + 5}, once each."""
    up, down, h = _kind(kind)
    Q = geometry(len(h), up, down)[3]
    c1, c3 = _chunk_inputs(kind), _chunk_inputs(kind, lambda ch: 3 * ch + 5)
    return sorted({n for n in (1, 2, Q + 1, Q + 2, Q + 3, down, down + 1, c1 - 1, c1, c1 + 1, c3) if n >= 1})


@functools.lru_cache(maxsize=48)
def _case(N, dtype, kind, ends):
    """(input [45, N], oracle output), computed once per case and never written to; the tests on fewer rows take
    the first rows of both."""
    up, down, h = _kind(kind)
    x = make_recording(45, N, 1000 + N, DTYPES[dtype])
    y = oracle_resample(x, h, up, down, ends)
    for a in (x, y):
        a.setflags(write=False)
    return x, y


def _rs(x, kind, ends="reflect_limited", taps=None, **kw):
    from eegnetreplication_amd import resample
    up, down, h = _kind(kind)
    return resample(x, up, down, h if taps is None else taps, ends, **kw)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("ends", ENDS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_parity_with_the_oracle(kind, ends, dtype):
    dev = _dev()
    up, down, h = _kind(kind)
    ht = torch.from_numpy(h).to(dev)
    for N in _sizes(kind):
        x, ref = _case(N, dtype, kind, ends)
        for rows in ROWS:
            got = _rs(torch.tensor(x[:rows], device=dev), kind, ends, ht)
            assert got.dtype == torch.float32 and got.shape == (rows, out_length(N, up, down))
            assert_resample_close(got.cpu().numpy(), ref[:rows], x[:rows], h, up, down, ends,
                                  name=f"{kind} {ends} {rows} x {N} {dtype}")


@pytest.mark.parametrize("ends", ENDS)
@pytest.mark.parametrize("ratio", [(64, 125), (3, 2), (1, 3)])
def test_a_delta_prototype_is_a_decimated_shift_exactly(ratio, ends):
    """h[half + s] = up alone: y[m] = up u[(m down - s) / up] where the division is exact, else 0 -- the extended
    input shifted by s / up samples, decimated, nothing added to it.  s < 0 reaches past the tail, s > 0 past the
    head; N = 30 is shorter than the reflection at 64/125 (Q + 1 = 33 with these 4097 taps), so zeros follow it."""
    from eegnetreplication_amd import resample
    dev = _dev()
    up, down = ratio
    L = 4097 if up == 64 else 61
    half = (L - 1) // 2
    for N in (1, 2, 30, _chunk_inputs("64/125") + 77):
        x = make_recording(3, N, 70 + N)
        u, pad = extend(x, L, up, ends)
        xt = torch.tensor(x, device=dev)
        m = np.arange(out_length(N, up, down))
        for s in (0, half, -half, 5 * up, -7 * up + (1 if up > 1 else 0)):
            hit = (m * down - s) % up == 0
            n = (m * down - s) // up
            want = np.where(hit[None, :], float(up) * u[:, np.where(hit, pad + n, 0)], 0.0).astype(np.float32)
            got = resample(xt, up, down, delta_taps(L, half + s, float(up)), ends).cpu().numpy()
            assert np.array_equal(got, want), (ratio, ends, N, s, np.abs(got - want).max())


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_a_time_slice_of_a_larger_buffer_and_a_pitched_output(dtype):
    """x is a time slice that starts at an odd element of a NaN-filled buffer, at a pitch above N: a load outside
    the slice would turn outputs into NaN.  y is a time slice of a canary-filled buffer: no byte outside a row's
    outputs is written, and the result carries the bits of the contiguous call, of the ``out=`` call included."""
    from eegnetreplication_amd import ops, resample
    dev = _dev()
    kind, ends = "64/125", "reflect_limited"
    up, down, h = _kind(kind)
    ht = torch.from_numpy(h).to(dev)
    rows, N = 45, _chunk_inputs(kind) + 1
    x, ref = _case(N, dtype, kind, ends)
    n_out = ref.shape[1]
    tdt = torch.float32 if dtype == "f32" else torch.float64
    want = _rs(torch.tensor(x, device=dev), kind, ends, ht)
    for R, C in ((1, rows), (5, 9)):
        buf = torch.full((R, C, N + 13), float("nan"), dtype=tdt, device=dev)
        view = buf[:, :, 3:3 + N]
        view.copy_(torch.tensor(x, device=dev).view(R, C, N))
        assert view.data_ptr() % (2 * view.element_size()) == view.element_size()      # an odd element
        ybuf = torch.full((R, C, n_out + 9), -12345.5, dtype=torch.float32, device=dev)
        out = ybuf[:, :, 5:5 + n_out]
        got = ops.resample(view, ht, up, down, out, ends=ends)
        assert got is out
        torch.cuda.synchronize()
        assert (ybuf[:, :, :5] == -12345.5).all() and (ybuf[:, :, 5 + n_out:] == -12345.5).all()
        assert torch.equal(out.reshape(rows, n_out), want)
        assert torch.isnan(buf[:, :, :3]).all() and torch.isnan(buf[:, :, 3 + N:]).all()
        if R > 1:
            o2 = torch.full((R, C, n_out), 7.0, dtype=torch.float32, device=dev)
            assert resample(view, up, down, ht, ends, out=o2) is o2 and torch.equal(o2.reshape(rows, n_out), want)
            assert torch.equal(resample(view[2], up, down, ht, ends), want.view(R, C, n_out)[2])   # a 2-D recording
    assert_resample_close(want.cpu().numpy(), ref, x, h, up, down, ends, name=f"slice {dtype}")


def test_resampling_in_place_and_bad_arguments_are_refused():
    from eegnetreplication_amd import ops, resample
    dev = _dev()
    x = torch.zeros((4, 600), device=dev)
    buf = torch.zeros((4, 1000), device=dev)
    with pytest.raises(ValueError, match="in place is not supported"):
        resample(buf[:, :600], 1, 2, out=buf[:, 300:600])
    with pytest.raises(ValueError, match="odd number of taps"):
        resample(x, 1, 2, torch.zeros(4, dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError, match="n_taps must be odd and in"):
        resample(x, 1, 2, torch.zeros(ops.resample_max_taps() + 2, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="ends must be one of"):
        resample(x, 1, 2, ends="constant")
    with pytest.raises(RuntimeError, match="beyond up <="):
        resample(x, 257, 2, np.ones(3))


def test_rows_and_calls_do_not_mix():
    """Row i of a 45-row call equals the one-row call on it; two calls give the same bits; [R, C, N] is [R C, N]."""
    dev = _dev()
    kind = "64/125"
    ht = torch.from_numpy(_kind(kind)[2]).to(dev)
    N = _chunk_inputs(kind, lambda ch: 3 * ch + 5)
    x, _ = _case(N, "f32", kind, "reflect_limited")
    xt = torch.tensor(x, device=dev)
    a = _rs(xt, kind, taps=ht)
    assert torch.equal(a, _rs(xt, kind, taps=ht))
    for i in (0, 7, 44):
        assert torch.equal(_rs(xt[i:i + 1], kind, taps=ht), a[i:i + 1]), i
    y3 = _rs(xt.view(5, 9, N), kind, taps=ht)
    assert y3.shape == (5, 9, a.shape[1]) and torch.equal(y3.view(45, -1), a)


@pytest.mark.parametrize("ends", ENDS)
@pytest.mark.parametrize("kind", ["64/125", "3/2", "64/125 asym2501"])
def test_stream_blocks_equal_the_whole_recording_bit_for_bit(kind, ends):
    """Blocks of Q + 2 (the shortest first block), 1, 1, down - 1, a chunk's inputs + 1 and 777 samples, then
    flush(): every push returns the count the host helper names for it, and laid end to end they are the
    whole-recording call.  The same for [R, C, n] blocks, and for one block and the flush."""
    from eegnetreplication_amd import StreamResampler, ops
    dev = _dev()
    up, down, h = _kind(kind)
    Q = geometry(len(h), up, down)[3]
    blocks = [Q + 2, 1, 1, down - 1, _chunk_inputs(kind) + 1, 777]
    rows, N = 6, sum(blocks)
    x, ref = _case(N, "f32", kind, ends)
    xt = torch.tensor(x[:rows], device=dev)
    whole = _rs(xt, kind, ends)
    assert_resample_close(whole.cpu().numpy(), ref[:rows], x[:rows], h, up, down, ends, name=f"whole {kind} {ends}")
    for lead, view in (((rows,), xt), ((2, 3), xt.view(2, 3, N))):
        s = StreamResampler(lead if len(lead) > 1 else rows, up, down, h, ends)
        with pytest.raises(ValueError, match=f"at least {Q + 2} samples"):
            s.push(view[..., :Q + 1])
        parts, t = [], 0
        for i, n in enumerate(blocks):
            want_n = s.output_count(n)
            assert want_n == ops.resample_count(n, len(h), up, down, mode=ops.RESAMPLE_FIRST if i == 0 else ops.RESAMPLE_NEXT,
                                                n_before=t)
            y = s.push(view[..., t:t + n])                           # a time slice, as it lies
            assert y.shape[-1] == want_n and y.dtype == torch.float32 and tuple(y.shape[:-1]) == lead
            parts.append(y)
            t += n
        tail_n = s.output_count()
        parts.append(s.flush())
        assert parts[-1].shape[-1] == tail_n
        got = torch.cat(parts, dim=-1)
        assert got.shape[-1] == whole.shape[-1] == out_length(N, up, down)
        assert torch.equal(got.reshape(rows, -1), whole), (kind, ends)
        with pytest.raises(RuntimeError, match="flushed"):
            s.push(view[..., :5])
        with pytest.raises(RuntimeError, match="flushed"):
            s.flush()
        s.reset()
        one = torch.cat([s.push(view), s.flush()], dim=-1)           # one block and the flush
        assert torch.equal(one.reshape(rows, -1), whole)


def test_fp64_blocks_and_the_default_taps():
    """An fp64 recording streamed in three blocks with the stream's own default design."""
    from eegnetreplication_amd import StreamResampler, resample
    dev = _dev()
    up, down, h = _kind("64/125")
    rows, N = 3, 21 + 400 + 3
    x, ref = _case(N, "f64", "64/125", "reflect_limited")
    xt = torch.tensor(x[:rows], device=dev)
    s = StreamResampler(rows, 128, 250)
    got = torch.cat([s.push(xt[:, :21]), s.push(xt[:, 21:421]), s.push(xt[:, 421:]), s.flush()], dim=1)
    assert torch.equal(got, resample(xt, 128, 250))
    assert_resample_close(got.cpu().numpy(), ref[:rows], x[:rows], h, up, down, "reflect_limited", name="fp64 stream")


def test_the_stream_feeds_the_streaming_band_pass():
    """StreamResampler -> StreamBandpass block by block equals resample -> bandpass_filter of the whole recording."""
    from eegnetreplication_amd import StreamBandpass, StreamResampler, bandpass_filter, design_bandpass, resample
    dev = _dev()
    taps = design_bandpass()
    rec = torch.from_numpy(make_recording(22, 3000, 81)).to(dev)
    want = bandpass_filter(resample(rec, 64, 125), taps)
    rs, bp = StreamResampler(22, 64, 125), StreamBandpass(22, taps)
    parts = []
    for a, b in ((0, 500), (500, 501), (501, 1700), (1700, 3000)):
        y = rs.push(rec[:, a:b])
        if y.shape[-1]:
            parts.append(bp.push(y))
    parts.append(bp.push(rs.flush()))
    parts.append(bp.flush())
    assert torch.equal(torch.cat(parts, dim=1), want)


def test_graph_capture_and_the_preprocessing_chain():
    """One capture of resample on device taps; the replay, on a recording changed in place since the capture,
    equals the eager call bit for bit.  preprocess_recording(resample=(64, 125)) is the three calls made by hand."""
    from eegnetreplication_amd import (bandpass_filter, design_bandpass, exponential_moving_standardize,
                                       preprocess_recording, resample, resample_to)
    dev = _dev()
    h = torch.from_numpy(_kind("64/125")[2]).to(dev)
    bp = torch.from_numpy(design_bandpass()).to(dev)
    C, N = 22, _chunk_inputs("64/125") + 900
    rec = torch.from_numpy(make_recording(C, N, 61)).to(dev)

    def run():
        return resample(rec, 64, 125, h)

    run()                                                            # eager once: code objects loaded
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    rec.copy_(torch.from_numpy(make_recording(C, N, 62)).to(dev))
    g.replay()
    torch.cuda.synchronize()
    got = out.clone()
    want = run()
    assert torch.equal(got, want) and torch.isfinite(want).all()
    assert torch.equal(resample_to(rec, 250.0), want) and torch.equal(resample(rec, 128, 250), want)
    by_hand = bandpass_filter(want, bp)
    by_hand = exponential_moving_standardize(by_hand, out=by_hand)
    assert torch.equal(preprocess_recording(rec, bp, resample=(64, 125)), by_hand)
    assert torch.isfinite(by_hand).all()
