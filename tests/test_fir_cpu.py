"""Host side of the FIR band-pass and of cue epoching (``design_bandpass``, eegnet_fir, eegnet_fir_chunk,
eegnet_fir_max_taps, ``StreamBandpass``, ``epoch_starts``, ``epoch_logits``' host tables,
eegnet_forward_eval_windows_at): the filter design against its scipy restatement and the figures it is
documented with, the oracle against the ordered sum the kernel runs, and every rejection with its message.
The validation precedes every device call, so nothing here needs a GPU; the pointers handed in are never
dereferenced."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from fir_cases import (asymmetric_taps, extend, fir_bound, firwin_bandpass, gain, make_recording, oracle_fir,
                       ordered_fir)


def _lib():
    from eegnetreplication_amd import _lib
    return _lib.load()


def test_design_matches_the_firwin_restatement():
    from eegnetreplication_amd import design_bandpass
    for args in ((128.0, 4.0, 38.0), (250.0, 4.0, 38.0), (128.0, 8.0, 30.0), (100.0, 1.0, 45.0)):
        got, want = design_bandpass(*args), firwin_bandpass(*args)
        assert got.dtype == np.float64 and got.shape == want.shape, args
        err = float(np.abs(got - want).max())
        print(f"design_bandpass{args}: {len(got)} taps, max |diff| to firwin {err:.3e}")
        assert err <= 1e-15, args
    with pytest.raises(ValueError, match="l_freq < h_freq < sfreq / 2"):
        design_bandpass(128.0, 4.0, 64.0)


def test_design_figures():
    """The figures DESIGN 4.7 and the docstring quote: length, transitions, symmetry, DC gain and the gains at
    the band edges and at the middle and end of each transition band."""
    from eegnetreplication_amd import design_bandpass
    h = design_bandpass()                                          # 128 Hz, 4-38 Hz
    assert len(h) == 213
    assert np.abs(h - h[::-1]).max() <= 7e-18
    assert abs(h.sum()) <= 2e-16
    for f, want, tol in ((3.0, 0.499, 2e-3), (4.0, 0.9956, 2e-4), (38.0, 0.9949, 2e-4), (42.75, 0.499, 2e-3),
                         (47.5, 0.003, 1e-3)):
        g = gain(h, f, 128.0)
        print(f"|H({f} Hz)| = {g:.5f}")
        assert abs(g - want) <= tol, (f, g)
    assert len(design_bandpass(250.0)) == 413
    assert len(design_bandpass(250.0)) <= _lib().eegnet_fir_max_taps()


def test_oracle_against_the_ordered_loop():
    """np.convolve's sum against the tap-by-tap sum the kernel runs, on the GPU tests' recordings at the
    213-tap design: the difference is the fp64 reassociation error, which the bound's second term covers
    twice over (once per side).  Printed: the largest difference and the smallest second term on the rows
    that ride on a DC offset of 100 -- measured 5.4e-14 against 1.3e-11: the bound is derived from the
    worst case of L roundings, the roundings of a real sum mostly cancel."""
    from eegnetreplication_amd import design_bandpass
    h = design_bandpass()
    worst, least = 0.0, np.inf
    for N in (1, 2, 106, 107, 213, 1000):
        for dt in (np.float32, np.float64):
            x = make_recording(45, N, 2000 + N, dt)
            ref, got = oracle_fir(x, h), ordered_fir(x, h)
            assert ref.shape == got.shape == (45, N)
            fp64_term = fir_bound(x, h, np.zeros_like(ref))
            assert (np.abs(got - ref) <= fp64_term).all(), N
            worst = max(worst, float(np.abs(got - ref).max()))
            least = min(least, float(fp64_term[1::3].min()))       # the rows on a DC offset of 100
    print(f"ordered loop vs oracle: max |diff| {worst:.3e}; the bound's fp64 term on the offset rows {least:.3e}")
    assert worst <= least / 100                                    # two orders of magnitude of room
    # the asymmetric taps tell a reversed convolution from the right one
    ha = asymmetric_taps(213)
    x = make_recording(3, 500, 5, np.float64)
    assert np.abs(oracle_fir(x, ha) - oracle_fir(x, ha[::-1])).max() > 1e-2
    assert np.abs(oracle_fir(x, ha) - ordered_fir(x, ha)).max() <= 1e-12


def test_the_extension_rule():
    x = np.arange(1.0, 6.0)[None]                                  # 1 2 3 4 5
    assert extend(x, 5).tolist() == [[-1.0, 0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]]
    # the reflection runs out at N - 1 samples: zero beyond
    assert extend(x[:, :2], 7).tolist() == [[0.0, 0.0, 0.0, 1.0, 2.0, 3.0, 0.0, 0.0]]
    assert extend(x[:, :1], 5).tolist() == [[0.0, 0.0, 1.0, 0.0, 0.0]]
    assert oracle_fir(x, [0.0, 0.0, 1.0]).tolist() == [[0.0, 1.0, 2.0, 3.0, 4.0]]     # h[L-1]: a delay of M
    assert oracle_fir(x, [1.0, 0.0, 0.0]).tolist() == [[2.0, 3.0, 4.0, 5.0, 6.0]]     # h[0]: an advance of M


WHOLE, FIRST, NEXT, TAIL = 0, 1, 2, 3


def _call(lib, *, x=4096, f64=0, rows=3, n=512, x_pitch=None, taps=8192, n_taps=213, y=1 << 20, y_pitch=None,
          hist_in=None, hist_out=None, mode=WHOLE):
    """eegnet_fir with dummy non-NULL pointers (every call here fails before a launch)."""
    vp = lambda v: None if v is None else ctypes.c_void_p(v)
    rc = lib.eegnet_fir(vp(x), f64, rows, n, n if x_pitch is None else x_pitch, vp(taps), n_taps, vp(y),
                        n if y_pitch is None else y_pitch, vp(hist_in), vp(hist_out), mode, None)
    return rc, lib.eegnet_last_error().decode()


def test_fir_geometry_calls():
    lib = _lib()
    from eegnetreplication_amd import ops
    assert lib.eegnet_fir_max_taps() >= 2049 and lib.eegnet_fir_max_taps() % 2 == 1
    assert ops.fir_max_taps() == lib.eegnet_fir_max_taps()
    assert lib.eegnet_fir_chunk() >= 64 and ops.fir_chunk() == lib.eegnet_fir_chunk()
    assert (ops.FIR_WHOLE, ops.FIR_FIRST, ops.FIR_NEXT, ops.FIR_TAIL) == (WHOLE, FIRST, NEXT, TAIL)


def test_fir_rejections():
    lib = _lib()
    cap, ch = lib.eegnet_fir_max_taps(), lib.eegnet_fir_chunk()
    for name, kw in [("x", dict(x=None)), ("y", dict(y=None)), ("taps", dict(taps=None))]:
        assert _call(lib, **kw) == (-1, f"{name} is NULL"), name
    odd = "eegnet_fir: a zero-phase filter needs an odd n_taps (got 212); only a continuation call takes an even one"
    cases = [
        (dict(mode=4), "eegnet_fir: unknown mode 4"),
        (dict(mode=-1), "eegnet_fir: unknown mode -1"),
        (dict(n_taps=0), f"eegnet_fir: n_taps must be in [1, {cap}] (got 0)"),
        (dict(n_taps=cap + 1), f"eegnet_fir: n_taps must be in [1, {cap}] (got {cap + 1})"),
        (dict(n_taps=cap + 2), f"eegnet_fir: n_taps must be in [1, {cap}] (got {cap + 2})"),
        (dict(n_taps=212), odd),
        (dict(n_taps=212, mode=FIRST, hist_out=64), odd),
        (dict(n_taps=212, mode=TAIL, n=0, hist_in=64), odd),
        (dict(rows=0), "eegnet_fir: n_rows must be >= 1 (got 0)"),
        (dict(n=0), "eegnet_fir: n_samples must be >= 1 (got 0)"),
        (dict(mode=FIRST, n=212, hist_out=64),
         "eegnet_fir: n_samples must be >= 213 = n_taps for a stream's first block (got 212)"),
        (dict(mode=TAIL, n=5, hist_in=64), "eegnet_fir: the tail call takes no samples (n_samples = 5)"),
        (dict(mode=NEXT, hist_out=64), "eegnet_fir: this mode reads the history: hist_in is NULL"),
        (dict(mode=TAIL, n=0), "eegnet_fir: this mode reads the history: hist_in is NULL"),
        (dict(mode=NEXT, hist_in=64), "eegnet_fir: this mode writes the history: hist_out is NULL"),
        (dict(mode=FIRST), "eegnet_fir: this mode writes the history: hist_out is NULL"),
        (dict(n=512, x_pitch=511), "eegnet_fir: x_pitch = 511 is below n_samples = 512"),
        (dict(n=512, y_pitch=511), "eegnet_fir: y_pitch = 511 is below the 512 outputs of a row"),
        (dict(mode=FIRST, n=512, y_pitch=405, hist_out=64), "eegnet_fir: y_pitch = 405 is below the 406 outputs of a row"),
        (dict(x=4098), "eegnet_fir: x, y, taps and the histories must be aligned to their element size"),
        (dict(x=4100, f64=1), "eegnet_fir: x, y, taps and the histories must be aligned to their element size"),
        (dict(taps=8196), "eegnet_fir: x, y, taps and the histories must be aligned to their element size"),
        (dict(mode=NEXT, hist_in=68, hist_out=1 << 24),
         "eegnet_fir: x, y, taps and the histories must be aligned to their element size"),
    ]
    for kw, msg in cases:
        assert _call(lib, **kw) == (-1, msg), kw
    # no in-place filtering: y on x, y inside x, y's last row reaching x's first
    over = "eegnet_fir: y overlaps x (filtering in place is not supported)"
    nbytes = 4 * (2 * 512 + 512)
    for kw in (dict(x=4096, y=4096), dict(x=4096, y=4096 + 400), dict(x=4096, y=4096 + nbytes - 4),
               dict(x=4096 + nbytes - 4, y=4096), dict(x=8192, f64=1, y=8192 + 8 * 1536 - 4)):
        assert _call(lib, **kw) == (-1, over), kw
    hover = "eegnet_fir: hist_out overlaps hist_in (the call reads one and writes the other)"
    hb = 3 * 212 * 8
    for hi, ho in ((1 << 24, 1 << 24), (1 << 24, (1 << 24) + hb - 8), ((1 << 24) + 8, 1 << 24)):
        assert _call(lib, mode=NEXT, hist_in=hi, hist_out=ho) == (-1, hover), (hi, ho)
    # the grid: n_rows * chunks workgroups, the limit named
    rc, msg = _call(lib, rows=1 << 31, n=ch + 1)
    assert rc == -1 and "2 chunks" in msg and "exceed the grid limit of 2147483647 workgroups" in msg
    rc, msg = _call(lib, rows=3, n=1 << 62)
    assert rc == -1 and "exceed the grid limit of 2147483647 workgroups" in msg
    # an even filter is a continuation's alone, and a one-tap stream needs no history
    rc, msg = _call(lib, n_taps=212, mode=NEXT)
    assert rc == -1 and msg == "eegnet_fir: this mode reads the history: hist_in is NULL"


def test_python_surface_refusals_need_no_device():
    from eegnetreplication_amd import StreamBandpass, bandpass_filter, design_bandpass, preprocess_recording
    h = design_bandpass()
    with pytest.raises(RuntimeError, match="HIP device"):
        bandpass_filter(torch.zeros(22, 512), h)
    with pytest.raises(RuntimeError, match="HIP device"):
        preprocess_recording(torch.zeros(22, 512), h)
    for shape in ((512,), (2, 3, 22, 512)):
        with pytest.raises(RuntimeError, match="expected a recording"):
            bandpass_filter(torch.zeros(shape), h)
    with pytest.raises(ValueError, match="out must have the recording's shape"):
        bandpass_filter(torch.zeros(22, 512), h, out=torch.zeros(22, 511))
    # the stream: an odd filter, a first block of at least L samples
    with pytest.raises(ValueError, match="odd number of taps"):
        StreamBandpass(22, h[:-1])
    with pytest.raises(ValueError, match="leading shape"):
        StreamBandpass((2, 3, 4), h)
    s = StreamBandpass(22, h)
    with pytest.raises(ValueError, match="at least the filter's 213 samples \\(got 212\\)"):
        s.push(torch.zeros(22, 212))
    with pytest.raises(RuntimeError, match="expected a block"):
        s.push(torch.zeros(21, 512))
    with pytest.raises(RuntimeError, match="before the first push"):
        s.flush()
    with pytest.raises(RuntimeError, match="HIP device"):
        s.push(torch.zeros(22, 213))                                # long enough: it gets as far as the device
    s.reset()


def test_epoch_starts():
    from eegnetreplication_amd import epoch_starts
    got = epoch_starts([0, 100, 1000])
    assert got.dtype == torch.int64 and got.tolist() == [64, 164, 1064]          # 0.5 s at 128 Hz
    assert epoch_starts(np.array([250, 500]), sfreq=250.0, tmin=0.5).tolist() == [375, 625]
    assert epoch_starts(torch.tensor([10], dtype=torch.int32), 128.0, 0.0).tolist() == [10]
    assert epoch_starts([7], 100.0, 0.125).tolist() == [7 + 12]                  # round(12.5): to even, as round()
    with pytest.raises(ValueError, match="expected integers"):
        epoch_starts([1.5])


def test_epoch_logits_rejects_a_bad_host_table():
    """A host table is checked before anything touches a device: the recording may even be a CPU tensor."""
    from eegnetreplication_amd import EEGNet, epoch_logits
    m = EEGNet(22, 257)
    rec = torch.zeros(3, 22, 1000)
    last = 1000 - 257
    for starts in ([0, last + 1], np.array([-1, 5]), torch.tensor([last, 1000])):
        with pytest.raises(ValueError, match=r"starts\[\d\] = -?\d+ is outside \[0, 743\]"):
            epoch_logits(m, rec, starts)
    with pytest.raises(ValueError, match=r"rec_index\[1\] = 3 is outside \[0, 2\]"):
        epoch_logits(m, rec, [0, 5], rec_index=[0, 3])
    with pytest.raises(ValueError, match=r"rec_index\[0\] = -1 is outside"):
        epoch_logits(m, rec, [0, 5], rec_index=np.array([-1, 0]))
    with pytest.raises(ValueError, match=r"rec_index\[0\] = 1 is outside \[0, 0\]"):
        epoch_logits(m, rec[0], [0], rec_index=[1])                   # a 2-D recording is recording 0
    with pytest.raises(ValueError, match="rec_index holds 1 entries, starts 2"):
        epoch_logits(m, rec, [0, 5], rec_index=[0])
    with pytest.raises(ValueError, match="table of integers"):
        epoch_logits(m, rec, [0.5, 2.0])
    with pytest.raises(RuntimeError, match="expected a recording"):
        epoch_logits(m, torch.zeros(22, 256), [0])
    with pytest.raises(RuntimeError, match="HIP device"):
        epoch_logits(m, rec, [0, last], rec_index=[2, 0])            # a valid table gets as far as the device


def test_windows_at_rejections():
    from eegnetreplication_amd import _lib as L
    lib = _lib()
    d = L.dims(1, 22, 257)
    p = ctypes.c_void_p(4096)

    def call(dims=d, params=p, bn=p, rec=p, n_rec=3, n=1000, pitch=1000, starts=ctypes.c_void_p(8192), idx=None, W=5,
             logits=p):
        rc = lib.eegnet_forward_eval_windows_at(ctypes.byref(dims), params, bn, rec, n_rec, n, pitch, starts, idx, W,
                                                logits, None)
        return rc, lib.eegnet_last_error().decode()

    for name, kw in [("params", dict(params=None)), ("bn_buffers", dict(bn=None)), ("rec", dict(rec=None)),
                     ("logits", dict(logits=None)), ("starts", dict(starts=None))]:
        assert call(**kw) == (-1, f"{name} is NULL"), name
    cases = [
        (dict(n_rec=0), "windows at a table: n_rec must be in [1, 2^31) (got 0)"),
        (dict(n=256), "windows at a table: n_samples = 256 is shorter than one window (T = 257)"),
        (dict(pitch=999), "windows at a table: pitch = 999 is below n_samples = 1000"),
        (dict(W=0), "windows at a table: n_windows must be in [1, 2^31) (got 0)"),
        (dict(W=1 << 31), "windows at a table: n_windows must be in [1, 2^31) (got 2147483648)"),
        (dict(starts=ctypes.c_void_p(8196)),
         "windows at a table: rec, starts and rec_index must be aligned to their element size"),
        (dict(idx=ctypes.c_void_p(8194)),
         "windows at a table: rec, starts and rec_index must be aligned to their element size"),
    ]
    for kw, msg in cases:
        assert call(**kw) == (-1, msg), kw
    rc, msg = call(dims=L.dims(1, 64, 512, F1=16, D=4))
    assert rc == -1 and "windows at a table: F1*D = 64 > 16 is not supported" in msg
