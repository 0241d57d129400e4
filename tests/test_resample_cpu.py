"""Host side of the polyphase resampler (``design_resampler``, ``resampled_length``, ``resampled_onsets``,
``resample_ratio``, eegnet_resample, eegnet_resample_count, ``StreamResampler``): the oracle against
``scipy.signal.resample_poly`` and against an independent construction of the reflected ends, the filter design
against ``firwin``, the ordered sum the kernel runs against the bound, and every rejection with its message.
The validation precedes every device call, so nothing here needs a GPU; the pointers handed in are never
dereferenced."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from resample_cases import (asymmetric_taps, extend, firwin_resampler, geometry, make_recording, oracle_resample,
                            ordered_resample, out_length, resample_bound)

RATIOS = [(64, 125), (2, 5), (3, 2), (1, 3), (1, 2)]


def _lib():
    from eegnetreplication_amd import _lib
    return _lib.load()


def test_design_matches_firwin():
    pytest.importorskip("scipy")
    from eegnetreplication_amd import design_resampler
    for up, down in RATIOS + [(128, 250), (16, 125), (32, 25)]:
        got, want = design_resampler(up, down), firwin_resampler(up, down)
        assert got.dtype == np.float64 and got.shape == want.shape, (up, down)
        err = float(np.abs(got - want).max())
        print(f"design_resampler({up}, {down}): {len(got)} taps, max |diff| to firwin {err:.3e}")
        assert err <= 1e-15 * max(1.0, np.abs(want).max()), (up, down)
    h = design_resampler(128, 250)
    assert len(h) == 2501 and geometry(len(h), 64, 125)[4] == 40          # the figures the docstring quotes
    assert abs(h.sum() - 64.0) <= 1e-12
    assert len(design_resampler(3, 2, half_len_factor=4)) == 2 * 4 * 3 + 1
    with pytest.raises(ValueError, match="nothing to resample"):
        design_resampler(5, 5)
    with pytest.raises(ValueError, match="integers >= 1"):
        design_resampler(0, 5)


def test_oracle_against_scipy_resample_poly():
    """ends="zero" is resample_poly's default padtype='constant' with the same taps: equal lengths at every N, and
    values within the fp64 term of the bound (scipy convolves the zero-stuffed signal in another order)."""
    sig = pytest.importorskip("scipy.signal")
    from eegnetreplication_amd import design_resampler
    worst = 0.0
    for up, down in RATIOS:
        h = design_resampler(up, down)
        for N in list(range(1, 40)) + [125, 126, 250, 1001]:
            x = make_recording(3, N, 300 + N, np.float64)
            ref = oracle_resample(x, h, up, down, "zero")
            want = sig.resample_poly(x, up, down, axis=1, window=h / up)     # (scipy multiplies given taps by up)
            assert ref.shape == want.shape == (3, out_length(N, up, down)), (up, down, N)
            err = np.abs(ref - want)
            assert (err <= resample_bound(x, h, up, down, "zero", np.zeros_like(ref))).all(), (up, down, N)
            worst = max(worst, float(err.max()))
    print(f"oracle vs scipy.signal.resample_poly: max |diff| {worst:.3e} on values near 100")


def test_oracle_against_the_ordered_loop():
    """The per-phase matrix product against the term-by-term sum the kernel runs: the difference is the fp64
    reassociation error, which the bound's second term covers twice over (once per side).  Printed: the largest
    difference and the smallest second term on the rows that ride on a DC offset of 100."""
    from eegnetreplication_amd import design_resampler
    worst, least = 0.0, np.inf
    for up, down in RATIOS:
        h = design_resampler(up, down)
        for ends in ("zero", "reflect_limited"):
            for N in (1, 2, 21, 126, 1000):
                for dt in (np.float32, np.float64):
                    x = make_recording(6, N, 2000 + N, dt)
                    ref, got = oracle_resample(x, h, up, down, ends), ordered_resample(x, h, up, down, ends)
                    assert ref.shape == got.shape == (6, out_length(N, up, down))
                    fp64_term = resample_bound(x, h, up, down, ends, np.zeros_like(ref))
                    assert (np.abs(got - ref) <= fp64_term).all(), (up, down, ends, N)
                    worst = max(worst, float(np.abs(got - ref).max()))
                    least = min(least, float(fp64_term[1::3].min()))
    print(f"ordered loop vs oracle: max |diff| {worst:.3e}; the bound's fp64 term on the offset rows {least:.3e}")
    assert worst <= least / 10
    # asymmetric taps tell a sum run the wrong way round from the right one
    ha = asymmetric_taps(2501, 64)
    x = make_recording(3, 500, 5, np.float64)
    assert np.abs(oracle_resample(x, ha, 64, 125) - oracle_resample(x, ha[::-1], 64, 125)).max() > 1e-2
    assert np.abs(oracle_resample(x, ha, 64, 125) - ordered_resample(x, ha, 64, 125)).max() <= 1e-10


def test_the_extension_rule():
    x = np.arange(1.0, 6.0)[None]                                  # 1 2 3 4 5; L = 5, up = 1: Q = 2, Q + 1 = 3
    u, pad = extend(x, 5, 1, "reflect_limited", pad=4)
    assert pad == 4 and u.tolist() == [[0.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 0.0]]
    assert extend(x, 5, 1, "zero", pad=2)[0].tolist() == [[0.0, 0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 0.0, 0.0]]
    # the reflection runs out at N - 1 samples: zero beyond
    assert extend(x[:, :2], 5, 1, "reflect_limited", pad=3)[0].tolist() == [[0.0, 0.0, 0.0, 1.0, 2.0, 3.0, 0.0, 0.0]]
    assert extend(x[:, :1], 5, 1, "reflect_limited", pad=2)[0].tolist() == [[0.0, 0.0, 1.0, 0.0, 0.0]]
    # a delta prototype h[half + s] = up: y[m] = u[(m down - s) / up] where that is an integer, else 0
    h = np.zeros(5)
    h[2] = 1.0
    assert oracle_resample(x, h, 1, 2, "zero").tolist() == [[1.0, 3.0, 5.0]]
    h = np.zeros(5)
    h[3] = 2.0                                                     # s = 1 at 2/1: y[2 n + 1] = 2 x[n]
    assert oracle_resample(x, h, 2, 1, "zero").tolist() == [[0.0, 2.0, 0.0, 4.0, 0.0, 6.0, 0.0, 8.0, 0.0, 10.0]]


def test_reflected_ends_against_a_padded_row():
    """Independent of ``extend``'s reflection: pad the row by P = down k samples reflected by hand, run the
    zero-ends oracle, and drop up k outputs at each end.  P >= Q + 1 samples of reflection are all an output can
    reach, so the two agree (to the fp64 term: the matrix products see other shapes) wherever both are defined --
    P <= N - 1."""
    from eegnetreplication_amd import design_resampler
    for up, down in RATIOS:
        h = design_resampler(up, down)
        up, down, half, Q, K = geometry(len(h), up, down)
        k = -(-(Q + 1) // down)
        P = down * k
        for N in (P + 1, P + 2, 3 * P + 7):
            x = make_recording(4, N, 900 + N, np.float64)
            j = np.arange(1, P + 1)
            padded = np.concatenate([2.0 * x[:, :1] - x[:, j[::-1]], x, 2.0 * x[:, N - 1:] - x[:, N - 1 - j]], axis=1)
            wide = oracle_resample(padded, h, up, down, "zero")
            ref = oracle_resample(x, h, up, down, "reflect_limited")
            assert wide.shape[1] == ref.shape[1] + 2 * up * k, (up, down, N)
            cut = wide[:, up * k:up * k + ref.shape[1]]
            err = np.abs(cut - ref)
            assert (err <= resample_bound(x, h, up, down, "reflect_limited", np.zeros_like(ref))).all(), (up, down, N)
            # and the zero ends are another thing: decimated, an input near 100 comes out far from it
            if down > up:
                assert np.abs(oracle_resample(x, h, up, down, "zero")[1, 0] - x[1, 0]) > 10.0


def test_lengths_onsets_and_ratios():
    from eegnetreplication_amd import resample_ratio, resampled_length, resampled_onsets
    assert resample_ratio(250.0, 128.0) == (64, 125) and resample_ratio(250) == (64, 125)
    assert resample_ratio(256.0) == (1, 2)
    assert resample_ratio(1000.0) == (16, 125)
    assert resample_ratio(100.0) == (32, 25)
    assert resample_ratio(128.0, 250.0) == (125, 64)
    with pytest.raises(ValueError, match="nothing to resample"):
        resample_ratio(128.0, 128.0)
    with pytest.raises(ValueError, match="up exceeds the resampler's 256"):
        resample_ratio(1000.0, 257.0)
    for (up, down), n, want in [((64, 125), 672000, 344064), ((128, 250), 1001, 513), ((1, 2), 7, 4), ((16, 125), 1000, 128),
                                ((32, 25), 100, 128), ((3, 2), 1, 2), ((1, 3), 1, 1)]:
        assert resampled_length(n, up, down) == want == out_length(n, up, down), (up, down, n)
    # the nearest new sample, a tie going up: 125 samples at 250 Hz are 64 at 128 Hz
    got = resampled_onsets([0, 1, 125, 250, 251, 672000 - 1], 64, 125)
    assert got.dtype == torch.int64 and got.tolist() == [0, 1, 64, 128, 129, 344063]
    assert resampled_onsets(np.array([0, 1, 2, 3]), 1, 2).tolist() == [0, 1, 1, 2]        # 0.5 -> 1, 1.5 -> 2
    assert resampled_onsets(torch.tensor([3], dtype=torch.int32), 3, 2).tolist() == [5]  # 4.5 -> 5
    with pytest.raises(ValueError, match="expected integers"):
        resampled_onsets([1.5], 64, 125)


WHOLE, FIRST, NEXT, TAIL = 0, 1, 2, 3
ZERO, REFLECT = 0, 1


def _call(lib, *, x=4096, f64=0, rows=3, n=1000, x_pitch=None, taps=8192, n_taps=2501, up=64, down=125, ends=REFLECT,
          y=1 << 20, y_pitch=None, n_before=0, hist_in=None, hist_out=None, mode=WHOLE):
    """eegnet_resample with dummy non-NULL pointers (every call here fails before a launch)."""
    vp = lambda v: None if v is None else ctypes.c_void_p(v)
    rc = lib.eegnet_resample(vp(x), f64, rows, n, n if x_pitch is None else x_pitch, vp(taps), n_taps, up, down, ends,
                             vp(y), n if y_pitch is None else y_pitch, n_before, vp(hist_in), vp(hist_out), mode, None)
    return rc, lib.eegnet_last_error().decode()


def _count(lib, n, n_before=0, n_taps=2501, up=64, down=125, mode=WHOLE):
    out = ctypes.c_int64(-1)
    rc = lib.eegnet_resample_count(n, n_before, n_taps, up, down, mode, ctypes.byref(out))
    return rc, out.value


def test_resample_geometry_calls():
    lib = _lib()
    from eegnetreplication_amd import ops
    assert lib.eegnet_resample_max_taps() >= 4097 and lib.eegnet_resample_max_taps() % 2 == 1
    assert ops.resample_max_taps() == lib.eegnet_resample_max_taps()
    assert ops.resample_max_up() == lib.eegnet_resample_max_up() >= 64
    assert (ops.RESAMPLE_WHOLE, ops.RESAMPLE_FIRST, ops.RESAMPLE_NEXT, ops.RESAMPLE_TAIL) == (WHOLE, FIRST, NEXT, TAIL)
    assert ops.RESAMPLE_ENDS == {"zero": ZERO, "reflect_limited": REFLECT}
    # the counts: scipy's length for a whole row, the ratio reduced first
    for up, down in RATIOS + [(128, 250)]:
        for n in (1, 2, 124, 125, 126, 1001, 672000):
            assert _count(lib, n, up=up, down=down, n_taps=61) == (0, out_length(n, up, down)), (up, down, n)
    # a stream's counts: output m is out once m down + half < t up; the pushes and the flush add up to the whole
    for (up, down), L in (((64, 125), 2501), ((3, 2), 61), ((1, 3), 61), ((2, 5), 1)):
        u, d, half, Q, K = geometry(L, up, down)
        done = lambda t: sum(1 for m in range(out_length(t, u, d) + 1) if m * d + half < t * u)
        t, total = Q + 2, 0
        rc, c = _count(lib, t, n_taps=L, up=up, down=down, mode=FIRST)
        assert (rc, c) == (0, done(t)), (up, down)
        total += c
        for n in (1, 1, d - 1, 300, 7):
            rc, c = _count(lib, n, t, n_taps=L, up=up, down=down, mode=NEXT)
            assert (rc, c) == (0, done(t + n) - done(t)), (up, down, t, n)
            t, total = t + n, total + c
        rc, c = _count(lib, 0, t, n_taps=L, up=up, down=down, mode=TAIL)
        assert rc == 0 and total + c == out_length(t, u, d), (up, down)


def test_resample_rejections():
    lib = _lib()
    cap, cup = lib.eegnet_resample_max_taps(), lib.eegnet_resample_max_up()
    for name, kw in [("x", dict(x=None)), ("y", dict(y=None)), ("taps", dict(taps=None))]:
        assert _call(lib, **kw) == (-1, f"{name} is NULL"), name
    taps = lambda v: f"eegnet_resample: n_taps must be odd and in [1, {cap}] (got {v})"
    span = (1 << 61) // 125
    cases = [
        (dict(mode=4), "eegnet_resample: unknown mode 4"),
        (dict(mode=-1), "eegnet_resample: unknown mode -1"),
        (dict(n_taps=0), taps(0)),
        (dict(n_taps=2500), taps(2500)),
        (dict(n_taps=cap + 1), taps(cap + 1)),
        (dict(n_taps=cap + 2), taps(cap + 2)),
        (dict(up=0), "eegnet_resample: up and down must be >= 1 (got 0/125)"),
        (dict(down=-3), "eegnet_resample: up and down must be >= 1 (got 64/-3)"),
        (dict(up=125), "eegnet_resample: 125/125 reduces to 1/1: nothing to resample"),
        (dict(up=1, down=1), "eegnet_resample: 1/1 reduces to 1/1: nothing to resample"),
        (dict(up=cup + 1, down=cup + 2),
         f"eegnet_resample: {cup + 1}/{cup + 2} reduces to {cup + 1}/{cup + 2}, beyond up <= {cup}, down <= 1048576"),
        (dict(up=1, down=(1 << 20) + 1),
         f"eegnet_resample: 1/1048577 reduces to 1/1048577, beyond up <= {cup}, down <= 1048576"),
        (dict(ends=2), "eegnet_resample: unknown ends 2"),
        (dict(rows=0), "eegnet_resample: n_rows must be >= 1 (got 0)"),
        (dict(n=0), f"eegnet_resample: n_samples must be in [1, {span}] (got 0)"),
        (dict(n=1 << 62), f"eegnet_resample: n_samples must be in [1, {span}] (got {1 << 62})"),
        (dict(n_before=5), "eegnet_resample: a recording's first samples come after none (n_before = 5)"),
        (dict(n_before=-1), f"eegnet_resample: n_before must be in [0, {span}] (got -1)"),
        # 2501 taps at up = 64: Q = 1250 // 64 = 19, a first block of Q + 2 = 21 samples
        (dict(mode=FIRST, n=20, hist_out=64), f"eegnet_resample: n_samples must be in [21, {span}], at least half / up + 2 "
                                              f"for a stream's first block (got 20)"),
        (dict(mode=NEXT, n_before=20, hist_in=64, hist_out=1 << 24),
         "eegnet_resample: a stream's first block holds at least 21 samples (n_before = 20)"),
        (dict(mode=TAIL, n=5, n_before=100, hist_in=64), "eegnet_resample: the tail call takes no samples (n_samples = 5)"),
        (dict(mode=NEXT, n_before=100, hist_out=64), "eegnet_resample: this mode reads the history: hist_in is NULL"),
        (dict(mode=TAIL, n=0, n_before=100), "eegnet_resample: this mode reads the history: hist_in is NULL"),
        (dict(mode=NEXT, n_before=100, hist_in=64), "eegnet_resample: this mode writes the history: hist_out is NULL"),
        (dict(mode=FIRST), "eegnet_resample: this mode writes the history: hist_out is NULL"),
        (dict(n=1000, x_pitch=999), "eegnet_resample: x_pitch = 999 is below n_samples = 1000"),
        (dict(n=1000, y_pitch=511), "eegnet_resample: y_pitch = 511 is below the 512 outputs of a row"),
        (dict(up=128, down=250, n=1000, y_pitch=511), "eegnet_resample: y_pitch = 511 is below the 512 outputs of a row"),
        (dict(x=4098), "eegnet_resample: x, y, taps and the histories must be aligned to their element size"),
        (dict(x=4100, f64=1), "eegnet_resample: x, y, taps and the histories must be aligned to their element size"),
        (dict(taps=8196), "eegnet_resample: x, y, taps and the histories must be aligned to their element size"),
        (dict(mode=NEXT, n_before=100, hist_in=68, hist_out=1 << 24),
         "eegnet_resample: x, y, taps and the histories must be aligned to their element size"),
    ]
    for kw, msg in cases:
        assert _call(lib, **kw) == (-1, msg), kw
    # no resampling in place: y on x, y inside x, y's last row reaching x's first
    over = "eegnet_resample: y overlaps x (resampling in place is not supported)"
    xbytes, ybytes = 4 * (2 * 1000 + 1000), 4 * (2 * 1000 + 512)
    for kw in (dict(x=4096, y=4096), dict(x=4096, y=4096 + 400), dict(x=4096, y=4096 + xbytes - 4),
               dict(x=4096 + ybytes - 4, y=4096), dict(x=8192, f64=1, y=8192 + 8 * 3000 - 4)):
        assert _call(lib, **kw) == (-1, over), kw
    hover = "eegnet_resample: hist_out overlaps hist_in (the call reads one and writes the other)"
    hb = 3 * 40 * 8                                                 # 2 Q + 2 = 40 doubles per row
    for hi, ho in ((1 << 24, 1 << 24), (1 << 24, (1 << 24) + hb - 8), ((1 << 24) + 8, 1 << 24)):
        assert _call(lib, mode=NEXT, n_before=100, hist_in=hi, hist_out=ho) == (-1, hover), (hi, ho)
    # the grid: n_rows * chunks workgroups, the limit named
    rc, msg = _call(lib, rows=1 << 31, n=10)
    assert rc == -1 and "1 chunks" in msg and "exceed the grid limit of 2147483647 workgroups" in msg
    rc, msg = _call(lib, rows=3, n=1 << 50, x_pitch=1 << 50, y_pitch=1 << 50)
    assert rc == -1 and "exceed the grid limit of 2147483647 workgroups" in msg
    # the count helper refuses the same integers in the same words
    assert _count(lib, 0)[0] == -1 and lib.eegnet_last_error().decode() == f"eegnet_resample: n_samples must be in [1, {span}] (got 0)"
    assert _count(lib, 10, n_taps=2500)[0] == -1 and lib.eegnet_last_error().decode() == taps(2500)
    assert lib.eegnet_resample_count(10, 0, 61, 1, 2, 0, None) == -1


def test_python_surface_refusals_need_no_device():
    from eegnetreplication_amd import (StreamResampler, design_bandpass, design_resampler, preprocess_recording, resample,
                                       resample_to)
    with pytest.raises(RuntimeError, match="HIP device"):
        resample(torch.zeros(22, 512), 64, 125)
    with pytest.raises(RuntimeError, match="HIP device"):
        resample_to(torch.zeros(22, 512), 250.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        preprocess_recording(torch.zeros(22, 512), design_bandpass(), resample=(64, 125))
    for shape in ((512,), (2, 3, 22, 512)):
        with pytest.raises(RuntimeError, match="expected a recording"):
            resample(torch.zeros(shape), 64, 125)
    with pytest.raises(ValueError, match="nothing to resample"):
        resample(torch.zeros(22, 512), 5, 5)
    with pytest.raises(ValueError, match=r"out must have the shape \[22, 263\]"):
        resample(torch.zeros(22, 512), 64, 125, out=torch.zeros(22, 262))
    # the stream: an odd prototype, a first block of at least Q + 2 samples
    h = design_resampler(64, 125)
    with pytest.raises(ValueError, match="odd number of taps"):
        StreamResampler(22, 64, 125, h[:-1])
    with pytest.raises(ValueError, match="leading shape"):
        StreamResampler((2, 3, 4), 64, 125)
    with pytest.raises(ValueError, match="ends must be one of"):
        StreamResampler(22, 64, 125, ends="constant")
    s = StreamResampler(22, 128, 250)                               # reduced to 64/125, the default taps
    assert (s.up, s.down, s.n_taps, s.first_block) == (64, 125, 2501, 21)
    assert s.output_count(21) == 1 and s.output_count(100) == 42    # m 125 + 1250 < 64 t
    with pytest.raises(ValueError, match="at least 21 samples \\(got 20\\)"):
        s.push(torch.zeros(22, 20))
    with pytest.raises(RuntimeError, match="expected a block"):
        s.push(torch.zeros(21, 512))
    with pytest.raises(RuntimeError, match="before the first push"):
        s.flush()
    with pytest.raises(RuntimeError, match="HIP device"):
        s.push(torch.zeros(22, 21))                                 # long enough: it gets as far as the device
    s.reset()
