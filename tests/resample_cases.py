"""Rational polyphase resampling of recordings: the float64 oracle, an ordered restatement of the sum the kernel
runs, the bound every GPU comparison is held to, and the taps the tests use.

With the prototype taps h[0..L-1], L = 2 half + 1, up/down reduced, Q = half // up and c = m down + half, output m
of the ceil(N up / down) of a row of N samples is

    y[m] = sum_{n = ceil((c - 2 half) / up) .. floor(c / up)} h[c - n up] u[n]

u being the row extended past its ends: by zeros (``ends="zero"``: ``scipy.signal.resample_poly``'s default), or by
the band-pass's odd reflection (``ends="reflect_limited"``): u[-j] = 2 x[0] - x[j], u[N-1+j] = 2 x[N-1] - x[N-1-j]
for 1 <= j <= min(Q + 1, N - 1), zero beyond.  With p = c mod up and q = c // up the terms are h[p + j up] u[q - j],
j = 0 .. K-1, K = ceil(L / up), h read as 0 past its end.  ``oracle_resample`` gathers, phase by phase, the K
samples of every output of that phase and multiplies by the phase's taps (one matrix product per phase);
``ordered_resample`` adds the same products term by term in the order j = 0..K-1, the kernel's order (without its
fused multiply-add).  This is the polyphase method, not the FFT method of the reference's ``raw.resample``:
``mne`` is not installed where these tests run, and nothing here restates it.

The bound: |gpu - oracle| <= 2^-23 |oracle| + 2 K 2^-53 max_p sum_j |h[p + j up]| max|u|.  The first term is one
fp32 ulp, for the single final rounding; the second is the fp64 dot-product error bound of K terms
(K u sum|h_k u_k|, u = 2^-53) for the kernel plus the same for the oracle.  It is derived, not measured;
test_resample_cpu.py prints how far the ordered loop stays under it.
"""

from __future__ import annotations

import math

import numpy as np

from ems_cases import make_recording  # noqa: F401  (the recordings: rows on a DC offset of 100, rows scaled to 1e-5)

REL_TOL = 2.0 ** -23


def geometry(L, up, down):
    """(up, down reduced, half, Q, K) of a prototype of L taps."""
    g = math.gcd(up, down)
    up, down = up // g, down // g
    assert L % 2 == 1 and up != down
    half = (L - 1) // 2
    return up, down, half, half // up, -(-L // up)


def out_length(N, up, down):
    g = math.gcd(up, down)
    return -(-N * (up // g) // (down // g))


def phase_table(h, up):
    """[K, up]: row j holds h[j up .. j up + up - 1], zeros past the prototype's end."""
    h = np.asarray(h, dtype=np.float64)
    K = -(-len(h) // up)
    t = np.zeros(K * up)
    t[:len(h)] = h
    return t.reshape(K, up)


def extend(x, L, up, ends, pad=None):
    """x [rows, N] -> (u [rows, pad + N + pad] float64, pad), u[:, pad + g] being sample g of the extended rows;
    pad defaults to K + 1, beyond anything a sum reads."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    rows, N = x.shape
    assert N >= 1 and ends in ("zero", "reflect_limited")
    half = (L - 1) // 2
    Q, K = half // up, -(-L // up)
    pad = K + 1 if pad is None else pad
    u = np.zeros((rows, N + 2 * pad))
    u[:, pad:pad + N] = x
    if ends == "reflect_limited":
        r = min(Q + 1, N - 1, pad)
        j = np.arange(1, r + 1)
        u[:, pad - j] = 2.0 * x[:, :1] - x[:, j]
        u[:, pad + N - 1 + j] = 2.0 * x[:, N - 1:] - x[:, N - 1 - j]
    return u, pad


def _positions(N, L, up, down):
    m = np.arange(-(-N * up // down), dtype=np.int64)
    c = m * down + (L - 1) // 2
    return c // up, c % up


def oracle_resample(x, h, up, down, ends="reflect_limited"):
    """float64 [rows, ceil(N up / down)]: every row of x [rows, N] resampled with the prototype taps h."""
    h = np.asarray(h, dtype=np.float64)
    up, down, half, Q, K = geometry(len(h), up, down)
    u, pad = extend(x, len(h), up, ends)
    tab = phase_table(h, up)
    q, p = _positions(np.shape(x)[1], len(h), up, down)
    y = np.zeros((u.shape[0], len(q)))
    back = np.arange(K)
    for ph in np.unique(p):
        idx = np.nonzero(p == ph)[0]
        y[:, idx] = u[:, (pad + q[idx])[:, None] - back[None, :]] @ tab[:, ph]
    return y


def ordered_resample(x, h, up, down, ends="reflect_limited"):
    """The same sum added term by term, j = 0..K-1 (ascending tap index), from a zero start: the kernel's order."""
    h = np.asarray(h, dtype=np.float64)
    up, down, half, Q, K = geometry(len(h), up, down)
    u, pad = extend(x, len(h), up, ends)
    tab = phase_table(h, up)
    q, p = _positions(np.shape(x)[1], len(h), up, down)
    acc = np.zeros((u.shape[0], len(q)))
    for j in range(K):
        acc = acc + tab[j, p][None, :] * u[:, pad + q - j]
    return acc


def resample_bound(x, h, up, down, ends, ref):
    """The bound of a comparison with ``ref`` = oracle_resample(x, h, up, down, ends), elementwise."""
    h = np.asarray(h, dtype=np.float64)
    up, down, half, Q, K = geometry(len(h), up, down)
    umax = np.abs(extend(x, len(h), up, ends)[0]).max(axis=1, keepdims=True)
    gain = np.abs(phase_table(h, up)).sum(axis=0).max()
    return REL_TOL * np.abs(ref) + 2.0 * K * 2.0 ** -53 * gain * umax


def assert_resample_close(got, ref, x, h, up, down, ends, name=""):
    """|got - ref| within resample_bound, elementwise; prints the worst case before it asserts."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    err = np.abs(got - ref)
    bound = resample_bound(x, h, up, down, ends, ref)
    worst = int(np.argmax(err - bound))
    print(f"{name}: max |diff| {err.max():.3e}; worst against its bound {err.flat[worst]:.3e} / {bound.flat[worst]:.3e}")
    assert (err <= bound).all(), f"{name}: {int((err > bound).sum())} of {err.size} beyond the bound"


def firwin_resampler(up, down):
    """``design_resampler`` restated with scipy: resample_poly's default anti-alias filter."""
    from scipy.signal import firwin
    g = math.gcd(up, down)
    up, down = up // g, down // g
    m = max(up, down)
    return firwin(2 * 10 * m + 1, 1.0 / m, window=("kaiser", 5.0)) * up


def asymmetric_taps(L, up, seed=7):
    """Random taps with no symmetry, of a gain near ``up``: a sum run the wrong way round gives another result."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(L) * np.linspace(1.0, 0.05, L) * up / np.sqrt(L)


def delta_taps(L, k, value):
    h = np.zeros(L)
    h[k] = value
    return h
