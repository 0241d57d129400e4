"""Zero-phase FIR filtering of recordings: the float64 oracle, an ordered restatement of the sum the kernel
runs, the bound every GPU comparison is held to, and the taps the tests use.

``oracle_fir`` builds each row extended as ``mne``'s 'reflect_limited' padding extends it --
u[-j] = 2 x[0] - x[j] and u[N-1+j] = 2 x[N-1] - x[N-1-j] for 1 <= j <= min(M, N - 1), zero beyond, M = (L - 1) / 2
-- and applies ``np.convolve(u, h, 'valid')``: y[t] = sum_k h[k] u[t + M - k].  ``ordered_fir`` adds the same
products tap by tap in the order k = 0..L-1, the kernel's order (without its fused multiply-add).  ``mne`` is
not installed where these tests run, so there is no ``mne`` fixture: the padding rule and the filter design
are restated from its documentation.

The bound: |gpu - oracle| <= 2^-23 |oracle| + 2 L 2^-53 sum|h| max|u|.  The first term is one fp32 ulp, for the
single final rounding; the second is the fp64 dot-product error bound of L terms (L u sum|h_k u_k|, u = 2^-53)
for the kernel plus the same for the oracle.  It is derived, not measured; test_fir_cpu.py prints how far the
ordered loop stays under it.
"""

from __future__ import annotations

import numpy as np

from ems_cases import make_recording  # noqa: F401  (the recordings: rows on a DC offset of 100, rows scaled to 1e-5)

REL_TOL = 2.0 ** -23


def extend(x, L):
    """x [rows, N] -> u [rows, N + 2 M] float64, u[:, M + g] being sample g of the extended rows."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    rows, N = x.shape
    assert L % 2 == 1 and N >= 1
    M = (L - 1) // 2
    r = min(M, N - 1)
    j = np.arange(1, r + 1)
    left = 2.0 * x[:, :1] - x[:, j[::-1]]                       # u[-r] .. u[-1]
    right = 2.0 * x[:, N - 1:] - x[:, N - 1 - j]                 # u[N] .. u[N-1+r]
    z = np.zeros((rows, M - r))
    return np.concatenate([z, left, x, right, z], axis=1)


def oracle_fir(x, h):
    """float64 [rows, N]: the zero-phase filter of every row of x [rows, N] with the taps h (odd length)."""
    h = np.asarray(h, dtype=np.float64)
    u = extend(x, len(h))
    return np.stack([np.convolve(row, h, "valid") for row in u])


def ordered_fir(x, h):
    """The same sum added tap by tap, k = 0..L-1, from a zero start: the kernel's order."""
    h = np.asarray(h, dtype=np.float64)
    L, N = len(h), np.shape(x)[1]
    M = (L - 1) // 2
    u = extend(x, L)
    acc = np.zeros((u.shape[0], N))
    for k in range(L):
        acc = acc + h[k] * u[:, 2 * M - k:2 * M - k + N]        # u[t + M - k] at padded index t + 2M - k
    return acc


def fir_bound(x, h, ref):
    """The bound of a comparison with ``ref`` = oracle_fir(x, h), elementwise [rows, N]."""
    h = np.asarray(h, dtype=np.float64)
    umax = np.abs(extend(x, len(h))).max(axis=1, keepdims=True)
    return REL_TOL * np.abs(ref) + 2.0 * len(h) * 2.0 ** -53 * np.abs(h).sum() * umax


def assert_fir_close(got, ref, x, h, name=""):
    """|got - ref| within fir_bound, elementwise; prints the worst case before it asserts."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    err = np.abs(got - ref)
    bound = fir_bound(x, h, ref)
    worst = int(np.argmax(err - bound))
    print(f"{name}: max |diff| {err.max():.3e}; worst against its bound {err.flat[worst]:.3e} / {bound.flat[worst]:.3e}")
    assert (err <= bound).all(), f"{name}: {int((err > bound).sum())} of {err.size} beyond the bound"


def firwin_bandpass(sfreq=128.0, l_freq=4.0, h_freq=38.0):
    """``design_bandpass`` restated with ``scipy.signal.firwin``: the rule ``mne`` documents for
    fir_design='firwin' -- the upper low-pass minus the lower one, each of its own odd length, centred."""
    from scipy.signal import firwin
    l_trans = min(max(0.25 * l_freq, 2.0), l_freq)
    h_trans = min(max(0.25 * h_freq, 2.0), sfreq / 2.0 - h_freq)
    odd = lambda n: n + 1 - n % 2
    n = odd(int(np.ceil(3.3 * sfreq / min(l_trans, h_trans))))
    h = np.zeros(n)
    for sign, cutoff, trans in ((1.0, h_freq + h_trans / 2.0, h_trans), (-1.0, l_freq - l_trans / 2.0, l_trans)):
        k = odd(int(round(3.3 * sfreq / trans)))
        off = (n - k) // 2
        h[off:n - off] += sign * firwin(k, cutoff, window="hamming", pass_zero=True, fs=sfreq)
    return h


def gain(h, f, sfreq):
    """|H(f)| of the taps h at sampling rate sfreq."""
    n = np.arange(len(h))
    return float(np.abs(np.sum(h * np.exp(-2j * np.pi * f / sfreq * n))))


def asymmetric_taps(L, seed=7):
    """Random taps with no symmetry: a convolution run the wrong way round gives another result."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(L) * np.linspace(1.0, 0.05, L) / np.sqrt(L)


def delta_taps(L, j):
    h = np.zeros(L)
    h[j] = 1.0
    return h
