"""Exponential moving standardisation: the float64 oracle, a numpy restatement of the blocked algorithm
the kernels run, and the recordings the tests feed both.

``oracle_ems`` restates the reference's ``raw_exponential_moving_standardize`` (dataset.py:45-70) sample
by sample in float64 and also returns the final state; it reproduces ``golden/ems/EMS1.npz``, written by
the reference's own function, bit for bit.  ``blocked_ems`` follows eegnet_ems.hip step for step (chunks,
the three carry-independent scans of the aggregates, the walk over the chunks, the output pass) with the
thread-level scans done serially: it prices the reassociation error of the blocked form against the
oracle without a GPU.
"""

from __future__ import annotations

import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EMS1 = os.path.join(HERE, "golden", "ems", "EMS1.npz")

FACTOR_NEW, INIT_BLOCK, EPS = 1e-3, 1000, 1e-10          # the reference's defaults (eps is a literal there)

# The bound of every GPU comparison: |gpu - oracle| <= 2^-23 |oracle| + ABS_TOL.  The first term is one fp32
# ulp, for a flip at the boundary of the single final rounding; the second bounds the fp64 reassociation
# error of the blocked scan (measured with blocked_ems on these inputs: test_ems_cpu.py).
REL_TOL, ABS_TOL = 2.0 ** -23, 1e-9
STATE_RTOL = 1e-11


def oracle_ems(x, factor_new=FACTOR_NEW, init_block_size=INIT_BLOCK, eps=EPS, state=None):
    """(y, state) for x [rows, N]: y float64 [rows, N], state float64 [rows, 2] = the final (mean, var).
    ``state`` given: start from it instead of from the first ``init_block_size`` samples."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    rows, N = x.shape
    if state is None:
        head = x[:, :init_block_size]
        m = np.mean(head, axis=1, keepdims=True)
        v = np.var(head, axis=1, keepdims=True)
    else:
        state = np.asarray(state, dtype=np.float64)
        m, v = state[:, 0:1].copy(), state[:, 1:2].copy()
    y = np.zeros_like(x)
    for t in range(N):
        xt = x[:, t:t + 1]
        m = (1 - factor_new) * m + factor_new * xt
        v = (1 - factor_new) * v + factor_new * (xt - m) ** 2
        y[:, t:t + 1] = (xt - m) / np.sqrt(v + eps)
    return y, np.concatenate([m, v], axis=1)


def _scan(vals, p, start):
    """s_k = p s_{k-1} + vals_k from s_{-1} = start, per row: [rows, n] -> [rows, n]."""
    out = np.empty_like(vals)
    s = start
    for k in range(vals.shape[1]):
        s = p * s + vals[:, k]
        out[:, k] = s
    return out


def blocked_ems(x, L, factor_new=FACTOR_NEW, init_block_size=INIT_BLOCK, eps=EPS, state=None):
    """The algorithm of eegnet_ems.hip in float64 numpy, chunks of L samples: (y, state) as oracle_ems."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    rows, N = x.shape
    a, p = factor_new, 1 - factor_new
    zero = np.zeros(rows)
    if state is None:
        head = x[:, :init_block_size]
        m = head.sum(1) / head.shape[1]
        v = ((head - m[:, None]) ** 2).sum(1) / head.shape[1]
    else:
        m, v = np.array(state[:, 0], dtype=np.float64), np.array(state[:, 1], dtype=np.float64)
    chunks = [(t0, min(L, N - t0)) for t0 in range(0, N, L)]
    # k_ems_agg: per chunk r, A, S0, E from a zero start
    agg = []
    for t0, n in chunks:
        r = x[:, t0]
        xs = x[:, t0:t0 + n] - r[:, None]
        loc = _scan(a * xs, p, zero)
        e = xs - loc
        agg.append((r, loc[:, -1], _scan(a * e * e, p, zero)[:, -1], e.sum(1)))
    # k_ems_carry: the (m, v) every chunk is entered with
    carry = []
    for (t0, n), (r, A, S0, E) in zip(chunks, agg):
        carry.append((m, v))
        pn, c = p ** n, m - r
        m = r + A + c * pn
        v = pn * (v - 2.0 * c * a * E + c * c * p * (1.0 - pn)) + S0
    # k_ems_out: the scans from the true carries
    y = np.empty_like(x)
    for (t0, n), (r, _, _, _), (m_in, v_in) in zip(chunks, agg, carry):
        xs = x[:, t0:t0 + n] - r[:, None]
        d = xs - _scan(a * xs, p, m_in - r)
        y[:, t0:t0 + n] = d / np.sqrt(_scan(a * d * d, p, v_in) + eps)
    return y, np.stack([m, v], axis=1)


def make_recording(rows, N, seed, dtype=np.float32):
    """[rows, N] of unit noise plus a slow drift.  Row i with i % 3 == 1 rides on a DC offset of 100
    standard deviations; row i with i % 3 == 2 is scaled to 1e-5, where eps = 1e-10 is of the variance's
    size."""
    rng = np.random.default_rng(seed)
    t = np.arange(N, dtype=np.float64)
    x = rng.standard_normal((rows, N))
    x += 0.5 * np.sin(2 * np.pi * t / 700.0 + rng.uniform(0, 6.0, (rows, 1))) + 3e-4 * t * rng.uniform(-1, 1, (rows, 1))
    i = np.arange(rows)
    x[i % 3 == 1] += 100.0
    x[i % 3 == 2] *= 1e-5
    return np.ascontiguousarray(x.astype(dtype))


# the fixture: 3 rows x 2600 float64 samples, rows 1 and 2 on DC offsets; regenerated, never stored
EMS1_ROWS, EMS1_N, EMS1_SEED = 3, 2600, 4501


def ems1_input():
    rng = np.random.default_rng(EMS1_SEED)
    x = rng.standard_normal((EMS1_ROWS, EMS1_N))
    x += 0.5 * np.sin(np.arange(EMS1_N) / 90.0)
    x[1] += 100.0
    x[2] = 3.0 * x[2] - 250.0
    return np.ascontiguousarray(x)


def assert_ems_close(got, ref, name=""):
    """|got - ref| <= 2^-23 |ref| + 1e-9, elementwise; prints the worst excess before it asserts."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    err = np.abs(got - ref)
    bound = REL_TOL * np.abs(ref) + ABS_TOL
    worst = int(np.argmax(err - bound))
    print(f"{name}: max |diff| {err.max():.3e}; worst against its bound {err.flat[worst]:.3e} / {bound.flat[worst]:.3e}")
    assert (err <= bound).all(), f"{name}: {int((err > bound).sum())} of {err.size} beyond the bound"


def assert_state_close(got, ref, name=""):
    got = np.asarray(got, dtype=np.float64)
    rel = np.abs(got - ref) / np.abs(ref)
    print(f"{name}: state max relative error {rel.max():.3e}")
    assert (rel <= STATE_RTOL).all(), f"{name}: state relative error {rel.max():.3e} > {STATE_RTOL}"
