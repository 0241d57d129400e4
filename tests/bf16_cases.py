"""The bf16 eval forward restated in float64 in the kernels' order, rounding to bf16 where they round.

``oracle.numpy_ref.forward(train=False)`` is the reference's arithmetic; the two bf16 kernels
(eegnet_infer_bf16.hip ``k_infer_bf16<PFU>``, eegnet_infer_bf16c.hip ``k_infer_bf16_cfg5``) reorder it --
eval BatchNorm is affine, so conv1 -> BN1 -> spatial collapses to spatial -> FIR -> affine -- and round some
operands and intermediates to bf16.  ``bf16_forward`` follows that order, folds BatchNorm as the kernel
prologues do and rounds a named quantity exactly when it is in ``points``:

    a1 = g1 / sqrt(rv1 + eps), c1 = b1 - a1 rm1, s2 = g2 / sqrt(rv2 + eps)
    al = a1 s2,  be = (c1 sum_c ws - rm2) s2 + b2          (ws NOT rounded in the sum: as the prologue)
    s3 = g3 / sqrt(rv3 + eps),  b3' = b3 - rm3 s3
    1. s = ws x                       2. v = FIR_w1(s), 'same' pad (K1-1)//2 | the rest
    3. a = pool4(ELU(al v + be))      4. z = depthwise_w2(a), pad 7 | 8
    5. r = W3 z                       6. h = pool8(ELU(s3 r + b3'))       7. logits = Wfc h + bfc

With ``points`` empty this is numpy_ref.forward to rounding error of float64 (test_bf16_cases_cpu.py), so
the difference between the two is what bf16 costs a case, and a quarter of it is the tolerance of the GPU
comparison (``tolerance``): nothing in it comes from a GPU result.

Rounding points, read from the kernel sources (every ``(__bf16)`` conversion and ``pack_bf16x2`` there):

    whole-trial kernel, eegnet_infer_bf16.hip          chunk kernel, eegnet_infer_bf16c.hip
    ws   wsf fragment, :194                            ws   :182
    W3   w3f fragment, :205                            W3   :189
    w1   af Toeplitz fragment, :287                    w1   af, :214
    s    s_store's pack_bf16x2, :231-232               s    :316-317
    z    step 3's pack_bf16x2, :352-353                z    :359-360
                                                       a    pooled rows kept as bf16, :274
                                                       w2   depthwise taps as an MFMA operand, :167

Everything else is fp32 in both: the input arrives as bf16 (the tests round it before the oracle sees it),
al / be / s3 / b3', the pooled rows a and the taps w2 of the whole-trial kernel (fp32 VALU depthwise), the
classifier weights and every accumulator.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from oracle import numpy_ref as nr

POINTS_NONE = frozenset()
POINTS_WHOLE = frozenset({"ws", "s", "w1", "z", "W3"})
POINTS_CFG5 = POINTS_WHOLE | {"a", "w2"}
ALL_POINTS = POINTS_CFG5

TOL_FACTOR = 0.25          # the GPU bound is this fraction of what all the bf16 roundings do to the logits
TOL_MAX = 1e-3             # a case whose tolerance() is above this is not admitted
PERTURB = 2.0 ** -21       # relative size of the noise-floor perturbation
N_UNIQUE = 7               # distinct trials of a multi-trial batch: coprime to every grid size used


def round_bf16(a):
    """float64 -> the nearest bf16 value (8 significand bits, ties to even, as ``(__bf16)`` rounds), as
    float64.  No subnormals or overflow: the activations here are of order 1."""
    m, e = np.frexp(np.asarray(a, dtype=np.float64))
    return np.ldexp(np.rint(m * 256.0), e - 8)


def _corr(a, w, left, right, dt):
    """out[..., t] = sum_k w[..., k] apad[..., t + k] with apad = a padded left | right, summed in ``dt``."""
    K = w.shape[-1]
    n = a.shape[-1] + left + right - K + 1
    ap = np.pad(a, [(0, 0)] * (a.ndim - 1) + [(left, right)])
    out = np.zeros(np.broadcast_shapes(a.shape[:-1], w.shape[:-1]) + (n,), dtype=dt)
    for k in range(K):
        out += w[..., k:k + 1] * ap[..., k:k + n]
    return out


def _elu(y):
    return np.where(y > 0, y, np.expm1(np.minimum(y, 0)))


def _pool(a, k):
    n = a.shape[-1] // k
    return a[..., :n * k].reshape(a.shape[:-1] + (n, k)).mean(axis=-1)


def bf16_forward(params, buffers, x, points, perturb=None, acc=np.float64, fir_pad=None, dw_pad=(7, 8),
                 pool_shift=0):
    """Logits [B, 4] (float64) of x [B, C, T] in the kernels' order; the quantities named in ``points``
    are rounded to bf16.

    ``perturb=(seed, eps)`` multiplies every activation by 1 + u eps, u uniform in [-1, 1], before its
    rounding point (the noise floor: roundings that fall the other way).  ``acc=np.float32`` does every
    sum and elementwise step after the BatchNorm folding in fp32, as the kernels' accumulators do.
    ``fir_pad``, ``dw_pad`` and ``pool_shift`` exist for the seeded defects (DEFECTS) only."""
    P = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    bf = {k: np.asarray(v, dtype=np.float64) for k, v in buffers.items()}
    x = np.asarray(x, dtype=np.float64)
    B, C, T = x.shape
    dm = nr.dims_from_params(params, C, T)
    F1, D, F2, K1 = dm.F1, dm.D, dm.F2, dm.K1
    rng = np.random.default_rng(perturb[0]) if perturb is not None else None

    def pt(name, a):
        if rng is not None and name not in ("ws", "w1", "w2", "W3"):
            a = a * (1.0 + perturb[1] * rng.uniform(-1.0, 1.0, a.shape)).astype(a.dtype)
        return round_bf16(a).astype(a.dtype) if name in points else a

    w1 = P["temporal.0.weight"].reshape(F1, K1)
    ws = P["spatial.weight"].reshape(F2, C)
    w2 = P["block_2.0.weight"].reshape(F2, nr.K2)
    W3 = P["block_2.1.weight"].reshape(F2, F2)
    Wfc, bfc = P["classifier.weight"], P["classifier.bias"]
    grp = np.arange(F2) // D
    a1 = P["temporal.1.weight"] / np.sqrt(bf["temporal.1.running_var"] + nr.BN_EPS)
    c1 = P["temporal.1.bias"] - a1 * bf["temporal.1.running_mean"]
    s2 = P["aggregation.0.weight"] / np.sqrt(bf["aggregation.0.running_var"] + nr.BN_EPS)
    al = a1[grp] * s2
    be = (c1[grp] * ws.sum(axis=1) - bf["aggregation.0.running_mean"]) * s2 + P["aggregation.0.bias"]
    s3 = P["block_2.2.weight"] / np.sqrt(bf["block_2.2.running_var"] + nr.BN_EPS)
    b3 = P["block_2.2.bias"] - bf["block_2.2.running_mean"] * s3

    c = lambda a: np.asarray(a, dtype=acc)
    s = pt("s", np.einsum("oc,bct->bot", c(pt("ws", ws)), c(x)))
    left, right = nr.same_pad(K1) if fir_pad is None else fir_pad
    v = pt("v", _corr(s, c(pt("w1", w1))[grp][None], left, right, acc))
    e = _elu(c(al)[None, :, None] * v + c(be)[None, :, None])
    if pool_shift:
        e = np.pad(e, [(0, 0), (0, 0), (0, pool_shift)])[..., pool_shift:]
    a = pt("a", _pool(e, nr.POOL1))
    z = pt("z", _corr(a, c(pt("w2", w2))[None], dw_pad[0], dw_pad[1], acc))
    r = pt("r", np.einsum("ji,bit->bjt", c(pt("W3", W3)), z))
    h = pt("h", _pool(_elu(c(s3)[None, :, None] * r + c(b3)[None, :, None]), nr.POOL2))
    return np.asarray(h.reshape(B, -1) @ c(Wfc).T + c(bfc), dtype=np.float64)


def rounding_effect(got, plain):
    """max |got - plain| / max |plain|."""
    return float(np.abs(got - plain).max() / np.abs(plain).max())


def tolerance(params, buffers, x, points, x0=None):
    """The relative bound of a GPU comparison on this case: a quarter of what all the bf16 roundings of
    ``points`` together do to its logits, over max |logits|.  With ``x0`` the same for the response
    logits(x) - logits(x0).

    Why a quarter: two correct fp32 implementations differ by about eps_fp32 / ulp_bf16 ~ 1e-4 of their
    roundings falling the other way, each such flip worth at most two typical rounding errors; in
    quadrature that is about 3 % of the total effect, and a quarter leaves about eight times that."""
    got, plain = (bf16_forward(params, buffers, x, pts) for pts in (points, POINTS_NONE))
    if x0 is not None:
        got = got - bf16_forward(params, buffers, x0, points)
        plain = plain - bf16_forward(params, buffers, x0, POINTS_NONE)
    return TOL_FACTOR * rounding_effect(got, plain)


@dataclass(frozen=True)
class Case:
    C: int
    T: int
    F1: int
    D: int
    K1: int
    points: frozenset
    branch: str
    chunk: bool = False        # the host picks k_infer_bf16_cfg5 (grid min(B, 2 CUs)), else min(B, CUs)
    seed: int = 0              # of the model; the input's is seed + 1

    @property
    def id(self):
        return f"{self.C}x{self.T}-F{self.F1}D{self.D}-K{self.K1}"


# PFU (geo_shape_bf16, eegnet_geometry.h): 0 when T % 8 != 0, else units = rup(C, 32) * rup(T, 128) / 8
# 16-byte units over 512 threads, rounded up to a power of two.  Re-derived on paper for every row:
#   64x512: 64*512/8 = 4096 -> 8          64x768: 64*768/8 = 6144 -> 12 -> 16 (units 12..15 of a thread lie
#   32x1000: 32*1024/8 = 4096 -> 8        past row CP = 64 for most threads: the c < CP guard of xi_store)
#   22x256 and 40x256: CP = 32 / 64, 32*256/8 = 1024 -> 2, 64*256/8 = 2048 -> 4
#   8x64: 32*128/8 = 512 -> 1             1x32: 32*128/8 = 512 -> 1        T = 257, 100: 0
# LDS of 64x512 F2 = 64 K1 = 64: x image 65536 + s rows 64*600*2 = 76800 + tables = 151680 B; the
# classifier's 16384 B no longer fit under 163840, so offF = 0 and Wfc is read from global memory.
CASES = [
    Case(64, 512, 16, 4, 32, POINTS_CFG5, "chunk kernel k_infer_bf16_cfg5", chunk=True),
    Case(64, 512, 8, 2, 32, POINTS_WHOLE, "PFU 8"),
    Case(64, 768, 8, 2, 32, POINTS_WHOLE, "PFU 16, 12 of 16 units live (c < CP guards)"),
    Case(32, 1000, 8, 2, 32, POINTS_WHOLE, "PFU 8, NT = 63, partial FIR block, T1 = 250, T2 = 31"),
    Case(64, 512, 16, 4, 64, POINTS_WHOLE, "whole-trial at F2 = 64, three FIR K-steps, offF == 0, PFU 8"),
    Case(22, 256, 8, 2, 64, POINTS_WHOLE, "K1 = 64 (KSF = 3, P = 31), PFU 2"),
    Case(22, 257, 8, 2, 64, POINTS_WHOLE, "K1 = 64, element staging (PFU 0)"),
    Case(22, 256, 8, 2, 32, POINTS_WHOLE, "PFU 2"),
    Case(22, 257, 8, 2, 32, POINTS_WHOLE, "PFU 0"),
    Case(8, 64, 8, 2, 32, POINTS_WHOLE, "PFU 1"),
    Case(40, 256, 12, 2, 32, POINTS_WHOLE, "F2 = 24 padded to 32, C = 40 (two K-steps), PFU 4", seed=3),
    Case(22, 256, 16, 1, 32, POINTS_WHOLE, "D = 1 (tap reload on every FIR row), PFU 2"),
    Case(22, 256, 4, 8, 32, POINTS_WHOLE, "D = 8 (one tap fragment over a wave's rows), PFU 2"),
    Case(1, 32, 2, 2, 32, POINTS_WHOLE, "smallest legal everything, F2 = 4 in a 16-row tile, PFU 1", seed=1),
    Case(8, 100, 8, 2, 32, POINTS_WHOLE, "T % 8 != 0, T1 = 25, T2 = 3, PFU 0"),
]
CASE_IDS = [c.id for c in CASES]
CFG5 = CASES[0]
CFG2 = CASES[7]
EDGE_CASES = [CASES[0], CASES[1]]          # the edge-response test: the chunk kernel and 64x512 EEGNet-8,2
B_CPU = N_UNIQUE                           # the CPU tests run the very trials the GPU test compares


def case_model(case):
    """The case's model (tests/hip_cases.random_model: default init, BatchNorm state off identity)."""
    from hip_cases import random_model
    return random_model(case.C, case.T, F1=case.F1, D=case.D, K1=case.K1, seed=1000 + case.seed).eval()


def case_input(case, B, seed=None):
    """[B, C, T] standard normal rounded to bf16 (float32 array of bf16-representable values)."""
    rng = np.random.default_rng(case.seed + 1 if seed is None else seed)
    return round_bf16(rng.standard_normal((B, case.C, case.T))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_oracle(case):
    """(params, buffers, x, plain, want, tol) of a case's B_CPU trials, computed once and shared: the
    logits with no rounding and with the case's rounding points, and tolerance() of them."""
    from hip_cases import state_np
    params, bufs = state_np(case_model(case))
    x = case_input(case, B_CPU)
    plain = bf16_forward(params, bufs, x, POINTS_NONE)
    want = bf16_forward(params, bufs, x, case.points)
    for a in (x, plain, want):
        a.setflags(write=False)
    return params, bufs, x, plain, want, TOL_FACTOR * rounding_effect(want, plain)


def dup_batch(n_unique, B, case, seed=None):
    """(xu, idx): ``n_unique`` distinct trials and the index of the trial that batch row b copies,
    idx[b] = b % n_unique.  With n_unique coprime to the grid every distinct trial meets every position of
    a workgroup's trial loop, and the oracle runs on n_unique trials only."""
    return case_input(case, n_unique, seed), np.arange(B) % n_unique


EDGE_AMP = 4.0


def edge_input(case, B, seed=None):
    """Zero but for random bf16 values at samples 0..15 and T-16..T-1 and, for the chunk kernel, at the
    four samples 64j-2..64j+1 around each chunk seam j = 1..7 (its halos).

    The values are EDGE_AMP = 4 standard deviations in size.  The roundings of a and z act on the whole of
    those planes, the part that the bias makes included, so against the response of so sparse an input they
    weigh more than against the logits: at unit amplitude the response is 2e-2 (cfg5) and 8e-3 (64x512
    EEGNet-8,2) beside logits of 0.25 and 0.12, and a quarter of the rounding effect on it is 1.2e-3 and
    3.6e-3, above TOL_MAX.  At 4 the response is a tenth and a third of the logits' size and the same
    figure is 5e-4 and 7e-4 (test_bf16_cases_cpu.py asserts the conditions for it)."""
    rng = np.random.default_rng(case.seed + 2 if seed is None else seed)
    t = list(range(16)) + list(range(case.T - 16, case.T))
    if case.chunk:
        t += [64 * j + d for j in range(1, 8) for d in (-2, -1, 0, 1)]
    x = np.zeros((B, case.C, case.T), dtype=np.float32)
    x[:, :, t] = round_bf16(EDGE_AMP * rng.standard_normal((B, case.C, len(t))))
    return x


# ---- seeded defects: each returns (params, x, keyword arguments of bf16_forward) ----

def _with(params, name, fn):
    p = dict(params)
    w = np.array(p[name], dtype=np.float64, copy=True)
    fn(w)
    p[name] = w
    return p


def _zero(w, idx):
    w[idx] = 0.0


def _zero_x(x, sl):
    x = np.array(x, copy=True)
    x[:, :, sl] = 0.0
    return x


DEFECTS = {
    "first temporal tap dropped": lambda p, x: (_with(p, "temporal.0.weight", lambda w: _zero(w, (..., 0))), x, {}),
    "last temporal tap dropped": lambda p, x: (_with(p, "temporal.0.weight", lambda w: _zero(w, (..., -1))), x, {}),
    "last electrode dropped": lambda p, x: (_with(p, "spatial.weight", lambda w: _zero(w, (slice(None), 0, -1, 0))), x, {}),
    "depthwise tap 0 dropped": lambda p, x: (_with(p, "block_2.0.weight", lambda w: _zero(w, (..., 0))), x, {}),
    "depthwise tap 15 dropped": lambda p, x: (_with(p, "block_2.0.weight", lambda w: _zero(w, (..., 15))), x, {}),
    "sample column t = 0 zeroed": lambda p, x: (p, _zero_x(x, 0), {}),
    "sample column t = 63 zeroed": lambda p, x: (p, _zero_x(x, 63), {}),
    "sample column t = 64 zeroed": lambda p, x: (p, _zero_x(x, 64), {}),
    "sample column t = T - 1 zeroed": lambda p, x: (p, _zero_x(x, -1), {}),
    "last 16 samples zeroed": lambda p, x: (p, _zero_x(x, slice(-16, None)), {}),
    "last classifier column dropped": lambda p, x: (_with(p, "classifier.weight", lambda w: _zero(w, (slice(None), -1))), x, {}),
    "FIR 'same' pad 16 | 15": lambda p, x: (p, x, {"fir_pad": (16, 15)}),
    "depthwise pad 8 | 7": lambda p, x: (p, x, {"dw_pad": (8, 7)}),
    "pool4 over samples 4q+1 .. 4q+4": lambda p, x: (p, x, {"pool_shift": 1}),
}
DEFECT_CASES = [CFG5, CFG2]


def assert_within(got, want, tol, scale, what):
    """|got - want| <= tol * scale elementwise; prints the figures before it asserts."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite logits"
    err = float(np.abs(got - want).max())
    print(f"{what}: max |gpu - oracle| {err:.3e} = {err / scale:.3e} of the scale {scale:.3e}; tolerance {tol:.3e}")
    assert err <= tol * scale, (f"{what}: max |gpu - oracle| {err:.3e} is {err / scale:.3e} of {scale:.3e}, "
                                f"above tolerance(case) = {tol:.3e}")
