"""The rounding-aware oracle of the bf16 eval kernels (tests/bf16_cases.py) has teeth and a known floor.

No GPU: everything here is float64 / float32 numpy on the very trials that test_gpu_bf16_emulated.py sends
to the kernels.  Three things are shown for every case of the table:

* with no rounding point, ``bf16_forward`` is ``oracle.numpy_ref.forward(train=False)`` to 1e-12: the
  reordering (spatial before temporal) and the BatchNorm folding are exact;
* ``tolerance()`` -- a quarter of what all bf16 roundings do to the case's logits -- is at most 1e-3, and
  what a correct fp32 implementation may differ by stays under half of it: roundings falling the other
  way (every activation perturbed by 2^-21, the worst of 8 seeds) and fp32 instead of fp64 accumulation;
* at cfg5 and 22 x 256, each seeded defect moves the logits by more than four tolerances.

The conditions are fixed; a case that misses one gets another seed (bf16_cases.Case.seed), never a wider
condition.  Figures on these inputs: tolerance 8.7e-5 .. 5.6e-4, floor <= 0.33 tolerance, smallest seeded
defect 15 tolerances (cfg5, sample column 0 zeroed) and 27 (22 x 256, column 63).
"""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import bf16_cases as bc
from oracle import numpy_ref as nr

N_SEEDS = 8


_case = bc.case_oracle


def _conditions(what, tol, floor, f32):
    print(f"{what}: tolerance {tol:.3e}, perturbation floor {floor:.3e} ({floor / tol:.2f} of it), "
          f"fp32 accumulation {f32:.3e} ({f32 / tol:.2f} of it)")
    assert 0.0 < tol <= bc.TOL_MAX, f"{what}: tolerance {tol:.3e} not in (0, {bc.TOL_MAX}]"
    assert floor <= tol / 2, f"{what}: perturbation floor {floor:.3e} > tolerance / 2 = {tol / 2:.3e}"
    assert f32 <= tol / 2, f"{what}: fp32 accumulation {f32:.3e} > tolerance / 2 = {tol / 2:.3e}"


def test_round_bf16_is_round_to_nearest_even():
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.standard_normal(20000) * 10.0 ** rng.integers(-6, 6, 20000),
                        [0.0, 1.0, -1.0, 1.00390625, 1.01171875, 255.5, 0.99804688]]).astype(np.float32)
    want = torch.from_numpy(v).to(torch.bfloat16).float().numpy()
    assert np.array_equal(bc.round_bf16(v), want.astype(np.float64))
    # ties: 1 + 2^-8 lies between 1 and 1 + 2^-7 -> even (1); 1 + 3 * 2^-8 -> 1 + 2^-6
    assert bc.round_bf16(1.0 + 2.0 ** -8) == 1.0 and bc.round_bf16(1.0 + 3 * 2.0 ** -8) == 1.0 + 2.0 ** -6


def test_point_sets():
    assert bc.POINTS_WHOLE == {"ws", "s", "w1", "z", "W3"}
    assert bc.POINTS_CFG5 == bc.POINTS_WHOLE | {"a", "w2"}
    assert [c.points for c in bc.CASES].count(bc.POINTS_CFG5) == 1 and bc.CFG5.chunk
    assert all(c.branch for c in bc.CASES) and len(set(bc.CASE_IDS)) == len(bc.CASES) == 15


@pytest.mark.parametrize("case", bc.CASES, ids=bc.CASE_IDS)
def test_without_rounding_it_is_the_float64_oracle(case):
    params, bufs, x, plain, _, _ = _case(case)
    ref = nr.forward(params, bufs, x, train=False)[0]
    err = bc.rounding_effect(plain, ref)
    print(f"{case.id}: max |bf16_forward(no points) - numpy_ref| / max |ref| = {err:.2e}")
    assert plain.shape == ref.shape == (bc.B_CPU, 4) and err <= 1e-12


@pytest.mark.parametrize("case", bc.CASES, ids=bc.CASE_IDS)
def test_tolerance_is_tight_and_above_the_floor(case):
    params, bufs, x, plain, got, tol = _case(case)
    assert tol == bc.tolerance(params, bufs, x, case.points)
    floor = max(bc.rounding_effect(bc.bf16_forward(params, bufs, x, case.points, perturb=(seed, bc.PERTURB)), got)
                for seed in range(N_SEEDS))
    f32 = bc.rounding_effect(bc.bf16_forward(params, bufs, x, case.points, acc=np.float32), got)
    _conditions(case.id, tol, floor, f32)


@pytest.mark.parametrize("defect", list(bc.DEFECTS))
@pytest.mark.parametrize("case", bc.DEFECT_CASES, ids=[c.id for c in bc.DEFECT_CASES])
def test_seeded_defect_is_seen(case, defect):
    params, bufs, x, _, got, tol = _case(case)
    p2, x2, kw = bc.DEFECTS[defect](params, x)
    dev = bc.rounding_effect(bc.bf16_forward(p2, bufs, x2, case.points, **kw), got)
    print(f"{case.id}, {defect}: {dev:.3e} = {dev / tol:.1f} tolerances")
    assert dev > 4 * tol, f"{case.id}, {defect}: moves the logits by {dev:.3e}, not above 4 * {tol:.3e}"


@pytest.mark.parametrize("case", bc.EDGE_CASES, ids=[c.id for c in bc.EDGE_CASES])
def test_edge_response_conditions(case):
    """The edge-response input of the GPU test: its tolerance is taken on the response logits(x) -
    logits(0), and the three conditions hold for that."""
    params, bufs = _case(case)[:2]
    x, x0 = bc.edge_input(case, bc.B_CPU), np.zeros((1, case.C, case.T), dtype=np.float32)
    on = np.nonzero(np.abs(x).sum(axis=(0, 1)))[0]
    seams = [64 * j + d for j in range(1, 8) for d in (-2, -1, 0, 1)] if case.chunk else []
    assert sorted(on) == sorted(list(range(16)) + seams + list(range(case.T - 16, case.T)))

    def resp(points, **kw):
        return bc.bf16_forward(params, bufs, x, points, **kw) - bc.bf16_forward(params, bufs, x0, points, **kw)

    plain, got = resp(bc.POINTS_NONE), resp(case.points)
    assert np.abs(plain).max() > 0.05 * np.abs(bc.bf16_forward(params, bufs, x0, bc.POINTS_NONE)).max()
    tol = bc.TOL_FACTOR * bc.rounding_effect(got, plain)
    assert math.isclose(tol, bc.tolerance(params, bufs, x, case.points, x0=x0), rel_tol=1e-9)
    floor = max(bc.rounding_effect(resp(case.points, perturb=(seed, bc.PERTURB)), got) for seed in range(N_SEEDS))
    f32 = bc.rounding_effect(resp(case.points, acc=np.float32), got)
    _conditions(f"{case.id} edge response", tol, floor, f32)


def test_dup_batch_meets_every_position():
    case = bc.CFG2
    for grid in (256, 512, 304, 608):
        B = 2 * grid + 3
        xu, idx = bc.dup_batch(bc.N_UNIQUE, B, case)
        assert xu.shape == (bc.N_UNIQUE, case.C, case.T) and np.array_equal(xu, bc.case_input(case, bc.B_CPU))
        assert math.gcd(bc.N_UNIQUE, grid) == 1 and np.array_equal(idx[:bc.N_UNIQUE], np.arange(bc.N_UNIQUE))
        # workgroup w runs trials w, w + grid (and w + 2 grid for w < 3).  A trial's position: (trials its
        # workgroup ran before it, trials it runs after it).  Every distinct trial is first with a prefetch
        # behind it and last with none; the three-trial workgroups add the middle positions
        pos = [{(b // grid, (B - 1 - b) // grid) for b in np.nonzero(idx == u)[0]} for u in range(bc.N_UNIQUE)]
        assert all({(0, 1), (1, 0)} <= p for p in pos), (grid, pos)
        assert set().union(*pos) == {(0, 2), (1, 1), (2, 0), (0, 1), (1, 0)}
