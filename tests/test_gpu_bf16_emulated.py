"""The two bf16 eval kernels (eegnet_infer_bf16.hip k_infer_bf16<PFU>, eegnet_infer_bf16c.hip
k_infer_bf16_cfg5) against the rounding-aware float64 oracle of tests/bf16_cases.py.

Every numerical assertion is

    |gpu - bf16_forward(points)| <= tolerance(case) * max |ref|,  elementwise,

with ``tolerance(case)`` a quarter of what all the bf16 roundings do to that case's logits: 8.7e-5 .. 5.6e-4
here, from the oracle alone (test_bf16_cases_cpu.py shows that it is at most 1e-3, at least twice the noise
floor of a correct fp32 implementation, and a quarter of the smallest seeded defect or less).  The 2e-2 of
test_gpu_bf16_infer.py is SURVEY's contract; this file is the one that sees a dropped tap or a lost column.

Every case of the table (bf16_cases.CASES, each row naming the branch it exists for) runs at
B = 2 * grid + 3 trials, so that some workgroups run three trials and the rest two: the prefetch re-arm,
the re-staging of x over the aliased a / z planes, the chunk kernel's hand-over of the first chunk.  The batch
repeats 7 distinct trials (7 is coprime to the grid), the first seven rows are checked against the oracle
and every row must carry the bits of the first row with its input.

Reached: PFU 0 (22x257 at both K1, 8x100), 1 (8x64, 1x32), 2 (22x256 at both K1, D = 1, D = 8), 4 (40x256),
8 (64x512 EEGNet-8,2, 32x1000, 64x512 K1 = 64), 16 (64x768); K1 = 64 (three rows); offF == 0 (64x512
EEGNet-16,4 K1 = 64); the chunk kernel (cfg5).
"""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import bf16_cases as bc

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _bf16(x_np, dev):
    """float32 array of bf16-representable values -> bf16 tensor on ``dev`` (exact)."""
    t = torch.from_numpy(np.array(x_np, dtype=np.float32))          # a copy: the shared oracle arrays are read-only
    assert torch.equal(t.to(torch.bfloat16).float(), t)
    return t.to(torch.bfloat16).to(dev)


def _grid(case, B, dev):
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    return min(B, (2 if case.chunk else 1) * n_cu)


@pytest.mark.parametrize("case", bc.CASES, ids=bc.CASE_IDS)
def test_every_trial_of_a_multi_trial_batch(case):
    dev = _dev()
    grid = _grid(case, 1 << 30, dev)
    B = 2 * grid + 3
    assert math.gcd(bc.N_UNIQUE, grid) == 1 and _grid(case, B, dev) == grid
    _, _, xu, plain, want, tol = bc.case_oracle(case)
    xu2, idx = bc.dup_batch(bc.N_UNIQUE, B, case)
    assert np.array_equal(xu2, xu)
    m = bc.case_model(case).to(dev)
    idx_d = torch.from_numpy(idx).to(dev)
    x = _bf16(xu, dev)[idx_d].contiguous()
    assert x.shape == (B, case.C, case.T) and x.data_ptr() % 16 == 0
    with torch.no_grad():
        out = m(x)
    torch.cuda.synchronize()
    assert out.shape == (B, 4) and out.dtype == torch.float32
    bc.assert_within(out[:bc.N_UNIQUE].cpu().numpy(), want, tol, float(np.abs(plain).max()),
                     f"{case.id} ({case.branch}), B = {B} over {grid} workgroups")
    same = (out == out[:bc.N_UNIQUE][idx_d]).all(dim=1)
    assert bool(same.all()), (f"{case.id}: {int((~same).sum())} of {B} trials differ from the first trial with "
                              f"their input, first at b = {int(torch.nonzero(~same)[0])} (grid {grid})")


@pytest.mark.parametrize("case", bc.EDGE_CASES, ids=[c.id for c in bc.EDGE_CASES])
def test_edge_response(case):
    """Input that is zero but at the first and last 16 samples and, for the chunk kernel, around its seven
    chunk seams: the response logits(x) - logits(0) against the oracle's, to the tolerance taken on the
    response (bf16_cases.edge_input says why) times max |oracle response|."""
    dev = _dev()
    params, bufs = bc.case_oracle(case)[:2]
    x = bc.edge_input(case, bc.B_CPU)
    x0 = np.zeros((1, case.C, case.T), dtype=np.float32)

    def resp(points):
        return bc.bf16_forward(params, bufs, x, points) - bc.bf16_forward(params, bufs, x0, points)

    plain, want = resp(bc.POINTS_NONE), resp(case.points)
    scale = float(np.abs(plain).max())
    assert scale > 0.0 and np.abs(want).max() > 0.0, "the oracle does not respond to the edges"
    tol = bc.TOL_FACTOR * bc.rounding_effect(want, plain)
    assert 0.0 < tol <= bc.TOL_MAX
    m = bc.case_model(case).to(dev)
    with torch.no_grad():
        out = m(_bf16(np.concatenate([x, x0]), dev)).cpu().numpy().astype(np.float64)
    bc.assert_within(out[:-1] - out[-1:], want, tol, scale, f"{case.id} edge response")


def _offset_view(x, buf_elems, off):
    """x [B, C, T] copied into a contiguous view ``off`` elements into a 16-byte-aligned buffer."""
    buf = torch.zeros(buf_elems, dtype=torch.bfloat16, device=x.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + 2 * off
    return v


@pytest.mark.parametrize("off", [1, 4])
def test_misaligned_x_is_refused_on_the_16_byte_path(off):
    """T % 8 == 0 stages x in 16-byte loads (PFU > 0): the host refuses an x that is not 16-byte aligned
    (eegnet_forward_eval_bf16) before anything is launched."""
    dev = _dev()
    case = bc.CFG2
    x = _bf16(bc.case_oracle(case)[2], dev)
    v = _offset_view(x, x.numel() + 16, off)
    m = bc.case_model(case).to(dev)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        m(v)
    torch.cuda.synchronize()


def test_two_byte_aligned_x_runs_on_the_element_path():
    """T % 8 != 0 stages x element by element (PFU 0): an x one element into a buffer is as good as any."""
    dev = _dev()
    case = next(c for c in bc.CASES if (c.T, c.K1) == (257, 32))
    _, _, xu, plain, want, tol = bc.case_oracle(case)
    x = _bf16(xu, dev)
    v = _offset_view(x, x.numel() + 16, 1)
    assert v.data_ptr() % 16 == 2
    m = bc.case_model(case).to(dev)
    with torch.no_grad():
        out = m(v)
        ref = m(x)
    torch.cuda.synchronize()
    bc.assert_within(out.cpu().numpy(), want, tol, float(np.abs(plain).max()), f"{case.id} at a 2-byte offset")
    assert torch.equal(out, ref), "the logits depend on the alignment of x"
