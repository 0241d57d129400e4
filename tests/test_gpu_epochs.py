"""Cue epoching in place (eegnet_forward_eval_windows_at: k_infer_win's table variant) on the GPU.

The kernel is k_infer_win with the window origin read from a table, and no arithmetic crosses windows, so the
bar for the logits is bit-equality with ``ops.forward_eval`` on the windows copied out into a contiguous
batch.  The whole chain -- band-pass, standardisation, epochs -- is held to the float64 oracles of its three
steps within a tolerance measured on the oracle side alone (test_whole_chain_against_the_oracles)."""

from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"22x256": (22, 256), "22x257": (22, 257)}
_models = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _model(C, T, dev, seed=3):
    from hip_cases import random_model
    key = (C, T, seed)
    if key not in _models:
        _models[key] = random_model(C, T, seed=seed).to(dev).eval()
    return _models[key]


def _rec_np(R, C, N, seed):
    return np.random.default_rng(seed).standard_normal((R, C, N), dtype=np.float32)


def _copied(m, rec, starts, idx):
    """forward_eval on the windows copied out: [W, 4]."""
    from eegnetreplication_amd import ops
    x = torch.stack([rec[r, :, s:s + m.T] for s, r in zip(starts, idx)]).contiguous()
    return ops.forward_eval(m.shape, m.flat_parameters(), m.flat_bn_buffers(), x)


def _table(T, N, R, seed):
    """Starts covering 0, 1, 2, 3 mod 4, the last start N - T and its neighbours, and a shuffled rec_index."""
    last = N - T
    starts = [0, 1, 2, 3, 4, 5, 6, 7, T // 2, T // 2 + 1, T, T + 2, T + 3, last - 3, last - 2, last - 1, last, 0, last]
    rng = np.random.default_rng(seed)
    idx = rng.permutation(np.arange(len(starts)) % R)
    assert {s % 4 for s in starts} == {0, 1, 2, 3} and set(idx.tolist()) == set(range(R))
    return starts, idx.tolist()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_logits_bit_equal_to_forward_eval_on_the_copied_windows(shape):
    """R = 3 recordings of 4T + 37 samples, contiguous and as a time slice that starts one float into a
    NaN-filled buffer (a load outside the slice would turn a logit into NaN); host tables (a list, numpy, a
    CPU tensor) and device tables give the same bits."""
    from eegnetreplication_amd import epoch_logits
    dev = _dev()
    C, T = SHAPES[shape]
    m = _model(C, T, dev)
    R, N = 3, 4 * T + 37
    rec = torch.from_numpy(_rec_np(R, C, N, 51)).to(dev)
    starts, idx = _table(T, N, R, 52)
    ref = _copied(m, rec, starts, idx)
    got = epoch_logits(m, rec, starts, idx)
    assert got.shape == (len(starts), 4) and got.dtype == torch.float32
    assert torch.isfinite(got).all()
    assert torch.equal(got, ref), f"max |diff| {(got - ref).abs().max().item():.3e}"
    assert torch.equal(epoch_logits(m, rec, np.array(starts), np.array(idx, dtype=np.int32)), ref)
    assert torch.equal(epoch_logits(m, rec, torch.tensor(starts), torch.tensor(idx)), ref)
    ds = torch.tensor(starts, dtype=torch.int64, device=dev)
    di = torch.tensor(idx, dtype=torch.int32, device=dev)
    assert torch.equal(epoch_logits(m, rec, ds, di), ref)
    # the misaligned slice: pitch N + 7 (odd), one float in
    buf = torch.full((R, C, N + 7), float("nan"), dtype=torch.float32, device=dev)
    view = buf[:, :, 1:1 + N]
    view.copy_(rec)
    assert not view.is_contiguous() and view.data_ptr() % 16 == 4
    assert torch.equal(epoch_logits(m, view, ds, di), ref)
    # an aligned slice at a pitch that is a multiple of 4: the 16-byte loads where a start allows them
    buf4 = torch.full((R, C, N + 11), float("nan"), dtype=torch.float32, device=dev)
    assert (N + 11) % 4 == 0
    view4 = buf4[:, :, 4:4 + N]
    view4.copy_(rec)
    assert torch.equal(epoch_logits(m, view4, ds, di), ref)
    # recording 0 when there is no rec_index, and a 2-D recording
    ref0 = _copied(m, rec, starts, [0] * len(starts))
    assert torch.equal(epoch_logits(m, rec, starts), ref0)
    assert torch.equal(epoch_logits(m, rec[0], ds), ref0)
    assert epoch_logits(m, rec, []).shape == (0, 4)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("hop", [1, 4, 37])
def test_starts_on_a_hop_grid_reproduce_sliding_logits(shape, hop):
    from eegnetreplication_amd import epoch_logits, sliding_logits, window_starts
    dev = _dev()
    C, T = SHAPES[shape]
    m = _model(C, T, dev)
    R, N = 2, T + 40 * hop + min(hop - 1, 2)
    rec = torch.from_numpy(_rec_np(R, C, N, 60 + hop)).to(dev)
    want = sliding_logits(m, rec, hop)                               # [R, W, 4]
    st = window_starts(N, T, hop)
    W = len(st)
    assert want.shape == (R, W, 4)
    got = epoch_logits(m, rec, st.repeat(R), torch.arange(R).repeat_interleave(W))
    assert torch.equal(got.view(R, W, 4), want)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_device_table_is_read_clamped(shape):
    """Device tables are never read by the host, so the kernel clamps them: starts -5 and N give the logits at
    0 and N - T, recording indices -1 and R those of recordings 0 and R - 1.  Every load stays inside the
    recordings -- the recordings sit in the middle of a NaN-filled buffer, and the logits are finite."""
    from eegnetreplication_amd import epoch_logits
    dev = _dev()
    C, T = SHAPES[shape]
    m = _model(C, T, dev)
    R, N = 3, 2 * T + 21
    buf = torch.full((R + 2, C, N + 8), float("nan"), dtype=torch.float32, device=dev)
    rec = buf[1:1 + R, :, 4:4 + N]
    rec.copy_(torch.from_numpy(_rec_np(R, C, N, 71)).to(dev))
    last = N - T
    ds = torch.tensor([-5, N, last + 1, -(1 << 40), 1 << 40, 7, 7], dtype=torch.int64, device=dev)
    di = torch.tensor([1, 1, 2, 0, 2, -1, R], dtype=torch.int32, device=dev)
    got = epoch_logits(m, rec, ds, di)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    want = epoch_logits(m, rec, [0, last, last, 0, last, 7, 7], [1, 1, 2, 0, 2, 0, R - 1])
    assert torch.equal(got, want)
    assert torch.equal(want, _copied(m, rec, [0, last, last, 0, last, 7, 7], [1, 1, 2, 0, 2, 0, R - 1]))


def test_more_windows_than_workgroups_and_two_calls():
    """600 windows: above one per CU, so the strided loop and the prefetch of the next window run."""
    from eegnetreplication_amd import epoch_logits
    dev = _dev()
    C, T = SHAPES["22x257"]
    m = _model(C, T, dev)
    R, N = 3, T + 700
    rec = torch.from_numpy(_rec_np(R, C, N, 81)).to(dev)
    rng = np.random.default_rng(82)
    starts = rng.integers(0, N - T + 1, 600).tolist()
    idx = rng.integers(0, R, 600).tolist()
    got = epoch_logits(m, rec, starts, idx)
    assert torch.equal(got, _copied(m, rec, starts, idx))
    assert torch.equal(got, epoch_logits(m, rec, starts, idx))


def test_graph_capture_with_device_tables():
    from eegnetreplication_amd import epoch_logits
    dev = _dev()
    C, T = SHAPES["22x257"]
    m = _model(C, T, dev)
    R, N = 2, T + 300
    rec = torch.from_numpy(_rec_np(R, C, N, 91)).to(dev)
    ds = torch.tensor([0, 64, 300, 17], dtype=torch.int64, device=dev)
    di = torch.tensor([0, 1, 1, 0], dtype=torch.int32, device=dev)
    epoch_logits(m, rec, ds, di)                                     # eager once: the kernel's attributes are set
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = epoch_logits(m, rec, ds, di)
    rec.copy_(torch.from_numpy(_rec_np(R, C, N, 92)).to(dev))
    ds.copy_(torch.tensor([5, 300, 1, 128], dtype=torch.int64))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.clone(), epoch_logits(m, rec, ds, di))


def test_wide_models_are_refused():
    from eegnetreplication_amd import EEGNet, epoch_logits
    dev = _dev()
    wide = EEGNet(64, 512, F1=16, D=4).to(dev).eval()
    with pytest.raises(NotImplementedError, match="F1\\*D = 64 > 16 is not supported"):
        epoch_logits(wide, torch.zeros((64, 1024), device=dev), [0, 5])


def test_whole_chain_against_the_oracles():
    """preprocess_recording -> epoch_logits on raw recordings against oracle_fir -> oracle_ems -> the copied
    windows (rounded to float32) -> forward_eval, at the reference's epochs (257 samples from 64 samples after
    the cue): both sides end in the same float32 eval kernel, so what is compared is the preprocessing.

    Tolerance: four times the largest move of a logit when the oracle's own preprocessed input is perturbed
    by one fp32 ulp per sample (random signs, fixed seed) -- the size of the rounding a float32 hand-over
    commits -- measured on the reference side alone, on the CPU: the float32 forward of oracle/torch_ref.py
    stands in for forward_eval.  The float32 oracle, not the float64 one of oracle/numpy_ref.py, because the
    quantity bounded is a difference of two float32 forwards: in float64 the same perturbation moves the logits
    by 2.0e-9, four times which (7.9e-9) is below half an ulp of these logits (2^-26 = 1.5e-8 at |logit| 0.3),
    a bound only bit-identical inputs could meet.  Measured: the float32 oracle's logits move by 2.98e-8 (one
    ulp of a logit) on one host and by 4.47e-8 on another (torch's CPU kernels differ between processors),
    so the tolerance is 1.19e-7 or 1.79e-7; the device path differs from the reference by 2.98e-8, and from
    the float64 forward by 4.2e-8 (printed, not asserted: that figure holds the eval kernel's own float32
    arithmetic; the float32 oracle is 4.2e-8 off it as well).  The preprocessed
    input itself differs from the oracle's by 0.40 ulp on average and by up to 400 ulp at samples near a zero
    crossing, where the filter's float32 rounding, divided by the standard deviation, is large against the
    sample."""
    from ems_cases import make_recording, oracle_ems
    from fir_cases import oracle_fir
    from hip_cases import oracle_eval
    from oracle import torch_ref as tr
    from eegnetreplication_amd import design_bandpass, epoch_logits, epoch_starts, ops, preprocess_recording
    dev = _dev()
    C, T = SHAPES["22x257"]
    m = _model(C, T, dev)
    R, N = 2, 1900
    h = design_bandpass()
    raw = make_recording(R * C, N, 77).reshape(R, C, N)
    onsets = [0, 130, 700, 1001, N - T - 64]
    starts = epoch_starts(onsets).tolist()
    idx = [0, 1, 1, 0, 1]
    # the oracle side, float64 throughout
    z = oracle_ems(oracle_fir(raw.reshape(R * C, N), h))[0].reshape(R, C, N)
    cut = lambda a: np.stack([a[r, :, s:s + T] for s, r in zip(starts, idx)])
    ref64 = oracle_eval(m, cut(z))
    ulp = np.spacing(np.abs(z).astype(np.float32)).astype(np.float64)
    sign = np.random.default_rng(5).choice([-1.0, 1.0], size=z.shape)
    moved64 = float(np.abs(oracle_eval(m, cut(z + sign * ulp)) - ref64).max())
    cpu32 = tr.TorchRefEEGNet({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, p=0.0)
    cpu32.training = False
    f32 = lambda a: cpu32(torch.from_numpy(a.astype(np.float32))).detach().double().numpy()
    moved = float(np.abs(f32(cut(z + sign * ulp)) - f32(cut(z))).max())
    tol = 4.0 * moved
    wins = torch.from_numpy(cut(z).astype(np.float32)).to(dev)
    ref = ops.forward_eval(m.shape, m.flat_parameters(), m.flat_bn_buffers(), wins).double().cpu().numpy()
    rec = preprocess_recording(torch.from_numpy(raw).to(dev), h)
    got = epoch_logits(m, rec, starts, idx).double().cpu().numpy()
    err = float(np.abs(got - ref).max())
    dz = np.abs(rec.double().cpu().numpy() - z) / ulp
    print(f"whole chain: one fp32 ulp per input sample moves the float32 oracle's logits by {moved:.3e} "
          f"(the float64 oracle's by {moved64:.3e}); "
          f"tolerance {tol:.3e}; max |gpu - reference| {err:.3e}; max |logit| {np.abs(ref).max():.3f}; "
          f"preprocessed input off by at most {dz.max():.2f} ulp (mean {dz.mean():.3f}); "
          f"max |gpu - float64 forward| {np.abs(got - ref64).max():.3e}")
    assert np.isfinite(got).all()
    assert err <= tol
