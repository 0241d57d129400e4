"""Sliding-window inference over continuous recordings (eegnet_forward_eval_windows: k_infer_win +
k_win_reduce) on the GPU.

k_infer_win is k_infer with a loader that reads window w of a recording in place, and no arithmetic
crosses windows, so the bar for the logits is bit-equality with ``ops.forward_eval`` on the windows
unfolded into a contiguous batch.  ``probs`` is compared with a float64 numpy softmax-mean of the kernel's
own logits to 1e-6 absolute: the kernel accumulates in fp64, so what is left is the fp32 rounding of a
value <= 1 (6e-8) and the difference of two fp64 exponentials and sums (1e-15 per term); ``pred`` must be
that mean's argmax exactly, on recordings whose top-2 gap exceeds 1e-3."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"22x256": (22, 256), "22x257": (22, 257), "5x96-runtime": (5, 96), "6x101-runtime": (6, 101)}
SENT_F, SENT_I = -12345.5, -777
_models = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _model(C, T, dev, seed=3):
    """One random model per shape (BN state off its identity values), on the device, in eval mode."""
    from hip_cases import random_model
    key = (C, T, seed)
    if key not in _models:
        _models[key] = random_model(C, T, seed=seed).to(dev).eval()
    return _models[key]


def _rec_np(R, C, N, seed):
    return np.random.default_rng(seed).standard_normal((R, C, N), dtype=np.float32)


def _unfold(rec, T, hop):
    """[R, C, N] -> the windows as a contiguous batch [R * W, C, T], window w of recording r at r W + w."""
    R, C, _ = rec.shape
    u = rec.unfold(-1, T, hop).permute(0, 2, 1, 3)          # [R, W, C, T]
    return u.reshape(-1, C, T).contiguous(), u.shape[1]


def _ref_logits(m, rec, hop):
    from eegnetreplication_amd import ops
    x, W = _unfold(rec, m.T, hop)
    return ops.forward_eval(m.shape, m.flat_parameters(), m.flat_bn_buffers(), x).view(rec.shape[0], W, 4)


def _win(m, rec, hop, reduce=False):
    from eegnetreplication_amd import ops
    return ops.forward_eval_windows(m.shape, m.flat_parameters(), m.flat_bn_buffers(), rec, hop, reduce=reduce)


def _softmax_mean64(logits):
    """float64 numpy mean over the windows of softmax(logits [R, W, 4])."""
    l = np.asarray(logits, dtype=np.float64)
    e = np.exp(l - l.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).mean(1)


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_logits_bit_equal_to_forward_eval_on_the_unfolded_windows(shape, R):
    """Hops 1, 3, 4, 32, T and T + 5 at seven windows per recording, with up to two samples left over
    behind the last window (the count rounds down).  At an odd N the rows past the first start off
    16-byte alignment: the scalar loads, also at hop 4; hop 4 runs once more with nothing left over,
    N % 4 == 0, where every row of every recording is 16-byte aligned: the float4 loads."""
    dev = _dev()
    C, T = SHAPES[shape]
    m = _model(C, T, dev)
    for hop, left in [(h, min(h - 1, 2)) for h in (1, 3, 4, 32, T, T + 5)] + [(4, 0)]:
        N = T + 6 * hop + left
        rec = torch.from_numpy(_rec_np(R, C, N, 100 + hop)).to(dev)
        got = _win(m, rec, hop)
        ref = _ref_logits(m, rec, hop)
        assert got.shape == ref.shape == (R, (N - T) // hop + 1, 4), hop
        assert torch.isfinite(got).all(), hop
        assert torch.equal(got, ref), f"hop {hop}: max |diff| {(got - ref).abs().max().item():.3e}"
    # a 2-D recording is one recording without the leading axis
    if R == 1:
        assert torch.equal(_win(m, rec[0], hop), got[0])


@pytest.mark.parametrize("shape", ["22x256", "22x257", "5x96-runtime"])
def test_a_recording_of_exactly_one_window(shape):
    from eegnetreplication_amd import ops
    dev = _dev()
    C, T = SHAPES[shape]
    m = _model(C, T, dev)
    rec = torch.from_numpy(_rec_np(3, C, T, 7)).to(dev)
    for hop in (1, T):
        got = _win(m, rec, hop)
        assert got.shape == (3, 1, 4)
        assert torch.equal(got[:, 0], ops.forward_eval(m.shape, m.flat_parameters(), m.flat_bn_buffers(), rec))


@pytest.mark.parametrize("shape,N", [("22x256", 556), ("22x257", 557), ("5x96-runtime", 396)])
def test_more_windows_than_workgroups(shape, N):
    """301 windows at hop 1: above one window per CU, so the strided loop and the prefetch of the
    window after next run (and at 22 x 256 the rows of three windows in four are off 16-byte
    alignment: scalar loads)."""
    dev = _dev()
    C, T = SHAPES[shape]
    m = _model(C, T, dev)
    rec = torch.from_numpy(_rec_np(1, C, N, 8)).to(dev)
    got = _win(m, rec, 1)
    assert got.shape == (1, 301, 4)
    assert torch.equal(got, _ref_logits(m, rec, 1))
    rec4 = torch.from_numpy(_rec_np(3, C, T + 4 * 120, 9)).to(dev)      # 3 x 121 windows, the 16-byte path
    assert torch.equal(_win(m, rec4, 4), _ref_logits(m, rec4, 4))


@pytest.mark.parametrize("shape", ["22x256", "22x257", "5x96-runtime"])
@pytest.mark.parametrize("offset,hop", [(1, 4), (4, 4), (4, 3), (3, 32)],
                         ids=["off1-scalar", "off4-aligned", "off4-hop3", "off3-hop32"])
def test_in_place_views_of_a_larger_buffer(shape, offset, hop):
    """The recording is a time slice of a NaN-filled buffer (pitch > N): a load outside the slice
    would turn a logit into NaN.  The pitch is a multiple of 4 above N, so with T % 4 == 0 the offset
    and the hop decide the loader: a one-float offset forces scalar loads, offset 4 with hop 4 runs the
    float4 loads (every window row 16-byte aligned) at a pitch above N; hop 3 and offset 3 are scalar."""
    dev = _dev()
    C, T = SHAPES[shape]
    m = _model(C, T, dev)
    R, N = 2, T + 9 * hop + 1
    P = (N + 16 + 3) // 4 * 4
    assert P % 4 == 0 and P >= offset + N + 4
    data = torch.from_numpy(_rec_np(R, C, N, 31 + offset)).to(dev)
    buf = torch.full((R, C, P), float("nan"), dtype=torch.float32, device=dev)
    buf[:, :, offset:offset + N] = data
    view = buf[:, :, offset:offset + N]
    assert not view.is_contiguous() and view.stride() == (C * P, P, 1)
    assert view.data_ptr() % 16 == (4 * offset) % 16
    got = _win(m, view, hop)
    assert torch.isfinite(got).all()
    assert torch.equal(got, _win(m, data, hop))
    assert torch.equal(got, _ref_logits(m, data, hop))


def test_views_that_cannot_be_read_in_place_are_copied():
    """A time step of 2, a channel subset (recording stride != C * pitch) and a transposed layout."""
    dev = _dev()
    C, T = SHAPES["5x96-runtime"]
    m = _model(C, T, dev)
    big = torch.from_numpy(_rec_np(2, C + 2, 2 * (T + 40), 33)).to(dev)
    for view in (big[:, :C, ::2], big[:, 1:C + 1, 3:T + 43], big[:, :C, :T + 40].transpose(1, 2).contiguous().transpose(1, 2)):
        assert not view.is_contiguous()
        assert torch.equal(_win(m, view, 4), _ref_logits(m, view.contiguous(), 4))


@pytest.mark.parametrize("shape", ["22x256", "22x257"])
def test_outputs_stay_inside_their_buffers(shape):
    """The C entry point on sentinel-framed logits / probs / pred: the frames are untouched, and each of
    probs and pred can be asked for without the other."""
    from eegnetreplication_amd import _lib
    dev = _dev()
    C, T = SHAPES[shape]
    m = _model(C, T, dev)
    R, hop, N, M = 3, 5, T + 5 * 11 + 2, 64
    W = (N - T) // hop + 1
    rec = torch.from_numpy(_rec_np(R, C, N, 12)).to(dev)
    want_l, want_p, want_y = _win(m, rec, hop, reduce=True)
    vp = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    for use_p, use_y in ((True, True), (True, False), (False, True), (False, False)):
        lg = torch.full((R * W * 4 + 2 * M,), SENT_F, dtype=torch.float32, device=dev)
        pr = torch.full((R * 4 + 2 * M,), SENT_F, dtype=torch.float32, device=dev)
        yy = torch.full((R + 2 * M,), SENT_I, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().eegnet_forward_eval_windows(
            ctypes.byref(m.shape.dims(1)), vp(m.flat_parameters()), vp(m.flat_bn_buffers()), vp(rec), R, N, N, hop,
            vp(lg[M:]), vp(pr[M:] if use_p else None), vp(yy[M:] if use_y else None),
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "eegnet_forward_eval_windows")
        torch.cuda.synchronize()
        for buf, n, sent in ((lg, R * W * 4, SENT_F), (pr, R * 4, SENT_F), (yy, R, SENT_I)):
            assert (buf[:M] == sent).all() and (buf[M + n:] == sent).all()
        assert torch.equal(lg[M:M + R * W * 4].view(R, W, 4), want_l)
        assert torch.equal(pr[M:M + R * 4].view(R, 4), want_p) if use_p else (pr == SENT_F).all()
        assert torch.equal(yy[M:M + R], want_y) if use_y else (yy == SENT_I).all()


@pytest.mark.parametrize("shape,hop", [("22x256", 3), ("22x256", 4), ("22x257", 3), ("5x96-runtime", 4)])
def test_a_nan_sample_reaches_only_the_windows_that_hold_it(shape, hop):
    dev = _dev()
    C, T = SHAPES[shape]
    m = _model(C, T, dev)
    R, N = 2, T + 40 * hop
    W = (N - T) // hop + 1
    rec = torch.from_numpy(_rec_np(R, C, N, 13)).to(dev)
    clean = _win(m, rec, hop)
    for r, c, p in ((1, C - 1, T + 7), (0, 0, 0), (0, 2, N - 1)):
        dirty = rec.clone()
        dirty[r, c, p] = float("nan")
        got = _win(m, dirty, hop)
        starts = torch.arange(W, device=dev) * hop
        holds = (starts <= p) & (p < starts + T)                 # windows of recording r that hold sample p
        assert holds.any() and not holds.all()
        outside = torch.ones((R, W), dtype=torch.bool, device=dev)
        outside[r] = ~holds
        assert torch.equal(got[outside], clean[outside]), (r, c, p)
        assert torch.isfinite(got[outside]).all()


def test_two_calls_give_the_same_bits():
    dev = _dev()
    C, T = SHAPES["22x257"]
    m = _model(C, T, dev)
    rec = torch.from_numpy(_rec_np(3, C, T + 8 * 70, 14)).to(dev)
    a = _win(m, rec, 8, reduce=True)
    b = _win(m, rec, 8, reduce=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_graph_capture_and_replay():
    """One capture of a reduce=True call; the replay, on a recording changed in place since the capture,
    equals the eager call on the new data."""
    dev = _dev()
    C, T = SHAPES["22x256"]
    m = _model(C, T, dev)
    rec = torch.from_numpy(_rec_np(2, C, T + 4 * 30, 15)).to(dev)
    _win(m, rec, 4, reduce=True)                                 # eager once: the kernels' attributes are set
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _win(m, rec, 4, reduce=True)
    rec.copy_(torch.from_numpy(_rec_np(2, C, T + 4 * 30, 16)).to(dev))
    g.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in out]
    want = _win(m, rec, 4, reduce=True)
    for u, v in zip(got, want):
        assert torch.equal(u, v)


def test_public_api_against_the_float64_oracle():
    from eegnetreplication_amd import sliding_logits
    from golden_util import assert_close
    from hip_cases import oracle_eval
    dev = _dev()
    C, T = SHAPES["22x256"]
    m = _model(C, T, dev)
    rec_np = _rec_np(2, C, T + 32 * 4 + 9, 17)
    got = sliding_logits(m, torch.from_numpy(rec_np).to(dev), 32)
    wins = np.stack([rec_np[r, :, s:s + T] for r in range(2) for s in range(0, rec_np.shape[-1] - T + 1, 32)])
    ref = oracle_eval(m, wins).reshape(2, -1, 4)
    assert_close(got.cpu().numpy(), ref, name="sliding logits vs the float64 oracle")


# the recordings of the probs / pred test: (shape, R, N, hop, data seed), the seeds chosen so that every
# recording's top-2 gap exceeds 1e-3 (asserted below).  5 x 96: 300 windows per recording, above
# k_win_reduce's 256 threads.
REDUCE_CASES = [("5x96-runtime", 3, 395, 1, 21), ("22x257", 3, 257 + 8 * 20, 8, 22), ("22x256", 2, 256 + 128 * 3, 128, 23)]


@pytest.mark.parametrize("shape,R,N,hop,seed", REDUCE_CASES, ids=[c[0] for c in REDUCE_CASES])
def test_probs_and_pred(shape, R, N, hop, seed):
    dev = _dev()
    C, T = SHAPES[shape]
    m = _model(C, T, dev)
    rec = torch.from_numpy(_rec_np(R, C, N, seed)).to(dev)
    logits, probs, pred = _win(m, rec, hop, reduce=True)
    assert probs.shape == (R, 4) and probs.dtype == torch.float32
    assert pred.shape == (R,) and pred.dtype == torch.int32
    assert torch.equal(logits, _win(m, rec, hop))                # the same first kernel with or without the reduction
    ref = _softmax_mean64(logits.cpu().numpy())
    err = np.abs(probs.double().cpu().numpy() - ref).max()
    top = np.sort(ref, axis=1)
    gaps = top[:, -1] - top[:, -2]
    print(f"{shape}: max |probs - ref| {err:.3e}; top-2 gaps {gaps}")
    assert err <= 1e-6
    assert (gaps > 1e-3).all(), gaps                             # every recording: none is left out
    assert pred.cpu().numpy().tolist() == ref.argmax(1).tolist()


def test_a_tie_goes_to_the_lowest_class():
    """Classifier weight and bias zero: every logit is 0, every softmax exactly 0.25 and so is its mean."""
    from hip_cases import random_model
    dev = _dev()
    C, T = SHAPES["22x257"]
    m = random_model(C, T, seed=5).to(dev).eval()
    with torch.no_grad():
        m.classifier.weight.zero_()
        m.classifier.bias.zero_()
    rec = torch.from_numpy(_rec_np(3, C, T + 8 * 12, 18)).to(dev)
    logits, probs, pred = _win(m, rec, 8, reduce=True)
    assert (logits == 0).all()
    assert (probs == 0.25).all()
    assert (pred == 0).all()


def test_cropped_predict_and_evaluate_cropped():
    from eegnetreplication_amd import cropped_predict, evaluate_cropped, sliding_logits
    dev = _dev()
    C, T = SHAPES["22x257"]
    m = _model(C, T, dev)
    hop, N = 16, T + 16 * 9 + 3
    batches = [torch.from_numpy(_rec_np(b, C, N, 40 + b)).to(dev) for b in (5, 3)]
    m.train()                                                    # eval semantics whatever the mode, mode untouched
    try:
        preds = []
        for x in batches:
            probs, pred, logits = cropped_predict(m, x, hop)
            sl = sliding_logits(m, x, hop)
            assert m.training
            assert torch.equal(logits, sl) and torch.equal(sl, _ref_logits(m, x, hop))
            ref = torch.softmax(sl.double(), -1).mean(1)
            assert (probs.double() - ref).abs().max().item() <= 1e-6
            assert torch.equal(pred.long(), ref.argmax(1))
            preds.append(pred.long())
        p1, y1, l1 = cropped_predict(m, batches[0][0], hop)      # a 2-D recording
        assert p1.shape == (4,) and y1.dim() == 0 and l1.shape == (sl.shape[1], 4)
        assert torch.equal(l1, cropped_predict(m, batches[0], hop)[2][0])
        # labels: the prediction for every other trial, another class for the rest
        labels = [torch.where(torch.arange(len(p), device=dev) % 2 == 0, p, (p + 1) % 4) for p in preds]
        want = 100 * sum(int((p == y).sum()) for p, y in zip(preds, labels)) / sum(len(p) for p in preds)
        assert want == 100 * 5 / 8
        acc = evaluate_cropped(m, [(x.cpu(), y.cpu()) for x, y in zip(batches, labels)], hop)
        assert acc == want
        assert m.training
    finally:
        m.eval()


def test_wide_models_and_bad_recordings_are_refused():
    from eegnetreplication_amd import EEGNet, cropped_predict, sliding_logits
    dev = _dev()
    wide = EEGNet(64, 512, F1=16, D=4).to(dev).eval()
    rec = torch.zeros((64, 1024), device=dev)
    with pytest.raises(NotImplementedError, match="F1\\*D = 64 > 16 is not supported"):
        sliding_logits(wide, rec, 64)
    with pytest.raises(NotImplementedError, match="is not supported"):
        cropped_predict(wide, rec, 64)
    m = _model(22, 256, dev)
    with pytest.raises(RuntimeError, match="hop must be >= 1"):
        sliding_logits(m, torch.zeros((22, 512), device=dev), 0)
    with pytest.raises(RuntimeError, match="expected a recording"):
        sliding_logits(m, torch.zeros((22, 255), device=dev), 1)
    with pytest.raises(RuntimeError, match="expected a recording"):
        sliding_logits(m, torch.zeros((21, 512), device=dev), 1)
