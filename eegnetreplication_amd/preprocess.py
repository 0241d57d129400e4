"""Preprocessing of continuous recordings on the device: rational polyphase resampling, the zero-phase FIR
band-pass and the exponential moving standardisation the reference applies to every recording before it cuts
trials out of it (``raw.resample(128, npad="auto")``, dataset.py:114; ``raw.filter(4., 38.,
fir_design='firwin')``, dataset.py:113-125; ``raw_exponential_moving_standardize``, dataset.py:45-70).
``raw recording -> resample -> bandpass_filter -> exponential_moving_standardize -> epoch_logits /
sliding_logits`` runs without a host step; ``StreamResampler``, ``StreamBandpass`` and ``StreamStandardizer`` are
the same calls fed block by block with the state carried along.  The resampler is the polyphase FIR method
(``scipy.signal.resample_poly``, ``mne``'s ``method="polyphase"``), not the FFT method that the reference's call
defaults to: that one is a DFT of the whole padded recording and cannot stream.
"""

from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import torch

from . import ops
from .ops import require_device


def _as_rows(rec, what, step="exponential moving standardisation"):
    """``rec`` [C, N] or [R, C, N] on the device, float32 or float64 -> ([R, C, N] view, was 2-D)."""
    if rec.dim() not in (2, 3):
        raise RuntimeError(f"expected a recording [C, N] or [R, C, N], got {list(rec.shape)}")
    require_device(rec, what)
    if rec.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"{step} expects a float32 or float64 recording "
                           f"(got {rec.dtype})")
    return (rec.unsqueeze(0), True) if rec.dim() == 2 else (rec, False)


def _standardize(rec, out, **kw):
    if out is not None and out.shape != rec.shape:
        raise ValueError(f"out must have the recording's shape {list(rec.shape)} (got {list(out.shape)})")
    r3, squeeze = _as_rows(rec, "EEGNet recording")
    o3 = None
    if out is not None:
        require_device(out, "out")
        o3 = out.unsqueeze(0) if squeeze else out
    with torch.no_grad():
        y = ops.ems(r3.detach(), o3, **kw)
    if out is not None:
        return out
    return y[0] if squeeze else y


def exponential_moving_standardize(rec, factor_new=1e-3, init_block_size=1000, eps=1e-10, out=None):
    """Exponential moving standardisation of continuous recordings, per channel row:

        m_t = (1 - factor_new) m_{t-1} + factor_new x_t
        v_t = (1 - factor_new) v_{t-1} + factor_new (x_t - m_t)^2
        y_t = (x_t - m_t) / sqrt(v_t + eps)

    with (m, v) started at the mean and the population variance of the row's first
    min(init_block_size, N) samples.  ``rec`` is [C, N] or [R, C, N], float32 or float64, on the device, and
    is read in place when its last stride is 1 and its rows lie at one pitch (a contiguous tensor, or a
    time slice of a larger buffer, passed as it lies).  Returns float32 of the same shape; all arithmetic is
    float64 on the device and the result is rounded once.  ``out``: a float32 tensor of that shape to
    receive the result -- ``rec`` itself for an in-place call on a float32 recording.  The result goes
    straight into ``sliding_logits`` / ``cropped_predict``, a time slice of it included.  The same inputs
    give the same bits."""
    return _standardize(rec, out, factor_new=float(factor_new), init_block=int(init_block_size), eps=float(eps))


class StreamStandardizer:
    """``exponential_moving_standardize`` fed block by block: the standardiser of a pseudo-online decoder.

    ``n_rows_or_shape``: the number of channel rows C, or the leading shape of every block -- ``(C,)`` for
    blocks [C, n], ``(R, C)`` for blocks [R, C, n].  ``push(block)`` returns the standardised block
    (float32) and carries the running (mean, var) of every row to the next push; ``state`` is that float64
    [rows, 2] tensor on the device (None before the first push), ``reset()`` forgets it.

    The first push starts from the mean and variance of its own first min(init_block_size, n) samples.
    The concatenated output therefore equals ``exponential_moving_standardize`` of the whole recording
    only when the first block holds at least ``init_block_size`` samples; with a shorter first block the
    start values come from fewer samples and the outputs differ until the moving statistics forget them."""

    def __init__(self, n_rows_or_shape, factor_new=1e-3, init_block_size=1000, eps=1e-10):
        lead = (int(n_rows_or_shape),) if isinstance(n_rows_or_shape, int) else tuple(int(s) for s in n_rows_or_shape)
        if len(lead) not in (1, 2) or min(lead) < 1:
            raise ValueError(f"expected a row count or a leading shape (C,) or (R, C), got {n_rows_or_shape!r}")
        self.lead = lead
        self.factor_new, self.init_block_size, self.eps = float(factor_new), int(init_block_size), float(eps)
        self.state = None

    def reset(self):
        self.state = None

    def push(self, block):
        if tuple(block.shape[:-1]) != self.lead:
            raise RuntimeError(f"expected a block {list(self.lead)} + [n], got {list(block.shape)}")
        resume = self.state is not None
        if not resume:
            require_device(block, "EEGNet recording block")
            rows = 1
            for s in self.lead:
                rows *= s
            state = torch.empty((rows, 2), dtype=torch.float64, device=block.device)
        else:
            state = self.state
        y = _standardize(block, None, factor_new=self.factor_new, init_block=self.init_block_size, eps=self.eps,
                         state=state, resume=resume)
        if block.shape[-1] > 0:
            self.state = state
        return y


# ----------------------------------------------------------------------------------------------
# zero-phase FIR band-pass (dataset.py:113-125: raw.filter(4., 38., fir_design='firwin'))
# ----------------------------------------------------------------------------------------------
_HAMMING_LENGTH_FACTOR = 3.3          # taps = factor * sfreq / transition width, for a Hamming window


def _odd(n):
    return n + 1 - n % 2


def _lowpass(numtaps, cutoff, sfreq):
    """A Hamming-windowed-sinc low-pass of ``numtaps`` (odd) taps with its -6 dB point at ``cutoff`` Hz, scaled to
    unit gain at DC: ``scipy.signal.firwin(numtaps, cutoff, window='hamming', fs=sfreq)`` in plain numpy."""
    c = cutoff / (0.5 * sfreq)
    m = np.arange(numtaps) - 0.5 * (numtaps - 1)
    h = c * np.sinc(c * m)
    if numtaps > 1:
        h = h * (0.54 + 0.46 * np.cos(np.linspace(-np.pi, np.pi, numtaps)))
    h = 0.5 * (h + h[::-1])               # the window's two halves differ in the last bit: exactly linear phase
    return h / math.fsum(h)               # (the exactly rounded sum: the DC gain is 1 to the last bit or two)


def design_bandpass(sfreq=128.0, l_freq=4.0, h_freq=38.0):
    """Taps (float64 numpy, odd length, symmetric) of the zero-phase band-pass that ``mne`` designs for
    ``raw.filter(l_freq, h_freq, fir_design='firwin')`` with its defaults, by the rule ``mne`` documents:

      * transition bands  l_trans = min(max(0.25 l_freq, 2), l_freq),
                          h_trans = min(max(0.25 h_freq, 2), sfreq / 2 - h_freq);
      * length            ceil(3.3 sfreq / min(l_trans, h_trans)), made odd (3.3: the Hamming window);
      * taps              a Hamming-windowed-sinc low-pass with its -6 dB point at h_freq + h_trans / 2, of
                          round(3.3 sfreq / h_trans) taps made odd, centred in the full length, minus the
                          low-pass at l_freq - l_trans / 2 of round(3.3 sfreq / l_trans) taps made odd; each
                          low-pass has unit gain at DC, so the band-pass has none.

    At 128 Hz, 4-38 Hz: 213 taps (transitions 2 and 9.5 Hz); at 250 Hz: 413.  Pure numpy: scipy is not needed
    at run time.  ``mne`` itself is not installed where this package is developed, so the agreement with
    ``mne.filter.create_filter`` is by construction from its documented rule and is not checked by a test; taps
    that ``mne`` computed (``create_filter(...)``) can be passed to ``bandpass_filter`` unchanged."""
    sfreq, l_freq, h_freq = float(sfreq), float(l_freq), float(h_freq)
    if not 0.0 < l_freq < h_freq < 0.5 * sfreq:
        raise ValueError(f"expected 0 < l_freq < h_freq < sfreq / 2 (got {l_freq}, {h_freq}, sfreq {sfreq})")
    l_trans = min(max(0.25 * l_freq, 2.0), l_freq)
    h_trans = min(max(0.25 * h_freq, 2.0), 0.5 * sfreq - h_freq)
    n = _odd(int(math.ceil(_HAMMING_LENGTH_FACTOR * sfreq / min(l_trans, h_trans))))
    h = np.zeros(n)
    for sign, cutoff, trans in ((1.0, h_freq + 0.5 * h_trans, h_trans), (-1.0, l_freq - 0.5 * l_trans, l_trans)):
        k = _odd(int(round(_HAMMING_LENGTH_FACTOR * sfreq / trans)))
        off = (n - k) // 2
        h[off:n - off] += sign * _lowpass(k, cutoff, sfreq)
    return h


def _device_taps(taps, device):
    """float64 taps on ``device``: a float64 device tensor is used as it lies, anything else is uploaded."""
    if isinstance(taps, torch.Tensor) and taps.device.type == "cuda":
        if taps.dtype != torch.float64 or taps.dim() != 1:
            raise ValueError(f"device taps must be a float64 [L] tensor (got {taps.dtype} {list(taps.shape)})")
        return taps.contiguous()
    t = np.ascontiguousarray(taps.detach().numpy() if isinstance(taps, torch.Tensor) else taps, dtype=np.float64)
    if t.ndim != 1 or t.size < 1:
        raise ValueError(f"taps must be a non-empty 1-D array (got shape {list(t.shape)})")
    return torch.from_numpy(t).to(device)


def bandpass_filter(rec, taps, out=None):
    """Zero-phase FIR filtering of continuous recordings, per channel row:

        y[t] = sum_k taps[k] u[t + M - k],   M = (L - 1) / 2,

    u being the row extended past its ends as ``mne``'s 'reflect_limited' padding extends it
    (u[-j] = 2 x[0] - x[j], u[N-1+j] = 2 x[N-1] - x[N-1-j] for j up to min(M, N - 1), zero beyond): what
    ``raw.filter`` computes with symmetric taps.  ``rec`` is [C, N] or [R, C, N], float32 or float64, on the
    device, read in place when its last stride is 1 and its rows lie at one pitch.  ``taps``: an odd number of
    them (``design_bandpass()``, or ``mne``'s own) as a float64 device tensor, used as it lies -- what a graph
    capture must pass -- or a numpy array / CPU tensor, uploaded once per call.  Returns float32 of the same
    shape; all arithmetic is float64 on the device, the result is rounded once, and the same inputs give the
    same bits.  ``out``: a float32 tensor of that shape to receive the result; it must not overlap ``rec``
    (ValueError): there is no in-place filtering."""
    if out is not None and out.shape != rec.shape:
        raise ValueError(f"out must have the recording's shape {list(rec.shape)} (got {list(out.shape)})")
    r3, squeeze = _as_rows(rec, "EEGNet recording", "the band-pass filter")
    o3 = None
    if out is not None:
        require_device(out, "out")
        o3 = out.unsqueeze(0) if squeeze else out
    t = _device_taps(taps, rec.device)
    if t.shape[0] % 2 == 0:
        raise ValueError(f"a zero-phase filter needs an odd number of taps (got {int(t.shape[0])})")
    with torch.no_grad():
        y = ops.fir(r3.detach(), t, o3)
    if out is not None:
        return out
    return y[0] if squeeze else y


def preprocess_recording(rec, taps, factor_new=1e-3, init_block_size=1000, eps=1e-10, resample=None):
    """The reference's per-recording preprocessing: ``bandpass_filter(rec, taps)``, then
    ``exponential_moving_standardize`` of the result in place.  ``resample``: None for a recording at its final
    rate, or ``(up, down)`` to run ``resample(rec, up, down)`` first (the polyphase method with the default
    taps and ends -- not the FFT method of the reference's ``raw.resample``).  A composition of the calls,
    nothing fused; float32 [.., outputs], ready for ``epoch_logits`` / ``sliding_logits``."""
    if resample is not None:
        rec = _resample(rec, *resample)
    y = bandpass_filter(rec, taps)
    return exponential_moving_standardize(y, factor_new, init_block_size, eps, out=y)


class StreamBandpass:
    """``bandpass_filter`` fed block by block: the filter of a pseudo-online decoder, the companion of
    ``StreamStandardizer``.

    ``n_rows_or_shape``: the number of channel rows C, or the leading shape of every block -- ``(C,)`` for
    blocks [C, n], ``(R, C)`` for blocks [R, C, n].  ``taps``: as ``bandpass_filter`` takes them (L of them, L
    odd, M = (L - 1) / 2), uploaded at the first push.

    A zero-phase filter looks M samples ahead, so the output lags the input by M samples: the first
    ``push(block)`` must hold at least L samples (ValueError otherwise -- the head reflection is then the
    block's own) and returns n - M samples; every later push takes any n >= 1 and returns n samples;
    ``flush()`` returns the last M samples, reflected about the recording's end, and ends the stream
    (``reset()`` starts another).  Everything returned, concatenated, equals ``bandpass_filter`` of the
    whole recording bit for bit.  The last L - 1 input samples per row are carried as float64 in two device
    buffers that alternate (a call reads one and writes the other)."""

    def __init__(self, n_rows_or_shape, taps):
        lead = (int(n_rows_or_shape),) if isinstance(n_rows_or_shape, int) else tuple(int(s) for s in n_rows_or_shape)
        if len(lead) not in (1, 2) or min(lead) < 1:
            raise ValueError(f"expected a row count or a leading shape (C,) or (R, C), got {n_rows_or_shape!r}")
        n_taps = int(taps.shape[0]) if hasattr(taps, "shape") and len(taps.shape) == 1 else len(taps)
        if n_taps < 1 or n_taps % 2 == 0:
            raise ValueError(f"a zero-phase filter needs an odd number of taps (got {n_taps})")
        self.lead, self.taps, self.n_taps = lead, taps, n_taps
        self._hist = None                  # [current, spare] once the first block is in
        self._done = False

    def reset(self):
        self._hist, self._done = None, False

    def _lead3(self):
        return (1, self.lead[0]) if len(self.lead) == 1 else self.lead

    def push(self, block):
        if tuple(block.shape[:-1]) != self.lead:
            raise RuntimeError(f"expected a block {list(self.lead)} + [n], got {list(block.shape)}")
        if self._done:
            raise RuntimeError("the stream was flushed: reset() starts another")
        n, L = int(block.shape[-1]), self.n_taps
        first = self._hist is None
        if first and n < L:
            raise ValueError(f"the first block must hold at least the filter's {L} samples (got {n}): the head "
                             f"reflection has to be the block's own")
        if not first and n < 1:
            raise ValueError("a block must hold at least one sample")
        b3, squeeze = _as_rows(block, "EEGNet recording block", "the band-pass filter")
        R, C = self._lead3()
        if first:
            self.taps = _device_taps(self.taps, block.device)
            hist = [torch.empty((R * C, L - 1), dtype=torch.float64, device=block.device) for _ in range(2)]
            cur, new = None, hist[0]
        else:
            hist = self._hist
            cur, new = hist
        with torch.no_grad():
            y = ops.fir(b3.detach(), self.taps, mode=ops.FIR_FIRST if first else ops.FIR_NEXT, hist_in=cur, hist_out=new)
        self._hist = [hist[0], hist[1]] if first else [new, cur]
        return y[0] if squeeze else y

    def flush(self):
        if self._hist is None:
            raise RuntimeError("flush() before the first push")
        if self._done:
            raise RuntimeError("the stream was flushed: reset() starts another")
        self._done = True
        with torch.no_grad():
            y = ops.fir(None, self.taps, mode=ops.FIR_TAIL, hist_in=self._hist[0], lead=self._lead3())
        return y[0] if len(self.lead) == 1 else y


# ----------------------------------------------------------------------------------------------
# rational polyphase resampling (dataset.py:114: raw.resample(128) -- by another method, see resample)
# ----------------------------------------------------------------------------------------------
def _ratio(up, down):
    """(up, down) reduced by their gcd; integers >= 1 that do not reduce to 1/1."""
    if int(up) != up or int(down) != down or up < 1 or down < 1:
        raise ValueError(f"up and down must be integers >= 1 (got {up!r}/{down!r})")
    up, down = int(up), int(down)
    g = math.gcd(up, down)
    if up == down:
        raise ValueError(f"{up}/{down} reduces to 1/1: nothing to resample")
    return up // g, down // g


def design_resampler(up, down, half_len_factor=10, beta=5.0):
    """Prototype taps (float64 numpy, 2 * half_len_factor * max(up, down) + 1 of them, up/down reduced first) of
    the anti-alias low-pass that ``scipy.signal.resample_poly`` designs by default:
    ``firwin(2 * 10 * max(up, down) + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up``, restated in plain
    numpy -- a Kaiser-windowed sinc with its -6 dB point at the lower of the two Nyquist rates, scaled to unit
    gain at DC, times ``up``.  2501 taps and 40 terms per output for 64/125 (250 -> 128 Hz).  scipy is not needed
    at run time."""
    up, down = _ratio(up, down)
    m = max(up, down)
    half = int(half_len_factor) * m
    if half < 0:
        raise ValueError(f"half_len_factor must be >= 0 (got {half_len_factor})")
    c = 1.0 / m
    h = c * np.sinc(c * (np.arange(2 * half + 1) - float(half))) * np.kaiser(2 * half + 1, float(beta))
    return h / h.sum() * up


def resampled_length(n, up, down):
    """ceil(n up / down): the samples of a recording of ``n`` samples after ``resample`` (scipy's length)."""
    up, down = _ratio(up, down)
    return -(-int(n) * up // down)


def resampled_onsets(onsets, up, down):
    """Cue sample indices at the old rate -> int64 tensor of indices at the new rate.  The rounding rule chosen
    here: the nearest new sample to the cue's instant, ``floor(onset * up / down + 1/2)`` in exact integer
    arithmetic (a tie goes up).  Output m of ``resample`` stands at the instant of input sample m down / up, so
    the index returned is the output nearest in time to the cue.  (``mne`` is not installed where this package is
    developed: no agreement with its event resampling is claimed.)"""
    up, down = _ratio(up, down)
    t = torch.as_tensor(np.asarray(onsets))
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"expected integers (sample indices), got {t.dtype}")
    t = t.to(torch.int64)
    return torch.div(2 * t * up + down, 2 * down, rounding_mode="floor")


def resample_ratio(sfreq, new_sfreq=128.0):
    """(up, down), reduced, that takes ``sfreq`` to ``new_sfreq``: the exact ratio of the two rates through
    ``fractions.Fraction`` (250 -> 128 is 64/125).  ValueError for equal rates and for a ratio whose reduced
    ``up`` exceeds what the kernel takes (``ops.resample_max_up()``)."""
    f = Fraction(new_sfreq) / Fraction(sfreq)
    if f <= 0:
        raise ValueError(f"expected positive rates (got {sfreq} -> {new_sfreq})")
    up, down = _ratio(f.numerator, f.denominator)
    cap = ops.resample_max_up()
    if up > cap:
        raise ValueError(f"{sfreq} -> {new_sfreq} Hz is {up}/{down}: up exceeds the resampler's {cap}")
    return up, down


def resample(rec, up, down, taps=None, ends="reflect_limited", out=None):
    """Rational polyphase resampling ``up/down`` of continuous recordings, per channel row: with the prototype taps
    h (L = 2 half + 1 of them), c = m down + half and Q = half // up, output m of the ceil(N up / down) is

        y[m] = sum_{n = ceil((c - 2 half) / up) .. floor(c / up)} h[c - n up] u[n]

    -- ``scipy.signal.resample_poly(x, up, down, window=h)`` and ``mne``'s ``method="polyphase"``.  This is NOT the
    method of the reference's ``raw.resample(128, npad="auto")``, which is ``mne``'s FFT method; the two differ at
    the recording's ends and by the anti-alias filter's response.  u is the row extended past its ends:
    ``ends="reflect_limited"`` (the default: raw EEG sits on a DC offset) by the band-pass's odd reflection,
    u[-j] = 2 x[0] - x[j], u[N-1+j] = 2 x[N-1] - x[N-1-j] for j up to min(Q + 1, N - 1), zero beyond;
    ``ends="zero"`` by zeros, ``resample_poly``'s default.  ``rec`` is [C, N] or [R, C, N], float32 or float64, on
    the device, read in place when its last stride is 1 and its rows lie at one pitch.  ``taps``: None for
    ``design_resampler(up, down)``; a float64 device tensor, used as it lies -- what a graph capture must pass --
    or a numpy array / CPU tensor, uploaded once per call.  Returns float32 [.., ceil(N up / down)]; all arithmetic
    is float64 on the device, the result is rounded once, and the same inputs give the same bits.  ``out``: a
    float32 tensor of that shape to receive the result; it must not overlap ``rec``."""
    up, down = _ratio(up, down)
    if out is not None and rec.dim() in (2, 3):
        want = tuple(rec.shape[:-1]) + (resampled_length(rec.shape[-1], up, down),)
        if tuple(out.shape) != want:
            raise ValueError(f"out must have the shape {list(want)} (got {list(out.shape)})")
    r3, squeeze = _as_rows(rec, "EEGNet recording", "the resampler")
    o3 = None
    if out is not None:
        require_device(out, "out")
        o3 = out.unsqueeze(0) if squeeze else out
    t = _device_taps(design_resampler(up, down) if taps is None else taps, rec.device)
    if t.shape[0] % 2 == 0:
        raise ValueError(f"the resampler needs an odd number of taps (got {int(t.shape[0])})")
    with torch.no_grad():
        y = ops.resample(r3.detach(), t, up, down, o3, ends=ends)
    if out is not None:
        return out
    return y[0] if squeeze else y


_resample = resample                   # (preprocess_recording has a keyword of the name)


def resample_to(rec, sfreq, new_sfreq=128.0, taps=None, ends="reflect_limited", out=None):
    """``resample(rec, up, down, ...)`` with ``up/down = resample_ratio(sfreq, new_sfreq)``: what stands in for the
    reference's ``raw.resample(128)`` -- by the polyphase method, not by the FFT method that call defaults to."""
    up, down = resample_ratio(sfreq, new_sfreq)
    return resample(rec, up, down, taps, ends, out)


class StreamResampler:
    """``resample`` fed block by block: the resampler of a pseudo-online decoder fed by an amplifier at another
    rate, the companion of ``StreamBandpass`` (whose ``push`` takes what this one returns).  The polyphase method,
    as ``resample``: not the FFT method of the reference's ``raw.resample``.

    ``n_rows_or_shape``: the number of channel rows C, or the leading shape of every block -- ``(C,)`` for
    blocks [C, n], ``(R, C)`` for blocks [R, C, n].  ``taps``, ``ends``: as ``resample`` takes them; the taps
    are uploaded at the first push.

    ``push(block)`` returns the outputs whose whole support has arrived -- output m once m down + half < t up, t
    the samples pushed so far.  Their count varies from push to push (a short block may return none); it is
    ``output_count(n)`` before the push, computed on the host from integers alone.  The first block must hold at
    least Q + 2 = half // up + 2 samples (ValueError otherwise: the head's reflection has to be the block's
    own); every later one any n >= 1.  ``flush()`` returns the remaining outputs, the tail extended by ``ends``,
    and ends the stream (``reset()`` starts another).  Everything returned, concatenated, equals ``resample`` of
    the whole recording bit for bit.  The last 2 Q + 2 values of the extended row are carried as float64 in two
    device buffers that alternate (a call reads one and writes the other)."""

    def __init__(self, n_rows_or_shape, up, down, taps=None, ends="reflect_limited"):
        lead = (int(n_rows_or_shape),) if isinstance(n_rows_or_shape, int) else tuple(int(s) for s in n_rows_or_shape)
        if len(lead) not in (1, 2) or min(lead) < 1:
            raise ValueError(f"expected a row count or a leading shape (C,) or (R, C), got {n_rows_or_shape!r}")
        self.up, self.down = _ratio(up, down)
        if taps is None:
            taps = design_resampler(self.up, self.down)
        n_taps = int(taps.shape[0]) if hasattr(taps, "shape") and len(taps.shape) == 1 else len(taps)
        if n_taps < 1 or n_taps % 2 == 0:
            raise ValueError(f"the resampler needs an odd number of taps (got {n_taps})")
        if ends not in ops.RESAMPLE_ENDS:
            raise ValueError(f"ends must be one of {sorted(ops.RESAMPLE_ENDS)} (got {ends!r})")
        self.lead, self.taps, self.n_taps, self.ends = lead, taps, n_taps, ends
        self.first_block = n_taps // 2 // self.up + 2          # Q + 2
        self.reset()

    def reset(self):
        self._hist, self._done, self.n_seen = None, False, 0

    def _lead3(self):
        return (1, self.lead[0]) if len(self.lead) == 1 else self.lead

    def output_count(self, n=None):
        """The outputs the next ``push`` of ``n`` samples returns, or (``n`` None) the next ``flush()``."""
        if n is None:
            mode = ops.RESAMPLE_TAIL
        else:
            mode = ops.RESAMPLE_FIRST if self.n_seen == 0 else ops.RESAMPLE_NEXT
        return ops.resample_count(0 if n is None else int(n), self.n_taps, self.up, self.down, mode=mode,
                                  n_before=self.n_seen)

    def push(self, block):
        if tuple(block.shape[:-1]) != self.lead:
            raise RuntimeError(f"expected a block {list(self.lead)} + [n], got {list(block.shape)}")
        if self._done:
            raise RuntimeError("the stream was flushed: reset() starts another")
        n = int(block.shape[-1])
        first = self._hist is None
        if first and n < self.first_block:
            raise ValueError(f"the first block must hold at least {self.first_block} samples (got {n}): the head's "
                             f"extension has to be the block's own")
        if not first and n < 1:
            raise ValueError("a block must hold at least one sample")
        b3, squeeze = _as_rows(block, "EEGNet recording block", "the resampler")
        R, C = self._lead3()
        if first:
            self.taps = _device_taps(self.taps, block.device)
            hist = [torch.empty((R * C, 2 * self.first_block - 2), dtype=torch.float64, device=block.device)
                    for _ in range(2)]
            cur, new = None, hist[0]
        else:
            hist = self._hist
            cur, new = hist
        with torch.no_grad():
            y = ops.resample(b3.detach(), self.taps, self.up, self.down, ends=self.ends,
                             mode=ops.RESAMPLE_FIRST if first else ops.RESAMPLE_NEXT, n_before=self.n_seen,
                             hist_in=cur, hist_out=new)
        self._hist = [hist[0], hist[1]] if first else [new, cur]
        self.n_seen += n
        return y[0] if squeeze else y

    def flush(self):
        if self._hist is None:
            raise RuntimeError("flush() before the first push")
        if self._done:
            raise RuntimeError("the stream was flushed: reset() starts another")
        self._done = True
        with torch.no_grad():
            y = ops.resample(None, self.taps, self.up, self.down, ends=self.ends, mode=ops.RESAMPLE_TAIL,
                             n_before=self.n_seen, hist_in=self._hist[0], lead=self._lead3())
        return y[0] if len(self.lead) == 1 else y
