"""How far the polyphase resampler (``resample``: scipy's ``resample_poly`` with reflected ends) lies from the FFT
method (``scipy.signal.resample``; what ``mne``'s ``raw.resample`` defaults to, here WITHOUT ``mne``'s own
padding, which is not reproduced) where it matters: after the 4-38 Hz band-pass.  CPU only, needs scipy.

    python tools/resample_method_diff.py [--out profiles/resample_method_diff.json]

The signal: trials of the seeded synthetic session generator (dataset.synthetic_session, the one
tools/accuracy_parity.py trains on) laid end to end as a 22-channel recording of 120,000 samples, read as 250 Hz,
once as generated and once on a DC offset of 100.  Both methods take it to 128 Hz in float64 (the float64 oracles
of the tests stand in for the kernels), both results pass the oracle band-pass (``design_bandpass()``), and the
difference is reported over the interior -- 1,000 output samples from each end left out -- as relative rms and
as maximum, together with the number of samples near the ends where the two differ by more than that maximum."""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from eegnetreplication_amd import design_bandpass, design_resampler  # noqa: E402
from eegnetreplication_amd.dataset import synthetic_session  # noqa: E402

UP, DOWN, EDGE = 64, 125, 1000


def compare(x):
    from fir_cases import oracle_fir
    from resample_cases import oracle_resample
    from scipy.signal import resample as fft_resample
    bp = design_bandpass()
    poly = oracle_fir(oracle_resample(x, design_resampler(UP, DOWN), UP, DOWN, "reflect_limited"), bp)
    fft = oracle_fir(fft_resample(x, poly.shape[1], axis=1), bp)
    d = np.abs(poly - fft)
    inner = slice(EDGE, poly.shape[1] - EDGE)
    rel_rms = float(np.sqrt((d[:, inner] ** 2).mean() / (fft[:, inner] ** 2).mean()))
    dmax = float(d[:, inner].max())
    ends = np.concatenate([d[:, :EDGE], d[:, -EDGE:]], axis=1)
    worse = (ends > dmax).any(axis=0)                              # per end sample, over the channels
    return {"n_out": int(poly.shape[1]), "interior_relative_rms": rel_rms, "interior_max_abs_diff": dmax,
            "interior_signal_rms": float(np.sqrt((fft[:, inner] ** 2).mean())),
            "end_samples_beyond_interior_max": {"head": int(worse[:EDGE].sum()), "tail": int(worse[EDGE:].sum())},
            "ends_max_abs_diff": float(ends.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_method_diff.json"))
    args = ap.parse_args()
    ds = synthetic_session(1, "Train", n=48, T=2500)
    x = np.ascontiguousarray(np.asarray(ds.X, dtype=np.float64).transpose(1, 0, 2).reshape(ds.X.shape[1], -1))
    out = {"tool": "resample_method_diff", "signal": "synthetic_session(1, 'Train', n=48, T=2500) laid end to end: "
           f"{x.shape[0]} x {x.shape[1]} samples read as 250 Hz", "ratio": f"{UP}/{DOWN}",
           "fft_method": "scipy.signal.resample (no padding: mne's npad='auto' is not reproduced)",
           "band_pass": "design_bandpass(): 213 taps, 4-38 Hz at 128 Hz", "edge_samples_left_out": EDGE,
           "as_generated": compare(x), "on_a_dc_offset_of_100": compare(x + 100.0)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
