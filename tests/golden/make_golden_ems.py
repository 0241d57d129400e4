"""Generate the standardisation fixture tests/golden/ems/EMS1.npz from the REFERENCE implementation.

Runs on the development machine only, where the reference lies, like make_golden_dx.py:
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_ems.py

The reference's ``raw_exponential_moving_standardize`` (src/eegnet_repl/dataset.py:45-70) with its defaults
(factor_new 0.001, init_block_size 1000, eps the literal 1e-10) on 3 rows x 2600 float64 samples, rows 1
and 2 on DC offsets.  The input is regenerated from ``ems_cases.ems1_input`` by seed and is not stored; the
fixture holds the function's output ``y`` alone.

dataset.py imports mne, braindecode and torchvision at module level, which are not installed here, and uses
none of them in this function: empty stand-in modules carrying the imported names go into ``sys.modules``
before the import.
"""

from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference/src")


def _stand_in(name, **attrs):
    mod = sys.modules.get(name)
    if mod is None:
        try:
            __import__(name)
            return
        except ImportError:
            mod = sys.modules[name] = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)


_stand_in("mne")
_stand_in("torchvision")
_stand_in("torchvision.transforms", ToTensor=None)
_stand_in("braindecode")
_stand_in("braindecode.preprocessing", Preprocessor=None, exponential_moving_standardize=None, preprocess=None,
          create_windows_from_events=None)

from ems_cases import EMS1_N, EMS1_ROWS, EMS1_SEED, ems1_input  # noqa: E402
from eegnet_repl.dataset import raw_exponential_moving_standardize  # noqa: E402  (the reference)


def main():
    x = ems1_input()
    assert x.shape == (EMS1_ROWS, EMS1_N) and x.dtype == np.float64
    y = raw_exponential_moving_standardize(x)
    meta = dict(name="EMS1", rows=EMS1_ROWS, N=EMS1_N, seed=EMS1_SEED, factor_new=0.001, init_block_size=1000,
                eps=1e-10, numpy=np.__version__,
                reference="PraKesEy/EEGNetReplication src/eegnet_repl/dataset.py raw_exponential_moving_standardize")
    os.makedirs(os.path.join(HERE, "ems"), exist_ok=True)
    path = os.path.join(HERE, "ems", "EMS1.npz")
    np.savez_compressed(path, y=y, meta=np.array(json.dumps(meta)))
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
