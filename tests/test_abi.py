"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/eegnet_abi.h declares; host-side geometry/validation calls work without a GPU."""

from __future__ import annotations

import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    txt = open(os.path.join(ROOT, "include", "eegnet_abi.h")).read()
    return sorted(set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(eegnet_\w+)\s*\(", txt, re.M)))


def test_header_matches_binding():
    from eegnetreplication_amd import _lib
    assert _header_symbols() == sorted(_lib.EXPORTED_SYMBOLS)


def test_library_exports_every_symbol():
    from eegnetreplication_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libeegnet_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    for name in _header_symbols():
        assert hasattr(lib, name), name
    assert b"gfx950" in lib.eegnet_build_info()
    txt = open(os.path.join(ROOT, "include", "eegnet_abi.h")).read()
    ver = int(re.search(r"#define EEGNET_ABI_VERSION (\d+)", txt).group(1))
    assert lib.eegnet_abi_version() == ver == _lib.ABI_VERSION


def test_param_count_and_validation():
    from eegnetreplication_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libeegnet_hip.so not built")
    d = _lib.dims(4096, 22, 256)
    assert _lib.param_count(d) == 1716          # paper Table 3 / SURVEY section 6
    assert _lib.workspace_bytes(d) > 4 * 4096 * 16 * 64 * 4
    d16 = _lib.dims(8, 64, 512, F1=16, D=4)
    assert _lib.param_count(d16) == 14116       # EEGNet-16,4 at 64x512
    with pytest.raises(RuntimeError, match="K1"):
        _lib.param_count(_lib.dims(8, 22, 256, K1=48))
    with pytest.raises(RuntimeError, match="F1\\*D"):
        _lib.param_count(_lib.dims(8, 22, 256, F1=3, D=1))


def test_shape_param_layout_matches_library():
    from eegnetreplication_amd import _lib
    from eegnetreplication_amd.ops import Shape
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libeegnet_hip.so not built")
    for C, T, F1, D in [(22, 256, 8, 2), (22, 257, 8, 2), (64, 512, 16, 4), (8, 64, 8, 2)]:
        s = Shape(C=C, T=T, F1=F1, D=D)
        assert s.n_params() == _lib.param_count(s.dims(4))


def _header_param_count(name):
    txt = open(os.path.join(ROOT, "include", "eegnet_abi.h")).read()
    m = re.search(r"^\s*(?:int|size_t|const char\*)\s+" + name + r"\s*\((.*?)\);", txt, re.S | re.M)
    args = m.group(1).strip()
    return 0 if args in ("", "void") else args.count(",") + 1


def test_binding_argument_counts_match_header():
    """Every ctypes signature has exactly as many arguments as the C prototype (a short argtypes
    list leaves trailing pointer arguments -- e.g. num_batches_tracked -- undefined)."""
    from eegnetreplication_amd import _lib
    for name, (_, args) in _lib._SIGS.items():
        assert len(args) == _header_param_count(name), name


def test_integration_ctypes_example_matches_binding():
    """The ctypes snippet a maintainer copies from INTEGRATION.md binds eegnet_train_step with the
    full parameter list (it once omitted num_batches_tracked) and passes every argument."""
    from eegnetreplication_amd import _lib
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"lib\.eegnet_train_step\.argtypes = \[(.*?)\]\n", txt, re.S)
    n_decl = m.group(1).count(",") + 1
    assert n_decl == len(_lib._SIGS["eegnet_train_step"][1]) == _header_param_count("eegnet_train_step")
    fields = re.findall(r'\("(\w+)", ctypes\.c_(?:int|float)\)', re.search(r"class Dims\(ctypes\.Structure\):(.*?)\]\n",
                                                                    txt, re.S).group(1))
    assert fields == [n for n, _ in _lib.Dims._fields_]          # the struct mirror, field for field
    call = re.search(r"rc = lib\.eegnet_train_step\((.*?)\)\s*(?:#.*)?\n(?=if rc)", txt, re.S).group(1)
    call = re.sub(r"#[^\n]*", "", call)
    depth, n_args = 0, 1
    for ch in call:
        depth += ch == "("
        depth -= ch == ")"
        n_args += ch == "," and depth == 0
    assert n_args == n_decl


def test_flag_and_kernel_id_constants_match_header():
    """The Python side's flag values and profiling kernel ids are the ones include/eegnet_abi.h
    documents (EEGNET_NO_CLAMP, EEGNET_KEY_FROM_STEP; eegnet_profile_enable's bit order)."""
    from eegnetreplication_amd import _lib, ops
    txt = open(os.path.join(ROOT, "include", "eegnet_abi.h")).read()
    flags = dict((k, int(v)) for k, v in re.findall(r"(EEGNET_[A-Z_]+)\s*=\s*(\d+)", txt))
    assert flags["EEGNET_NO_CLAMP"] == ops.NO_CLAMP
    assert flags["EEGNET_KEY_FROM_STEP"] == ops.KEY_FROM_STEP
    doc = re.search(r"i-th name eegnet_profile_collect reports:(.*?);", txt, re.S).group(1)
    assert [n.strip(" *\n") for n in doc.replace("\n", " ").split(",")] == list(_lib.KERNEL_IDS)


def test_cfg5_runs_the_compile_time_geometry_kernels():
    """The wide kernels compiled for EEGNet-16,4 at 64 x 512 are launched for exactly those dims, whatever
    the batch; their compile-time geometry (kGeoW5, eegnet_geometry.h) is the host's own shape function
    evaluated for them, so a layout change (coefficient block, workspace, LDS carve-up) reaches both at
    once.  Any other shape runs the generic kernels (cfg5 train 1.4M instead of 1.8M trials/s).  No GPU
    needed."""
    import ctypes
    from eegnetreplication_amd import _lib
    lib = _lib.load()
    d5 = _lib.dims(1024, 64, 512, F1=16, D=4, K1=32)
    assert lib.eegnet_wide_spec(ctypes.byref(d5)) == 1, lib.eegnet_last_error().decode()
    for B in (1, 7, 4096):           # the batch is a run-time field
        d = _lib.dims(B, 64, 512, F1=16, D=4, K1=32)
        assert lib.eegnet_wide_spec(ctypes.byref(d)) == 1
    assert lib.eegnet_wide_spec(ctypes.byref(_lib.dims(4096, 22, 256))) == 0      # narrow
    assert lib.eegnet_wide_spec(ctypes.byref(_lib.dims(64, 64, 256, F1=16, D=4, K1=32))) == 0


def test_x_pitch_entry_point_and_validation():
    """eegnet_x_pitch: 260 for the recordings' 22 x 257 EEGNet-8,2 (16-byte rows), T elsewhere; a
    pitch is accepted only where the kernels honour it (checked by the geometry, no GPU needed)."""
    import ctypes
    from eegnetreplication_amd import _lib
    lib = _lib.load()
    xp = lambda *a, **k: lib.eegnet_x_pitch(ctypes.byref(_lib.dims(*a, **k)))
    assert xp(64, 22, 257) == 260
    assert xp(64, 22, 256) == 256
    assert xp(64, 22, 257, K1=64) == 257
    assert xp(64, 32, 257) == 257
    assert xp(64, 64, 512, F1=16, D=4) == 512
    nb = ctypes.c_size_t()
    ok = lambda d: lib.eegnet_workspace_bytes(ctypes.byref(d), ctypes.byref(nb))
    assert ok(_lib.dims(64, 22, 257, x_pitch=260)) == 0
    assert ok(_lib.dims(64, 22, 257, x_pitch=257)) == 0
    assert ok(_lib.dims(64, 22, 257, x_pitch=258)) != 0          # not a multiple of 4
    assert ok(_lib.dims(64, 22, 257, x_pitch=256)) != 0          # below T
    assert ok(_lib.dims(64, 32, 257, x_pitch=260)) != 0          # a runtime-shape kernel
    assert ok(_lib.dims(64, 22, 256, x_pitch=256)) == 0
    assert ok(_lib.dims(64, 22, 256, x_pitch=260)) != 0          # 22 x 256: pitch compiled in as T


def test_fold_mirror_matches_header():
    """The eegnet_fold mirror (_lib.Fold) and INTEGRATION.md's snippet list the header's fields in
    order (a field added to the struct -- xstat -- shifts every later one)."""
    from eegnetreplication_amd import _lib
    txt = open(os.path.join(ROOT, "include", "eegnet_abi.h")).read()
    body = re.search(r"typedef struct eegnet_fold \{(.*?)\} eegnet_fold;", txt, re.S).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\**(\w+);", body, re.M)
    assert fields == [n for n, _ in _lib.Fold._fields_]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    snippet = re.search(r"class Fold\(ctypes\.Structure\):(.*?)\nassert", doc, re.S).group(1)
    assert re.findall(r'"(\w+)"', snippet) == fields


def test_x_stats_width_matches_pass_a_row_head():
    """eegnet_x_stats_width = K1 + 1 + the edge items (head pairs, tail pairs, head and tail sums):
    pass A's partial-row head a fold launch with xstat replaces."""
    import ctypes
    from eegnetreplication_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libeegnet_hip.so not built")
    lib = _lib.load()
    for K1 in (32, 64):
        P, R = (K1 - 1) // 2, K1 - 1 - (K1 - 1) // 2
        want = K1 + 1 + R * (R + 1) // 2 + P * (P + 1) // 2 + R + P
        assert lib.eegnet_x_stats_width(ctypes.byref(_lib.dims(64, 22, 257, K1=K1))) == want
    assert lib.eegnet_x_stats_width(ctypes.byref(_lib.dims(64, 64, 512, F1=16, D=4))) < 0    # narrow path only


def test_launch_grids_follow_the_documented_split():
    """eegnet_launch_grids against the rule DESIGN 6 / eegnet_abi.h document, for the CU count the
    library itself reports (the eval forward's grid at a batch far above it; 256 without a GPU):
    streaming passes A, B, D, E over min(B, 2 CUs) workgroups and pass C and the eval forward over
    min(B, CUs) for F1*D <= 16; for F1*D > 16 the streaming passes over min(B NOC, CUs) workgroups
    rounded down to a multiple of NOC (of 8 NOC when it reaches that), NOC = ceil(F1*D / 16) per trial
    range, and the block-2 passes and the eval forward over min(B, CUs); a fold launch gives a
    workgroup 4 trials in the streaming passes and 16 in pass C.  Pass C of the F1*D <= 16 step is
    counted in per-wave trial streams: workgroups x 8 waves at a runtime shape, x 16 at the compile-time
    ones.  The trials per workgroup of fold launches and the waves of pass C are the default build's
    values (a -DEEGNET_FOLD_TPW_* build has others)."""
    from eegnetreplication_amd import _lib, ops
    from eegnetreplication_amd.ops import Shape
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libeegnet_hip.so not built")
    cus = ops.launch_grids(Shape(8, 64), 1 << 20)["eval"]
    assert cus >= 1
    batches = (1, 7, 64, 2 * cus + 3, 4 * cus + 3, 16 * cus)
    for shape, nwc in ((Shape(8, 64), 8), (Shape(22, 257), 16)):
        for B in batches:
            s, c = min(B, 2 * cus), min(B, cus)
            assert ops.launch_grids(shape, B) == dict(A=s, B=s, C=c * nwc, D=s, E=s, eval=c), (shape, B)
            fs, fc = min(s, (B + 3) // 4), min(c, (B + 15) // 16)
            assert ops.launch_grids(shape, B, fold_launch=True) == dict(A=fs, B=fs, C=fc * nwc, D=fs, E=fs,
                                                                       eval=0), (shape, B)
    wide = Shape(10, 128, F1=12, D=4)
    noc = (wide.F2 + 15) // 16
    for B in batches:
        G = max(noc, min(B * noc, cus) // noc * noc)
        if G >= 8 * noc:
            G = G // (8 * noc) * (8 * noc)
        r, c = G // noc, min(B, cus)
        assert ops.launch_grids(wide, B) == dict(A=r, B=r, C=c, D=c, E=r, eval=c), B
    with pytest.raises(RuntimeError, match="F1\\*D"):
        ops.launch_grids(wide, 64, fold_launch=True)         # fold launches: the narrow path only
    with pytest.raises(RuntimeError, match="B must be"):
        ops.launch_grids(Shape(8, 64), 0)


def test_wide_training_with_64_taps_is_rejected():
    """F1*D > 16 with K1 = 64: eegnet_forward_train, eegnet_backward and eegnet_train_step refuse the
    dims before they look at a pointer or launch anything (its train step ended in a GPU memory fault
    whose cause is not known); eegnet_train_stage and eegnet_train_step_folds refuse every F1*D > 16.
    The geometry calls and K1 = 32 are unaffected.  Runs without a GPU."""
    import ctypes
    from eegnetreplication_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libeegnet_hip.so not built")
    lib = _lib.load()
    d = _lib.dims(8, 5, 72, F1=8, D=4, K1=64)
    assert _lib.workspace_bytes(d) > 0 and _lib.param_count(d) > 0
    n = None                                         # never dereferenced: the calls fail on the dims
    calls = {
        "eegnet_forward_train": lambda dd: lib.eegnet_forward_train(ctypes.byref(dd), n, n, n, n, n, 1, 2, n, n, n, n),
        "eegnet_backward": lambda dd: lib.eegnet_backward(ctypes.byref(dd), n, n, n, n, n, n, 1, 2, n, n, n, n, 0),
        "eegnet_train_step": lambda dd: lib.eegnet_train_step(ctypes.byref(dd), n, n, n, n, 1, 2, n, n, n, 1e-3, 0.9,
                                                              0.999, 1e-7, n, n, n, n, 0, n),
    }
    for name, call in calls.items():
        assert call(d) == -1, name
        msg = lib.eegnet_last_error().decode()
        assert name in msg and "K1 = 64 is not supported" in msg, msg
        assert call(_lib.dims(8, 5, 72, F1=8, D=4, K1=32)) == -1          # K1 = 32 gets as far as the NULL pointers
        assert "is NULL" in lib.eegnet_last_error().decode(), name
        assert call(_lib.dims(8, 3, 64, F1=8, D=2, K1=64)) == -1          # and so does F1*D <= 16 with 64 taps
        assert "is NULL" in lib.eegnet_last_error().decode(), name


def test_retired_persist_flag_is_rejected():
    """Round 5's opt-in one-launch persistent step (flag bit 4) is gone from the shipped library: the
    C-ABI rejects that bit (and every other unknown one) before any launch, so no caller -- FusedTrainer,
    DataParallelTrainer, FoldBatch or a C binding -- can reach a step whose results are not the
    five-launch step's bit for bit.  Runs without a GPU: the flag check precedes every device call."""
    import ctypes
    import inspect
    from eegnetreplication_amd import _lib, ops
    from eegnetreplication_amd.model import FusedTrainer
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libeegnet_hip.so not built")
    assert "persist" not in inspect.signature(FusedTrainer).parameters
    assert "persist" not in inspect.signature(ops.train_step).parameters
    assert not hasattr(ops, "PERSIST")
    lib = _lib.load()
    d = _lib.dims(64, 22, 256)
    dummy = ctypes.c_void_p(256)                     # never dereferenced: the call fails on the flags
    for flags in (4, 4 | 2, 8, 1 << 20):
        rc = lib.eegnet_train_step(ctypes.byref(d), dummy, dummy, dummy, dummy, 1, 2, dummy, dummy, dummy,
                                   1e-3, 0.9, 0.999, 1e-7, dummy, None, dummy, None, flags, None)
        assert rc == -1, flags
        assert b"unknown flags" in lib.eegnet_last_error()
    hdr = open(os.path.join(ROOT, "include", "eegnet_abi.h")).read()
    assert "EEGNET_PERSIST" not in hdr


# ---- the argument checks of the five train entry points and eegnet_stage_sums, one table ----
_NARROW = dict(B=8, C=3, T=64)
_WIDE = dict(B=8, C=5, T=72, F1=8, D=4, K1=32)
# entry point -> (its required pointers in the order the library checks them, every pointer a caller
# may pass, F1*D > 16 accepted).  The call builders below take {pointer name: address or None}.
_TRAIN_ENTRY_POINTS = {
    "eegnet_forward_train": (("params", "bn_buffers", "x", "logits", "ws"), ("mask2", "mask3", "nbt"), True),
    "eegnet_backward": (("params", "x", "grads", "ws"), ("dlogits", "labels", "mask2", "mask3", "loss"), True),
    "eegnet_train_step": (("params", "bn_buffers", "x", "labels", "grads", "ws"),
                          ("adam_state", "step", "loss", "logits", "nbt"), True),
    "eegnet_train_stage": (("params", "bn_buffers", "x", "labels", "grads", "ws"),
                           ("adam_state", "step", "loss", "nbt"), False),
    "eegnet_train_step_folds": (("folds",), (), False),
}


def _train_call(lib, name, d, p, flags=0, stage=0, norm_batch=None, nfolds=2, row0=0, slot=0):
    """One call of a train entry point with the pointers of `p` (a missing name is NULL)."""
    import ctypes
    g = lambda k: p.get(k)
    dd = ctypes.byref(d)
    if name == "eegnet_forward_train":
        return lib.eegnet_forward_train(dd, g("params"), g("bn_buffers"), g("x"), g("mask2"), g("mask3"), 1, 2,
                                        g("logits"), g("ws"), None, g("nbt"))
    if name == "eegnet_backward":
        return lib.eegnet_backward(dd, g("params"), g("x"), g("dlogits"), g("labels"), g("mask2"), g("mask3"), 1, 2,
                                   g("grads"), g("loss"), g("ws"), None, flags)
    if name == "eegnet_train_step":
        return lib.eegnet_train_step(dd, g("params"), g("bn_buffers"), g("x"), g("labels"), 1, 2, g("grads"),
                                     g("adam_state"), g("step"), 1e-3, 0.9, 0.999, 1e-7, g("loss"), g("logits"),
                                     g("ws"), None, flags, g("nbt"))
    if name == "eegnet_train_stage":
        return lib.eegnet_train_stage(dd, stage, d.B if norm_batch is None else norm_batch, g("params"),
                                      g("bn_buffers"), g("x"), g("labels"), 1, 2, g("grads"), g("adam_state"),
                                      g("step"), 1e-3, 0.9, 0.999, 1e-7, g("loss"), g("ws"), None, flags, g("nbt"))
    assert name == "eegnet_train_step_folds"
    return lib.eegnet_train_step_folds(dd, nfolds, g("folds"), row0, slot, 3, 1e-3, 0.9, 0.999, 1e-7, None)


def test_train_entry_points_name_the_argument_they_refuse():
    """The argument checks of eegnet_forward_train, eegnet_backward, eegnet_train_step, eegnet_train_stage
    and eegnet_train_step_folds at a narrow and a wide shape: with every pointer a dummy address and exactly
    one required pointer NULL the call returns -1 and eegnet_last_error names that pointer; with all of them
    NULL it names the first one the library checks.  The stage and fold entry points refuse F1*D > 16 before
    they look at a pointer.  Then the checks beside the pointers, and eegnet_stage_sums against the
    partial-row lengths of the five passes.  Every call leaves an argument invalid (the checks precede every
    device call) or is a geometry query: nothing is launched, no GPU is needed."""
    import ctypes
    from eegnetreplication_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libeegnet_hip.so not built")
    lib = _lib.load()
    err = lambda: lib.eegnet_last_error().decode()
    dummy = 4096                                     # never dereferenced: every call fails on an argument
    for kw in (_NARROW, _WIDE):
        d = _lib.dims(**kw)
        wide = d.F1 * d.D > 16
        for name, (required, optional, takes_wide) in _TRAIN_ENTRY_POINTS.items():
            every = {k: dummy for k in required + optional}
            patterns = [({k: v for k, v in every.items() if k != miss}, miss) for miss in required]
            patterns.append(({}, required[0]))
            for p, named in patterns:
                assert _train_call(lib, name, d, p) == -1, (name, kw, named)
                if wide and not takes_wide:
                    assert err() == f"{name}: F1*D = {d.F1 * d.D} > 16 is not supported", (name, named)
                else:
                    assert err() == f"{named} is NULL", (name, kw, named)

    d = _lib.dims(**_NARROW)
    full = lambda name: {k: dummy for k in sum(_TRAIN_ENTRY_POINTS[name][:2], ())}
    without = lambda name, *ks: {k: v for k, v in full(name).items() if k not in ks}
    for kw in (_NARROW, _WIDE):
        assert _train_call(lib, "eegnet_backward", _lib.dims(**kw), without("eegnet_backward", "dlogits", "labels")) == -1
        assert err() == "need dlogits or labels"
    for name in ("eegnet_train_step", "eegnet_train_stage"):
        assert _train_call(lib, name, d, without(name, "step")) == -1
        assert err() == "step is NULL", name
        assert _train_call(lib, name, d, without(name, "step", "adam_state"), flags=ops.KEY_FROM_STEP) == -1
        assert err() == "EEGNET_KEY_FROM_STEP needs the device step counter", name
    for stage in (-1, 10):
        assert _train_call(lib, "eegnet_train_stage", d, full("eegnet_train_stage"), stage=stage) == -1
        assert err() == f"stage must be in [0, 10) (got {stage})"
    assert _train_call(lib, "eegnet_train_stage", d, full("eegnet_train_stage"), norm_batch=d.B - 1) == -1
    assert err() == f"norm_batch must be in [B, 2^30] (got {d.B - 1})"
    folds = {"folds": dummy}
    for nfolds in (0, 65536):
        assert _train_call(lib, "eegnet_train_step_folds", d, folds, nfolds=nfolds) == -1
        assert err() == f"nfolds must be in [1, 65535] (got {nfolds})"
    assert _train_call(lib, "eegnet_train_step_folds", d, {}) == -1
    assert err() == "folds is NULL"
    for bad in (dict(row0=-1), dict(slot=-1)):
        assert _train_call(lib, "eegnet_train_step_folds", d, folds, **bad) == -1
        assert err() == "row0 / slot must be >= 0"

    # eegnet_stage_sums: pass k's count is the length of its partial row (eegnet_geometry.h, the part-row
    # comments of the pass kernels); the head of pass A's row is what eegnet_x_stats_width reports
    off, cnt = ctypes.c_size_t(0), ctypes.c_int(0)
    sums = lambda dd, k: lib.eegnet_stage_sums(ctypes.byref(dd), k, ctypes.byref(off), ctypes.byref(cnt))
    for kw in (_NARROW, _WIDE):
        d = _lib.dims(**kw)
        for k in (-1, 5):
            assert sums(d, k) == -1
            assert err() == f"pass must be in [0, 5) (got {k})"
        F2, NF = d.F1 * d.D, d.F1 * d.D * (d.T // 32)
        P = (d.K1 - 1) // 2
        R = d.K1 - 1 - P
        head = d.K1 + 1 + R * (R + 1) // 2 + P * (P + 1) // 2 + R + P
        if F2 <= 16:
            assert lib.eegnet_x_stats_width(ctypes.byref(d)) == head
        QR = d.F1 if (F2 <= 16 and d.D == 2) else F2
        want = (head + 2 * F2, 2 * F2, 4 * NF + 4 + 2 * F2 + 1, F2 * F2 + 18 * F2, QR * d.K1 + F2 * d.C + 2 * F2)
        offs = set()
        for k in range(5):
            assert sums(d, k) == 0, err()
            assert cnt.value == want[k], (kw, k)
            offs.add(off.value)
        assert len(offs) == 1 and 0 < off.value < _lib.workspace_bytes(d)      # one region for every pass
        assert lib.eegnet_stage_sums(ctypes.byref(d), 0, None, ctypes.byref(cnt)) == -1
        assert err() == "null output pointer"
