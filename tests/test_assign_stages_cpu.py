"""Staged assignment, the part that needs no GPU: busca_assign_stages is declared (include/busca_assign_stages.h), typed (busca_amd._lib) and
exported by the cross-compiled libbusca_hip.so; the LDS request of its kernel, by the host function that sizes the launch; the stage tables
SortStore.match builds against a literal restatement of Tracker._match (adapters/StrongSORT/deep_sort/tracker.py:226-248) with
matching_cascade's levels (deep_sort/linear_assignment.py:88-162); the argument errors of SortStore.match and of tracking.assign_stages, which are
raised before anything touches a device."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_declared_typed_and_exported():
    from busca_amd.build import build
    hip_lib = build()
    from busca_amd import _lib, tracking
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", _lib.ASSIGN_STAGES_HEADER)).read(), flags=re.S)
    declared = {}
    for name, args in re.findall(r"\b(busca_[a-z0-9_]+)\s*\((.*?)\)\s*;", hdr, flags=re.S):
        declared[name] = len(args.split(","))
    assert declared == {"busca_assign_stages": 16, "busca_assign_stages_lds_bytes": 3}
    assert declared == {name: len(args) for name, (_, args) in _lib.ASSIGN_STAGES_API.items()}
    assert re.search(r'#include\s+"busca_assign.h"', hdr)                        # the context, the error codes and BUSCA_ASSIGN_MAX come from there
    assert re.search(r"#define\s+BUSCA_ASSIGN_STAGES_MAX\s+%d\b" % _lib.ASSIGN_STAGES_MAX, hdr) and _lib.ASSIGN_STAGES_MAX == 128
    assert re.search(r"int32_t\s+plane;\s*int32_t\s+reserved;[^}]*double\s+limit;", hdr)      # the 16-byte stage record
    nm = subprocess.run(["nm", "-D", "--defined-only", hip_lib], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    assert set(declared) <= exported
    assert not [n for t in _lib.HEADERS.values() for n in t if n in declared]   # a name lives in exactly one table
    lib = _lib.load()
    assert len(lib.busca_assign_stages.argtypes) == 16 and lib.busca_assign_stages.restype is not None
    assert callable(tracking.assign_stages) and tracking.assign_stages.__module__ == "busca_amd.assignment"


def test_lds_request_fits_the_workgroup_limit():
    from busca_amd import _lib
    lib = _lib.load()
    top = _lib.ASSIGN_MAX
    unstaged = lib.busca_assign_stages_lds_bytes(top, top, 0)
    # the solver's state (3 f64 and 5 i32 per row / column pair, the exchange slots), four stage words per row, the histogram, two counters
    assert unstaged == 8 * (3 * top + 8) + 4 * (4 * top + 16) + 4 * (4 * top + _lib.ASSIGN_STAGES_MAX + 2)
    assert 0 < unstaged <= 160 * 1024 and lib.busca_assign_stages_lds_bytes(top, top, 1) == 160 * 1024       # staged: whatever the workgroup has left
    for n, m in ((1, 1), (7, 2048), (2048, 7), (50, 60), (139, 139), (140, 140), (150, 150), (2048, 2048)):
        s0, s1 = lib.busca_assign_stages_lds_bytes(n, m, 0), lib.busca_assign_stages_lds_bytes(n, m, 1)
        assert 0 < s0 <= s1 <= 160 * 1024 and s0 % 8 == 0 and s1 % 8 == 0
        assert s1 == min(s0 + 8 * n * m, 160 * 1024)                     # a whole plane where it fits, else the rest of the 160 KiB for the rows of a stage
    assert lib.busca_assign_stages_lds_bytes(139, 139, 1) < 160 * 1024 == lib.busca_assign_stages_lds_bytes(140, 140, 1)      # from here a stage of all rows reads global memory
    assert lib.busca_assign_stages_lds_bytes(top + 1, 4, 0) == -1 and lib.busca_assign_stages_lds_bytes(4, -1, 0) == -1


# ---- the stage tables ----------------------------------------------------------------------------------------------------
def r_match_stages(tsu, confirmed, cascade_depth):
    """tracker.py:226-248 and linear_assignment.py:136-150, literally: which tracks stand in which call of min_cost_matching, in call order.
    -> (levels: one list of track indices per call of the cascade, iou: the tracks that MAY stand in the IoU call - the unconfirmed ones for
    certain, a confirmed one with time_since_update == 1 if the cascade leaves it unmatched)."""
    tracks = [types.SimpleNamespace(time_since_update=t, is_confirmed=(lambda c=c: bool(c))) for t, c in zip(tsu, confirmed)]
    confirmed_tracks = [i for i, t in enumerate(tracks) if t.is_confirmed()]
    unconfirmed_tracks = [i for i, t in enumerate(tracks) if not t.is_confirmed()]
    if cascade_depth is None:                                                # opt.woC: one problem of all confirmed tracks
        levels = [list(confirmed_tracks)]
    else:
        levels = [[k for k in confirmed_tracks if tracks[k].time_since_update == 1 + level] for level in range(cascade_depth)]
    unmatched_tracks_a = confirmed_tracks                                    # the most the cascade can leave
    iou_track_candidates = unconfirmed_tracks + [k for k in unmatched_tracks_a if tracks[k].time_since_update == 1]
    return levels, unconfirmed_tracks, iou_track_candidates


STAGE_CASES = [
    ("ages 1, 2, 30, 31 at depth 30", [1, 2, 30, 31], [1, 1, 1, 1], 30),
    ("unconfirmed of age 1 and 2", [1, 2, 1, 3], [0, 0, 1, 1], 30),
    ("woC", [1, 2, 30, 31, 1, 2], [1, 1, 1, 1, 0, 0], None),
    ("no tracks", [], [], 30),
    ("a mixed frame", [1, 1, 1, 2, 2, 5, 1, 1, 1], [1, 1, 1, 1, 1, 1, 0, 0, 0], 6),
    ("depth 1", [1, 2, 1], [1, 1, 0], 1),
]


@pytest.mark.parametrize("name,tsu,confirmed,depth", STAGE_CASES, ids=[c[0] for c in STAGE_CASES])
def test_match_stage_tables_restate_the_tracker(name, tsu, confirmed, depth):
    from busca_amd.sort_store import _match_stage_tables
    first, again = _match_stage_tables(tsu, confirmed, depth)
    assert first.dtype == again.dtype == np.int32 and first.shape == again.shape == (len(tsu),)
    levels, unconfirmed, iou = r_match_stages(tsu, confirmed, depth)
    iou_stage = len(levels)
    assert iou_stage == (1 if depth is None else depth)
    for s, rows in enumerate(levels):                                        # every call of the cascade is a stage with exactly its tracks
        assert sorted(np.nonzero(first == s)[0].tolist()) == sorted(rows), (name, s)
    assert sorted(np.nonzero(first == iou_stage)[0].tolist()) == sorted(unconfirmed)
    assert sorted(np.nonzero((first == iou_stage) | (again == iou_stage))[0].tolist()) == sorted(iou)
    in_a_level = {k for rows in levels for k in rows}
    for k in range(len(tsu)):
        assert first[k] in in_a_level_stage(k, levels, in_a_level, unconfirmed, iou_stage), (name, k)
        assert again[k] in (-1, iou_stage) and (again[k] < 0 or again[k] > first[k])
    if name.startswith("ages"):
        assert first.tolist() == [0, 1, 29, -1] and again.tolist() == [30, -1, -1, -1]       # age 31 is deeper than the cascade: it stands nowhere
    if name.startswith("unconfirmed"):
        assert first.tolist() == [30, 30, 0, 2] and again.tolist() == [-1, -1, 30, -1]
    if name == "woC":
        assert first.tolist() == [0, 0, 0, 0, 1, 1] and again.tolist() == [1, -1, -1, -1, -1, -1]


def in_a_level_stage(k, levels, in_a_level, unconfirmed, iou_stage):
    if k in unconfirmed:
        return (iou_stage,)
    return tuple(s for s, rows in enumerate(levels) if k in rows) if k in in_a_level else (-1,)


def test_match_stage_tables_refuse_what_the_solver_cannot_hold():
    from busca_amd import _lib
    from busca_amd.sort_store import _match_stage_tables
    assert _match_stage_tables([1], [1], _lib.ASSIGN_STAGES_MAX - 1)[1].tolist() == [_lib.ASSIGN_STAGES_MAX - 1]
    with pytest.raises(ValueError, match="stages"):
        _match_stage_tables([1], [1], _lib.ASSIGN_STAGES_MAX)
    with pytest.raises(ValueError, match="confirmed"):
        _match_stage_tables([1, 2], [1], 30)


# ---- argument errors -------------------------------------------------------------------------------------------------------
def test_match_argument_errors_touch_no_device(monkeypatch):
    from busca_amd import _xfer, geometry
    from busca_amd.sort_store import SortStore

    def no_device(*a, **k):
        raise AssertionError("an argument error must be raised before anything touches the device")
    monkeypatch.setattr(geometry, "default_context", no_device)
    monkeypatch.setattr(_xfer, "h2d_async", no_device)
    st = SortStore.__new__(SortStore)                                        # the store's constructor names a device; these checks need none
    st.capacity = 16
    metric = types.SimpleNamespace(matching_threshold=0.3, ctx=None, distance=no_device)
    z, f = np.zeros((3, 4)), np.zeros((3, 8))
    ok = dict(metric=metric, slots=[0, 1], track_ids=[7, 8], time_since_update=[1, 1], confirmed=[True, False], det_features=f, det_xyah=z, det_tlwh=z,
              max_iou_distance=0.7, cascade_depth=30)
    for key, value, what in (("track_ids", [7], "track ids"), ("time_since_update", [1], "time_since_update"), ("confirmed", [True] * 3, "confirmed"),
                             ("det_features", f[:2], "feature rows"), ("det_tlwh", z[:1], "tlwh boxes"), ("slots", [3, 3], "distinct"),
                             ("slots", [0, 16], "capacity"), ("cascade_depth", 128, "stages")):
        with pytest.raises(ValueError, match=what):
            st.match(**dict(ok, **{key: value}))


def test_assign_stages_argument_errors():
    from busca_amd import _lib
    from busca_amd.assignment import _stage_tables_dev
    with pytest.raises(ValueError, match="stages"):
        _stage_tables_dev([], [0], None, None)
    with pytest.raises(ValueError, match="stages"):
        _stage_tables_dev([(0, 0.5)] * (_lib.ASSIGN_STAGES_MAX + 1), [0], None, None)
