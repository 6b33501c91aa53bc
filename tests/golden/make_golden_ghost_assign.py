#!/usr/bin/env python3
"""Generate tests/golden/ghost_assign.npz, the fixture of the host restatement in tests/test_ghost_frame.py.  Run from the repo root where the
reference is present:

    python tests/golden/make_golden_ghost_assign.py

The fixture holds arrays only.  Every recorded output comes from the reference's own Tracker.assign_act_inact_same_time and Tracker.assign_separatly
(adapters/GHOST/src/tracker.py:597-682), loaded as make_golden_ghost.load_reference loads them and called on a SimpleNamespace whose tracks record
their add_detection calls.  `solve_dense` is make_golden_ghost's stand-in (lapsolver is not installed), wrapped so that the matrix the separate mode
hands to its second solve, and the pairs it gets back, are recorded.

  params [K,4]              per case: sep (0 / 1), m detections, num_active, num_inactive
  dist_<k> [m,n]            the cost matrix in GHOST's [detections, tracks] orientation, active tracks first; NaN entries; in some cases a matched
                            cost is made EQUAL to its threshold (the filter is strict)
  row_<k>, col_<k>          the matching handed in (same-time: of the whole matrix; separate: of the active block)
  ids_<k> [n]               the track ids of the columns
  thr_<k> [2]               act_reid_thresh, inact_reid_thresh (a NaN threshold in one case)
  assigned_<k>              sorted(assigned)
  tr_ids_<k> [m]            tr_ids, None as -1.  In the separate mode the reference writes the second stage's ids at the COMPACTED detection index
                            (tracker.py:633 with the compacted list of :674): recorded as it is
  active_<k>                active_tracks, in the order the reference appended them
  added_<k> [q,2]           (track id, detection) of every add_detection, in call order
  second_<k> [1]            separate mode: whether the second solve_dense ran;  compact_<k> [u,ni] its matrix;  row2_<k>, col2_<k> its pairs
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden_ghost  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ghost_assign.npz")
CASES = 36


class _Track:
    def __init__(self, tid, log):
        self.tid, self.log, self.inactive_count = tid, log, 3

    def add_detection(self, idx, save_memory=None):
        self.log.append((self.tid, idx))


def main():
    _, _, Tracker = make_golden_ghost.load_reference()
    mod = sys.modules["src.tracker"]
    solve = mod.solve_dense
    out, params = {}, []
    for k in range(CASES):
        rs = np.random.RandomState(900 + k)
        sep = k % 2
        m, na, ni = int(rs.randint(1, 9)), int(rs.randint(0, 6)), int(rs.randint(0, 5))
        if k == 5:
            na = 0                                                 # the separate mode without active tracks: dist_inact = None
        if k == 7:
            ni = 0
        n = na + ni
        dist = np.round(rs.uniform(0.05, 0.95, (m, n)), 3)
        dist[rs.uniform(size=(m, n)) < 0.15] = np.nan
        ids = rs.permutation(50)[:n] + 1
        thr = np.array([0.6, 0.7])
        row, col = solve(dist[:, :na] if sep else dist)
        row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
        if k % 3 == 0 and len(row):                                # a matched cost equal to its threshold: not assigned
            r, c = row[0], col[0]
            dist[r, c] = thr[0 if c < na else 1]
        if k % 3 == 1 and len(row) > 1:                            # and one just below
            r, c = row[1], col[1]
            dist[r, c] = np.nextafter(thr[0 if c < na else 1], 0.0)
        if k == 9:
            thr[1] = np.nan
        log, seconds = [], []
        ns = types.SimpleNamespace(act_reid_thresh=thr[0], inact_reid_thresh=thr[1], save_memory=False,
                                   tracks={int(i): _Track(int(i), log) for i in ids[:na]},
                                   inactive_tracks={int(i): _Track(int(i), log) for i in ids[na:]})
        ns.assign_act_inact_same_time = types.MethodType(Tracker.assign_act_inact_same_time, ns)

        def recorder(d):
            r2, c2 = solve(d)
            seconds.append((np.array(d, dtype=np.float64), np.asarray(r2, dtype=np.int64), np.asarray(c2, dtype=np.int64)))
            return r2, c2
        mod.solve_dense = recorder
        try:
            dets = [{"idx": j} for j in range(m)]
            active, tr_ids = [], [None] * m
            if sep:
                d = [dist[:, :na].copy(), dist[:, na:].copy() if na > 0 else None]
                assigned = Tracker.assign_separatly(ns, row, col, d, dets, active, [int(i) for i in ids], tr_ids)
            else:
                assigned = ns.assign_act_inact_same_time(row, col, dist.copy(), dets, active, [int(i) for i in ids], tr_ids)
        finally:
            mod.solve_dense = solve
        params.append((sep, m, na, ni))
        out["dist_%d" % k], out["row_%d" % k], out["col_%d" % k], out["ids_%d" % k], out["thr_%d" % k] = dist, row, col, ids.astype(np.int64), thr
        out["assigned_%d" % k] = np.array(sorted(assigned), dtype=np.int64)
        out["tr_ids_%d" % k] = np.array([-1 if t is None else t for t in tr_ids], dtype=np.int64)
        out["active_%d" % k] = np.array(active, dtype=np.int64)
        out["added_%d" % k] = np.array(log, dtype=np.int64).reshape(-1, 2)
        if sep:
            assert len(seconds) <= 1
            out["second_%d" % k] = np.array([len(seconds)], dtype=np.int64)
            if seconds:
                out["compact_%d" % k], out["row2_%d" % k], out["col2_%d" % k] = seconds[0]
    out["params"] = np.array(params, dtype=np.int64)
    sep_cases = [k for k in range(CASES) if params[k][0]]
    assert sum(int(out["second_%d" % k][0]) for k in sep_cases) >= 8, "too few cases reach the second solve"
    assert any(np.isnan(out["compact_%d" % k]).any() for k in sep_cases if "compact_%d" % k in out)
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d cases, %d bytes" % (OUT, CASES, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
