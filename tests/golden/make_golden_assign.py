#!/usr/bin/env python3
"""Generate tests/golden/assign.npz, the fixture of tests/test_linear_assignment.py.  Run from the repo root where the reference is present:

    python tests/golden/make_golden_assign.py

The fixture holds arrays only.  The big cost matrices are not stored: a case is (kind, seed, n, m, inf share, limit) and the test rebuilds
its matrix with busca_amd.synth.tracker_costs / uniform_costs, which are bit-reproducible everywhere.

  names, params [K,6]     the generic cases: kind (0 tracker-like IoU costs, 1 uniform), seed, n, m, share of +inf entries, limit
  x_<name> [n] int16      the matched column of every row, or -1
  objective [K]           the reduced objective, the sum of (c_ij - limit) over the matches
  mcm_params [Q,4]        min_cost_matching cases: seed, number of tracks, number of detections, max_distance (uniform costs in [0, 1.5))
  mcm_ti_<q>, mcm_di_<q>  track_indices / detection_indices of case q
  mcm_matches_<q> [k,2], mcm_ut_<q>, mcm_ud_<q>    what the reference's min_cost_matching returns
  tie_names, tie_cost_<name>, tie_limit, tie_objective   matrices with many optimal matchings and their optimal reduced objective only

The lapjv route (matching.linear_assignment, adapters/ByteTrack/yolox/tracker/matching.py:39-50) is UNPINNED against `lap` itself: lap is
not installed where this runs, so the route is recorded through the padded-matrix restatement of lap.lapjv(extend_cost=True, cost_limit=t) -
the (n + m) x (n + m) matrix with the costs top left, t / 2 top right and bottom left, 0 bottom right - solved by
scipy.optimize.linear_sum_assignment.  The min_cost_matching cases are the output of the reference's own function
(adapters/StrongSORT/deep_sort/linear_assignment.py:15-85), imported with stand-in modules for `opts` and `deep_sort.kalman_filter`.

A generic case is kept only if its optimum is unique: it is re-solved with each matched pair forbidden in turn, and every such objective
must exceed the optimum by more than 1e-9.  Candidates that fail are dropped (the next seed is tried) and counted."""
import importlib.util
import os
import sys
import types

import numpy as np
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

from busca_amd import synth  # noqa: E402

TRACKER, UNIFORM = 0, 1
# name, kind, first seed, n, m, inf share, limit
GENERIC = [
    ("iou_t50", TRACKER, 11, 37, 41, 0.0, 0.5), ("iou_t80", TRACKER, 12, 52, 33, 0.0, 0.8), ("iou_t90", TRACKER, 13, 29, 29, 0.0, 0.9),
    ("iou_inf_t50", TRACKER, 14, 41, 37, 0.2, 0.5), ("iou_inf_t80", TRACKER, 15, 33, 52, 0.2, 0.8), ("iou_inf_t90", TRACKER, 16, 45, 45, 0.2, 0.9),
    ("cols63", TRACKER, 21, 70, 63, 0.2, 0.8), ("cols64", TRACKER, 22, 70, 64, 0.2, 0.8), ("cols65", TRACKER, 23, 70, 65, 0.2, 0.8),
    ("cols255", UNIFORM, 24, 40, 255, 0.0, 0.8), ("cols256", UNIFORM, 25, 40, 256, 0.0, 0.8), ("cols257", UNIFORM, 26, 40, 257, 0.0, 0.8),
    ("switch140", UNIFORM, 31, 140, 140, 0.0, 0.9), ("switch141", UNIFORM, 32, 141, 141, 0.0, 0.9),
    ("dense64", UNIFORM, 41, 64, 64, 0.0, 1.0), ("dense128x96", UNIFORM, 42, 128, 96, 0.0, 1.0), ("dense256", UNIFORM, 43, 256, 256, 0.0, 1.0),
    ("sparse1000", TRACKER, 51, 1000, 1000, 0.0, 0.8),
    ("batch0", TRACKER, 60, 12, 17, 0.0, 0.8), ("batch1", TRACKER, 61, 30, 9, 0.2, 0.8), ("batch2", UNIFORM, 62, 1, 24, 0.0, 0.8),
    ("batch3", UNIFORM, 63, 24, 1, 0.0, 0.8), ("batch4", TRACKER, 64, 40, 40, 0.0, 0.8), ("batch5", UNIFORM, 65, 17, 33, 0.0, 0.8),
    ("batch6", TRACKER, 66, 5, 5, 0.0, 0.8), ("batch7", UNIFORM, 67, 33, 40, 0.0, 0.8),
]
MCM = [(71, 24, 30, 0.2), (72, 40, 18, 0.4), (73, 33, 33, 0.3)]


def build(kind, seed, n, m, inf_frac):
    return synth.tracker_costs(seed, n, m, inf_frac) if kind == TRACKER else synth.uniform_costs(seed, n, m)


def solve_padded(c, t):
    """lap.lapjv(c, extend_cost=True, cost_limit=t) restated: row -> column or -1."""
    n, m = c.shape
    big = np.full((n + m, n + m), t / 2.0)
    big[n:, m:] = 0.0
    big[:n, :m] = c
    rows, cols = linear_sum_assignment(big)
    x = np.full(n, -1, dtype=np.int64)
    for r, j in zip(rows, cols):
        if r < n and j < m:
            x[r] = j
    return x


def solve_clamped(c, t):
    """The rectangular problem with every inadmissible entry at t, clamped pairs dropped: row -> column or -1."""
    n, m = c.shape
    rows, cols = linear_sum_assignment(np.where(c < t, c, t))
    x = np.full(n, -1, dtype=np.int64)
    for r, j in zip(rows, cols):
        if c[r, j] < t:
            x[r] = j
    return x


def reduced(c, t, x):
    rows = np.nonzero(x >= 0)[0]
    return float((c[rows, x[rows]] - t).sum())


def unique(c, t, x, margin=1e-9):
    best = reduced(c, t, x)
    for r in np.nonzero(x >= 0)[0]:
        d = c.copy()
        d[r, x[r]] = np.inf
        if not reduced(d, t, solve_clamped(d, t)) > best + margin:
            return False
    return True


def load_min_cost_matching():
    opts = types.ModuleType("opts")
    opts.opt = types.SimpleNamespace()
    pkg = types.ModuleType("deep_sort")
    pkg.__path__ = []
    kf = types.ModuleType("deep_sort.kalman_filter")
    kf.chi2inv95 = {}
    pkg.kalman_filter = kf
    sys.modules.update({"opts": opts, "deep_sort": pkg, "deep_sort.kalman_filter": kf})
    spec = importlib.util.spec_from_file_location("deep_sort.linear_assignment", os.path.join(REF, "adapters/StrongSORT/deep_sort/linear_assignment.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.min_cost_matching


def main():
    out, dropped = {}, 0
    names, params, objective = [], [], []
    for name, kind, seed, n, m, inf_frac, t in GENERIC:
        while True:
            c = build(kind, seed, n, m, inf_frac)
            x = solve_padded(c, t)
            if unique(c, t, x):
                assert np.array_equal(x, solve_clamped(c, t)), name                         # the two restatements agree on a unique optimum
                break
            dropped += 1
            seed += 100
        assert (x >= 0).sum() >= 1, name
        names.append(name)
        params.append([kind, seed, n, m, inf_frac, t])
        objective.append(reduced(c, t, x))
        out["x_" + name] = x.astype(np.int16)
        print("%-12s seed %3d  %4d x %4d  limit %.1f: %d matched, %d admissible entries" % (name, seed, n, m, t, (x >= 0).sum(), (c < t).sum()))
    print("generic candidates dropped for a non-unique optimum: %d" % dropped)
    out.update(names=np.array(names), params=np.array(params, dtype=np.float64), objective=np.array(objective))

    mcm = load_min_cost_matching()
    rows = []
    for q, (seed, nt, nd, max_distance) in enumerate(MCM):
        while True:
            full = synth.uniform_costs(seed, nt, nd, 0.0, 1.5)
            ti = np.nonzero(synth.uniform(seed, "ti", (nt,), 0.0, 1.0) < 0.8)[0]
            di = np.nonzero(synth.uniform(seed, "di", (nd,), 0.0, 1.0) < 0.8)[0]
            sub = full[np.ix_(ti, di)]
            t = max_distance + 1e-5
            if np.abs(sub - max_distance).min() > 1e-4 and unique(sub, t, solve_clamped(sub, t)):
                break
            dropped += 1
            seed += 100
        matches, ut, ud = mcm(lambda tr, de, a, b: full[np.ix_(a, b)].copy(), max_distance, list(range(nt)), list(range(nd)), list(ti), list(di))
        assert len(matches) >= 3 and len(ut) + len(ud) >= 1
        rows.append([seed, nt, nd, max_distance])
        out.update({"mcm_ti_%d" % q: ti.astype(np.int64), "mcm_di_%d" % q: di.astype(np.int64),
                    "mcm_matches_%d" % q: np.array(matches, dtype=np.int64).reshape(-1, 2),
                    "mcm_ut_%d" % q: np.array(ut, dtype=np.int64), "mcm_ud_%d" % q: np.array(ud, dtype=np.int64)})
        print("min_cost_matching %d: %d x %d of %d x %d, max_distance %.1f: %d matches" % (q, len(ti), len(di), nt, nd, max_distance, len(matches)))
    out["mcm_params"] = np.array(rows, dtype=np.float64)

    # ---- ties: many optimal matchings, only the objective is pinned ----------------------------------------------------------
    base = synth.tracker_costs(81, 9, 12)
    ties = [("dup_rows", np.concatenate([base, base[:6], base[2:5]], 0), 0.8),
            ("dup_rows_inf", np.concatenate([synth.tracker_costs(82, 10, 8, 0.2)] * 2, 0), 0.9),
            ("const_5x7", np.full((5, 7), 0.3), 0.8), ("const_7x5", np.full((7, 5), 0.3), 0.8), ("const_at_limit", np.full((4, 4), 0.8), 0.8),
            ("int_12x12", np.floor(synth.uniform_costs(83, 12, 12, 0.0, 6.0)), 3.0), ("int_20x15", np.floor(synth.uniform_costs(84, 20, 15, 0.0, 4.0)), 2.0)]
    tl, to = [], []
    for name, c, t in ties:
        c = np.ascontiguousarray(c, dtype=np.float64)
        a, b = reduced(c, t, solve_padded(c, t)), reduced(c, t, solve_clamped(c, t))
        assert abs(a - b) <= 1e-12 * max(1.0, abs(a)), (name, a, b)
        out["tie_cost_" + name] = c
        tl.append(t)
        to.append(a)
        print("tie %-14s %2d x %2d  limit %.1f: objective %.6f" % (name, c.shape[0], c.shape[1], t, a))
    out.update(tie_names=np.array([n for n, _, _ in ties]), tie_limit=np.array(tl), tie_objective=np.array(to))

    path = os.path.join(OUT, "assign.npz")
    np.savez_compressed(path, **out)
    print("wrote assign.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
