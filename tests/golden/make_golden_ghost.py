#!/usr/bin/env python3
"""Generate tests/golden/ghost.npz, the fixture of tests/test_ghost_round.py.  Run from the repo root where the reference is present:

    python tests/golden/make_golden_ghost.py

The fixture holds arrays only: parameters, index vectors and recorded outputs.  Features are not stored: a case names (seed, n, m, E, budget) and the
test rebuilds its vectors with busca_amd.synth.appearance_features(seed, n, m, E, budget, twins=True), which is bit-reproducible everywhere.

Every recorded output comes from the reference's own functions (adapters/GHOST/src/tracker.py, base_tracker.py, tracking_utils.py), imported from
their files with stand-in modules for what is not installed or not needed (lapsolver, cython_bbox, cv2, src.kalman, busca.network, busca.tracking,
numpy.lib.arraysetops; matplotlib, tqdm and sklearn only where they do not import) and called unbound on a SimpleNamespace.

  dist_params [K,5]            seed, n tracks, m detections, E, budget of the distance cases;  dist_count_<k> [n], dist_tlabel_<k> [n], dist_dlabel_<k> [m]
  pd_<k>_<num> [n,m]           Tracker.proxy_dist of every track stacked (tracks x detections), avg_inact.num = 1 .. 5, class-masked
  lf_<k> [n,m]                 Tracker.last_frame (the newest sample of every track), class-masked
  pd_err [K,5], lf_err [K]     ref_err: the largest difference between a float64 numpy restatement and the reference's float32 output
  px_params [5], px_count [n], px_newest [n]     the proxy case: a gallery whose full rings have wrapped (newest anywhere)
  px_<mode>_<avg> [n,E] f32    tracking_utils.get_proxy: last, mean / median with avg = 3 and 40 (below and above the gallery length), meannorm
                               with avg = 40 (its avg <= len branch raises in the reference);  px_err_<mode>_<avg>.  There is no 'first': that branch
                               (`avg == 'first'`, :80) cannot be reached in the reference, int('first') raises at :70 before it
  thr_every, thr_tbd [2]       BaseTracker.update_thresholds on pd_0_2 without the class mask, first `thr_na` tracks active;  thr_err_every / _tbd
  rd_params [Q,8]              the rounds: seed, n, m, E, budget, num_active, route (0 each_sample, 1 with_proxy), candidates tried
  rd_count_<q>, rd_newest_<q>, rd_tlabel_<q>, rd_dlabel_<q>     the tracks and labels of round q
  rd_masked_<q> [m,n]          the stacked (each_sample: class-masked) matrix solve_hungarian receives, GHOST's [detections, tracks]
  rd_blend_<q> [m,n]           combine_motion_appearance('sum_0.4') of it (rounds with a motion model; the motion cost is synth.tracker_costs(seed, n, m))
  rd_dist_<q> [m,n]            the nan_first result: what solve_dense gets
  rd_thr_<q> [2]               the thresholds in force (fixed, or what update_thresholds computed)
  rd_row_<q>_<sep>, rd_col_<q>_<sep>     the matching, sep = 0 / 1
  rd_err [Q], rd_thr_err [Q]   ref_err of rd_dist and rd_thr;  rd_masked_err_<q>, rd_blend_err_<q>: of the two earlier stages
  dropped [2]                  candidates dropped: [a cost within 1e-6 of a threshold, optimum not unique]; candidates [1] the number tried

STAND-IN: lapsolver is not installed, so `solve_dense` is replaced by scipy.optimize.linear_sum_assignment on the big-M matrix - every NaN entry at
M = 8192, matched pairs at M dropped (make_golden_assign.solve_clamped): the maximum-cardinality minimum-cost matching over the finite entries.
lapsolver's own behaviour on infeasible rows is third-party and unpinned.

A round candidate is dropped (next seed) if any cost lies within 1e-6 of its threshold - ten times the float32 noise observed between the
reference and a float64 restatement - or if the optimum of either sep mode is not unique by 1e-9 (make_golden_assign.unique) or differs on the
float64 restatement.  At most one candidate in ten may be dropped (asserted)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from busca_amd import synth  # noqa: E402
from make_golden_assign import solve_clamped, unique  # noqa: E402

LIMIT = 8192.0
ALPHA = 0.4
DIST_CASES = [(400, 12, 21, 512, 9), (401, 7, 70, 64, 4), (402, 5, 3, 16, 33)]
PX_CASE = (403, 10, 4, 128, 9)
THR_NA = 7
# route, avg_act, avg_inact, act thresh, inact thresh, motion, classes, first seed, (n, m, E, budget, num_active).  The rounds with data-driven thresholds
# run at E = 16: unrelated 512-dimensional vectors all sit within 0.05 of distance 1, so mean - k std would leave under 15 % of the entries finite.
ROUNDS = [
    (0, {"do": True, "num": 5, "proxy": "each_sample"}, {"do": True, "num": 5, "proxy": "each_sample"}, 1.005, 1.0, True, 2, 420, (24, 30, 512, 8, 14)),
    (0, {"do": False, "num": 4, "proxy": "each_sample"}, {"do": True, "num": 4, "proxy": "each_sample"}, "every", "every", False, 1, 421, (20, 26, 16, 6, 13)),
    (1, {"do": True, "num": 3, "proxy": "mean"}, {"do": True, "num": "all", "proxy": "median"}, "tbd", "tbd", False, 1, 422, (22, 25, 16, 7, 18)),
]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def solve_dense_standin(dist):
    """[detections, tracks] with NaN for impossible pairs -> (rows, cols) of the maximum-cardinality minimum-cost matching, sorted by row."""
    x = solve_clamped(np.asarray(dist, dtype=np.float64), LIMIT)
    rows = np.nonzero(x >= 0)[0]
    return rows, x[rows]


def load_reference():
    def stub(name, **attrs):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
        return mod

    for name in ("matplotlib", "tqdm", "sklearn"):
        try:
            importlib.import_module(name)
        except Exception:
            if name == "matplotlib":
                m = stub("matplotlib")
                m.__path__ = []
                m.pyplot, m.colors = stub("matplotlib.pyplot"), stub("matplotlib.colors")
            elif name == "tqdm":
                stub("tqdm", tqdm=lambda x, **k: x)
            else:
                m = stub("sklearn")
                m.__path__ = []
                m.metrics = stub("sklearn.metrics", average_precision_score=None)
    if not hasattr(np.lib, "arraysetops"):
        np.lib.arraysetops = stub("numpy.lib.arraysetops")
    sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))          # cv2
    stub("lapsolver", solve_dense=solve_dense_standin)
    stub("cython_bbox", bbox_overlaps=None)
    src = stub("src")
    src.__path__ = []
    stub("src.kalman", KalmanFilter=object)
    busca = stub("busca")
    busca.__path__ = []
    stub("busca.network", BUSCA=object)
    stub("busca.tracking", center_distance=None)
    base = os.path.join(REF, "adapters", "GHOST", "src")
    tu = _load("src.tracking_utils", os.path.join(base, "tracking_utils.py"))
    bt = _load("src.base_tracker", os.path.join(base, "base_tracker.py"))
    tr = _load("src.tracker", os.path.join(base, "tracker.py"))
    assert tr.solve_dense is solve_dense_standin
    return tu, bt.BaseTracker, tr.Tracker


def r_cosine(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return 1.0 - (a @ b.T) / (np.sqrt((a * a).sum(1))[:, None] * np.sqrt((b * b).sum(1))[None, :])


REDUCE = {1: lambda c: c.min(0), 2: lambda c: c.mean(0), 3: lambda c: c.max(0), 4: lambda c: (c.max(0) + c.min(0)) / 2, 5: lambda c: np.median(c, 0)}


def chrono(ring, count, newest):
    """The valid rows of one ring, oldest first."""
    budget = ring.shape[0]
    return ring[[(newest - (count - 1) + k) % budget for k in range(count)]]


def tracks_of(trk, count, newest, labels):
    out = {}
    for i in range(len(trk)):
        rows = chrono(trk[i], int(count[i]), int(newest[i]))
        feats = [torch.from_numpy(r.copy()) for r in rows]
        out[100 + i] = types.SimpleNamespace(past_feats=feats, feats=feats[-1], label=[int(labels[i])], inactive_count=0)
    return out


def counts(seed, n, budget, wrap):
    count = 1 + (synth.uniform(seed, "count", (n,), 0.0, 1.0) * budget).astype(np.int64) % budget
    count[0], count[n - 1] = budget, 1
    newest = count - 1
    if wrap:
        full = count == budget
        newest = np.where(full, (synth.uniform(seed, "newest", (n,), 0.0, 1.0) * budget).astype(np.int64) % budget, newest)
    return count.astype(np.int32), newest.astype(np.int32)


def labels_of(seed, n, m, classes):
    tl = (synth.uniform(seed, "tlabel", (n,), 0.0, 1.0) * classes).astype(np.int32) % classes
    dl = (synth.uniform(seed, "dlabel", (m,), 0.0, 1.0) * classes).astype(np.int32) % classes
    return tl, dl


def nan_err(rest, ref):
    assert np.array_equal(np.isnan(rest), np.isnan(ref))
    fin = ~np.isnan(ref)
    return float(np.abs(rest[fin] - np.asarray(ref, dtype=np.float64)[fin]).max()) if fin.any() else 0.0


def namespace(Base, Tracker, cfg, act_thr, inact_thr, motion_dt):
    """What the unbound methods read of `self`."""
    ns = types.SimpleNamespace(tracker_cfg=cfg, motion_model_cfg=cfg["motion_config"], act_reid_thresh=act_thr, inact_reid_thresh=inact_thr,
                               nan_first=cfg["nan_first"], kalman=False, mv_avg={}, inactive_tracks={}, inact_patience=50,
                               thresh_every=act_thr == "every", thresh_tbd=act_thr == "tbd", seen={})
    ns.dist = lambda x, y: Base.dist(ns, x, y)
    ns.last_frame = lambda *a: Tracker.last_frame(ns, *a)
    ns.proxy_dist = lambda *a: Tracker.proxy_dist(ns, *a)
    ns.update_thresholds = lambda *a: Base.update_thresholds(ns, *a)

    def combine(iou, dist):
        ns.seen["masked"] = np.array(dist, copy=True)
        out = Base.combine_motion_appearance(ns, iou, dist)
        ns.seen["blend"] = np.array(out, copy=True)
        return out
    ns.combine_motion_appearance = combine
    ns.motion = lambda *a, **k: None
    ns.get_motion_dist = lambda detections, curr_it: motion_dt

    def solve(dist, *a):
        ns.seen.setdefault("masked", np.array(dist, copy=True))
        return Tracker.solve_hungarian(ns, dist, *a)
    ns.solve_hungarian = solve
    return ns


def restate_round(route, act, inact, act_thr, inact_thr, blend, trk, det, count, newest, tl, dl, na, motion):
    """The round in float64 numpy, tracks x detections -> (masked, blended or None, thresholds, final)."""
    n = len(trk)
    app = np.empty((n, len(det)))
    for i in range(n):
        rows = chrono(trk[i], int(count[i]), int(newest[i]))
        entry = act if i < na else inact
        if route == 0:
            app[i] = REDUCE[inact["num"]](r_cosine(rows, det)) if entry["do"] else r_cosine(rows[-1:], det)[0]
        else:
            w = rows if entry["num"] == "all" or len(rows) < entry["num"] else rows[-entry["num"]:]
            if entry["proxy"] == "mean":
                p = w.astype(np.float64).mean(0).astype(np.float32)
            else:
                p = np.sort(w, 0)[(len(w) - 1) // 2]
            app[i] = r_cosine(p[None], det)[0]
    if route == 0:
        app[tl[:, None] != dl[None, :]] = np.nan
    thr = [act_thr, inact_thr]
    if act_thr in ("every", "tbd"):
        k = (0.0, 2.0) if act_thr == "every" else (0.5, 1.0)
        thr = [app[:na].mean() - k[0] * app[:na].std(), app[na:].mean() - k[1] * app[na:].std()]
    thr = np.asarray(thr, dtype=np.float64)
    pre = (1 - ALPHA) * app + ALPHA * motion if blend else app
    final = pre.copy()
    final[:na] = np.where(final[:na] <= thr[0], final[:na], np.nan)
    final[na:] = np.where(final[na:] <= thr[1], final[na:], np.nan)
    with np.errstate(invalid="ignore"):
        edge = min(np.nanmin(np.abs(pre[:na] - thr[0])), np.nanmin(np.abs(pre[na:] - thr[1])))
    return app, (pre if blend else None), thr, final, edge


def main():
    tu, Base, Tracker = load_reference()
    out = {}
    base_cfg = {"use_bism": False, "distance": "cosine", "nan_first": True, "motion_config": {"apply_motion_model": False, "combi": "sum_%g" % ALPHA}}

    # ---- proxy_dist, last_frame ------------------------------------------------------------------------------------------------
    pd_err, lf_err = [], []
    for k, (seed, n, m, E, budget) in enumerate(DIST_CASES):
        trk, det = synth.appearance_features(seed, n, m, E, budget, twins=True)
        count, newest = counts(seed, n, budget, wrap=False)
        tl, dl = labels_of(seed, n, m, 2)
        tracks = tracks_of(trk, count, newest, tl)
        x = torch.from_numpy(det.copy())
        mask = tl[:, None] != dl[None, :]
        errs = []
        for num in range(1, 6):
            cfg = dict(base_cfg, avg_inact={"do": True, "num": num, "proxy": "each_sample"})
            ns = namespace(Base, Tracker, cfg, 1.0, 1.0, None)
            ref = np.stack([Tracker.proxy_dist(ns, t, x, True, dl) for t in tracks.values()])
            assert ref.shape == (n, m) and ref.dtype == np.float32
            rest = np.stack([REDUCE[num](r_cosine(trk[i, :count[i]], det)) for i in range(n)])
            rest[mask] = np.nan
            out["pd_%d_%d" % (k, num)] = ref
            errs.append(nan_err(rest, ref))
        ids = []
        ref = Tracker.last_frame(ns, ids, tracks, x, True, dl)
        rest = np.stack([r_cosine(trk[i, count[i] - 1:count[i]], det)[0] for i in range(n)])
        rest[mask] = np.nan
        out["lf_%d" % k] = ref
        lf_err.append(nan_err(rest, ref))
        pd_err.append(errs)
        out.update({"dist_count_%d" % k: count, "dist_tlabel_%d" % k: tl, "dist_dlabel_%d" % k: dl})
        print("proxy_dist %2d x %2d x %3d budget %2d: ref_err num 1..5 %s, last_frame %.3g" % (n, m, E, budget, " ".join("%.3g" % e for e in errs), lf_err[-1]))
    out.update(dist_params=np.array(DIST_CASES, dtype=np.int64), pd_err=np.array(pd_err), lf_err=np.array(lf_err))

    # ---- update_thresholds on an unmasked matrix -------------------------------------------------------------------------------
    seed, n, m, E, budget = DIST_CASES[0]
    trk, det = synth.appearance_features(seed, n, m, E, budget, twins=True)
    count, newest = counts(seed, n, budget, wrap=False)
    tracks = tracks_of(trk, count, newest, np.zeros(n, dtype=np.int32))
    ns = namespace(Base, Tracker, dict(base_cfg, avg_inact={"do": True, "num": 2, "proxy": "each_sample"}), 1.0, 1.0, None)
    mat = np.stack([Tracker.proxy_dist(ns, t, torch.from_numpy(det.copy()), False, None) for t in tracks.values()])       # tracks x detections, float32
    rest = np.stack([r_cosine(trk[i, :count[i]], det).mean(0) for i in range(n)])
    for kind, ks in (("every", (0.0, 2.0)), ("tbd", (0.5, 1.0))):
        ns = namespace(Base, Tracker, base_cfg, kind, kind, None)
        Base.update_thresholds(ns, mat.T.copy(), THR_NA, n - THR_NA)
        ref = np.array([ns.act_reid_thresh, ns.inact_reid_thresh], dtype=np.float64)
        want = np.array([rest[:THR_NA].mean() - ks[0] * rest[:THR_NA].std(), rest[THR_NA:].mean() - ks[1] * rest[THR_NA:].std()])
        out["thr_" + kind] = ref
        out["thr_err_" + kind] = np.abs(want - ref).max()
        print("update_thresholds %-5s: %s, ref_err %.3g" % (kind, ref, out["thr_err_" + kind]))
    out["thr_na"] = np.array([THR_NA], dtype=np.int64)

    # ---- get_proxy -----------------------------------------------------------------------------------------------------------------
    seed, n, m, E, budget = PX_CASE
    trk, _ = synth.appearance_features(seed, n, m, E, budget, twins=True)
    count, newest = counts(seed, n, budget, wrap=True)
    assert ((count == budget) & (newest != budget - 1)).any() and (count < 3).any() and (count > 3).any()
    tracks = tracks_of(trk, count, newest, np.zeros(n, dtype=np.int32))
    for mode, avg in (("last", 3), ("mean", 3), ("mean", 40), ("median", 3), ("median", 40), ("meannorm", 40)):
        ref = tu.get_proxy(curr_it=tracks, mode="inact", tracker_cfg={"avg_inact": {"num": avg, "proxy": mode}}, mv_avg=None).numpy()
        assert ref.shape == (n, E) and ref.dtype == np.float32
        rest = []
        for i in range(n):
            rows = chrono(trk[i], int(count[i]), int(newest[i]))
            w = rows if isinstance(avg, str) or len(rows) < avg else rows[-avg:]
            if mode == "last":
                rest.append(rows[-1])
            elif mode == "median":
                rest.append(np.sort(w, 0)[(len(w) - 1) // 2])
            else:
                mu = w.astype(np.float64).mean(0)
                if mode == "meannorm":
                    mu = mu.astype(np.float32).astype(np.float64)
                    mu = mu / max(np.sqrt((mu * mu).sum()), 1e-12)
                rest.append(mu)
        err = float(np.abs(np.asarray(rest, dtype=np.float64) - ref).max())
        assert err == 0.0 or mode in ("mean", "meannorm")
        out["px_%s_%s" % (mode, avg)] = ref
        out["px_err_%s_%s" % (mode, avg)] = err
        print("get_proxy %-8s avg %-5s: ref_err %.3g" % (mode, avg, err))
    out.update(px_params=np.array(PX_CASE, dtype=np.int64), px_count=count, px_newest=newest)

    # ---- whole rounds --------------------------------------------------------------------------------------------------------------
    dropped, candidates, rd_params, rd_err, rd_thr_err = [0, 0], 0, [], [], []
    for q, (route, act, inact, act_thr, inact_thr, blend, classes, seed, (n, m, E, budget, na)) in enumerate(ROUNDS):
        tried = 0
        while True:
            tried += 1
            candidates += 1
            trk, det = synth.appearance_features(seed, n, m, E, budget, twins=True)
            count, newest = counts(seed, n, budget, wrap=True)
            tl, dl = labels_of(seed, n, m, classes)
            motion = synth.tracker_costs(seed, n, m)
            r_masked, r_blend, r_thr, r_final, edge = restate_round(route, act, inact, act_thr, inact_thr, blend, trk, det, count, newest, tl, dl, na, motion)
            res = {}
            for sep in (0, 1):
                cfg = dict(base_cfg, avg_act=act, avg_inact=inact, motion_config={"apply_motion_model": blend, "combi": "sum_%g" % ALPHA})
                ns = namespace(Base, Tracker, cfg, act_thr, inact_thr, motion.T.copy())
                tracks = tracks_of(trk, count, newest, tl)
                ids = list(tracks)
                ns.tracks = {i: tracks[i] for i in ids[:na]}
                ns.curr_it = {i: tracks[i] for i in ids[na:]}
                ns.inactive_tracks = ns.curr_it
                dets = [{"feats": torch.from_numpy(det[j].copy()), "label": int(dl[j])} for j in range(m)]
                fn = Tracker.get_hungarian_each_sample if route == 0 else Tracker.get_hungarian_with_proxy
                dist, row, col, got_ids = fn(ns, dets, sep=bool(sep))
                assert got_ids == ids
                if sep:
                    dist = np.hstack(dist)
                res[sep] = (np.asarray(dist), np.asarray(row), np.asarray(col), np.array([ns.act_reid_thresh, ns.inact_reid_thresh], dtype=np.float64), ns.seen)
            ref = res[0][0]
            assert np.array_equal(res[0][0], res[1][0], equal_nan=True) and ref.shape == (m, n)
            if edge < 1e-6:
                dropped[0] += 1
                seed += 100
                continue
            ok = True
            for sep, rows in ((0, n), (1, na)):
                c = np.asarray(ref, dtype=np.float64).T[:rows]
                x = solve_clamped(c, LIMIT)
                xr = solve_clamped(r_final[:rows], LIMIT)
                ok = ok and unique(c, LIMIT, x) and np.array_equal(x, xr)
                if ok:                                            # a unique optimum is the same in either orientation
                    assert np.array_equal(np.nonzero(x >= 0)[0], np.sort(res[sep][2])) and np.array_equal(x[res[sep][2]], res[sep][1])
            if not ok:
                dropped[1] += 1
                seed += 100
                continue
            break
        err = nan_err(r_final.T, ref)
        fin = np.isfinite(ref).mean()
        assert 0.2 <= fin <= 0.8, fin
        seen = res[0][4]
        out["rd_masked_%d" % q] = seen["masked"]
        out["rd_masked_err_%d" % q] = nan_err(r_masked.T, seen["masked"])
        if blend:
            out["rd_blend_%d" % q] = seen["blend"]
            out["rd_blend_err_%d" % q] = nan_err(r_blend.T, seen["blend"])
        out.update({"rd_dist_%d" % q: ref, "rd_thr_%d" % q: res[0][3], "rd_count_%d" % q: count, "rd_newest_%d" % q: newest, "rd_tlabel_%d" % q: tl,
                    "rd_dlabel_%d" % q: dl})
        for sep in (0, 1):
            out["rd_row_%d_%d" % (q, sep)] = res[sep][1].astype(np.int64)
            out["rd_col_%d_%d" % (q, sep)] = res[sep][2].astype(np.int64)
            assert len(res[sep][1]) >= 5
        assert not np.array_equal(res[0][1], res[1][1]) or not np.array_equal(res[0][2], res[1][2])      # sep decides differently
        rd_params.append([seed, n, m, E, budget, na, route, tried])
        rd_err.append(err)
        rd_thr_err.append(float(np.abs(r_thr - res[0][3]).max()))
        print("round %d (route %d): seed %d, %d x %d, %.0f %% finite, thresholds %s, %d / %d matches, ref_err %.3g, thr ref_err %.3g, edge %.3g, tried %d"
              % (q, route, seed, n, m, 100 * fin, res[0][3], len(res[0][1]), len(res[1][1]), err, rd_thr_err[-1], edge, tried))
    assert 10 * sum(dropped) <= candidates, (dropped, candidates)
    out.update(rd_params=np.array(rd_params, dtype=np.int64), rd_err=np.array(rd_err), rd_thr_err=np.array(rd_thr_err),
               dropped=np.array(dropped, dtype=np.int64), candidates=np.array([candidates], dtype=np.int64), alpha=np.array([ALPHA]))
    print("round candidates: %d tried, dropped %d knife-edge, %d non-unique" % (candidates, dropped[0], dropped[1]))

    path = os.path.join(OUT, "ghost.npz")
    np.savez_compressed(path, **out)
    print("wrote ghost.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
