#!/usr/bin/env python3
"""Generate tests/golden/appearance.npz, the fixture of tests/test_appearance.py.  Run from the repo root where the reference is present:

    python tests/golden/make_golden_appearance.py

The fixture holds arrays only: parameters and recorded outputs.  Features are not stored: a case is (seed, n, m, E, budget) and the test rebuilds
its vectors with busca_amd.synth.appearance_features, which is bit-reproducible everywhere.  Kalman states and measurements are kalman.npz's.

  emb_params [K,4]              embedding_distance cases: seed, n, m, E
  emb_<k> [n,m]                 matching.embedding_distance (adapters/ByteTrack/yolox/tracker/matching.py:113-129) of case k
  restatement_err_emb [K]       the largest disagreement of a LAPACK-free, left-to-right numpy float64 restatement with emb_<k>
  restatement_err_emb_f32 [K]   the same restatement carried out in float32, for scale
  fuse_params [4]               fuse_iou case: feature seed, box seed, n, m  (boxes: synth.tracker_boxes; cost: embedding_distance at E = 128)
  fuse_cost, fuse_ref [n,m]     its input cost and matching.fuse_iou (matching.py:159-170); restatement_err_fuse
  gate_params [5]               gating / matching cases: feature seed, E, samples per track, MC_lambda, max_distance.  Tracks: kalman.npz's 96 states,
                                track_id 100 + i, time_since_update 1 + i mod 4, features with `twins`; detections: kalman.npz's 40 gate_meas.
  gate_ti, gate_di              track_indices / detection_indices
  gate_cost [96,40]             the nearest-neighbour cost: min over a track's samples of embedding_distance
  gate_ref_mc0 / gate_ref_mc1   linear_assignment.gate_cost_matrix (adapters/StrongSORT/deep_sort/linear_assignment.py:164-210) of
                                gate_cost[ti x di], opt.MC off / on; restatement_err_gate_mc0 / _mc1 against the recorded gating distances
  mcm_matches [k,2], mcm_ut, mcm_ud         linear_assignment.min_cost_matching (:15-85) on gate_cost, over gate_ti x gate_di
  casc_<woc>_matches, _ut, _ud              linear_assignment.matching_cascade (:88-162), opt.woC off (0) / on (1), cascade depth 4
  dropped                       candidates dropped: [gate knife-edge, non-unique or knife-edge matching]

The reference's functions are imported from their files with stand-in modules: `lap` (never called here), `cython_bbox.bbox_overlaps` (the
oracle's restatement of its '+1' pixel IoU), `cv2` (oracle/ref_shims), `yolox.tracker.kalman_filter` / `deep_sort.kalman_filter` (the vendored
mot_online KalmanFilter, which the track objects also carry as `.kf`), `opts.opt`, and np.float = float for the pinned numpy 1.23 spelling.

A gate case is kept only if no gating distance lies within 1e-9 of chi2inv95[4]; a matching case only if at every level no cost lies within
1e-4 of max_distance and the optimum is unique by more than 1e-9 (make_golden_assign.unique).  Others are dropped (next seed) and counted."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from busca_amd import synth  # noqa: E402
from make_golden_assign import solve_clamped, unique  # noqa: E402
from oracle import geometry as ogeo  # noqa: E402

SIZES = [(1, 1), (15, 17), (16, 16), (17, 15), (33, 65), (97, 53)]
DIMS = [16, 128, 512, 2048]
EMB_SEED = 300
MC_LAMBDA, MAX_DISTANCE, DEPTH = 0.98, 0.45, 4


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    if not hasattr(np, "float"):
        np.float = float
    kfm = _load("ref_kalman_filter", os.path.join(REF, "adapters/CenterTrack/src/lib/utils/mot_online/kalman_filter.py"))
    sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))          # cv2
    lap = types.ModuleType("lap")
    cb = types.ModuleType("cython_bbox")
    cb.bbox_overlaps = lambda a, b: ogeo.iou_matrix(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    yolox, tracker = types.ModuleType("yolox"), types.ModuleType("yolox.tracker")
    yolox.__path__, tracker.__path__ = [], []
    yolox.tracker, tracker.kalman_filter = tracker, kfm
    opts = types.ModuleType("opts")
    opts.opt = types.SimpleNamespace(MC=False, MC_lambda=MC_LAMBDA, woC=False)
    pkg = types.ModuleType("deep_sort")
    pkg.__path__ = []
    pkg.kalman_filter = kfm
    sys.modules.update({"lap": lap, "cython_bbox": cb, "yolox": yolox, "yolox.tracker": tracker, "yolox.tracker.kalman_filter": kfm, "opts": opts,
                        "deep_sort": pkg, "deep_sort.kalman_filter": kfm})
    matching = _load("yolox.tracker.matching", os.path.join(REF, "adapters/ByteTrack/yolox/tracker/matching.py"))
    la = _load("deep_sort.linear_assignment", os.path.join(REF, "adapters/StrongSORT/deep_sort/linear_assignment.py"))
    return kfm, matching, la, opts.opt


def restate_cosine(a, b, dt):
    """max(0, 1 - <a_i, b_j> / (sqrt <a_i, a_i> sqrt <b_j, b_j>)) with every sum left to right in `dt`, no BLAS / LAPACK."""
    a, b = a.astype(dt), b.astype(dt)
    dot = np.zeros((a.shape[0], b.shape[0]), dtype=dt)
    na, nb = np.zeros(a.shape[0], dtype=dt), np.zeros(b.shape[0], dtype=dt)
    for k in range(a.shape[1]):
        dot += a[:, k, None] * b[None, :, k]
        na += a[:, k] * a[:, k]
        nb += b[:, k] * b[:, k]
    return np.maximum(dt(0), dt(1) - dot / (np.sqrt(na)[:, None] * np.sqrt(nb)[None, :]))


def feat_objs(f, attr):
    return [types.SimpleNamespace(**{attr: v}) for v in f]


def main():
    kfm, matching, la, opt = load_reference()
    out = {}

    # ---- embedding_distance ------------------------------------------------------------------------------------------------
    params, e64, e32 = [], [], []
    for E in DIMS:
        for n, m in SIZES:
            k = len(params)
            trk, det = synth.appearance_features(EMB_SEED + k, n, m, E)
            ref = matching.embedding_distance(feat_objs(trk[:, 0], "smooth_feat"), feat_objs(det, "curr_feat"))
            assert ref.shape == (n, m) and ref.dtype == np.float64 and np.isfinite(ref).all()
            params.append([EMB_SEED + k, n, m, E])
            out["emb_%d" % k] = ref
            e64.append(np.abs(restate_cosine(trk[:, 0], det, np.float64) - ref).max())
            e32.append(np.abs(restate_cosine(trk[:, 0], det, np.float32).astype(np.float64) - ref).max())
            print("embedding_distance %3d x %3d x %4d: cost %.4f .. %.4f, restatement f64 %.3g, f32 %.3g" % (n, m, E, ref.min(), ref.max(), e64[-1], e32[-1]))
    out.update(emb_params=np.array(params, dtype=np.int64), restatement_err_emb=np.array(e64), restatement_err_emb_f32=np.array(e32))

    # ---- fuse_iou ------------------------------------------------------------------------------------------------------------
    fseed, bseed, n, m = 340, 341, 37, 41
    trk, det = synth.appearance_features(fseed, n, m, 128)
    tb, db = synth.tracker_boxes(bseed, n, m)
    cost = matching.embedding_distance(feat_objs(trk[:, 0], "smooth_feat"), feat_objs(det, "curr_feat"))
    tobj = [types.SimpleNamespace(tlbr=b) for b in tb]
    dobj = [types.SimpleNamespace(tlbr=b, score=0.9) for b in db]
    fref = matching.fuse_iou(cost.copy(), tobj, dobj)
    frest = 1 - (1 - cost) * (1 + (1 - ogeo.iou_distance(tb, db))) / 2
    out.update(fuse_params=np.array([fseed, bseed, n, m], dtype=np.int64), fuse_cost=cost, fuse_ref=fref, restatement_err_fuse=np.abs(frest - fref).max())
    assert (ogeo.iou_distance(tb, db) < 1).sum() >= 20
    print("fuse_iou %d x %d: %.4f .. %.4f, restatement %.3g" % (n, m, fref.min(), fref.max(), out["restatement_err_fuse"]))

    # ---- gate_cost_matrix, min_cost_matching, matching_cascade -------------------------------------------------------------------
    with np.load(os.path.join(OUT, "kalman.npz")) as f:
        mean, cov, meas = f["mean"], f["cov"], f["gate_meas"]
    N, M, E, NS = len(mean), len(meas), 512, 2
    kf = kfm.KalmanFilter()
    thr = kfm.chi2inv95[4]
    gdist = np.asarray([kf.gating_distance(mean[i], cov[i], meas, False) for i in range(N)])
    drop_gate = drop_match = 0
    assert np.abs(gdist - thr).min() > 1e-9                     # kalman.npz keeps no knife-edge entry; a failure here would count as a dropped gate case
    seed = 350
    while True:
        trk, det = synth.appearance_features(seed, N, M, E, NS, twins=True)
        full = np.minimum.reduce([matching.embedding_distance(feat_objs(trk[:, s], "smooth_feat"), feat_objs(det, "curr_feat")) for s in range(NS)])
        ti = [int(i) for i in np.nonzero(synth.uniform(seed, "ti", (N,), 0.0, 1.0) < 0.85)[0]]
        di = [int(j) for j in np.nonzero(synth.uniform(seed, "di", (M,), 0.0, 1.0) < 0.9)[0]]
        tracks = [types.SimpleNamespace(mean=mean[i], covariance=cov[i], kf=kf, track_id=100 + i, time_since_update=1 + i % 4) for i in range(N)]
        dets = [types.SimpleNamespace(to_xyah=(lambda z=meas[j]: z)) for j in range(M)]
        sub = full[np.ix_(ti, di)]
        gated = {}
        for mc in (False, True):
            opt.MC = mc
            gated[mc] = la.gate_cost_matrix(sub.copy(), tracks, dets, ti, di)
        whole = full                                             # the matching cases run on the appearance cost itself, indexed by (track, detection)
        metric = lambda tr, de, a, b: whole[np.ix_(a, b)].copy()      # noqa: E731
        limit = MAX_DISTANCE + 1e-5

        def level_ok(rows, cols):
            s = whole[np.ix_(rows, cols)]
            return np.abs(s - MAX_DISTANCE).min() > 1e-4 and unique(np.where(s > MAX_DISTANCE, limit, s), limit, solve_clamped(np.where(s > MAX_DISTANCE, limit, s), limit))

        ok, res = level_ok(ti, di), {}
        opt.woC = False
        mcm = la.min_cost_matching(metric, MAX_DISTANCE, tracks, dets, list(ti), list(di))
        for woc in (0, 1):
            opt.woC = bool(woc)
            res[woc] = la.matching_cascade(metric, MAX_DISTANCE, DEPTH, tracks, dets, list(ti), list(di))
        left = list(di)                                           # replay the cascade's levels to prove each level's optimum unique
        for level in range(DEPTH):
            rows = [k for k in ti if tracks[k].time_since_update == 1 + level]
            if not left or not rows:
                continue
            ok = ok and level_ok(rows, left)
            taken = set(d for t, d in res[0][0] if t in rows)
            left = [d for d in left if d not in taken]
        if ok:
            break
        drop_match += 1
        seed += 100
    gsub = gdist[np.ix_(ti, di)]
    for mc in (False, True):
        r = sub.copy()
        r[gsub > thr] = la.INFTY_COST
        if mc:
            r = MC_LAMBDA * r + (1 - MC_LAMBDA) * gsub
        out["gate_ref_mc%d" % mc] = gated[mc]
        out["restatement_err_gate_mc%d" % mc] = np.abs(r - gated[mc]).max()
    ngated = int((gsub > thr).sum())
    assert 30 <= ngated <= gsub.size - 30
    assert len(mcm[0]) >= 8 and len(res[0][0]) >= 8 and len(res[1][0]) >= 8 and len(res[0][2]) >= 1 and sorted(res[0][0]) != sorted(res[1][0])
    out.update(gate_params=np.array([seed, E, NS, MC_LAMBDA, MAX_DISTANCE]), gate_ti=np.array(ti, dtype=np.int64), gate_di=np.array(di, dtype=np.int64),
               gate_cost=full, mcm_matches=np.array(mcm[0], dtype=np.int64).reshape(-1, 2), mcm_ut=np.array(mcm[1], dtype=np.int64),
               mcm_ud=np.array(mcm[2], dtype=np.int64), dropped=np.array([drop_gate, drop_match], dtype=np.int64))
    for woc in (0, 1):
        out.update({"casc_%d_matches" % woc: np.array(res[woc][0], dtype=np.int64).reshape(-1, 2), "casc_%d_ut" % woc: np.array(res[woc][1], dtype=np.int64),
                    "casc_%d_ud" % woc: np.array(res[woc][2], dtype=np.int64)})
    print("gate %d x %d: %d gated entries; min_cost_matching %d matches; cascade %d matches (woC %d); dropped %d gate, %d matching candidates"
          % (len(ti), len(di), ngated, len(mcm[0]), len(res[0][0]), len(res[1][0]), drop_gate, drop_match))

    path = os.path.join(OUT, "appearance.npz")
    np.savez_compressed(path, **out)
    print("wrote appearance.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
