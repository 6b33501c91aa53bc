"""Appearance association on the device: busca_appearance_cost (include/busca_appearance.h) and its mirrors in busca_amd.tracking
(appearance_cost, embedding_distance, fuse_iou, NearestNeighborDistanceMetric, gate_cost_matrix_mc, matching_cascade, appearance_round).

The reference is tests/golden/appearance.npz, written by tests/golden/make_golden_appearance.py from the reference's own functions; the
features are rebuilt from busca_amd.synth seeds, the Kalman states and measurements are kalman.npz's.

Bars, none of them taken from a kernel's output:
  * plain flavour against matching.embedding_distance: 20 x the fixture's `restatement_err_emb` of the same case - the largest disagreement of
    a left-to-right numpy float64 restatement with the reference (scipy's cdist).  The kernel's order is a third valid one; 20 x leaves room
    for it without hiding a wrong formula (the same computation in float32 errs at 1e-7, a wrong one at 1e-3 or worse).
  * gallery flavour against a numpy restatement: u = 2^-53; a dot product or squared norm of E terms summed in any order is off by at most
    E u relative to sum |x_k y_k| <= |x| |y|, so a cosine is off by at most (2 E + 4) u whichever way it is summed, two evaluations of it
    differ by at most (4 E + 8) u, and the mean of up to `budget` distances (each at most 2) adds 2 (budget + 1) u:
    bar = (4 E + 8 + 2 (budget + 1)) u.  min / max select one of the distances and stay inside the same bar.
  * gating, fuse_iou: the bars tests/test_kalman_filter.py derives for busca_kalman_gating (20 x its restatement's error).
  * matches: exact.  The generator keeps a matching case only if every level's optimum is unique by more than 1e-9 and no cost lies within
    1e-4 of max_distance.

Measured on an MI355X (printed by the tests, copied into DESIGN.md, "K-APPEAR"): plain flavour at most 4.4e-16 / 1.4e-15 / 2.0e-15 / 4.8e-15
at E = 16 / 128 / 512 / 2048; gallery flavour 7.8e-16 at E = 48, 3.2e-15 at E = 512."""
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "appearance.npz")
KALMAN = os.path.join(ROOT, "tests", "golden", "kalman.npz")
U = 2.0 ** -53
SIZES = [(1, 1), (15, 17), (16, 16), (17, 15), (33, 65), (97, 53)]
DIMS = [16, 128, 512, 2048]
CHI2_4 = 9.4877

_CACHE = {}


def gold():
    if "g" not in _CACHE:
        with np.load(GOLD) as f:
            _CACHE["g"] = {k: f[k] for k in f.files}
    return _CACHE["g"]


def kalman():
    if "k" not in _CACHE:
        with np.load(KALMAN) as f:
            _CACHE["k"] = {k: f[k] for k in ("mean", "cov", "gate_meas", "gate_maha4")}
    return _CACHE["k"]


def gate_case():
    """Features, tracks and detections of the fixture's gating / matching case, built once."""
    if "gate" not in _CACHE:
        from busca_amd import synth
        g, k = gold(), kalman()
        seed, E, ns = int(g["gate_params"][0]), int(g["gate_params"][1]), int(g["gate_params"][2])
        trk, det = synth.appearance_features(seed, 96, 40, E, ns, twins=True)
        trk.setflags(write=False)
        det.setflags(write=False)
        _CACHE["gate"] = (trk, det, float(g["gate_params"][3]), float(g["gate_params"][4]))
    trk, det, lam, maxd = _CACHE["gate"]
    k = kalman()
    tracks = [types.SimpleNamespace(mean=k["mean"][i].copy(), covariance=k["cov"][i].copy(), track_id=100 + i, time_since_update=1 + i % 4) for i in range(96)]
    dets = [types.SimpleNamespace(to_xyah=(lambda z=k["gate_meas"][j]: z.copy()), feature=det[j]) for j in range(40)]
    return trk, det, lam, maxd, tracks, dets


def r_cosine(a, b):
    """[n,E] x [m,E] float32 -> float64 cosine distances, numpy."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    return 1.0 - (a @ b.T) / (np.sqrt((a * a).sum(1))[:, None] * np.sqrt((b * b).sum(1))[None, :])


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_symbol_declared_typed_and_exported():
    from busca_amd.build import build
    build()
    from busca_amd import _lib

    def declared(header):
        hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return set(re.findall(r"\b(busca_[a-z0-9_]+)\s*\(", hdr))
    assert declared("busca_appearance.h") == {"busca_appearance_cost"} == set(_lib.APPEARANCE_SIGNATURES)
    for header, table in _lib.HEADERS.items():
        if header == "busca_appearance.h":
            continue
        assert "busca_appearance_cost" not in declared(header) and "busca_appearance_cost" not in table
    lib = _lib.load()
    fn = lib.busca_appearance_cost
    assert fn.restype is not None and len(fn.argtypes) == 13
    assert lib.busca_version() >= 2002 and lib.busca_version() // 1000 == 2
    assert (_lib.APPEAR_MIN, _lib.APPEAR_MEAN, _lib.APPEAR_MAX, _lib.APPEAR_CLAMP0) == (0, 1, 2, 1)
    hdr = open(os.path.join(ROOT, "include", "busca_appearance.h")).read()
    for name, val in (("BUSCA_APPEAR_MIN", 0), ("BUSCA_APPEAR_MEAN", 1), ("BUSCA_APPEAR_MAX", 2), ("BUSCA_APPEAR_CLAMP0", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name


def test_mirrors_reachable_from_the_alias_package():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "busca_amd", "compat"))
    try:
        import busca.tracking as bt
    finally:
        sys.path.pop(0)
    for name in ("appearance_cost", "embedding_distance", "fuse_iou", "NearestNeighborDistanceMetric", "gate_cost_matrix_mc", "matching_cascade", "appearance_round"):
        assert callable(getattr(bt, name)), name


def test_fixture_contents():
    from busca_amd import synth
    g = gold()
    p = g["emb_params"]
    assert [(int(n), int(m)) for _, n, m, E in p if E == 512] == SIZES and sorted(set(int(E) for E in p[:, 3])) == DIMS and len(p) == len(SIZES) * len(DIMS)
    assert g["restatement_err_emb"].shape == (len(p),) and (g["restatement_err_emb"] > 0).all() and g["restatement_err_emb"].max() < 1e-13
    assert g["restatement_err_emb_f32"].min() > 1e-10                    # float32 would not pass: the bars tell the two apart
    lo, hi = 1.0, 0.0
    for k, (seed, n, m, E) in enumerate(p):
        ref = g["emb_%d" % k]
        assert ref.shape == (n, m) and ref.dtype == np.float64 and np.isfinite(ref).all() and ref.min() >= 0
        lo, hi = min(lo, ref.min()), max(hi, ref.max())
    assert lo < 0.01 and hi > 0.9                                         # costs span 0 to about 1
    seed, n, m, E = [int(v) for v in p[-1]]
    trk, det = synth.appearance_features(seed, n, m, E)
    assert trk.dtype == det.dtype == np.float32 and (np.abs(trk).sum(-1) > 0).all() and (np.abs(det).sum(-1) > 0).all()   # no zero-norm vector
    assert np.abs(np.maximum(0, r_cosine(trk[:, 0], det)) - g["emb_%d" % (len(p) - 1)]).max() < 1e-13     # the seeds rebuild the recorded case
    assert g["fuse_ref"].shape == g["fuse_cost"].shape == (37, 41) and float(g["restatement_err_fuse"]) < 1e-14
    ti, di = g["gate_ti"], g["gate_di"]
    assert g["gate_cost"].shape == (96, 40) and g["gate_ref_mc0"].shape == g["gate_ref_mc1"].shape == (len(ti), len(di))
    gm = kalman()["gate_maha4"][np.ix_(ti, di)]
    assert np.abs(gm - CHI2_4).min() > 1e-9                               # no knife-edge entry at the gate
    assert np.array_equal(g["gate_ref_mc0"] == 1e5, gm > CHI2_4) and 30 <= (gm > CHI2_4).sum() <= gm.size - 30
    assert float(g["restatement_err_gate_mc0"]) == 0.0 and float(g["restatement_err_gate_mc1"]) < 1e-10
    assert len(g["mcm_matches"]) >= 8 and len(g["casc_0_matches"]) >= 8 and len(g["casc_1_matches"]) >= 8
    assert sorted(map(tuple, g["casc_0_matches"])) != sorted(map(tuple, g["casc_1_matches"]))     # the cascade decides differently from one problem
    assert g["dropped"].shape == (2,)
    assert os.path.getsize(GOLD) < 1 << 20


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from busca_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("E", DIMS)
def test_plain_flavour_against_embedding_distance(ctx, E):
    from busca_amd import synth, tracking
    g = gold()
    for k, (seed, n, m, e) in enumerate(g["emb_params"]):
        if e != E:
            continue
        trk, det = synth.appearance_features(int(seed), int(n), int(m), int(E))
        ref, bar = g["emb_%d" % k], 20.0 * g["restatement_err_emb"][k]
        raw = tracking.appearance_cost(trk[:, 0], det, clamp=True, ctx=ctx).cpu().numpy()
        got = tracking.embedding_distance(trk[:, 0], det, ctx=ctx)
        objs = tracking.embedding_distance([types.SimpleNamespace(smooth_feat=v) for v in trk[:, 0]], [types.SimpleNamespace(curr_feat=v) for v in det], ctx=ctx)
        err = np.abs(got - ref).max()
        print("plain %3d x %3d x %4d: max |d| %.3g, bar %.3g" % (n, m, E, err, bar))
        assert got.shape == (n, m) and got.dtype == np.float64 and np.array_equal(got, raw) and np.array_equal(got, objs)
        assert err <= bar
        unclamped = tracking.appearance_cost(trk[:, 0], det, ctx=ctx).cpu().numpy()
        assert np.array_equal(np.maximum(0.0, unclamped), got)
    # identical vectors: exactly 0 with the clamp, wherever the pair sits in its tile
    trk, det = synth.appearance_features(900 + E, 97, 53, E)
    both = np.concatenate([trk[:, 0], det])
    d = tracking.appearance_cost(both, both, clamp=True, ctx=ctx).cpu().numpy()
    assert np.array_equal(np.diag(d), np.zeros(len(both)))
    d = tracking.appearance_cost(both, both[::-1].copy(), clamp=True, ctx=ctx).cpu().numpy()
    assert np.array_equal(np.diag(d[:, ::-1]), np.zeros(len(both)))


def test_embedding_distance_empty_and_metric():
    from busca_amd import tracking
    assert tracking.embedding_distance([], [1, 2, 3]).shape == (0, 3) and tracking.embedding_distance(np.zeros((4, 16), np.float32), []).shape == (4, 0)
    assert tracking.embedding_distance([], []).dtype == np.float64
    with pytest.raises(ValueError):
        tracking.embedding_distance(np.zeros((4, 16), np.float32), np.zeros((4, 16), np.float32), metric="euclidean")


def _gallery_case(budget, E, S=9, m=70):
    from busca_amd import synth
    trk, det = synth.appearance_features(500 + budget, S, m, E, budget)
    count = np.array([0, budget, 1, min(2, budget), budget // 2, max(budget - 1, 0), min(16, budget), budget, min(15, budget)], dtype=np.int32)[:S]
    slot = np.array([4, -1, 0, 8, 1, 1, 7, 3, -5, 2, 6, 5], dtype=np.int32)
    poisoned = trk.copy()
    for s in range(S):
        poisoned[s, count[s]:] = np.nan
    return trk, poisoned, det, count, slot


def _r_gallery(trk, det, count, slot, reduce, clamp):
    out = np.full((len(slot), len(det)), np.inf)
    for i, s in enumerate(slot):
        if s < 0 or count[s] == 0:
            continue
        c = r_cosine(trk[s, :count[s]], det)
        if clamp:
            c = np.maximum(0.0, c)
        out[i] = {"min": c.min(0), "mean": c.mean(0), "max": c.max(0)}[reduce]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("budget", [1, 3, 16, 17, 100])
def test_gallery_flavour_against_restatement(ctx, budget):
    from busca_amd import tracking
    for E in (48, 512):
        trk, poisoned, det, count, slot = _gallery_case(budget, E)
        bar = (4 * E + 8 + 2 * (budget + 1)) * U
        for reduce in ("min", "mean", "max"):
            for clamp in (False, True):
                ref = _r_gallery(trk, det, count, slot, reduce, clamp)
                got = tracking.appearance_cost(poisoned, det, reduce, clamp, slot=slot, count=count, ctx=ctx).cpu().numpy()
                assert got.shape == ref.shape and not np.isnan(got).any()            # the NaN rows beyond `count` never reach the output
                empty = np.isinf(ref)
                assert np.array_equal(np.isposinf(got), empty) and empty[[1, 8]].all() and empty[2].all()      # negative slot, count 0: +inf rows
                err = np.abs(got[~empty] - ref[~empty]).max()
                print("gallery budget %3d E %3d %-4s clamp %d: max |d| %.3g, bar %.3g" % (budget, E, reduce, clamp, err, bar))
                assert err <= bar
        # slot = None: row i is slot i; count = None: every row of the ring is valid
        got = tracking.appearance_cost(poisoned, det, "min", count=count, ctx=ctx).cpu().numpy()
        ref = _r_gallery(trk, det, count, np.arange(len(count)), "min", False)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isposinf(got), ~fin) and np.abs(got[fin] - ref[fin]).max() <= bar
        got = tracking.appearance_cost(trk, det, "max", slot=slot, ctx=ctx).cpu().numpy()
        ref = _r_gallery(trk, det, np.full(len(count), budget), slot, "max", False)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isposinf(got), ~fin) and np.abs(got[fin] - ref[fin]).max() <= bar


@pytest.mark.gpu
def test_zero_norm_gives_nan(ctx):
    from busca_amd import synth, tracking
    trk, det = synth.appearance_features(77, 5, 6, 32, 3)
    trk, det = trk.copy(), det.copy()
    det[2] = 0.0
    trk[3, 1] = 0.0
    got = tracking.appearance_cost(trk, det, "min", clamp=True, ctx=ctx).cpu().numpy()
    want = np.zeros((5, 6), dtype=bool)
    want[:, 2] = True
    want[3, :] = True                                                     # a NaN among a track's distances makes its reduced cost NaN, as numpy's min does
    assert np.array_equal(np.isnan(got), want)
    got = tracking.appearance_cost(trk[:, 0], det, clamp=True, ctx=ctx).cpu().numpy()
    want[3, :] = False
    want[:, 2] = True
    assert np.array_equal(np.isnan(got), want)


@pytest.mark.gpu
def test_determinism_and_row_independence(ctx):
    from busca_amd import synth, tracking
    trk, det = synth.appearance_features(610, 97, 150, 512, 17)
    a = tracking.appearance_cost(trk[:, 0], det, ctx=ctx).cpu().numpy()
    b = tracking.appearance_cost(trk[:, 0], det, ctx=ctx).cpu().numpy()
    assert np.array_equal(a, b)
    rows = np.array([5, 40, 41, 96, 0, 17])
    assert np.array_equal(tracking.appearance_cost(trk[rows, 0], det, ctx=ctx).cpu().numpy(), a[rows])
    assert np.array_equal(tracking.appearance_cost(trk[3:50, 0], det, ctx=ctx).cpu().numpy(), a[3:50])
    count = (np.arange(97) % 18).astype(np.int32)
    for reduce in ("min", "mean", "max"):
        a = tracking.appearance_cost(trk, det, reduce, count=count, ctx=ctx).cpu().numpy()
        b = tracking.appearance_cost(trk, det, reduce, count=count, ctx=ctx).cpu().numpy()
        assert np.array_equal(a, b)
        sub = tracking.appearance_cost(trk, det, reduce, slot=rows.astype(np.int32), count=count, ctx=ctx).cpu().numpy()
        assert np.array_equal(sub, a[rows])
        # the same samples in another gallery, at other slots
        moved = tracking.appearance_cost(trk[rows], det, reduce, count=count[rows], ctx=ctx).cpu().numpy()
        assert np.array_equal(moved, a[rows])


@pytest.mark.gpu
def test_fuse_iou_against_the_reference(ctx):
    import torch
    from busca_amd import synth, tracking
    from tests import test_kalman_filter as tkf
    g = gold()
    _, bar = tkf.bars()
    fseed, bseed, n, m = [int(v) for v in g["fuse_params"]]
    tb, db = synth.tracker_boxes(bseed, n, m)
    tracks, dets = [types.SimpleNamespace(tlbr=b) for b in tb], [types.SimpleNamespace(tlbr=b, score=0.9) for b in db]
    got = tracking.fuse_iou(g["fuse_cost"].copy(), tracks, dets, ctx=ctx)
    err = tkf.err_gate(got, g["fuse_ref"])
    print("fuse_iou: max |d| / max(1, |ref|) %.3g, bar %.3g" % (err, bar["gate"]))
    assert got.shape == (n, m) and err <= bar["gate"]
    dcost = torch.from_numpy(g["fuse_cost"]).to(torch.device("cuda", 0))
    assert np.array_equal(tracking.fuse_iou(dcost, tracks, dets, ctx=ctx), got) and np.array_equal(dcost.cpu().numpy(), g["fuse_cost"])
    # the whole ByteTrack chain from features: embedding_distance on the device, then fuse_iou
    trk, det = synth.appearance_features(fseed, n, m, 128)
    chain = tracking.fuse_iou(tracking.appearance_cost(trk[:, 0], det, clamp=True, ctx=ctx), tracks, dets, ctx=ctx)
    assert np.abs(chain - g["fuse_ref"]).max() <= 20.0 * g["restatement_err_emb"][g["emb_params"][:, 3] == 128].max() + bar["gate"] * 2
    empty = np.zeros((0, m))
    assert tracking.fuse_iou(empty, [], dets, ctx=ctx) is empty


@pytest.mark.gpu
def test_gate_cost_matrix_mc_against_the_reference(ctx):
    from busca_amd import tracking
    from tests import test_kalman_filter as tkf
    g = gold()
    _, bar = tkf.bars()
    trk, det, lam, maxd, tracks, dets = gate_case()
    ti, di = [int(i) for i in g["gate_ti"]], [int(j) for j in g["gate_di"]]
    cost = g["gate_cost"][np.ix_(ti, di)]
    gate = kalman()["gate_maha4"][np.ix_(ti, di)]
    got = tracking.gate_cost_matrix_mc(cost.copy(), tracks, dets, ti, di, ctx=ctx)
    assert np.array_equal(got, g["gate_ref_mc0"])                        # 1e5 exactly where the reference gates, the cost elsewhere
    got = tracking.gate_cost_matrix_mc(cost.copy(), tracks, dets, ti, di, mc_lambda=lam, ctx=ctx)
    ref = g["gate_ref_mc1"]
    assert np.array_equal(got > 1e4, ref > 1e4) and np.array_equal(ref > 1e4, gate > CHI2_4)      # the identical set of gated entries
    # the only term that may differ is (1 - lambda) * distance, by the gating bar; two roundings on top
    tol = (1 - lam) * bar["gate"] * np.maximum(1.0, np.abs(gate)) + 4 * np.finfo(np.float64).eps * np.abs(ref)
    print("gate_cost_matrix_mc: max |d| %.3g" % np.abs(got - ref).max())
    assert (np.abs(got - ref) <= tol).all()
    assert np.array_equal(tracking.gate_cost_matrix_mc(cost.copy(), tracks, dets, ti, di, gated_cost=7.0, ctx=ctx) == 7.0, gate > CHI2_4)
    empty = np.zeros((0, len(di)))
    assert tracking.gate_cost_matrix_mc(empty, tracks, dets, [], di, ctx=ctx) is empty


def _fitted_metric(ctx, trk, threshold, budget=None):
    from busca_amd import tracking
    metric = tracking.NearestNeighborDistanceMetric("cosine", threshold, budget, ctx=ctx)
    n, ns, E = trk.shape
    metric.partial_fit(trk.reshape(n * ns, E), np.repeat(100 + np.arange(n), ns), 100 + np.arange(n))
    return metric


@pytest.mark.gpu
def test_matching_on_the_device_cost_returns_the_reference_matches(ctx):
    from busca_amd import tracking
    g = gold()
    trk, det, lam, maxd, tracks, dets = gate_case()
    ti, di = [int(i) for i in g["gate_ti"]], [int(j) for j in g["gate_di"]]
    metric = _fitted_metric(ctx, trk, maxd)
    calls = []

    def nn_cost(tr, de, a, b):
        calls.append((len(a), len(b)))
        return metric.distance(det[list(b)], [tr[i].track_id for i in a], device=True)

    full = metric.distance(det, [t.track_id for t in tracks])
    err = np.abs(full - g["gate_cost"]).max()
    bar = 20.0 * g["restatement_err_emb"][g["emb_params"][:, 3] == 512].max()
    print("nearest-neighbour cost 96 x 40 x 512, 2 samples: max |d| %.3g, bar %.3g" % (err, bar))
    assert err <= bar
    matches, ut, ud = tracking.min_cost_matching(nn_cost, maxd, tracks, dets, ti, di, ctx=ctx)
    assert matches == [tuple(p) for p in g["mcm_matches"]] and sorted(ut) == sorted(g["mcm_ut"]) and sorted(ud) == sorted(g["mcm_ud"])
    for woc in (0, 1):
        matches, ut, ud = tracking.matching_cascade(nn_cost, maxd, 4, tracks, dets, ti, di, woC=bool(woc), ctx=ctx)
        assert matches == [tuple(p) for p in g["casc_%d_matches" % woc]]
        assert set(ut) == set(g["casc_%d_ut" % woc]) and len(ut) == len(g["casc_%d_ut" % woc])        # the reference builds this list from a set
        assert sorted(ud) == sorted(g["casc_%d_ud" % woc])
    assert len(calls) >= 1 + 4 + 1
    # defaults: all tracks, all detections
    m2, ut2, ud2 = tracking.matching_cascade(nn_cost, maxd, 4, tracks, dets, ctx=ctx)
    assert len(m2) + len(ut2) == 96 and len(m2) + len(ud2) == 40
    assert tracking.matching_cascade(nn_cost, maxd, 4, tracks, dets, [], di, ctx=ctx) == ([], [], di)


def _r_metric_fit(samples, budget, features, targets, active):
    """The published partial_fit, on features normalised as deep_sort/track.py:244 stores them (float64 norm, float32 storage)."""
    for f, t in zip(features, targets):
        f = f.astype(np.float64)
        samples.setdefault(int(t), []).append((f / np.sqrt((f * f).sum())).astype(np.float32))
        if budget is not None:
            samples[int(t)] = samples[int(t)][-budget:]
    return {k: samples[k] for k in active if k in samples}


@pytest.mark.gpu
@pytest.mark.parametrize("budget", [3, None])
def test_nearest_neighbor_distance_metric(ctx, budget):
    from busca_amd import synth, tracking
    E = 64
    metric = tracking.NearestNeighborDistanceMetric("cosine", 0.3, budget, ctx=ctx)
    assert metric.matching_threshold == 0.3 and metric.budget == budget
    # frame -> (targets that get a feature, active targets): 7 is dropped after frame 1 and re-added in frame 3; 5 gets two features in frame 2
    frames = [([1, 2, 7], [1, 2, 7]), ([1, 2, 7, 5], [1, 2, 7, 5]), ([1, 5, 5, 2], [1, 2, 5]), ([1, 7, 9], [1, 2, 5, 7, 9]), ([1, 1, 1, 1, 1, 9, 2], [1, 2, 7, 9])]
    samples, bar = {}, (4 * E + 8) * U
    for k, (targets, active) in enumerate(frames):
        feats = synth.normal(700 + k, "f", (len(targets), E)) * 3.0                    # not unit vectors: partial_fit normalises
        metric.partial_fit(feats, np.asarray(targets), active)
        samples = _r_metric_fit(samples, budget, feats, targets, active)
        stored = metric.samples
        assert sorted(stored) == sorted(samples)
        for t in samples:
            assert np.array_equal(stored[t], np.stack(samples[t])), (k, t)
        query = synth.normal(750 + k, "q", (11, E))
        asked = [1, 2, 5, 7, 9, 1]
        got = metric.distance(query, asked)
        assert got.shape == (6, 11)
        for i, t in enumerate(asked):
            if t in samples:
                ref = r_cosine(np.stack(samples[t]), query).min(0)
                assert np.abs(got[i] - ref).max() <= bar, (k, t)
            else:
                assert np.isposinf(got[i]).all(), (k, t)                              # no samples: never admissible
        dev = metric.distance(query, asked, device=True)
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)
    with pytest.raises(ValueError):
        tracking.NearestNeighborDistanceMetric("euclidean", 0.3, 3, ctx=ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("mc_lambda", [None, 0.98])
def test_appearance_round_equals_the_composition(ctx, mc_lambda):
    import torch
    from busca_amd import tracking
    g = gold()
    trk, det, lam, maxd, tracks, dets = gate_case()
    ti, di = [int(i) for i in g["gate_ti"]], [int(j) for j in g["gate_di"]]
    metric = _fitted_metric(ctx, trk, maxd, budget=3)

    def gated_metric(tr, de, a, b):                                                   # Tracker._match's closure, on the host-visible mirrors
        cost = metric.distance(np.stack([de[j].feature for j in b]), [tr[i].track_id for i in a])
        return tracking.gate_cost_matrix_mc(cost, tr, de, a, b, mc_lambda=mc_lambda, ctx=ctx)

    for depth in (None, 4):
        want = tracking.matching_cascade(gated_metric, metric.matching_threshold, depth or 1, tracks, dets, ti, di, woC=depth is None, ctx=ctx)
        got = tracking.appearance_round(metric, tracks, dets, ti, di, cascade_depth=depth, mc_lambda=mc_lambda, ctx=ctx)
        assert got[0] == want[0] and len(got[0]) >= 5
        assert set(got[1]) == set(want[1]) and len(got[1]) == len(want[1]) and sorted(got[2]) == sorted(want[2])
        dev_feats = torch.from_numpy(det.copy()).to(torch.device("cuda", 0))
        again = tracking.appearance_round(metric, tracks, dets, ti, di, cascade_depth=depth, mc_lambda=mc_lambda, ctx=ctx, det_features=dev_feats)
        assert again[0] == got[0] and sorted(again[2]) == sorted(got[2])
    m, ut, ud = tracking.appearance_round(metric, tracks, dets, ti, ctx=ctx)          # all detections
    assert len(m) + len(ud) == 40 and len(m) + len(ut) == len(ti)
    assert tracking.appearance_round(metric, tracks, dets, [], di, ctx=ctx) == ([], [], di)
    assert tracking.appearance_round(metric, tracks, dets, ti, [], ctx=ctx) == ([], ti, [])


@pytest.mark.gpu
def test_argument_errors(ctx):
    import torch
    from busca_amd import _lib
    dev = torch.device("cuda", 0)
    gal = torch.ones(4, 2, 32, dtype=torch.float32, device=dev)
    det = torch.ones(3, 32, dtype=torch.float32, device=dev)
    out = torch.full((4, 3), -7.0, dtype=torch.float64, device=dev)
    fn, s = ctx.lib.busca_appearance_cost, torch.cuda.current_stream(dev).cuda_stream

    def call(gallery=gal.data_ptr(), n=4, budget=2, dets=det.data_ptr(), m=3, E=32, reduce=0, flags=0, o=out.data_ptr()):
        return fn(ctx.h, gallery, None, None, n, budget, dets, m, E, reduce, flags, o, s)

    EINVAL = -1
    for kw in (dict(E=24), dict(E=8), dict(E=0), dict(E=2064), dict(E=4096), dict(n=-1), dict(m=-1), dict(budget=0), dict(budget=-3), dict(gallery=None),
               dict(dets=None), dict(o=None), dict(reduce=3), dict(reduce=-1), dict(flags=2), dict(gallery=gal.data_ptr() + 4)):
        assert call(**kw) == EINVAL, kw
        assert ctx.lib.busca_last_error(ctx.h).decode().startswith("busca_appearance_cost:"), kw
        with pytest.raises(_lib.BuscaError):
            ctx.check(call(**kw))
    assert call(n=0) == 0 and call(m=0) == 0 and call(n=0, gallery=None, o=None) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()                                          # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0.0).all()                                           # identical vectors, two identical rows per slot
    with pytest.raises(ValueError):
        from busca_amd import tracking
        tracking.appearance_cost(gal, det, reduce="median", ctx=ctx)
