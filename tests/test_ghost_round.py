"""GHOST association on the device: busca_ghost_distance / _proxies / _thresholds / _combine (include/busca_ghost.h) and their mirrors in
busca_amd.tracking (ghost_distance, ghost_proxies, ghost_thresholds, ghost_cost, ghost_round).

The reference is tests/golden/ghost.npz, written by tests/golden/make_golden_ghost.py from the reference's own functions (solve_dense replaced by
a scipy stand-in, see there); features are rebuilt from busca_amd.synth seeds.

Bars, none of them taken from a kernel's output:
  * against what already ships: exact.  MIN / MEAN / MAX are busca_appearance_cost's bits, MIDRANGE is (max + min) / 2 of its outputs, MEDIAN is
    np.median of the per-sample distances busca_appearance_cost gives when the gallery is viewed as [S * budget, 1, E].
  * against the fixture: the reference computes in float32, so every recorded output comes with `ref_err`, the largest difference between a float64
    numpy restatement and the reference's output for that case (1e-7 .. 2e-7); the bar is ref_err + 1e-12, the 1e-12 for float64 summation order
    (appearance.npz records < 1e-13 up to E = 2048).  NaN patterns are identical: the generator keeps no cost within 1e-6 of a threshold.
  * proxies: LAST, FIRST and MEDIAN copy a stored value: exact.  MEAN and MEANNORM round a float64 result once to float32: ref_err + one float32 ulp
    of the value.
  * matches: exact; the generator keeps a round only if its optimum is unique by more than 1e-9 in both sep modes."""
import os
import re
import types
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ghost.npz")
COUNTS = [0, 1, 2, 15, 16, 17, 32, 33, 255, 256]
BUDGET = 256
ALPHA = 0.4
# the rounds of make_golden_ghost.ROUNDS: route, tracker_cfg pieces, motion model
ROUND_CFG = [
    dict(avg_act={"do": True, "num": 5, "proxy": "each_sample"}, avg_inact={"do": True, "num": 5, "proxy": "each_sample"}, act_reid_thresh=1.005,
         inact_reid_thresh=1.0, motion_config={"apply_motion_model": True, "combi": "sum_0.4"}),
    dict(avg_act={"do": False, "num": 4, "proxy": "each_sample"}, avg_inact={"do": True, "num": 4, "proxy": "each_sample"}, act_reid_thresh="every",
         inact_reid_thresh="every", motion_config={"apply_motion_model": False, "combi": "sum_0.4"}),
    dict(avg_act={"do": True, "num": 3, "proxy": "mean"}, avg_inact={"do": True, "num": "all", "proxy": "median"}, act_reid_thresh="tbd",
         inact_reid_thresh="tbd", motion_config={"apply_motion_model": False, "combi": "sum_0.4"}),
]

_CACHE = {}


def gold():
    if "g" not in _CACHE:
        with np.load(GOLD) as f:
            _CACHE["g"] = {k: f[k] for k in f.files}
    return _CACHE["g"]


def feats(seed, n, m, E, budget):
    key = ("f", seed, n, m, E, budget)
    if key not in _CACHE:
        from busca_amd import synth
        trk, det = synth.appearance_features(int(seed), int(n), int(m), int(E), int(budget), twins=True)
        trk.setflags(write=False)
        det.setflags(write=False)
        _CACHE[key] = (trk, det)
    return _CACHE[key]


def r_cosine(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return 1.0 - (a @ b.T) / (np.sqrt((a * a).sum(1))[:, None] * np.sqrt((b * b).sum(1))[None, :])


def chrono(ring, count, newest):
    budget = ring.shape[0]
    return ring[[(int(newest) - (int(count) - 1) + k) % budget for k in range(int(count))]]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def close(got, ref, bar):
    """Identical NaN pattern and |got - ref| <= bar elsewhere -> the largest difference (None when the patterns differ)."""
    if got.shape != ref.shape or not np.array_equal(np.isnan(got), np.isnan(ref)):
        return None
    fin = ~np.isnan(ref)
    return float(np.abs(got[fin] - ref[fin].astype(np.float64)).max()) if fin.any() else 0.0


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_symbols_declared_typed_and_exported():
    from busca_amd.build import build
    build()
    from busca_amd import _lib

    def declared(header):
        hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return set(re.findall(r"\b(busca_[a-z0-9_]+)\s*\(", hdr))
    names = {"busca_ghost_distance", "busca_ghost_proxies", "busca_ghost_thresholds", "busca_ghost_combine"}
    assert declared("busca_ghost.h") == names == set(_lib.GHOST_SIGNATURES)
    for header, table in _lib.HEADERS.items():
        if header == "busca_ghost.h":
            continue
        assert not names & declared(header) and not names & set(table)
    lib = _lib.load()
    for name, nargs in (("busca_ghost_distance", 12), ("busca_ghost_proxies", 12), ("busca_ghost_thresholds", 9), ("busca_ghost_combine", 12)):
        fn = getattr(lib, name)                                            # exported
        assert fn.restype is not None and len(fn.argtypes) == nargs == len(_lib.GHOST_SIGNATURES[name][1])
    assert lib.busca_version() >= 2003 and lib.busca_version() // 1000 == 2
    hdr = open(os.path.join(ROOT, "include", "busca_ghost.h")).read()
    for name, val in (("BUSCA_GHOST_MIN", _lib.GHOST_MIN), ("BUSCA_GHOST_MEAN", _lib.GHOST_MEAN), ("BUSCA_GHOST_MAX", _lib.GHOST_MAX),
                      ("BUSCA_GHOST_MIDRANGE", _lib.GHOST_MIDRANGE), ("BUSCA_GHOST_MEDIAN", _lib.GHOST_MEDIAN),
                      ("BUSCA_GHOST_MEDIAN_BUDGET_MAX", _lib.GHOST_MEDIAN_BUDGET_MAX), ("BUSCA_GHOST_PROXY_LAST", _lib.GHOST_PROXY_LAST),
                      ("BUSCA_GHOST_PROXY_FIRST", _lib.GHOST_PROXY_FIRST), ("BUSCA_GHOST_PROXY_MEAN", _lib.GHOST_PROXY_MEAN),
                      ("BUSCA_GHOST_PROXY_MEANNORM", _lib.GHOST_PROXY_MEANNORM), ("BUSCA_GHOST_PROXY_MEDIAN", _lib.GHOST_PROXY_MEDIAN)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name
    assert (_lib.GHOST_MIN, _lib.GHOST_MEAN, _lib.GHOST_MAX, _lib.GHOST_MIDRANGE, _lib.GHOST_MEDIAN, _lib.GHOST_MEDIAN_BUDGET_MAX) == (0, 1, 2, 3, 4, 256)


def test_mirrors_reachable_from_the_alias_package():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "busca_amd", "compat"))
    try:
        import busca.tracking as bt
    finally:
        sys.path.pop(0)
    for name in ("ghost_distance", "ghost_proxies", "ghost_thresholds", "ghost_cost", "ghost_round", "ghost_check_config"):
        assert callable(getattr(bt, name)), name


def test_fixture_contents():
    g = gold()
    assert g["dist_params"].shape == (3, 5) and g["pd_err"].shape == (3, 5) and g["lf_err"].shape == (3,)
    for k, (seed, n, m, E, budget) in enumerate(g["dist_params"]):
        count = g["dist_count_%d" % k]
        assert count.shape == (n,) and count.min() >= 1 and count.max() == budget
        mask = g["dist_tlabel_%d" % k][:, None] != g["dist_dlabel_%d" % k][None, :]
        assert 0.2 <= mask.mean() <= 0.8
        for num in range(1, 6):
            ref = g["pd_%d_%d" % (k, num)]
            assert ref.shape == (n, m) and ref.dtype == np.float32 and np.array_equal(np.isnan(ref), mask)
        assert g["lf_%d" % k].shape == (n, m) and np.array_equal(np.isnan(g["lf_%d" % k]), mask)
    assert (g["pd_err"] > 0).all() and g["pd_err"].max() < 1e-6 and g["lf_err"].max() < 1e-6        # float32 noise, no more
    # the seeds rebuild the recorded case: np.median of the float64 restatement sits within the recorded ref_err
    seed, n, m, E, budget = g["dist_params"][0]
    trk, det = feats(seed, n, m, E, budget)
    rest = np.stack([np.median(r_cosine(trk[i, :g["dist_count_0"][i]], det), 0) for i in range(n)])
    fin = ~np.isnan(g["pd_0_5"])
    assert np.abs(rest[fin] - g["pd_0_5"][fin]).max() <= g["pd_err"][0, 4]
    n, E = int(g["px_params"][1]), int(g["px_params"][3])
    for key in ("px_last_3", "px_mean_3", "px_mean_40", "px_median_3", "px_median_40", "px_meannorm_40"):
        assert g[key].shape == (n, E) and g[key].dtype == np.float32 and float(g[key.replace("px_", "px_err_")]) < 1e-6
    assert float(g["px_err_last_3"]) == 0.0 and float(g["px_err_median_3"]) == 0.0 and float(g["px_err_median_40"]) == 0.0
    full = g["px_count"] == g["px_params"][4]
    assert (full & (g["px_newest"] != g["px_params"][4] - 1)).any() and (g["px_count"] < 3).any() and (g["px_count"] > 3).any()     # a wrapped ring; avg above and below
    assert g["thr_every"].shape == g["thr_tbd"].shape == (2,) and float(g["thr_err_every"]) < 1e-6 and float(g["thr_err_tbd"]) < 1e-6
    assert g["rd_params"].shape == (len(ROUND_CFG), 8) and float(g["alpha"][0]) == ALPHA
    for q, (seed, n, m, E, budget, na, route, tried) in enumerate(g["rd_params"]):
        ref, thr = g["rd_dist_%d" % q], g["rd_thr_%d" % q]
        assert ref.shape == (m, n) and 0 < na < n
        assert 0.2 <= np.isfinite(ref).mean() <= 0.8 and 0.2 <= np.isnan(ref).mean() <= 0.8       # every thresholded case: >= 20 % finite, >= 20 % NaN
        pre = g["rd_blend_%d" % q] if ("rd_blend_%d" % q) in g else g["rd_masked_%d" % q]
        with np.errstate(invalid="ignore"):
            edge = min(np.nanmin(np.abs(pre[:, :na] - thr[0])), np.nanmin(np.abs(pre[:, na:] - thr[1])))
        assert edge > 1e-6                                                                        # no cost within 1e-6 of its threshold
        assert np.array_equal(np.isnan(ref[:, :na]), ~(pre[:, :na] <= thr[0])) and np.array_equal(np.isnan(ref[:, na:]), ~(pre[:, na:] <= thr[1]))
        for sep in (0, 1):
            row, col = g["rd_row_%d_%d" % (q, sep)], g["rd_col_%d_%d" % (q, sep)]
            assert len(row) == len(col) >= 5 and len(set(row)) == len(row) and len(set(col)) == len(col) and np.isfinite(ref[row, col]).all()
            assert (np.diff(row) > 0).all() and (sep == 0 or col.max() < na)
        assert float(g["rd_err"][q]) < 1e-6 and float(g["rd_thr_err"][q]) < 1e-6
    assert g["dropped"].shape == (2,) and 10 * int(g["dropped"].sum()) <= int(g["candidates"][0])
    assert os.path.getsize(GOLD) < 1 << 20


def test_refused_configs_raise_with_the_reason():
    from busca_amd import tracking
    state = dict(gallery=np.zeros((2, 1, 16), np.float32), num_active=1)
    det = np.zeros((3, 16), np.float32)
    with pytest.raises(ValueError, match=r"pairwise_distance.*base_tracker\.py:101"):
        tracking.ghost_round(state, det, cfg={"distance": "euclidean"})
    with pytest.raises(ValueError, match=r"use_bism.*crashes.*base_tracker\.py:105-106"):
        tracking.ghost_round(state, det, cfg={"use_bism": True})
    with pytest.raises(ValueError):
        tracking.ghost_check_config({"distance": "cosine", "use_bism": True})
    assert tracking.ghost_check_config({"distance": "cosine", "use_bism": False}) == {"distance": "cosine", "use_bism": False}
    with pytest.raises(ValueError, match="reduce"):
        tracking.ghost_distance(np.zeros((2, 16), np.float32), det, reduce="mode")
    with pytest.raises(ValueError, match="reduce"):
        tracking.ghost_distance(np.zeros((2, 16), np.float32), det, reduce=6)
    with pytest.raises(NotImplementedError, match="mv_avg"):
        tracking.ghost_proxies(np.zeros((2, 1, 16), np.float32), mode="mv_avg")
    with pytest.raises(ValueError, match="mode"):
        tracking.ghost_proxies(np.zeros((2, 1, 16), np.float32), mode="newest")


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from busca_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def edge_gallery(E):
    """12 slots of budget 256: slot s < 10 holds COUNTS[s] samples, slot 10 five with rows 1 and 3 (and 0 and 4) identical, slot 11 six with a zero-norm row.
    -> (clean, poisoned with NaN beyond the counts, detections [65,E], count)."""
    key = ("edge", E)
    if key not in _CACHE:
        from busca_amd import synth
        trk, det = synth.appearance_features(800 + E, 12, 65, E, BUDGET)
        trk = trk.copy()
        count = np.array(COUNTS + [5, 6], dtype=np.int32)
        trk[10, 3], trk[10, 4] = trk[10, 1], trk[10, 0]
        trk[11, 2] = 0.0
        poisoned = trk.copy()
        for s in range(12):
            poisoned[s, count[s]:] = np.nan
        poisoned.setflags(write=False)
        det.setflags(write=False)
        _CACHE[key] = (poisoned, det, count)
    return _CACHE[key]


SLOTS = {17: np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, -1, 9, 3, 10, 7], dtype=np.int32)}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("E", [16, 512])
def test_edge_shapes_bit_exact_against_appearance_cost(ctx, E, n):
    import torch
    from busca_amd import tracking
    gal, det, count = edge_gallery(E)
    dev = torch.device("cuda", 0)
    gdev, cdev = torch.from_numpy(gal.copy()).to(dev), torch.from_numpy(count).to(dev)
    slot_sets = [SLOTS[17]] if n == 17 else [np.array([s], dtype=np.int32) for s in (9, 10, 11, -1, 0, 5)]
    for m in (1, 63, 64, 65):
        d = torch.from_numpy(det[:m].copy()).to(dev)
        # every stored sample's own distance, from the entry point that already ships: the gallery as S * budget one-sample tracks
        per = tracking.appearance_cost(gdev.view(-1, 1, E), d, "min", ctx=ctx).cpu().numpy().reshape(12, BUDGET, m)
        for slot in slot_sets:
            assert len(slot) == n
            base = {r: tracking.appearance_cost(gdev, d, r, slot=slot, count=cdev, ctx=ctx).cpu().numpy() for r in ("min", "mean", "max")}
            got = {r: tracking.ghost_distance(gdev, d, r, slot=slot, count=cdev, ctx=ctx).cpu().numpy() for r in ("min", "mean", "max", "midrange", "median")}
            for r in ("min", "mean", "max"):
                assert same(got[r], base[r]), (m, r)
            assert same(got["midrange"], (base["max"] + base["min"]) / 2), m
            want = np.full((n, m), np.inf)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)                      # np.median warns about the NaN it propagates
                for i, s in enumerate(slot):
                    if s >= 0 and count[s] > 0:
                        want[i] = np.median(per[s, :count[s]], axis=0)
            assert same(got["median"], want), (m, slot)
            again = tracking.ghost_distance(gdev, d, "median", slot=slot, count=cdev, ctx=ctx).cpu().numpy()
            assert same(again, got["median"])                                        # run to run
            for r in got:                                                            # NaN only where a zero-norm sample is among the valid rows: the poison is never read
                assert np.array_equal(np.isnan(got[r]), np.repeat((slot == 11)[:, None], m, 1)), (m, r)
                assert np.array_equal(np.isposinf(got[r]), np.repeat(((slot < 0) | (slot == 0))[:, None], m, 1)), (m, r)
            assert same(tracking.ghost_distance(gdev, d, 5, slot=slot, count=cdev, ctx=ctx).cpu().numpy(), got["median"])      # GHOST's num spelling
    if n == 17:
        dup = tracking.ghost_distance(gdev, torch.from_numpy(det.copy()).to(dev), "median", slot=np.array([10], dtype=np.int32), count=cdev, ctx=ctx).cpu().numpy()
        assert np.isfinite(dup).all()                                                # two pairs of identical samples: ranks still a permutation


@pytest.mark.gpu
def test_median_is_independent_of_n_and_row_order(ctx):
    from busca_amd import tracking
    gal, det, count = edge_gallery(512)
    full = tracking.ghost_distance(gal, det, "median", count=count, ctx=ctx).cpu().numpy()
    assert full.shape == (12, 65)
    perm = np.array([7, 3, 11, 0, 9, 10, 1, 8, 2, 6, 5, 4], dtype=np.int32)
    assert same(tracking.ghost_distance(gal, det, "median", slot=perm, count=count, ctx=ctx).cpu().numpy(), full[perm])
    sub = np.array([8, 8, 2], dtype=np.int32)
    assert same(tracking.ghost_distance(gal, det, "median", slot=sub, count=count, ctx=ctx).cpu().numpy(), full[sub])
    # the same samples in another gallery, at other slots
    assert same(tracking.ghost_distance(gal[perm], det, "median", count=count[perm], ctx=ctx).cpu().numpy(), full[perm])
    for r in ("midrange", "mean"):
        a = tracking.ghost_distance(gal, det, r, count=count, ctx=ctx).cpu().numpy()
        assert same(tracking.ghost_distance(gal, det, r, slot=perm, count=count, ctx=ctx).cpu().numpy(), a[perm])


@pytest.mark.gpu
def test_proxy_dist_and_last_frame_against_the_reference(ctx):
    from busca_amd import tracking
    g = gold()
    for k, (seed, n, m, E, budget) in enumerate(g["dist_params"]):
        trk, det = feats(seed, n, m, E, budget)
        count, tl, dl = g["dist_count_%d" % k], g["dist_tlabel_%d" % k], g["dist_dlabel_%d" % k]
        poisoned = trk.copy()
        for i in range(n):
            poisoned[i, count[i]:] = np.nan
        for num in range(1, 6):
            app = tracking.ghost_distance(poisoned, det, num, count=count, ctx=ctx)
            got = tracking.ghost_cost(app, track_labels=tl, det_labels=dl, ctx=ctx).cpu().numpy()
            bar = g["pd_err"][k, num - 1] + 1e-12
            err = close(got, g["pd_%d_%d" % (k, num)], bar)
            print("proxy_dist case %d num %d: max |d| %s, bar %.3g" % (k, num, err, bar))
            assert err is not None and err <= bar
        last = tracking.ghost_proxies(poisoned, "last", count=count, ctx=ctx)
        assert np.array_equal(last.cpu().numpy(), np.stack([trk[i, count[i] - 1] for i in range(n)]))
        got = tracking.ghost_cost(tracking.ghost_distance(last, det, "min", ctx=ctx), track_labels=tl, det_labels=dl, ctx=ctx).cpu().numpy()
        bar = g["lf_err"][k] + 1e-12
        err = close(got, g["lf_%d" % k], bar)
        print("last_frame case %d: max |d| %s, bar %.3g" % (k, err, bar))
        assert err is not None and err <= bar


@pytest.mark.gpu
def test_thresholds_against_the_reference_and_numpy(ctx):
    import torch
    from busca_amd import tracking
    g = gold()
    seed, n, m, E, budget = g["dist_params"][0]
    trk, det = feats(seed, n, m, E, budget)
    na = int(g["thr_na"][0])
    app = tracking.ghost_distance(trk, det, "mean", count=g["dist_count_0"], ctx=ctx)
    host = app.cpu().numpy()
    for kind, ks in (("every", (0.0, 2.0)), ("tbd", (0.5, 1.0))):
        got = tracking.ghost_thresholds(app, na, ks[0], ks[1], ctx=ctx).cpu().numpy()
        bar = float(g["thr_err_" + kind]) + 1e-12
        print("update_thresholds %s: %s, max |d| %.3g, bar %.3g" % (kind, got, np.abs(got - g["thr_" + kind]).max(), bar))
        assert np.abs(got - g["thr_" + kind]).max() <= bar
        want = np.array([host[:na].mean() - ks[0] * host[:na].std(), host[na:].mean() - ks[1] * host[na:].std()])
        assert np.abs(got - want).max() <= 1e-12                                        # the same float64 data, another summation order
        assert np.array_equal(tracking.ghost_thresholds(app, na, ks[0], ks[1], ctx=ctx).cpu().numpy(), got)      # run to run
    # a group without rows keeps its entry; NaN propagates as in numpy; sizes that are no multiple of the workgroup
    keep = torch.tensor([0.25, 0.75], dtype=torch.float64, device=app.device)
    got = tracking.ghost_thresholds(app, n, 0.5, 1.0, out=keep, ctx=ctx).cpu().numpy()
    assert got[1] == 0.75 and abs(got[0] - (host.mean() - 0.5 * host.std())) <= 1e-12
    keep[0] = 0.25
    got = tracking.ghost_thresholds(app, 0, 0.5, 1.0, out=keep, ctx=ctx).cpu().numpy()
    assert got[0] == 0.25 and abs(got[1] - (host.mean() - 1.0 * host.std())) <= 1e-12
    holed = host.copy()
    holed[na + 1, 3] = np.nan
    got = tracking.ghost_thresholds(holed, na, 0.0, 2.0, ctx=ctx).cpu().numpy()
    assert np.isnan(got[1]) and abs(got[0] - host[:na].mean()) <= 1e-12
    one = tracking.ghost_thresholds(host[:1, :1].copy(), 1, 0.5, 1.0, ctx=ctx).cpu().numpy()
    assert one[0] == host[0, 0] and np.isposinf(one[1])


@pytest.mark.gpu
def test_proxies_against_the_reference_and_numpy(ctx):
    from busca_amd import tracking
    g = gold()
    seed, n, m, E, budget = g["px_params"]
    trk, _ = feats(seed, n, m, E, budget)
    count, newest = g["px_count"], g["px_newest"]
    poisoned = trk.copy()
    for i in range(n):
        poisoned[i, count[i]:] = np.nan
    for mode, avg in (("last", 3), ("median", 3), ("median", 40)):
        got = tracking.ghost_proxies(poisoned, mode, avg, count=count, newest=newest, ctx=ctx).cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got, g["px_%s_%d" % (mode, avg)]), (mode, avg)
    for mode, avg in (("mean", 3), ("mean", 40), ("meannorm", 40)):
        ref = g["px_%s_%d" % (mode, avg)]
        got = tracking.ghost_proxies(poisoned, mode, avg, count=count, newest=newest, ctx=ctx).cpu().numpy()
        bar = float(g["px_err_%s_%d" % (mode, avg)]) + np.spacing(np.abs(ref)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - ref)
        print("get_proxy %s avg %d: max |d| %.3g" % (mode, avg, err.max()))
        assert (err <= bar).all(), (mode, avg)
    assert np.array_equal(tracking.ghost_proxies(poisoned, "mean", "all", count=count, newest=newest, ctx=ctx).cpu().numpy(),
                          tracking.ghost_proxies(poisoned, "mean", 40, count=count, newest=newest, ctx=ctx).cpu().numpy())
    # FIRST has no reference output (its branch cannot be reached there): the oldest stored sample.  MEANNORM below the gallery length: numpy
    rows = [chrono(trk[i], count[i], newest[i]) for i in range(n)]
    assert np.array_equal(tracking.ghost_proxies(poisoned, "first", count=count, newest=newest, ctx=ctx).cpu().numpy(), np.stack([r[0] for r in rows]))
    got = tracking.ghost_proxies(poisoned, "meannorm", 3, count=count, newest=newest, ctx=ctx).cpu().numpy()
    mu = np.stack([r[-3:].astype(np.float64).mean(0).astype(np.float32).astype(np.float64) for r in rows])
    want = mu / np.sqrt((mu * mu).sum(1, keepdims=True))
    assert (np.abs(got - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    # slot: rows in another order, a track without samples -> NaN; newest = None is count - 1
    slot = np.array([3, -1, 0, 3], dtype=np.int32)
    got = tracking.ghost_proxies(poisoned, "median", 3, slot=slot, count=count, newest=newest, ctx=ctx).cpu().numpy()
    assert np.array_equal(got[[0, 2, 3]], g["px_median_3"][[3, 0, 3]]) and np.isnan(got[1]).all()
    short = count < budget
    got = tracking.ghost_proxies(poisoned, "last", count=count, ctx=ctx).cpu().numpy()
    assert np.array_equal(got[short], g["px_last_3"][short])
    # E that is no multiple of the workgroup, more rows than a wave: a second block of features, against numpy
    from busca_amd import synth
    big = synth.normal(77, "px", (3, 5, 300))
    got = tracking.ghost_proxies(big, "median", 4, ctx=ctx).cpu().numpy()
    assert np.array_equal(got, np.sort(big[:, 1:], 1)[:, 1])
    big = big.copy()
    big[1, 2, 299] = np.nan
    got = tracking.ghost_proxies(big, "median", 0, ctx=ctx).cpu().numpy()
    assert np.isnan(got[1, 299]) and np.isnan(got).sum() == 1                        # torch.median's NaN


def round_state(q):
    g = gold()
    seed, n, m, E, budget, na, route, _ = [int(v) for v in g["rd_params"][q]]
    trk, det = feats(seed, n, m, E, budget)
    poisoned = trk.copy()
    count = g["rd_count_%d" % q]
    for i in range(n):
        poisoned[i, count[i]:] = np.nan
    state = types.SimpleNamespace(gallery=poisoned, count=count, newest=g["rd_newest_%d" % q], slot=None, num_active=na)
    return state, det, (g["rd_tlabel_%d" % q], g["rd_dlabel_%d" % q]), seed, n, m, na


@pytest.mark.gpu
@pytest.mark.parametrize("q", range(len(ROUND_CFG)))
def test_ghost_round_against_the_reference(ctx, q):
    import torch
    from busca_amd import synth, tracking
    g = gold()
    state, det, labels, seed, n, m, na = round_state(q)
    cfg = dict(ROUND_CFG[q], nan_first=True, distance="cosine", use_bism=False)
    motion = synth.tracker_costs(seed, n, m) if cfg["motion_config"]["apply_motion_model"] else None
    bar = float(g["rd_err"][q]) + 1e-12
    for sep in (0, 1):
        thr = torch.zeros(2, dtype=torch.float64, device=torch.device("cuda", 0))
        dist, row, col = tracking.ghost_round(state, det, labels, motion, dict(cfg, assign_separately=bool(sep)), thresholds=thr, ctx=ctx)
        if sep:
            assert isinstance(dist, list) and tuple(dist[0].shape) == (m, na) and tuple(dist[1].shape) == (m, n - na)
            dist = torch.cat(dist, 1)
        dist = dist.cpu().numpy()
        err = close(dist, g["rd_dist_%d" % q], bar)
        terr = np.abs(thr.cpu().numpy() - g["rd_thr_%d" % q]).max()
        print("round %d sep %d: max |d| %s (bar %.3g), thresholds max |d| %.3g (bar %.3g), %d matches" % (q, sep, err, bar, terr, float(g["rd_thr_err"][q]) + 1e-12, len(row)))
        assert err is not None and err <= bar                                        # the identical NaN pattern after masks and thresholds
        assert terr <= float(g["rd_thr_err"][q]) + 1e-12
        assert np.array_equal(row, g["rd_row_%d_%d" % (q, sep)]) and np.array_equal(col, g["rd_col_%d_%d" % (q, sep)])
        # `sep` as an argument, features already on the device, slot spelled out: the same answer
        dstate = types.SimpleNamespace(gallery=torch.from_numpy(state.gallery.copy()).to(thr.device), count=state.count, newest=state.newest,
                                       slot=np.arange(n, dtype=np.int32), num_active=na)
        _, row2, col2 = tracking.ghost_round(dstate, torch.from_numpy(det.copy()).to(thr.device), labels, motion, cfg, sep=bool(sep), ctx=ctx)
        assert np.array_equal(row2, row) and np.array_equal(col2, col)
    # the stages on their own: the stacked, class-masked matrix and the blend
    masked = g["rd_masked_%d" % q]
    if int(g["rd_params"][q][6]) == 0:
        num = cfg["avg_inact"]["num"]
        app = torch.empty(n, m, dtype=torch.float64, device=thr.device)
        if cfg["avg_act"]["do"]:
            tracking.ghost_distance(state.gallery, det, num, slot=np.arange(na, dtype=np.int32), count=state.count, out=app[:na], ctx=ctx)
        else:
            last = tracking.ghost_proxies(state.gallery, "last", slot=np.arange(na, dtype=np.int32), count=state.count, newest=state.newest, ctx=ctx)
            tracking.ghost_distance(last, det, "min", out=app[:na], ctx=ctx)
        tracking.ghost_distance(state.gallery, det, num, slot=np.arange(na, n, dtype=np.int32), count=state.count, out=app[na:], ctx=ctx)
        got = tracking.ghost_cost(app, track_labels=labels[0], det_labels=labels[1], ctx=ctx)
        err = close(got.cpu().numpy().T, masked, float(g["rd_masked_err_%d" % q]) + 1e-12)
        assert err is not None and err <= float(g["rd_masked_err_%d" % q]) + 1e-12
        if motion is not None:
            blend = tracking.ghost_cost(app, motion, ALPHA, labels[0], labels[1], ctx=ctx).cpu().numpy()
            err = close(blend.T, g["rd_blend_%d" % q], float(g["rd_blend_err_%d" % q]) + 1e-12)
            assert err is not None and err <= float(g["rd_blend_err_%d" % q]) + 1e-12
            a = got.cpu().numpy()
            assert same(blend, (1 - ALPHA) * a + ALPHA * motion)                     # two products and a sum, no contraction
    assert tracking.ghost_round(state, det[:0], labels, motion, cfg, ctx=ctx)[1].shape == (0,)


@pytest.mark.gpu
def test_error_codes(ctx):
    import torch
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    lib, EINVAL = ctx.lib, -1
    gal = torch.ones(4, 2, 32, dtype=torch.float32, device=dev)
    det = torch.ones(3, 32, dtype=torch.float32, device=dev)
    out = torch.full((4, 3), -7.0, dtype=torch.float64, device=dev)
    big = torch.ones(1, 257, 16, dtype=torch.float32, device=dev)

    def check(name, rc, kw):
        assert rc == EINVAL, (name, kw)
        assert lib.busca_last_error(ctx.h).decode().startswith(name + ":"), (name, kw, lib.busca_last_error(ctx.h))

    def dist(gallery=gal.data_ptr(), n=4, budget=2, dets=det.data_ptr(), m=3, E=32, reduce=0, o=out.data_ptr()):
        return lib.busca_ghost_distance(ctx.h, gallery, None, None, n, budget, dets, m, E, reduce, o, s)
    for kw in (dict(E=24), dict(E=8), dict(E=2064), dict(n=-1), dict(m=-1), dict(budget=0), dict(gallery=None), dict(dets=None), dict(o=None), dict(reduce=5),
               dict(reduce=-1), dict(gallery=gal.data_ptr() + 4), dict(dets=det.data_ptr() + 8), dict(o=out.data_ptr() + 4),
               dict(gallery=big.data_ptr(), n=1, budget=257, E=16, reduce=4)):
        check("busca_ghost_distance", dist(**kw), kw)
    assert dist(gallery=big.data_ptr(), n=1, budget=257, E=16, dets=det.data_ptr(), reduce=3) == 0          # only MEDIAN has a budget limit
    assert dist(gallery=big.data_ptr(), n=1, budget=256, E=16, dets=det.data_ptr(), reduce=4) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[0] == 0.0).all()
    out.fill_(-7.0)
    assert dist(n=0) == 0 and dist(m=0) == 0 and dist(n=0, gallery=None, o=None) == 0

    pout = torch.full((4, 32), -7.0, dtype=torch.float32, device=dev)

    def prox(gallery=gal.data_ptr(), n=4, budget=2, E=32, mode=0, window=0, o=pout.data_ptr()):
        return lib.busca_ghost_proxies(ctx.h, gallery, None, None, None, n, budget, E, mode, window, o, s)
    for kw in (dict(n=-1), dict(budget=0), dict(E=0), dict(E=-16), dict(mode=5), dict(mode=-1), dict(gallery=None), dict(o=None), dict(gallery=gal.data_ptr() + 2)):
        check("busca_ghost_proxies", prox(**kw), kw)
    assert prox(n=0) == 0 and prox(n=0, gallery=None, o=None) == 0

    thr = torch.full((2,), -7.0, dtype=torch.float64, device=dev)

    def thresh(cost=out.data_ptr(), n=4, m=3, na=2, o=thr.data_ptr()):
        return lib.busca_ghost_thresholds(ctx.h, cost, n, m, na, 0.5, 1.0, o, s)
    for kw in (dict(n=-1), dict(m=-1), dict(na=-1), dict(na=5), dict(cost=None), dict(o=None), dict(cost=out.data_ptr() + 4), dict(o=thr.data_ptr() + 4)):
        check("busca_ghost_thresholds", thresh(**kw), kw)
    assert thresh(n=0, na=0) == 0 and thresh(m=0) == 0

    lab = torch.zeros(4, dtype=torch.int32, device=dev)
    cout = torch.full((4, 3), -7.0, dtype=torch.float64, device=dev)

    def comb(app=out.data_ptr(), motion=None, n=4, m=3, alpha=0.4, tl=None, dl=None, na=2, t=None, o=cout.data_ptr()):
        return lib.busca_ghost_combine(ctx.h, app, motion, n, m, alpha, tl, dl, na, t, o, s)
    for kw in (dict(n=-1), dict(m=-1), dict(alpha=float("nan")), dict(tl=lab.data_ptr()), dict(dl=lab.data_ptr()), dict(app=None), dict(o=None),
               dict(app=out.data_ptr() + 4), dict(motion=out.data_ptr() + 4), dict(t=thr.data_ptr() + 4), dict(o=cout.data_ptr() + 4),
               dict(tl=lab.data_ptr() + 2, dl=lab.data_ptr())):
        check("busca_ghost_combine", comb(**kw), kw)
    assert comb(n=0) == 0 and comb(m=0) == 0
    torch.cuda.synchronize()
    for t in (out, pout, thr, cout):
        assert (t.cpu().numpy() == -7.0).all()                                        # nothing was launched
    assert comb() == 0 and dist() == 0
    torch.cuda.synchronize()
    assert (cout.cpu().numpy() == -7.0).all() and (out.cpu().numpy() == 0.0).all()    # combine copied the matrix as it was when it ran
    from busca_amd import _lib
    with pytest.raises(_lib.BuscaError):
        ctx.check(dist(reduce=9))
