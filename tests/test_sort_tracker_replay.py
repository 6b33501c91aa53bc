"""The reference's StrongSORT tracker, replayed through SortStore.frame.

The reference is tests/golden/sort_tracker.npz: adapters/StrongSORT/deep_sort/tracker.py, track.py, linear_assignment.py and detection.py
themselves, driven by tests/golden/make_golden_sort_tracker.py as deep_sort_app.py:186-190 drives them (camera_update where the frame has a matrix,
then predict, then update) over three scripted scenes - small, the same detections with opt.woC and without the MC blend, crowded - with the clamped
matrix, the index lists, the limit and the pairs of every min_cost_matching call, the gating distances, Tracker._match's three lists and every
track's state recorded frame by frame.  tests/sort_replay.py is the adapter loop INTEGRATION.md prints for SortStore.frame, made executable; here it
drives the recorded detections through a numpy backend (CPU), through SortStore.frame, through the composed calls and through
SortStore.frame_batch (GPU).  Everything discrete - ids, states, hits, ages, time_since_update, the order of Tracker.tracks, deletions, the
matches in _match's order, the unmatched lists, new tracks and their slots, output ids - is compared exactly.

Bars.  predict, update and the gate go through BLAS and LAPACK in the reference, so states and everything computed from them are compared within 20 x
the distance of the numpy restatement from the reference, recorded in the fixture as restatement_err_* (the convention of
tests/test_byte_tracker_replay.bars: room for a third valid evaluation order, none for a wrong formula); KalmanFilter.initiate is exact.  The device
keeps feature rows in float32 and forms the appearance cost from them, so feature rows and plane 0 of the cost slab use the recordings of the numpy
backend's float32 mode (_feat32, _cost32).  The bars come from the fixture and never from a kernel's output.  Two recorded errors are zero - the IoU
matrices and the float64 feature rows, where the restatement performs the reference's own numpy operations - so every bar is floored at the
rounding bound of its quantity (u = 2^-53, or 2^-24 for the float32 quantities):
  mean, cov   a state entry that no update has touched is a sum of at most F products of entries of the recorded initiation by powers of the motion
              matrix: (F + 1) u relative after F predictions
  iou         1 - (iw * ih) / ((a + b) - iw * ih): 4 differences (8 roundings), 3 products, 2 sums, 1 quotient and the final difference, at most
              16 u in absolute value as every intermediate ratio is at most 1
  gate        four squares of a 4 x 4 triangular solve (10 products, 6 differences, 4 quotients) on 4 differences, over a Cholesky factor of as
              many operations again, summed: at most 64 u relative
  feat        x / ||x||: E squares and E - 1 sums, a root, a quotient, and the EMA's two products, sum and second normalisation: (E + 8) u in
              absolute value, every entry being at most 1
  cost        a dot product and two norms of E terms each, two roots, a product, a quotient, a difference: (2 E + 8) u in absolute value
The generator asserts that every decision of every frame has a margin - unique optima, costs off their limits, gating distances off chi2inv95[4] -
of 1e-6 (IoU plane, gate), which exceeds 1000 x every float64 bar, and of 1.2e-2 on the appearance plane, which exceeds the float32 bar by the factor
the fixture records as appearance_margin_factor (1000): a device result within its bars cannot change a decision, so exact comparison of the
decisions is meaningful.

Measured on one MI355X (printed by the GPU tests): see DESIGN.md, K-SFRAME."""
import importlib.util
import os

import numpy as np
import pytest

from tests import sort_replay as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATOR = os.path.join(ROOT, "tests", "golden", "make_golden_sort_tracker.py")
_CACHE = {}


def _generator():
    if "gen" not in _CACHE:
        spec = importlib.util.spec_from_file_location("make_golden_sort_tracker", GENERATOR)
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)
        _CACHE["gen"] = gen
    return _CACHE["gen"]


REFERENCE = _generator().REF                               # where the generator looks for the reference tree
KEYS = ("mean", "cov", "iou", "gate", "feat", "cost", "feat32", "cost32")


def bars(name):
    """-> the bars of a scene by quantity: 20 x the recorded restatement error, floored at the rounding bound of the quantity."""
    g, k = sr.gold(), sr.SCENES.index(name)
    floor = _generator().floors(int(g[name + "_params"][8]))
    return {key: max(20.0 * float(g["restatement_err_" + key][k]), floor[key]) for key in KEYS}


def device_bars(name):
    """(mean, cov, feature rows) as compare_frame takes them: the feature rows are float32 on the device."""
    b = bars(name)
    return b["mean"], b["cov"], b["feat32"]


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_fixture_contents():
    g, gen = sr.gold(), _generator()
    assert os.path.getsize(sr.GOLD) < 1 << 20
    assert all(v.dtype.kind in "fiu" for v in g.values())                         # arrays of numbers only
    for key in KEYS:
        e = g["restatement_err_" + key]
        assert e.shape == (3,) and np.isfinite(e).all() and (e >= 0).all(), key
        if key not in ("iou", "feat"):                                             # the two the restatement computes with the reference's own operations
            assert (e > 0).all(), key
    for name in sr.SCENES:
        b, fl = bars(name), gen.floors(int(g[name + "_params"][8]))
        assert all(1000 * b[k] < gen.MARGIN for k in ("mean", "cov", "iou", "gate")) and 1000 * b["cost"] < gen.MARGIN_APP
        assert all(fl[k] > 0 for k in KEYS)
    factor = float(g["appearance_margin_factor"][0])
    assert 100 <= factor <= 1000 and all(factor * bars(name)["cost32"] <= gen.MARGIN_APP for name in sr.SCENES)
    scenes = {name: sr.load_scene(name) for name in sr.SCENES}
    for name, (p, frames) in scenes.items():
        assert (p["max_age"], p["n_init"], p["E"], p["woc"], p["mc_lambda"] is None) == (3, 3, 32, name == "small_woc", name == "small_woc")
        assert len(frames) == p["frames"] and g[name + "_feat"].dtype == np.float32 and g[name + "_warp"].shape == (p["frames"], 3, 3)
        for fr in frames:
            T, m = len(fr["trk_int"]), len(fr["det"])
            assert fr["det"].shape == (m, 5) and fr["feat"].shape == (m, 32)
            assert fr["trk_mean"].shape == (T, 8) and fr["trk_cov"].shape == (T, 8, 8) and fr["trk_feat"].shape == (T, 32) and fr["trk_int"].shape == (T, 5)
            assert fr["out_tlwh"].shape == (len(fr["out_id"]), 4) and fr["match"].shape[1] == 2 and T <= p["capacity"]
            assert np.allclose(np.linalg.norm(fr["trk_feat"], axis=1), 1.0, atol=1e-12)
            for c in fr["calls"]:
                assert c["cost"].shape == (len(c["rows"]), len(c["cols"])) and c["cost"].size and (c["cost"] <= c["limit"] + 1e-5).all()
                assert c["limit"] == (p["match_thresh"] if c["kind"] == 0 else p["max_iou"])
    small, woc, crowded = (scenes[n][1] for n in sr.SCENES)
    assert len(small) == 40 and len(crowded) == 12 and max(len(fr["trk_int"]) for fr in small) <= 14
    assert all(np.array_equal(a["det"], b["det"]) and np.array_equal(a["feat"], b["feat"]) for a, b in zip(small, woc))
    assert np.array_equal(g["small_warp"], g["small_woc_warp"]) and g["small_warp_on"].sum() == 3 and g["crowded_warp_on"].sum() == 1
    for kind in (0, 1):                                                            # more than one 16 x 64 tile, both ways, in both planes
        assert any(c["kind"] == kind and len(c["rows"]) > 16 and len(c["cols"]) > 64 for fr in crowded for c in fr["calls"])
    found = {}
    gen.check_scenes(scenes, found)                                                # every case of gen.CASES, and the margins, from the fixture alone
    print("\n".join("%s: %s" % kv for kv in sorted(found.items())))
    assert len(gen.CASES) == 19 and set(gen.CASES) <= set(found)
    assert len(small[29]["det"]) == 0 and len(small[29]["trk_int"])


@pytest.mark.skipif(not os.path.exists(REFERENCE), reason="the reference tree is not on this machine")
def test_generator_reproduces_the_fixture():
    gen = _generator()
    made, g = gen.make(gen.load_reference()), sr.gold()          # make() asserts the cases and the margins on the way
    assert sorted(made) == sorted(g)
    for k in g:
        assert made[k].dtype == g[k].dtype and made[k].shape == g[k].shape and made[k].tobytes() == g[k].tobytes(), k


@pytest.mark.parametrize("name", sr.SCENES)
def test_numpy_replay(name):
    """The driver on the numpy backend, in float64 and with float32 features: every decision is the reference's, and the distances are the
    recorded ones (that is their definition)."""
    g, k, gen = sr.gold(), sr.SCENES.index(name), _generator()
    for f32 in (False, True):
        worst = {"iou": 0.0, "cost": 0.0, "gate": 0.0}

        def on_frame(rp, want, f):
            gen.compare_calls(rp.backend.calls, want["calls"], worst, (name, f + 1))
        bad, err, rp = sr.replay_scene(name, lambda cap, e, q: sr.NumpyBackend(cap, e, q, f32=f32), on_frame=on_frame)
        assert bad is None, bad
        print("%s: numpy replay%s mean %.3g  covariance %.3g  iou %.3g  gate %.3g  feature %.3g  cost %.3g  output tlwh %.3g" % (
            name, " (float32 features)" if f32 else "", err["mean"], err["cov"], worst["iou"], worst["gate"], err["feat"], worst["cost"],
            err.get("tlwh", 0.0)))
        if f32:
            assert err["feat"] == g["restatement_err_feat32"][k] and worst["cost"] == g["restatement_err_cost32"][k]
        else:
            got = dict(mean=err["mean"], cov=err["cov"], feat=err["feat"], **worst)
            assert all(got[key] == g["restatement_err_" + key][k] for key in KEYS[:6]), got
        assert err.get("tlwh", 0.0) <= bars(name)["mean"]
        if name != "crowded":                                    # the slot of a deleted track is taken again at a later birth
            assert any(len(ids) > 1 for ids in rp.slot_history.values())


@pytest.mark.parametrize("deviation", sr.DEVIATIONS)
def test_sensitivity(deviation):
    """Each planted misreading of the reference makes the replay of some scene leave the fixture - in ids, pairs, or states beyond the bars.  The
    switches live in tests/sort_replay.py; the product code has none."""
    found = []
    for name in sr.SCENES:
        b = bars(name)
        bad, _, _ = sr.replay_scene(name, lambda cap, e, q: sr.NumpyBackend(cap, e, q, (deviation,)), deviations=(deviation,),
                                    bars=(b["mean"], b["cov"], b["feat"]))
        if bad is not None:
            found.append("%s, %s" % (name, bad.splitlines()[0]))
    print("%s: %s" % (deviation, "; ".join(found)))
    assert found, "%s: no scene notices (no diverging frame)" % deviation


def test_the_order_fix_is_what_small_notices():
    """With the advance step in the old order - predict, then the camera update - the replay of `small` fails on its first camera frame that has
    rotation and scale, and nowhere before."""
    b = bars("small")
    bad, _, rp = sr.replay_scene("small", lambda cap, e, q: sr.NumpyBackend(cap, e, q, ("predict_before_camera",)), bars=(b["mean"], b["cov"], b["feat"]))
    warps = sr.gold()["small_warp"]
    first = [f for f in range(40) if sr.gold()["small_warp_on"][f] and abs(warps[f][0, 1]) > 1e-3][0]
    assert bad is not None and bad.startswith("frame %d: states off by" % (first + 1)), bad


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _raw_cost(st, slots, tsu, confirmed, tlwh, feats, p, guard=64, canary=777.25):
    """busca_sframe_cost itself on the state as it is, into a slab with a guard band on both sides (as _raw_cost of tests/test_sort_frame.py)
    -> (the slab [2, n, m], first, again)."""
    import torch
    from busca_amd import _sframe_lib
    from busca_amd.sort_store import INFTY_COST, _match_stage_tables
    from tests.test_kalman_store import _dev
    n, m = len(slots), len(tlwh)
    first, again = _match_stage_tables(tsu, confirmed, p["depth"])
    depth = 1 if p["depth"] is None else p["depth"]
    cost = sr.RowMetric(st, p["match_thresh"]).distance(_dev(np.ascontiguousarray(feats, dtype=np.float32)), [int(s) for s in slots], device=True)
    buf = torch.full((2 * n * m + 2 * guard,), canary, dtype=torch.float64, device=st.dev)
    status = torch.full((n + 2 * guard,), -7, dtype=torch.int32, device=st.dev)
    d = [_dev(np.ascontiguousarray(x)) for x in (sr.xyah_of(tlwh), np.asarray(tlwh, dtype=np.float64), (np.asarray(tsu) > 1).astype(np.uint8),
                                                  first.astype(np.int32), again.astype(np.int32), np.asarray(slots, dtype=np.int32))]
    lam = p["mc_lambda"]
    _sframe_lib.check(_sframe_lib.load().busca_sframe_cost(
        st.mean.data_ptr(), st.cov.data_ptr(), st.capacity, d[5].data_ptr(), n, d[0].data_ptr(), d[1].data_ptr(), m, d[2].data_ptr(), cost.data_ptr(), m,
        INFTY_COST, (_sframe_lib.MC if lam is not None else 0) | _sframe_lib.CLAMP, 0.0 if lam is None else lam, p["match_thresh"], p["max_iou"],
        d[3].data_ptr(), d[4].data_ptr(), depth, buf.data_ptr() + 8 * guard, status.data_ptr() + 4 * guard, *st._where()))
    buf, status = buf.cpu().numpy(), status.cpu().numpy()
    assert (buf[:guard] == canary).all() and (buf[guard + 2 * n * m:] == canary).all(), "written outside the slab"
    assert (status[:guard] == -7).all() and (status[guard + n:] == -7).all(), "written outside the status words"
    assert not status[guard:guard + n].any()
    return buf[guard:guard + 2 * n * m].reshape(2, n, m), first, again


def _device(cap, e, p):
    return sr.DeviceBackend(cap, e, p)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sr.SCENES)
def test_replay_through_frame(name):
    """One SortStore.frame per recorded frame: the decisions exactly (compare_frame: matches in _match's order, both unmatched lists, new tracks and
    their slots, the state machine, deletions, output ids), means, covariances, feature rows and output boxes within the bars, a newborn's Kalman
    state bit for bit, no overflow (Replay.finish asserts it), and the slot of a deleted track taken again."""
    b = bars(name)
    bad, err, rp = sr.replay_scene(name, _device, bars=device_bars(name))
    print("%s: SortStore.frame replay mean %.3g (bar %.3g)  covariance %.3g (bar %.3g)  feature rows %.3g (bar %.3g)  output tlwh %.3g (bar %.3g)" % (
        name, err["mean"], b["mean"], err["cov"], b["cov"], err["feat"], b["feat32"], err.get("tlwh", 0.0), b["mean"]))
    assert bad is None, bad
    if name != "crowded":
        reused = [s for s, ids in rp.slot_history.items() if len(ids) > 1]
        assert reused, "the slot of a deleted track was not taken again"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sr.SCENES)
def test_cost_slab_equals_the_recorded_matrices(name):
    """Raw busca_sframe_cost on the replay's advanced state, at every frame with recorded matrices: plane 0 at the rows and columns of a recorded
    cascade call is that call's matrix (within the float32 cost bar), plane 1 at the IoU call's rows and columns its matrix (within the IoU bar);
    +inf exactly where a row is not in a plane; guard words and canaries intact.  Every recorded matrix is met."""
    from busca_amd.sort_store import SortStore
    p, frames = sr.load_scene(name)
    b = bars(name)
    worst, checked = {0: 0.0, 1: 0.0}, [0]

    def before_frame(rp, want, f, args):
        slots, tsu, confirmed, tlwh, _, feats, _, matrix = args
        if not len(slots) or not len(tlwh):
            return
        src = rp.backend.store
        probe = SortStore(src.capacity, feature_dim=p["E"])      # a copy of the state, advanced as frame() is about to advance it
        probe._state()
        probe.mean, probe.cov, probe.feat = src.mean.clone(), src.cov.clone(), src.feat.clone()
        if matrix is not None:
            probe.camera_update(slots, matrix)
        probe.predict(slots)
        slab, first, again = _raw_cost(probe, slots, tsu, confirmed, tlwh, feats, p)
        depth = 1 if p["depth"] is None else p["depth"]
        in0, in1 = (first >= 0) & (first < depth), (first == depth) | (again == depth)
        assert np.isposinf(slab[0][~in0]).all() and np.isposinf(slab[1][~in1]).all(), (name, f + 1)
        assert np.isfinite(slab[0][in0]).all() and np.isfinite(slab[1][in1]).all(), (name, f + 1)
        for c in want["calls"]:
            got = slab[c["kind"]][np.ix_(c["rows"], c["cols"])]
            d = float(np.abs(got - c["cost"]).max())
            worst[c["kind"]], checked[0] = max(worst[c["kind"]], d), checked[0] + 1
            assert d <= (b["cost32"], b["iou"])[c["kind"]], (name, f + 1, c["kind"], d)
    bad, _, _ = sr.replay_scene(name, _device, bars=device_bars(name), before_frame=before_frame)
    print("%s: busca_sframe_cost against %d recorded matrices: plane 0 %.3g (bar %.3g)  plane 1 %.3g (bar %.3g)" % (
        name, checked[0], worst[0], b["cost32"], worst[1], b["iou"]))
    assert bad is None, bad
    recorded = sum(len(fr["calls"]) for fr in frames)
    assert checked[0] == recorded and recorded >= 15                              # every recorded matrix, of both planes, was met


def _same_frames(a, b, where):
    for field in sr.Frame._fields:
        x, y = ([tuple(int(v) for v in e) if isinstance(e, tuple) else int(e) for e in getattr(fr, field)] for fr in (a, b))
        assert x == y, (where, field, x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sr.SCENES)
def test_composed_route_stays_bit_identical(name):
    """The same replay through camera_update, predict, match, update, initiate and busca_store_ema_fit on a second store: after every one of the
    chained frames the same lists and the same bits in mean, cov and feat as frame()."""
    p, frames = sr.load_scene(name)
    a, b = sr.Replay(sr.DeviceBackend(p["capacity"], p["E"], p), p), sr.Replay(sr.ComposedBackend(p["capacity"], p["E"], p), p)
    for f, want in enumerate(frames):
        for rp in (a, b):
            rp.step(want["det"], want["feat"], want["warp"])
        _same_frames(a.fr, b.fr, (name, f + 1))
        assert np.array_equal(a.held()[0], b.held()[0]) and a.free() == b.free(), (name, f + 1)
        sa, sb = a.backend.store, b.backend.store
        for x, y, what in ((sa.mean, sb.mean, "mean"), (sa.cov, sb.cov, "cov"), (sa.feat, sb.feat, "feat")):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy()), (name, f + 1, what)
    assert np.array_equal(a.held()[0], frames[-1]["trk_int"])                      # and it is the recorded scene that was replayed


@pytest.mark.gpu
def test_batched_replay():
    """`small`, a second `small` that starts five steps later and `crowded` in lock step through SortStore.frame_batch, on disjoint slot ranges
    of one store: every problem's decisions are the fixture's, its states within the bars, and after every step the store is bit for bit what
    frame() leaves sequence by sequence on a second store."""
    from busca_amd.sort_store import SortStore
    scenes = [sr.load_scene(n) for n in ("small", "small", "crowded")]
    names, shift = ("small", "small", "crowded"), (0, 5, 0)
    p = scenes[0][0]
    assert all(all(q[k] == p[k] for k in ("max_age", "n_init", "max_iou", "match_thresh", "ema_alpha", "mc_lambda", "depth", "E")) for q, _ in scenes)
    base = np.concatenate([[0], np.cumsum([q["capacity"] for q, _ in scenes])])
    stores = [SortStore(int(base[-1]), feature_dim=p["E"]) for _ in range(2)]
    replays = [[sr.Replay(sr.DeviceBackend(int(base[-1]), p["E"], p, store=st), p, base=int(base[k]), capacity=q["capacity"])
                for k, (q, _) in enumerate(scenes)] for st in stores]
    frames_of = [[None] * s + fr for s, (_, fr) in zip(shift, scenes)]
    errs = [{"mean": 0.0, "cov": 0.0, "feat": 0.0} for _ in scenes]
    busiest = 0
    for step, wants in sr.run_batched(stores[0], replays[0], frames_of):
        active = [k for k, w in enumerate(wants) if w is not None]
        busiest = max(busiest, len(active))
        for k in active:
            bad = sr.compare_frame(replays[0][k], wants[k], step - shift[k], errs[k], device_bars(names[k]))
            assert bad is None, (names[k], k, bad)
            one = replays[1][k]
            one.step(wants[k]["det"], wants[k]["feat"], wants[k]["warp"])          # the same frame through frame(), on the second store
            _same_frames(replays[0][k].fr, one.fr, (step, k))
        for x, y, what in ((stores[0].mean, stores[1].mean, "mean"), (stores[0].cov, stores[1].cov, "cov"), (stores[0].feat, stores[1].feat, "feat")):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy()), (step, what)
    assert busiest == 3 and step == 44
    for k, e in enumerate(errs):
        print("%s (problem %d): frame_batch replay mean %.3g  covariance %.3g  feature rows %.3g  output tlwh %.3g" % (
            names[k], k, e["mean"], e["cov"], e["feat"], e.get("tlwh", 0.0)))
