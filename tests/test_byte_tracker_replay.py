"""BYTETracker.update of the reference, replayed through KalmanStore.frame.

The reference is tests/golden/byte_tracker.npz: adapters/ByteTrack/yolox/tracker/byte_tracker.py itself, run by
tests/golden/make_golden_byte_tracker.py over three scripted scenes (small, the same detections with mot20, crowded) with its own cost matrices,
limits, pairs, duplicate decisions and removals recorded frame by frame.  tests/byte_replay.py is the adapter loop INTEGRATION.md prints for
KalmanStore.frame, made executable; here it drives the recorded detections through a numpy float64 backend (CPU), through KalmanStore.frame and
through the composed route of three round() calls, update and initiate (GPU).  Everything discrete - ids, the fields of the state machine, list
memberships and order, removed ids, output ids, the pairs of the three rounds, unmatched_pool against the reference's unassigned_stracks - is
compared exactly.

Bars.  update goes through LAPACK in the reference, so the states and everything computed from them (the cost matrices, the output boxes) are
compared within 20 x the distance of the numpy restatement from the reference, recorded in the fixture as restatement_err_mean / _cov / _cost
(the convention of tests/test_kalman_filter.bars: room for a third valid evaluation order, none for a wrong formula); initiation is exact.  The
bars come from the fixture and never from a kernel's output.  None of the recorded restatement errors is zero; were one zero, the bar's floor
would be the rounding bound of that quantity and not a chosen number: with u = 2^-53, a state entry that no update has touched is a sum of at
most F products of entries of the recorded initiation by powers of the motion matrix, (F + 1) u relative after F predictions; a cost entry
1 - s * (iw * ih) / ((a + b) - iw * ih) is 4 differences (+1 each, 8 roundings), 3 products, 2 sums, 1 quotient, 1 product by the score and the
final difference, at most 16 u in absolute value as every intermediate ratio is at most 1.  `bars()` applies these floors.
The generator asserts that every decision of every frame has a margin of 1e-6 (unique optima, costs off their limits, duplicate costs off 0.15,
scores off the thresholds but for three deliberate equalities) and that 1e-6 exceeds 1000 x every bar: a device result within its bars cannot
change a decision, so exact comparison of the decisions is meaningful.

Measured on one MI355X (printed by the GPU tests): see DESIGN.md, K-FRAME."""
import importlib.util
import os

import numpy as np
import pytest

from tests import byte_replay as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATOR = os.path.join(ROOT, "tests", "golden", "make_golden_byte_tracker.py")
U = 2.0 ** -53
_CACHE = {}


def _generator():
    if "gen" not in _CACHE:
        spec = importlib.util.spec_from_file_location("make_golden_byte_tracker", GENERATOR)
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)
        _CACHE["gen"] = gen
    return _CACHE["gen"]


REFERENCE = _generator().REF                               # where the generator looks for the reference tree


def bars(name):
    """-> (mean, cov, cost) bars of a scene: 20 x the recorded restatement error, floored at the rounding bound of the quantity."""
    g, k = br.gold(), br.SCENES.index(name)
    frames = int(g[name + "_params"][4])
    floor = ((frames + 1) * U, (frames + 1) * U, 16 * U)
    return tuple(max(20.0 * float(g["restatement_err_" + key][k]), fl) for key, fl in zip(("mean", "cov", "cost"), floor))


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_fixture_contents():
    g = br.gold()
    gen = _generator()
    assert os.path.getsize(br.GOLD) < 1 << 20
    assert all(v.dtype.kind in "fiu" for v in g.values())                         # arrays of numbers only
    for key in ("mean", "cov", "cost"):
        e = g["restatement_err_" + key]
        assert e.shape == (3,) and np.isfinite(e).all() and (e > 0).all() and 1000 * 20 * e.max() < gen.MARGIN
    scenes = {name: br.load_scene(name) for name in br.SCENES}
    for name, (params, frames) in scenes.items():
        assert params["mot20"] == (name == "small_mot20") and params["track_buffer"] == 5 and len(frames) == params["frames"]
        for fr in frames:
            T = len(fr["trk_int"])
            assert fr["det"].shape[1] == 5 and fr["trk_mean"].shape == (T, 8) and fr["trk_cov"].shape == (T, 8, 8) and fr["trk_int"].shape == (T, 7)
            assert fr["out_tlwh"].shape == (len(fr["out_id"]), 4)
            for r in fr["rounds"]:
                assert r["cost"].shape == (len(r["rows"]), len(r["cols"])) and r["pairs"].shape[1] == 2
    assert len(scenes["small"][1]) == 40 and len(scenes["crowded"][1]) == 12
    assert max(len(fr["trk_int"]) for fr in scenes["small"][1]) <= 12
    assert all(np.array_equal(a["det"], b["det"]) for a, b in zip(scenes["small"][1], scenes["small_mot20"][1]))
    big = [f for f, fr in enumerate(scenes["crowded"][1]) if len(fr["rounds"][0]["rows"]) + len(fr["rounds"][2]["rows"]) > 16 and len(fr["det"]) > 64]
    assert big and scenes["crowded"][1][big[0]]["rounds"][0]["cost"].size                # more than one 16 x 64 tile, both ways, matrices kept
    assert any([r["pairs"].tolist() for r in a["rounds"]] != [r["pairs"].tolist() for r in b["rounds"]]
               for a, b in zip(scenes["small"][1], scenes["small_mot20"][1]))
    gen.check_scenes(scenes)                                     # every case of gen.CASES, and the margins, from the fixture alone
    small = scenes["small"][1]
    assert small[0]["trk_int"][:, 2].all() and len(small[24]["det"]) == 0 and (small[29]["det"][:, 4] < 0.5).all()
    scores = np.concatenate([fr["det"][:, 4] for fr in small])
    assert (scores == 0.5).sum() == 1 and (scores == 0.1).sum() == 1 and (scores == 0.5 + 0.1).sum() == 1
    assert any(len(fr["dup_a"]) for fr in small) and any(len(fr["dup_b"]) for fr in small) and any(len(fr["rounds"][1]["pairs"]) for fr in small)
    assert any(3 in fr["trk_int"][:, 1] for fr in small)                              # an expired track, still listed for a frame
    assert len(gen.CASES) == 20


@pytest.mark.skipif(not os.path.exists(REFERENCE), reason="the reference tree is not on this machine")
def test_generator_reproduces_the_fixture():
    gen = _generator()
    made, g = gen.make(gen.load_reference()), br.gold()          # make() asserts the cases and the margins on the way
    assert sorted(made) == sorted(g)
    for k in g:
        assert made[k].dtype == g[k].dtype and made[k].shape == g[k].shape and made[k].tobytes() == g[k].tobytes(), k


@pytest.mark.parametrize("name", br.SCENES)
def test_numpy_replay(name):
    """The driver on the numpy backend: every decision is the reference's, and the distances are the recorded ones (that is their definition)."""
    g, k = br.gold(), br.SCENES.index(name)
    worst = [0.0]

    def on_frame(rp, want, f):
        for r in range(3):
            ref = want["rounds"][r]
            rows = [(rp.pool if r < 2 else rp.unconfirmed)[i].track_id for i in rp.backend.rounds[r][0]]
            assert rows == ref["rows"].tolist() and rp.backend.rounds[r][1] == ref["cols"].tolist(), (name, f + 1, r)
            if ref["cost"].size:
                worst[0] = max(worst[0], float(np.abs(rp.backend.costs[r] - ref["cost"]).max()))
    bad, err, rp = br.replay_scene(name, br.NumpyBackend, on_frame=on_frame)
    assert bad is None, bad
    print("%s: numpy replay mean %.3g  covariance %.3g  cost %.3g" % (name, err["mean"], err["cov"], worst[0]))
    assert err["mean"] == g["restatement_err_mean"][k] and err["cov"] == g["restatement_err_cov"][k] and worst[0] == g["restatement_err_cost"][k]
    assert err.get("tlwh", 0.0) <= bars(name)[0]
    if name.startswith("small"):                                 # the slot of the expired track is taken again at the later birth
        assert len(rp.slot_history[0]) > 1


@pytest.mark.parametrize("deviation", br.DEVIATIONS)
def test_sensitivity(deviation):
    """Each planted misreading of byte_tracker.py makes the replay of `small` or `crowded` leave the fixture - in ids, pairs, or states beyond the
    bars.  The switches live in tests/byte_replay.py; the product code has none."""
    found = []
    for name in ("small", "crowded"):
        bad, _, _ = br.replay_scene(name, lambda cap: br.NumpyBackend(cap, (deviation,)), deviations=(deviation,), bars=bars(name)[:2])
        if bad is not None:
            found.append("%s, %s" % (name, bad.splitlines()[0]))
    print("%s: %s" % (deviation, "; ".join(found)))
    assert found, "%s: neither scene notices (no diverging frame)" % deviation


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _raw_cost(store, slots, dets, scores, cls, mot20, guard=64, canary=777.25):
    """busca_frame_cost itself into a slab with a guard band on both sides -> the slab [2, n, m] (as tests/test_byte_frame._raw_cost)."""
    import torch
    from busca_amd import _frame_lib
    from tests.test_kalman_store import _dev
    n, m = len(slots), len(dets)
    det = store.detections(dets, scores)
    buf = torch.full((2 * n * m + 2 * guard,), canary, dtype=torch.float64, device=store.dev)
    status = torch.full((n + 2 * guard,), -7, dtype=torch.int32, device=store.dev)
    d_cls, slot = _dev(cls), _dev(np.asarray(slots, dtype=np.int32))
    _frame_lib.check(_frame_lib.load().busca_frame_cost(store.mean.data_ptr(), store.cov.data_ptr(), store.capacity, slot.data_ptr(), n, det.tlbr.data_ptr(),
                                                        None if mot20 else det.score.data_ptr(), d_cls.data_ptr(), m,
                                                        buf.data_ptr() + 8 * guard, status.data_ptr() + 4 * guard, *store._where()))
    buf, status = buf.cpu().numpy(), status.cpu().numpy()
    assert (buf[:guard] == canary).all() and (buf[guard + 2 * n * m:] == canary).all(), "written outside the slab"
    assert (status[:guard] == -7).all() and (status[guard + n:] == -7).all(), "written outside the status words"
    assert not status[guard:guard + n].any()
    return buf[guard:guard + 2 * n * m].reshape(2, n, m)


@pytest.mark.gpu
@pytest.mark.parametrize("name", br.SCENES)
def test_replay_through_frame(name):
    """One KalmanStore.frame per recorded frame: the decisions exactly, the states and output boxes within the bars, new tracks bit for bit, no
    overflow (Replay.step asserts it), and the expired track's slot taken again."""
    params, frames = br.load_scene(name)

    def on_frame(rp, want, f):
        sc = want["det"][:, 4]
        cls = np.where(sc > params["track_thresh"], 0, np.where(np.logical_and(sc > 0.1, sc < params["track_thresh"]), 1, 2))
        assert np.array_equal(rp.fr.det_class, cls) and list(rp.fr.overflow) == [], (name, f + 1)
    bad, err, rp = br.replay_scene(name, br.DeviceBackend, bars=bars(name)[:2], on_frame=on_frame)
    print("%s: KalmanStore.frame replay mean %.3g (bar %.3g)  covariance %.3g (bar %.3g)  output tlwh %.3g" %
          ((name, err["mean"], bars(name)[0], err["cov"], bars(name)[1], err.get("tlwh", 0.0))))
    assert bad is None, bad
    if name.startswith("small"):
        assert len(rp.slot_history[0]) > 1, "the slot of the expired track was not taken again"


@pytest.mark.gpu
@pytest.mark.parametrize("name", br.SCENES)
def test_cost_slab_equals_the_recorded_matrices(name):
    """Raw busca_frame_cost on the replay's predicted state, at every frame with recorded matrices: plane 0 at (pool rows, first-round columns) is
    the reference's round-one matrix, plane 1 at (round-two rows, second-round columns) its round-two matrix, plane 0 at (unconfirmed rows, round
    three's columns) its round-three matrix, each within 20 x restatement_err_cost; +inf exactly where a column is not in a plane; guard words and
    canaries intact."""
    from busca_amd.kalman_store import KalmanStore
    params, frames = br.load_scene(name)
    bar = bars(name)[2]
    worst, checked = [0.0], [0]

    def before_frame(rp, pool, flags, unconfirmed, dets, scores):
        want = frames[rp.frame_id - 1]
        slots = [t.slot for t in pool] + [t.slot for t in unconfirmed]
        if not slots or not len(dets):
            return
        probe = KalmanStore(rp.backend.capacity)                # a copy of the state, predicted as frame() is about to predict it
        probe.mean, probe.cov = rp.backend.store.mean.clone(), rp.backend.store.cov.clone()
        probe.predict([t.slot for t in pool], flags)
        cls = np.full(len(scores), 2, dtype=np.uint8)
        cls[np.logical_and(scores > 0.1, scores < params["track_thresh"])] = 1
        cls[scores > params["track_thresh"]] = 0
        slab = _raw_cost(probe, slots, dets, scores, cls, params["mot20"])
        assert np.isposinf(slab[0][:, cls != 0]).all() and np.isposinf(slab[1][:, cls != 1]).all()
        assert np.isfinite(slab[0][:, cls == 0]).all() and np.isfinite(slab[1][:, cls == 1]).all()
        ids = [t.track_id for t in pool] + [t.track_id for t in unconfirmed]
        for r, plane in ((0, 0), (1, 1), (2, 0)):
            ref = want["rounds"][r]
            if ref["cost"] is None or not ref["cost"].size:
                continue
            got = slab[plane][np.ix_([ids.index(int(i)) for i in ref["rows"]], ref["cols"])]
            d = float(np.abs(got - ref["cost"]).max())
            worst[0], checked[0] = max(worst[0], d), checked[0] + 1
            assert d <= bar, (name, rp.frame_id, r, d, bar)
    bad, _, _ = br.replay_scene(name, br.DeviceBackend, bars=bars(name)[:2], before_frame=before_frame)
    print("%s: busca_frame_cost against %d recorded matrices: %.3g (bar %.3g)" % (name, checked[0], worst[0], bar))
    assert bad is None, bad
    recorded = sum(1 for fr in frames for r in fr["rounds"] if r["cost"] is not None and r["cost"].size)
    assert checked[0] == recorded and recorded >= 12                               # every recorded matrix, of every round, was met


@pytest.mark.gpu
@pytest.mark.parametrize("name", br.SCENES)
def test_composed_route_stays_bit_identical(name):
    """The same replay through three round() calls, update and initiate on a second store: after every one of the chained frames the same lists,
    the same pairs and the same bits in every slot as frame()."""
    params, frames = br.load_scene(name)
    a = br.Replay(br.DeviceBackend(params["capacity"]), params["track_thresh"], params["track_buffer"], params["match_thresh"], params["mot20"])
    b = br.Replay(br.ComposedBackend(params["capacity"]), params["track_thresh"], params["track_buffer"], params["match_thresh"], params["mot20"])
    for f, want in enumerate(frames):
        a.step(want["det"])
        b.step(want["det"])
        for field in br.Frame._fields[:-1]:
            assert [tuple(int(v) for v in x) if isinstance(x, tuple) else int(x) for x in getattr(a.fr, field)] == \
                   [tuple(int(v) for v in x) if isinstance(x, tuple) else int(x) for x in getattr(b.fr, field)], (name, f + 1, field)
        assert np.array_equal(a.fr.det_class, b.fr.det_class) and a.pairs == b.pairs and a.free == b.free, (name, f + 1)
        assert np.array_equal(a.held()[0], b.held()[0]), (name, f + 1)
        sa, sb = a.backend.store, b.backend.store
        assert np.array_equal(sa.mean.cpu().numpy(), sb.mean.cpu().numpy()) and np.array_equal(sa.cov.cpu().numpy(), sb.cov.cpu().numpy()), (name, f + 1)


@pytest.mark.gpu
def test_duplicate_masks_are_the_recorded_ones():
    """tracking.remove_duplicate_stracks on the replay's boxes returns the reference's survivors at the frames where duplicates occur - from the
    tracked list (an older or equally old lost track wins) and from the lost list."""
    seen = set()
    for name in br.SCENES:
        params, frames = br.load_scene(name)

        def on_frame(rp, want, f):
            if len(want["dup_a"]) or len(want["dup_b"]):
                assert rp.dup_a == want["dup_a"].tolist() and rp.dup_b == want["dup_b"].tolist()
                seen.update(["a"] * bool(rp.dup_a) + ["b"] * bool(rp.dup_b))
                listed = want["trk_int"]
                assert not set(rp.dup_a + rp.dup_b) & set(listed[:, 0].tolist())
        bad, _, _ = br.replay_scene(name, br.DeviceBackend, bars=bars(name)[:2], on_frame=on_frame)
        assert bad is None, bad
    assert seen == {"a", "b"}
