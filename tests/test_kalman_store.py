"""ByteTrack's Kalman state resident on the device: libbusca_track.so (include/busca_track.h), its binding and busca_amd.kalman_store.KalmanStore.

References: tests/golden/kalman_store.npz, a 16-frame script run through the reference's vendored KalmanFilter by
tests/golden/make_golden_kalman_store.py; tests/golden/kalman.npz; and the list-ordered kernels and wrappers this repository had before
(busca_kalman_*, kalman._predicted_cost_dev, associate_round), which the slot-indexed ones must equal bit for bit.  Predicted and initiated states
are compared with np.array_equal; updated states against the reference with the chain bars of tests/test_kalman_filter.py (20 x the worst
disagreement of its float64 restatement with the reference), as the list-ordered update kernel is."""
import importlib.util
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

from tests.test_kalman_filter import _detections, _tracks, bars, err_cov, err_mean, gold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kalman_store.npz")
GENERATOR = os.path.join(ROOT, "tests", "golden", "make_golden_kalman_store.py")
CAP = 16
_CACHE = {}


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_kalman_store", GENERATOR)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


REFERENCE = _generator().REF                               # where the generator looks for the reference tree


def script():
    if "s" not in _CACHE:
        with np.load(GOLD) as f:
            _CACHE["s"] = {k: f[k] for k in f.files}
    return _CACHE["s"]


def phase(f, key_slot, key_n, *more):
    """The lists of one phase of frame f (1-based), cut to their length."""
    s = script()
    k = int(s[key_n][f - 1])
    return [s[key][f - 1, :k].copy() for key in (key_slot,) + more]


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    from busca_amd.build import build
    hip_lib = build()
    from busca_amd import _lib, _track_lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "busca_track.h")).read(), flags=re.S)
    declared = {}
    for name, args in re.findall(r"\b(busca_track_[a-z0-9_]+)\s*\((.*?)\)\s*;", hdr, flags=re.S):
        declared[name] = 0 if args.strip() == "void" else len(args.split(","))
    assert declared == {name: len(args) for name, (_, args) in _track_lib.TRACK_API.items()}
    assert len(declared) == 7

    def exported(path):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    assert {n for n in exported(_track_lib.TRACK_LIB_PATH) if not n.startswith("_")} == set(_track_lib.TRACK_API)
    assert os.path.basename(hip_lib) == "libbusca_hip.so" and not [n for n in exported(hip_lib) if n.startswith("busca_track")]
    assert not [n for n in exported(_track_lib.TRACK_LIB_PATH) if n in {k for t in _lib.HEADERS.values() for k in t}]
    assert "busca_track.h" not in _lib.HEADERS and "_track_lib" not in open(_lib.__file__.replace(".pyc", ".py")).read()
    lib = _track_lib.load()
    assert lib.busca_track_version() == 1000 and lib.busca_track_last_error() is not None


def test_refusals_and_noops_need_no_gpu():
    """Every argument is checked before the first HIP call: the pointers below are never followed."""
    from busca_amd import _track_lib
    lib = _track_lib.load()
    P, ODD, S, n, m = 0x10000, 0x10004, 8, 3, 5          # an aligned address, one that is 4- but not 8-byte aligned

    def calls(mean=P, cov=P, S=S, slot=P, n=n, meas=P, det=P, m=m, status=P, out=P, tlbr=1, nt=None, xyah=P, score=None, flags=1, lam=0.98, dev=0):
        return {
            "busca_track_kalman_initiate": lambda: lib.busca_track_kalman_initiate(mean, cov, S, slot, n, meas, det, m, dev, None),
            "busca_track_kalman_predict": lambda: lib.busca_track_kalman_predict(mean, cov, S, slot, nt, n, dev, None),
            "busca_track_kalman_update": lambda: lib.busca_track_kalman_update(mean, cov, S, slot, n, meas, det, m, status, dev, None),
            "busca_track_kalman_boxes": lambda: lib.busca_track_kalman_boxes(mean, S, slot, n, tlbr, out, dev, None),
            "busca_track_round_cost": lambda: lib.busca_track_round_cost(mean, cov, S, slot, n, meas, xyah, score, m, flags, lam, out, status, dev, None),
        }

    def refused(name, words, **kw):
        rc = calls(**kw)[name]()
        msg = lib.busca_track_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":") and words in msg, (name, kw, rc, msg)

    every = list(calls())
    for name in every:
        assert calls(n=0)[name]() == 0, name                                       # the no-op
        assert calls(n=0, mean=None, cov=None, slot=None, out=None)[name]() == 0, name
        refused(name, "null pointer", mean=None)
        refused(name, "null pointer", slot=None)
        refused(name, "negative size", n=-1)
        refused(name, "negative size", S=-1)
        refused(name, "negative device", dev=-1)
        refused(name, "misaligned", mean=ODD)
        refused(name, "misaligned", slot=0x10002)
    for name in ("busca_track_kalman_initiate", "busca_track_kalman_predict", "busca_track_kalman_update"):
        refused(name, "null pointer", cov=None)
        refused(name, "misaligned", cov=ODD)
    for name in ("busca_track_kalman_initiate", "busca_track_kalman_update"):
        refused(name, "null pointer", meas=None)
        refused(name, "negative size", m=-1)
        refused(name, "misaligned", meas=ODD)
        refused(name, "misaligned", det=0x10002)
        refused(name, "no det_index", det=None, n=6)
        assert calls(det=None, n=0)[name]() == 0
    refused("busca_track_kalman_update", "misaligned", status=0x10002)
    refused("busca_track_kalman_boxes", "null pointer", out=None)
    refused("busca_track_kalman_boxes", "misaligned", out=ODD)
    refused("busca_track_kalman_boxes", "tlbr", tlbr=2)
    name = "busca_track_round_cost"
    assert calls(m=0)[name]() == 0
    refused(name, "negative size", m=-1)
    refused(name, "null pointer", cov=None)                                        # required with a motion flag ...
    refused(name, "null pointer", meas=None, flags=0)
    refused(name, "null pointer", out=None, flags=0)
    refused(name, "det_xyah is NULL", xyah=None, flags=1)
    refused(name, "det_xyah is NULL", xyah=None, flags=4 | 2)
    refused(name, "unknown flag bits", flags=8)
    refused(name, "unknown flag bits", flags=-1)
    refused(name, "exclude each other", flags=1 | 4)
    refused(name, "lambda is NaN", lam=float("nan"))
    refused(name, "misaligned", xyah=ODD)
    refused(name, "misaligned", score=ODD)
    refused(name, "misaligned", out=ODD)
    refused(name, "misaligned", status=0x10002)
    refused(name, "more workgroups than a grid holds", n=16 * 65535 + 1)
    # the message is the calling thread's own
    import threading
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.busca_track_last_error()))
    t.start()
    t.join()
    assert seen == [b""] and lib.busca_track_last_error() != b""


def test_python_level_checks():
    import torch
    from busca_amd import tracking
    from busca_amd.kalman_store import KalmanStore
    sys.path.insert(0, os.path.join(ROOT, "busca_amd", "compat"))
    import busca.tracking as alias
    assert tracking.KalmanStore is KalmanStore is alias.KalmanStore and KalmanStore.__module__ == "busca_amd.kalman_store"
    st = KalmanStore(CAP)
    assert st.capacity == CAP and st.dev == torch.device("cuda", 0) and st.mean is None      # nothing is allocated before the first use
    z = np.ones((4, 4))
    for call in (lambda s: st.predict(s), lambda s: st.initiate(s, z), lambda s: st.update(s, z), lambda s: st.boxes(s), lambda s: st.cost(s, []),
                 lambda s: st.round(s, [], 0.8), lambda s: st.load(s, [None] * len(s)), lambda s: st.store(s, [None] * len(s))):
        with pytest.raises(ValueError, match="distinct"):
            call([3, 1, 3])
        with pytest.raises(ValueError, match="beyond the capacity"):
            call([0, CAP])
    with pytest.raises(ValueError):
        KalmanStore(-1)


def test_fixture_is_what_the_issue_asks_for():
    s = script()
    assert os.path.getsize(GOLD) < 100 << 10
    assert s["mean"].shape == (16, 3, CAP, 8) and s["cov"].shape == (16, 3, CAP, 8, 8) and s["meas"].shape == (16, 8, 4)
    assert [f + 1 for f in range(16) if s["ini_n"][f]] == [1, 3, 9, 10]
    assert s["meas_m"][12] == 0 and (s["pred_slot"][13] == -1).sum() == 1 and (s["upd_slot"][13] == -1).sum() == 1
    assert s["pred_nt"][5:9].sum() == 4 and s["mean"][5, 0, 7, 7] == 0.0


@pytest.mark.skipif(not os.path.exists(REFERENCE), reason="the reference tree is not on this machine")
def test_generator_reproduces_the_fixture():
    gen = _generator()
    made, s = gen.make(gen.load_kalman()), script()
    assert sorted(made) == sorted(s)
    for k in s:
        assert made[k].dtype == s[k].dtype and made[k].shape == s[k].shape and made[k].tobytes() == s[k].tobytes(), k


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from busca_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def busy():
    from tests.test_streams_gpu import Busy
    b = Busy()
    yield b
    b.report()


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))
    return t if dtype is None else t.to(dtype)


def _store(capacity, mean=None, cov=None, slots=None):
    """A KalmanStore; the states mean[i] / cov[i] in slot slots[i] (None: slot i), zeros elsewhere."""
    from busca_amd.kalman_store import KalmanStore
    st = KalmanStore(capacity)
    st._state()
    if mean is not None:
        rows = _dev(np.arange(len(mean)) if slots is None else np.asarray(slots)).long()
        st.mean[rows] = _dev(mean)
        st.cov[rows] = _dev(cov)
    return st


def _state_of(st):
    return st.mean.cpu().numpy(), st.cov.cpu().numpy()


def _untouched(before, after, listed, what):
    keep = np.ones(len(before[0]), dtype=bool)
    keep[[s for s in listed if s >= 0]] = False
    assert np.array_equal(before[0][keep], after[0][keep]) and np.array_equal(before[1][keep], after[1][keep]), what


def _run_frame(st, f, on_phase=None):
    """Frame f of the script through the store; on_phase(phase, listed slots, state before, state after)."""
    s = script()
    meas = s["meas"][f - 1, :int(s["meas_m"][f - 1])]
    slots, nt = phase(f, "pred_slot", "pred_n", "pred_nt")
    before = _state_of(st) if on_phase else None
    st.predict(slots, nt)
    if on_phase:
        on_phase(0, slots, before, _state_of(st))
    slots, det = phase(f, "upd_slot", "upd_n", "upd_det")
    before = _state_of(st) if on_phase else None
    status = st.update(slots, meas, det)
    if on_phase:
        assert not status.cpu().numpy().any()
        on_phase(1, slots, before, _state_of(st))
    slots, det = phase(f, "ini_slot", "ini_n", "ini_det")
    before = _state_of(st) if on_phase else None
    st.initiate(slots, meas, det)
    if on_phase:
        on_phase(2, slots, before, _state_of(st))


def _near(got, want, what):
    """Updated states against the reference: the chain bars; states no update has touched since: equal."""
    _, bar = bars()
    em, ec = err_mean(got[0], want[0]), err_cov_safe(got[1], want[1])
    assert em <= bar["chain_mean"] and ec <= bar["chain_cov"], (what, em, ec, bar["chain_mean"], bar["chain_cov"])
    return em, ec


def err_cov_safe(got, ref):
    """err_cov over the slots that hold a state (an empty slot's covariance is all zero on both sides, which err_cov would divide by)."""
    used = np.abs(ref).reshape(len(ref), -1).max(1) > 0
    assert np.array_equal(got[~used], ref[~used])
    return err_cov(got[used], ref[used]) if used.any() else 0.0


@pytest.mark.gpu
def test_the_script_replays_to_the_fixture():
    s = script()
    st = _store(CAP)
    worst = [0.0, 0.0]
    exact = {"ok": True}                                   # until the first update, and in slots no update has reached, the replay is exact

    def check(f):
        def on_phase(ph, listed, before, after):
            want = (s["mean"][f - 1, ph], s["cov"][f - 1, ph])
            _untouched(before, after, listed, (f, ph))
            got = (after[0][:CAP], after[1][:CAP])
            em, ec = _near(got, want, (f, ph))
            worst[0], worst[1] = max(worst[0], em), max(worst[1], ec)
            live = [x for x in listed if x >= 0]
            if ph == 2:                                    # an initiated state is the reference's, bit for bit
                assert np.array_equal(got[0][live], want[0][live]) and np.array_equal(got[1][live], want[1][live]), (f, "initiate")
            if ph == 0:                                    # a prediction is bit-exact given its input: predict the REFERENCE's previous state
                prev = (s["mean"][f - 2, 2], s["cov"][f - 2, 2]) if f > 1 else (np.zeros((CAP, 8)), np.zeros((CAP, 8, 8)))
                ref_in = _store(CAP, prev[0], prev[1])
                ref_in.predict(*phase(f, "pred_slot", "pred_n", "pred_nt"))
                m, c = _state_of(ref_in)
                assert np.array_equal(m[:CAP], want[0]) and np.array_equal(c[:CAP], want[1]), (f, "predict")
            if np.any(after[0][CAP] != 0) or np.any(after[1][CAP] != 0):
                exact["ok"] = False
        return on_phase
    for f in range(1, 17):
        _run_frame(st, f, check(f))
    assert exact["ok"], "the spare slot was written"
    print("replay: worst mean error %.3g, covariance %.3g (bars %.3g, %.3g)" % (worst[0], worst[1], bars()[1]["chain_mean"], bars()[1]["chain_cov"]))


PERM = np.random.RandomState(3).permutation(128)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 96])
def test_bit_equal_to_the_list_ordered_kernels(ctx, n):
    import torch
    from busca_amd._xfer import stream_of
    g = gold()
    slots = PERM[:96]
    st = _store(128, g["mean"], g["cov"], slots)
    listed = slots[:n][::-1].copy()                        # the gathered order: the listed tracks, last first
    src = np.arange(96)[:n][::-1].copy()
    stream = stream_of(ctx)
    nt = (np.arange(n) % 3 == 0).astype(np.uint8)
    # predict
    m, c = _dev(g["mean"][src].reshape(-1, 8)), _dev(g["cov"][src].reshape(-1, 8, 8))
    ctx.check(ctx.lib.busca_kalman_multi_predict(ctx.h, m.data_ptr(), c.data_ptr(), _dev(nt).data_ptr() if n else None, n, stream))
    before = _state_of(st)
    st.predict(listed, nt)
    after = _state_of(st)
    _untouched(before, after, listed, "predict")
    assert np.array_equal(after[0][listed], m.cpu().numpy()) and np.array_equal(after[1][listed], c.cpu().numpy())
    # boxes
    for tlbr in (0, 1):
        out = torch.empty(n, 4, dtype=torch.float64, device=m.device)
        ctx.check(ctx.lib.busca_kalman_boxes(ctx.h, m.data_ptr(), n, tlbr, out.data_ptr(), stream))
        assert np.array_equal(st.boxes(listed, tlbr=bool(tlbr)).cpu().numpy(), out.cpu().numpy())
    # update with a det_index that is no identity, more measurements than tracks
    det = ((np.arange(n) * 37 + 5) % 96).astype(np.int32)
    status = torch.full((n,), -7, dtype=torch.int32, device=m.device)
    ctx.check(ctx.lib.busca_kalman_update(ctx.h, m.data_ptr(), c.data_ptr(), _dev(g["meas"][det].reshape(-1, 4)).data_ptr(), n, status.data_ptr(), stream))
    before = after
    got_status = st.update(listed, g["meas"], det)
    after = _state_of(st)
    _untouched(before, after, listed, "update")
    assert np.array_equal(after[0][listed], m.cpu().numpy()) and np.array_equal(after[1][listed], c.cpu().numpy())
    assert np.array_equal(got_status.cpu().numpy(), status.cpu().numpy()) and not status.cpu().numpy().any()
    # initiate
    det = ((np.arange(n) * 11 + 3) % 64).astype(np.int32)
    ctx.check(ctx.lib.busca_kalman_initiate(ctx.h, _dev(g["init_meas"][det].reshape(-1, 4)).data_ptr(), n, m.data_ptr(), c.data_ptr(), stream))
    before = after
    st.initiate(listed, g["init_meas"], det)
    after = _state_of(st)
    _untouched(before, after, listed, "initiate")
    assert np.array_equal(after[0][listed], m.cpu().numpy()) and np.array_equal(after[1][listed], c.cpu().numpy())
    if n:
        assert np.array_equal(after[0][listed], g["init_mean"][det]) and np.array_equal(after[1][listed], g["init_cov"][det])


def _parent_cost(ctx, tracks, dets, scores, mode, only_position, lam):
    """The cost matrix and status words of the list-ordered chain: prediction, boxes, pairwise, gating, torch.where and the blend."""
    import torch
    from busca_amd import kalman
    fuse = mode == "fuse"
    mean, cov, cost, status = kalman._predicted_cost_dev(ctx, tracks, dets, scores, fuse, only_position, lam)
    if mode == "gate":
        gate, status = kalman._gating_dev(ctx, mean, cov, torch.from_numpy(kalman._measurements(dets)).to(mean.device), only_position, 0)
        cost = kalman._gate_dev(cost, gate, only_position, None)
    st = np.zeros(len(tracks), dtype=np.int32) if status is None else status.cpu().numpy()
    return mean.cpu().numpy(), cov.cpu().numpy(), cost.cpu().numpy(), st


MODES = [("iou", False), ("fuse", False), ("fuse", True), ("gate", False), ("gate", True)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(1, 1), (15, 63), (16, 64), (17, 65), (96, 40)])
def test_round_cost_equals_the_five_launch_chain(ctx, n, m):
    g = gold()
    cols = np.arange(m) % 40
    # detections scattered around the tracks, so that entries fall on both sides of the gate
    scores = 0.3 + 0.7 * ((np.arange(m) * 7 % 10) / 10.0)
    dets = _detections(g["gate_meas"][cols])
    slots = PERM[:n]
    states = (np.arange(n) % 4 != 1).astype(int)          # TrackState: 1 Tracked, else not
    gated = 0
    for mode, only_position in MODES:
        for sc in (None, scores):
            tracks = _tracks(g["mean"][:n], g["cov"][:n], states)
            pm, pc, want, want_status = _parent_cost(ctx, tracks, dets, sc, mode, only_position, 0.98)
            st = _store(128, g["mean"][:n], g["cov"][:n], slots)
            st.predict(slots, states != 1)
            got_m, got_c = _state_of(st)
            assert np.array_equal(got_m[slots], pm) and np.array_equal(got_c[slots], pc)
            cost, status = st.cost(slots, dets, sc, fuse_motion=mode == "fuse", only_position=only_position, lambda_=0.98, gate_only=mode == "gate")
            cost, status = cost.cpu().numpy(), status.cpu().numpy()
            assert cost.shape == (n, m) and np.array_equal(cost, want, equal_nan=True) and np.array_equal(status, want_status), (mode, only_position)
            gated += int(np.isinf(want).sum())
            # a listed -1: a row of +inf, the other rows as they were
            if mode == "fuse" and sc is not None:
                with_hole = np.insert(slots, n // 2, -1)
                c2, s2 = st.cost(with_hole, dets, sc, fuse_motion=True, only_position=only_position)
                c2, s2 = c2.cpu().numpy(), s2.cpu().numpy()
                assert np.isposinf(c2[n // 2]).all() and s2[n // 2] == 0
                assert np.array_equal(np.delete(c2, n // 2, 0), want, equal_nan=True) and np.array_equal(np.delete(s2, n // 2), want_status)
    if (n, m) == (96, 40):
        assert gated > 100                                 # the gate did close somewhere


@pytest.mark.gpu
def test_round_cost_of_nothing_launches_nothing():
    g = gold()
    st = _store(8, g["mean"][:8], g["cov"][:8])
    c, s = st.cost([], _detections(g["gate_meas"][:3]))
    assert c.shape == (0, 3) and s.shape == (0,)
    c, s = st.cost([2, 1], [], fuse_motion=True)
    assert c.shape == (2, 0) and s.cpu().numpy().tolist() == [0, 0]
    assert st.round([], _detections(g["gate_meas"][:3]), 0.8)[1:] == ((), (0, 1, 2))
    assert st.round([2, 1], [], 0.8)[1:] == ((0, 1), ())


@pytest.mark.gpu
def test_not_positive_definite(ctx):
    g = gold()
    _, bar = bars()
    idx = [4, 5, 6]
    mean, cov, meas = g["mean"][idx].copy(), g["cov"][idx].copy(), g["meas"][idx].copy()
    cov[1, :4, :4] = -np.eye(4)
    slots = [9, 2, 5]
    st = _store(CAP, mean, cov, slots)
    status = st.update(slots, meas).cpu().numpy()
    m, c = _state_of(st)
    assert status.tolist() == [0, 1, 0]
    assert np.array_equal(m[2], mean[1]) and np.array_equal(c[2], cov[1])                      # untouched
    assert err_mean(m[[9, 5]], g["upd_mean"][[4, 6]]) <= bar["mean"] and err_cov(c[[9, 5]], g["upd_cov"][[4, 6]]) <= bar["cov"]
    st = _store(CAP, mean, cov, slots)
    dets = _detections(g["gate_meas"])
    cost, status = st.cost(slots, dets, fuse_motion=True)
    cost = cost.cpu().numpy()
    assert status.cpu().numpy().tolist() == [0, 1, 0] and np.isnan(cost[1]).all() and not np.isnan(cost[[0, 2]]).any()
    with pytest.raises(np.linalg.LinAlgError, match="track 1"):
        st.round(slots, dets, 0.8, fuse_motion=True, predict=False)
    assert st.round(slots, dets, 0.8, predict=False)[0].shape[1] == 2                          # without the gate nothing is factored


@pytest.mark.gpu
@pytest.mark.parametrize("fuse_motion", [False, True])
def test_round_equals_associate_round(ctx, fuse_motion):
    from busca_amd import tracking
    g = gold()
    n, m = 96, 40
    scores = 0.3 + 0.7 * ((np.arange(m) * 7 % 10) / 10.0)
    dets = _detections(g["gate_meas"])
    states = (np.arange(n) % 5 != 2).astype(int)
    tracks = _tracks(g["mean"], g["cov"], states)
    want = tracking.associate_round(tracks, dets, 0.8, det_scores=scores, fuse_motion=fuse_motion, ctx=ctx)
    slots = PERM[:n]
    st = _store(128, g["mean"], g["cov"], slots)
    got = st.round(slots, dets, 0.8, det_scores=scores, fuse_motion=fuse_motion, not_tracked=states != 1)
    assert len(want[0]) >= 10
    for a, b in zip(got, want):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    gm, gc = _state_of(st)
    assert np.array_equal(gm[slots], np.stack([t.mean for t in tracks])) and np.array_equal(gc[slots], np.stack([t.covariance for t in tracks]))


@pytest.mark.gpu
def test_slots_outside_the_store_touch_nothing():
    import torch
    from busca_amd.kalman_store import KalmanStore
    g = gold()
    S, GUARD, CANARY = 8, 6, 777.25
    mean_buf = torch.full((S + 1 + GUARD, 8), CANARY, dtype=torch.float64, device="cuda:0")
    cov_buf = torch.full((S + 1 + GUARD, 8, 8), CANARY, dtype=torch.float64, device="cuda:0")
    st = KalmanStore(S)
    st.mean, st.cov = mean_buf[:S + 1], cov_buf[:S + 1]
    st.mean[:S], st.cov[:S] = _dev(g["mean"][:S]), _dev(g["cov"][:S])
    slot = _dev(np.array([S, 3, S + 1, 2 ** 31 - 1, -5, S + GUARD - 1, -2 ** 31], dtype=np.int32))      # one entry inside the store
    meas = g["meas"][:7]
    before = (mean_buf.cpu().numpy(), cov_buf.cpu().numpy())

    def only_slot_3_changed(what):
        after = (mean_buf.cpu().numpy(), cov_buf.cpu().numpy())
        keep = np.arange(S + 1 + GUARD) != 3
        assert np.array_equal(after[0][keep], before[0][keep]) and np.array_equal(after[1][keep], before[1][keep]), what
        assert not np.array_equal(after[1][3], before[1][3]), what
        assert (after[0][S:] == CANARY).all() and (after[1][S:] == CANARY).all(), what
    st.predict(slot, np.ones(7, dtype=bool))
    only_slot_3_changed("predict")
    assert st.update(slot, meas).cpu().numpy().tolist() == [0] * 7
    only_slot_3_changed("update")
    box = st.boxes(slot).cpu().numpy()
    assert np.isnan(box[[0, 2, 3, 4, 5, 6]]).all() and np.isfinite(box[1]).all()
    cost, status = st.cost(slot, _detections(g["gate_meas"]), fuse_motion=True)
    cost = cost.cpu().numpy()
    assert np.isposinf(cost[[0, 2, 3, 4, 5, 6]]).all() and not np.isnan(cost[1]).any() and not status.cpu().numpy().any()
    # a detection index outside the measurements skips the pair
    st.initiate(slot, meas, _dev(np.array([0, 7, 1, 2, 3, 4, 5], dtype=np.int32)))
    after = mean_buf.cpu().numpy()
    st.initiate(slot, meas, _dev(np.array([0, -1, 1, 2, 3, 4, 5], dtype=np.int32)))
    assert np.array_equal(mean_buf.cpu().numpy(), after)
    st.initiate(slot, meas)
    only_slot_3_changed("initiate")
    assert np.array_equal(mean_buf.cpu().numpy()[3, :4], meas[1])


@pytest.mark.gpu
def test_frame_10_behind_a_busy_stream(ctx, busy):
    from busca_amd.kalman_store import KalmanStore
    from tests.test_streams_gpu import behind
    s = script()
    f = 10
    pad = lambda a: np.concatenate([a, np.zeros_like(a[:1])])                                  # noqa: E731  (the spare slot)
    true = [_dev(pad(s["mean"][f - 2, 2])), _dev(pad(s["cov"][f - 2, 2]))]
    poison = [_dev(pad(s["mean"][4, 2])), _dev(pad(s["cov"][4, 2]))]                        # the states of frame 5: other tracks in other places
    meas = s["meas"][f - 1, :int(s["meas_m"][f - 1])]
    dets = _detections(meas)
    slots = phase(f, "upd_slot", "upd_n")[0]
    st = KalmanStore(CAP)

    def call(x, outs, stream):
        st.mean, st.cov = x
        _run_frame(st, f)
        return st.round(slots, dets, 0.8, det_scores=np.linspace(0.5, 1.0, len(dets)), fuse_motion=True, predict=False)
    want, got = behind(busy, "KalmanStore frame 10", call, true=true, poison=poison, form="current", host=True)
    assert len(got[2]) >= 4                                                                   # the round matched the tracks it had just updated
    state = (got[0][:CAP], got[1][:CAP])
    _near(state, (s["mean"][f - 1, 2], s["cov"][f - 1, 2]), "frame 10")
    new = phase(f, "ini_slot", "ini_n")[0]
    assert np.array_equal(state[0][new], s["mean"][f - 1, 2][new]) and np.array_equal(state[1][new], s["cov"][f - 1, 2][new])


@pytest.mark.gpu
def test_load_store_and_a_frame_on_both_routes(ctx):
    from busca_amd import tracking
    s = script()
    g = gold()
    # round trip
    slots = [11, 0, 6, 3]
    objs = _tracks(g["mean"][:4], g["cov"][:4])
    st = _store(CAP)
    st.load(slots, objs)
    m, c = _state_of(st)
    assert np.array_equal(m[slots], g["mean"][:4]) and np.array_equal(c[slots], g["cov"][:4])
    assert not m[[i for i in range(CAP) if i not in slots]].any()
    back = [types.SimpleNamespace(mean=None, covariance=None) for _ in slots]
    st.store(slots[::-1], back)
    assert all(np.array_equal(b.mean, g["mean"][3 - i]) and np.array_equal(b.covariance, g["cov"][3 - i]) for i, b in enumerate(back))
    # frame 12: every track is updated; three of them as objects through multi_update, the others in the store
    f = 12
    start = (s["mean"][f - 2, 2], s["cov"][f - 2, 2])
    meas = s["meas"][f - 1, :int(s["meas_m"][f - 1])]
    all_store = _store(CAP, *start)
    _run_frame(all_store, f)
    mixed = _store(CAP, *start)
    mixed.predict(*phase(f, "pred_slot", "pred_n", "pred_nt"))
    slots, det = phase(f, "upd_slot", "upd_n", "upd_det")
    assert len(slots) == 6
    objs = [types.SimpleNamespace(mean=None, covariance=None, state=1) for _ in range(3)]
    mixed.store(slots[[0, 2, 4]], objs)
    tracking.multi_update(objs, meas[det[[0, 2, 4]]], ctx=ctx)
    mixed.load(slots[[0, 2, 4]], objs)
    assert not mixed.update(slots[[1, 3, 5]], meas, det[[1, 3, 5]]).cpu().numpy().any()
    a, b = _state_of(all_store), _state_of(mixed)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
