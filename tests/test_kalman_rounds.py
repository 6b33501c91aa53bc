"""The association rounds of many sequences in one launch: libbusca_rounds.so (include/busca_rounds.h), its binding busca_amd._rounds_lib and
KalmanStore.detections_batch / cost_batch / round_batch.

References, none of them the new kernel: busca_track_round_cost (KalmanStore.cost) and KalmanStore.round of each problem alone, which
tests/test_kalman_store.py pins to the list-ordered kernels and through them to the reference, and the committed script tests/golden/kalman_store.npz
replayed one sequence at a time.  Everything is compared with np.array_equal: the batched kernel runs the tile body of the single-problem kernel
on the same operands, so nothing may differ.  Shapes are the smallest that cross the 16-row / 64-column tile."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from tests.test_kalman_filter import _detections, gold
from tests.test_kalman_store import CAP, MODES, PERM, _run_frame, _state_of, _store, phase, script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["busca_rounds_cost", "busca_rounds_last_error", "busca_rounds_version"]
BATCHES = {
    "one": [(1, 1)],
    "ragged": [(15, 63), (16, 64), (17, 65), (0, 5), (5, 0), (33, 130), (1, 1)],      # 87 disjoint slots, N = 33, M = 130
    "shared": [(96, 40), (3, 2)],                                                      # the second problem: the first three slots of the first
}
HOLES = (2, 4, 11)                   # problem 2 of "ragged" lists no slot at rows 4 and 11
CANARY, GUARD = 777.25, 6


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    from busca_amd.build import build
    hip_lib = build()
    from busca_amd import _lib, _rounds_lib, _store_lib, _track_lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "busca_rounds.h")).read(), flags=re.S)
    declared = {}
    for name, args in re.findall(r"\b(busca_rounds_[a-z0-9_]+)\s*\((.*?)\)\s*;", hdr, flags=re.S):
        declared[name] = 0 if args.strip() == "void" else len(args.split(","))
    assert declared == {name: len(args) for name, (_, args) in _rounds_lib.ROUNDS_API.items()}
    assert sorted(declared) == NAMES and declared["busca_rounds_cost"] == 19

    def exported(path):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    ours = exported(_rounds_lib.ROUNDS_LIB_PATH)
    assert {n for n in ours if not n.startswith("_")} == set(NAMES)
    assert os.path.basename(hip_lib) == "libbusca_hip.so"
    for other in (hip_lib, _track_lib.TRACK_LIB_PATH, _store_lib.STORE_LIB_PATH):
        assert not [n for n in exported(other) if n.startswith("busca_rounds")], other
    theirs = {k for t in _lib.HEADERS.values() for k in t} | set(_track_lib.TRACK_API) | set(_store_lib.STORE_API)
    assert not ours & theirs
    assert "busca_rounds.h" not in _lib.HEADERS and "_rounds_lib" not in open(_lib.__file__.replace(".pyc", ".py")).read()
    lib = _rounds_lib.load()
    assert lib.busca_rounds_version() == 1000 and _rounds_lib.ABI_MAJOR == 1 and lib.busca_rounds_last_error() is not None


def test_refusals_and_noops_need_no_gpu():
    """Every argument is checked before the first HIP call: the pointers below are never followed."""
    from busca_amd import _rounds_lib
    lib = _rounds_lib.load()
    P, ODD, ODD4 = 0x10000, 0x10004, 0x10002              # an aligned address, one 4- but not 8-byte aligned, one not 4-byte aligned
    name = "busca_rounds_cost"

    def call(mean=P, cov=P, S=8, slot=P, n=3, tlbr=P, xyah=P, score=None, m=5, problems=P, batch=2, N=3, M=5, flags=1, lam=0.98, out=P, status=P, dev=0):
        return lib.busca_rounds_cost(mean, cov, S, slot, n, tlbr, xyah, score, m, problems, batch, N, M, flags, lam, out, status, dev, None)

    def refused(words, **kw):
        rc = call(**kw)
        msg = lib.busca_rounds_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":") and words in msg, (kw, rc, msg)

    # the no-ops: nothing is launched, so nothing else is looked at
    for kw in (dict(batch=0), dict(N=0), dict(M=0), dict(n=0), dict(m=0)):
        assert call(**kw) == 0, kw
        assert call(mean=None, cov=None, slot=None, tlbr=None, xyah=None, problems=None, out=None, status=None, **kw) == 0, kw
    # what busca_track_round_cost refuses
    for kw in (dict(n=-1), dict(S=-1), dict(m=-1), dict(batch=-1), dict(N=-1), dict(M=-1)):
        refused("negative size", **kw)
    refused("negative device", dev=-1)
    refused("null pointer", mean=None)
    refused("null pointer", slot=None)
    refused("null pointer", cov=None)                     # required with a motion flag ...
    refused("null pointer", tlbr=None, flags=0)
    refused("null pointer", out=None, flags=0)
    refused("det_xyah is NULL", xyah=None, flags=1)
    refused("det_xyah is NULL", xyah=None, flags=4 | 2)
    refused("unknown flag bits", flags=8)
    refused("unknown flag bits", flags=-1)
    refused("exclude each other", flags=1 | 4)
    refused("lambda is NaN", lam=float("nan"))
    for kw in (dict(mean=ODD), dict(cov=ODD), dict(tlbr=ODD), dict(xyah=ODD), dict(score=ODD), dict(out=ODD), dict(slot=ODD4), dict(status=ODD4)):
        refused("misaligned", **kw)
    # and what the table and the slab add
    refused("null pointer (problems)", problems=None)
    refused("misaligned", problems=ODD4)
    refused("more than a grid holds (65535 at most)", batch=65536)
    refused("more workgroups than a grid holds", N=16 * 65535 + 1)
    # the message is the calling thread's own
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.busca_rounds_last_error()))
    t.start()
    t.join()
    assert seen == [b""] and lib.busca_rounds_last_error() != b""


def test_python_level_checks():
    from busca_amd import tracking
    from busca_amd.kalman_store import KalmanStore, RoundProblem
    assert tracking.RoundProblem is RoundProblem and tracking.KalmanStore is KalmanStore
    assert RoundProblem._fields == ("slots", "detections", "det_scores", "not_tracked") and RoundProblem([1], [])[2:] == (None, None)
    g = gold()
    dets = _detections(g["gate_meas"][:3])
    st = KalmanStore(CAP)
    assert st.round_batch([], 0.8) == []
    with pytest.raises(ValueError, match="for all problems or for none"):
        st.detections_batch([dets, dets], [np.ones(3), None])
    with pytest.raises(ValueError, match="for all problems or for none"):
        st.round_batch([RoundProblem([0, 1], dets, np.ones(3)), RoundProblem([2], dets)], 0.8)
    with pytest.raises(ValueError, match="for all problems or for none"):
        st.cost_batch([([0, 1], dets), ([2], dets, np.ones(3))])
    with pytest.raises(ValueError, match="distinct across the whole batch"):
        st.round_batch([RoundProblem([0, 1], dets), RoundProblem([2, 1], dets)], 0.8)
    with pytest.raises(ValueError, match="distinct across the whole batch"):
        st.round_batch([([0, 1], dets), ([-1, 2], dets), ([-1, 0], dets)], 0.8, predict=True)
    # within one problem the slots are checked as round() checks them, with or without the prediction
    for predict in (True, False):
        with pytest.raises(ValueError, match="problem 1: the slots of one call must be distinct"):
            st.round_batch([([0, 1], dets), ([2, 2], dets)], 0.8, predict=predict)
        with pytest.raises(ValueError, match="beyond the capacity"):
            st.round_batch([([0, CAP], dets)], 0.8, predict=predict)
    with pytest.raises(ValueError, match="`not_tracked` flags for 2 slots"):
        st.round_batch([RoundProblem([0, 1], dets, None, [True])], 0.8)
    assert st.mean is None                                 # nothing was allocated on the way to any of these


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def busy():
    from tests.test_streams_gpu import Busy
    b = Busy()
    yield b
    b.report()


def _filled():
    """A 128-slot store holding gold()'s 96 states at PERM[:96]."""
    g = gold()
    return _store(128, g["mean"], g["cov"], PERM[:96])


@pytest.fixture(scope="module")
def predicted():
    """_filled() after predict, every fourth track not Tracked: the states test_round_cost_equals_the_five_launch_chain has at (96, 40).  Read-only."""
    st = _filled()
    st.predict(PERM[:96], np.arange(96) % 4 == 1)
    return st


def _batch(name, scores, hole=None):
    """[(slots, detections, scores)] of a batch: consecutive pieces of PERM[:96], problem k's detections gate_meas[(arange(m_k) + 7 k) % 40].
    `hole`: what stands at the two HOLES of "ragged" (rows without a slot)."""
    g = gold()
    out, at = [], 0
    for k, (n, m) in enumerate(BATCHES[name]):
        if name == "shared" and k == 1:
            slots = PERM[:3].astype(np.int64)
        else:
            slots, at = PERM[at:at + n].astype(np.int64), at + n
        if name == "ragged" and k == HOLES[0] and hole is not None:
            slots[list(HOLES[1:])] = hole
        sc = 0.3 + 0.7 * (((np.arange(m) + k) * 7 % 10) / 10.0) if scores else None
        out.append((slots, _detections(g["gate_meas"][(np.arange(m) + 7 * k) % 40]), sc))
    return out


def _kw(mode, only_position):
    return dict(fuse_motion=mode == "fuse", only_position=only_position, lambda_=0.98, gate_only=mode == "gate")


def _flag_word(mode, only_position):
    return {"iou": 0, "fuse": 1, "gate": 4}[mode] | (2 if only_position and mode != "iou" else 0)


def _dev_i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to("cuda:0")


def _reference(st, problems, mode, only_position):
    """[(cost [n_k, m_k], status [n_k])] of busca_track_round_cost, one problem at a time; the slot lists go as device tensors (not checked)."""
    want = []
    for slots, dets, sc in problems:
        c, s = st.cost(_dev_i32(slots), dets, sc, **_kw(mode, only_position))
        want.append((c.cpu().numpy(), s.cpu().numpy()))
    return want


def _raw(st, problems, flags, rows=None, N=None, M=None):
    """busca_rounds_cost itself on a slab and a status vector filled with canaries, GUARD rows of canary behind the slab
    -> (slab [B, N, M], guard, status [n_total], the table's rows)."""
    import torch
    from busca_amd import _rounds_lib
    from busca_amd._xfer import stream_of
    det, dbegin = st.detections_batch([p[1] for p in problems], [p[2] for p in problems])
    slot = np.concatenate([p[0] for p in problems])
    sbegin = np.concatenate([[0], np.cumsum([len(p[0]) for p in problems])])
    if rows is None:
        rows = np.stack([sbegin[:-1], np.diff(sbegin), dbegin[:-1], np.diff(dbegin)], 1)
    B = len(problems)
    N, M = N or int(np.diff(sbegin).max()), M or int(np.diff(dbegin).max())
    buf = torch.full((B * N * M + GUARD * M,), CANARY, dtype=torch.float64, device="cuda:0")
    status = torch.full((len(slot),), -7, dtype=torch.int32, device="cuda:0")
    slot_dev, rows_dev = _dev_i32(slot), _dev_i32(rows)
    _rounds_lib.check(_rounds_lib.load().busca_rounds_cost(
        st.mean.data_ptr(), st.cov.data_ptr(), st.capacity, slot_dev.data_ptr(), len(slot), det.tlbr.data_ptr(), det.xyah.data_ptr(),
        None if det.score is None else det.score.data_ptr(), det.m, rows_dev.data_ptr(), B, N, M, flags, 0.98, buf.data_ptr(), status.data_ptr(), 0,
        stream_of(st.dev)))
    host = buf.cpu().numpy()
    return host[:B * N * M].reshape(B, N, M), host[B * N * M:], status.cpu().numpy(), np.asarray(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_cost_batch_equals_round_cost_of_each_problem(predicted, name):
    st = predicted
    shapes = BATCHES[name]
    begin = np.concatenate([[0], np.cumsum([n for n, _ in shapes])])
    gated = finite = 0
    for mode, only_position in MODES:
        for scores in (False, True):
            # the C call: a -1 and an entry >= S in one problem of "ragged"; the Python call, whose host lists may not leave the capacity: two -1
            probs = _batch(name, scores, hole=np.array([-1, 128 + 5]))
            want = _reference(st, probs, mode, only_position)
            slab, _, status, _ = _raw(st, probs, _flag_word(mode, only_position))
            cost, dims, pstatus = st.cost_batch(_batch(name, scores, hole=-1), **_kw(mode, only_position))
            cost, pstatus = cost.cpu().numpy(), pstatus.cpu().numpy()
            assert dims.tolist() == [list(s) for s in shapes] and cost.shape == slab.shape == (len(shapes), max(n for n, _ in shapes), max(m for _, m in shapes))
            for k, (n, m) in enumerate(shapes):
                what = (name, mode, only_position, scores, k)
                assert want[k][0].shape == (n, m)
                assert np.array_equal(slab[k, :n, :m], want[k][0], equal_nan=True) and np.array_equal(cost[k, :n, :m], want[k][0], equal_nan=True), what
                if m:                                     # without a column there is no tile to write the status words
                    assert np.array_equal(status[begin[k]:begin[k + 1]], want[k][1]) and np.array_equal(pstatus[begin[k]:begin[k + 1]], want[k][1]), what
                else:
                    assert (status[begin[k]:begin[k + 1]] == -7).all() and not pstatus[begin[k]:begin[k + 1]].any(), what
            if name == "ragged":
                k, rows = HOLES[0], list(HOLES[1:])
                assert np.isposinf(slab[k, rows, :65]).all() and not status[begin[k]:begin[k + 1]][rows].any()
                assert np.isposinf(cost[k, rows, :65]).all() and not pstatus[begin[k]:begin[k + 1]][rows].any()
            if name == "shared":
                if mode == "iou":
                    finite += int(np.isfinite(want[0][0]).all())
                else:
                    gated += int(np.isinf(want[0][0]).sum())
                    assert np.isfinite(want[0][0]).any()
    if name == "shared":
        assert gated > 100 and finite == 2                 # the gate closed somewhere, and only the gate made an entry infinite


@pytest.mark.gpu
def test_nothing_else_is_written(predicted):
    st = predicted
    shapes = BATCHES["ragged"]
    probs = _batch("ragged", True, hole=np.array([-1, 128 + 5]))
    before = _state_of(st)
    slab, guard, status, rows = _raw(st, probs, 1)
    valid = np.zeros(slab.shape, dtype=bool)
    for k, (n, m) in enumerate(shapes):
        valid[k, :n, :m] = True
    assert (slab[~valid] == CANARY).all() and (guard == CANARY).all() and len(guard) == GUARD * 130
    assert not (slab[valid] == CANARY).any()
    assert (status[48:53] == -7).all() and not np.delete(status, np.arange(48, 53)).any()      # the (5, 0) problem has no tile
    after = _state_of(st)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # a row the table should not hold skips its problem; the others come out as before
    k = 5
    outside, too_tall = rows.copy(), rows.copy()
    outside[k, 0] = 87 - 32                                # 33 rows from there leave the slot list by one
    too_tall[k, :2] = 0, 34                                # inside the slot list, but more rows than the slab has
    for bad in (outside, too_tall):
        slab2, guard2, status2, _ = _raw(st, probs, 1, rows=bad, N=33, M=130)
        assert (slab2[k] == CANARY).all() and (guard2 == CANARY).all()
        assert np.array_equal(np.delete(slab2, k, 0), np.delete(slab, k, 0), equal_nan=True)
        theirs = np.arange(rows[k, 0], rows[k, 0] + rows[k, 1])
        assert (status2[theirs] == -7).all() and np.array_equal(np.delete(status2, theirs), np.delete(status, theirs))
    after = _state_of(st)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


@pytest.mark.gpu
def test_not_positive_definite():
    from busca_amd.kalman_store import RoundProblem
    g = gold()
    idx = [4, 5, 6, 7, 8, 9]
    mean, cov = g["mean"][idx].copy(), g["cov"][idx].copy()
    cov[3, :4, :4] = -np.eye(4)
    lists = [[9, 2], [5, 7, 11], [1]]                     # the states in list order: the bad one is track 1 of problem 1, position 3 of all
    st = _store(CAP, mean, cov, [s for ls in lists for s in ls])
    dets = _detections(g["gate_meas"])
    probs = [RoundProblem(ls, dets[3 * k:17 + k]) for k, ls in enumerate(lists)]
    plain, _, status = st.cost_batch(probs)
    assert not status.cpu().numpy().any()
    fused, dims, status = st.cost_batch(probs, fuse_motion=True)
    fused = fused.cpu().numpy()
    assert status.cpu().numpy().tolist() == [0, 0, 0, 1, 0, 0] and dims.tolist() == [[2, 17], [3, 15], [1, 13]]
    assert np.isnan(fused[1, 1, :15]).all() and not np.isnan(fused[1, [0, 2], :15]).any()
    assert not np.isnan(fused[0, :2, :17]).any() and not np.isnan(fused[2, :1, :13]).any()
    gate, _, status = st.cost_batch(probs, gate_only=True)
    gate, plain = gate.cpu().numpy(), plain.cpu().numpy()
    assert status.cpu().numpy().tolist() == [0, 0, 0, 1, 0, 0]
    assert np.array_equal(gate[1, 1, :15], plain[1, 1, :15]) and np.isfinite(gate[1, 1, :15]).all()      # a NaN distance passes no comparison
    before = _state_of(st)
    with pytest.raises(np.linalg.LinAlgError, match="problem 1: .* track 1 "):
        st.round_batch(probs, 0.8, fuse_motion=True, predict=False)
    after = _state_of(st)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    got = st.round_batch(probs, 0.8, predict=False)       # without the gate nothing is factored
    assert len(got) == 3 and all(g3[0].shape[1] == 2 for g3 in got)


def _same_triples(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x), np.asarray(y)) and np.asarray(x).shape == np.asarray(y).shape, (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("fuse_motion", [False, True])
@pytest.mark.parametrize("name", list(BATCHES))
def test_round_batch_equals_the_list_of_rounds(name, fuse_motion):
    from busca_amd.kalman_store import RoundProblem
    probs = _batch(name, True, hole=-1)
    predict = name != "shared"                             # problems that share slots cannot be predicted in one launch: predicted beforehand
    a, b = _filled(), _filled()
    if not predict:
        for st in (a, b):
            st.predict(PERM[:96], np.arange(96) % 5 == 2)
    nts = [None if k % 3 == 2 else (np.arange(len(p[0])) + k) % 5 == 2 for k, p in enumerate(probs)]      # some problems give no flags
    want = [b.round(p[0], p[1], 0.8, det_scores=p[2], fuse_motion=fuse_motion, not_tracked=nt, predict=predict) for p, nt in zip(probs, nts)]
    got = a.round_batch([RoundProblem(p[0], p[1], p[2], nt) for p, nt in zip(probs, nts)], 0.8, fuse_motion=fuse_motion, predict=predict)
    _same_triples(got, want, (name, fuse_motion))
    sa, sb = _state_of(a), _state_of(b)
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    if name == "shared":
        assert len(want[0][0]) >= 10                       # as test_round_equals_associate_round has it for these inputs
    if name == "ragged":
        assert want[3][1:] == ((), (0, 1, 2, 3, 4)) and want[4][1:] == ((0, 1, 2, 3, 4), ())      # the empty problems
    print("%s, fuse_motion %s: %s matches" % (name, fuse_motion, [len(w[0]) for w in want]))


@pytest.mark.gpu
def test_every_problem_empty_launches_nothing_after_the_predict():
    g = gold()
    a, b = _filled(), _filled()
    dets = _detections(g["gate_meas"][:3])
    got = a.round_batch([(PERM[:5], []), ([], dets), (PERM[5:7], [], None, [True, False])], 0.8)
    assert [t[1:] for t in got] == [((0, 1, 2, 3, 4), ()), ((), (0, 1, 2)), ((0, 1), ())]
    b.predict(PERM[:7], [False] * 5 + [True, False])
    sa, sb = _state_of(a), _state_of(b)
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    cost, dims, status = a.cost_batch([(PERM[:5], []), ([], dets)])
    assert cost.shape == (2, 5, 3) and dims.tolist() == [[5, 0], [0, 3]] and status.cpu().numpy().tolist() == [0] * 5


@pytest.mark.gpu
def test_lock_step_replay_of_the_golden_script():
    """Three sequences on slots [16 k, 16 k + 16) of one store, sequence k two frames behind sequence k - 1: every phase of a step is one call."""
    from busca_amd.kalman_store import RoundProblem
    s = script()
    st = _store(3 * CAP)
    refs = [_store(CAP) for _ in range(3)]
    matched = 0

    def shifted(slots, k):
        return np.where(slots >= 0, slots + CAP * k, slots)
    for t in range(1, 21):
        active = [(k, t - 2 * k) for k in range(3) if 1 <= t - 2 * k <= 16]
        meas = [s["meas"][f - 1, :int(s["meas_m"][f - 1])] for _, f in active]
        scores = [np.linspace(0.5, 1.0, len(z)) for z in meas]
        pred = [phase(f, "pred_slot", "pred_n", "pred_nt") for _, f in active]
        # the single-sequence replays, with round() on the states as the prediction leaves them
        want = []
        for (k, f), z, sc, (slots, _) in zip(active, meas, scores, pred):
            def on_phase(ph, listed, before, after, k=k, z=z, sc=sc, slots=slots):
                if ph == 0:
                    want.append(refs[k].round(slots, _detections(z), 0.8, det_scores=sc, fuse_motion=True, predict=False))
            _run_frame(refs[k], f, on_phase)
        # the same step for all active sequences at once
        st.predict(np.concatenate([shifted(p[0], k) for (k, _), p in zip(active, pred)]), np.concatenate([p[1] for p in pred]))
        got = st.round_batch([RoundProblem(shifted(p[0], k), _detections(z), sc) for (k, _), p, z, sc in zip(active, pred, meas, scores)], 0.8,
                             fuse_motion=True, predict=False)
        _same_triples(got, want, t)
        matched += sum(len(g3[0]) for g3 in got)
        det_all, begin = st.detections_batch(meas)
        assert det_all.tlbr is None and begin.tolist() == np.concatenate([[0], np.cumsum([len(z) for z in meas])]).tolist()
        for key in ("upd", "ini"):
            lists = [phase(f, key + "_slot", key + "_n", key + "_det") for _, f in active]
            slots = np.concatenate([shifted(ls[0], k) for (k, _), ls in zip(active, lists)])
            index = np.concatenate([ls[1] + begin[i] for i, ls in enumerate(lists)])
            if key == "upd":
                assert not st.update(slots, det_all, index).cpu().numpy().any()
            else:
                st.initiate(slots, det_all, index)
        mean, cov = _state_of(st)
        for k in range(3):
            rm, rc = _state_of(refs[k])
            assert np.array_equal(mean[CAP * k:CAP * (k + 1)], rm[:CAP]) and np.array_equal(cov[CAP * k:CAP * (k + 1)], rc[:CAP]), (t, k)
    # a track is initiated from its own measurement and measured on its path: the rounds do match (16 frames x 3 sequences)
    assert matched >= 3 * int(s["upd_n"].sum()) // 2, (matched, int(s["upd_n"].sum()))


@pytest.mark.gpu
def test_round_batch_behind_a_busy_stream(busy):
    from busca_amd.kalman_store import KalmanStore, RoundProblem
    from tests.test_kalman_store import _dev
    from tests.test_streams_gpu import behind
    s = script()
    f = 10
    pad = lambda a: np.concatenate([a, np.zeros_like(a[:1])])                                  # noqa: E731  (the spare slot)
    true = [_dev(pad(s["mean"][f - 2, 2])), _dev(pad(s["cov"][f - 2, 2]))]
    poison = [_dev(pad(s["mean"][4, 2])), _dev(pad(s["cov"][4, 2]))]                        # the states of frame 5: other tracks in other places
    meas = s["meas"][f - 1, :int(s["meas_m"][f - 1])]
    dets = _detections(meas)
    slots, nt = phase(f, "pred_slot", "pred_n", "pred_nt")
    half = len(slots) // 2
    assert half >= 2
    sc = np.linspace(0.5, 1.0, len(dets))
    probs = [RoundProblem(slots[:half], dets, sc, nt[:half]), RoundProblem(slots[half:], dets[::-1], sc[::-1].copy(), nt[half:])]
    st = KalmanStore(CAP)

    def call(x, outs, stream):
        st.mean, st.cov = x
        return st.round_batch(probs, 0.8, fuse_motion=True)
    want, got = behind(busy, "KalmanStore.round_batch", call, true=true, poison=poison, form="current", host=True)
    # x (mean, cov), then two triples: on the true states the tracks sit on their measurements, on the poison they do not
    assert len(got) == 8 and len(got[2]) + len(got[5]) >= 4, (len(got[2]), len(got[5]))
    ref = _store(CAP, s["mean"][f - 2, 2], s["cov"][f - 2, 2])
    ref.predict(slots, nt)
    rm, rc = _state_of(ref)
    assert np.array_equal(got[0], rm) and np.array_equal(got[1], rc)
