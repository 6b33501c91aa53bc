"""StrongSORT's track state resident on the device: libbusca_sort.so (include/busca_sort.h), its binding and busca_amd.sort_store.SortStore.

The float64 oracle is numpy or pure Python evaluated here: deep_sort/kalman_filter.py and iou_matching.py of upstream StrongSORT are not part of the
reference tree, so predict, the confidence-scaled update and iou_cost are restated below from the published code, and Track.camera_update from
adapters/StrongSORT/deep_sort/track.py:220-230.  What is compared how:
  * predict, initiate, boxes, iou_cost, camera_update: np.array_equal against the restatement.
  * update at confidence 0: np.array_equal against busca_track_kalman_update on the same store, which tests/test_kalman_store.py pins to the
    reference; at confidence > 0 against r_update_nsa (tests/test_kalman_filter.py's r_update with the (1 - c) factor) inside that module's
    bars - 20 x its restatement's own distance from the reference.
  * gate_cost: np.array_equal against the object route's chain (_upload_states, busca_kalman_gating, kalman._gate_dev, torch.where), and against
    the reference's gate_ref_mc0 / gate_ref_mc1 of tests/golden/appearance.npz with the tolerance of test_gate_cost_matrix_mc_against_the_reference.
  * the rounds: the matches of the object route."""
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests.test_kalman_filter import bars, err_cov, err_mean, gold, r_boxes, r_cholesky, r_initiate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 40
EPS = np.finfo(np.float64).eps
INFTY = 1e+5
CHI2_4 = 9.4877
PERM = np.random.RandomState(11).permutation(S)
F = np.eye(8)
F[np.arange(4), np.arange(4) + 4] = 1.0
_CACHE = {}


# ---- the restatement ----------------------------------------------------------------------------------------------------
def r_predict(mean, cov):
    """KalmanFilter.predict of upstream StrongSORT for one state, in numpy as upstream writes it."""
    wp, wv = 1.0 / 20, 1.0 / 160
    std_pos = [wp * mean[3], wp * mean[3], 1e-2, wp * mean[3]]
    std_vel = [wv * mean[3], wv * mean[3], 1e-5, wv * mean[3]]
    motion_cov = np.diag(np.square(np.r_[std_pos, std_vel]))
    return np.dot(F, mean), np.linalg.multi_dot((F, cov, F.T)) + motion_cov


def r_update_nsa(mean, cov, z, c):
    """KalmanFilter.update(mean, covariance, measurement, confidence): tests/test_kalman_filter.py's r_update with std = [(1 - c) * x for x in std]
    in the projection.  None where the reference raises LinAlgError."""
    h = float(mean[3])
    std = [(1.0 - c) * x for x in ((1.0 / 20) * h, (1.0 / 20) * h, 1e-1, (1.0 / 20) * h)]
    Sm = [[float(cov[i][j]) + (std[i] * std[i] if i == j else 0.0) for j in range(4)] for i in range(4)]
    L = r_cholesky(Sm, 4)
    if L is None:
        return None
    K = [[0.0] * 4 for _ in range(8)]
    for r in range(8):
        y, x = [0.0] * 4, [0.0] * 4
        for i in range(4):
            v = float(cov[r][i])
            for k in range(i):
                v = v - L[i][k] * y[k]
            y[i] = v / L[i][i]
        for i in (3, 2, 1, 0):
            v = y[i]
            for k in range(3, i, -1):
                v = v - L[k][i] * x[k]
            x[i] = v / L[i][i]
        K[r] = x
    inn = [float(z[i]) - float(mean[i]) for i in range(4)]
    new_mean = np.array([float(mean[i]) + (((inn[0] * K[i][0] + inn[1] * K[i][1]) + inn[2] * K[i][2]) + inn[3] * K[i][3]) for i in range(8)])
    KS = [[((K[i][0] * Sm[0][k] + K[i][1] * Sm[1][k]) + K[i][2] * Sm[2][k]) + K[i][3] * Sm[3][k] for k in range(4)] for i in range(8)]
    new_cov = np.array([[float(cov[i][j]) - (((KS[i][0] * K[j][0] + KS[i][1] * K[j][1]) + KS[i][2] * K[j][2]) + KS[i][3] * K[j][3])
                         for j in range(8)] for i in range(8)])
    return new_mean, new_cov


def r_iou_cost(tlwh, cand, stale=None, max_distance=None):
    """iou_matching.iou_cost of upstream StrongSORT on [n,4] track boxes and [m,4] candidates (tlwh), with min_cost_matching's clamp."""
    out = np.zeros((len(tlwh), len(cand)))
    for r, bbox in enumerate(tlwh):
        if stale is not None and stale[r]:
            out[r, :] = INFTY
            continue
        bbox_tl, bbox_br = bbox[:2], bbox[:2] + bbox[2:]
        cand_tl, cand_br = cand[:, :2], cand[:, :2] + cand[:, 2:]
        tl = np.c_[np.maximum(bbox_tl[0], cand_tl[:, 0])[:, np.newaxis], np.maximum(bbox_tl[1], cand_tl[:, 1])[:, np.newaxis]]
        br = np.c_[np.minimum(bbox_br[0], cand_br[:, 0])[:, np.newaxis], np.minimum(bbox_br[1], cand_br[:, 1])[:, np.newaxis]]
        wh = np.maximum(0., br - tl)
        inter = wh.prod(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[r, :] = 1. - inter / (bbox[2:].prod() + cand[:, 2:].prod(axis=1) - inter)
    if max_distance is not None:
        out[out > max_distance] = max_distance + 1e-5
    return out


def r_camera(mean, mat):
    """Track.camera_update of one state with the sums evaluated left to right in Python floats -> the new mean[:4]."""
    x1, y1, x2, y2 = (float(v) for v in r_boxes(np.asarray(mean, dtype=np.float64).reshape(1, 8), True)[0])
    m = [[float(v) for v in row] for row in mat]
    x1_, y1_ = (m[0][0] * x1 + m[0][1] * y1) + m[0][2], (m[1][0] * x1 + m[1][1] * y1) + m[1][2]
    x2_, y2_ = (m[0][0] * x2 + m[0][1] * y2) + m[0][2], (m[1][0] * x2 + m[1][1] * y2) + m[1][2]
    w, h = x2_ - x1_, y2_ - y1_
    return [x1_ + w / 2, y1_ + h / 2, w / h, h]


def r_camera_numpy(mean, mat):
    """track.py:220-230 as written, `matrix @ v` and all."""
    x1, y1, x2, y2 = r_boxes(np.asarray(mean, dtype=np.float64).reshape(1, 8), True)[0]
    x1_, y1_, _ = mat @ np.array([x1, y1, 1]).T
    x2_, y2_, _ = mat @ np.array([x2, y2, 1]).T
    w, h = x2_ - x1_, y2_ - y1_
    return [x1_ + w / 2, y1_ + h / 2, w / h, h]


def camera_bound(mean, mat):
    """How far two float64 evaluations of camera_update may lie apart, per entry of mean[:4].  A warped coordinate is two products and two sums;
    whatever the order or fusing, one evaluation is off by at most 3 roundings of u * (|m00 x| + |m01 y| + |m02|), two evaluations by twice that:
    3 eps * (...).  Sums and the quotient propagate to first order; each result adds one rounding per evaluation (eps of its magnitude for two)."""
    x1, y1, x2, y2 = (abs(float(v)) for v in r_boxes(np.asarray(mean, dtype=np.float64).reshape(1, 8), True)[0])
    a = np.abs(np.asarray(mat, dtype=np.float64))
    ex1, ey1 = 3 * EPS * (a[0, 0] * x1 + a[0, 1] * y1 + a[0, 2]), 3 * EPS * (a[1, 0] * x1 + a[1, 1] * y1 + a[1, 2])
    ex2, ey2 = 3 * EPS * (a[0, 0] * x2 + a[0, 1] * y2 + a[0, 2]), 3 * EPS * (a[1, 0] * x2 + a[1, 1] * y2 + a[1, 2])
    cx, cy, asp, h = (abs(v) for v in r_camera(mean, mat))
    w = asp * h
    dw, dh = ex1 + ex2 + EPS * w, ey1 + ey2 + EPS * h
    slack = 1.0 + 1e-9                                            # the second-order terms
    return [slack * (ex1 + dw / 2 + EPS * cx), slack * (ey1 + dh / 2 + EPS * cy), slack * (dw / h + w * dh / (h * h) + EPS * asp), dh]


def euclidean_warps():
    rs = np.random.RandomState(5)
    mats = []
    for _ in range(8):
        t, dx, dy = rs.uniform(-5e-3, 5e-3), rs.uniform(-20, 20), rs.uniform(-20, 20)
        mats.append(np.array([[math.cos(t), -math.sin(t), dx], [math.sin(t), math.cos(t), dy], [0.0, 0.0, 1.0]]))
    return mats


def states(steps):
    """(mean [24,8], cov [24,8,8]) after `steps` predict / update steps of the restated filter on the fixture's first 24 initiated states, or
    ("fixture") the fixture's first 24 tracked states; the covariances are not symmetric in their last bits from the first update on.  Built once
    per `steps`, never written."""
    key = ("states", steps)
    if steps == "fixture":                                         # the reference's own states of tests/golden/kalman.npz
        return gold()["mean"][:24], gold()["cov"][:24]
    if key not in _CACHE:
        g = gold()
        rs = np.random.RandomState(100 + steps)
        z0 = g["init_meas"][:24]
        mean, cov = r_initiate(z0)
        for s in range(steps):
            new = []
            for i in range(len(mean)):
                m, c = r_predict(mean[i], cov[i])
                z = m[:4] + rs.uniform(-1, 1, 4) * np.array([0.02 * m[3], 0.02 * m[3], 0.01, 0.02 * m[3]])
                new.append(r_update_nsa(m, c, z, [0.0, 0.35, 0.8, 0.999][(i + s) % 4]))
            mean, cov = np.stack([a for a, _ in new]), np.stack([b for _, b in new])
        mean.setflags(write=False)
        cov.setflags(write=False)
        _CACHE[key] = (mean, cov)
    return _CACHE[key]


def listed(n):
    """A slot list of n entries over the S = 40 store, permuted; from 16 entries on two of them are outside the store (-1 and S).
    -> (list int32 [n], the positions of its live entries)."""
    slots = PERM[:n].astype(np.int32).copy()
    if n >= 16:
        slots[2], slots[9] = -1, S
    return slots, np.nonzero((slots >= 0) & (slots < S))[0]


def detections_near(mean, m, seed):
    """[m,4] xyah measurements scattered around the states, so that gating distances fall on both sides of the gate."""
    rs = np.random.RandomState(seed)
    base = mean[rs.randint(0, len(mean), m), :4]
    h = base[:, 3:4]
    return base + rs.uniform(-1, 1, (m, 4)) * np.concatenate([0.15 * h, 0.15 * h, np.full_like(h, 0.3), 0.15 * h], 1)


def tlwh_of(xyah):
    out = np.array(xyah, dtype=np.float64).reshape(-1, 4)
    out[:, 2] *= out[:, 3]
    out[:, :2] -= out[:, 2:] / 2
    return out


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    from busca_amd.build import build
    hip_lib = build()
    from busca_amd import _lib, _sort_lib, _track_lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "busca_sort.h")).read(), flags=re.S)
    declared = {}
    for name, args in re.findall(r"\b(busca_sort_[a-z0-9_]+)\s*\((.*?)\)\s*;", hdr, flags=re.S):
        declared[name] = 0 if args.strip() == "void" else len(args.split(","))
    assert declared == {name: len(args) for name, (_, args) in _sort_lib.SORT_API.items()}
    assert len(declared) == 7
    for name, val in (("BUSCA_SORT_MC", _sort_lib.MC), ("BUSCA_SORT_CLAMP", _sort_lib.CLAMP)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name

    def exported(path):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    assert {n for n in exported(_sort_lib.SORT_LIB_PATH) if not n.startswith("_")} == set(_sort_lib.SORT_API)
    assert not [n for n in exported(hip_lib) | exported(_track_lib.TRACK_LIB_PATH) if n.startswith("busca_sort")]
    assert "busca_sort.h" not in _lib.HEADERS and len(_lib.HEADERS) == 7
    lib = _sort_lib.load()
    assert lib.busca_sort_version() == 1000 and lib.busca_sort_last_error() is not None
    assert _track_lib.load().busca_track_version() == 1000


def test_refusals_and_noops_need_no_gpu():
    """Every argument is checked before the first HIP call: the pointers below are never followed."""
    from busca_amd import _sort_lib
    lib = _sort_lib.load()
    P, ODD, n, m = 0x10000, 0x10004, 3, 5                 # an aligned address, one that is 4- but not 8-byte aligned
    nan = float("nan")

    def calls(mean=P, cov=P, S=8, slot=P, n=n, meas=P, det=P, m=m, conf=None, status=P, cost=P, ld=None, gated=1e5, flags=3, lam=0.98, maxd=0.3,
              out=P, stale=None, matrix=P, dev=0):
        ld = m if ld is None else ld
        return {
            "busca_sort_predict": lambda: lib.busca_sort_predict(mean, cov, S, slot, n, dev, None),
            "busca_sort_update": lambda: lib.busca_sort_update(mean, cov, S, slot, n, meas, det, m, conf, status, dev, None),
            "busca_sort_gate_cost": lambda: lib.busca_sort_gate_cost(mean, cov, S, slot, n, meas, m, cost, ld, gated, flags, lam, maxd, out, status, dev, None),
            "busca_sort_iou_cost": lambda: lib.busca_sort_iou_cost(mean, S, slot, n, stale, meas, m, flags & 2, maxd, out, dev, None),
            "busca_sort_camera_update": lambda: lib.busca_sort_camera_update(mean, S, slot, n, matrix, dev, None),
        }

    def refused(name, words, **kw):
        rc = calls(**kw)[name]()
        msg = lib.busca_sort_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":") and words in msg, (name, kw, rc, msg)

    for name in calls():
        assert calls(n=0)[name]() == 0, name                                       # the no-op
        assert calls(n=0, mean=None, cov=None, slot=None, out=None, cost=None, matrix=None)[name]() == 0, name
        refused(name, "null pointer", mean=None)
        refused(name, "null pointer", slot=None)
        refused(name, "negative size", n=-1)
        refused(name, "negative size", S=-1)
        refused(name, "negative device", dev=-1)
        refused(name, "misaligned", mean=ODD)
        refused(name, "misaligned", slot=0x10002)
    for name in ("busca_sort_predict", "busca_sort_update", "busca_sort_gate_cost"):
        refused(name, "null pointer", cov=None)
        refused(name, "misaligned", cov=ODD)
    name = "busca_sort_update"
    refused(name, "null pointer", meas=None)
    refused(name, "negative size", m=-1)
    refused(name, "misaligned", meas=ODD)
    refused(name, "misaligned", conf=ODD)
    refused(name, "misaligned", det=0x10002)
    refused(name, "misaligned", status=0x10002)
    refused(name, "no det_index", det=None, n=6)
    assert calls(det=None, n=0)[name]() == 0
    for name in ("busca_sort_gate_cost", "busca_sort_iou_cost"):
        assert calls(m=0)[name]() == 0
        assert calls(m=0, meas=None, out=None, cost=None)[name]() == 0
        refused(name, "negative size", m=-1)
        refused(name, "null pointer", meas=None)
        refused(name, "null pointer", out=None)
        refused(name, "misaligned", meas=ODD)
        refused(name, "misaligned", out=ODD)
        refused(name, "max_distance is NaN", maxd=nan, flags=2)
        refused(name, "more workgroups than a grid holds", n=16 * 65535 + 1)
    assert calls(maxd=nan, flags=0, n=0)["busca_sort_iou_cost"]() == 0                # NaN without CLAMP is no argument of the call
    name = "busca_sort_gate_cost"
    refused(name, "unknown flag bits", flags=4)
    refused(name, "unknown flag bits", flags=-1)
    refused(name, "lambda is NaN", lam=nan, flags=1)
    refused(name, "ld_cost", ld=4)
    refused(name, "null pointer", cost=None)
    refused(name, "misaligned", cost=ODD)
    refused(name, "misaligned", status=0x10002)
    assert calls(lam=nan, maxd=nan, flags=0, n=0)[name]() == 0
    rc = lib.busca_sort_iou_cost(P, 8, P, n, None, P, m, 1, 0.7, P, 0, None)           # MC is no flag of iou_cost
    assert rc == -1 and "unknown flag bits" in lib.busca_sort_last_error().decode()
    refused("busca_sort_camera_update", "null pointer", matrix=None)
    refused("busca_sort_camera_update", "misaligned", matrix=ODD)
    # the message is the calling thread's own
    import threading
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.busca_sort_last_error()))
    t.start()
    t.join()
    assert seen == [b""] and lib.busca_sort_last_error() != b""


def test_python_level_checks_and_facade():
    import torch
    from busca_amd import sort_store, tracking
    SortStore = sort_store.SortStore
    assert tracking.SortStore is SortStore and SortStore.__module__ == "busca_amd.sort_store"
    st = SortStore(S)
    assert st.capacity == S and st.dev == torch.device("cuda", 0) and st.mean is None       # nothing is allocated before the first use
    z = np.ones((4, 4))
    metric = types.SimpleNamespace(matching_threshold=0.3)
    for call in (lambda s: st.predict(s), lambda s: st.initiate(s, z), lambda s: st.update(s, z), lambda s: st.boxes(s),
                 lambda s: st.camera_update(s, np.eye(3)), lambda s: st.gate_cost(s, np.zeros((len(s), 4)), z), lambda s: st.iou_cost(s, z),
                 lambda s: st.appearance_round(metric, s, [1] * len(s), [1] * len(s), z, z), lambda s: st.iou_round(s, z, 0.7),
                 lambda s: st.load(s, [None] * len(s)), lambda s: st.store(s, [None] * len(s))):
        with pytest.raises(ValueError, match="distinct"):
            call([3, 1, 3])
        with pytest.raises(ValueError, match="beyond the capacity"):
            call([0, S])
    with pytest.raises(ValueError):
        SortStore(-1)
    with pytest.raises(ValueError, match="3 x 3"):
        st.camera_update([], np.eye(2))
    with pytest.raises(ValueError, match="track ids"):
        st.appearance_round(metric, [0, 1], [7], [1, 1], z, z)


def test_multi_dot_evaluates_f_times_p_ft():
    """The specification's finding: numpy's multi_dot((F, P, F.T)) is F @ (P @ F.T) bit for bit - and not (F @ P) @ F.T, the order of ByteTrack's
    kernel, on covariances that are not symmetric to the last bit (a symmetric one gives the same sums in both orders)."""
    differs = 0
    for steps in (1, 5, "fixture"):
        mean, cov = states(steps)
        assert any(not np.array_equal(c, c.T) for c in cov)
        for c in cov:
            md = np.linalg.multi_dot((F, c, F.T))
            assert np.array_equal(md, F @ (c @ F.T))
            differs += int(not np.array_equal(md, (F @ c) @ F.T))
    assert differs >= 8, differs


def test_camera_update_of_the_reference_is_inside_the_bound():
    """numpy's `matrix @ v` route of Track.camera_update against the left-to-right evaluation the kernel is held to (bit for bit): inside the bound
    derived from the inputs.  Euclidean warps, rotation up to 5 mrad, shift up to 20 px, coordinates up to 2000."""
    mean, _ = states(5)
    worst = 0.0
    assert np.abs(r_boxes(mean, True)).max() <= 2000.0
    for mat in euclidean_warps():
        for mu in mean:
            want, got, bound = r_camera(mu, mat), r_camera_numpy(mu, mat), camera_bound(mu, mat)
            for k in range(4):
                assert abs(got[k] - want[k]) <= bound[k], (k, got[k], want[k], bound[k])
                worst = max(worst, abs(got[k] - want[k]) / bound[k])
    print("camera_update: numpy route at most %.3g of the bound" % worst)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from busca_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))
    return t if dtype is None else t.to(dtype)


def _store(mean=None, cov=None, slots=None, capacity=S):
    """A SortStore; the states mean[i] / cov[i] in slot slots[i] for the live entries of `slots`, zeros elsewhere."""
    from busca_amd.sort_store import SortStore
    st = SortStore(capacity)
    st._state()
    if mean is not None:
        slots = np.asarray(slots)
        live = (slots >= 0) & (slots < capacity)
        st.mean[_dev(slots[live]).long()] = _dev(np.asarray(mean)[live])
        st.cov[_dev(slots[live]).long()] = _dev(np.asarray(cov)[live])
    return st


def _state_of(st):
    return st.mean.cpu().numpy(), st.cov.cpu().numpy()


def _untouched(before, after, slots, what):
    keep = np.ones(len(before[0]), dtype=bool)
    keep[[s for s in slots if 0 <= s < len(keep) - 1]] = False
    assert np.array_equal(before[0][keep], after[0][keep]) and np.array_equal(before[1][keep], after[1][keep]), what


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [1, 5, "fixture"])
@pytest.mark.parametrize("n", [1, 16, 17])
def test_predict_initiate_boxes_camera_update_are_bit_exact(n, steps):
    mean, cov = states(steps)
    slots, live = listed(n)
    st = _store(mean[:n], cov[:n], slots)
    dslots = _dev(slots)                                           # a device slot list is read in place: entries outside the store are skipped
    # predict
    before = _state_of(st)
    st.predict(dslots)
    after = _state_of(st)
    _untouched(before, after, slots, "predict")
    want = [r_predict(mean[i], cov[i]) for i in live]
    assert np.array_equal(after[0][slots[live]], np.stack([m for m, _ in want]))
    assert np.array_equal(after[1][slots[live]], np.stack([c for _, c in want]))
    bytetrack = np.stack([(F @ cov[i]) @ F.T for i in live])
    if n >= 16 and steps != 1:
        assert not np.array_equal(np.stack([F @ (cov[i] @ F.T) for i in live]), bytetrack)     # the two association orders do differ here
    # boxes
    pm = after[0]
    for tlbr in (False, True):
        box = st.boxes(dslots, tlbr=tlbr).cpu().numpy()
        assert np.array_equal(box[live], r_boxes(pm[slots[live]], tlbr)) and np.isnan(np.delete(box, live, 0)).all()
    # camera_update
    for mat in euclidean_warps()[:2]:
        before = _state_of(st)
        st.camera_update(dslots, mat)
        after = _state_of(st)
        _untouched(before, after, slots, "camera_update")
        for i in live:
            assert after[0][slots[i], :4].tolist() == r_camera(before[0][slots[i]], mat)
        assert np.array_equal(after[0][:, 4:], before[0][:, 4:]) and np.array_equal(after[1], before[1])
    # initiate, through det_index
    z = gold()["init_meas"]
    det = ((np.arange(n) * 11 + 3) % 64).astype(np.int32)
    before = after
    st.initiate(dslots, z, det)
    after = _state_of(st)
    _untouched(before, after, slots, "initiate")
    wm, wc = r_initiate(z[det[live]])
    assert np.array_equal(after[0][slots[live]], wm) and np.array_equal(after[1][slots[live]], wc)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 64, 65])
@pytest.mark.parametrize("n", [1, 16, 17])
def test_iou_cost_is_bit_exact(n, m):
    for steps in (1, 5):
        mean, cov = states(steps)
        slots, live = listed(n)
        st = _store(mean[:n], cov[:n], slots)
        det = tlwh_of(detections_near(mean[:n], m, 7 * n + m))
        tlwh = r_boxes(mean[:n], False)
        stale = (np.arange(n) % 5 == 3)
        skipped = np.ones(n, dtype=bool)
        skipped[live] = False
        for flags, maxd in ((None, None), (stale, None), (stale, 0.7), (None, 0.7)):
            got = st.iou_cost(_dev(slots), det, stale=flags, max_distance=maxd).cpu().numpy()
            want = r_iou_cost(tlwh, det, skipped | (flags if flags is not None else False), maxd)
            assert got.shape == (n, m) and np.array_equal(got, want), (steps, maxd)
        if m >= 64:
            assert (got[live] < 0.7).any()                          # some pair does overlap


@pytest.mark.gpu
def test_iou_cost_edge_cases():
    mean = np.zeros((3, 8))
    mean[:, :4] = [[100.0, 200.0, 0.5, 80.0], [400.0, 300.0, 0.4, 100.0], [50.5, 60.25, 0.3, 33.0]]
    st = _store(mean, np.zeros((3, 8, 8)), [5, 0, 9])
    tlwh = r_boxes(mean, False)
    det = np.stack([tlwh[0],                                       # identical to track 0
                    [1000.0, 1000.0, 10.0, 10.0],                  # disjoint from all
                    [tlwh[1][0] + 5, tlwh[1][1] + 5, 0.0, 30.0],   # zero area, inside track 1
                    [tlwh[0][0] + tlwh[0][2], tlwh[0][1], 20.0, 20.0],      # touches track 0 along an edge
                    tlwh[2] + [0.125, -0.25, 0.5, 1.0]])
    for stale in (None, [False, True, False]):
        for maxd in (None, 0.7):
            got = st.iou_cost([5, 0, 9], det, stale=stale, max_distance=maxd).cpu().numpy()
            assert np.array_equal(got, r_iou_cost(tlwh, det, stale, maxd))
            if maxd is None:
                assert got[0, 0] == 0.0 and (got[:, 1] == (1.0 if stale is None else [1.0, INFTY, 1.0])).all() and got[0, 3] == 1.0
                assert got[1, 2] == (1.0 if stale is None else INFTY) and 0.0 < got[2, 4] < 0.2
            else:
                assert got.max() == 0.7 + 1e-5 and got[0, 0] == 0.0
    assert st.iou_cost([], det).shape == (0, 5) and st.iou_cost([5], np.zeros((0, 4))).shape == (1, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 16, 17])
def test_update_at_confidence_0_is_busca_track_kalman_update(n):
    from busca_amd.kalman_store import KalmanStore
    g = gold()
    slots, live = listed(n)
    det = ((np.arange(n) * 37 + 5) % 96).astype(np.int32)
    want = None
    for conf in ("track", None, 0.0, np.zeros(96)):
        st = _store(g["mean"][:n], g["cov"][:n], slots)
        before = _state_of(st)
        if isinstance(conf, str):                                   # busca_track_kalman_update itself, on the same tensors
            ks = KalmanStore(S)
            ks.mean, ks.cov = st.mean, st.cov
            status = ks.update(_dev(slots), g["meas"], det)
        else:
            status = st.update(_dev(slots), g["meas"], det, confidence=conf)
        after = _state_of(st)
        _untouched(before, after, slots, "update")
        assert not status.cpu().numpy().any() and not np.array_equal(after[1][slots[live]], before[1][slots[live]])
        if want is None:
            want = after
        assert np.array_equal(after[0], want[0]) and np.array_equal(after[1], want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("conf", [0.3, 0.9, 1.0, "mix"])
def test_update_with_confidence_is_inside_the_bars(conf):
    g = gold()
    _, bar = bars()
    n = 17
    slots, live = listed(n)
    det = ((np.arange(n) * 37 + 5) % 96).astype(np.int32)
    c = np.full(96, conf) if conf != "mix" else np.array([0.0, 0.3, 0.9, 0.999, 1.0, 0.5])[np.arange(96) % 6]
    st = _store(g["mean"][:n], g["cov"][:n], slots)
    status = st.update(_dev(slots), g["meas"], det, confidence=c if conf == "mix" else conf)
    got = _state_of(st)
    want = [r_update_nsa(g["mean"][i], g["cov"][i], g["meas"][det[i]], float(c[det[i]])) for i in live]
    em = err_mean(got[0][slots[live]], np.stack([a for a, _ in want]))
    ec = err_cov(got[1][slots[live]], np.stack([b for _, b in want]))
    print("update, confidence %s: mean error %.3g (bar %.3g), covariance %.3g (bar %.3g)" % (conf, em, bar["mean"], ec, bar["cov"]))
    assert not status.cpu().numpy().any() and em <= bar["mean"] and ec <= bar["cov"]
    if conf != "mix" and conf < 1.0:                                # the confidence is used: the result is not the plain update's
        plain = [r_update_nsa(g["mean"][i], g["cov"][i], g["meas"][det[i]], 0.0) for i in live]
        assert err_cov(np.stack([b for _, b in plain]), np.stack([b for _, b in want])) > 1e-4


@pytest.mark.gpu
def test_update_chain_of_16_steps_is_inside_the_chain_bars():
    g = gold()
    _, bar = bars()
    m, c = g["chain_mean0"].copy(), g["chain_cov0"].copy()
    k = len(m)
    slots = PERM[:k]
    st = _store(m, c, slots)
    conf = np.array([0.0, 0.3, 0.9, 0.999, 0.6, 1.0, 0.1, 0.75])
    em = ec = 0.0
    for s in range(16):
        st.predict(slots)
        st.update(slots, g["chain_meas"][s], confidence=np.roll(conf, s))
        up = [r_update_nsa(*r_predict(m[i], c[i]), g["chain_meas"][s, i], float(np.roll(conf, s)[i])) for i in range(k)]
        m, c = np.stack([a for a, _ in up]), np.stack([b for _, b in up])
        got = _state_of(st)
        em, ec = max(em, err_mean(got[0][slots], m)), max(ec, err_cov(got[1][slots], c))
    print("16-step chain: mean error %.3g (bar %.3g), covariance %.3g (bar %.3g)" % (em, bar["chain_mean"], ec, bar["chain_cov"]))
    assert em <= bar["chain_mean"] and ec <= bar["chain_cov"]


@pytest.mark.gpu
def test_update_not_positive_definite():
    import torch
    from busca_amd import _sort_lib
    from busca_amd._xfer import stream_of
    g = gold()
    mean, cov = g["mean"][4:7].copy(), g["cov"][4:7].copy()
    cov[1, :4, :4] = -np.eye(4)
    slots = np.array([9, 2, 5])
    st = _store(mean, cov, slots)
    status = st.update(slots, g["meas"][4:7], confidence=0.4).cpu().numpy()
    m, c = _state_of(st)
    assert status.tolist() == [0, 1, 0]
    assert np.array_equal(m[2], mean[1]) and np.array_equal(c[2], cov[1])                      # untouched, bit for bit
    assert not np.array_equal(c[9], cov[0]) and not np.array_equal(c[5], cov[2])
    # status = NULL is accepted
    st2 = _store(mean, cov, slots)
    z, sl = _dev(g["meas"][4:7]), _dev(slots.astype(np.int32))
    cf = _dev(np.full(3, 0.4))
    dev = torch.device("cuda", 0)
    _sort_lib.check(_sort_lib.load().busca_sort_update(st2.mean.data_ptr(), st2.cov.data_ptr(), S, sl.data_ptr(), 3, z.data_ptr(), None, 3, cf.data_ptr(),
                                                       None, 0, stream_of(dev)))
    m2, c2 = _state_of(st2)
    assert np.array_equal(m2, m) and np.array_equal(c2, c)


def _chain(ctx, mean, cov, xyah, cost, mc_lambda, gated_cost, max_distance):
    """The object route's device chain on gathered states: _upload_states, busca_kalman_gating, kalman._gate_dev, the torch.where clamp."""
    import torch
    from busca_amd import kalman
    objs = [types.SimpleNamespace(mean=m, covariance=c) for m, c in zip(mean, cov)]
    dm, dc = kalman._upload_states(objs, torch.device("cuda", 0))
    gate, status = kalman._gating_dev(ctx, dm, dc, _dev(xyah), False, 0)
    out = kalman._gate_dev(_dev(cost), gate, False, mc_lambda, float(gated_cost))
    if max_distance is not None:
        out = torch.where(out > max_distance, max_distance + 1e-5, out)
    return out.cpu().numpy(), status.cpu().numpy(), gate.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 64, 65])
@pytest.mark.parametrize("n", [1, 16, 17])
def test_gate_cost_equals_the_chain(ctx, n, m):
    import torch
    from busca_amd import _sort_lib
    from busca_amd._xfer import stream_of
    mean, cov = (a[:n].copy() for a in states(5))
    slots, live = listed(n)
    if n >= 16:
        cov[4, :4, :4] = -np.eye(4)                                # one row that is not positive definite
    bad = np.zeros(n, dtype=bool)
    bad[4:5] = n >= 16
    good = live[~bad[live]]
    st = _store(mean, cov, slots)
    xyah = detections_near(mean, m, 3 * n + m)
    cost = np.random.RandomState(n * m).uniform(0.0, 0.6, (n, m))
    gated_seen = 0
    for lam in (None, 0.98):
        for maxd in (None, 0.3):
            for gated_cost in (1e5, 7.0):
                want, wstatus, gate = _chain(ctx, mean, cov, xyah, cost, lam, gated_cost, maxd)
                got, status = st.gate_cost(_dev(slots), cost, xyah, mc_lambda=lam, gated_cost=gated_cost, max_distance=maxd)
                got, status = got.cpu().numpy(), status.cpu().numpy()
                assert np.array_equal(got[good], want[good]), (lam, maxd, gated_cost)
                assert np.array_equal(status[live], wstatus[live]) and np.array_equal(status != 0, bad)
                assert np.isnan(got[bad]).all()                                                # not positive definite: NaN whatever the flags
                skipped_value = gated_cost if maxd is None or not gated_cost > maxd else maxd + 1e-5
                assert (np.delete(got, live, 0) == skipped_value).all()
                gated_seen += int((gate[good] > CHI2_4).sum())
    if n >= 16 and m >= 64:
        assert gated_seen and (gate[good] <= CHI2_4).any()        # entries on both sides of the gate
    # `out` aliasing `cost`, and a cost matrix with a leading dimension beyond m - the raw call
    lib, dev = _sort_lib.load(), torch.device("cuda", 0)
    want, _, _ = _chain(ctx, mean, cov, xyah, cost, 0.98, 1e5, 0.3)
    sl, z = _dev(slots), _dev(xyah)
    inplace = _dev(cost)
    _sort_lib.check(lib.busca_sort_gate_cost(st.mean.data_ptr(), st.cov.data_ptr(), S, sl.data_ptr(), n, z.data_ptr(), m, inplace.data_ptr(), m, 1e5, 3, 0.98,
                                             0.3, inplace.data_ptr(), None, 0, stream_of(dev)))
    assert np.array_equal(inplace.cpu().numpy()[good], want[good])
    wide = torch.full((n, m + 3), -1.0, dtype=torch.float64, device=dev)
    wide[:, :m] = _dev(cost)
    out = torch.full((n + 1, m), -3.0, dtype=torch.float64, device=dev)
    _sort_lib.check(lib.busca_sort_gate_cost(st.mean.data_ptr(), st.cov.data_ptr(), S, sl.data_ptr(), n, z.data_ptr(), m, wide.data_ptr(), m + 3, 1e5, 3, 0.98,
                                             0.3, out.data_ptr(), None, 0, stream_of(dev)))
    out = out.cpu().numpy()
    assert np.array_equal(out[:n][good], want[good]) and (out[n] == -3.0).all() and (wide[:, m:] == -1.0).all().item()


@pytest.mark.gpu
def test_gate_cost_against_the_reference(ctx):
    from tests import test_appearance as ta
    g = ta.gold()
    _, bar = bars()
    trk, det, lam, maxd, tracks, dets = ta.gate_case()
    ti, di = [int(i) for i in g["gate_ti"]], [int(j) for j in g["gate_di"]]
    cost = g["gate_cost"][np.ix_(ti, di)]
    gate = ta.kalman()["gate_maha4"][np.ix_(ti, di)]
    slots = np.random.RandomState(2).permutation(128)[:len(ti)]
    st = _store(np.stack([tracks[i].mean for i in ti]), np.stack([tracks[i].covariance for i in ti]), slots, capacity=128)
    xyah = np.stack([dets[j].to_xyah() for j in di])
    got, status = st.gate_cost(slots, cost, xyah)
    assert np.array_equal(got.cpu().numpy(), g["gate_ref_mc0"]) and not status.cpu().numpy().any()
    got = st.gate_cost(slots, cost, xyah, mc_lambda=lam)[0].cpu().numpy()
    ref = g["gate_ref_mc1"]
    assert np.array_equal(got > 1e4, ref > 1e4) and np.array_equal(ref > 1e4, gate > CHI2_4)      # the identical set of gated entries
    tol = (1 - lam) * bar["gate"] * np.maximum(1.0, np.abs(gate)) + 4 * EPS * np.abs(ref)
    print("SortStore.gate_cost with MC: max |d| %.3g" % np.abs(got - ref).max())
    assert (np.abs(got - ref) <= tol).all()
    assert np.array_equal(st.gate_cost(slots, cost, xyah, gated_cost=7.0)[0].cpu().numpy() == 7.0, gate > CHI2_4)


def _separated(cost, threshold, what):
    """No two candidate costs of a row, and no cost and its threshold, closer than 1e-6 (host matrix of the object route)."""
    for r, row in enumerate(cost):
        cand = np.sort(row[row <= threshold])
        assert len(cand) < 2 or np.diff(cand).min() >= 1e-6, (what, r)
    assert np.abs(cost - threshold).min() >= 1e-6, what


@pytest.mark.gpu
@pytest.mark.parametrize("mc_lambda", [None, 0.98])
@pytest.mark.parametrize("depth", [None, 3])
def test_appearance_round_equals_the_object_route(ctx, depth, mc_lambda):
    from busca_amd import tracking
    from tests import test_appearance as ta
    g = ta.gold()
    trk, det, lam, maxd, tracks, dets = ta.gate_case()
    ti, di = [int(i) for i in g["gate_ti"]], [int(j) for j in g["gate_di"]]
    metric = ta._fitted_metric(ctx, trk, maxd, budget=3)
    sub = [tracks[i] for i in ti]
    sel = [dets[j] for j in di]
    host = tracking.gate_cost_matrix_mc(metric.distance(np.stack([d.feature for d in sel]), [t.track_id for t in sub]), sub, sel, list(range(len(sub))),
                                        list(range(len(sel))), mc_lambda=mc_lambda, ctx=ctx)
    _separated(host, metric.matching_threshold, "appearance")
    want = tracking.appearance_round(metric, sub, sel, list(range(len(sub))), cascade_depth=depth, mc_lambda=mc_lambda, ctx=ctx)
    slots = np.random.RandomState(4).permutation(128)[:len(sub)]
    st = _store(np.stack([t.mean for t in sub]), np.stack([t.covariance for t in sub]), slots, capacity=128)
    got = st.appearance_round(metric, slots, [t.track_id for t in sub], [t.time_since_update for t in sub], np.stack([d.feature for d in sel]),
                              np.stack([d.to_xyah() for d in sel]), cascade_depth=depth, mc_lambda=mc_lambda)
    assert got[0] == want[0] and len(got[0]) >= 5
    assert sorted(got[1]) == sorted(want[1]) and got[2] == want[2]
    assert st.appearance_round(metric, [], [], [], np.zeros((2, 4)), np.zeros((2, 4))) == ([], [], [0, 1])


@pytest.mark.gpu
def test_iou_round_equals_min_cost_matching(ctx):
    from busca_amd import tracking
    mean, cov = states(5)
    n = 17
    slots, live = listed(n)
    st = _store(mean[:n], cov[:n], slots)
    rs = np.random.RandomState(8)
    tlwh = r_boxes(mean[:n], False)
    det = tlwh[rs.permutation(n)[:12]] * (1 + rs.uniform(-0.08, 0.08, (12, 4)))
    det = np.concatenate([det, [[3000.0, 3000.0, 40.0, 90.0]]])
    stale = np.arange(n) % 6 == 1
    skipped = np.ones(n, dtype=bool)
    skipped[live] = False
    for di in (None, [12, 0, 3, 4, 7, 9, 10]):
        cand = det if di is None else det[di]
        host = r_iou_cost(tlwh, cand, stale | skipped)
        _separated(host, 0.7, "iou")
        want = tracking.min_cost_matching(lambda *a: r_iou_cost(tlwh, cand, stale | skipped), 0.7, None, None, list(range(n)),
                                          list(range(len(cand))) if di is None else di, ctx=ctx)
        got = st.iou_round(_dev(slots), det, 0.7, stale=stale, detection_indices=di)
        assert got[0] == [(int(a), int(b)) for a, b in want[0]] and len(got[0]) >= (4 if di is None else 1)
        assert got[1] == [int(a) for a in want[1]] and got[2] == [int(b) for b in want[2]]
    assert st.iou_round(_dev(slots), np.zeros((0, 4)), 0.7) == ([], list(range(n)), [])


# ---- the scripted scene -------------------------------------------------------------------------------------------------------
def _scene():
    """12 frames, 6 tracks, up to 8 detections a frame: per frame the tlwh boxes and confidences of the detections, in an order that is not the
    tracks'.  Target 2 is missed at frames 5-6 (its track is deleted at frame 6), target 6 is born at frame 7 (into the freed slot), target 5 is
    born at frame 3.  The camera moves a little at frames 4 and 9.  Confidences include exactly 0 and 0.999."""
    rs = np.random.RandomState(21)
    start = np.array([[100, 100, 40, 100], [400, 120, 50, 120], [700, 90, 45, 110], [250, 400, 60, 150], [900, 380, 55, 140],
                      [600, 600, 50, 125], [1200, 200, 48, 118]], dtype=np.float64)
    vel = np.array([[6, 1], [-5, 2], [4, -1], [3, 3], [-6, -2], [5, 0], [-4, 2]], dtype=np.float64)
    born = [1, 1, 1, 1, 1, 3, 7]
    frames = []
    for f in range(1, 13):
        boxes, conf = [], []
        for t in range(7):
            if f < born[t] or (t == 2 and f >= 5):
                continue
            b = start[t].copy()
            b[:2] += vel[t] * (f - 1) + rs.uniform(-1.5, 1.5, 2)
            b[2:] *= 1 + rs.uniform(-0.02, 0.02, 2)
            boxes.append(b)
            conf.append([0.0, 0.999, 0.6, 0.85, 0.3, 0.95, 0.7][(t + f) % 7])
        order = rs.permutation(len(boxes))
        frames.append((np.stack(boxes)[order], np.asarray(conf)[order]))
    warps = {f: np.array([[math.cos(t), -math.sin(t), dx], [math.sin(t), math.cos(t), dy], [0.0, 0.0, 1.0]]) for f, t, dx, dy in ((4, 2e-3, 3.0, -2.0), (9, -1e-3, -2.5, 1.5))}
    return frames, warps


def _xyah_of(tlwh):
    out = np.array(tlwh, dtype=np.float64).reshape(-1, 4)
    out[:, :2] += out[:, 2:] / 2
    out[:, 2] /= out[:, 3]
    return out


@pytest.mark.gpu
def test_scripted_replay(ctx):
    """The host loop over objects with the restated filter and the SortStore route, frame by frame.  Steps that are bit-exact given their input
    are checked on the store's own input state; the two chains as wholes stay inside the chain bars; the matches are identical."""
    from busca_amd import tracking
    _, bar = bars()
    frames, warps = _scene()
    st = _store(capacity=8)
    tracks = []                                                    # host objects: slot, mean, covariance, time_since_update
    free = list(range(8))[::-1]
    em = ec = 0.0
    seen = {"births": 0, "miss": 0, "deleted": 0, "reused": False, "camera": 0}
    freed = set()
    for f, (det, conf) in enumerate(frames, start=1):
        slots = np.array([t.slot for t in tracks], dtype=np.int32)
        n = len(tracks)
        # predict
        before = _state_of(st)
        st.predict(slots)
        after = _state_of(st)
        for t in tracks:
            pm, pc = r_predict(before[0][t.slot], before[1][t.slot])
            assert np.array_equal(after[0][t.slot], pm) and np.array_equal(after[1][t.slot], pc), (f, "predict")
            t.mean, t.covariance = r_predict(t.mean, t.covariance)
            t.time_since_update += 1
        # camera update
        if f in warps:
            before = after
            st.camera_update(slots, warps[f])
            after = _state_of(st)
            for t in tracks:
                assert after[0][t.slot, :4].tolist() == r_camera(before[0][t.slot], warps[f]), (f, "camera_update")
                t.mean = np.concatenate([r_camera(t.mean, warps[f]), t.mean[4:]])
            seen["camera"] += 1
        # boxes and the IoU round
        stale = np.array([t.time_since_update > 1 for t in tracks], dtype=bool)
        if n:
            assert np.array_equal(st.boxes(slots, tlbr=False).cpu().numpy(), r_boxes(after[0][slots], False)), (f, "boxes")
            assert np.array_equal(st.iou_cost(slots, det, stale=stale).cpu().numpy(), r_iou_cost(r_boxes(after[0][slots], False), det, stale)), (f, "iou")
        host_cost = r_iou_cost(r_boxes(np.stack([t.mean for t in tracks]), False), det, stale) if n else np.zeros((0, len(det)))
        if n:
            _separated(host_cost, 0.7, f)
        want = tracking.min_cost_matching(lambda *a: host_cost, 0.7, None, None, list(range(n)), list(range(len(det))), ctx=ctx) if n else ([], [], list(range(len(det))))
        got = st.iou_round(slots, det, 0.7, stale=stale)
        assert got[0] == [(int(a), int(b)) for a, b in want[0]] and got[1] == [int(a) for a in want[1]] and got[2] == [int(b) for b in want[2]], f
        # update of the matched pairs
        z = _xyah_of(det)
        if got[0]:
            rows, cols = [r for r, _ in got[0]], [c for _, c in got[0]]
            status = st.update(slots[rows], z, cols, confidence=conf)
            assert not status.cpu().numpy().any()
            for r, c in got[0]:
                tracks[r].mean, tracks[r].covariance = r_update_nsa(tracks[r].mean, tracks[r].covariance, z[c], float(conf[c]))
                tracks[r].time_since_update = 0
        # misses and deletions: a track is deleted at its second miss in a row
        for r in got[1]:
            seen["miss"] += 1
            if tracks[r].time_since_update >= 2:
                free.append(tracks[r].slot)
                freed.add(tracks[r].slot)
                tracks[r] = None
                seen["deleted"] += 1
        tracks = [t for t in tracks if t is not None]
        # initiation, into free slots
        if got[2]:
            new = [free.pop() for _ in got[2]]
            seen["reused"] |= bool(freed & set(new))
            before = _state_of(st)
            st.initiate(new, z, got[2])
            after = _state_of(st)
            wm, wc = r_initiate(z[got[2]])
            assert np.array_equal(after[0][new], wm) and np.array_equal(after[1][new], wc), (f, "initiate")
            _untouched(before, after, new, "initiate")
            tracks += [types.SimpleNamespace(slot=s, mean=wm[i], covariance=wc[i], time_since_update=0) for i, s in enumerate(new)]
            seen["births"] += len(new)
        # the two chains
        state = _state_of(st)
        slots = [t.slot for t in tracks]
        e1, e2 = err_mean(state[0][slots], np.stack([t.mean for t in tracks])), err_cov(state[1][slots], np.stack([t.covariance for t in tracks]))
        em, ec = max(em, e1), max(ec, e2)
        assert e1 <= bar["chain_mean"] and e2 <= bar["chain_cov"], (f, e1, e2)
    print("scripted replay: worst mean error %.3g (bar %.3g), covariance %.3g (bar %.3g); %r" % (em, bar["chain_mean"], ec, bar["chain_cov"], seen))
    assert seen["births"] == 7 and seen["miss"] == 2 and seen["deleted"] == 1 and seen["reused"] and seen["camera"] == 2 and len(tracks) == 6
    # store() then load() round-trips bit for bit
    slots = [t.slot for t in tracks]
    state = _state_of(st)
    back = [types.SimpleNamespace(mean=None, covariance=None) for _ in slots]
    st.store(slots, back)
    assert all(np.array_equal(b.mean, state[0][s]) and np.array_equal(b.covariance, state[1][s]) for b, s in zip(back, slots))
    other = _store(capacity=8)
    other.load(slots[::-1], back[::-1])
    again = _state_of(other)
    assert np.array_equal(again[0][slots], state[0][slots]) and np.array_equal(again[1][slots], state[1][slots])
    assert not again[0][[s for s in range(9) if s not in slots]].any()


@pytest.mark.gpu
def test_slots_outside_the_store_touch_nothing():
    import torch
    from busca_amd.sort_store import SortStore
    g = gold()
    CAP, GUARD, CANARY = 8, 6, 777.25
    dev = torch.device("cuda", 0)
    mean_buf = torch.full((GUARD + CAP + 1 + GUARD, 8), CANARY, dtype=torch.float64, device=dev)
    cov_buf = torch.full((GUARD + CAP + 1 + GUARD, 8, 8), CANARY, dtype=torch.float64, device=dev)
    st = SortStore(CAP)
    st.mean, st.cov = mean_buf[GUARD:GUARD + CAP + 1], cov_buf[GUARD:GUARD + CAP + 1]
    st.mean[:CAP], st.cov[:CAP] = _dev(g["mean"][:CAP]), _dev(g["cov"][:CAP])
    slot = _dev(np.array([CAP, 3, CAP + 1, 2 ** 31 - 1, -5, CAP + GUARD - 1, -2 ** 31], dtype=np.int32))      # one entry inside the store
    live = GUARD + 3
    meas = g["meas"][:7]
    before = (mean_buf.cpu().numpy(), cov_buf.cpu().numpy())

    def only_slot_3_changed(what):
        after = (mean_buf.cpu().numpy(), cov_buf.cpu().numpy())
        keep = np.arange(len(after[0])) != live
        assert np.array_equal(after[0][keep], before[0][keep]) and np.array_equal(after[1][keep], before[1][keep]), what
        assert not np.array_equal(after[0][live], before[0][live]) and not np.array_equal(after[1][live], before[1][live]), what
        assert (after[0][:GUARD] == CANARY).all() and (after[0][GUARD + CAP:] == CANARY).all(), what
        assert (after[1][:GUARD] == CANARY).all() and (after[1][GUARD + CAP:] == CANARY).all(), what
    st.predict(slot)
    only_slot_3_changed("predict")
    assert st.update(slot, meas, confidence=0.5).cpu().numpy().tolist() == [0] * 7
    only_slot_3_changed("update")
    cov_before = cov_buf.cpu().numpy()
    st.camera_update(slot, euclidean_warps()[0])
    assert np.array_equal(cov_buf.cpu().numpy(), cov_before)
    only_slot_3_changed("camera_update")
    box = st.boxes(slot).cpu().numpy()
    assert np.isnan(box[[0, 2, 3, 4, 5, 6]]).all() and np.isfinite(box[1]).all()
    # the cost matrices, between guard rows of their own
    m = 5
    cost, status = st.gate_cost(slot, np.full((7, m), 0.2), meas[:m], mc_lambda=0.98, gated_cost=7.0, max_distance=9.0)
    cost = cost.cpu().numpy()
    assert (cost[[0, 2, 3, 4, 5, 6]] == 7.0).all() and np.isfinite(cost[1]).all() and not status.cpu().numpy().any()
    iou = st.iou_cost(slot, tlwh_of(meas[:m]), stale=np.zeros(7, dtype=bool)).cpu().numpy()
    assert (iou[[0, 2, 3, 4, 5, 6]] == INFTY).all() and (iou[1] <= 1.0).all()
    # a detection index outside the measurements skips the pair
    st.update(slot, meas, _dev(np.array([0, 7, 1, 2, 3, 4, 5], dtype=np.int32)), confidence=0.5)
    st.update(slot, meas, _dev(np.array([0, -1, 1, 2, 3, 4, 5], dtype=np.int32)), confidence=0.5)
    st.initiate(slot, meas, _dev(np.array([0, 7, 1, 2, 3, 4, 5], dtype=np.int32)))
    after = (mean_buf.cpu().numpy(), cov_buf.cpu().numpy())
    st.initiate(slot, meas)
    only_slot_3_changed("initiate")
    assert np.array_equal(mean_buf.cpu().numpy()[live, :4], meas[1]) and not np.array_equal(mean_buf.cpu().numpy()[live], after[0][live])
