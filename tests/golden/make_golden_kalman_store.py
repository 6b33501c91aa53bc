#!/usr/bin/env python3
"""Generate tests/golden/kalman_store.npz: a 16-frame ByteTrack-like script over a store of 16 slots, run through the reference's vendored
KalmanFilter (adapters/CenterTrack/src/lib/utils/mot_online/kalman_filter.py, loaded by path as make_golden_kalman.py does).  Run from the repo
root where the reference is present:

    python tests/golden/make_golden_kalman_store.py

Every frame f = 1 .. 16 (row f - 1 of every array) has three phases, each a list of slots, padded to 16 entries with PAD:
  phase 0  predict   pred_slot, pred_nt (the `not_tracked` flags: mean[7] = 0 first), pred_n entries         STrack.multi_predict
  phase 1  update    upd_slot, upd_det (the measurement of each pair), upd_n entries                         KalmanFilter.update
  phase 2  initiate  ini_slot, ini_det, ini_n entries                                                        KalmanFilter.initiate
  meas [16, 8, 4], meas_m   the frame's measurements (x, y, a, h); more of them than pairs, and det indices that are no identity
  mean [16, 3, 16, 8], cov [16, 3, 16, 8, 8]   EVERY slot's state after each phase (zeros where a slot was never initiated)
A listed slot of -1 is skipped, as the kernels skip it.  What the script contains is asserted below, so an edit cannot lose a case silently.
The fixture holds arrays only."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

from busca_amd import synth  # noqa: E402

SEED = 61
FRAMES, CAPACITY, MAX_M, PAD = 16, 16, 8, -2

# track -> (slot, first frame, frames without a measurement).  A track is initiated in its first frame, updated in every later frame that has a
# measurement for it, and predicted from its SECOND frame after the first on: in the frame after its initiation it is unconfirmed, which
# ByteTrack updates without having predicted it (byte_tracker.py: strack_pool holds tracked and lost tracks only) - unless it started in frame 1,
# where tracks are activated at once.
TRACKS = {
    "A": (3, 1, {13}),
    "B": (7, 1, {5, 6, 7, 8, 13}),          # lost at frames 5-8: predicted with not_tracked from frame 6 until it is found again at frame 9
    "C": (0, 1, {13}),
    "D": (12, 3, {13}),
    "E": (5, 3, set()),                     # abandoned at frame 6: its slot is listed no more ...
    "F": (9, 9, {13}),
    "G": (5, 10, {13}),                     # ... until this track moves in at frame 10
}
LAST_FRAME = {"E": 5}
NO_DETECTION, MINUS_ONE = 13, 14           # the frame without a detection; the frame whose predict and update lists carry a slot of -1


def load_kalman():
    spec = importlib.util.spec_from_file_location("ref_kalman_filter", os.path.join(REF, "adapters/CenterTrack/src/lib/utils/mot_online/kalman_filter.py"))
    kfm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kfm)
    return kfm


def path_of(name):
    """The measurement of track `name` (number k) at every frame: a straight path, jittered in proportion to the box height."""
    z0 = np.array([synth.uniform(SEED, name + "x", (1,), 200, 1700)[0], synth.uniform(SEED, name + "y", (1,), 200, 900)[0],
                   synth.uniform(SEED, name + "a", (1,), 0.25, 0.9)[0], synth.uniform(SEED, name + "h", (1,), 40, 500)[0]], dtype=np.float64)
    vel = np.array([synth.uniform(SEED, name + "vx", (1,), -0.04, 0.04)[0], synth.uniform(SEED, name + "vy", (1,), -0.02, 0.02)[0]]) * z0[3]
    noise = synth.uniform(SEED, name + "n", (FRAMES + 1, 4), -1, 1).astype(np.float64)
    out = np.zeros((FRAMES + 1, 4))
    for f in range(FRAMES + 1):
        h = z0[3]
        out[f] = [z0[0] + vel[0] * f + 0.03 * h * noise[f, 0], z0[1] + vel[1] * f + 0.03 * h * noise[f, 1], z0[2] * (1.0 + 0.02 * noise[f, 2]),
                  h * (1.0 + 0.004 * f + 0.02 * noise[f, 3])]
    return out


def make(kfm):
    kf = kfm.KalmanFilter()
    paths = {name: path_of(name) for name in sorted(TRACKS)}
    clutter = np.stack([synth.uniform(SEED, "cx", (FRAMES + 1, 2), 100, 1800), synth.uniform(SEED, "cy", (FRAMES + 1, 2), 100, 1000),
                        synth.uniform(SEED, "ca", (FRAMES + 1, 2), 0.25, 0.9), synth.uniform(SEED, "ch", (FRAMES + 1, 2), 40, 500)], 2).astype(np.float64)
    mean, cov = np.zeros((CAPACITY, 8)), np.zeros((CAPACITY, 8, 8))
    out = {k: np.full((FRAMES, CAPACITY), PAD, dtype=np.int32) for k in ("pred_slot", "upd_slot", "upd_det", "ini_slot", "ini_det")}
    out.update(pred_nt=np.zeros((FRAMES, CAPACITY), dtype=np.uint8), meas=np.zeros((FRAMES, MAX_M, 4)),
               mean=np.zeros((FRAMES, 3, CAPACITY, 8)), cov=np.zeros((FRAMES, 3, CAPACITY, 8, 8)))
    out.update({k: np.zeros(FRAMES, dtype=np.int32) for k in ("pred_n", "upd_n", "ini_n", "meas_m")})
    seen = set()

    def put(key, f, values):
        out[key][f - 1, :len(values)] = values

    for f in range(1, FRAMES + 1):
        alive = [t for t in sorted(TRACKS) if TRACKS[t][1] <= f <= LAST_FRAME.get(t, FRAMES)]
        measured = [t for t in alive if f not in TRACKS[t][2]] if f != NO_DETECTION else []
        # ---- the frame's measurements: the measured tracks' and two of clutter, in an order that is no identity
        owners = measured + (["", ""] if f != NO_DETECTION else [])
        order = np.argsort(synth.uniform(SEED, "order%d" % f, (len(owners),), 0, 1), kind="stable")[::-1]
        owners = [owners[i] for i in order]
        n_clutter = 0
        for j, t in enumerate(owners):
            if t == "":
                out["meas"][f - 1, j] = clutter[f, n_clutter]
                n_clutter += 1
            else:
                out["meas"][f - 1, j] = paths[t][f]
        out["meas_m"][f - 1] = len(owners)
        assert len(owners) <= MAX_M
        # ---- phase 0: predict, newest track first (descending track name: the slots come in no particular order)
        pred = [t for t in reversed(alive) if TRACKS[t][1] < f and not (TRACKS[t][1] > 1 and f == TRACKS[t][1] + 1)]
        slots = [TRACKS[t][0] for t in pred]
        lost = [int(f - 1 in TRACKS[t][2]) for t in pred]                      # no measurement in the previous frame: the track is Lost
        if f == MINUS_ONE:
            slots.insert(1, -1)
            lost.insert(1, 1)
        put("pred_slot", f, slots)
        put("pred_nt", f, lost)
        out["pred_n"][f - 1] = len(slots)
        for s, nt in zip(slots, lost):
            if s < 0:
                continue
            m = mean[s].copy()
            if nt:
                m[7] = 0
                seen.add("zeroed")
            pm, pc = kf.multi_predict(m[None], cov[s][None])
            mean[s], cov[s] = pm[0], pc[0]
        out["mean"][f - 1, 0], out["cov"][f - 1, 0] = mean, cov
        # ---- phase 1: update of every measured track that existed before this frame
        upd = [t for t in reversed(alive) if t in measured and TRACKS[t][1] < f]
        slots, dets = [TRACKS[t][0] for t in upd], [owners.index(t) for t in upd]
        if f == MINUS_ONE:
            slots.insert(0, -1)
            dets.insert(0, owners.index(""))
        put("upd_slot", f, slots)
        put("upd_det", f, dets)
        out["upd_n"][f - 1] = len(slots)
        for t in upd:
            s = TRACKS[t][0]
            if TRACKS[t][1] > 1 and f == TRACKS[t][1] + 1:
                assert s not in out["pred_slot"][f - 1]
                seen.add("unconfirmed")
            if t == "B" and f == 9:
                assert out["pred_nt"][f - 1, list(out["pred_slot"][f - 1]).index(s)] == 1
                seen.add("found again")
            mean[s], cov[s] = kf.update(mean[s], cov[s], out["meas"][f - 1, owners.index(t)])
        out["mean"][f - 1, 1], out["cov"][f - 1, 1] = mean, cov
        # ---- phase 2: initiation of the tracks that start here
        ini = [t for t in reversed(alive) if TRACKS[t][1] == f]
        slots, dets = [TRACKS[t][0] for t in ini], [owners.index(t) for t in ini]
        put("ini_slot", f, slots)
        put("ini_det", f, dets)
        out["ini_n"][f - 1] = len(slots)
        for t, s, j in zip(ini, slots, dets):
            if np.any(mean[s] != 0):
                assert t == "G" and f == 10
                seen.add("reused")
            mean[s], cov[s] = kf.initiate(out["meas"][f - 1, j])
        out["mean"][f - 1, 2], out["cov"][f - 1, 2] = mean, cov

    # ---- what the script must contain
    assert seen == {"zeroed", "unconfirmed", "found again", "reused"}, seen
    assert [f + 1 for f in range(FRAMES) if out["ini_n"][f]] == [1, 3, 9, 10]
    b = TRACKS["B"][0]
    for f in (5, 6, 7, 8):
        assert b not in out["upd_slot"][f - 1] and b in out["pred_slot"][f - 1]
    assert [int(out["pred_nt"][f - 1, list(out["pred_slot"][f - 1]).index(b)]) for f in (5, 6, 7, 8, 9, 10)] == [0, 1, 1, 1, 1, 0]
    assert out["mean"][6 - 1, 0, b, 7] == 0.0 and out["mean"][5 - 1, 0, b, 7] != 0.0
    e = TRACKS["E"][0]
    assert all(e not in out[k][f - 1] for k in ("pred_slot", "upd_slot", "ini_slot") for f in (6, 7, 8, 9)) and e in out["ini_slot"][10 - 1]
    live = [out["pred_slot"][f][:out["pred_n"][f]] for f in range(FRAMES)]
    assert any(len(s) > 2 and (np.diff(s) < 0).any() and (np.diff(s) > 0).any() for s in live)           # neither ascending nor descending
    for f in range(FRAMES):
        k = out["upd_n"][f]
        if k:
            assert out["meas_m"][f] > k and not np.array_equal(out["upd_det"][f, :k], np.arange(k))
    assert out["meas_m"][NO_DETECTION - 1] == 0 and out["upd_n"][NO_DETECTION - 1] == 0 and out["pred_n"][NO_DETECTION - 1] > 0
    assert (out["pred_slot"][MINUS_ONE - 1] == -1).sum() == 1 and (out["upd_slot"][MINUS_ONE - 1] == -1).sum() == 1
    assert np.isfinite(out["mean"]).all() and np.isfinite(out["cov"]).all()
    return out


def main():
    out = make(load_kalman())
    path = os.path.join(OUT, "kalman_store.npz")
    np.savez_compressed(path, **out)
    print("wrote kalman_store.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
