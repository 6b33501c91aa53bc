#!/usr/bin/env python3
"""Generate tests/golden/ghost_motion.npz, the fixture of tests/test_ghost_motion.py.  Run from the repo root where the reference is present:

    python tests/golden/make_golden_ghost_motion.py

The fixture holds arrays only.  Every recorded value comes from the reference's own code (adapters/GHOST/src/tracking_utils.py: Track, warp_pos,
bbox_overlaps; src/base_tracker.py: BaseTracker.motion, motion_step, motion_compensation, get_motion_dist), loaded through
make_golden_ghost.load_reference() and called unbound on a SimpleNamespace.  motion_compensation estimates its warp with cv2.findTransformECC; here
findTransformECC, cvtColor and the constants it reads are set on the imported cv2 stand-in module at run time so that it returns the next scripted
warp - the loop over the tracks that follows is the reference's own.

Two scripted sequences of 8 tracks (slot = track id) over 12 frames whose numbers have gaps of 1 .. 3, with 5 .. 7 detections a frame (the visible
objects in a scripted shuffle plus false positives that match nothing).  Matches are scripted: track k follows object k.  Tracks 1, 2, 3, 4 and 6 go
inactive (3 for good, 4 with a single position) and all but 3 come back, tracks 6 and 7 start mid-sequence, track 5 never gets a second position.
  static   fixed camera, float64 boxes, last_n_frames 3, no warp;  rings of H = 4 rows, which wrap
  moving   moving camera, float64 boxes, last_n_frames 100000000 (all), another near-identity warp before every frame but the first;  H = 16
A frame runs the reference's order: motion_compensation (moving), motion() + get_motion_dist, then the scripted add_detection / new Track calls.

Per sequence <q> in (static, moving), F = 12 frames, S = 8 slots:
  <q>_frame [F]                 frame numbers;  <q>_params [2] = H, last_n_frames
  <q>_hist [F,4,S,H,4] f64, <q>_frames [F,4,S,H] i32, <q>_count / <q>_newest [F,4,S] i32, <q>_pos / <q>_vel [F,4,S,4] f64
                                the reference's full state at four stages of every frame: 0 before the warp, 1 before motion() (= 0 for static),
                                2 before the adds, 3 after them (= stage 0 of the next frame).  Sample q of a track sits in ring row q mod H, what an
                                append from an empty ring gives; rows that hold nothing are zero.
  <q>_f32 [F,S] u8              1 = every stored row of the track was a float32 array when motion() ran (numpy's dtype rule for the difference)
  <q>_nmk [F,3] i32             per frame: n tracks, m detections, k adds;  <q>_na [F]: how many of the n tracks are active
  <q>_slots [F,S] i32           the n tracks of the frame in the reference's order, active ones first (-1 beyond n)
  <q>_dets [F,7,4] f64          the m detections' boxes (zero beyond m)
  <q>_dist [F,7,S] f64          get_motion_dist, the reference's [detections, tracks], in the leading [m,n] (NaN beyond)
  <q>_add [F,S,3] i32           the frame's k adds: slot, detection index, 1 = a new track (-1 beyond k)
  moving_warp [F,6] f32         the warp applied before frame f (row 0 unused: identity);  warp_err [1]: the largest difference between a float64
                                evaluation of W . (x, y, 1) on the stored float64 values and the reference's float32 output

The generator asserts that a sequential float64 restatement (oldest pair first, one divide per pair, one divide by the pair count) reproduces every
`static` velocity and position bit for bit, that every window is float64 in `static` and float32 in `moving` when motion() runs, and that
oracle.geometry.iou_distance(pos, dets) is the recorded motion distance transposed, bit for bit.  The file is written with fixed zip timestamps: two
runs give the same bytes."""
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from busca_amd import synth  # noqa: E402
from make_golden_ghost import load_reference  # noqa: E402
from oracle import geometry as og  # noqa: E402

S = 8
FRAMES = [1, 2, 4, 5, 8, 9, 10, 12, 15, 16, 18, 19]
VISIBLE = {0: range(12), 1: [0, 1, 2, 3, 6, 7, 8, 9, 10, 11], 2: [0, 1, 3, 4, 5, 6, 9, 10, 11], 3: range(6), 4: [0, 3, 4, 5, 6, 7, 8, 9, 10, 11], 5: [0],
           6: [4, 5, 6, 7, 9, 10, 11], 7: range(6, 12)}
FALSE_POS = [0, 1, 2, 1, 0, 1, 0, 1, 1, 0, 1, 0]
SEQS = [("static", 500, 4, 3, False), ("moving", 501, 16, 100000000, True)]


def objects(seed, moving):
    """Box of object k at frame number t: linear motion, a size that breathes, and the camera's drift when it moves."""
    cx0 = synth.uniform(seed, "cx", (S,), 200, 1700).astype(np.float64)
    cy0 = synth.uniform(seed, "cy", (S,), 200, 900).astype(np.float64)
    v = synth.uniform(seed, "v", (S, 2), -6, 6).astype(np.float64)
    h0 = synth.uniform(seed, "h", (S,), 80, 300).astype(np.float64)
    ar = synth.uniform(seed, "ar", (S,), 0.3, 0.5).astype(np.float64)

    def box(k, f, t):
        jit = synth.uniform(seed, "jit_%d_%d" % (k, f), (4,), -1.5, 1.5).astype(np.float64)
        cx, cy = cx0[k] + v[k, 0] * t + (3.0 * t if moving else 0.0), cy0[k] + v[k, 1] * t - (1.5 * t if moving else 0.0)
        h = h0[k] * (1.0 + 0.01 * t)
        w = h * ar[k]
        return np.array([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], dtype=np.float64) + jit
    return box


def frame_script(seed, f, box):
    """-> (dets [m,4] float64, {object: detection index}): the visible objects and the false positives, shuffled."""
    vis = [k for k in range(S) if f in VISIBLE[k]]
    rows = [box(k, f, FRAMES[f]) for k in vis]
    for j in range(FALSE_POS[f]):
        c = synth.uniform(seed, "fp_%d_%d" % (f, j), (4,), 0, 1).astype(np.float64)
        x, y, w, h = 100 + 1600 * c[0], 100 + 800 * c[1], 40 + 80 * c[2], 90 + 200 * c[3]
        rows.append(np.array([x, y, x + w, y + h], dtype=np.float64))
    order = np.argsort(synth.uniform(seed, "order_%d" % f, (len(rows),), 0, 1), kind="stable")
    dets = np.stack([rows[i] for i in order])
    where = {int(i): j for j, i in enumerate(order)}
    assert 5 <= len(dets) <= 7
    return dets, {k: where[i] for i, k in enumerate(vis)}


def snapshot(tracks, H):
    """The reference's state of every track as the six arrays, sample q in ring row q mod H."""
    st = dict(hist=np.zeros((S, H, 4)), frames=np.zeros((S, H), np.int32), count=np.zeros(S, np.int32), newest=np.zeros(S, np.int32),
              pos=np.zeros((S, 4)), vel=np.zeros((S, 4)))
    for k, t in tracks.items():
        n = len(t.last_pos)
        assert len(t.past_frames) == n
        for q in range(max(0, n - H), n):
            st["hist"][k, q % H] = np.asarray(t.last_pos[q], dtype=np.float64)
            st["frames"][k, q % H] = t.past_frames[q]
        st["count"][k], st["newest"][k] = min(n, H), (n - 1) % H
        st["pos"][k], st["vel"][k] = np.asarray(t.pos, dtype=np.float64), np.asarray(t.last_v, dtype=np.float64)
    return st


def restate_step(t, last_n, active, diff32):
    """motion() for one track in sequential float64 (diff32: the difference of two positions in float32) -> (pos, vel)."""
    pos, vel = np.asarray(t.pos, dtype=np.float64).copy(), np.asarray(t.last_v, dtype=np.float64).copy()
    if len(t.last_pos) > 1:
        if active:
            P, Fr = [np.asarray(p, dtype=np.float64) for p in t.last_pos[-last_n:]], t.past_frames[-last_n:]
            for c in range(4):
                acc = None
                for i in range(len(P) - 1):
                    d = np.float64(np.float32(P[i + 1][c]) - np.float32(P[i][c])) if diff32 else P[i + 1][c] - P[i][c]
                    q = d / np.float64(Fr[i + 1] - Fr[i])
                    acc = q if acc is None else acc + q
                vel[c] = acc / np.float64(len(P) - 1)
        pos = pos + vel
    return pos, vel


def run(tu, Base, name, seed, H, last_n, moving, out):
    import cv2
    box = objects(seed, moving)
    mcfg = {"center_only": False, "last_n_frames": last_n, "motion_compensation": True, "num_iter_mc": 100, "termination_eps_mc": 1e-5,
            "warp_mode": "Euclidean", "apply_motion_model": True, "combi": "sum_0.4"}
    ns = types.SimpleNamespace(motion_model_cfg=mcfg, warp_mode_dct={"Euclidean": 0}, is_moving=moving, tracks={}, inactive_tracks={}, i=1,
                               last_image=torch.zeros(3, 4, 4), warp_matrix_nomr=None)
    ns.motion_step = lambda t: Base.motion_step(ns, t)
    warps = np.zeros((len(FRAMES), 6), np.float32)
    warps[:, [0, 4]] = 1.0
    script = {}
    cv2.COLOR_RGB2GRAY, cv2.TERM_CRITERIA_EPS, cv2.TERM_CRITERIA_COUNT = 7, 2, 1
    cv2.cvtColor = lambda im, code: im[..., 0]
    cv2.findTransformECC = lambda a, b, w, mode, crit, mask, gauss: (1.0, script["warp"].copy())
    stages = {k: [] for k in ("hist", "frames", "count", "newest", "pos", "vel")}
    F = len(FRAMES)
    per = dict(slots=np.full((F, S), -1, np.int32), dets=np.zeros((F, 7, 4)), dist=np.full((F, 7, S), np.nan), add=np.full((F, S, 3), -1, np.int32),
               nmk=np.zeros((F, 3), np.int32))
    f32, nas, warp_err = np.zeros((len(FRAMES), S), np.uint8), [], 0.0
    everyone = lambda: dict(list(ns.tracks.items()) + list(ns.inactive_tracks.items()))

    def record():
        st = snapshot(everyone(), H)
        for k in stages:
            stages[k].append(st[k])
    for f, fr in enumerate(FRAMES):
        dets, where = frame_script(seed, f, box)
        record()                                                          # stage 0
        if moving and f > 0:
            a = synth.uniform(seed, "warp_%d" % f, (6,), -1, 1).astype(np.float64)
            W = np.array([[1 + 0.01 * a[0], 0.01 * a[1], 6 * a[2]], [0.01 * a[3], 1 + 0.01 * a[4], 6 * a[5]]], dtype=np.float32)
            warps[f], script["warp"] = W.reshape(6), W
            before = {k: [np.asarray(p, dtype=np.float64) for p in t.last_pos] for k, t in everyone().items()}
            Base.motion_compensation(ns, torch.zeros(3, 4, 4), f)
            W64 = W.astype(np.float64)
            for k, t in everyone().items():
                for p0, p1 in zip(before[k], t.last_pos):
                    assert p1.dtype == np.float32 and p1.shape == (4,)
                    want = np.concatenate([W64 @ np.array([p0[0], p0[1], 1.0]), W64 @ np.array([p0[2], p0[3], 1.0])])
                    warp_err = max(warp_err, float(np.abs(want - p1).max()))
        record()                                                          # stage 1
        ids, na = list(ns.tracks) + list(ns.inactive_tracks), len(ns.tracks)
        for k, t in everyone().items():
            kinds = {np.asarray(p).dtype for p in t.last_pos}
            f32[f, k] = kinds == {np.dtype(np.float32)}
            assert len(t.last_pos) < 2 or kinds == ({np.dtype(np.float32)} if moving else {np.dtype(np.float64)}), (name, f, k, kinds)
        want = {k: restate_step(t, last_n, k in ns.tracks, moving) for k, t in everyone().items()}
        Base.motion(ns)
        dist = np.zeros((len(dets), 0))                                   # (the reference runs no round without tracks)
        if ids:
            dist = Base.get_motion_dist(ns, [{"bbox": d} for d in dets], ns.inactive_tracks).numpy()
        for k, t in everyone().items():
            assert np.asarray(t.pos).dtype == np.float64
            assert np.array_equal(want[k][0], t.pos) and np.array_equal(want[k][1], np.asarray(t.last_v, dtype=np.float64)), (name, f, k)
        pos = np.array([everyone()[k].pos for k in ids], dtype=np.float64).reshape(-1, 4)
        assert dist.shape == (len(dets), len(ids)) and dist.dtype == np.float64
        if ids:
            assert np.array_equal(og.iou_distance(pos, dets).T, dist)
        record()                                                          # stage 2
        add_slot, add_det, add_new = [], [], []
        for k in list(ns.tracks) + list(ns.inactive_tracks):              # matches: active tracks, then reactivated ones
            if k in where:
                if k in ns.inactive_tracks:
                    ns.tracks[k] = ns.inactive_tracks.pop(k)
                ns.tracks[k].add_detection(dets[where[k]].copy(), None, f, k, 1.0, 0.9, fr, 0)
                add_slot.append(k), add_det.append(where[k]), add_new.append(0)
        for k in [k for k in ns.tracks if k not in where]:
            ns.inactive_tracks[k] = ns.tracks.pop(k)
        for k in sorted(where, key=lambda k: where[k]):                   # unmatched detections of objects start tracks, in detection order
            if k not in ns.tracks:
                ns.tracks[k] = tu.Track(k, dets[where[k]].copy(), None, f, k, 1.0, 0.9, fr, 0)
                add_slot.append(k), add_det.append(where[k]), add_new.append(1)
        record()                                                          # stage 3
        n, m, k = len(ids), len(dets), len(add_slot)
        per["slots"][f, :n], per["dets"][f, :m], per["dist"][f, :m, :n] = ids, dets, dist
        per["add"][f, :k] = np.stack([add_slot, add_det, add_new], 1)
        per["nmk"][f] = n, m, k
        nas.append(na)
    for k, v in stages.items():
        a = np.stack(v).reshape((len(FRAMES), 4) + v[0].shape)
        out["%s_%s" % (name, k)] = a
    out[name + "_na"] = np.array(nas, dtype=np.int32)
    out.update({"%s_%s" % (name, k): v for k, v in per.items()})
    out[name + "_frame"] = np.array(FRAMES, dtype=np.int32)
    out[name + "_params"] = np.array([H, last_n], dtype=np.int64)
    out[name + "_f32"] = f32
    if moving:
        out["moving_warp"], out["warp_err"] = warps, np.array([warp_err])
    return warp_err


def write_npz(path, arrays):
    """np.load-compatible, with fixed timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    tu, Base, _ = load_reference()
    out = {}
    for name, seed, H, last_n, moving in SEQS:
        err = run(tu, Base, name, seed, H, last_n, moving, out)
        cnt = out[name + "_count"]
        print("%-6s: H %2d, last_n %d, tracks per frame %s (active %s), longest history %d rows, warp_err %.3g"
              % (name, H, last_n, out[name + "_nmk"][:, 0].tolist(), out[name + "_na"].tolist(), int(cnt.max()), err))
    assert 0.0 < float(out["warp_err"][0]) < 1e-3
    path = os.path.join(OUT, "ghost_motion.npz")
    write_npz(path, out)
    print("wrote ghost_motion.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 64 << 10                               # four full states a frame; most of it is `moving` with H = 16


if __name__ == "__main__":
    main()
