#!/usr/bin/env python3
"""Generate tests/golden/kalman.npz by running the reference's vendored KalmanFilter (adapters/CenterTrack/src/lib/utils/
mot_online/kalman_filter.py, the copy adapters/ByteTrack/yolox/tracker/byte_tracker.py:15 falls back to), loaded by path as
make_golden.py's make_track does.  Run from the repo root where the reference is present:

    python tests/golden/make_golden_kalman.py

The fixture holds arrays only: seeded inputs and the reference's outputs.

  mean, cov [96]                    predicted states after a 1-40 step predict/update history (heights 20-900 px, aspect 0.2-1.2)
  meas, upd_mean, upd_cov           one measurement per track and KalmanFilter.update of it
  chain_*                           8 tracks x 20 steps of multi_predict + update: every intermediate state and the measurements
  init_meas, init_mean, init_cov    64 KalmanFilter.initiate inputs and outputs
  gate_meas [40,4], gate_{maha,gauss}{4,2} [96,40]   KalmanFilter.gating_distance, only_position False (4) / True (2)
  tlwh, tlbr [96,4]                 STrack.tlwh / tlbr of `mean`.  UNPINNED: byte_tracker.py needs the tracker's whole environment
                                    (cython_bbox, lap, torch models) and cannot be imported here, so these are its formula
                                    (byte_tracker.py:142-163) restated in numpy, not its output.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

from busca_amd import synth  # noqa: E402

SEED = 57
N, N_CHAIN, STEPS, N_INIT, M = 96, 8, 20, 64, 40


def load_kalman():
    spec = importlib.util.spec_from_file_location("ref_kalman_filter", os.path.join(REF, "adapters/CenterTrack/src/lib/utils/mot_online/kalman_filter.py"))
    kfm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kfm)
    return kfm


def boxes(tag, n):
    """(x, y, a, h): centres inside a 1920 x 1080 frame, heights 20-900 px, aspect ratios 0.2-1.2."""
    return np.stack([synth.uniform(SEED, tag + "x", (n,), 50, 1870), synth.uniform(SEED, tag + "y", (n,), 50, 1030),
                     synth.uniform(SEED, tag + "a", (n,), 0.2, 1.2), synth.uniform(SEED, tag + "h", (n,), 20, 900)], 1).astype(np.float64)


def noisy(z0, vel, step, noise):
    """Measurement `step` frames down a straight path, jittered by `noise` (4 values in -1..1) scaled to the box height."""
    h = z0[3]
    return np.array([z0[0] + vel[0] * step + 0.03 * h * noise[0], z0[1] + vel[1] * step + 0.03 * h * noise[1],
                     z0[2] * (1.0 + 0.02 * noise[2]), h * (1.0 + 0.004 * step + 0.02 * noise[3])], dtype=np.float64)


def main():
    kfm = load_kalman()
    kf = kfm.KalmanFilter()
    out = {}

    # ---- 96 tracks with a history, one update each ------------------------------------------------------------------
    z0 = boxes("t", N)
    hist = synth.uniform(SEED, "hist", (N,), 1, 41).astype(int).clip(1, 40)
    vel = np.stack([synth.uniform(SEED, "vx", (N,), -0.04, 0.04), synth.uniform(SEED, "vy", (N,), -0.02, 0.02)], 1) * z0[:, 3:4]
    noise = synth.uniform(SEED, "noise", (N, 42, 4), -1, 1)
    means, covs, meas, um, uc = [], [], [], [], []
    for i in range(N):
        m, c = kf.initiate(z0[i])
        for s in range(int(hist[i])):
            m, c = kf.predict(m, c)
            m, c = kf.update(m, c, noisy(z0[i], vel[i], s + 1, noise[i, s]))
        m, c = kf.predict(m, c)
        z = noisy(z0[i], vel[i], int(hist[i]) + 1, noise[i, 41])
        m2, c2 = kf.update(m, c, z)
        means.append(m); covs.append(c); meas.append(z); um.append(m2); uc.append(c2)
    mean, cov = np.asarray(means), np.asarray(covs)
    out.update(mean=mean, cov=cov, hist=hist, meas=np.asarray(meas), upd_mean=np.asarray(um), upd_cov=np.asarray(uc))
    assert hist.min() <= 3 and hist.max() >= 38

    # ---- chained run: STrack.multi_predict + update, 8 tracks x 20 steps ----------------------------------------------
    c0 = boxes("c", N_CHAIN)
    cvel = np.stack([synth.uniform(SEED, "cvx", (N_CHAIN,), -0.04, 0.04), synth.uniform(SEED, "cvy", (N_CHAIN,), -0.02, 0.02)], 1) * c0[:, 3:4]
    cnoise = synth.uniform(SEED, "cnoise", (N_CHAIN, STEPS, 4), -1, 1)
    init = [kf.initiate(c0[i]) for i in range(N_CHAIN)]
    cm, cc = np.asarray([a for a, _ in init]), np.asarray([b for _, b in init])
    out.update(chain_mean0=cm, chain_cov0=cc)
    cz = np.zeros((STEPS, N_CHAIN, 4))
    pms, pcs, ums, ucs = [], [], [], []
    for s in range(STEPS):
        cm, cc = kf.multi_predict(cm, cc)
        pms.append(cm); pcs.append(cc)
        nm, nc = [], []
        for i in range(N_CHAIN):
            cz[s, i] = noisy(c0[i], cvel[i], s + 1, cnoise[i, s])
            a, b = kf.update(cm[i], cc[i], cz[s, i])
            nm.append(a); nc.append(b)
        cm, cc = np.asarray(nm), np.asarray(nc)
        ums.append(cm); ucs.append(cc)
    out.update(chain_meas=cz, chain_pred_mean=np.asarray(pms), chain_pred_cov=np.asarray(pcs), chain_upd_mean=np.asarray(ums),
               chain_upd_cov=np.asarray(ucs))

    # ---- initiate ---------------------------------------------------------------------------------------------------
    iz = boxes("i", N_INIT)
    init = [kf.initiate(iz[i]) for i in range(N_INIT)]
    out.update(init_meas=iz, init_mean=np.asarray([a for a, _ in init]), init_cov=np.asarray([b for _, b in init]))

    # ---- gating: 40 measurements, each scattered around one of the tracks -----------------------------------------------
    owner = (np.arange(M) * 7) % N
    gn = synth.uniform(SEED, "gnoise", (M, 4), -1, 1)
    gz = mean[owner, :4].copy()
    hh = mean[owner, 3]
    gz[:, 0] += 0.18 * hh * gn[:, 0]
    gz[:, 1] += 0.18 * hh * gn[:, 1]
    gz[:, 2] *= 1.0 + 0.1 * gn[:, 2]
    gz[:, 3] *= 1.0 + 0.1 * gn[:, 3]
    out["gate_meas"] = gz
    for only_position, dim in ((False, 4), (True, 2)):
        for metric, tag in (("maha", "maha"), ("gaussian", "gauss")):
            g = np.asarray([kf.gating_distance(mean[i], cov[i], gz, only_position, metric) for i in range(N)])
            assert g.shape == (N, M) and np.isfinite(g).all()
            out["gate_%s%d" % (tag, dim)] = g
        thr = kfm.chi2inv95[dim]
        g = out["gate_maha%d" % dim]
        # no knife-edge entry: the gate decides the same way for every float64 evaluation order of the distance
        assert np.abs(g - thr).min() > 1e-9, np.abs(g - thr).min()
        inside = int((g <= thr).sum())
        assert 30 <= inside <= N * M - 30, inside
        print("gating dim %d: %d of %d entries inside the gate, closest to the threshold %.3g" % (dim, inside, N * M, np.abs(g - thr).min()))
    out["chi2inv95"] = np.array([kfm.chi2inv95[2], kfm.chi2inv95[4]])

    # ---- STrack.tlwh / tlbr (byte_tracker.py:142-163), restated: see the module docstring ---------------------------------
    tlwh = mean[:, :4].copy()
    tlwh[:, 2] *= tlwh[:, 3]
    tlwh[:, :2] -= tlwh[:, 2:] / 2
    tlbr = tlwh.copy()
    tlbr[:, 2:] += tlbr[:, :2]
    out.update(tlwh=tlwh, tlbr=tlbr)

    path = os.path.join(OUT, "kalman.npz")
    np.savez_compressed(path, **out)
    print("wrote kalman.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
