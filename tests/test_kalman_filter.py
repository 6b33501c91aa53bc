"""ByteTrack's Kalman filter on the device: measurement update, initiate, state -> box, gating distances, and the mirrors of
busca_amd.tracking built on them (multi_update, multi_initiate, gating_distance, gate_cost_matrix, fuse_motion, predicted_cost).

The reference is tests/golden/kalman.npz, written by tests/golden/make_golden_kalman.py from the reference's vendored
KalmanFilter (adapters/CenterTrack/src/lib/utils/mot_online/kalman_filter.py).  The checker is the plain-numpy restatement
below - no LAPACK: a hand-written 4x4 Cholesky factorisation with forward and back substitution, every sum left to right.

update and gating_distance go through LAPACK in the reference, so neither the restatement nor the kernels reproduce its
bits: all three are valid float64 evaluation orders of the same formulas.  How far two such orders drift apart is measured
here, on the fixture, as the restatement's worst disagreement with the reference:

    mean        max |d| / max(1, |ref|)                      1.73e-15   (96 single updates)
    covariance  max |d| / max |ref covariance|, per matrix   1.68e-15
    gating      max |d| / max(1, |ref|)                      6.62e-16   (96 x 40, all four modes)
    8 x 20 chained multi_predict + update: mean 2.39e-14, covariance 2.21e-15

Each GPU bar is 20 x the corresponding value, computed from the fixture by `bars()` at run time and never from a kernel's
output: the kernels' order is a third valid one, and 20 x leaves room for it without hiding a wrong formula, which errs at
1e-3 or worse.  initiate and the box conversion are sums and products numpy evaluates in a fixed order: bit-exact."""
import math
import os
import re
import types

import numpy as np
import pytest

from oracle import bytetrack as obt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kalman.npz")
NEW_SYMBOLS = ("busca_kalman_update", "busca_kalman_initiate", "busca_kalman_boxes", "busca_kalman_gating")
CHI2 = {2: 5.9915, 4: 9.4877}
MODES = [(False, "maha"), (False, "gaussian"), (True, "maha"), (True, "gaussian")]


# ---- the restatement ----------------------------------------------------------------------------------------------------
def r_project(mean, cov):
    """Innovation covariance S = P[:4,:4] + diag(std^2), kalman_filter.py:125-152."""
    h = float(mean[3])
    std = [(1.0 / 20) * h, (1.0 / 20) * h, 1e-1, (1.0 / 20) * h]
    S = [[float(cov[i][j]) + (std[i] * std[i] if i == j else 0.0) for j in range(4)] for i in range(4)]
    return S


def r_cholesky(S, dim):
    """Lower Cholesky factor of the leading dim x dim block, or None at a pivot that is not positive and finite."""
    L = [[0.0] * 4 for _ in range(4)]
    for j in range(dim):
        d = S[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not (d > 0.0) or math.isinf(d):
            return None
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, dim):
            v = S[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    return L


def r_update(mean, cov, z):
    """KalmanFilter.update, kalman_filter.py:193-225.  None where the reference raises LinAlgError."""
    S = r_project(mean, cov)
    L = r_cholesky(S, 4)
    if L is None:
        return None
    K = [[0.0] * 4 for _ in range(8)]
    for r in range(8):                                   # S x = P[r,:4]^T: forward, then back substitution
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
    KS = [[((K[i][0] * S[0][k] + K[i][1] * S[1][k]) + K[i][2] * S[2][k]) + K[i][3] * S[3][k] for k in range(4)] for i in range(8)]
    new_cov = np.array([[float(cov[i][j]) - (((KS[i][0] * K[j][0] + KS[i][1] * K[j][1]) + KS[i][2] * K[j][2]) + KS[i][3] * K[j][3])
                         for j in range(8)] for i in range(8)])
    return new_mean, new_cov


def r_gating(mean, cov, meas, only_position, metric):
    """KalmanFilter.gating_distance, kalman_filter.py:227-269, of one track against meas [m,4]."""
    dim = 2 if only_position else 4
    d = [meas[:, i] - float(mean[i]) for i in range(dim)]
    if metric == "maha":
        L = r_cholesky(r_project(mean, cov), dim)
        if L is None:
            return np.full(meas.shape[0], np.nan)
        z = []
        for i in range(dim):
            v = d[i]
            for k in range(i):
                v = v - L[i][k] * z[k]
            z.append(v / L[i][i])
        d = z
    s = d[0] * d[0]
    for i in range(1, dim):
        s = s + d[i] * d[i]
    return s


def r_initiate(z):
    """KalmanFilter.initiate, kalman_filter.py:54-85, of z [n,4]."""
    h = z[:, 3]
    wp, wv = 1.0 / 20, 1.0 / 160
    std = np.stack([2 * wp * h, 2 * wp * h, np.full_like(h, 1e-2), 2 * wp * h, 10 * wv * h, 10 * wv * h, np.full_like(h, 1e-5), 10 * wv * h], 1)
    cov = np.zeros((len(z), 8, 8))
    cov[:, np.arange(8), np.arange(8)] = np.square(std)
    return np.concatenate([z, np.zeros_like(z)], 1), cov


def r_boxes(mean, tlbr):
    """STrack.tlwh / tlbr, byte_tracker.py:142-163."""
    ret = mean[:, :4].copy()
    ret[:, 2] *= ret[:, 3]
    ret[:, :2] -= ret[:, 2:] / 2
    if tlbr:
        ret[:, 2:] += ret[:, :2]
    return ret


# ---- the three error measures ---------------------------------------------------------------------------------------------
def err_mean(got, ref):
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def err_cov(got, ref):
    got, ref = got.reshape(-1, 8, 8), ref.reshape(-1, 8, 8)
    return float((np.abs(got - ref).max(axis=(1, 2)) / np.abs(ref).max(axis=(1, 2))).max())


err_gate = err_mean


_CACHE = {}


def gold():
    if "g" not in _CACHE:
        with np.load(GOLD) as f:
            _CACHE["g"] = {k: f[k] for k in f.files}
    return _CACHE["g"]


def gate_key(only_position, metric):
    return "gate_%s%d" % ("maha" if metric == "maha" else "gauss", 2 if only_position else 4)


def bars():
    """The restatement's worst disagreement with the reference over the fixture (computed once), and 20 x it."""
    if "bars" in _CACHE:
        return _CACHE["bars"]
    g = gold()
    up = [r_update(g["mean"][i], g["cov"][i], g["meas"][i]) for i in range(len(g["mean"]))]
    v = {"mean": err_mean(np.stack([m for m, _ in up]), g["upd_mean"]), "cov": err_cov(np.stack([c for _, c in up]), g["upd_cov"])}
    v["gate"] = max(err_gate(np.stack([r_gating(g["mean"][i], g["cov"][i], g["gate_meas"], op, mt) for i in range(len(g["mean"]))]),
                             g[gate_key(op, mt)]) for op, mt in MODES)
    # the chained run: the oracle's multi_predict (bit-exact against the reference) + the restated update, fed with their own output
    m, c = g["chain_mean0"], g["chain_cov0"]
    cm, cc = 0.0, 0.0
    for s in range(g["chain_meas"].shape[0]):
        m, c = obt.kalman_multi_predict(m, c)
        up = [r_update(m[i], c[i], g["chain_meas"][s, i]) for i in range(len(m))]
        m, c = np.stack([a for a, _ in up]), np.stack([b for _, b in up])
        cm, cc = max(cm, err_mean(m, g["chain_upd_mean"][s])), max(cc, err_cov(c, g["chain_upd_cov"][s]))
    v["chain_mean"], v["chain_cov"] = cm, cc
    _CACHE["bars"] = (v, {k: 20.0 * x for k, x in v.items()})
    return _CACHE["bars"]


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_fixture_contents():
    g = gold()
    assert g["mean"].shape == (96, 8) and g["cov"].shape == (96, 8, 8) and g["meas"].shape == (96, 4)
    assert g["hist"].min() >= 1 and g["hist"].max() <= 40
    assert g["mean"][:, 3].min() < 60 and g["mean"][:, 3].max() > 800
    assert g["chain_meas"].shape == (20, 8, 4) and g["chain_upd_cov"].shape == (20, 8, 8, 8) and g["chain_pred_mean"].shape == (20, 8, 8)
    assert g["init_meas"].shape == (64, 4) and g["gate_meas"].shape == (40, 4)
    for dim in (2, 4):
        gm = g["gate_maha%d" % dim]
        assert gm.shape == (96, 40) and np.abs(gm - CHI2[dim]).min() > 1e-9          # no knife-edge entry at the gate
        assert (gm > CHI2[dim]).sum() >= 30 and (gm <= CHI2[dim]).sum() >= 30
    assert os.path.getsize(GOLD) < 1 << 20


def test_restatement_reproduces_the_fixture():
    g = gold()
    v, bar = bars()
    print("restatement vs reference: mean %.3g  covariance %.3g  gating %.3g  chained mean %.3g  chained covariance %.3g"
          % (v["mean"], v["cov"], v["gate"], v["chain_mean"], v["chain_cov"]))
    # two float64 orders of ~100 operations on factors whose condition numbers reach ~1e3: far below 1e-11; a wrong formula: >= 1e-3
    assert all(x < 1e-11 for x in v.values()), v
    assert all(bar[k] == 20.0 * v[k] for k in v)
    # the chained prediction the update is fed with is the reference's, bit for bit
    m, c = obt.kalman_multi_predict(g["chain_mean0"], g["chain_cov0"])
    assert np.array_equal(m, g["chain_pred_mean"][0]) and np.array_equal(c, g["chain_pred_cov"][0])
    # initiate and the boxes are bit-exact
    im, ic = r_initiate(g["init_meas"])
    assert np.array_equal(im, g["init_mean"]) and np.array_equal(ic, g["init_cov"])
    assert np.array_equal(r_boxes(g["mean"], False), g["tlwh"]) and np.array_equal(r_boxes(g["mean"], True), g["tlbr"])
    # a covariance that is not positive definite: no update, NaN distances
    bad = g["cov"][5].copy()
    bad[:4, :4] = -np.eye(4)
    assert r_update(g["mean"][5], bad, g["meas"][5]) is None
    assert np.isnan(r_gating(g["mean"][5], bad, g["gate_meas"], False, "maha")).all()


def test_new_symbols_declared_typed_and_exported():
    from busca_amd.build import build
    build()
    from busca_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "busca_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(busca_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert len(declared) == 37 and declared == set(_lib.SIGNATURES)


def test_measurements_of_detections():
    from busca_amd import tracking
    g = gold()
    tlwh = g["tlwh"][:7]
    want = []
    for b in tlwh:                                       # STrack.tlwh_to_xyah, byte_tracker.py:165-172
        ret = np.asarray(b).copy()
        ret[:2] += ret[2:] / 2
        ret[2] /= ret[3]
        want.append(ret)
    assert np.array_equal(tracking.tlwh_to_xyah(tlwh), np.stack(want))
    assert tracking.tlwh_to_xyah([]).shape == (0, 4)
    assert tracking.CHI2INV95 == {2: float(g["chi2inv95"][0]), 4: float(g["chi2inv95"][1])} == CHI2


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from busca_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _stream():
    import torch
    return torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream


def gpu_update(ctx, mean, cov, meas):
    import torch
    m, c, z = _dev(mean), _dev(cov), _dev(meas)
    st = torch.full((len(mean),), -7, dtype=torch.int32, device=m.device)
    ctx.check(ctx.lib.busca_kalman_update(ctx.h, m.data_ptr(), c.data_ptr(), z.data_ptr(), len(mean), st.data_ptr(), _stream()))
    return m.cpu().numpy(), c.cpu().numpy(), st.cpu().numpy()


def gpu_gating(ctx, mean, cov, meas, only_position, metric):
    import torch
    m, c, z = _dev(mean), _dev(cov), _dev(meas)
    out = torch.full((len(mean), len(meas)), -7.0, dtype=torch.float64, device=m.device)
    st = torch.full((len(mean),), -7, dtype=torch.int32, device=m.device)
    ctx.check(ctx.lib.busca_kalman_gating(ctx.h, m.data_ptr(), c.data_ptr(), len(mean), z.data_ptr(), len(meas), int(only_position),
                                          0 if metric == "maha" else 1, out.data_ptr(), st.data_ptr(), _stream()))
    return out.cpu().numpy(), st.cpu().numpy()


def _tracks(mean, cov, states=None):
    return [types.SimpleNamespace(mean=mean[i].copy(), covariance=cov[i].copy(), state=1 if states is None else int(states[i]))
            for i in range(len(mean))]


def _detections(xyah, scores=None):
    """Detection objects whose tlwh gives back (almost) the measurement xyah."""
    out = []
    for k, z in enumerate(xyah):
        w = z[2] * z[3]
        tlwh = np.array([z[0] - w / 2, z[1] - z[3] / 2, w, z[3]])
        out.append(types.SimpleNamespace(tlwh=tlwh, tlbr=np.array([tlwh[0], tlwh[1], tlwh[0] + tlwh[2], tlwh[1] + tlwh[3]]),
                                         score=None if scores is None else float(scores[k])))
    return out


@pytest.mark.gpu
def test_update_meets_the_bars(ctx):
    g = gold()
    _, bar = bars()
    m, c, st = gpu_update(ctx, g["mean"], g["cov"], g["meas"])
    em, ec = err_mean(m, g["upd_mean"]), err_cov(c, g["upd_cov"])
    print("update: mean %.3g (bar %.3g)  covariance %.3g (bar %.3g)" % (em, bar["mean"], ec, bar["cov"]))
    assert (st == 0).all()
    assert em <= bar["mean"] and ec <= bar["cov"]
    # status may be NULL
    m2, c2 = _dev(g["mean"]), _dev(g["cov"])
    ctx.check(ctx.lib.busca_kalman_update(ctx.h, m2.data_ptr(), c2.data_ptr(), _dev(g["meas"]).data_ptr(), 96, None, _stream()))
    assert np.array_equal(m2.cpu().numpy(), m) and np.array_equal(c2.cpu().numpy(), c)


@pytest.mark.gpu
def test_chained_predict_update_meets_the_bars(ctx):
    import torch
    g = gold()
    _, bar = bars()
    m, c = _dev(g["chain_mean0"]), _dev(g["chain_cov0"])
    z = _dev(g["chain_meas"])
    st = torch.zeros(8, dtype=torch.int32, device=m.device)
    ms, cs = [], []
    for s in range(20):
        ctx.check(ctx.lib.busca_kalman_multi_predict(ctx.h, m.data_ptr(), c.data_ptr(), None, 8, _stream()))
        if s == 0:
            assert np.array_equal(m.cpu().numpy(), g["chain_pred_mean"][0]) and np.array_equal(c.cpu().numpy(), g["chain_pred_cov"][0])
        ctx.check(ctx.lib.busca_kalman_update(ctx.h, m.data_ptr(), c.data_ptr(), z[s].data_ptr(), 8, st.data_ptr(), _stream()))
        ms.append(m.clone()); cs.append(c.clone())
    ms, cs = torch.stack(ms).cpu().numpy(), torch.stack(cs).cpu().numpy()
    em = max(err_mean(ms[s], g["chain_upd_mean"][s]) for s in range(20))
    ec = max(err_cov(cs[s], g["chain_upd_cov"][s]) for s in range(20))
    print("chained: mean %.3g (bar %.3g)  covariance %.3g (bar %.3g)" % (em, bar["chain_mean"], ec, bar["chain_cov"]))
    assert em <= bar["chain_mean"] and ec <= bar["chain_cov"]


@pytest.mark.gpu
def test_initiate_and_boxes_bit_exact(ctx):
    import torch
    g = gold()
    z = _dev(g["init_meas"])
    m = torch.full((64, 8), -7.0, dtype=torch.float64, device=z.device)
    c = torch.full((64, 8, 8), -7.0, dtype=torch.float64, device=z.device)
    ctx.check(ctx.lib.busca_kalman_initiate(ctx.h, z.data_ptr(), 64, m.data_ptr(), c.data_ptr(), _stream()))
    assert np.array_equal(m.cpu().numpy(), g["init_mean"]) and np.array_equal(c.cpu().numpy(), g["init_cov"])
    assert not np.signbit(c.cpu().numpy()).any()
    mean = _dev(g["mean"])
    for tlbr, key in ((0, "tlwh"), (1, "tlbr")):
        for n in (96, 1):
            out = torch.full((n, 4), -7.0, dtype=torch.float64, device=z.device)
            ctx.check(ctx.lib.busca_kalman_boxes(ctx.h, mean.data_ptr(), n, tlbr, out.data_ptr(), _stream()))
            assert np.array_equal(out.cpu().numpy(), g[key][:n])
    # more tracks than one block of the box kernel holds
    big = np.tile(g["mean"], (4, 1))[:300]
    out = torch.full((300, 4), -7.0, dtype=torch.float64, device=z.device)
    ctx.check(ctx.lib.busca_kalman_boxes(ctx.h, _dev(big).data_ptr(), 300, 1, out.data_ptr(), _stream()))
    assert np.array_equal(out.cpu().numpy(), np.tile(g["tlbr"], (4, 1))[:300])


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(1, 1), (3, 257), (96, 40)])
def test_gating_meets_the_bar(ctx, n, m):
    g = gold()
    _, bar = bars()
    cols = np.arange(m) % 40                             # more measurements than the fixture has: its 40, over and over
    for only_position, metric in MODES:
        out, st = gpu_gating(ctx, g["mean"][:n], g["cov"][:n], g["gate_meas"][cols], only_position, metric)
        ref = g[gate_key(only_position, metric)][:n][:, cols]
        e = err_gate(out, ref)
        print("gating (%d, %d) only_position=%d %s: %.3g (bar %.3g)" % (n, m, only_position, metric, e, bar["gate"]))
        assert (st == 0).all() and out.shape == (n, m)
        assert e <= bar["gate"]


@pytest.mark.gpu
def test_not_positive_definite_is_flagged(ctx):
    from busca_amd import tracking
    g = gold()
    _, bar = bars()
    idx = [4, 5, 6]
    mean, cov, meas = g["mean"][idx].copy(), g["cov"][idx].copy(), g["meas"][idx].copy()
    cov[1, :4, :4] = -np.eye(4)
    m, c, st = gpu_update(ctx, mean, cov, meas)
    assert st.tolist() == [0, 1, 0]
    assert np.array_equal(m[1], mean[1]) and np.array_equal(c[1], cov[1])                 # untouched
    assert err_mean(m[[0, 2]], g["upd_mean"][[4, 6]]) <= bar["mean"] and err_cov(c[[0, 2]], g["upd_cov"][[4, 6]]) <= bar["cov"]
    # a NaN pivot is flagged too
    cov2 = cov.copy()
    cov2[1] = g["cov"][5]
    cov2[1, 2, 2] = np.nan
    assert gpu_update(ctx, mean, cov2, meas)[2].tolist() == [0, 1, 0]
    # gating: the row is NaN, the others are computed; only_position looks at the leading 2 x 2 block only; 'gaussian' factors nothing
    out, st = gpu_gating(ctx, mean, cov, g["gate_meas"], False, "maha")
    assert st.tolist() == [0, 1, 0] and np.isnan(out[1]).all()
    assert err_gate(out[[0, 2]], g["gate_maha4"][[4, 6]]) <= bar["gate"]
    cov3 = g["cov"][idx].copy()
    cov3[1, 3, 3] = -1e9
    out, st = gpu_gating(ctx, mean, cov3, g["gate_meas"], True, "maha")
    assert st.tolist() == [0, 0, 0] and err_gate(out, g["gate_maha2"][idx]) <= bar["gate"]
    assert gpu_gating(ctx, mean, cov3, g["gate_meas"], False, "maha")[1].tolist() == [0, 1, 0]
    out, st = gpu_gating(ctx, mean, cov, g["gate_meas"], False, "gaussian")
    assert st.tolist() == [0, 0, 0] and err_gate(out, g["gate_gauss4"][idx]) <= bar["gate"]
    # the mirror raises what the reference raises - after the other tracks of the call were updated
    tracks = _tracks(mean, cov)
    with pytest.raises(np.linalg.LinAlgError, match="track 1"):
        tracking.multi_update(tracks, meas, ctx=ctx)
    assert np.array_equal(tracks[1].mean, mean[1]) and np.array_equal(tracks[1].covariance, cov[1])
    assert np.array_equal(tracks[0].mean, m[0]) and np.array_equal(tracks[2].covariance, c[2])
    with pytest.raises(np.linalg.LinAlgError, match="track 1"):
        tracking.gating_distance(_tracks(mean, cov), g["gate_meas"], ctx=ctx)
    with pytest.raises(np.linalg.LinAlgError):
        tracking.fuse_motion(np.zeros((3, 40)), _tracks(mean, cov), g["gate_meas"], ctx=ctx)


@pytest.mark.gpu
def test_mirrors_on_simple_namespace_tracks(ctx):
    from busca_amd import tracking
    g = gold()
    _, bar = bars()
    # multi_update with measurements given as an array: the fixture's own
    tracks = _tracks(g["mean"], g["cov"])
    tracking.multi_update(tracks, g["meas"], ctx=ctx)
    m, c = np.stack([t.mean for t in tracks]), np.stack([t.covariance for t in tracks])
    assert err_mean(m, g["upd_mean"]) <= bar["mean"] and err_cov(c, g["upd_cov"]) <= bar["cov"]
    assert tracks[0].mean.shape == (8,) and tracks[0].covariance.shape == (8, 8)
    # ... and with detection objects: the measurement is tlwh_to_xyah(det.tlwh)
    dets = _detections(g["meas"])
    tracks = _tracks(g["mean"], g["cov"])
    tracking.multi_update(tracks, dets, ctx=ctx)
    wm, wc, _ = gpu_update(ctx, g["mean"], g["cov"], tracking.tlwh_to_xyah([d.tlwh for d in dets]))
    assert np.array_equal(np.stack([t.mean for t in tracks]), wm) and np.array_equal(np.stack([t.covariance for t in tracks]), wc)
    assert err_mean(wm, g["upd_mean"]) < 1e-9            # the tlwh round trip moves the measurement by an ulp or two
    # multi_initiate
    im, ic = tracking.multi_initiate(g["init_meas"], ctx=ctx)
    assert np.array_equal(im, g["init_mean"]) and np.array_equal(ic, g["init_cov"])
    im, ic = tracking.multi_initiate(_detections(g["init_meas"][:5]), ctx=ctx)
    rm, rc = r_initiate(tracking.tlwh_to_xyah([d.tlwh for d in _detections(g["init_meas"][:5])]))
    assert np.array_equal(im, rm) and np.array_equal(ic, rc)
    # gating_distance
    tracks = _tracks(g["mean"], g["cov"])
    for only_position, metric in MODES:
        out = tracking.gating_distance(tracks, g["gate_meas"], only_position, metric, ctx=ctx)
        assert out.shape == (96, 40) and err_gate(out, g[gate_key(only_position, metric)]) <= bar["gate"]
    with pytest.raises(ValueError):
        tracking.gating_distance(tracks, g["gate_meas"], metric="cosine", ctx=ctx)
    with pytest.raises(ValueError):
        tracking.multi_update(tracks[:3], g["meas"][:2], ctx=ctx)
    # empty lists
    tracking.multi_update([], [], ctx=ctx)
    em, ec = tracking.multi_initiate([], ctx=ctx)
    assert em.shape == (0, 8) and ec.shape == (0, 8, 8)
    assert tracking.gating_distance([], g["gate_meas"], ctx=ctx).shape == (0, 40)
    assert tracking.gating_distance(tracks, [], ctx=ctx).shape == (96, 0)
    empty = np.zeros((0, 40))
    assert tracking.fuse_motion(empty, [], g["gate_meas"], ctx=ctx) is empty and tracking.gate_cost_matrix(empty, [], g["gate_meas"], ctx=ctx) is empty
    assert tracking.predicted_cost([], dets, ctx=ctx).shape == (0, 96)
    tr = _tracks(g["mean"][:2], g["cov"][:2])
    assert tracking.predicted_cost(tr, [], ctx=ctx).shape == (2, 0)
    pm, pc = obt.kalman_multi_predict(g["mean"][:2], g["cov"][:2])
    assert np.array_equal(np.stack([t.mean for t in tr]), pm) and np.array_equal(np.stack([t.covariance for t in tr]), pc)


@pytest.mark.gpu
@pytest.mark.parametrize("only_position", [False, True])
def test_gate_and_fuse_equal_the_host_composition(ctx, only_position):
    import torch
    from busca_amd import synth, tracking
    g = gold()
    _, bar = bars()
    lam = 0.98
    dim = 2 if only_position else 4
    gate = g["gate_maha%d" % dim]
    cost = synth.uniform(71, "cost", (96, 40), 0.0, 1.0).astype(np.float64)
    tracks = _tracks(g["mean"], g["cov"])
    # matching.py:132-142 / :145-156 on the reference's own distances
    gated = cost.copy()
    gated[gate > CHI2[dim]] = np.inf
    fused = lam * gated + (1 - lam) * gate
    got = tracking.gate_cost_matrix(cost.copy(), tracks, g["gate_meas"], only_position, ctx=ctx)
    assert np.array_equal(got, gated)                    # every entry: inf exactly where the reference gates, the cost elsewhere
    assert np.isinf(gated).sum() >= 30 and np.isfinite(gated).sum() >= 30
    got = tracking.fuse_motion(cost.copy(), tracks, g["gate_meas"], only_position, lam, ctx=ctx)
    assert np.array_equal(np.isinf(got), np.isinf(fused)) and not np.isnan(got).any()
    fin = np.isfinite(fused)
    # the only term that may differ is (1 - lambda) * distance, by the gating bar; two roundings on top
    tol = (1 - lam) * bar["gate"] * np.maximum(1.0, np.abs(gate)) + 4 * np.finfo(np.float64).eps * np.abs(fused)
    assert (np.abs(got[fin] - fused[fin]) <= tol[fin]).all()
    # a cost matrix that is already on the device gives the same bits
    dcost = torch.from_numpy(cost).to(torch.device("cuda", 0))
    assert np.array_equal(tracking.fuse_motion(dcost, tracks, g["gate_meas"], only_position, lam, ctx=ctx), got)
    assert np.array_equal(dcost.cpu().numpy(), cost)     # the caller's tensor is not written


@pytest.mark.gpu
def test_predicted_cost_equals_the_separate_calls(ctx):
    from busca_amd import synth, tracking
    g = gold()
    states = np.arange(96) % 3                           # Tracked (1) and others: multi_predict zeroes mean[7] of the others
    scores = synth.uniform(72, "scores", (40,), 0.3, 1.0).astype(np.float64)
    dets = _detections(g["gate_meas"], scores)
    for fuse, with_scores, only_position in ((True, True, False), (True, False, True), (False, True, False), (False, False, False)):
        sc = scores if with_scores else None
        a = _tracks(g["mean"], g["cov"], states)
        got = tracking.predicted_cost(a, dets, det_scores=sc, fuse_motion=fuse, only_position=only_position, ctx=ctx)
        b = _tracks(g["mean"], g["cov"], states)
        tracking.multi_predict(b, ctx=ctx)
        for t in b:
            t.tlbr = r_boxes(t.mean[None], True)[0]
        want = tracking.iou_distance(b, dets, det_scores=sc, ctx=ctx)
        if fuse:
            want = tracking.fuse_motion(want, b, dets, only_position, ctx=ctx)
        assert got.shape == (96, 40) and np.array_equal(got, want)
        assert np.array_equal(np.stack([t.mean for t in a]), np.stack([t.mean for t in b]))
        assert np.array_equal(np.stack([t.covariance for t in a]), np.stack([t.covariance for t in b]))
        if fuse:
            assert np.isinf(got).any() and np.isfinite(got).any()
        else:
            assert (got < 1.0).any()


@pytest.mark.gpu
def test_empty_and_null_arguments(ctx):
    lib, h = ctx.lib, ctx.h
    g = gold()
    assert lib.busca_kalman_update(h, None, None, None, 0, None, None) == 0
    assert lib.busca_kalman_initiate(h, None, 0, None, None, None) == 0
    assert lib.busca_kalman_boxes(h, None, 0, 0, None, None) == 0
    assert lib.busca_kalman_gating(h, None, None, 0, None, 5, 0, 0, None, None, None) == 0
    assert lib.busca_kalman_gating(h, None, None, 5, None, 0, 0, 0, None, None, None) == 0
    assert lib.busca_kalman_update(h, None, None, None, 3, None, None) == -1
    assert lib.busca_kalman_initiate(h, None, 3, None, None, None) == -1
    assert lib.busca_kalman_boxes(h, None, 3, 1, None, None) == -1
    assert lib.busca_kalman_gating(h, None, None, 3, None, 4, 0, 0, None, None, None) == -1
    m, c, z = _dev(g["mean"]), _dev(g["cov"]), _dev(g["meas"])
    assert lib.busca_kalman_update(h, m.data_ptr(), None, z.data_ptr(), 3, None, None) == -1
    assert lib.busca_kalman_update(h, m.data_ptr(), c.data_ptr(), z.data_ptr(), -1, None, None) == -1
    assert lib.busca_kalman_boxes(h, m.data_ptr(), 3, 2, z.data_ptr(), None) == -1            # tlbr is 0 or 1
    assert lib.busca_kalman_gating(h, m.data_ptr(), c.data_ptr(), 3, z.data_ptr(), 4, 2, 0, z.data_ptr(), None, None) == -1
    assert lib.busca_kalman_gating(h, m.data_ptr(), c.data_ptr(), 3, z.data_ptr(), 4, 0, 2, z.data_ptr(), None, None) == -1
    assert np.array_equal(m.cpu().numpy(), g["mean"]) and np.array_equal(z.cpu().numpy(), g["meas"])    # nothing was launched
    assert b"busca_kalman_gating" in lib.busca_last_error(h)
