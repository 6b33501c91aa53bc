"""Stream order of libbusca_sort.so and SortStore: each of the five calls and the two rounds behind a busy non-default stream, with the helper and
the reasoning of tests/test_streams_gpu.py - the state tensors hold POISON (other tracks' states) until the true values arrive on the side stream
behind a prefix of matmuls, every output is poisoned, and the result must equal the idle default-stream run bit for bit with only the side stream
synchronised.  The five calls are made through the C-ABI with the stream passed explicitly; the rounds through SortStore with the side stream as
torch's current one, as a tracker calls them."""
import numpy as np
import pytest

from tests.test_kalman_filter import gold
from tests.test_streams_gpu import _dev, _full, behind

gpu = pytest.mark.gpu
S, N, M = 40, 17, 20
SLOTS = np.random.RandomState(6).permutation(S)[:N].astype(np.int32)


@pytest.fixture(scope="module")
def busy():
    from tests.test_streams_gpu import Busy
    b = Busy()
    yield b
    b.report()


@pytest.fixture(scope="module")
def ctx():
    from busca_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _pad(a):
    return np.concatenate([a, np.zeros_like(a[:1])])                                          # the spare slot


def _states():
    """(true, poison): the fixture's states 0 .. 39 in their slots, and states 40 .. 79 in the same slots."""
    g = gold()
    return [_dev(_pad(g["mean"][:S])), _dev(_pad(g["cov"][:S]))], [_dev(_pad(g["mean"][S:2 * S])), _dev(_pad(g["cov"][S:2 * S]))]


def _tlwh(xyah):
    out = np.array(xyah, dtype=np.float64)
    out[:, 2] *= out[:, 3]
    out[:, :2] -= out[:, 2:] / 2
    return out


@gpu
@pytest.mark.parametrize("which", ["predict", "update", "camera_update", "gate_cost", "iou_cost"])
def test_the_calls_behind_a_busy_stream(busy, which):
    import torch
    from busca_amd import _sort_lib
    lib = _sort_lib.load()
    g = gold()
    true, poison = _states()
    slot = _dev(SLOTS)
    meas = _dev(g["meas"][SLOTS])                                                             # measurement i belongs to the state in slot SLOTS[i]
    conf = _dev(np.linspace(0.0, 0.999, N))
    matrix = _dev(np.array([[0.999995, -0.003, 12.5], [0.003, 0.999995, -7.25], [0.0, 0.0, 1.0]]))
    xyah = _dev(g["meas"][:M])
    boxes = _dev(_tlwh(g["meas"][:M]))
    cost = _dev(np.random.RandomState(1).uniform(0.0, 0.6, (N, M)))
    stale = _dev((np.arange(N) % 5 == 2).astype(np.uint8))
    outs = {"update": lambda: [_full((N,), -7, torch.int32)],
            "gate_cost": lambda: [_full((N, M), float("nan"), torch.float64), _full((N,), -7, torch.int32)],
            "iou_cost": lambda: [_full((N, M), float("nan"), torch.float64)]}.get(which)

    def call(x, o, st):
        mean, cov = x[0].data_ptr(), x[1].data_ptr()
        if which == "predict":
            rc = lib.busca_sort_predict(mean, cov, S, slot.data_ptr(), N, 0, st)
        elif which == "update":
            rc = lib.busca_sort_update(mean, cov, S, slot.data_ptr(), N, meas.data_ptr(), None, N, conf.data_ptr(), o[0].data_ptr(), 0, st)
        elif which == "camera_update":
            rc = lib.busca_sort_camera_update(mean, S, slot.data_ptr(), N, matrix.data_ptr(), 0, st)
        elif which == "gate_cost":
            rc = lib.busca_sort_gate_cost(mean, cov, S, slot.data_ptr(), N, xyah.data_ptr(), M, cost.data_ptr(), M, 1e5, 3, 0.98, 0.4, o[0].data_ptr(),
                                          o[1].data_ptr(), 0, st)
        else:
            rc = lib.busca_sort_iou_cost(mean, S, slot.data_ptr(), N, stale.data_ptr(), boxes.data_ptr(), M, 2, 0.7, o[0].data_ptr(), 0, st)
        _sort_lib.check(rc)
    want, got = behind(busy, "busca_sort_" + which, call, true=true, poison=poison, outs=outs, form="explicit")
    if which in ("predict", "update", "camera_update"):                                       # the call did something: the state is not the input
        assert not np.array_equal(got[0], true[0].cpu().numpy())
    else:
        assert np.isfinite(got[2]).all() and (got[2] < 0.7).any()


@gpu
def test_iou_round_behind_a_busy_stream(busy):
    from busca_amd.sort_store import SortStore
    g = gold()
    true, poison = _states()
    boxes = _tlwh(g["mean"][SLOTS[:12], :4])
    boxes[:, 2:] *= 1.05
    st = SortStore(S)

    def call(x, o, stream):
        st.mean, st.cov = x
        m, ut, ud = st.iou_round(SLOTS, boxes, 0.7, stale=np.arange(N) % 5 == 2)
        return np.asarray(m, dtype=np.int64).reshape(-1, 2), np.asarray(ut, dtype=np.int64), np.asarray(ud, dtype=np.int64)
    want, got = behind(busy, "SortStore.iou_round", call, true=true, poison=poison, form="current", host=True)
    assert len(got[2]) >= 6                                                                   # pairs were matched


@gpu
@pytest.mark.parametrize("depth", [None, 3])
def test_appearance_round_behind_a_busy_stream(ctx, busy, depth):
    from busca_amd.sort_store import SortStore
    from tests import test_appearance as ta
    trk, det, lam, maxd, tracks, dets = ta.gate_case()
    metric = ta._fitted_metric(ctx, trk, maxd, budget=3)
    n = len(tracks)
    slots = np.random.RandomState(9).permutation(128)[:n]
    mean, cov = np.zeros((129, 8)), np.zeros((129, 8, 8))
    mean[slots], cov[slots] = np.stack([t.mean for t in tracks]), np.stack([t.covariance for t in tracks])
    true = [_dev(mean), _dev(cov)]
    poison = [_dev(np.roll(mean, 7, axis=0)), _dev(np.roll(cov, 7, axis=0))]
    feats, xyah = np.stack([d.feature for d in dets]), np.stack([d.to_xyah() for d in dets])
    ids, tsu = [t.track_id for t in tracks], [t.time_since_update for t in tracks]
    st = SortStore(128)

    def call(x, o, stream):
        st.mean, st.cov = x
        m, ut, ud = st.appearance_round(metric, slots, ids, tsu, feats, xyah, cascade_depth=depth, mc_lambda=lam)
        return np.asarray(m, dtype=np.int64).reshape(-1, 2), np.asarray(sorted(ut), dtype=np.int64), np.asarray(ud, dtype=np.int64)
    want, got = behind(busy, "SortStore.appearance_round", call, true=true, poison=poison, form="current", host=True)
    assert len(got[2]) >= 5
