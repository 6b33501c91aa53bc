"""Staged assignment on the device: busca_assign_stages (include/busca_assign_stages.h), tracking.assign_stages and SortStore.match.

The oracle of the solver is the existing, separately tested busca_linear_assignment on COMPACTED matrices (`oracle` below): for every stage the
member rows and the columns no earlier stage matched are selected on the host, the sub-matrix of the stage's plane is solved with the stage's
limit, and the matched columns are withdrawn.  The staged kernel must return the identical integers - row_to_col, col_to_row, row_stage -, ties
included: equality is exact everywhere in this file, nothing is compared within a tolerance.  On the continuous-cost cases, where the optimum of a
stage is unique, every stage is also compared with scipy's linear_sum_assignment on the limit-reduced matrix (test_linear_assignment.r_clamped).

The oracle of SortStore.match is today's composition: SortStore.appearance_round and SortStore.iou_round wired as Tracker._match wires
matching_cascade and min_cost_matching (adapters/StrongSORT/deep_sort/tracker.py:226-252), on the same store, metric and detections (`r_match`).

The stage table is shared by the problems of a batch, so a record with a plane outside the slab gives EVERY problem of that call status 2; that
a faulty problem leaves the others of its batch alone is shown with the status a single problem can earn by itself, 1 (a -inf cost)."""
import numpy as np
import pytest

from tests.test_linear_assignment import gpu_solve, r_clamped

gpu = pytest.mark.gpu
INF, NAN = np.inf, np.nan


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


def stage_table(stages):
    t = np.zeros(len(stages), dtype=np.dtype([("plane", "<i4"), ("reserved", "<i4"), ("limit", "<f8")]))
    t["plane"], t["limit"] = [p for p, _ in stages], [lim for _, lim in stages]
    return t.view(np.uint8).reshape(-1)


def gpu_stages(ctx, cost, stages, first, again=None, dims=None, rc=0):
    """The raw busca_assign_stages call on cost [planes,n,m] or [batch,planes,n,m] with every output requested; the outputs start out as garbage."""
    import torch
    cost = np.asarray(cost, dtype=np.float64)
    single = cost.ndim == 3
    b, p, n, m = (1,) + cost.shape if single else cost.shape
    dc, dev = _dev(cost), torch.device("cuda", 0)
    outs = [torch.full((b, k), -7, dtype=torch.int32, device=dev) for k in (n, m, n, 1)]
    tab = _dev(stage_table(stages))
    df = _dev(np.asarray(first, dtype=np.int32).reshape(b, n))
    da = None if again is None else _dev(np.asarray(again, dtype=np.int32).reshape(b, n))
    dd = None if dims is None else _dev(np.asarray(dims, dtype=np.int32))
    got = ctx.lib.busca_assign_stages(ctx.h, dc.data_ptr(), p, b, n, m, None if dd is None else dd.data_ptr(), tab.data_ptr(), len(stages), df.data_ptr(),
                                      None if da is None else da.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
                                      _stream())
    assert got == rc, ctx.lib.busca_last_error(ctx.h)
    x, y, st, status = (o.cpu().numpy().astype(np.int64) for o in outs)
    out = dict(x=x, y=y, stage=st, status=status[:, 0])
    return {k: v[0] for k, v in out.items()} if single else out


def members(s, first, again, x):
    """The rows of stage s by the header's rule: first == s, or again == s with again > first and the row still unmatched."""
    return [i for i in range(len(first)) if first[i] == s or (again is not None and again[i] == s and again[i] > first[i] and x[i] < 0)]


def oracle(ctx, cost, stages, first, again=None, scipy=False):
    """The chain of compacted busca_linear_assignment solves of one problem cost [planes,n,m] -> the dict gpu_stages returns for it, and the number of
    solves it took."""
    _, n, m = cost.shape
    x, y, st = np.full(n, -1, dtype=np.int64), np.full(m, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    solves = 0
    for s, (plane, limit) in enumerate(stages):
        rows, cols = members(s, first, again, x), [j for j in range(m) if y[j] < 0]
        if not rows or not cols:
            continue
        sub = np.ascontiguousarray(cost[plane][np.ix_(rows, cols)])
        r = gpu_solve(ctx, sub, limit)
        solves += 1
        if r["status"] != 0:
            return dict(x=np.full(n, -1), y=np.full(m, -1), stage=np.full(n, -1), status=1), solves
        if scipy:
            assert np.array_equal(r["x"], r_clamped(sub, limit)), ("the stage's optimum is not scipy's", s)
        for a, i in enumerate(rows):
            if r["x"][a] >= 0:
                j = cols[r["x"][a]]
                x[i], y[j], st[i] = j, i, s
    return dict(x=x, y=y, stage=st, status=0), solves


def same(got, want, what=""):
    for k in ("status", "x", "y", "stage"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])


def both_ways(ctx, cost, stages, first, again=None):
    """The kernel with the rows of a stage staged in LDS (where they fit) and read from global memory: the same integers."""
    assert ctx.get_option("assign_stage") == -1
    a = gpu_stages(ctx, cost, stages, first, again)
    assert ctx.get_option("last_assign_staged") == 1
    ctx.set_option("assign_stage", 0)
    try:
        b = gpu_stages(ctx, cost, stages, first, again)
        assert ctx.get_option("last_assign_staged") == 0
    finally:
        ctx.set_option("assign_stage", -1)
    same(a, b, "staged against unstaged")
    return a


def consistent(r, n, m):
    x, y = r["x"], r["y"]
    rows = np.nonzero(x >= 0)[0]
    assert all(y[x[i]] == i for i in rows) and (y >= 0).sum() == len(rows) and len(set(x[rows])) == len(rows)
    assert np.array_equal(r["stage"] >= 0, x >= 0)


# ---- the solver ------------------------------------------------------------------------------------------------------------
@gpu
def test_small_chain_two_planes(ctx):
    rs = np.random.RandomState(11)
    cost = rs.uniform(0.0, 1.0, (2, 5, 4))
    stages = [(0, 0.45), (1, 0.7), (0, 0.9)]
    first, again = [0, 0, 1, 2, 0], [2, 1, -1, -1, 2]
    got = both_ways(ctx, cost, stages, first, again)
    want, solves = oracle(ctx, cost, stages, first, again, scipy=True)
    same(got, want)
    consistent(got, 5, 4)
    assert solves == 3 and (got["x"] >= 0).sum() >= 3 and len(set(got["stage"][got["x"] >= 0])) >= 2      # the chain is a chain: matches in several stages


@gpu
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_ties_choose_the_compacted_solvers_pairs(ctx, seed):
    """Costs on a grid of 1/8: equal distances abound, and a masked solver that broke ties by anything but the lowest free column would still find a
    matching of the same cost - and differ from the compacted solve."""
    rs = np.random.RandomState(100 + seed)
    cost = rs.randint(0, 9, (2, 12, 9)) / 8.0
    stages = [(0, 0.5), (1, 0.5), (0, 0.75), (1, 1.01)]
    first = rs.randint(0, 4, 12)
    again = np.where(rs.uniform(size=12) < 0.6, rs.randint(1, 4, 12), -1)
    got = both_ways(ctx, cost, stages, first, again)
    want, solves = oracle(ctx, cost, stages, first, again)
    same(got, want)
    consistent(got, 12, 9)
    assert solves >= 3
    assert sum(len(set(row[row < 0.5])) < (row < 0.5).sum() for row in cost[0]) >= 6   # ties among the admissible entries of most rows


@gpu
def test_the_again_rule(ctx):
    big = 0.9
    p0 = np.full((6, 6), big)
    p1 = np.full((6, 6), big)
    p0[0, 0] = 0.1                    # row 0: matched in stage 0 ...
    p1[0, 3] = 0.05                   # ... and the cheapest entry of stage 1, which it must not enter again
    p1[1, 1] = 0.2                    # row 1: nothing admissible in stage 0, again = 1: matched in stage 1
    p1[2, 2] = 0.2                    # row 2: unmatched after stage 0 and again = -1: stays unmatched
    p1[3, 3] = 0.3                    # row 3: first = again = 1 (again <= first: ignored), matched once in stage 1
    p0[4, 4] = 0.1
    p1[4, 4] = 0.1                    # row 4: first = 1, again = 0 (<= first: ignored): stage 0 must not see it, stage 1 matches it
    p1[5, 5] = 0.4                    # row 5: first = -1 (never), again = 1: takes part in stage 1
    cost = np.stack([p0, p1])
    stages = [(0, 0.5), (1, 0.5)]
    first, again = [0, 0, 0, 1, 1, -1], [1, 1, -1, 1, 0, 1]
    got = both_ways(ctx, cost, stages, first, again)
    assert got["status"] == 0 and got["x"].tolist() == [0, 1, -1, 3, 4, 5] and got["stage"].tolist() == [0, 1, -1, 1, 1, 1]
    assert got["y"].tolist() == [0, 1, -1, 3, 4, 5]
    same(got, oracle(ctx, cost, stages, first, again)[0])
    # without `again` (NULL) the rows take part once
    got = gpu_stages(ctx, cost, stages, first, None)
    assert got["x"].tolist() == [0, -1, -1, 3, 4, -1]
    same(got, oracle(ctx, cost, stages, first, None)[0])
    # values outside 0 .. n_stages - 1 mean never, on either side
    got = gpu_stages(ctx, cost, stages, [0, 2, 7, 1, 1, -3], [1, 1, 1, 2, 9, 1])
    assert got["x"].tolist() == [0, -1, -1, 3, 4, 5]
    same(got, oracle(ctx, cost, stages, [0, 2, 7, 1, 1, -3], [1, 1, 1, 2, 9, 1])[0])


@gpu
@pytest.mark.parametrize("m", [256, 257])
def test_wave_boundary(ctx, m):
    """Up to 256 columns one wave scans a row, beyond four waves with an LDS exchange: both sides of it."""
    rs = np.random.RandomState(m)
    cost = rs.uniform(0.0, 1.0, (2, 8, m))
    cost[:, :, m - 1] = 1e-4 * (1 + np.arange(8))                  # the last column (of the fourth wave, where there is one) is every row's cheapest
    stages = [(0, 0.004), (1, 0.004), (0, 0.5)]
    first, again = [0, 1, 2, 0, 1, 2, 0, 0], [1, 2, -1, 2, 2, -1, 1, 2]
    got = both_ways(ctx, cost, stages, first, again)
    want, solves = oracle(ctx, cost, stages, first, again, scipy=True)
    same(got, want)
    consistent(got, 8, m)
    assert solves == 3 and (got["x"] == m - 1).sum() == 1 and got["stage"][got["x"] == m - 1] == 0 and (got["x"] >= 0).sum() >= 4


@gpu
@pytest.mark.parametrize("big", [0, 1])
def test_where_the_lds_staging_stops(ctx, big):
    """The member rows of a stage are staged in LDS when they fit what the workgroup has left of its 160 KiB.  150 x 150: `fit` rows of 150 doubles
    do, fit + 1 do not (the host function that sizes the launch says so).  Stage 0 holds fit + big rows, stage 1 the other rows and, again, every
    row stage 0 left - a staged stage behind an unstaged one and the other way round."""
    from busca_amd import _lib
    size = 150
    fit = (160 * 1024 - _lib.load().busca_assign_stages_lds_bytes(size, size, 0)) // (8 * size)
    assert _lib.load().busca_assign_stages_lds_bytes(size, size, 1) == 160 * 1024 and 100 < fit < size - 1
    rs = np.random.RandomState(size + big)
    cost = rs.uniform(0.0, 1.0, (2, size, size))
    cost[0, ::3] = 0.9                                                 # a third of the rows finds nothing in stage 0
    stages = [(0, 0.05), (1, 0.5)]
    first = np.where(np.arange(size) < fit + big, 0, 1)
    again = np.where(np.arange(size) % 2 == 0, 1, -1)
    got = both_ways(ctx, cost, stages, first, again)
    want, solves = oracle(ctx, cost, stages, first, again, scipy=True)
    same(got, want)
    consistent(got, size, size)
    assert solves == 2 and (got["stage"] == 0).sum() >= 40 and (got["stage"] == 1).sum() >= 30


@gpu
def test_degenerate_stages(ctx):
    rs = np.random.RandomState(5)
    n, m = 9, 6
    cost = rs.uniform(0.0, 1.0, (2, n, m))
    # 30 stages of which 0, 3 and 29 are populated; rows 7 and 8 never take part
    stages = [(s % 2, 0.8) for s in range(30)]
    first = [0, 0, 3, 3, 29, 29, 29, -1, -1]
    got = both_ways(ctx, cost, stages, first, None)
    want, solves = oracle(ctx, cost, stages, first, None, scipy=True)
    same(got, want)
    assert solves == 3 and set(got["stage"][got["x"] >= 0]) == {0, 3, 29} and (got["x"][7:] == -1).all()
    # a stage whose columns are all taken: stage 0 takes both columns, stages 1 and 2 find none
    cost2 = rs.uniform(0.0, 0.5, (1, 5, 2))
    got = both_ways(ctx, cost2, [(0, 0.9)] * 3, [0, 0, 1, 2, 2], None)
    want, solves = oracle(ctx, cost2, [(0, 0.9)] * 3, [0, 0, 1, 2, 2], None)
    same(got, want)
    assert solves == 1 and got["x"][:2].min() >= 0 and (got["x"][2:] == -1).all() and (got["y"] >= 0).all()
    # a stage whose every cost is >= its limit, NaN or +inf: nothing matched there, the later stage sees every column
    cost3 = rs.uniform(0.0, 0.5, (2, 4, 5))
    cost3[0] = [[0.6, NAN, INF, 0.6, 0.7], [INF, INF, INF, INF, INF], [NAN, NAN, NAN, NAN, NAN], [0.6, 0.6, 0.6, 0.6, 0.6]]
    stages3 = [(0, 0.6), (1, 0.6)]
    got = both_ways(ctx, cost3, stages3, [0, 0, 0, 0], [1, 1, 1, -1])
    want, solves = oracle(ctx, cost3, stages3, [0, 0, 0, 0], [1, 1, 1, -1], scipy=True)
    same(got, want)
    assert solves == 2 and (got["stage"][:3] == 1).all() and got["x"][3] == -1
    # nobody takes part at all
    got = gpu_stages(ctx, cost, stages, [-1] * n, [-1] * n)
    assert got["status"] == 0 and (got["x"] == -1).all() and (got["y"] == -1).all() and (got["stage"] == -1).all()


@gpu
def test_batch_with_dims(ctx):
    rs = np.random.RandomState(9)
    cost = rs.uniform(0.0, 1.0, (3, 2, 7, 6))
    dims = [[7, 6], [3, 6], [0, 4]]
    stages = [(0, 0.4), (1, 0.6), (0, 0.9)]
    first = rs.randint(0, 3, (3, 7))
    again = np.where(rs.uniform(size=(3, 7)) < 0.5, 2, -1)
    got = gpu_stages(ctx, cost, stages, first, again, dims)
    assert got["status"].tolist() == [0, 0, 0]
    for k, (nk, mk) in enumerate(dims):
        assert (got["x"][k, nk:] == -1).all() and (got["stage"][k, nk:] == -1).all() and (got["y"][k, mk:] == -1).all()      # padding
        if nk == 0:
            assert (got["x"][k] == -1).all() and (got["y"][k] == -1).all()
            continue
        corner = np.ascontiguousarray(cost[k][:, :nk, :mk])
        one = gpu_stages(ctx, corner, stages, first[k, :nk], again[k, :nk])                          # its single-problem call
        same(dict(x=got["x"][k, :nk], y=got["y"][k, :mk], stage=got["stage"][k, :nk], status=got["status"][k]), one, k)
        same(one, oracle(ctx, corner, stages, first[k, :nk], again[k, :nk], scipy=True)[0], k)
        assert (one["x"] >= 0).sum() >= 1
    # a pair outside the slab: that problem status 1 and all -1, the others as before
    bad = gpu_stages(ctx, cost, stages, first, again, [[7, 6], [8, 6], [0, 4]])
    assert bad["status"].tolist() == [0, 1, 0] and (bad["x"][1] == -1).all() and (bad["y"][1] == -1).all() and (bad["stage"][1] == -1).all()
    assert np.array_equal(bad["x"][0], got["x"][0]) and np.array_equal(bad["y"][0], got["y"][0])


@gpu
def test_status_words_are_ordinary_returns(ctx):
    rs = np.random.RandomState(3)
    cost = rs.uniform(0.0, 0.5, (2, 2, 4, 5))
    first = np.zeros((2, 4), dtype=np.int32)
    first[:, 2:] = 1
    good = gpu_stages(ctx, cost, [(0, 0.9), (1, 0.9)], first)
    assert good["status"].tolist() == [0, 0] and (good["x"] >= 0).all()
    # plane 5 of 2: status 2 and -1 everywhere - the table is the batch's, so in both problems; nothing is read through the index
    r = gpu_stages(ctx, cost, [(0, 0.9), (5, 0.9)], first)
    assert r["status"].tolist() == [2, 2] and (r["x"] == -1).all() and (r["y"] == -1).all() and (r["stage"] == -1).all()
    r = gpu_stages(ctx, cost, [(-1, 0.9), (1, 0.9)], first)
    assert r["status"].tolist() == [2, 2] and (r["x"] == -1).all()
    # a -inf cost in problem 0: status 1 there, as busca_linear_assignment reports it; problem 1 is its own single call
    poisoned = cost.copy()
    poisoned[0, 1, 2, :] = -INF                                          # row 2 stands in stage 1, which reads plane 1
    r = gpu_stages(ctx, poisoned, [(0, 0.9), (1, 0.9)], first)
    assert r["status"].tolist() == [1, 0] and (r["x"][0] == -1).all() and (r["y"][0] == -1).all() and (r["stage"][0] == -1).all()
    assert oracle(ctx, poisoned[0], [(0, 0.9), (1, 0.9)], first[0])[0]["status"] == 1
    assert np.array_equal(r["x"][1], good["x"][1]) and np.array_equal(r["y"][1], good["y"][1]) and np.array_equal(r["stage"][1], good["stage"][1])
    # and the context goes on as before
    same(gpu_stages(ctx, cost, [(0, 0.9), (1, 0.9)], first), good)


@gpu
def test_einval_and_noops(ctx):
    import torch
    from busca_amd import _lib
    lib, h, dev = ctx.lib, ctx.h, torch.device("cuda", 0)
    cost = _dev(np.zeros((1, 2, 3)))
    tab = _dev(stage_table([(0, 0.5)]))
    first = _dev(np.zeros(2, dtype=np.int32))
    x = torch.full((2,), -7, dtype=torch.int32, device=dev)
    st = torch.full((1,), -7, dtype=torch.int32, device=dev)

    def call(cost=cost.data_ptr(), planes=1, batch=1, n=2, m=3, stages=tab.data_ptr(), n_stages=1, first=first.data_ptr(), x=x.data_ptr()):
        return lib.busca_assign_stages(h, cost, planes, batch, n, m, None, stages, n_stages, first, None, x, None, None, st.data_ptr(), _stream())
    assert call() == 0
    assert x.cpu().tolist() == [0, 1] and st.item() == 0                 # col_to_row and row_stage may be NULL
    x.fill_(-7)
    for kw in (dict(batch=0), dict(n=0), dict(m=0)):                     # nothing is launched, nothing is written
        assert call(**kw) == 0
    assert x.cpu().tolist() == [-7, -7]
    for kw in (dict(batch=-1), dict(n=-1), dict(m=-1), dict(planes=-1), dict(n_stages=0), dict(n_stages=_lib.ASSIGN_STAGES_MAX + 1), dict(cost=None),
               dict(stages=None), dict(first=None), dict(x=None), dict(n=_lib.ASSIGN_MAX + 1), dict(m=_lib.ASSIGN_MAX + 1)):
        assert call(**kw) == -1, kw                                      # BUSCA_EINVAL
        assert lib.busca_last_error(h)
    assert lib.busca_assign_stages(None, cost.data_ptr(), 1, 1, 2, 3, None, tab.data_ptr(), 1, first.data_ptr(), None, x.data_ptr(), None, None, None, None) == -1
    assert x.cpu().tolist() == [-7, -7]


@gpu
def test_python_front_host_tables_and_device_tensors(ctx):
    import torch
    from busca_amd import tracking
    rs = np.random.RandomState(21)
    cost = rs.uniform(0.0, 1.0, (2, 2, 6, 5))
    stages = [(0, 0.4), (1, 0.6), (0, 0.9)]
    first = rs.randint(0, 3, (2, 6))
    again = np.where(rs.uniform(size=(2, 6)) < 0.5, 2, -1)
    raw = gpu_stages(ctx, cost, stages, first, again)
    out = tracking.assign_stages(ctx, _dev(cost), stages, first, again)              # host tables: one pinned upload
    assert torch.is_tensor(out) and out.is_cuda and out.dtype == torch.int32 and out.shape == (2 * (6 + 5 + 6 + 1),)
    host = out.cpu().numpy()
    for got in (host, tracking.assign_stages(ctx, cost, _dev(stage_table(stages)), _dev(first.astype(np.int32)), _dev(again.astype(np.int32))).cpu().numpy()):
        assert np.array_equal(got[:12].reshape(2, 6), raw["x"]) and np.array_equal(got[12:22].reshape(2, 5), raw["y"])
        assert np.array_equal(got[22:34].reshape(2, 6), raw["stage"]) and np.array_equal(got[34:], raw["status"])
    one = tracking.assign_stages(ctx, cost[1], stages, first[1]).cpu().numpy()        # [planes, n, m], no `again`
    want = gpu_stages(ctx, cost[1], stages, first[1], None)
    assert np.array_equal(one, np.concatenate([want["x"], want["y"], want["stage"], [0]]))
    dims = tracking.assign_stages(ctx, cost, stages, first, again, dims=[[6, 5], [2, 3]]).cpu().numpy()
    assert np.array_equal(dims[:6], raw["x"][0]) and (dims[8:12] == -1).all() and dims[34:].tolist() == [0, 0]
    empty = tracking.assign_stages(ctx, np.zeros((2, 0, 4)), stages, []).cpu().numpy()
    assert empty.tolist() == [-1] * 4 + [0]
    with pytest.raises(ValueError, match="first"):
        tracking.assign_stages(ctx, cost, stages, first[0], again)
    with pytest.raises(ValueError, match="again"):
        tracking.assign_stages(ctx, cost, stages, first, again[0])


# ---- SortStore.match ---------------------------------------------------------------------------------------------------------
E = 16                                               # the smallest feature width busca_appearance_cost takes (a multiple of 16)
AGES = [1, 1, 1, 2, 2, 5, 1, 1, 1]                   # six confirmed tracks, then three unconfirmed ones
CONFIRMED = [True] * 6 + [False] * 3
SLOTS = np.array([11, 3, 27, 8, 19, 0, 30, 5, 14])
IDS = [100 + k for k in range(9)]


def _tlwh(k, dx=0.0):
    return np.array([60.0 + 170.0 * k + dx, 200.0 + 7.0 * (k % 3), 50.0, 120.0])


def _xyah_of(tlwh):
    out = np.array(tlwh, dtype=np.float64).reshape(-1, 4)
    out[:, :2] += out[:, 2:] / 2
    out[:, 2] /= out[:, 3]
    return out


def scene(ctx, n=9, m=7):
    """A frame that makes every branch of tracker.py:239-248 fire.  Track k stands at _tlwh(k) with the unit feature F[k]; detection j:
      0, 1, 2  tracks 0 (age 1), 3 (age 2), 5 (age 5) with their own features: matched by their cascade levels
      3        track 6 (unconfirmed), overlapping: the IoU stage
      4        track 1 (age 1) overlapping, with a far feature: the cascade rejects it, the IoU stage recovers it
      5        track 4 (age 2) in the same situation: time_since_update != 1, the IoU stage must NOT take it
      6        nobody's
    Tracks 2, 7 and 8 see nothing.  -> (store, metric, feats [m,E], xyah [m,4], tlwh [m,4])."""
    from busca_amd import tracking
    from busca_amd.sort_store import SortStore
    rs = np.random.RandomState(31)
    F = rs.normal(size=(9, E))
    F /= np.linalg.norm(F, axis=1, keepdims=True)
    st = SortStore(32)
    st.initiate(SLOTS, _xyah_of([_tlwh(k) for k in range(9)]))
    st.predict(SLOTS)
    metric = tracking.NearestNeighborDistanceMetric("cosine", 0.3, budget=3, ctx=ctx)
    metric.partial_fit(F[:6].astype(np.float32), IDS[:6], IDS[:6])                       # the confirmed tracks have galleries, the others none
    owner = [0, 3, 5, 6, 1, 4]
    tlwh = np.stack([_tlwh(k, dx=1.5 + 0.5 * j) for j, k in enumerate(owner)] + [np.array([3000.0, 900.0, 40.0, 90.0])])
    feats = np.stack([F[0], F[3], F[5], F[6], -F[1], -F[4], F[2][::-1]]) + rs.normal(scale=0.01, size=(7, E))
    return st, metric, feats[:m].astype(np.float32), _xyah_of(tlwh[:m]), tlwh[:m]


def r_match(st, metric, slots, ids, tsu, confirmed, feats, xyah, tlwh, max_iou, depth, lam, seen=None):
    """Tracker._match (tracker.py:226-252) on SortStore.appearance_round and SortStore.iou_round."""
    confirmed_tracks = [i for i in range(len(slots)) if confirmed[i]]
    unconfirmed_tracks = [i for i in range(len(slots)) if not confirmed[i]]
    ma, ua, ud = st.appearance_round(metric, slots[confirmed_tracks], [ids[i] for i in confirmed_tracks], [tsu[i] for i in confirmed_tracks], feats, xyah,
                                     cascade_depth=depth, mc_lambda=lam)
    matches_a = [(confirmed_tracks[r], j) for r, j in ma]
    unmatched_tracks_a = [confirmed_tracks[r] for r in ua]
    iou_track_candidates = unconfirmed_tracks + [k for k in unmatched_tracks_a if tsu[k] == 1]
    unmatched_tracks_a = [k for k in unmatched_tracks_a if tsu[k] != 1]
    mb, ub, ud = st.iou_round(slots[iou_track_candidates], tlwh, max_iou, stale=[tsu[k] > 1 for k in iou_track_candidates], detection_indices=ud)
    matches_b = [(iou_track_candidates[r], j) for r, j in mb]
    unmatched_tracks_b = [iou_track_candidates[r] for r in ub]
    if seen is not None:
        seen.update(matches_a=matches_a, matches_b=matches_b, unmatched_tracks_a=unmatched_tracks_a, iou_track_candidates=iou_track_candidates)
    return matches_a + matches_b, list(set(unmatched_tracks_a + unmatched_tracks_b)), ud


def same_match(got, want):
    assert sorted((int(a), int(b)) for a, b in got[0]) == sorted((int(a), int(b)) for a, b in want[0])
    assert len(got[1]) == len(set(got[1])) and set(int(a) for a in got[1]) == set(int(a) for a in want[1])
    assert len(got[2]) == len(set(got[2])) and set(int(a) for a in got[2]) == set(int(a) for a in want[2])


@gpu
@pytest.mark.parametrize("lam", [None, 0.98])
@pytest.mark.parametrize("depth", [6, None])
def test_match_equals_the_two_rounds(ctx, depth, lam):
    st, metric, feats, xyah, tlwh = scene(ctx)
    seen = {}
    want = r_match(st, metric, SLOTS, IDS, AGES, CONFIRMED, feats, xyah, tlwh, 0.7, depth, lam, seen)
    # the oracle walks every branch of tracker.py:239-248 on this frame
    assert sorted(seen["matches_a"]) == [(0, 0), (3, 1), (5, 2)]                        # cascade levels 0, 1 and 4 (woC: one problem)
    assert (1, 4) in seen["matches_b"] and (6, 3) in seen["matches_b"]                  # the age-1 track recovered by IoU, and the unconfirmed one
    assert 4 in seen["unmatched_tracks_a"] and 4 not in seen["iou_track_candidates"]    # the age-2 track the cascade left is NOT an IoU candidate ...
    assert 5 in want[2] and 4 in want[1]                                                # ... so its overlapping detection stays free
    assert 1 in seen["iou_track_candidates"] and 2 in seen["iou_track_candidates"] and 2 in want[1] and 6 in want[2]
    got = st.match(metric, SLOTS, IDS, AGES, CONFIRMED, feats, xyah, tlwh, 0.7, cascade_depth=depth, mc_lambda=lam)
    same_match(got, want)
    assert got[0][:3] == [(0, 0), (3, 1), (5, 2)] and sorted(got[0][3:]) == [(1, 4), (6, 3)]      # in stage order, as _match lists them
    # device operands are read in place
    got = st.match(metric, _dev(SLOTS.astype(np.int32)), IDS, AGES, CONFIRMED, _dev(feats), _dev(xyah), _dev(tlwh), 0.7, cascade_depth=depth, mc_lambda=lam)
    same_match(got, want)


@gpu
def test_match_edge_sizes(ctx):
    st, metric, feats, xyah, tlwh = scene(ctx)
    none = np.zeros(0, dtype=np.int64)
    assert st.match(metric, SLOTS, IDS, AGES, CONFIRMED, feats[:0], xyah[:0], tlwh[:0], 0.7, cascade_depth=6) == ([], list(range(9)), [])
    assert st.match(metric, none, [], [], [], feats, xyah, tlwh, 0.7, cascade_depth=6) == ([], [], list(range(7)))
    for rows in ([6, 7, 8], [0, 1, 2, 3, 4, 5]):                             # only unconfirmed tracks; only confirmed tracks
        sub = [SLOTS[rows], [IDS[i] for i in rows], [AGES[i] for i in rows], [CONFIRMED[i] for i in rows]]
        for depth in (6, None):
            want = r_match(st, metric, *sub, feats, xyah, tlwh, 0.7, depth, None)
            got = st.match(metric, *sub, feats, xyah, tlwh, 0.7, cascade_depth=depth)
            same_match(got, want)
            assert len(got[0]) == (1 if rows[0] == 6 else 4)


@gpu
def test_match_raises_where_appearance_round_raises(ctx):
    import torch
    st, metric, feats, xyah, tlwh = scene(ctx)
    args = (metric, SLOTS, IDS, AGES, CONFIRMED, feats, xyah, tlwh, 0.7)
    keep = st.cov.clone()
    st.cov[int(SLOTS[7])] = -torch.eye(8, dtype=torch.float64, device=st.cov.device)      # an unconfirmed track: the gate of the cascade never sees it
    same_match(st.match(*args, cascade_depth=6), r_match(st, *args, 6, None))
    st.cov.copy_(keep)
    st.cov[int(SLOTS[3])] = -torch.eye(8, dtype=torch.float64, device=st.cov.device)      # a confirmed one
    with pytest.raises(np.linalg.LinAlgError, match="positive definite"):
        r_match(st, *args, 6, None)
    with pytest.raises(np.linalg.LinAlgError, match="positive definite"):
        st.match(*args, cascade_depth=6)
    st.cov.copy_(keep)
    same_match(st.match(*args, cascade_depth=6), r_match(st, *args, 6, None))


@gpu
def test_match_makes_one_copy_whatever_the_depth(ctx, monkeypatch):
    """Every route from a device tensor to the host is counted (Tensor.cpu / .item / .tolist / .numpy, torch.Tensor.to of a device tensor to the
    CPU): match at depth 30 takes exactly one, the two rounds one per populated level and one for the IoU stage."""
    import torch
    st, metric, feats, xyah, tlwh = scene(ctx)
    ages = [1, 1, 9, 2, 17, 30, 1, 1, 1]
    want = r_match(st, metric, SLOTS, IDS, ages, CONFIRMED, feats, xyah, tlwh, 0.7, 30, 0.98)
    count = {"n": 0}

    def counted(name):
        orig = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            to_host = name != "to" or any(str(x).startswith("cpu") for x in list(a) + list(k.values()) if isinstance(x, (str, torch.device)))
            if self.is_cuda and to_host:
                count["n"] += 1
            return orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, f)
    for name in ("cpu", "item", "tolist", "numpy", "to"):
        counted(name)
    got = st.match(metric, SLOTS, IDS, ages, CONFIRMED, feats, xyah, tlwh, 0.7, cascade_depth=30, mc_lambda=0.98)
    copies = count["n"]
    count["n"] = 0
    r_match(st, metric, SLOTS, IDS, ages, CONFIRMED, feats, xyah, tlwh, 0.7, 30, 0.98)
    monkeypatch.undo()
    assert copies == 1
    assert count["n"] == 5 + 1                                           # levels 0, 1, 8, 16 and 29 hold tracks
    same_match(got, want)


@gpu
def test_match_behind_a_busy_stream(ctx):
    """SortStore.match with a busy non-default stream as torch's current one: the states arrive on that stream behind a prefix of matmuls, and only
    that stream is synchronised (tests/test_sort_store_streams.py)."""
    import torch
    from tests.test_streams_gpu import Busy, behind
    busy = Busy()
    st, metric, feats, xyah, tlwh = scene(ctx)
    true = [st.mean.clone(), st.cov.clone()]
    poison = [torch.roll(true[0], 5, 0), torch.roll(true[1], 5, 0)]
    want = r_match(st, metric, SLOTS, IDS, AGES, CONFIRMED, feats, xyah, tlwh, 0.7, 6, 0.98)

    def call(x, o, stream):
        st.mean, st.cov = x
        m, ut, ud = st.match(metric, SLOTS, IDS, AGES, CONFIRMED, feats, xyah, tlwh, 0.7, cascade_depth=6, mc_lambda=0.98)
        return np.asarray(m, dtype=np.int64).reshape(-1, 2), np.asarray(sorted(ut), dtype=np.int64), np.asarray(ud, dtype=np.int64)
    _, got = behind(busy, "SortStore.match", call, true=true, poison=poison, form="current", host=True)
    busy.report()
    same_match(([tuple(p) for p in got[2].tolist()], got[3].tolist(), got[4].tolist()), want)
    assert len(got[2]) == 5
