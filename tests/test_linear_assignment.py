"""Linear assignment on the device: busca_linear_assignment (include/busca_assign.h) and its mirrors in busca_amd.tracking
(linear_assignment, linear_assignment_batch, min_cost_matching, associate_round).

The reference is tests/golden/assign.npz, written by tests/golden/make_golden_assign.py.  Both adapter routes solve one problem: for a
limit t, the partial matching M of pairs with c_ij < t that minimises the sum of (c_ij - t) over M.  The checkers are the two scipy
restatements below: lap.lapjv(extend_cost=True, cost_limit=t) as its padded square problem (`r_padded`), and min_cost_matching's
clamped rectangular problem (`r_clamped`).  The fixture's generic cases have a unique optimum (the generator proves it), so matches are
compared exactly; its tie cases pin the optimal objective only, and the kernel's potentials are checked as a certificate of optimality.

Tolerances, none of them measured: the objective of k matches against a host sum, k * eps * sum |c| (two float64 summation orders); the
reduced objective of a tie case, 64 * eps * sum |c_ij - t| over the matches; the certificate, 64 * eps * (|c_ij| + |t|) per entry."""
import os
import re
import types

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "assign.npz")
KALMAN = os.path.join(ROOT, "tests", "golden", "kalman.npz")
EPS = np.finfo(np.float64).eps
INF, NAN = np.inf, np.nan

# (matrix, limit, row -> column) written by hand
HAND = [
    ("1x1 below", [[0.3]], 0.8, [0]),
    ("1x1 above", [[0.9]], 0.8, [-1]),
    ("1x1 equal", [[0.8]], 0.8, [-1]),                                           # the test is a strict <
    ("greedy is wrong", [[0.1, 0.2], [0.15, 0.9]], 0.8, [1, 0]),
    # rows 0 and 1 could both be matched through the chain 1 -> col 0, 0 -> col 1 (-0.05 - 0.01), but row 0 alone on col 0 (-0.7) is better
    ("unmatched beats the chain", [[0.1, 0.79, 0.95], [0.75, 0.9, 0.85], [0.99, 0.95, 0.3]], 0.8, [0, -1, 2]),
    ("all inf", [[INF, INF, INF], [INF, INF, INF]], 0.8, [-1, -1]),
    ("nan beside a pair", [[NAN, 0.2], [0.3, NAN]], 0.8, [1, 0]),
    ("n > m", [[0.5, 0.1], [0.2, 0.6], [0.3, 0.25]], 0.8, [1, 0, -1]),
    ("n < m", [[0.5, 0.2, 0.3], [0.1, 0.6, 0.25]], 0.8, [1, 0]),
]


# ---- the restatements ---------------------------------------------------------------------------------------------------
def r_padded(c, t):
    """lap.lapjv(c, extend_cost=True, cost_limit=t): the (n + m) square matrix with t / 2 beside the costs and 0 in the far corner."""
    n, m = c.shape
    big = np.full((n + m, n + m), t / 2.0)
    big[n:, m:] = 0.0
    big[:n, :m] = np.where(np.isnan(c), INF, c)
    rows, cols = linear_sum_assignment(big)
    x = np.full(n, -1, dtype=np.int64)
    for r, j in zip(rows, cols):
        if r < n and j < m and c[r, j] < t:
            x[r] = j
    return x


def r_clamped(c, t):
    """min_cost_matching, linear_assignment.py:59-85: inadmissible entries clamped to t, the rectangular problem, clamped pairs dropped."""
    rows, cols = linear_sum_assignment(np.where(c < t, c, t))
    x = np.full(c.shape[0], -1, dtype=np.int64)
    for r, j in zip(rows, cols):
        if c[r, j] < t:
            x[r] = j
    return x


def reduced(c, t, x):
    rows = np.nonzero(x >= 0)[0]
    return float((c[rows, x[rows]] - t).sum())


def triple_of(x, m):
    """What matching.linear_assignment returns for the row -> column vector x."""
    rows = np.nonzero(x >= 0)[0]
    taken = set(int(j) for j in x[rows])
    return np.stack([rows, x[rows]], 1).reshape(-1, 2), np.nonzero(x < 0)[0], np.array([j for j in range(m) if j not in taken], dtype=np.int64)


_CACHE = {}


def gold():
    if "g" not in _CACHE:
        with np.load(GOLD) as f:
            _CACHE["g"] = {k: f[k] for k in f.files}
    return _CACHE["g"]


def case(name):
    """(cost matrix, limit, fixture row -> column) of a generic case; the matrix is rebuilt from its seed once."""
    if name not in _CACHE:
        from busca_amd import synth
        g = gold()
        kind, seed, n, m, inf_frac, t = g["params"][list(g["names"]).index(name)]
        c = synth.tracker_costs(int(seed), int(n), int(m), float(inf_frac)) if int(kind) == 0 else synth.uniform_costs(int(seed), int(n), int(m))
        c.setflags(write=False)
        _CACHE[name] = (c, float(t), g["x_" + name].astype(np.int64))
    return _CACHE[name]


def mcm_case(q):
    from busca_amd import synth
    g = gold()
    seed, nt, nd, max_distance = g["mcm_params"][q]
    return synth.uniform_costs(int(seed), int(nt), int(nd), 0.0, 1.5), float(max_distance)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_symbol_declared_typed_and_exported():
    from busca_amd.build import build
    build()
    from busca_amd import _lib

    def declared(header):
        hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return set(re.findall(r"\b(busca_[a-z0-9_]+)\s*\(", hdr))
    assert declared("busca_assign.h") == {"busca_linear_assignment"} == set(_lib.ASSIGN_SIGNATURES)
    assert "busca_linear_assignment" not in declared("busca_hip.h") and "busca_linear_assignment" not in _lib.SIGNATURES
    assert len(declared("busca_hip.h")) == 37
    lib = _lib.load()
    fn = lib.busca_linear_assignment
    assert fn.restype is not None and len(fn.argtypes) == 13
    assert lib.busca_version() // 1000 == 2 and lib.busca_version() % 1000 >= 1


def test_fixture_contents():
    g = gold()
    names = list(g["names"])
    assert len(names) == len(set(names)) == len(g["params"]) == len(g["objective"])
    for want in ("iou_t50", "iou_t80", "iou_t90", "iou_inf_t50", "iou_inf_t80", "iou_inf_t90", "cols63", "cols64", "cols65", "cols255", "cols256",
                 "cols257", "switch140", "switch141", "dense64", "dense128x96", "dense256", "sparse1000"):
        assert want in names
    for name in names:
        c, t, x = case(name)
        assert x.shape == (c.shape[0],) and x.max() < c.shape[1] and (x >= 0).any()
    assert os.path.getsize(GOLD) < 1 << 20


def test_restatements_reproduce_the_fixture():
    g = gold()
    for k, name in enumerate(g["names"]):
        c, t, x = case(name)
        assert np.array_equal(r_padded(c, t), x), name
        assert np.array_equal(r_clamped(c, t), x), name
        assert abs(reduced(c, t, x) - g["objective"][k]) <= 64 * EPS * abs(g["objective"][k]), name
    for k, name in enumerate(g["tie_names"]):
        c, t = g["tie_cost_" + name], float(g["tie_limit"][k])
        for solve in (r_padded, r_clamped):
            got = reduced(c, t, solve(c, t))
            assert abs(got - g["tie_objective"][k]) <= 64 * EPS * max(abs(got), abs(g["tie_objective"][k])), (name, solve.__name__)
    for q in range(len(g["mcm_params"])):
        full, max_distance = mcm_case(q)
        ti, di = g["mcm_ti_%d" % q], g["mcm_di_%d" % q]
        sub = full[np.ix_(ti, di)]
        for solve in (r_padded, r_clamped):
            x = solve(sub, max_distance + 1e-5)
            pairs = [(int(ti[r]), int(di[x[r]])) for r in range(len(ti)) if x[r] >= 0]
            assert pairs == [tuple(p) for p in g["mcm_matches_%d" % q].tolist()], (q, solve.__name__)
    for name, c, t, want in HAND:
        c = np.array(c, dtype=np.float64)
        assert r_padded(c, t).tolist() == want and r_clamped(c, t).tolist() == want, name


def test_empty_inputs_need_no_context(monkeypatch):
    from busca_amd import geometry, tracking

    def no_context(*a, **k):
        raise AssertionError("an empty input must not create a context")
    monkeypatch.setattr(geometry, "default_context", no_context)
    for n, m in ((0, 0), (0, 4), (3, 0)):
        matches, ua, ub = tracking.linear_assignment(np.zeros((n, m)), 0.8)
        assert matches.shape == (0, 2) and matches.dtype == np.empty((0, 2), dtype=int).dtype
        assert ua == tuple(range(n)) and ub == tuple(range(m))                   # matching.py:40-41
    assert tracking.linear_assignment_batch([], 0.8) == []
    (m0, a0, b0), = tracking.linear_assignment_batch([np.zeros((0, 5))], 0.8)
    assert m0.shape == (0, 2) and a0 == () and b0 == (0, 1, 2, 3, 4)
    ti = [4, 7]
    matches, ut, ud = tracking.min_cost_matching(no_context, 0.2, list(range(9)), [], ti, [])
    assert matches == [] and ut is ti and ud == []                               # linear_assignment.py:56-57
    matches, ut, ud = tracking.min_cost_matching(no_context, 0.2, [], list(range(3)))
    assert matches == [] and len(ut) == 0 and list(ud) == [0, 1, 2]
    assert tracking.associate_round([], [object()] * 3, 0.8) [1:] == ((), (0, 1, 2))


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from busca_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))                 # a copy: fixture matrices are read-only


def _stream():
    import torch
    return torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream


def gpu_solve(ctx, cost, limit, dims=None):
    """busca_linear_assignment with every output requested, on cost [n,m] or [batch,n,m]; the outputs start out as garbage."""
    import torch
    cost = np.asarray(cost, dtype=np.float64)
    single = cost.ndim == 2
    b, n, m = (1,) + cost.shape if single else cost.shape
    dc = _dev(cost)
    dev = dc.device
    r2c = torch.full((b, n), -7, dtype=torch.int32, device=dev)
    c2r = torch.full((b, m), -7, dtype=torch.int32, device=dev)
    duals = torch.full((b, n + m), -7.0, dtype=torch.float64, device=dev)
    obj = torch.full((b,), -7.0, dtype=torch.float64, device=dev)
    st = torch.full((b,), -7, dtype=torch.int32, device=dev)
    dd = None if dims is None else _dev(np.asarray(dims, dtype=np.int32))
    ctx.check(ctx.lib.busca_linear_assignment(ctx.h, dc.data_ptr(), b, n, m, None if dd is None else dd.data_ptr(), float(limit), r2c.data_ptr(),
                                              c2r.data_ptr(), duals.data_ptr(), obj.data_ptr(), st.data_ptr(), _stream()))
    out = dict(x=r2c.cpu().numpy().astype(np.int64), y=c2r.cpu().numpy().astype(np.int64), duals=duals.cpu().numpy(), objective=obj.cpu().numpy(),
               status=st.cpu().numpy())
    return {k: v[0] for k, v in out.items()} if single else out


def check_solution(c, t, r, want_x=None):
    """Status, consistency of the two match vectors, admissibility, the objective; and the matches when the optimum is unique."""
    n, m = c.shape
    x, y = r["x"], r["y"]
    assert r["status"] == 0
    assert x.shape == (n,) and y.shape == (m,) and x.min() >= -1 and x.max() < m and y.min() >= -1 and y.max() < n
    rows = np.nonzero(x >= 0)[0]
    assert all(y[x[i]] == i for i in rows) and (y >= 0).sum() == len(rows)
    assert (c[rows, x[rows]] < t).all()
    host = float(c[rows, x[rows]].sum())
    assert abs(r["objective"] - host) <= max(len(rows), 1) * EPS * float(np.abs(c[rows, x[rows]]).sum())
    if want_x is not None:
        assert np.array_equal(x, want_x)


def check_certificate(c, t, r):
    """The returned potentials prove optimality: dual feasible, complementary slackness against the returned matching."""
    n, m = c.shape
    x, y, u, v = r["x"], r["y"], r["duals"][:n], r["duals"][n:]
    adm = c < t
    tol = 64 * EPS * (np.abs(np.where(adm, c, 0.0)) + abs(t))
    slack = np.where(adm, (c - t) - (u[:, None] + v[None, :]), 0.0)
    assert (slack[adm] >= -tol[adm]).all()
    rows = np.nonzero(x >= 0)[0]
    assert (np.abs(slack[rows, x[rows]]) <= tol[rows, x[rows]]).all()
    assert (u <= 0).all() and (v <= 0).all()
    assert (u[x < 0] == 0).all() and (v[y < 0] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name,c,t,want", HAND, ids=[h[0] for h in HAND])
def test_hand_written_cases(ctx, name, c, t, want):
    c = np.array(c, dtype=np.float64)
    r = gpu_solve(ctx, c, t)
    check_solution(c, t, r, np.array(want))
    check_certificate(c, t, r)


GENERIC_SMALL = ["iou_t50", "iou_t80", "iou_t90", "iou_inf_t50", "iou_inf_t80", "iou_inf_t90", "cols63", "cols64", "cols65", "cols255", "cols256", "cols257"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", GENERIC_SMALL + ["dense64", "dense128x96", "dense256", "sparse1000"])
def test_fixture_generic_cases(ctx, name):
    c, t, x = case(name)
    r = gpu_solve(ctx, c, t)
    check_solution(c, t, r, x)
    k = list(gold()["names"]).index(name)
    assert abs(reduced(c, t, r["x"]) - gold()["objective"][k]) <= 64 * EPS * abs(gold()["objective"][k])
    if name.startswith("dense"):
        assert (c < t).all() and (r["x"] >= 0).sum() == min(c.shape)             # every entry admissible: the long-path regime
    if name == "sparse1000":
        assert c.shape == (1000, 1000) and 1 <= (c < t).sum(1).mean() <= 8
    # the same input again: the same bits
    r2 = gpu_solve(ctx, c, t)
    assert all(np.array_equal(r[k], r2[k]) for k in r)


@pytest.mark.gpu
def test_lds_and_global_paths_agree(ctx):
    c, t, x = case("switch140")
    assert ctx.get_option("assign_stage") == -1
    staged = gpu_solve(ctx, c, t)
    assert ctx.get_option("last_assign_staged") == 1                             # 140 x 140 doubles fit beside the solver's state in 160 KiB ...
    check_solution(c, t, staged, x)
    ctx.set_option("assign_stage", 0)
    try:
        glob = gpu_solve(ctx, c, t)
        assert ctx.get_option("last_assign_staged") == 0
    finally:
        ctx.set_option("assign_stage", -1)
    assert all(np.array_equal(staged[k], glob[k]) for k in staged)               # matches, potentials and objective, bit for bit
    c, t, x = case("switch141")
    r = gpu_solve(ctx, c, t)
    assert ctx.get_option("last_assign_staged") == 0                             # ... 141 x 141 do not
    check_solution(c, t, r, x)
    check_certificate(c, t, r)


@pytest.mark.gpu
def test_tie_cases(ctx):
    g = gold()
    for k, name in enumerate(g["tie_names"]):
        c, t = g["tie_cost_" + name], float(g["tie_limit"][k])
        r = gpu_solve(ctx, c, t)
        check_solution(c, t, r)
        rows = np.nonzero(r["x"] >= 0)[0]
        got = reduced(c, t, r["x"])
        bound = 64 * EPS * max(float(np.abs(c[rows, r["x"][rows]] - t).sum()), abs(float(g["tie_objective"][k])))
        print("%s: reduced objective %.17g, fixture %.17g, bound %.3g" % (name, got, g["tie_objective"][k], bound))
        assert abs(got - g["tie_objective"][k]) <= bound, name
        check_certificate(c, t, r)


@pytest.mark.gpu
def test_batch_equals_one_by_one(ctx):
    names = ["batch%d" % k for k in range(8)]
    cases = [case(nm) for nm in names]
    n, m = max(c.shape[0] for c, _, _ in cases), max(c.shape[1] for c, _, _ in cases)
    slab = np.full((8, n, m), NAN)                                               # the padding is NaN: it is never read as data
    for k, (c, _, _) in enumerate(cases):
        slab[k, :c.shape[0], :c.shape[1]] = c
    dims = [c.shape for c, _, _ in cases]
    r = gpu_solve(ctx, slab, 0.8, dims)
    assert (r["status"] == 0).all()
    for k, (c, t, x) in enumerate(cases):
        nk, mk = c.shape
        one = gpu_solve(ctx, c, t)
        assert np.array_equal(r["x"][k, :nk], one["x"]) and np.array_equal(r["y"][k, :mk], one["y"]) and np.array_equal(one["x"], x)
        assert (r["x"][k, nk:] == -1).all() and (r["y"][k, mk:] == -1).all()
        assert np.array_equal(r["duals"][k, :nk], one["duals"][:nk]) and np.array_equal(r["duals"][k, n:n + mk], one["duals"][nk:])
        assert (r["duals"][k, nk:n] == 0).all() and (r["duals"][k, n + mk:] == 0).all()
        assert r["objective"][k] == one["objective"]
    # a size pair outside its slab is refused for that problem alone
    dims[3] = (n + 1, 1)
    r = gpu_solve(ctx, slab, 0.8, dims)
    assert r["status"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and (r["x"][3] == -1).all() and (r["y"][3] == -1).all() and np.isnan(r["objective"][3])
    assert np.array_equal(r["x"][4, :40], cases[4][2])


@pytest.mark.gpu
def test_non_finite_arithmetic_ends_with_status_1(ctx):
    # a -inf cost makes every distance -inf: the solver stops at its bound instead of spinning, and says so
    c = np.array([[0.2, -INF], [0.3, 0.4]])
    r = gpu_solve(ctx, c, 0.8)
    assert r["status"] == 1 and (r["x"] == -1).all() and (r["y"] == -1).all() and (r["duals"] == 0).all() and np.isnan(r["objective"])
    from busca_amd import _lib, tracking
    with pytest.raises(_lib.BuscaError, match="linear_assignment"):
        tracking.linear_assignment(c, 0.8, ctx=ctx)


@pytest.mark.gpu
def test_python_linear_assignment(ctx):
    import torch
    from busca_amd import tracking
    c, t, x = case("iou_inf_t80")
    want = triple_of(x, c.shape[1])
    host = tracking.linear_assignment(np.array(c), t, ctx=ctx)
    dc = _dev(c)
    dev = tracking.linear_assignment(dc, t, ctx=ctx)
    for got in (host, dev):
        assert isinstance(got[0], np.ndarray) and got[0].shape[1] == 2 and got[0].dtype.kind == "i"
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert np.array_equal(dc.cpu().numpy(), c)                                   # the caller's tensor is not written
    # float32 host input, as an adapter's own IoU code gives it
    got = tracking.linear_assignment(c.astype(np.float32), t, ctx=ctx)
    assert all(np.array_equal(a, b) for a, b in zip(got, triple_of(r_padded(c.astype(np.float32).astype(np.float64), t), c.shape[1])))
    # the batch: differing shapes, one launch; host arrays and device tensors alike
    names = ["batch%d" % k for k in range(8)]
    mats = [np.array(case(nm)[0]) for nm in names]
    for inputs in (mats + [np.zeros((0, 3))], [_dev(a) for a in mats]):
        res = tracking.linear_assignment_batch(inputs, 0.8, ctx=ctx)
        assert len(res) == len(inputs)
        for nm, got in zip(names, res):
            assert all(np.array_equal(a, b) for a, b in zip(got, triple_of(case(nm)[2], case(nm)[0].shape[1])))
    assert res[-1][0].shape[1] == 2
    with pytest.raises(ValueError, match="2048"):
        tracking.linear_assignment(torch.zeros(1, 2049, dtype=torch.float64, device=dc.device), 0.5, ctx=ctx)


@pytest.mark.gpu
def test_python_min_cost_matching(ctx):
    from busca_amd import tracking
    g = gold()
    for q in range(len(g["mcm_params"])):
        full, max_distance = mcm_case(q)
        nt, nd = full.shape
        ti, di = g["mcm_ti_%d" % q], g["mcm_di_%d" % q]
        calls = []

        def metric(tracks, dets, a, b):
            calls.append((len(tracks), len(dets)))
            return full[np.ix_(a, b)].copy()
        matches, ut, ud = tracking.min_cost_matching(metric, max_distance, list(range(nt)), list(range(nd)), list(ti), list(di), ctx=ctx)
        assert calls == [(nt, nd)]
        assert [tuple(int(v) for v in p) for p in matches] == [tuple(p) for p in g["mcm_matches_%d" % q].tolist()]
        assert set(int(v) for v in ut) == set(g["mcm_ut_%d" % q].tolist()) and len(ut) == len(g["mcm_ut_%d" % q])
        assert set(int(v) for v in ud) == set(g["mcm_ud_%d" % q].tolist()) and len(ud) == len(g["mcm_ud_%d" % q])
        assert all(full[a, b] <= max_distance for a, b in matches)
    # default indices, a metric that answers with a device tensor
    full, max_distance = mcm_case(0)
    matches, ut, ud = tracking.min_cost_matching(lambda tr, de, a, b: _dev(full[np.ix_(a, b)]), max_distance, list(range(full.shape[0])),
                                                 list(range(full.shape[1])), ctx=ctx)
    x = r_clamped(full, max_distance + 1e-5)
    assert [tuple(int(v) for v in p) for p in matches] == [(r, int(x[r])) for r in range(len(x)) if x[r] >= 0]
    assert sorted(int(v) for v in ut) == [r for r in range(len(x)) if x[r] < 0]


def _tracks(mean, cov, states):
    return [types.SimpleNamespace(mean=mean[i].copy(), covariance=cov[i].copy(), state=int(states[i])) for i in range(len(mean))]


def _detections(xyah, scores):
    out = []
    for k, z in enumerate(xyah):
        w = z[2] * z[3]
        tlwh = np.array([z[0] - w / 2, z[1] - z[3] / 2, w, z[3]])
        out.append(types.SimpleNamespace(tlwh=tlwh, tlbr=np.array([tlwh[0], tlwh[1], tlwh[0] + tlwh[2], tlwh[1] + tlwh[3]]), score=float(scores[k])))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("fuse", [False, True])
def test_associate_round_equals_predicted_cost_then_the_restatement(ctx, fuse):
    from busca_amd import synth, tracking
    with np.load(KALMAN) as f:
        mean, cov, meas = f["mean"], f["cov"], f["gate_meas"]
    states = np.arange(len(mean)) % 3
    scores = synth.uniform(72, "scores", (len(meas),), 0.3, 1.0).astype(np.float64)
    dets = _detections(meas, scores)
    thresh = 0.8
    a, b = _tracks(mean, cov, states), _tracks(mean, cov, states)
    cost = tracking.predicted_cost(a, dets, det_scores=scores, fuse_motion=fuse, ctx=ctx)
    want = triple_of(r_padded(cost, thresh), len(dets))
    got = tracking.associate_round(b, dets, thresh, det_scores=scores, fuse_motion=fuse, ctx=ctx)
    assert len(want[0]) >= 10 and len(want[1]) >= 10                             # matched and unmatched tracks both
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
    assert np.array_equal(np.stack([t.mean for t in a]), np.stack([t.mean for t in b]))
    assert np.array_equal(np.stack([t.covariance for t in a]), np.stack([t.covariance for t in b]))
    assert b[0].mean.shape == (8,) and b[0].covariance.shape == (8, 8)
    # no detections: every track unmatched, the states still predicted
    c = _tracks(mean[:4], cov[:4], states[:4])
    m0, ut, ud = tracking.associate_round(c, [], thresh, fuse_motion=fuse, ctx=ctx)
    assert m0.shape == (0, 2) and ut == (0, 1, 2, 3) and ud == ()
    assert np.array_equal(np.stack([t.mean for t in c]), np.stack([t.mean for t in a[:4]]))
    if fuse:                                                                     # LinAlgError exactly where predicted_cost raises it
        bad = cov.copy()
        bad[5, :4, :4] = -np.eye(4)
        for fn, args in ((tracking.predicted_cost, ()), (tracking.associate_round, (thresh,))):
            with pytest.raises(np.linalg.LinAlgError, match="track 5"):
                fn(_tracks(mean, bad, states), dets, *args, fuse_motion=True, ctx=ctx)
    else:
        bad = cov.copy()
        bad[5, :4, :4] = -np.eye(4)
        tracking.associate_round(_tracks(mean, bad, states), dets, thresh, ctx=ctx)       # no gate, no factorisation: nothing to raise


@pytest.mark.gpu
def test_argument_errors(ctx):
    lib, h = ctx.lib, ctx.h
    z = None
    assert lib.busca_linear_assignment(h, z, 0, 4, 4, z, 0.8, z, z, z, z, z, z) == 0
    assert lib.busca_linear_assignment(h, z, 2, 0, 4, z, 0.8, z, z, z, z, z, z) == 0
    assert lib.busca_linear_assignment(h, z, 2, 4, 0, z, 0.8, z, z, z, z, z, z) == 0
    c = _dev(np.full((2, 3), 0.25))
    x = _dev(np.full(2, -7, dtype=np.int32))
    cp, xp = c.data_ptr(), x.data_ptr()
    assert lib.busca_linear_assignment(h, z, 1, 2, 3, z, 0.8, xp, z, z, z, z, z) == -1
    assert lib.busca_linear_assignment(h, cp, 1, 2, 3, z, 0.8, z, z, z, z, z, z) == -1
    assert lib.busca_linear_assignment(h, cp, -1, 2, 3, z, 0.8, xp, z, z, z, z, z) == -1
    assert lib.busca_linear_assignment(h, cp, 1, -2, 3, z, 0.8, xp, z, z, z, z, z) == -1
    assert lib.busca_linear_assignment(h, cp, 1, 2, -3, z, 0.8, xp, z, z, z, z, z) == -1
    assert lib.busca_linear_assignment(h, cp, 1, 2, 3, z, NAN, xp, z, z, z, z, z) == -1
    assert b"busca_linear_assignment" in lib.busca_last_error(h)
    assert lib.busca_linear_assignment(h, cp, 1, 2049, 3, z, 0.8, xp, z, z, z, z, z) == -1
    assert b"busca_linear_assignment" in lib.busca_last_error(h) and b"2048" in lib.busca_last_error(h)
    assert (x.cpu().numpy() == -7).all()                                         # nothing was launched
    # every optional output may be NULL
    assert lib.busca_linear_assignment(h, cp, 1, 2, 3, z, 0.8, xp, z, z, z, z, _stream()) == 0
    assert x.cpu().numpy().tolist() == [0, 1]
