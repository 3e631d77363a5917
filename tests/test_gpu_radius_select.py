"""GPU: the selection of the uniform-grid radius search (csrc/radius_neighbors.hip: radius_grid_search_kernel) at its own edges -- the rank
sort of fewer than 64 staged hits, the staging drain at 64 and 128, exact ties at and around the cut, arrival order, batches, several queries
per wave with the largest count handed in per workgroup, and a grid built into a workspace that held other bytes.  The yardstick is the exhaustive kernel of the same file, which shares none of that (sorted insertion,
no grid, one query per wave slot): table, max_count and the sorted list of flagged tie rows are compared for equality; two cases also go
against the C oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

R = 0.1
HITS = (0, 1, 2, 7, 8, 9, 31, 32, 33, 62, 63, 64, 65, 100, 127, 128, 129, 200)


def _search(s, sl, radius, limit, q, ql, grid):
    """(table, max_count list, sorted tie rows) of one search: through `grid` (a RadiusGrid or True: build one), or exhaustive (False)."""
    from se3et_amd import ops
    ties = (torch.full((max(q.shape[0], 1),), -1, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda'))
    if grid is False:
        old, ops.GRID_SEARCH_MIN_SUPPORT = ops.GRID_SEARCH_MIN_SUPPORT, 10 ** 12
        try:
            tab, mc = ops.radius_neighbors(q, s, ql, sl, radius, limit, ties=ties)
        finally:
            ops.GRID_SEARCH_MIN_SUPPORT = old
    else:
        g = ops.RadiusGrid(s, sl, radius) if grid is True else grid
        tab, mc = g.search(q, ql, limit, ties=ties)
    n = int(ties[1].item())
    return tab.cpu(), mc.tolist(), sorted(ties[0][:n].tolist())


def _assert_grid_equals_exhaustive(s, sl, radius, limit, q, ql, grid=True):
    s, q = s.cuda(), q.cuda()
    a, b = _search(s, sl, radius, limit, q, ql, grid), _search(s, sl, radius, limit, q, ql, False)
    assert a[1] == b[1], 'max_count %s against %s' % (a[1], b[1])
    assert torch.equal(a[0], b[0]), 'tables differ in rows %s' % torch.nonzero((a[0] != b[0]).any(1))[:8, 0].tolist()
    assert a[2] == b[2], 'flagged tie rows differ'
    return a


def _neighbourhood(g, k, centre, n_out=70, n_fill=300):
    """k points inside the ball of radius R around `centre` at distinct distances (0.05 R .. 0.95 R), n_out just outside it (1.05 R .. 1.7 R:
    inside the 3 x 3 x 3 cell block), n_fill spread over the unit cube away from the ball, and the cube's two corners (so that the grid's
    origin is 0 and its cells have edge R: ten cells per axis).  Near points first."""
    def shell(n, lo, hi):
        d = g.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return centre + d * (lo + (hi - lo) * (np.arange(n)[:, None] + 0.5) / max(n, 1)) * R
    fill = g.uniform(0, 1, (4 * n_fill, 3))
    fill = fill[np.linalg.norm(fill - centre, axis=1) > 1.8 * R][:n_fill]
    return np.concatenate([shell(k, 0.05, 0.95), shell(n_out, 1.05, 1.7), fill, [[0, 0, 0], [1, 1, 1]]]).astype(np.float32)


@pytest.mark.parametrize('limit', [1, 36, 38, 64])
def test_hit_count_sweep(limit):
    """One query per cloud with exactly k in-radius support points, every k of HITS stacked into one call: the rank sort alone (k < 64), the
    drain once (64 .. 127) and twice (128 ..) with and without a remainder.  Limit 64 with more than 64 hits must flag the row."""
    g = np.random.default_rng(11)
    centre = np.array([0.5, 0.5, 0.5])                   # next to a cell corner: the ball reaches into all 27 cells' eight inner ones
    clouds = [_neighbourhood(g, k, centre) for k in HITS]
    clouds = [c[g.permutation(len(c))] for c in clouds]
    s = torch.from_numpy(np.concatenate(clouds))
    sl = torch.tensor([len(c) for c in clouds])
    q = torch.from_numpy(np.tile(centre.astype(np.float32), (len(HITS), 1)))
    ql = torch.ones(len(HITS), dtype=torch.int64)
    tab, mc, rows = _assert_grid_equals_exhaustive(s, sl, R, limit, q, ql)
    assert mc == list(HITS)
    starts = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    for i, k in enumerate(HITS):
        kept = tab[i][tab[i] != s.shape[0]]
        assert len(kept) == min(k, limit) and ((kept >= starts[i]) & (kept < starts[i + 1])).all()
    assert rows == ([i for i, k in enumerate(HITS) if k > 64] if limit == 64 else [])


@pytest.mark.parametrize('k', [40, 150])
@pytest.mark.parametrize('order', ['near_last', 'near_first', 'shuffled'])
def test_memory_order(order, k):
    """The same neighbourhood, spread over the cells around a cell corner, stored near points last / first / shuffled: the cells decide in
    which order the hits arrive, the result is the (d2, index) order all the same."""
    g = np.random.default_rng(12)
    centre = np.array([0.5, 0.5, 0.5])
    pts = _neighbourhood(g, k, centre, n_out=120)
    if order == 'near_last':
        pts = pts[::-1].copy()
    elif order == 'shuffled':
        pts = pts[g.permutation(len(pts))]
    q = torch.from_numpy((centre + g.uniform(-0.01, 0.01, (8, 3))).astype(np.float32))
    for limit in (38, 64):
        tab, mc, _ = _assert_grid_equals_exhaustive(torch.from_numpy(pts), torch.tensor([len(pts)]), R, limit, q, torch.tensor([8]))
        assert (mc[0] < 64) == (k == 40)                 # 40: the rank sort alone; 150: through the drain


@pytest.mark.parametrize('radius', [0.07, 0.1])
@pytest.mark.parametrize('limit', [1, 7, 33, 36, 38, 64])
def test_exact_ties_on_a_lattice(limit, radius):
    """Support = a 16^3 lattice of spacing 1/32 (exact in float32), stored shuffled.  A query on a lattice point sees shells of 1, 6, 12, 8, 6,
    24 (57 points: radius 0.07, rank sort) and further 24, 12, 30, 24 (147: radius 0.1, two drains) equal distances: limit 1 has its ties only
    beyond the cut, 7 and 33 cut between two shells, 36 / 38 / 64 cut inside one.  Half-step queries tie differently, random ones not at all."""
    g = np.random.default_rng(13)
    ax = np.arange(16) / 32.0
    lat = np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(-1, 3)
    lat = lat[g.permutation(len(lat))].astype(np.float32)
    on = lat[g.choice(len(lat), 150, replace=False)]
    half = on[:80] + np.float32([1 / 64.0, 0, 0])
    rnd = g.uniform(0, 15 / 32.0, (70, 3)).astype(np.float32)
    q = torch.from_numpy(np.concatenate([on, half, rnd]))
    tab, mc, rows = _assert_grid_equals_exhaustive(torch.from_numpy(lat), torch.tensor([len(lat)]), radius, limit, q, torch.tensor([len(q)]))
    assert mc[0] == (57 if radius == 0.07 else 147)
    flagged = set(rows)
    if limit == 1:
        assert not flagged & set(range(150)), 'a tie beyond the cut only must not flag the row'
    else:
        assert len(flagged & set(range(150))) == 150
    # index order inside every run of equal distances
    s = torch.from_numpy(lat)
    for r in range(0, len(q), 7):
        idx = tab[r][tab[r] != len(lat)]
        d = ((q[r] - s[idx]) ** 2)
        d2 = (d[:, 0] + d[:, 1]) + d[:, 2]
        assert (d2[1:] >= d2[:-1]).all()
        same = d2[1:] == d2[:-1]
        assert (idx[1:][same] > idx[:-1][same]).all()


def test_batches_empty_clouds_and_outside_queries():
    """Three clouds of different sizes in one call, one of them without queries; queries outside the support box; a far query: all padding."""
    g = np.random.default_rng(14)
    sizes, qs = [900, 300, 1500], [200, 0, 351]
    s = torch.from_numpy(np.concatenate([g.uniform(0, sc, (n, 3)) for n, sc in zip(sizes, (1.0, 0.4, 1.3))]).astype(np.float32))
    q = g.uniform(-0.25, 1.25, (sum(qs), 3)).astype(np.float32)
    q[-1] = 100.0
    q[-2] = [0.5, 0.5, -0.09]
    q = torch.from_numpy(q)
    for radius, limit in ((0.1, 38), (0.22, 64), (0.04, 5)):
        tab, mc, _ = _assert_grid_equals_exhaustive(s, torch.tensor(sizes), radius, limit, q, torch.tensor(qs))
        assert (tab[-1] == s.shape[0]).all()
        assert mc[1] == 0


@pytest.mark.parametrize('nq', [8191, 8192, 12301, 32767, 33001])
def test_several_queries_per_wave(nq):
    """A wave takes nq / 4096 queries (1 .. 8) one after the other and the workgroup hands in ONE largest count: both sides of the steps at
    8 192 (one to two) and 32 768 queries (seven to eight), with clouds whose query counts end in the middle of a workgroup's and of a
    wave's share, one query alone and a cloud without any; the first or the last cloud holds a dense spot that only a few queries see."""
    g = np.random.default_rng(17 + nq)
    sizes = [700, 400, 5, 900]
    clouds = [g.uniform(0, 1, (n, 3)) for n in sizes]
    spot = (0, 3)[nq % 2]
    clouds[spot][:90] = clouds[spot][0] + g.uniform(-0.02, 0.02, (90, 3))          # one dense spot: the largest count, seen by few queries
    s = torch.from_numpy(np.concatenate(clouds).astype(np.float32))
    qs = [nq - 1 - (nq // 3), 1, 0, nq // 3]
    q = torch.from_numpy(g.uniform(-0.05, 1.05, (nq, 3)).astype(np.float32))
    tab, mc, _ = _assert_grid_equals_exhaustive(s, torch.tensor(sizes), R, 38, q, torch.tensor(qs))
    assert mc[2] == 0 and max(mc) > 38


@pytest.mark.parametrize('second', [0.31, 0.03])
def test_rebuild_into_a_stale_workspace(second):
    """A grid rebuilt into a workspace full of 0xFF bytes, once coarser and once finer than what the workspace held before: nothing may be
    read that the build did not write."""
    from se3et_amd import ops
    g = np.random.default_rng(15)
    sizes = [1100, 700]
    s = torch.from_numpy(g.uniform(0, 1, (sum(sizes), 3)).astype(np.float32)).cuda()
    sl, ql = torch.tensor(sizes), torch.tensor([300, 200])
    q = torch.from_numpy(g.uniform(-0.1, 1.1, (500, 3)).astype(np.float32)).cuda()
    grid = ops.RadiusGrid(s, sl, R)
    _assert_grid_equals_exhaustive(s, sl, R, 38, q, ql, grid)
    for radius in (second, R):
        grid.ws.fill_(0xFF)
        ops.check(ops.lib().se3_radius_grid_build(s.data_ptr(), grid.ns, grid.lengths, grid.batch, radius, grid.ws.data_ptr(), grid.ws.numel(),
                                                  ops._stream()), 'se3_radius_grid_build')
        grid.radius = float(radius)
        _assert_grid_equals_exhaustive(s, sl, radius, 38 if radius < 0.3 else 64, q, ql, grid)


@pytest.mark.parametrize('radius,mean_hits', [(0.11, 8), (0.18, 35)])
def test_bench_like_clouds_match_the_c_oracle(radius, mean_hits):
    """Two clouds of 1 500 points at the hit counts of the benchmark's first and last stage, against the C oracle and the exhaustive kernel."""
    from oracle import native
    g = np.random.default_rng(16)
    s = torch.from_numpy(g.uniform(0, 1, (3000, 3)).astype(np.float32))
    sl = torch.tensor([1500, 1500])
    want = native.radius_search(s, s, sl, sl, radius, 38)
    tab, mc, _ = _assert_grid_equals_exhaustive(s, sl, radius, 38, s, sl)
    hits = torch.cat([(torch.cdist(c.double(), c.double()) < radius).sum(1) for c in (s[:1500], s[1500:])]).double().mean()
    assert 0.75 * mean_hits < float(hits) < 1.25 * mean_hits
    assert torch.equal(tab[:, :want.shape[1]], want) and (tab[:, want.shape[1]:] == 3000).all()
