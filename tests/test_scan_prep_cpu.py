"""CPU: the scan preparation (se3et_amd/scan_prep.py, csrc/voxel_downsample.hip, csrc/knn_normals.hip, csrc/pair_grid.h) without a GPU.

  - the library's host entries (se3_debug_voxel_downsample_host, se3_debug_knn_host, se3_debug_knn_normals_host: the __host__ __device__
    text the kernels run) against the numpy twin (tests/scan_prep_twin.py) at the demands of tests/scan_prep_fixture.py, on the fixture
    clouds and the edge cases;
  - the twin against the reference's own results in tests/golden/scan_prep.npz (regularize_normals exactly, the modified chamfer distance
    within the float32 bound of the reference's cancelling distance expression);
  - argument validation of every new entry, the refusal of CPU tensors."""
import os

import numpy as np
import pytest
import torch

import scan_prep_fixture as F
import scan_prep_twin as twin

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scan_prep.npz')


_ptr, _lib, host_voxel, host_knn, host_normals = F._ptr, F._lib, F.host_voxel, F.host_knn, F.host_normals


@pytest.mark.parametrize('name', F.CLOUDS)
def test_fixture_facts(name):
    _, _, counts = twin.voxel_downsample(F.cloud(name), F.VOXEL_SIZES[name])
    assert (len(counts), int(counts.max())) == F.VOXEL_FACTS[name] and counts.sum() == len(F.cloud(name))
    _, d2 = F.twin_knn(name)
    assert not (d2[:, F.KNN - 1] == d2[:, F.KNN]).any()                 # no distance tie at the 33rd place
    w = F.twin_normals(name)[3]
    assert ((w[:, 1] - w[:, 0]) / w[:, 2]).min() >= F.GAP_FACTS[name]


# ---- voxel downsampling -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('name', F.CLOUDS)
def test_host_voxel_entry_equals_the_twin(name, dtype):
    p, nr = F.cloud(name).astype(dtype), F.fake_normals(name).astype(dtype)
    for v in F.VOXEL_SIZES.values():
        tm, tn, _ = twin.voxel_downsample(p, v, nr)
        m, n, status = host_voxel(p, v, nr)
        assert status == 0 and np.array_equal(m, tm) and np.array_equal(n, tn)          # counts, order and every mean bit-equal
        m2, none, _ = host_voxel(p, v)
        assert none is None and np.array_equal(m2, tm)


voxel_edge_cases = F.voxel_edge_cases


@pytest.mark.parametrize('name', list(voxel_edge_cases()))
def test_host_voxel_entry_on_the_edge_cases(name):
    p, v, voxels = voxel_edge_cases()[name]
    nr = np.random.default_rng(1).standard_normal(p.shape)
    tm, tn, counts = twin.voxel_downsample(p, v, nr)
    m, n, status = host_voxel(p, v, nr)
    assert status == 0 and np.array_equal(m, tm) and np.array_equal(n, tn)
    assert voxels is None or len(m) == voxels
    if name == 'faces':          # a point on a face belongs to the voxel above it: the quotient is the integer itself (row 0 is the minimum)
        idx = np.floor((p - (p.min(0) - 0.5 * v)) / v)
        assert np.array_equal(idx[1:], (p[1:] + 2.125) / 0.25) and (idx[0] == 0).all() and len(m) == len(np.unique(idx, axis=0))


def test_host_voxel_entry_refuses_what_the_contract_refuses():
    p = F.cloud('micro').astype(np.float64)
    far = int(np.argmax(p[:, 1]))
    wide = p.copy()
    wide[far, 1] = p[:, 1].min() + 0.01 * 2.0 ** 21                     # (max - o) / v = 2^21 + 0.5: one voxel too many
    assert host_voxel(wide, 0.01)[2] == 2 and len(host_voxel(wide, 0.01)[0]) == 0
    with pytest.raises(ValueError, match='too many voxels'):
        twin.voxel_downsample(wide, 0.01)
    wide[far, 1] = p[:, 1].min() + 0.01 * (2.0 ** 21 - 1)
    m, _, status = host_voxel(wide, 0.01)
    assert status == 0 and np.array_equal(m, twin.voxel_downsample(wide, 0.01)[0])
    bad = p.copy()
    bad[7, 2] = np.nan
    assert host_voxel(bad, 0.05)[2] == 1
    bad[7, 2] = np.inf
    assert host_voxel(bad, 0.05)[2] == 1
    assert host_voxel(p, 0.05, np.where(np.arange(600)[:, None] == 3, np.nan, p))[2] == 1


# ---- k nearest neighbours ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', F.CLOUDS)
def test_host_knn_entry_equals_the_twin(name):
    from scipy.spatial import cKDTree
    p = F.cloud(name)
    tidx, td2 = F.twin_knn(name)
    for k in (1, 3, 33, 64):
        for dtype in (np.float32, np.float64):
            idx, d2 = host_knn(p, k, dtype=dtype)
            assert np.array_equal(idx, tidx[:, :k]) and np.array_equal(d2, td2[:, :k])
        _, kd = cKDTree(p.astype(np.float64)).query(p.astype(np.float64), k=k)
        assert np.array_equal(np.sort(np.asarray(kd).reshape(len(p), k), 1), np.sort(tidx[:, :k], 1))      # the neighbour sets
    assert np.array_equal(tidx[:, 0], np.arange(len(p)))                # each point is its own first neighbour


@pytest.mark.parametrize('name', list(F.edge_clouds()))
def test_host_knn_entry_on_the_edge_cases(name):
    p = F.edge_clouds()[name][0]
    q = np.concatenate([p[:40], p[:5] + 100.0, np.array([[-3.0, 7.0, 0.5]])], 0)          # rows of the cloud, and queries far outside its box
    for k in (1, 3, 33, 64):
        for queries in (None, q):
            tidx, td2 = twin.knn(p, k, queries)
            idx, d2 = host_knn(p, k, queries)
            assert np.array_equal(idx, tidx) and np.array_equal(d2, td2)
            assert (idx[:, min(k, len(p)):] == -1).all() and np.isinf(d2[:, min(k, len(p)):]).all()


# ---- normals ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', F.CLOUDS)
def test_host_normals_entry_meets_the_demands(name):
    tC, m, tn, w = F.twin_normals(name)
    for dtype in (np.float32, np.float64):
        n, C = host_normals(F.cloud(name).astype(dtype))
        F.assert_covariances(C, tC, m)
        F.assert_unit(n)
        K = F.assert_directions(n, tn, w, max_excluded=0.0)              # the fixture clouds exclude no row
        print('%s: largest K %.3f (bound %g)' % (name, K, F.DIRECTION_K))
        assert np.array_equal(n, twin.canonical(n))


@pytest.mark.parametrize('name', list(F.edge_clouds()))
def test_host_normals_entry_on_the_edge_cases(name):
    p, kind = F.edge_clouds()[name]
    n, C = host_normals(p)
    if len(p) == 0:
        return
    idx, _ = twin.knn(p, F.KNN)
    tC, m = twin.covariances(p, idx)
    tn, w = twin.normals_from(tC, m)
    F.assert_unit(n)
    assert np.array_equal(n, twin.canonical(n))
    if kind == 'fallback':                                               # m < 3 or C = 0: exactly (0, 0, 1)
        assert np.array_equal(n, np.tile([0.0, 0.0, 1.0], (len(p), 1)))
    elif kind == 'plane':                                                # z = 0 exactly: C's z row is zero and the normal exact
        assert np.array_equal(n, np.tile([0.0, 0.0, 1.0], (len(p), 1)))
    elif kind == 'direction':
        F.assert_covariances(C, tC, m)
        F.assert_directions(n, tn, w)
    # 'unit' (lattice: ties at the k-th place and equal eigenvalues; collinear: a two-dimensional null space): finite and unit only


def test_host_normals_entry_viewpoint():
    p = F.cloud('micro').astype(np.float64)
    view = np.array([0.3, 0.25, 0.2])
    plain, _ = host_normals(p)
    n, _ = host_normals(p, viewpoint=view)
    assert (((n * (view - p)).sum(1)) >= 0).all()
    assert np.array_equal(np.abs(n), np.abs(plain))                      # directions unchanged
    assert np.array_equal(np.sign(n), np.sign(twin.estimate_normals(p, F.KNN, view)))


# ---- the twin against the reference's results -------------------------------------------------------------------------------------------------
def test_regularize_normals_equals_the_reference():
    from se3et_amd.scan_prep import regularize_normals
    g = np.load(GOLDEN)
    p, n = g['reg/points'], g['reg/normals']
    assert -(p[0] * n[0]).sum() == 0                                      # the row with dot == 0
    for positive, key in ((True, 'reg/positive'), (False, 'reg/negative')):
        assert np.array_equal(twin.regularize_normals(p, n, positive), g[key])
        assert np.array_equal(regularize_normals(p, n, positive), g[key])
        assert np.array_equal(regularize_normals(torch.from_numpy(p), torch.from_numpy(n), positive).numpy(), g[key])
    assert np.array_equal(g['reg/positive'][0], -n[0])                    # flipped for positive=True


def test_twin_chamfer_distance_within_the_float32_bound_of_the_reference():
    g = np.load(GOLDEN)
    args = [g['mcd/' + k] for k in ('raw', 'ref', 'src', 'gt_transform', 'transform')]
    assert args[0].shape == (2, 300, 3) and args[1].shape == (2, 200, 3) and args[2].shape == (2, 180, 3)
    bound = F.chamfer_float32_bound(*args)
    none = twin.modified_chamfer_distance(*args, reduction='none')
    print('chamfer: twin', none, 'reference', g['mcd/none'], 'bound', bound)
    assert (np.abs(none - g['mcd/none']) <= bound).all()
    assert abs(twin.modified_chamfer_distance(*args, reduction='mean') - g['mcd/mean']) <= bound.mean()
    assert abs(twin.modified_chamfer_distance(*args, reduction='sum') - g['mcd/sum']) <= bound.sum()


# ---- argument validation ------------------------------------------------------------------------------------------------------------------------
def _refused(status, text):
    assert status != 0
    assert text in _lib().lib().se3_last_error().decode(), _lib().lib().se3_last_error().decode()


def test_argument_validation_of_the_voxel_entries():
    L = _lib().lib()
    buf = np.zeros((64, 3))
    words = np.zeros(8, np.int32)
    off = np.array([0, 10, 20], np.int64)
    ws = np.zeros(1 << 16, np.uint8)
    P = _ptr
    assert L.se3_voxel_downsample_workspace_bytes(1000, 4) > 0 and L.se3_voxel_downsample_workspace_bytes(1000, 33) == 0
    assert L.se3_voxel_downsample_workspace_bytes(-1, 1) == 0
    need = L.se3_voxel_downsample_workspace_bytes(20, 2)
    call = lambda **kw: L.se3_voxel_downsample_stack(*[kw.get(k, d) for k, d in (
        ('points', P(buf)), ('elem', 1), ('normals', None), ('offsets', P(off)), ('clouds', 2), ('voxel', 0.1), ('out', P(buf)), ('out_n', None),
        ('counts', P(words)), ('status', P(words[4:])), ('ws', P(ws)), ('bytes', need), ('stream', None))])
    _refused(call(points=None), 'null pointer')
    _refused(call(out=None), 'null pointer')
    _refused(call(status=None), 'null pointer')
    _refused(call(normals=P(buf)), 'null pointer')                      # normals without a place for their means
    _refused(call(clouds=33), 'at most 32')
    _refused(call(elem=2), 'elem 2')
    for v in (0.0, -1.0, float('nan'), float('inf')):
        _refused(call(voxel=v), 'not a positive finite number')
    _refused(call(offsets=P(np.array([1, 10, 20], np.int64))), 'offsets must start at 0')
    _refused(call(offsets=P(np.array([0, 10, 5], np.int64))), 'offsets must start at 0')
    _refused(call(bytes=need - 1), 'too small')
    count, status = np.zeros(1, np.int64), np.zeros(1, np.int32)
    host = lambda **kw: L.se3_debug_voxel_downsample_host(*[kw.get(k, d) for k, d in (
        ('points', P(buf)), ('n', 10), ('elem', 1), ('normals', None), ('voxel', 0.1), ('out', P(buf)), ('out_n', None), ('count', P(count)),
        ('status', P(status)))])
    _refused(host(points=None), 'null pointer')
    _refused(host(n=-1), 'n -1')
    for v in (0.0, -1.0, float('nan'), float('inf')):
        _refused(host(voxel=v), 'not a positive finite number')
    assert host() == 0 and host(n=0) == 0 and count[0] == 0


def test_argument_validation_of_the_knn_entries():
    L = _lib().lib()
    P = _ptr
    buf = np.zeros((64, 3))
    idx, d2 = np.zeros((64, 64), np.int64), np.zeros((64, 64))
    off = np.array([0, 10, 20], np.int64)
    need = L.se3_pair_grid_workspace_bytes(20, 2)
    ws = np.zeros(64, np.uint8)                                          # never read: every call below is refused before any launch
    for name, fn, tail in (('knn_stack', L.se3_knn_stack, (P(idx), P(d2))), ('knn_normals_stack', L.se3_knn_normals_stack, (None, P(buf)))):
        call = lambda fn=fn, tail=tail, **kw: fn(*([kw.get(k, d) for k, d in (
            ('ws', P(ws)), ('bytes', need), ('ns', 20), ('q', P(buf)), ('elem', 1), ('offsets', P(off)), ('clouds', 2), ('k', 33))] +
            list(kw.get('tail', tail)) + [None]))
        _refused(call(ws=None), name + ': null pointer')
        _refused(call(q=None), name + ': null pointer')
        _refused(call(tail=(tail[0], None)), name + ': null pointer')
        _refused(call(clouds=33), 'at most 32')
        _refused(call(k=0), 'k 0 not in [1, 64]')
        _refused(call(k=65), 'k 65 not in [1, 64]')
        _refused(call(offsets=P(np.array([0, 10, 5], np.int64))), 'offsets must start at 0')
        _refused(call(bytes=need - 1), 'too small')
        assert call(clouds=0, offsets=P(np.zeros(1, np.int64)), ns=0, bytes=L.se3_pair_grid_workspace_bytes(0, 0)) == 0   # zero clouds: a valid empty call
    view = np.array([[0.0, np.nan, 0.0], [0.0, 0.0, 0.0]])
    _refused(L.se3_knn_normals_stack(P(ws), need, 20, P(buf), 1, P(off), 2, 33, P(view), P(buf), None), 'non-finite viewpoint')
    _refused(L.se3_debug_knn_host(None, 4, P(buf), 10, 1, 3, P(idx), P(d2)), 'null pointer')
    _refused(L.se3_debug_knn_host(P(buf), 4, P(buf), 10, 1, 0, P(idx), P(d2)), 'k 0 not in [1, 64]')
    _refused(L.se3_debug_knn_host(P(buf), 4, P(buf), 10, 2, 3, P(idx), P(d2)), 'elem 2')
    _refused(L.se3_debug_knn_normals_host(None, 4, 1, 33, None, P(buf), None), 'null pointer')
    _refused(L.se3_debug_knn_normals_host(P(buf), 4, 1, 65, None, P(buf), None), 'k 65 not in [1, 64]')
    _refused(L.se3_debug_knn_normals_host(P(buf), 4, 1, 33, P(view), P(buf), None), 'non-finite viewpoint')
    words = np.zeros(2, np.int32)
    assert L.se3_voxel_downsample_stack(P(buf), 1, None, P(np.zeros(1, np.int64)), 0, 0.1, P(buf), None, P(words), P(words[1:]), P(ws), 1 << 20,
                                        None) == 0                       # zero clouds: a valid empty call


def test_batched_functions_refuse_cpu_tensors():
    from se3et_amd import pair_geometry as PG
    from se3et_amd import scan_prep as S
    c = torch.zeros((8, 3))
    with pytest.raises(RuntimeError, match='cloud 0 must be a GPU tensor .scan preparation has no CPU implementation'):
        S.voxel_downsample_clouds([c], 0.1)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        S.voxel_downsample_clouds([c], 0.1, [c])
    with pytest.raises(RuntimeError, match='GPU tensor'):
        S.knn_clouds([c], 3)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        S.estimate_normals_clouds([c])
    with pytest.raises(RuntimeError, match='GPU tensor'):
        PG.modified_chamfer_distance_pairs([c], [c], [c], [np.eye(4)], [np.eye(4)])
    with pytest.raises(RuntimeError, match='GPU tensor'):
        PG.modified_chamfer_distance(c[None], c[None], c[None], torch.eye(4)[None], torch.eye(4)[None])
    with pytest.raises(ValueError, match='positive finite'):
        S.voxel_downsample_clouds([c], float('nan'))
    with pytest.raises(ValueError, match='positive finite'):
        S.voxel_downsample_clouds([c], 0.0)
