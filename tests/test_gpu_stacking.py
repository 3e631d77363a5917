"""GPU: the chunked pair calls across a chunk boundary (se3et_amd/stacking.py: chunks, stack, the joins of the chunks' results), and the
calls that accept zero pairs.  PAIR_MAX_PAIRS + 1 pairs of 16 random points, float32 with every third pair float64 so that a chunk's stack
is promoted: the batched call must equal the same pairs called one at a time in every bit of every output (the kernels' contract: a pair's
result does not depend on its place in a batch or on the dtype its chunk is stacked in)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pairs():
    from se3et_amd.ops import PAIR_MAX_PAIRS
    rng = np.random.default_rng(11)
    P = PAIR_MAX_PAIRS + 1
    refs, srcs, Ts = [], [], []
    for p in range(P):
        dtype = np.float64 if p % 3 == 2 else np.float32
        ref = rng.uniform(-1, 1, (16, 3))
        a = rng.uniform(-0.05, 0.05)
        T = np.eye(4)
        T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        T[:3, 3] = rng.uniform(-0.02, 0.02, 3)
        src = (ref + rng.normal(0, 0.01, ref.shape) - T[:3, 3]) @ T[:3, :3]          # ref ~ T src
        refs.append(torch.from_numpy(ref.astype(dtype)).cuda())
        srcs.append(torch.from_numpy(src.astype(dtype)).cuda())
        Ts.append(T)
    return refs, srcs, torch.from_numpy(np.stack(Ts))


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def test_nearest_neighbor_pairs_across_a_chunk_boundary(pairs):
    from se3et_amd.pair_geometry import nearest_neighbor_pairs
    refs, srcs, Ts = pairs
    d, i = nearest_neighbor_pairs(refs, srcs, Ts, return_index=True)
    assert len(d) == len(i) == len(refs)
    for p in range(len(refs)):
        d1, i1 = nearest_neighbor_pairs(refs[p:p + 1], srcs[p:p + 1], Ts[p:p + 1], return_index=True)
        _same(d[p], d1[0])
        _same(i[p], i1[0])
    assert d[0].dtype == torch.float64 and i[0].dtype == torch.int64 and bool(torch.isfinite(torch.cat(d)).all())


def test_get_correspondences_pairs_across_a_chunk_boundary(pairs):
    from se3et_amd.pair_geometry import get_correspondences_pairs
    refs, srcs, Ts = pairs
    got = get_correspondences_pairs(refs, srcs, Ts, 0.3)
    assert len(got) == len(refs) and sum(int(c.shape[0]) for c in got) >= 16 * len(refs)
    for p in range(len(refs)):
        _same(got[p], get_correspondences_pairs(refs[p:p + 1], srcs[p:p + 1], Ts[p:p + 1], 0.3)[0])


def test_knn_clouds_across_a_chunk_boundary(pairs):
    from se3et_amd.scan_prep import knn_clouds
    refs, srcs, _ = pairs
    for queries in (None, srcs):
        idx, d2 = knn_clouds(refs, 5, queries)
        assert len(idx) == len(d2) == len(refs)
        for p in range(len(refs)):
            i1, d1 = knn_clouds(refs[p:p + 1], 5, None if queries is None else queries[p:p + 1])
            _same(idx[p], i1[0])
            _same(d2[p], d1[0])
        assert tuple(idx[0].shape) == (16, 5) and int(torch.cat(idx).min()) >= 0


def test_icp_pairs_across_a_chunk_boundary(pairs):
    from se3et_amd.icp import icp_pairs
    refs, srcs, _ = pairs
    T0 = torch.eye(4, dtype=torch.float64, device='cuda').repeat(len(refs), 1, 1)
    out = icp_pairs(srcs, refs, T0, 0.5, return_correspondences=True)
    assert len(out['correspondences']) == len(refs) and int(out['iterations'].min()) >= 1 and bool(torch.isfinite(out['transforms']).all())
    for p in range(len(refs)):
        one = icp_pairs(srcs[p:p + 1], refs[p:p + 1], T0[p:p + 1], 0.5, return_correspondences=True)
        for k in ('transforms', 'fitness', 'inlier_rmse', 'iterations', 'converged', 'status'):
            _same(out[k][p:p + 1], one[k])
        _same(out['correspondences'][p], one['correspondences'][0])


def test_strict_check_refuses_a_wrong_shape_dtype_or_device():
    from se3et_amd import stacking as S
    from se3et_amd.icp import icp_pairs
    from se3et_amd.scan_prep import knn_clouds
    dev = torch.device('cuda')
    good = torch.zeros((4, 3), device='cuda')
    turned = torch.zeros((3, 4), dtype=torch.float64, device='cuda').T
    assert S.gpu_rows(good, dev, 'x', 'y') is good and not turned.is_contiguous() and S.gpu_rows(turned, dev, 'x', 'y').is_contiguous()
    for bad in (torch.zeros((4, 4), device='cuda'), torch.zeros((4, 3), dtype=torch.float16, device='cuda'), torch.zeros((12,), device='cuda'),
                torch.zeros((4, 3), dtype=torch.int64, device='cuda')):
        with pytest.raises(RuntimeError, match=r'knn_clouds: cloud 1 must be \(n, 3\) float32 or float64 on cuda:0, got'):
            knn_clouds([good, bad], 3)
        with pytest.raises(RuntimeError, match=r'icp_pairs: reference cloud 0 must be \(n, 3\) float32 or float64'):
            icp_pairs([good], [bad], np.eye(4)[None], 0.1)
    with pytest.raises(RuntimeError, match=r'x 0 must be \(n, 3\) float32 or float64 on cuda:7, got \(4, 3\) torch.float32 on cuda:0'):
        S.gpu_rows_each([good], torch.device('cuda:7'), 'x', 'y')
    with pytest.raises(RuntimeError, match=r'f 0 must be \(n, C\) float32 on the GPU, got'):
        S.gpu_rows_each([good.double()], None, 'f', 'y', cols=None, dtypes=(torch.float32,))


def test_calls_without_pairs_return_their_empty_shapes():
    from se3et_amd.icp import icp_pairs
    from se3et_amd.pair_geometry import compute_overlap_pairs
    from se3et_amd.ransac import ransac_pairs
    f32, f64, i32 = torch.float32, torch.float64, torch.int32

    def check(out, want):
        assert set(out) == set(want)
        for k, (shape, dtype) in want.items():
            assert tuple(out[k].shape) == shape and out[k].dtype == dtype and out[k].is_cuda, k

    out = icp_pairs([], [], np.zeros((0, 4, 4)), 0.1, return_correspondences=True)
    assert out.pop('correspondences') == []
    check(out, dict(transforms=((0, 4, 4), f64), fitness=((0,), f64), inlier_rmse=((0,), f64), iterations=((0,), i32),
                    converged=((0,), i32), status=((0,), i32)))
    ov = compute_overlap_pairs([], [], None, 0.1)
    assert tuple(ov.shape) == (0,) and ov.dtype == f64 and ov.is_cuda
    check(ransac_pairs([], [], 0.05, 3, 64), dict(transforms=((0, 4, 4), f32), fitness=((0,), f32), inlier_rmse=((0,), f32),
                                                  best_hypothesis=((0,), i32)))
