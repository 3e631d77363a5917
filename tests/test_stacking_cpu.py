"""CPU: the shared plumbing of the batched pair tools (se3et_amd/stacking.py), the parts that need no device."""
import numpy as np
import pytest
import torch

from se3et_amd import ops, stacking as S
from se3et_amd._lib import CONSTANTS


def test_exclusive_offsets():
    """Plain sums as Python ints.  A negative length stays refused where it is refused today, by the wrappers that take host lengths and in
    their own exception type (ops._pair_offsets for the pair and scan wrappers): exclusive_offsets itself only adds."""
    assert S.exclusive_offsets([]) == [0]
    assert S.exclusive_offsets([0]) == [0, 0]
    assert S.exclusive_offsets([3, 0, 5]) == [0, 3, 3, 8]
    out = S.exclusive_offsets(np.array([3, 0, 5], dtype=np.int32))
    assert out == [0, 3, 3, 8] and all(type(v) is int for v in out)
    assert S.exclusive_offsets(n * m for n, m in [(2, 3), (4, 5)]) == [0, 6, 26]
    assert S.exclusive_offsets([4, -1]) == [0, 4, 3]
    with pytest.raises(RuntimeError, match='lengths that sum'):
        ops._pair_offsets([4, -1], 3, 'pair_grid_build')
    assert list(ops._pair_offsets([3, 0, 5], 8, 'pair_grid_build')) == [0, 3, 3, 8]


def test_chunks():
    limit = CONSTANTS['SE3_PAIR_MAX_PAIRS']
    assert S.PAIR_MAX_PAIRS == limit == ops.PAIR_MAX_PAIRS
    assert list(S.chunks(0)) == []
    assert list(S.chunks(1)) == [(0, 1)]
    assert list(S.chunks(limit)) == [(0, limit)]
    assert list(S.chunks(limit + 1)) == [(0, limit), (limit, limit + 1)]
    assert list(S.chunks(2 * limit + 1)) == [(0, limit), (limit, 2 * limit), (2 * limit, 2 * limit + 1)]
    assert list(S.chunks(5, 2)) == [(0, 2), (2, 4), (4, 5)]


def test_stack_joins_the_results_of_chunks():
    empty, a, b = torch.zeros((0, 2)), torch.ones((1, 2)), torch.full((2, 2), 2.0)
    assert S.stack([], empty) is empty
    assert S.stack([a], empty) is a
    assert torch.equal(S.stack([a, b], empty), torch.cat([a, b], 0))


def test_transforms_of():
    eye = np.eye(4)
    shift = torch.eye(4, dtype=torch.float32)
    shift[0, 3] = 0.5
    cases = [(eye, 1), ([eye, 2 * eye], 2), ([shift, eye, shift.double()], 3), (shift.repeat(3, 1, 1), 3), (None, 2), ([], 0)]
    for x, P in cases:
        for dtype in (torch.float64, torch.float32):
            t = S.transforms_of(x, P, 'caller', 'cpu', dtype)
            assert tuple(t.shape) == (P, 4, 4) and t.dtype == dtype and t.device.type == 'cpu' and t.is_contiguous()
    assert torch.equal(S.transforms_of([shift, eye, shift.double()], 3, 'caller', 'cpu')[2], shift.double())
    assert torch.equal(S.transforms_of(None, 2, 'caller', 'cpu'), S.identities(2))
    assert S.identities(3).dtype == torch.float64 and torch.equal(S.identities(3)[2], torch.eye(4, dtype=torch.float64))
    for x in (eye, [eye, eye, eye], shift.repeat(3, 1, 1)):
        with pytest.raises(ValueError, match='caller: one .4, 4. transform per pair'):
            S.transforms_of(x, 2, 'caller', 'cpu')
    with pytest.raises(RuntimeError, match='caller'):                      # the benchmark metrics keep their RuntimeError
        S.transforms_of(eye, 2, 'caller', 'cpu', error=RuntimeError)
    bad = np.eye(4)
    bad[1, 2] = np.nan
    assert torch.isnan(S.transforms_of([eye, bad], 2, 'caller', 'cpu')[1, 1, 2])     # not asked for: passed on (ICP's kernel refuses it)
    for x in ([eye, bad], torch.from_numpy(np.stack([eye, bad])), [eye, np.full((4, 4), np.inf)]):
        with pytest.raises(ValueError, match='caller: a transform is not finite'):
            S.transforms_of(x, 2, 'caller', 'cpu', finite=True)


def test_stack():
    a, b, c = torch.zeros((2, 3)), torch.ones((3, 3)), torch.full((1, 3), 2.0, dtype=torch.float64)
    assert S.stack([a]) is a and S.stack([c]) is c
    ab, abc = S.stack([a, b]), S.stack([a, c, b])
    assert ab.dtype == torch.float32 and torch.equal(ab, torch.cat([a, b], 0))
    assert abc.dtype == torch.float64 and torch.equal(abc, torch.cat([a.double(), c, b.double()], 0))
    assert S.stack([c, c]).dtype == torch.float64
    i = torch.arange(3)
    assert S.stack([i, i]).dtype == torch.int64
    assert S.lengths([a, c, b]) == [2, 1, 3]
    empty = torch.zeros((0, 3))
    assert S.stack([], empty) is empty
    with pytest.raises(ValueError):
        S.stack([])


def test_strict_check_names_its_caller():
    dev = torch.device('cuda')
    with pytest.raises(RuntimeError, match=r'icp_pairs: source cloud 0 must be a GPU tensor \(ICP has no CPU implementation\)'):
        S.gpu_rows(torch.zeros((4, 3)), dev, 'icp_pairs: source cloud 0', 'ICP')
    with pytest.raises(RuntimeError, match='knn_clouds: cloud 2 must be a GPU tensor'):          # (an (n, 4) tensor on the host is refused for
        S.gpu_rows(torch.zeros((4, 4)), dev, 'knn_clouds: cloud 2', 'scan preparation')         # where it is first: the shape is a GPU test)
    with pytest.raises(RuntimeError, match='knn_clouds: cloud 0 must be a GPU tensor'):
        S.gpu_rows_each([torch.zeros((4, 3))], dev, 'knn_clouds: cloud', 'scan preparation')
    with pytest.raises(RuntimeError, match='knn_clouds: cloud 2 must be a tensor'):
        S.gpu_rows(np.zeros((4, 3)), dev, 'knn_clouds: cloud 2', 'scan preparation')
    from se3et_amd import icp
    with pytest.raises(RuntimeError, match='icp_pairs: source cloud 0 .*ICP has no CPU'):
        icp.icp_pairs([torch.zeros((4, 3))], [torch.zeros((4, 3))], np.eye(4)[None], 0.1)


def test_device_of_and_the_permissive_converter():
    assert S.device_of('cpu', [torch.zeros(1)]) == torch.device('cpu')
    assert S.device_of(None, [np.zeros(3)], [torch.zeros(1)]) == torch.device('cuda')
    assert S.device_of('cuda:1', [torch.zeros(1)]) == torch.device('cuda:1')
    for x in ([[1, 2, 3], [4, 5, 6]], np.arange(6.0), torch.arange(6).reshape(3, 2)):
        t = S.as_rows(x, 'cpu')
        assert tuple(t.shape) == (2, 3) and t.dtype == torch.float32 and t.is_contiguous()
    assert tuple(S.as_rows([], 'cpu', 2, torch.int64).shape) == (0, 2)
    flat = S.as_rows([[1, 2], [3, 4]], 'cpu', None, torch.int64)
    assert flat.tolist() == [1, 2, 3, 4] and flat.dtype == torch.int64


def test_upload_dtypes():
    assert S.upload(np.zeros((2, 3), np.float32), 'cpu').dtype == torch.float32
    assert S.upload(np.zeros((2, 3), np.float16), 'cpu').dtype == torch.float64
    assert S.upload([[0, 1, 2]], 'cpu').dtype == torch.float64
    f = S.upload(np.zeros((2, 5)), 'cpu', None, np.float32)
    assert f.dtype == torch.float32 and tuple(f.shape) == (2, 5)
    assert tuple(S.upload(np.zeros(10), 'cpu', 5, np.float32).shape) == (2, 5)
