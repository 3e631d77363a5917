"""CPU: feature-space matching (se3et_amd/feature_matching.py, csrc/feature_nn.hip) and the RANSAC checkers without a GPU.

  - the numpy twin (tests/feature_matching_twin.py) against the reference's own lists in tests/golden/feature_matching.npz;
  - the torch form of the twin against the numpy form, as sets;
  - the twin on hand-made matrices (ties, NaN rows, an empty cloud, duplicate bilateral pairs) and the checker twin on hand-made samples;
  - argument validation of the new C entries, and the alias of the torch-named mirror without a reference tree."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feature_matching_twin as twin

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ('c256', 'c32')


def golden():
    return np.load(os.path.join(HERE, 'golden', 'feature_matching.npz'))


@pytest.mark.parametrize('name', CASES)
def test_twin_matches_the_reference(name):
    g = golden()
    ref, src = g[name + '/ref_feats'], g[name + '/src_feats']
    assert ref.dtype == np.float32 and ref.shape[0] == 400 and src.shape[0] == 350
    nn_src, _, near_a, _ = twin.near_ties(ref, src)
    nn_ref, _, near_b, _ = twin.near_ties(src, ref)
    assert not near_a.any() and not near_b.any()                   # the fixture does not depend on a tie rule
    for key, mode in (('one_way', 'one_way'), ('mutual', 'mutual'), ('bilateral', 'bilateral_concat')):
        i, j = twin.extract(nn_src, nn_ref, mode)
        assert np.array_equal(i, g[name + '/' + key + '_ref']) and np.array_equal(j, g[name + '/' + key + '_src']), (name, key)
    assert 150 < len(g[name + '/mutual_ref']) < 350


@pytest.mark.parametrize('name', CASES)
def test_torch_form_equals_the_numpy_form_as_sets(name):
    g = golden()
    ref, src = g[name + '/ref_feats'], g[name + '/src_feats']
    d2 = twin.sq_distances(ref, src)
    nn_src, nn_ref = twin.nearest_from_matrix(d2)[0], twin.nearest_from_matrix(d2.T)[0]
    for mutual in (False, True):
        ti, tj = twin.extract_torch_form(d2, mutual=mutual)
        ni, nj = twin.extract(nn_src, nn_ref, 'mutual' if mutual else 'one_way')
        assert set(zip(ti.tolist(), tj.tolist())) == set(zip(ni.tolist(), nj.tolist()))
        assert np.array_equal(ti, ni) and np.array_equal(tj, nj)      # both are ascending in the ref index
    # bilateral: the mask form is the de-duplicated, row-major form of the concatenated one
    bi, bj = twin.extract_torch_form(d2, bilateral=True)
    mi, mj = twin.extract(nn_src, nn_ref, 'bilateral_mask')
    ci, cj = twin.extract(nn_src, nn_ref, 'bilateral_concat')
    assert np.array_equal(bi, mi) and np.array_equal(bj, mj)
    assert sorted(set(zip(ci.tolist(), cj.tolist()))) == list(zip(mi.tolist(), mj.tolist()))


def test_twin_on_hand_made_matrices():
    inf, nan = np.inf, np.nan
    # ties go to the lowest index; a NaN candidate is never chosen; a row without a finite candidate gets -1 / inf
    d2 = np.array([[3.0, 1.0, 1.0, 2.0],
                   [nan, 5.0, 4.0, 4.0],
                   [nan, nan, inf, nan],
                   [0.0, 0.0, 0.0, 0.0]])
    idx, best = twin.nearest_from_matrix(d2)
    assert idx.tolist() == [1, 2, -1, 0] and best.tolist() == [1.0, 4.0, inf, 0.0]
    # an empty other cloud
    idx, best = twin.nearest_from_matrix(np.zeros((3, 0)))
    assert idx.tolist() == [-1, -1, -1] and np.all(np.isinf(best))
    idx, best = twin.nearest_from_matrix(np.zeros((0, 3)))
    assert idx.shape == (0,) and best.shape == (0,)
    # duplicated feature rows: exact ties in feature space
    x = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0]], np.float32)
    y = np.array([[0.0, 1.0], [1.0, 0.0], [1.0, 0.0], [0.0, 1.0]], np.float32)
    assert twin.nearest(x, y)[0].tolist() == [1, 0, 1] and twin.nearest(y, x)[0].tolist() == [1, 0, 0, 1]
    idx, best, near, allowed = twin.near_ties(x, y)
    assert near.all() and allowed.tolist() == [[False, True, True, False], [True, False, False, True], [False, True, True, False]]
    # NaN feature rows
    xn = np.array([[nan, 0.0], [0.0, 1.0]], np.float32)
    assert twin.nearest(xn, y)[0].tolist() == [-1, 0] and twin.nearest(y, xn)[0].tolist() == [1, 1, 1, 1]
    # extraction: rows with -1 produce nothing; duplicates of the bilateral mask form appear once, in row-major order
    nn_src = np.array([2, -1, 0, 2])             # ref row -> src row
    nn_ref = np.array([2, 3, 0, -1, 3])          # src row -> ref row
    assert [a.tolist() for a in twin.extract(nn_src, nn_ref, 'one_way')] == [[0, 2, 3], [2, 0, 2]]
    assert [a.tolist() for a in twin.extract(nn_src, nn_ref, 'mutual')] == [[0, 2], [2, 0]]
    assert [a.tolist() for a in twin.extract(nn_src, nn_ref, 'bilateral_concat')] == [[0, 2, 3, 2, 3, 0, 3], [2, 0, 2, 0, 1, 2, 4]]
    assert [a.tolist() for a in twin.extract(nn_src, nn_ref, 'bilateral_mask')] == [[0, 2, 3, 3, 3], [2, 0, 1, 2, 4]]
    assert [a.tolist() for a in twin.extract(np.zeros(0, np.int64), np.zeros(0, np.int64), 'bilateral_mask')] == [[], []]
    assert [a.tolist() for a in twin.extract(np.full(3, -1), np.zeros(0, np.int64), 'bilateral_concat')] == [[], []]


def test_tolerance_is_the_issue_formula():
    x, y = np.full((2, 24), 0.5, np.float32), np.full((3, 24), 0.25, np.float32)
    tr, tc = twin.tolerance(x, y)
    assert np.allclose(tr + tc[0], (24 + 8) * 2.0 ** -22 * (24 * 0.25 + 24 * 0.0625), rtol=1e-15)


def test_checker_twin_on_hand_made_samples():
    # one hypothesis of three correspondences; src is a 3-4-5 triangle
    S = np.array([[[0.0, 0, 0], [3.0, 0, 0], [0.0, 4, 0]]])
    ok, border = twin.edge_length_ok(S, S.copy(), 0.9)
    assert ok[0] and not border[0]
    ok, _ = twin.edge_length_ok(S, 0.95 * S, 0.9)                  # every ref edge 0.95 of the src edge: similar enough
    assert ok[0]
    ok, _ = twin.edge_length_ok(S, 0.85 * S, 0.9)                  # ref edges too short
    assert not ok[0]
    ok, _ = twin.edge_length_ok(0.85 * S, S, 0.9)                  # ... and the other way round
    assert not ok[0]
    R = S.copy()
    R[0, 2] = [0.0, 4.0 * 0.5, 0]                                  # one edge halved
    assert not twin.edge_length_ok(S, R, 0.9)[0][0]
    # exactly at the limit: the comparison is strict, and the hypothesis is flagged borderline
    S2 = np.array([[[0.0, 0, 0], [1.0, 0, 0], [0.0, 0, 0]]])
    R2 = np.array([[[0.0, 0, 0], [0.5, 0, 0], [0.0, 0, 0]]])
    ok, border = twin.edge_length_ok(S2, R2, 0.5)
    assert ok[0] and border[0]
    # a sample drawn twice (zero edges) passes, as in Open3D
    assert twin.edge_length_ok(np.zeros((1, 3, 3)), np.zeros((1, 3, 3)), 0.9)[0][0]
    # distance checker: identity fit, one sample 0.06 away at a threshold of 0.05
    Rm, tv = np.eye(3)[None], np.zeros((1, 3))
    far = S.copy()
    far[0, 1, 2] = 0.06
    assert twin.distance_ok(Rm, tv, S, S, 0.05)[0][0] and not twin.distance_ok(Rm, tv, S, far, 0.05)[0][0]
    # checked_run: a rejected hypothesis has count 0 and cannot win
    rng = np.random.default_rng(5)
    import ransac_twin
    src, ref, _T = ransac_twin.synthetic_pair(rng, 200, 0.5)
    hyp = rng.integers(0, 200, (64, 3))
    plain = ransac_twin.run(src, ref, 0.05, 3, hyp)
    both = twin.checked_run(src, ref, 0.05, 3, hyp, edge_t=0.9, check_distance=True)
    assert both['passed'].sum() < 64 and np.all(both['counts'][~both['passed']] == 0)
    assert np.array_equal(both['counts'][both['passed']], plain['counts'][both['passed']])
    assert both['best'] == -1 or both['passed'][both['best']]
    off = twin.checked_run(src, ref, 0.05, 3, hyp)
    assert off['best'] == plain['best'] and np.array_equal(off['counts'], plain['counts'])


def test_argument_validation_without_gpu():
    from se3et_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(256)          # a non-null "device" pointer: every call below must be refused before any launch

    def refused(status, word):
        assert status != 0 and word in L.se3_last_error(), L.se3_last_error()

    need = L.se3_feature_nn_workspace_bytes(5000, 4500)
    assert need > 0 and L.se3_feature_nn_workspace_bytes(-1, 4) == 0
    assert need < 64 * (5000 + 4500) * 4 + 4096                    # O(N + M)
    assert L.se3_feature_nn_workspace_bytes(20000, 20000) < 16 << 20
    nn = (fake, fake, fake, fake)
    refused(L.se3_feature_nn_stack(fake, fake, fake, fake, 1, 8, 8, 0, fake, need, *nn, None), b'channels')
    refused(L.se3_feature_nn_stack(fake, fake, fake, fake, -1, 8, 8, 4, fake, need, *nn, None), b'pairs')
    refused(L.se3_feature_nn_stack(fake, fake, fake, fake, 1, -8, 8, 4, fake, need, *nn, None), b'ref rows')
    refused(L.se3_feature_nn_stack(fake, fake, fake, fake, 0, 8, 8, 4, fake, need, *nn, None), b'rows without pairs')
    refused(L.se3_feature_nn_stack(None, fake, fake, fake, 1, 8, 8, 4, fake, need, *nn, None), b'null')
    refused(L.se3_feature_nn_stack(fake, fake, None, fake, 1, 8, 8, 4, fake, need, *nn, None), b'null')
    refused(L.se3_feature_nn_stack(fake, fake, fake, fake, 1, 8, 8, 4, fake, need, fake, None, fake, fake, None), b'null')
    refused(L.se3_feature_nn_stack(fake, fake, fake, fake, 1, 8, 8, 4, fake, 16, *nn, None), b'workspace')
    refused(L.se3_feature_nn_stack(fake, fake, fake, fake, 1, 8, 8, 4, None, need, *nn, None), b'workspace')
    assert L.se3_feature_nn_stack(None, None, fake, fake, 0, 0, 0, 4, None, 0, None, None, None, None, None) == 0   # an empty call
    refused(L.se3_feature_corr_count_stack(fake, fake, fake, fake, 1, 8, 8, 4, fake, None), b'mode')
    refused(L.se3_feature_corr_count_stack(fake, fake, fake, fake, 1, 8, 8, -1, fake, None), b'mode')
    refused(L.se3_feature_corr_count_stack(None, fake, fake, fake, 1, 8, 8, 0, fake, None), b'null')
    refused(L.se3_feature_corr_count_stack(fake, fake, fake, fake, 1, 8, 8, 0, None, None), b'null')
    refused(L.se3_feature_corr_count_stack(fake, fake, fake, fake, -2, 8, 8, 0, fake, None), b'pairs')
    refused(L.se3_feature_corr_fill_stack(fake, fake, fake, fake, 1, 8, 8, 1, fake, -1, fake, fake, None), b'total')
    refused(L.se3_feature_corr_fill_stack(fake, fake, fake, fake, 1, 8, 8, 1, fake, 4, None, fake, None), b'null')
    refused(L.se3_feature_corr_fill_stack(fake, fake, fake, fake, 1, 8, 8, 7, fake, 4, fake, fake, None), b'mode')
    assert L.se3_feature_corr_fill_stack(fake, fake, fake, fake, 1, 8, 8, 1, fake, 0, None, None, None) == 0         # nothing to fill
    # the checked RANSAC entry validates like the unchecked one, plus its own argument
    ws = L.se3_ransac_correspondences_workspace_bytes(1, 64)
    out = (fake, fake, fake, fake, None, None, None)
    refused(L.se3_ransac_correspondences_checked_stack(fake, fake, fake, 1, 0.05, 3, 64, 0, None, 1.5, 1, fake, ws, *out, None), b'edge_length')
    refused(L.se3_ransac_correspondences_checked_stack(fake, fake, fake, 1, 0.05, 3, 64, 0, None, float('nan'), 1, fake, ws, *out, None),
            b'edge_length')
    refused(L.se3_ransac_correspondences_checked_stack(None, fake, fake, 1, 0.05, 3, 64, 0, None, 0.9, 1, fake, ws, *out, None), b'null')
    refused(L.se3_ransac_correspondences_checked_stack(fake, fake, fake, 1, 0.05, 17, 64, 0, None, 0.9, 1, fake, ws, *out, None), b'ransac_n')
    refused(L.se3_ransac_correspondences_checked_stack(fake, fake, fake, 1, 0.05, 3, 64, 0, None, 0.9, 1, fake, ws - 1, *out, None),
            b'workspace')
    assert L.se3_ransac_correspondences_checked_stack(fake, fake, fake, 0, 0.05, 3, 64, 0, None, 0.9, 1, None, 0, *out, None) == 0


def test_product_refuses_cpu_and_float64_tensors():
    from se3et_amd import feature_matching as FM
    from se3et_amd.modules.registration import extract_correspondences_from_feats
    a, b = torch.zeros(8, 4), torch.ones(9, 4)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        FM.nearest_feature_pairs([a], [b])
    with pytest.raises(RuntimeError, match='GPU tensor'):
        FM.extract_correspondences_from_feats_pairs([a], [b], mutual=True)
    with pytest.raises(RuntimeError):
        FM.nearest_feature_pairs([a.numpy()], [b.numpy()])
    with pytest.raises(RuntimeError, match='GPU tensor'):
        extract_correspondences_from_feats(a, b)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        extract_correspondences_from_feats(a.double(), b.double())
    with pytest.raises(ValueError):
        FM.nearest_feature_pairs([a], [b, b])


def test_alias_resolves_without_a_reference_tree():
    """geotransformer.modules.registration.extract_correspondences_from_feats is this package's function once the aliases are installed,
    on a machine without the reference."""
    code = '''
import sys
import se3et_amd.dropin as d
sys.path = [p for p in sys.path if "reference" not in p]
d.install_aliases()
from geotransformer.modules.registration import extract_correspondences_from_feats
from geotransformer.modules.registration.matching import extract_correspondences_from_feats as again
import se3et_amd.modules.registration.matching as own
assert extract_correspondences_from_feats is own.extract_correspondences_from_feats is again
assert extract_correspondences_from_feats.__module__ == "se3et_amd.modules.registration.matching"
print("ok")
'''
    env = dict(os.environ, SE3_BLOCKING_SYNC='0', PYTHONPATH=os.path.dirname(HERE))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, timeout=600, cwd='/tmp')
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stderr[-3000:]
