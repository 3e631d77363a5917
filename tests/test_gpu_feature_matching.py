"""GPU: feature-space matching (se3et_amd/feature_matching.py, csrc/feature_nn.hip) and RANSAC from features (se3et_amd/ransac.py) against
the float64 twin (tests/feature_matching_twin.py) and the reference's lists in tests/golden/feature_matching.npz.

Allowance (feature_matching_twin.py): tol(i, j) = (C + 8) 2^-22 (|x_i|^2 + |y_j|^2).  A row whose float64 winner j0 has a rival j with
d2(i, j) - d2(i, j0) < tol(i, j) + tol(i, j0) is a near-tie row: there the device may return any candidate inside the bound, everywhere
else it must return j0.  Every input is checked to have at most 2 % near-tie rows per direction BEFORE the device output is looked at.
Returned squared distances: within 1e-5 relative plus tol of the twin's direct-difference value for the returned index."""
import os

import numpy as np
import pytest
import torch

import feature_matching_twin as twin
import ransac_twin as RT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CAP = 0.02


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_nn(refs, srcs):
    from se3et_amd.feature_matching import nearest_feature_pairs
    out = nearest_feature_pairs([_gpu(r) for r in refs], [_gpu(s) for s in srcs])
    torch.cuda.synchronize()
    return [[t.cpu().numpy() for t in lst] for lst in out]


def _check_direction(x, y, idx, dist, what, fast=True):
    """x queries, y keys; idx / dist the device's answer.  The twin's near-tie share is asserted first."""
    t_idx, t_best, near, allowed = twin.near_ties(x, y, fast=fast)
    share = float(near.mean()) if len(x) else 0.0
    print('%s: %d x %d, C = %d, near-tie rows %.2f %%' % (what, len(x), len(y), x.shape[1], 100 * share))
    assert share <= CAP, '%s: the input has %.2f %% near-tie rows' % (what, 100 * share)
    assert idx.dtype == np.int64 and dist.dtype == np.float32 and idx.shape == (len(x),) and dist.shape == (len(x),)
    clear = ~near
    assert np.array_equal(idx[clear], t_idx[clear]), (what, np.flatnonzero(idx != t_idx)[:5])
    rows = np.flatnonzero(near)
    assert np.all(idx[rows] >= 0) and np.all(allowed[rows, idx[rows]]), what
    # distances of the returned winners
    want = twin.direct_sq_distance(x, y, idx)
    ok = idx >= 0
    assert np.all(np.isinf(dist[~ok]) & (dist[~ok] > 0))
    tr, tc = twin.tolerance(x, y)
    bound = 1e-5 * want[ok] + tr[ok] + tc[idx[ok]]
    err = np.abs(dist[ok].astype(np.float64) - want[ok])
    assert np.all(err <= bound), (what, float((err - bound).max()))
    return t_idx, near


def _check_pair(ref, src, got, p, what, fast=True):
    nn_src, d_src, nn_ref, d_ref = (got[k][p] for k in range(4))
    _check_direction(ref, src, nn_src, d_src, what + ' ref->src', fast)
    _check_direction(src, ref, nn_ref, d_ref, what + ' src->ref', fast)


def _micro_feats():
    g = np.load(os.path.join(HERE, 'golden', 'micro_se3ete.npz'))
    f = g['out/feats_f'].astype(np.float32)
    assert f.shape == (845, 32)
    return f[:420], f[420:]


def _families():
    rng = np.random.default_rng(7)
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    yield 'planted C=256', twin.planted_features(rng, 5000, 4500, 256, 2500)
    yield 'planted C=32', twin.planted_features(rng, 5000, 4500, 32, 2500)
    yield 'planted C=3', twin.planted_features(rng, 5000, 4500, 3, 2500)
    yield 'planted rescaled', twin.planted_features(rng, 5000, 4500, 256, 2500, scale=True)
    yield 'random unit C=256', (unit(rng.normal(size=(4000, 256))), unit(rng.normal(size=(4000, 256))))
    yield 'gaussian C=37', (rng.normal(size=(3000, 37)).astype(np.float32), rng.normal(size=(2500, 37)).astype(np.float32))
    yield 'micro feats_f', _micro_feats()


@pytest.mark.parametrize('family', range(7))
def test_nearest_neighbour_families(family):
    name, (ref, src) = list(_families())[family]
    got = _device_nn([ref], [src])
    _check_pair(ref, src, got, 0, name)


@pytest.mark.parametrize('C', [1, 3, 32, 37, 256])
def test_shapes_and_batches(C):
    """Channel counts, sizes off the tile, one row, empty clouds, 1 / 3 / 16 pairs of unequal sizes."""
    rng = np.random.default_rng(100 + C)
    sizes = [(1, 70), (70, 1), (129, 65), (64, 128), (0, 50), (50, 0), (0, 0), (333, 257), (1, 1), (200, 190), (127, 63), (65, 300),
             (31, 33), (500, 450), (90, 90), (257, 129)]
    assert len(sizes) == 16
    if C == 1:                  # (on a line the allowance grows with the square of the extent: above ~350 lattice points it reaches the gap)
        sizes = [(min(n, 340), min(m, 340)) for n, m in sizes]

    def line(n, m):
        """C = 1: the ranking value cancels badly on a line, so each cloud sits near distinct points of a unit lattice (offsets below
        0.05 and 0.3: two candidates differ by about 0.4 in d^2 or more, above the allowance at these sizes)."""
        k = max(n, m)
        pick = lambda count: (rng.permutation(k)[:count] - (k - 1) / 2)[:, None]
        return ((pick(n) + rng.uniform(-0.05, 0.05, (n, 1))).astype(np.float32),
                (pick(m) + rng.uniform(-0.3, 0.3, (m, 1))).astype(np.float32))

    def make(n, m):
        if C == 1:
            return line(n, m)
        if C <= 3 or not min(n, m):
            return rng.normal(size=(n, C)).astype(np.float32), rng.normal(size=(m, C)).astype(np.float32)
        return twin.planted_features(rng, n, m, C, min(n, m) // 2)

    pairs = [make(n, m) for n, m in sizes]
    for count in (1, 3, 16):
        sub = pairs[7:8] if count == 1 else pairs[:count]
        got = _device_nn([p[0] for p in sub], [p[1] for p in sub])
        for p, (ref, src) in enumerate(sub):
            _check_pair(ref, src, got, p, 'C=%d batch %d pair %d' % (C, count, p), fast=False)
            if len(src) == 0:
                assert np.all(got[0][p] == -1) and np.all(np.isinf(got[1][p]))
            if len(ref) == 0:
                assert np.all(got[2][p] == -1) and np.all(np.isinf(got[3][p]))


def test_large_pair_allocates_no_matrix():
    """20k x 20k, C = 32: the search must not allocate anything of size N M (1.6 GB); its growth stays below 64 MB."""
    rng = np.random.default_rng(9)
    ref, src = twin.planted_features(rng, 20000, 20000, 32, 10000)
    from se3et_amd.feature_matching import extract_correspondences_from_feats_pairs, nearest_feature_pairs
    r, s = _gpu(ref), _gpu(src)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    nn_src, d_src, nn_ref, d_ref = nearest_feature_pairs([r], [s])
    ci, cj = extract_correspondences_from_feats_pairs([r], [s], mutual=True)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print('20k x 20k: peak growth %.1f MB' % (growth / 2 ** 20))
    assert growth < 64 << 20
    # a sample of rows against the twin (the whole matrix is too large for the host check)
    rows = rng.permutation(20000)[:1500]
    for x, y, idx, dist, what in ((ref, src, nn_src[0], d_src[0], 'ref->src'), (src, ref, nn_ref[0], d_ref[0], 'src->ref')):
        _check_direction(x[rows], y, idx.cpu().numpy()[rows], dist.cpu().numpy()[rows], '20k ' + what)
    a, b = nn_src[0].cpu().numpy(), nn_ref[0].cpu().numpy()
    ti, tj = twin.extract(a, b, 'mutual')
    assert np.array_equal(ci[0].cpu().numpy(), ti) and np.array_equal(cj[0].cpu().numpy(), tj) and len(ti) > 5000


def test_duplicated_rows_go_to_the_lowest_index():
    rng = np.random.default_rng(11)
    base = rng.normal(size=(300, 64)).astype(np.float32)
    src = np.concatenate([base, base[::-1], base[:150]], 0)          # every key row two or three times
    ref = base[rng.permutation(300)]
    ref = np.concatenate([ref, ref[:77]], 0)
    got = _device_nn([ref], [src])
    d2 = twin.sq_distances(ref, src)
    assert np.array_equal(got[0][0], twin.nearest_from_matrix(d2)[0])
    assert np.array_equal(got[2][0], twin.nearest_from_matrix(d2.T)[0])
    assert np.all(got[1][0] == 0) and np.all(got[3][0] == 0)
    assert np.all(got[0][0] < 300)                                   # the first of the copies
    # the same inside a batch, after another pair
    other = twin.planted_features(rng, 100, 90, 64, 40)
    both = _device_nn([other[0], ref], [other[1], src])
    for k in range(4):
        assert np.array_equal(both[k][1], got[k][0])


def test_non_finite_rows():
    rng = np.random.default_rng(12)
    ref, src = twin.planted_features(rng, 200, 180, 32, 90)
    ref[5] = np.nan
    ref[6, 3] = np.inf
    src[7, 0] = np.nan
    src[8] = -np.inf
    src[9, 1] = 3e38                                                # finite, but its squared norm is not
    got = _device_nn([ref, ref[5:7]], [src, src])
    nn_src, d_src, nn_ref, d_ref = (got[k][0] for k in range(4))
    assert nn_src[5] == -1 and nn_src[6] == -1 and np.isinf(d_src[5]) and np.isinf(d_src[6])
    assert nn_ref[7] == -1 and nn_ref[8] == -1 and nn_ref[9] == -1
    assert not np.isin(nn_src, [7, 8, 9]).any() and not np.isin(nn_ref, [5, 6]).any()
    clean_r, clean_s = np.delete(np.arange(200), [5, 6]), np.delete(np.arange(180), [7, 8, 9])
    t = twin.nearest(ref[clean_r], src[clean_s])[0]
    assert np.array_equal(nn_src[clean_r], clean_s[t])
    t = twin.nearest(src[clean_s], ref[clean_r])[0]
    assert np.array_equal(nn_ref[clean_s], clean_r[t])
    # a pair whose every ref row is non-finite: no candidate in either direction
    assert np.all(got[0][1] == -1) and np.all(got[2][1] == -1) and np.all(np.isinf(got[3][1]))
    from se3et_amd.feature_matching import extract_correspondences_from_feats_pairs
    for kwargs in (dict(), dict(mutual=True), dict(bilateral=True), dict(bilateral='concat')):
        i, j = extract_correspondences_from_feats_pairs([_gpu(ref[5:7])], [_gpu(src)], **kwargs)
        assert i[0].numel() == 0 and j[0].numel() == 0


def test_deterministic_and_batch_independent():
    rng = np.random.default_rng(13)
    pairs = [twin.planted_features(rng, n, m, 256, min(n, m) // 2) for n, m in ((3000, 2800), (700, 900), (1500, 1500))]
    refs, srcs = [p[0] for p in pairs], [p[1] for p in pairs]
    a, b = _device_nn(refs, srcs), _device_nn(refs, srcs)
    for k in range(4):
        for p in range(3):
            assert np.array_equal(a[k][p].view(np.int32 if k % 2 else np.int64), b[k][p].view(np.int32 if k % 2 else np.int64))
    for p in range(3):
        alone = _device_nn(refs[p:p + 1], srcs[p:p + 1])
        for k in range(4):
            assert np.array_equal(alone[k][0].view(np.int32 if k % 2 else np.int64), a[k][p].view(np.int32 if k % 2 else np.int64)), (p, k)


def test_extraction_modes_equal_the_twin_and_the_fixture():
    from se3et_amd import feature_matching as FM
    g = np.load(os.path.join(HERE, 'golden', 'feature_matching.npz'))
    rng = np.random.default_rng(14)
    hub = twin.planted_features(rng, 260, 240, 16, 100)
    hub[1][40:140] = hub[0][17] + 1e-3 * rng.normal(size=(100, 16)).astype(np.float32)     # a ref row that is nearest to 100 src rows
    pairs = [(g['c256/ref_feats'], g['c256/src_feats']), hub, (hub[0][:0], hub[1]), (hub[0][:1], hub[1][:1])]
    pairs32 = [(g['c32/ref_feats'], g['c32/src_feats'])]
    for batch in (pairs32, [(p[0][:, :16].copy(), p[1][:, :16].copy()) for p in pairs]):
        refs, srcs = [_gpu(p[0]) for p in batch], [_gpu(p[1]) for p in batch]
        nn_src, _, nn_ref, _ = FM.nearest_feature_pairs(refs, srcs)
        for mode, kwargs in (('one_way', {}), ('mutual', dict(mutual=True)), ('bilateral_mask', dict(bilateral=True)),
                             ('bilateral_concat', dict(bilateral='concat'))):
            ci, cj, cd = FM.extract_correspondences_from_feats_pairs(refs, srcs, return_feat_dist=True, **kwargs)
            for p in range(len(batch)):
                ti, tj = twin.extract(nn_src[p].cpu().numpy(), nn_ref[p].cpu().numpy(), mode)
                assert ci[p].dtype == torch.int64 and np.array_equal(ci[p].cpu().numpy(), ti) and np.array_equal(cj[p].cpu().numpy(), tj), \
                    (mode, p)
                want = twin.direct_sq_distance(batch[p][0][ti], batch[p][1], tj) if len(ti) else np.zeros(0)
                assert np.allclose(cd[p].cpu().numpy(), want, rtol=1e-4, atol=1e-5)
    # the reference's own lists, exactly (the fixture has no near-tie row), through the numpy drop-ins
    for name in ('c256', 'c32'):
        ref, src = g[name + '/ref_feats'], g[name + '/src_feats']
        for key, kwargs in (('one_way', {}), ('mutual', dict(mutual=True)), ('bilateral', dict(bilateral=True))):
            i, j = FM.extract_corr_indices_from_feats(ref, src, **kwargs)
            assert i.dtype == np.int64 and np.array_equal(i, g[name + '/' + key + '_ref']) and np.array_equal(j, g[name + '/' + key + '_src'])
        rp, sp = np.arange(400 * 3, dtype=np.float64).reshape(400, 3), np.arange(350 * 3, dtype=np.float64).reshape(350, 3)
        a, b, d = FM.extract_correspondences_from_feats(rp, sp, ref, src, mutual=True, return_feat_dist=True)
        i, j = g[name + '/mutual_ref'], g[name + '/mutual_src']
        assert np.array_equal(a, rp[i]) and np.array_equal(b, sp[j])
        assert np.allclose(d, np.linalg.norm(ref[i].astype(np.float64) - src[j], axis=1), rtol=1e-5)


@pytest.mark.parametrize('total', [1, 1023, 1024, 1025, 2049])
def test_extraction_at_the_chunk_sizes_of_the_entry_scan(total):
    """ref rows + src rows is the length of the one-workgroup scan of the entry offsets: one entry, the last sizes with one entry per
    thread, the first with two, an uneven multi-entry size."""
    from se3et_amd import feature_matching as FM
    rng = np.random.default_rng(total)
    ref = rng.normal(size=((total + 1) // 2, 16)).astype(np.float32)
    src = rng.normal(size=(total // 2, 16)).astype(np.float32)
    refs, srcs = [_gpu(ref)], [_gpu(src)]
    nn_src, _, nn_ref, _ = FM.nearest_feature_pairs(refs, srcs)
    for mode, kwargs in (('one_way', {}), ('mutual', dict(mutual=True))):
        ci, cj = FM.extract_correspondences_from_feats_pairs(refs, srcs, **kwargs)
        ti, tj = twin.extract(nn_src[0].cpu().numpy(), nn_ref[0].cpu().numpy(), mode)
        assert mode != 'one_way' or len(ti) == (len(ref) if len(src) else 0)          # (every ref row has a nearest src row)
        assert np.array_equal(ci[0].cpu().numpy(), ti) and np.array_equal(cj[0].cpu().numpy(), tj), mode


def test_torch_mirror_against_the_matrix_composition():
    from se3et_amd import ops
    from se3et_amd.modules.registration import extract_correspondences_from_feats
    rng = np.random.default_rng(15)
    ref, src = twin.planted_features(rng, 1200, 1100, 64, 600)
    r, s = _gpu(ref), _gpu(src)
    _, _, near_a, _ = twin.near_ties(ref, src)
    _, _, near_b, _ = twin.near_ties(src, ref)
    assert near_a.mean() <= CAP and near_b.mean() <= CAP
    d = ops.pairwise_distance(r, s)
    jm, im = torch.min(d, dim=1).indices.cpu().numpy(), torch.min(d, dim=0).indices.cpu().numpy()
    clear = lambda i, j: ~near_a[i] & ~near_b[j]
    for kwargs in (dict(), dict(mutual=True), dict(bilateral=True)):
        ti, tj, cd = extract_correspondences_from_feats(r, s, return_feat_dist=True, **kwargs)
        ci, cj = ti.cpu().numpy(), tj.cpu().numpy()
        mode = 'mutual' if kwargs.get('mutual') else ('bilateral_mask' if kwargs.get('bilateral') else 'one_way')
        wi, wj = twin.extract(jm, im, mode)
        got = {(a, b) for a, b in zip(ci.tolist(), cj.tolist()) if clear(a, b)}
        want = {(a, b) for a, b in zip(wi.tolist(), wj.tolist()) if clear(a, b)}
        assert got == want and len(got) > 500, mode
        assert np.all(np.diff(ci * 1100 + cj) > 0)                   # row-major, no duplicates
        assert np.allclose(cd.cpu().numpy(), d[ti, tj].cpu().numpy(), rtol=1e-3, atol=1e-4)
    # the exp(-d^2) > 0 cut: features 11 apart (d^2 = 121) are no correspondence, features 9 apart (d^2 = 81) are
    x = torch.zeros((3, 8), device='cuda')
    x[1, 0], x[2, 0] = 1000.0, 2000.0
    y = x.clone()
    y[0, 1], y[1, 1] = 11.0, 9.0
    y[2, 1] = 0.5
    i, j, dd = extract_correspondences_from_feats(x, y, return_feat_dist=True)
    assert i.tolist() == [1, 2] and j.tolist() == [1, 2] and dd.tolist() == [81.0, 0.25]
    i, j = extract_correspondences_from_feats(x, y, mutual=True)
    assert i.tolist() == [1, 2]
    i, j = extract_correspondences_from_feats(x, y, bilateral=True)
    assert i.tolist() == [1, 2] and j.tolist() == [1, 2]
    with pytest.raises(RuntimeError):
        extract_correspondences_from_feats(x.double(), y.double())
    with pytest.raises(RuntimeError):
        extract_correspondences_from_feats(x.cpu(), y.cpu())


def test_ransac_checkers_off_is_bit_identical():
    from se3et_amd.ransac import ransac_pairs
    rng = np.random.default_rng(16)
    pairs = [RT.synthetic_pair(rng, n, r) for n, r in ((400, 0.4), (2000, 0.2), (50, 0.5))]
    src, ref = [p[0] for p in pairs], [p[1] for p in pairs]
    plain = ransac_pairs(src, ref, 0.05, 3, 3000, seed=21, per_hypothesis=True)
    off = ransac_pairs(src, ref, 0.05, 3, 3000, seed=21, per_hypothesis=True, edge_length_similarity=None, check_distance=False)
    assert set(plain) == set(off) and 'passed' not in plain
    for k in plain:
        assert torch.equal(plain[k], off[k]), k
    # the checked entry with nothing to reject (similarity ~ 0, no distance check) computes the same, bit for bit
    loose = ransac_pairs(src, ref, 0.05, 3, 3000, seed=21, per_hypothesis=True, edge_length_similarity=1e-30)
    for k in plain:
        assert torch.equal(plain[k], loose[k]), k


@pytest.mark.parametrize('rn', [3, 4])
def test_ransac_checkers_match_the_twin(rn):
    """`passed` against the twin on explicit hypotheses.  A difference is allowed only on the twin's `open` hypotheses: an edge quantity
    within 1e-12 (|ds| + |dr|) of its limit, a sampled distance inside ransac_twin's borderline, or -- under the distance checker -- a
    degenerate fit (second singular value below 1e-9 of the first), where ransac_twin already treats device and twin rotations as
    legitimately different and the sample's residuals with them."""
    from se3et_amd.ransac import ransac_pairs
    H, thr = 2048, 0.05
    sizes, ratios = (60, 500, 3000), (0.6, 0.4, 0.3)
    rng = np.random.default_rng(17 + rn)
    pairs = [RT.synthetic_pair(rng, n, r) for n, r in zip(sizes, ratios)]
    idx = np.stack([rng.integers(0, n, (H, rn)) for n in sizes]).astype(np.int32)
    idx[:, 5, 1] = idx[:, 5, 0]
    src, ref = [p[0] for p in pairs], [p[1] for p in pairs]
    for edge, dist in ((0.9, True), (0.9, False), (None, True)):
        out = ransac_pairs(src, ref, thr, rn, H, hypothesis_indices=torch.from_numpy(idx), per_hypothesis=True,
                           edge_length_similarity=edge, check_distance=dist)
        passed, counts, errs = out['passed'].cpu().numpy(), out['counts'].cpu().numpy(), out['err_sums'].cpu().numpy()
        best = out['best_hypothesis'].cpu().numpy()
        assert passed.dtype == bool and passed.shape == (3, H)
        for p in range(3):
            tw = twin.checked_run(src[p], ref[p], thr, rn, idx[p], edge_t=edge, check_distance=dist)
            differ = passed[p] != tw['passed']
            assert not np.any(differ & ~tw['open']), (edge, dist, p, np.flatnonzero(differ & ~tw['open'])[:5])
            assert 0 < passed[p].sum() < H and tw['open'].sum() < 0.1 * H
            assert np.all(counts[p][~passed[p]] == 0) and np.all(errs[p][~passed[p]] == 0)
            # accepted hypotheses score as without checkers
            same = passed[p] & tw['passed'] & ~tw['degenerate'] & (tw['n_border'] == 0)
            assert np.array_equal(counts[p][same], tw['counts'][same])
            # the winner: the maximum of the total order over the device's own per-hypothesis results
            c, e = counts[p].astype(np.int64), errs[p].astype(np.float64)
            h = -1 if c.max() <= 0 else int(np.lexsort((np.arange(H), e, -c))[0])
            assert best[p] == h and (h < 0 or passed[p][h])
            # ... and as good as the twin's best among its passed hypotheses, within the borderline allowance of ransac_twin
            hb = tw['best']
            if hb >= 0 and not tw['open'][hb]:
                assert h >= 0
                if not tw['open'][h]:
                    assert tw['counts'][h] + tw['n_border'][h] >= tw['counts'][hb] - tw['n_border'][hb], (edge, dist, p, h, hb)


@pytest.mark.parametrize('mutual_filter', [False, True])
def test_registration_from_planted_descriptors(mutual_filter):
    """A cloud under a known transform with 30 % correct descriptor matches: RRE < 1 degree, RTE < 0.05."""
    from se3et_amd.ransac import registration_with_ransac_from_feats
    rng = np.random.default_rng(18)
    n, C = 3000, 32
    src_pts, ref_corr, T = RT.synthetic_pair(rng, n, 1.0, sigma=0.002)
    ref_pts = ref_corr[rng.permutation(n)]
    # descriptors: 30 % of the src points carry (a noisy copy of) the descriptor of their true ref point, the others a random one
    ref_feats = rng.normal(size=(n, C))
    ref_feats /= np.linalg.norm(ref_feats, axis=1, keepdims=True)
    match = np.argmin(((ref_corr[:, None, :] - ref_pts[None]) ** 2).sum(2), 1)       # src row -> its ref row
    src_feats = rng.normal(size=(n, C))
    good = rng.permutation(n)[:int(0.3 * n)]
    src_feats[good] = ref_feats[match[good]] + 0.02 * rng.normal(size=(len(good), C))
    src_feats /= np.linalg.norm(src_feats, axis=1, keepdims=True)
    E = registration_with_ransac_from_feats(src_pts, ref_pts, src_feats.astype(np.float32), ref_feats.astype(np.float32),
                                            distance_threshold=0.05, ransac_n=3, num_iterations=50000, mutual_filter=mutual_filter, seed=4)
    assert E.shape == (4, 4) and E.dtype == np.float64
    rre = np.degrees(np.arccos(np.clip((np.trace(E[:3, :3].T @ T[:3, :3]) - 1) / 2, -1, 1)))
    rte = np.linalg.norm(E[:3, 3] - T[:3, 3])
    print('mutual_filter %s: RRE %.3f deg, RTE %.4f' % (mutual_filter, rre, rte))
    assert rre < 1.0 and rte < 0.05


def test_mutual_filter_falls_back_when_too_few_remain():
    from se3et_amd.ransac import ransac_from_feats_pairs
    rng = np.random.default_rng(19)
    src_pts, ref_pts, _ = RT.synthetic_pair(rng, 40, 1.0)
    # every src descriptor is nearest to ref row 0, whose nearest src row is row 3: one mutual correspondence only
    ref_feats = np.eye(40, 8, dtype=np.float32) * 5 + 10
    ref_feats[0] = 0
    src_feats = (0.01 * (1 + np.abs(np.arange(40) - 3)))[:, None].astype(np.float32) * np.ones((1, 8), np.float32)
    args = ([_gpu(src_pts)], [_gpu(ref_pts)], [_gpu(src_feats)], [_gpu(ref_feats)])
    out = ransac_from_feats_pairs(*args, num_iterations=256, mutual_filter=True)
    assert out['correspondences'][0].shape == (40, 2) and out['correspondences'][0][:, 1].eq(0).all()
    assert torch.isfinite(out['transforms']).all()


def test_ransac_from_features_of_a_forward():
    from se3et_amd.batched import forward_pairs
    from se3et_amd.data import precompute_data_stack_mode
    from se3et_amd.model import create_model, load_synthetic_weights, make_cfg
    from se3et_amd.ransac import ransac_from_feats_pairs
    from se3et_amd.synthetic import make_pair
    cfg = make_cfg('micro_e')
    model = load_synthetic_weights(create_model(cfg)).cuda().eval()
    b = cfg.backbone
    clouds = []
    for i in range(3):
        ref, src, _T = make_pair('micro', i)
        clouds += [ref, src]
    pts = torch.from_numpy(np.concatenate(clouds, 0)).cuda()
    data = precompute_data_stack_mode(pts, torch.tensor([len(c) for c in clouds]), b.num_stages, b.init_voxel_size, b.init_radius,
                                      cfg.neighbor_limits)
    data['features'] = torch.ones((pts.shape[0], 1), device='cuda')
    with torch.no_grad():
        outs = forward_pairs(model, data)
    out = ransac_from_feats_pairs([o['src_points_f'] for o in outs], [o['ref_points_f'] for o in outs],
                                  [o['src_feats_f'] for o in outs], [o['ref_feats_f'] for o in outs],
                                  distance_threshold=0.05, num_iterations=5000, seed=1)
    T = out['transforms']
    assert T.shape == (3, 4, 4) and bool(torch.isfinite(T).all())
    assert torch.equal(T[:, 3], torch.tensor([0., 0, 0, 1], device='cuda').expand(3, 4))
    for o, c in zip(outs, out['correspondences']):
        assert c.shape == (o['src_points_f'].shape[0], 2)
    again = ransac_from_feats_pairs([o['src_points_f'] for o in outs], [o['ref_points_f'] for o in outs],
                                    [o['src_feats_f'] for o in outs], [o['ref_feats_f'] for o in outs],
                                    distance_threshold=0.05, num_iterations=5000, seed=1)
    assert torch.equal(T, again['transforms'])
