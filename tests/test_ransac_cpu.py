"""CPU: the RANSAC configuration (make_cfg's cfg.ransac), the seeded sampler of se3et_amd.ransac and the host twin (tests/ransac_twin.py)
that the GPU tests hold the kernels to."""
import numpy as np
import pytest

import ransac_twin as RT

# experiments/se3ete*.3dmatch/config.py and se3eti*.3dmatch/config.py: 62-68; experiments/se3eti.kitti/config.py:65-68
RANSAC_3DMATCH = dict(distance_threshold=0.05, num_points=3, num_iterations=50000)
RANSAC_KITTI = dict(distance_threshold=0.3, num_points=4, num_iterations=50000)


def test_make_cfg_carries_the_reference_ransac_section():
    from se3et_amd.model import VARIANTS, make_cfg
    for variant in VARIANTS:
        want = RANSAC_KITTI if variant.endswith('kitti') else RANSAC_3DMATCH
        assert vars(make_cfg(variant).ransac) == want, variant


def test_sample_indices_deterministic_and_in_range():
    from se3et_amd.ransac import sample_indices
    for n in (1, 3, 7, 1000, 5000, (1 << 32) - 1):
        a = sample_indices(123, n, 2000, 4)
        assert a.shape == (2000, 4) and a.dtype == np.int64
        assert a.min() >= 0 and a.max() < n
        assert np.array_equal(a, sample_indices(123, n, 2000, 4))
    assert not np.array_equal(sample_indices(0, 5000, 100, 3), sample_indices(1, 5000, 100, 3))
    # uniform enough: every bucket of a 10-way split of [0, n) gets its share of 60 000 draws within 5 %
    counts = np.bincount(sample_indices(7, 1000, 20000, 3).ravel() // 100, minlength=10)
    assert np.all(np.abs(counts - 6000) < 300), counts


def test_sample_stream_depends_on_seed_h_j_n_only():
    """idx[h, j] is a function of (seed, h * ransac_n + j, n): a longer run extends a shorter one, and the stream of ransac_n = 3 is the
    flat stream of ransac_n = 1 cut into rows of 3."""
    from se3et_amd.ransac import sample_indices
    a, b = sample_indices(5, 777, 100, 3), sample_indices(5, 777, 1000, 3)
    assert np.array_equal(a, b[:100])
    assert np.array_equal(sample_indices(5, 777, 300, 1).reshape(100, 3), a)
    # the formula, element by element in Python integers
    M = (1 << 64) - 1

    def sm(x):
        z = (x + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    for seed in (0, 5, (1 << 64) - 1):
        got = sample_indices(seed, 777, 4, 3)
        for h in range(4):
            for j in range(3):
                assert got[h, j] == ((sm((sm(seed) + h * 3 + j) & M) >> 32) * 777) >> 32


def test_twin_recovers_a_known_transform():
    from se3et_amd.ransac import sample_indices
    rng = np.random.default_rng(0)
    src, ref, T = RT.synthetic_pair(rng, 2000, 0.10)
    out = RT.run(src, ref, 0.05, 3, sample_indices(0, 2000, 20000, 3))
    E = out['transform']
    rre = np.degrees(np.arccos(np.clip((np.trace(E[:3, :3].T @ T[:3, :3]) - 1) / 2, -1, 1)))
    assert rre < 2.0 and np.linalg.norm(E[:3, 3] - T[:3, 3]) < 0.05
    assert 0.08 < out['fitness'] <= 0.11 and 0 < out['rmse'] < 0.05
    assert out['counts'][out['best']] == out['counts'].max()


def test_twin_exact_sample_fits_exactly():
    rng = np.random.default_rng(1)
    src, ref, T = RT.synthetic_pair(rng, 50, 1.0, sigma=0.0)
    R, t, deg = RT.fit(src[None, :5].astype(np.float64), ref[None, :5].astype(np.float64))
    assert not deg[0]
    assert np.abs(R[0] - T[:3, :3]).max() < 1e-6 and np.abs(t[0] - T[:3, 3]).max() < 1e-6
    # collinear and repeated samples are flagged
    line = np.outer(np.arange(3.0), [1.0, 2.0, 3.0])[None]
    assert RT.fit(line, line + 1.0)[2][0]
    same = np.repeat(src[None, :1].astype(np.float64), 3, axis=1)
    assert RT.fit(same, same)[2][0]


@pytest.mark.parametrize('case', ['few', 'rn2', 'thr0', 'thrneg', 'noinlier'])
def test_twin_identity_cases(case):
    rng = np.random.default_rng(2)
    src, ref, _ = RT.synthetic_pair(rng, 100, 0.5)
    idx = rng.integers(0, 100, (64, 3))
    if case == 'few':
        out = RT.run(src[:2], ref[:2], 0.05, 3, np.zeros((64, 3), np.int64))
    elif case == 'rn2':
        out = RT.run(src, ref, 0.05, 2, idx[:, :2])
    elif case == 'thr0':
        out = RT.run(src, ref, 0.0, 3, idx)
    elif case == 'thrneg':
        out = RT.run(src, ref, -1.0, 3, idx)
    else:       # no hypothesis has an inlier: far-apart ref points at a tiny threshold
        out = RT.run(src, ref * 100.0, 1e-9, 3, idx)
        assert out['counts'].max() == 0
    assert out['best'] == -1 and out['fitness'] == 0.0 and out['rmse'] == 0.0
    assert np.array_equal(out['transform'], np.eye(4))


def test_twin_ranking_ties_take_the_lowest_h():
    rng = np.random.default_rng(3)
    src, ref, _ = RT.synthetic_pair(rng, 200, 0.5)
    idx = rng.integers(0, 200, (32, 3))
    idx[20] = idx[7]                       # the same sample twice: equal count and error sum
    out = RT.run(src, ref, 0.05, 3, idx)
    order = sorted(range(32), key=lambda h: (-out['counts'][h], out['err_sums'][h], h))
    assert out['best'] == order[0]
    assert out['counts'][20] == out['counts'][7] and out['err_sums'][20] == out['err_sums'][7]
    idx[:] = idx[7]
    assert RT.run(src, ref, 0.05, 3, idx)['best'] == (0 if out['counts'][7] > 0 else -1)


def test_select_correspondences_is_a_stable_top_k():
    import torch
    from se3et_amd.ransac import select_correspondences
    scores = torch.tensor([0.5, 0.9, 0.5, 0.1, 0.9, 0.5])
    pts = torch.arange(18, dtype=torch.float32).reshape(6, 3)
    out = dict(ref_corr_points=pts, src_corr_points=pts + 100, corr_scores=scores)
    r, s, c = select_correspondences(out, 4)
    assert (r[:, 0] / 3).long().tolist() == [1, 4, 0, 2]
    assert torch.equal(c, scores[[1, 4, 0, 2]])
    assert torch.equal(s, r + 100)
    assert select_correspondences(out, None)[2] is scores and select_correspondences(out, 6)[2] is scores
