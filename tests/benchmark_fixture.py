"""Seeded inputs of tests/golden/benchmark_metrics.npz (shared by tests/golden/generate_benchmark_golden.py and the benchmark tests).

The correspondence sets are too large to store, so the fixture stores the seeds and checksums of what pair_inputs draws here; the tests
redraw them and check the checksums before comparing anything.  A pair's inputs depend only on (benchmark, index, attempt) and its
ground-truth transform:
  - n correspondences: log-uniform in [20, 2000], 20 000 for every 200th pair;
  - ref_corr points uniform in a box (8 m; KITTI 80 m) around the origin;
  - a seeded fraction of inliers, whose src point lies at |noise| in [0, 0.95 r) of its ref point, a tenth of near misses at
    (1.05 r, 2 r), the rest uniform in the box; src_corr = T^-1 of that point (float64, rounded to float32);
  - N, M coarse nodes in [8, 300), ground-truth node pairs (with repeats) and predicted node pairs that mix ground-truth pairs and
    random ones, drawn with replacement (duplicates), possibly none.
The generator redraws a pair (attempt + 1) until no inlier test and no nearest-neighbour distance lies within MARGIN r^2 of r^2 in
float64, so that float32 and float64 distances count the same points."""
import numpy as np

from eval_fixture import float_checksum, index_checksum

MARGIN = 1e-4
BIG_EVERY = 200
BENCH_ID = {'3DMatch': 1, '3DLoMatch': 2, 'KITTI': 3}


def pair_inputs(benchmark, index, attempt, transform, radius):
    """The seeded inputs of one pair: a dict of numpy arrays (float32 points and scores, int64 node indices) and node counts."""
    rng = np.random.default_rng([20261016, BENCH_ID[benchmark], int(index), int(attempt)])
    kitti = benchmark == 'KITTI'
    n = 20000 if index % BIG_EVERY == BIG_EVERY - 1 else int(np.exp(rng.uniform(np.log(20), np.log(2000))))
    box = 80.0 if kitti else 8.0
    ref = rng.uniform(-box / 2, box / 2, (n, 3))
    kind = rng.random(n)
    frac = rng.uniform(0.0, 0.9)
    inlier, near = kind < frac, (kind >= frac) & (kind < frac + 0.1)
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    mag = np.where(inlier, rng.uniform(0, 0.95, n), rng.uniform(1.05, 2.0, n)) * radius
    world = ref + direction * mag[:, None]
    far = ~(inlier | near)
    world[far] = rng.uniform(-box / 2, box / 2, (int(far.sum()), 3))
    T = np.asarray(transform, np.float64)
    src = (world - T[:3, 3]) @ T[:3, :3]                     # T^-1 (rows): R^T (x - t)
    N, M = int(rng.integers(8, 300)), int(rng.integers(8, 300))
    g = int(rng.integers(0, 3 * min(N, M)))
    gt = np.stack([rng.integers(0, N, g), rng.integers(0, M, g)], 1).astype(np.int64)
    k = 0 if index % 50 == 7 else int(rng.integers(1, 2 * min(N, M)))
    take_gt = rng.random(k) < rng.uniform(0, 1) if g else np.zeros(k, bool)
    pred = np.stack([rng.integers(0, N, k), rng.integers(0, M, k)], 1).astype(np.int64)
    if g:
        pred[take_gt] = gt[rng.integers(0, g, int(take_gt.sum()))]
    return dict(ref_corr_points=ref.astype(np.float32), src_corr_points=src.astype(np.float32),
                corr_scores=rng.random(n).astype(np.float32), ref_node_corr_indices=pred[:, 0].copy(),
                src_node_corr_indices=pred[:, 1].copy(), gt_node_corr_indices=gt, num_ref_nodes=N, num_src_nodes=M)


def inputs_checksum(d):
    """One order-sensitive checksum of a pair's inputs."""
    parts = [float_checksum(d[k]) for k in ('ref_corr_points', 'src_corr_points', 'corr_scores')]
    parts += [index_checksum(d[k]) for k in ('ref_node_corr_indices', 'src_node_corr_indices', 'gt_node_corr_indices')]
    parts += [d['num_ref_nodes'], d['num_src_nodes']]
    return index_checksum(np.array(parts, np.uint64) % np.uint64(2 ** 61 - 1))
