"""Fixture generator of the keypoint selection (runs ONLY where the reference tree exists; data only travels).

Imports the genuine reference through oracle/ref_shims.py and runs the five "Sampling methods" of geotransformer/utils/pointcloud.py:145-248
unmodified: random_sample_keypoints, sample_keypoints_with_scores, random_sample_keypoints_with_scores, sample_keypoints_with_nms and
random_sample_keypoints_with_nms.  The random forms are seeded with np.random.seed(GOLDEN_SEED) before each call.

Writes tests/golden/keypoints.npz, for every case of tests/keypoint_fixture.py GOLDEN_CASES (uniform random clouds in the unit cube):
  <case>/points (n, 3) float64, <case>/feats (n, FEAT_DIM) float32, <case>/scores (n,) float64
  <case>/<function>/points, <case>/<function>/feats        what the reference returned

Equality of index lists is the right demand only away from the thresholds, so the generator asserts, and fails rather than write:
  all scores of a case are distinct (the reference's argsort leaves ties unspecified);
  no pair of points has d^2 within 1e-9 relative of r^2.
Re-run with:  python tests/golden/generate_keypoints_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_shims  # noqa: E402
from keypoint_fixture import FEAT_DIM, GOLDEN_CASES, GOLDEN_FUNCTIONS, GOLDEN_SEED  # noqa: E402

OUT = os.path.join(HERE, 'keypoints.npz')
MARGIN = 1e-9


def threshold_gap(points, radius):
    """The smallest |d^2 - r^2| / r^2 over all pairs of points."""
    r2, best = radius * radius, np.inf
    for i in range(points.shape[0] - 1):
        d = points[i + 1:] - points[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        best = min(best, float(np.abs(d2 - r2).min()) / r2)
    return best


def main():
    ref_shims.install()
    from geotransformer.utils import pointcloud as P
    store = {}
    for c, (name, n, radius, K) in enumerate(GOLDEN_CASES):
        g = np.random.default_rng(300 + c)
        points = g.uniform(0, 1, (n, 3))
        feats = g.standard_normal((n, FEAT_DIM)).astype(np.float32)
        scores = g.uniform(0.05, 1.0, n)
        assert np.unique(scores).shape[0] == n, '%s: the scores are not distinct' % name
        gap = threshold_gap(points, radius)
        assert gap > MARGIN, '%s: a pair of points sits within %g relative of the radius' % (name, gap)
        store.update({name + '/points': points, name + '/feats': feats, name + '/scores': scores})
        for fn in GOLDEN_FUNCTIONS:
            args = [points, feats] + ([scores] if 'scores' in fn or 'nms' in fn else []) + [K] + ([radius] if 'nms' in fn else [])
            np.random.seed(GOLDEN_SEED)
            out_points, out_feats = getattr(P, fn)(*args)
            assert out_points.shape[0] == out_feats.shape[0] <= K
            store['%s/%s/points' % (name, fn)], store['%s/%s/feats' % (name, fn)] = out_points, out_feats
            print('%-8s %-38s %5d rows' % (name, fn, out_points.shape[0]), flush=True)
        print('%-8s smallest relative gap to the threshold %.3g' % (name, gap), flush=True)
    np.savez_compressed(OUT, **store)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
