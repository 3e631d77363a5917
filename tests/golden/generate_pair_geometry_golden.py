"""Fixture generator of the pair ground truth (runs ONLY where the reference tree exists; data only travels).

Imports the genuine reference through oracle/ref_shims.py: get_nearest_neighbor (geotransformer/utils/pointcloud.py), compute_overlap and
get_correspondences (utils/registration.py) and calibrate_ground_truth (datasets/registration/threedmatch/utils.py).  threedmatch/utils.py
imports nibabel, which is not installed here: the stand-in of generate_benchmark_golden.py is installed first.  calibrate_ground_truth takes
Open3D point clouds and voxel-downsamples them; Open3D is not here either, so it is handed a stand-in whose voxel_down_sample returns
itself and whose `points` is the array -- the functions under test take the clouds as given.

Writes tests/golden/pair_geometry.npz, per case of pair_geometry_twin.CASES (float32 inputs promoted to float64):
  <case>/nn_dist, nn_idx       get_nearest_neighbor(ref, apply_transform(src, T), return_index=True)
  <case>/overlap_radii, overlaps   compute_overlap at each radius
  <case>/corr_counts (int16 per ref row), corr_total, corr_checksum (pair_geometry_twin.checksum), corr_head / corr_tail (64 pairs each)
  <case>/voxel_sizes, seeds, info_overlap, info_cov, info_selected   calibrate_ground_truth per voxel size, numpy seeded before each call
                               (info_selected: the number of rows with d_nn < voxel_size before the draw)
and asserts the margins that make whole-array equality the right demand: no nearest-neighbour or pair distance within 1e-9 (relative) of a
threshold that is tested on it, no query with two exactly equidistant nearest candidates, and the smallest gap between the first and second
neighbour (stored as <case>/min_gap) far above float64 rounding.  It fails rather than write a fixture that sits on a threshold.
Re-run with:  python tests/golden/generate_pair_geometry_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from oracle import ref_shims  # noqa: E402
import pair_geometry_twin as twin  # noqa: E402
from generate_benchmark_golden import _install_nibabel  # noqa: E402

OUT = os.path.join(HERE, 'pair_geometry.npz')
MARGIN = 1e-9


class _Cloud:
    def __init__(self, points):
        self.points = points

    def voxel_down_sample(self, voxel_size):
        return self


def _clear_of(values, thresholds, what):
    for r in thresholds:
        near = np.abs(values - r) <= MARGIN * r
        assert not near.any(), '%s: %d distances within %g of %g' % (what, int(near.sum()), MARGIN, r)


def main():
    from scipy.spatial import cKDTree
    _install_nibabel()
    ref_shims.install()
    from geotransformer.datasets.registration.threedmatch import utils as ref_utils
    from geotransformer.utils import registration as R
    from geotransformer.utils.pointcloud import apply_transform, get_nearest_neighbor
    store = {}
    for case_index, (name, (matching_radius, overlap_radii, voxel_sizes)) in enumerate(twin.CASES.items()):
        ref, src, T = (np.asarray(a, np.float64) for a in twin.case_inputs(name))
        moved = apply_transform(src, T)
        dist, idx = get_nearest_neighbor(ref, moved, return_index=True)
        # margins
        tested = list(overlap_radii) + [v for v in voxel_sizes] + [5 * v for v in voxel_sizes]
        _clear_of(dist, tested, name + ' nearest neighbour')
        tree = cKDTree(moved)
        two = tree.query(ref, k=2)[0]
        gap = float((two[:, 1] - two[:, 0]).min())
        assert gap > 0.0, '%s: a query with two equidistant nearest candidates' % name
        assert gap > 1e-9 * float(np.abs(ref).max()), '%s: first and second neighbour %g apart' % (name, gap)
        inner = tree.query_ball_point(ref, matching_radius * (1 - MARGIN), return_length=True)
        outer = tree.query_ball_point(ref, matching_radius * (1 + MARGIN), return_length=True)
        assert np.array_equal(inner, outer), '%s: pair distances within %g of the matching radius' % (name, MARGIN)
        p = name + '/'
        store[p + 'nn_dist'], store[p + 'nn_idx'] = dist, idx.astype(np.int32)
        store[p + 'min_gap'] = np.float64(gap)
        store[p + 'overlap_radii'] = np.array(overlap_radii, np.float64)
        store[p + 'overlaps'] = np.array([R.compute_overlap(ref, src, T, positive_radius=r) for r in overlap_radii], np.float64)
        corr = R.get_correspondences(ref, src, T, matching_radius).reshape(-1, 2)
        counts = np.bincount(corr[:, 0], minlength=len(ref))
        assert counts.max() < 2 ** 15 and np.array_equal(counts, inner)
        store[p + 'matching_radius'] = np.float64(matching_radius)
        store[p + 'corr_counts'] = counts.astype(np.int16)
        store[p + 'corr_total'] = np.int64(len(corr))
        store[p + 'corr_checksum'] = twin.checksum(corr)
        store[p + 'corr_head'], store[p + 'corr_tail'] = corr[:64].astype(np.int64), corr[-64:].astype(np.int64)
        seeds, overlaps, covs, selected = [], [], [], []
        for k, v in enumerate(voxel_sizes):
            seed = 1000 + 10 * case_index + k
            np.random.seed(seed)
            ov, cov = ref_utils.calibrate_ground_truth(_Cloud(ref), _Cloud(src), T, voxel_size=v)
            seeds.append(seed), overlaps.append(ov), covs.append(cov), selected.append(int((dist < v).sum()))
        store[p + 'voxel_sizes'] = np.array(voxel_sizes, np.float64)
        store[p + 'seeds'] = np.array(seeds, np.int64)
        store[p + 'info_overlap'] = np.array(overlaps, np.float64)
        store[p + 'info_cov'] = np.stack(covs).astype(np.float64)
        store[p + 'info_selected'] = np.array(selected, np.int64)
        print('%-8s overlaps %s, %d correspondences, selected %s, min gap %.2e' % (name, np.round(store[p + 'overlaps'], 4), len(corr),
                                                                                 selected, gap))
    np.savez_compressed(OUT, **store)
    size = os.path.getsize(OUT)
    assert size < (1 << 20), '%d bytes: above the size limit of a committed file' % size
    print('wrote', OUT, size, 'bytes')


if __name__ == '__main__':
    main()
