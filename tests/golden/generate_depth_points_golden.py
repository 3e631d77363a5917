"""Fixture generator for tests/golden/depth_points.npz (runs only where the reference tree exists).

Imports the genuine reference through oracle/ref_shims.py and runs its convert_depth_mat_to_points
(geotransformer/utils/pointcloud.py) on the depth image of tests/tsdf_fixture.py: 24 x 32 uint16 with zeros, pixels beyond the distance
limit and non-square intrinsics.  The file holds data only: the image, the intrinsics, the two parameters and the reference's points,
with its fractional rows and its (0, 0, 0) rows for far pixels.  Re-run with:  python tests/golden/generate_depth_points_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_shims  # noqa: E402
import tsdf_fixture as F  # noqa: E402


def main():
    ref_shims.install()
    from geotransformer.utils.pointcloud import convert_depth_mat_to_points
    depth, K = F.depth_image(np.uint16)
    intrinsics = np.array([[K[0], 0.0, K[2]], [0.0, K[1], K[3]], [0.0, 0.0, 1.0]])
    out = {'depth': depth, 'intrinsics': intrinsics}
    for tag, (scale, limit) in {'default': (1000.0, 6.0), 'near': (500.0, 3.5)}.items():
        pts = convert_depth_mat_to_points(depth.copy(), intrinsics, scaling_factor=scale, distance_limit=limit)
        assert pts.dtype == np.float64
        out['%s_params' % tag], out['%s_points' % tag] = np.array([scale, limit]), pts
        print('%s: %d points, %d of them (0, 0, 0) rows, %d fractional rows' % (tag, len(pts), int((~pts.any(1)).sum()),
                                                                                int((pts[:, 2] > 0).sum())))
    np.savez_compressed(os.path.join(HERE, 'depth_points.npz'), **out)


if __name__ == '__main__':
    main()
