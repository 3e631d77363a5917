"""The C oracle (A1/A2) against the genuine reference extension (oracle/_ref/libref_ext.so) on the same seeded clouds: the reference's
outputs are held in tests/golden/ref_ext_tables.npz (generate_golden.py ref_ext) as lengths, float bit-pattern checksums and the
tie-canonical checksum of the neighbour table (the reference orders exact ties with an unstable std::sort)."""
import numpy as np
import pytest
import torch

from helpers import index_checksum, tie_canonical


@pytest.mark.parametrize('n1,n2,scale,voxel', [(5000, 4000, 1.0, 0.05), (12000, 9000, 2.0, 0.05), (3000, 100, 0.5, 0.1),
                                               (30, 2, 0.3, 0.1)])
def test_c_oracle_matches_reference_extension(n1, n2, scale, voxel, golden_dir):
    from oracle import native
    want = np.load(golden_dir + '/ref_ext_tables.npz')
    key = 'oracle/%d_%d_%g_%g/' % (n1, n2, scale, voxel)
    g = np.random.default_rng(0)
    pts = torch.from_numpy((g.uniform(0, 1, (n1 + n2, 3)) * scale).astype(np.float32))
    nrm = torch.from_numpy(g.normal(size=(n1 + n2, 3)).astype(np.float32))
    lens = torch.tensor([n1, n2])
    sp, sl, sn = native.grid_subsample(pts, lens, nrm, voxel)
    assert sl.tolist() == want[key + 'lengths'].tolist()
    bits = lambda t: index_checksum(np.ascontiguousarray(t.numpy()).view(np.uint32))
    assert bits(sp) == int(want[key + 'points']) and bits(sn) == int(want[key + 'normals'])     # same points, same unordered_map order
    nb = native.radius_search(sp, sp, sl, sl, voxel * 2.5, 38)
    assert list(nb.shape) == want[key + 'neighbors_shape'].tolist()
    assert index_checksum(tie_canonical(sp, sp, nb)[0]) == int(want[key + 'neighbors_tiecanon']), 'radius: differs beyond tied entries'
