"""Fixture generator of the geometric edge cases of grid subsampling and the radius search (runs ONLY where the reference tree and
oracle/_ref exist; recorded results only travel).

Runs the reference's own compiled extension (oracle/ref_shims._RefExt over oracle/_ref/libref_ext.so) on the seeded cases of
tests/precompute_edge_fixture.py and writes tests/golden/precompute_edges.npz:

  grid/<case>/lengths     (3, clouds) int64: the per-cloud counts of three chained stages (voxel, 2 voxel, 4 voxel)
  grid/<case>/points      (3,) order-sensitive checksums of the float BIT PATTERNS of each stage's points (helpers.index_checksum)
  grid/<case>/normals     (3,) the same of the normals
  radius/<case>/shape     the neighbour table cut to the case's limit
  radius/<case>/tiecanon  checksum of its tie-canonical form (helpers.tie_canonical: the reference leaves exact ties to an unstable sort)
  radius/<case>/counts    checksum of the per-row in-radius counts (from the uncut table)

What the reference cannot be given as it stands, and what is done instead:
  * a cloud without points in grid subsampling (it reads points[0] of every cloud: undefined).  Case `stack32`: the reference runs over
    the non-empty clouds only and the empty ones are recorded with length 0 -- the stacked outputs are the same rows either way;
  * a cloud without queries behind the first cloud of a radius search (its cloud counter advances once per query ROW and at most one
    cloud at a time: the rows behind an empty cloud would be searched in the wrong support).  Cases stack32_*: the reference runs over the
    clouds that have queries, and its indices into their stacked supports are mapped back to the full stack (padding -> the full total).
    A cloud without support points is fine (an empty k-d tree answers "no neighbour").
  * NaN and infinite queries ARE run: nanoflann only compares and subtracts them (no conversion to an index), every comparison is false and
    the row comes back empty, which this generator asserts.

The file is written with fixed zip time stamps: regenerating it reproduces it byte for byte.
Re-run with:  python tests/golden/generate_precompute_edges_golden.py"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_shims  # noqa: E402
from helpers import index_checksum, tie_canonical  # noqa: E402  (tests/helpers.py)
import precompute_edge_fixture as F  # noqa: E402  (tests/precompute_edge_fixture.py)

FIXTURE = os.path.join(HERE, 'precompute_edges.npz')


def float_bits_checksum(t):
    return index_checksum(np.ascontiguousarray(t.numpy()).view(np.uint32))


def run_grid_case(ext, name, case):
    lengths = torch.tensor(case['lengths'], dtype=torch.int64)
    some = lengths > 0                                           # (see the module docstring: the reference cannot take an empty cloud)
    p, n, l = torch.from_numpy(case['points'].copy()), torch.from_numpy(case['normals'].copy()), lengths[some].contiguous()
    out_l, out_p, out_n = [], [], []
    for k in range(F.CHAIN_STAGES):
        p, l, n = ext.grid_subsampling(p, l, n, case['voxel'] * 2 ** k)
        full = torch.zeros_like(lengths)
        full[some] = l
        out_l.append(full.numpy())
        out_p.append(float_bits_checksum(p))
        out_n.append(float_bits_checksum(n))
    print('grid  ', name, [int(v.sum()) for v in out_l], flush=True)
    key = 'grid/%s/' % name
    return {key + 'lengths': np.stack(out_l), key + 'points': np.array(out_p, np.int64), key + 'normals': np.array(out_n, np.int64)}


def run_radius_case(ext, name, case):
    q, s = torch.from_numpy(case['q'].copy()), torch.from_numpy(case['s'].copy())
    ql, sl = torch.tensor(case['q_lengths'], dtype=torch.int64), torch.tensor(case['s_lengths'], dtype=torch.int64)
    some = ql > 0                                                # (see the module docstring: only clouds that have queries)
    rows = torch.repeat_interleave(some, sl)                     # support rows of those clouds
    back = torch.cat((torch.nonzero(rows)[:, 0], torch.tensor([s.shape[0]])))
    full = back[ext.radius_neighbors(q, s[rows].contiguous(), ql[some].contiguous(), sl[some].contiguous(), case['radius'])]
    counts = (full < s.shape[0]).sum(1).numpy()
    np.testing.assert_array_equal(counts, F.radius_counts(case)[0], err_msg=name)          # (the predicate of the fixture module agrees)
    if 'awkward_rows' in case:
        assert counts[case['awkward_rows']].max() == 0, name
    t = full[:, :case['limit']].contiguous()
    canon, rows, entries = tie_canonical(q, s, t)
    print('radius', name, tuple(t.shape), 'largest count', int(counts.max()) if len(counts) else 0, 'rows with ties', rows, flush=True)
    key = 'radius/%s/' % name
    return {key + 'shape': np.array(t.shape, np.int64), key + 'tiecanon': np.int64(index_checksum(canon)),
            key + 'counts': np.int64(index_checksum(counts))}


def save_reproducibly(path, arrays):
    """An .npz (np.load reads it) whose bytes depend on the arrays alone: sorted members, a fixed time stamp."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


if __name__ == '__main__':
    ext = ref_shims._RefExt(ref_shims.REF_EXT_SO)
    res = {}
    for name, case in F.grid_cases().items():
        res.update(run_grid_case(ext, name, case))
    for name, case in F.radius_cases().items():
        res.update(run_radius_case(ext, name, case))
    save_reproducibly(FIXTURE, res)
    print(FIXTURE, os.path.getsize(FIXTURE), 'bytes')
