"""A numpy restatement of the block-sparse TSDF contract (se3et_amd/tsdf_sparse.py, csrc/tsdf_sparse.hip): contract A as float64 numpy
over the sampled pixels of a frame, contract B as tsdf_twin.integrate on each block with its frame subset, contract C as the plain loop
reading through a dictionary of blocks.  Nothing here is shared with the library.

A volume set is a dict (volume, bx, by, bz) -> tsdf_twin state of resolution 16."""
import numpy as np

import tsdf_twin as uniform

F32 = np.float32
BLOCK, COORD_BITS, MAX_TRUNC_VOXELS, MAX_STRIDE, POSE_WORDS = 16, 19, 16, 64, 16
BIAS = 1 << (COORD_BITS - 1)


def key_of(coord):
    v, bx, by, bz = (int(c) for c in coord)
    return (v << (3 * COORD_BITS)) | ((bx + BIAS) << (2 * COORD_BITS)) | ((by + BIAS) << COORD_BITS) | (bz + BIAS)


def coord_of(key):
    mask = (1 << COORD_BITS) - 1
    key = int(key)
    return (key >> (3 * COORD_BITS), ((key >> (2 * COORD_BITS)) & mask) - BIAS, ((key >> COORD_BITS) & mask) - BIAS, (key & mask) - BIAS)


def camera_poses(extrinsics):
    """P = E^-1, float64, one frame at a time"""
    E = np.asarray(extrinsics, dtype=np.float64).reshape(-1, 4, 4)
    return np.array([np.linalg.inv(e) for e in E]).reshape(-1, 4, 4)


def pose_table(extrinsics, intrinsics):
    """(F, 16) float64: the 3 x 4 camera pose by rows, then fx, fy, cx, cy"""
    P = camera_poses(extrinsics)
    K = np.broadcast_to(np.asarray(intrinsics, dtype=np.float64).reshape(-1, 4), (len(P), 4))
    return np.ascontiguousarray(np.concatenate([P[:, :3, :].reshape(len(P), 12), K], 1))


def volume_of_frame(counts):
    return np.repeat(np.arange(len(counts)), counts)


def touch(depths, poses, counts, vl, trunc, stride, depth_scale=1000.0, depth_trunc=3.0):
    """Contract A: the sorted list of distinct (key, frame).  ValueError('frame f') for a coordinate out of range."""
    F, H, W = depths.shape
    L = 16.0 * float(vl)
    vols = volume_of_frame(counts)
    records = set()
    for f in range(F):
        i, j = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing='ij')
        with np.errstate(all='ignore'):
            d = depths[f][i, j].astype(F32) / F32(depth_scale)
            d = np.where(d >= F32(depth_trunc), F32(0), d)
            keep = d > 0
            z = d.astype(np.float64)
            P, (fx, fy, cx, cy) = poses[f, :12].reshape(3, 4), poses[f, 12:]
            x, y = ((j - cx) * z) / fx, ((i - cy) * z) / fy
            q = [((P[a, 0] * x + P[a, 1] * y) + P[a, 2] * z) + P[a, 3] for a in range(3)]
            keep &= np.isfinite(q[0]) & np.isfinite(q[1]) & np.isfinite(q[2])
            lo = [np.floor((q[a] - trunc) / L) for a in range(3)]
            hi = [np.floor((q[a] + trunc) / L) for a in range(3)]
        for r, c in zip(*np.nonzero(keep)):
            l, h = [lo[a][r, c] for a in range(3)], [hi[a][r, c] for a in range(3)]
            if min(l) < -BIAS or max(h) >= BIAS:
                raise ValueError('frame %d' % f)
            for bx in range(int(l[0]), int(h[0]) + 1):
                for by in range(int(l[1]), int(h[1]) + 1):
                    for bz in range(int(l[2]), int(h[2]) + 1):
                        records.add((key_of((vols[f], bx, by, bz)), f))
    return sorted(records)


def frame_lists(records):
    """key -> its frames, ascending; keys in ascending order"""
    out = {}
    for key, f in records:
        out.setdefault(key, []).append(f)
    return out


def integrate(blocks, color, vl, trunc, depths, table, poses, counts, stride, colors=None, depth_scale=1000.0, depth_trunc=3.0):
    """Contracts A and B, in place: the touched blocks come to exist, then each integrates its frames as a uniform volume of resolution 16"""
    L = 16.0 * float(vl)
    for key, frames in frame_lists(touch(depths, poses, counts, vl, trunc, stride, depth_scale, depth_trunc)).items():
        coord = coord_of(key)
        state = blocks.setdefault(coord, uniform.new_state(BLOCK, color))
        origin = [L * float(b) for b in coord[1:]]
        uniform.integrate(state, vl, trunc, origin, depths[frames], table[frames], None if colors is None else colors[frames], depth_scale, depth_trunc)
    return blocks


def _at(blocks, coord, idx):
    """(state, local index) of voxel idx, each index in [-1, 17], around block coord; None in an absent block"""
    assert all(-1 <= i <= BLOCK + 1 for i in idx)
    there = (coord[0],) + tuple(coord[1 + a] + idx[a] // BLOCK for a in range(3))
    state = blocks.get(there)
    return None if state is None else (state, tuple(i % BLOCK for i in idx))


def _tsdf(blocks, coord, idx):
    hit = _at(blocks, coord, idx)
    return 0.0 if hit is None else float(hit[0]['tsdf'][hit[1]])


def _trilinear(blocks, coord, vl, q):
    g = [q[a] / vl - 0.5 for a in range(3)]
    i = [int(np.floor(x)) for x in g]
    r = [g[a] - np.floor(g[a]) for a in range(3)]
    s = [1.0 - x for x in r]
    f = lambda dx, dy, dz: _tsdf(blocks, coord, (i[0] + dx, i[1] + dy, i[2] + dz))
    plane = lambda dx: s[1] * (s[2] * f(dx, 0, 0) + r[2] * f(dx, 0, 1)) + r[1] * (s[2] * f(dx, 1, 0) + r[2] * f(dx, 1, 1))
    return s[0] * plane(0) + r[0] * plane(1)


def _usable(w, t):
    return w != 0 and t < F32(0.98) and t >= F32(-0.98)


def extract(blocks, vl, num_volumes, color):
    """Contract C: per volume (points, normals, colors or None), float64, blocks in key order, (x, y, z, axis) inside a block"""
    vl = float(vl)
    L = 16.0 * vl
    out = [([], [], []) for _ in range(num_volumes)]
    with np.errstate(all='ignore'):
        for coord in sorted(blocks, key=key_of):
            t, w = blocks[coord]['tsdf'], blocks[coord]['weight']
            points, normals, colors = out[coord[0]]
            origin = [L * float(b) for b in coord[1:]]
            usable = (w != 0) & (t < F32(0.98)) & (t >= F32(-0.98)) & (t != 0)
            for idx0 in [tuple(int(v) for v in i) for i in zip(*np.nonzero(usable))]:
                f0 = t[idx0]
                for axis in range(3):
                    idx1 = list(idx0)
                    idx1[axis] += 1
                    hit = _at(blocks, coord, idx1)
                    if hit is None:
                        continue
                    f1, w1 = hit[0]['tsdf'][hit[1]], hit[0]['weight'][hit[1]]
                    if not (_usable(w1, f1) and f1 != 0 and (f0 < 0) != (f1 < 0)):
                        continue
                    r0, r1 = abs(float(f0)), abs(float(f1))
                    p = [vl / 2.0 + vl * float(idx0[a]) for a in range(3)]
                    p1 = p[axis] + vl
                    p[axis] = ((p[axis] * r1) + (p1 * r0)) / (r0 + r1)
                    points.append([p[a] + origin[a] for a in range(3)])
                    if color:
                        c0, c1 = blocks[coord]['color'], hit[0]['color']
                        colors.append([((float(c0[k][idx0]) * r1) + (float(c1[k][hit[1]]) * r0)) / (r0 + r1) for k in range(3)])
                    h = 0.99 * vl
                    n = []
                    for a in range(3):
                        hi, lo = list(p), list(p)
                        hi[a], lo[a] = p[a] + h, p[a] - h
                        n.append(_trilinear(blocks, coord, vl, hi) - _trilinear(blocks, coord, vl, lo))
                    length = float(np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))
                    normals.append([v / length for v in n] if length > 0 else n)
    as_rows = lambda rows: np.array(rows, dtype=np.float64).reshape(-1, 3)
    return [(as_rows(p), as_rows(n), as_rows(c) if color else None) for p, n, c in out]
