"""What a user does next with the triangle meshes of TSDFVolumes / SparseTSDFVolumes.extract_triangle_meshes, on the host:

  write_triangle_mesh_ply(path, vertices, triangles, normals=None, colors=None)      a binary little-endian PLY file
  mesh_edge_census(triangles)      how often every directed edge and its reverse occur: the watertightness check

Both take tensors (from any device) or arrays."""
import numpy as np
import torch


def _host(x, dtype, what, name, rows=None):
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    if a.ndim != 2 or a.shape[1] != 3 or (rows is not None and a.shape[0] != rows):
        raise ValueError('%s: %s must be (%s, 3), got %s' % (what, name, 'n' if rows is None else rows, a.shape))
    return a.astype(dtype)


def write_triangle_mesh_ply(path, vertices, triangles, normals=None, colors=None):
    """A binary little-endian PLY file: vertices (n, 3) as double x, y, z, normals (n, 3) as double nx, ny, nz, colors (n, 3) in [0, 1] as
    uchar red, green, blue (rounded to nearest), triangles (m, 3) as faces `list uchar int vertex_indices`.  A triangle must name vertices
    in [0, n) and n must be below 2^31."""
    what = 'write_triangle_mesh_ply'
    v = _host(vertices, '<f8', what, 'vertices')
    n = len(v)
    t = _host(triangles, np.int64, what, 'triangles')
    if n >= 1 << 31 or (len(t) and (t.min() < 0 or t.max() >= n)):
        raise ValueError('%s: a triangle names a vertex outside [0, %d), or there are 2^31 vertices or more' % (what, n))
    fields, columns = [('x', '<f8'), ('y', '<f8'), ('z', '<f8')], [v[:, 0], v[:, 1], v[:, 2]]
    if normals is not None:
        nn = _host(normals, '<f8', what, 'normals', n)
        fields += [('nx', '<f8'), ('ny', '<f8'), ('nz', '<f8')]
        columns += [nn[:, 0], nn[:, 1], nn[:, 2]]
    if colors is not None:
        c = np.clip(np.rint(_host(colors, np.float64, what, 'colors', n) * 255.0), 0, 255).astype(np.uint8)
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
        columns += [c[:, 0], c[:, 1], c[:, 2]]
    names = {'<f8': 'double', 'u1': 'uchar'}
    header = ['ply', 'format binary_little_endian 1.0', 'comment se3et_amd', 'element vertex %d' % n]
    header += ['property %s %s' % (names[kind], name) for name, kind in fields]
    header += ['element face %d' % len(t), 'property list uchar int vertex_indices', 'end_header']
    rows = np.empty((n,), dtype=fields)
    for (name, _), column in zip(fields, columns):
        rows[name] = column
    faces = np.empty((len(t),), dtype=[('count', 'u1'), ('index', '<i4', (3,))])
    faces['count'], faces['index'] = 3, t
    with open(path, 'wb') as f:
        f.write(('\n'.join(header) + '\n').encode('ascii'))
        f.write(rows.tobytes())
        f.write(faces.tobytes())


def mesh_edge_census(triangles):
    """(edges (k, 2) int64, forward (k,), backward (k,) int64): every directed edge (a, b) that a triangle has, once, in ascending order,
    with the number of times it occurs and the number of times its reverse (b, a) occurs.  A closed oriented 2-manifold has forward ==
    backward == 1 everywhere; a boundary edge has backward == 0; an edge used more than twice has forward + backward > 2."""
    t = (triangles.detach().cpu().numpy() if torch.is_tensor(triangles) else np.asarray(triangles)).astype(np.int64).reshape(-1, 3)
    directed = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], 0)
    if len(directed) == 0:
        return np.zeros((0, 2), np.int64), np.zeros((0,), np.int64), np.zeros((0,), np.int64)
    if directed.min() < 0 or directed.max() >= 1 << 31:
        raise ValueError('mesh_edge_census: vertex numbers in [0, 2^31) expected')
    span = int(directed.max()) + 1
    code, forward = np.unique(directed[:, 0] * span + directed[:, 1], return_counts=True)          # (a, b) as one number: ascending in (a, b)
    edges = np.stack([code // span, code % span], 1)
    reverse = edges[:, 1] * span + edges[:, 0]
    at = np.searchsorted(code, reverse).clip(max=len(code) - 1)
    backward = np.where(code[at] == reverse, forward[at], 0)
    return edges, forward.astype(np.int64), backward.astype(np.int64)
