"""Questions to a triangle mesh (Open3D's RaycastingScene) on the DEVICE, for lists of meshes as extract_triangle_meshes and mesh.py
return them (vertices (n, 3) float64, triangles (m, 3) int64; csrc/mesh_query.hip carries the contract): lists of GPU tensors in, one entry
per mesh, lists of GPU tensors out; longer lists are cut into calls of at most PAIR_MAX_PAIRS meshes.  A host tensor raises RuntimeError:
there is no CPU implementation.  A triangle that names a vertex outside [0, n), or has a vertex that is not finite, raises ValueError;
a triangle of zero area is passed over (MeshTrees.zero_area counts them).

  build_bvh_meshes(vertices_list, triangles_list)        the trees, built once and asked many times (a MeshTrees)
  cast_rays_meshes(trees, rays_list, t_min, t_max)        cast_rays: t_hit, primitive_ids, primitive_uvs, primitive_normals per mesh
  test_occlusions_meshes(trees, rays_list, t_min, t_max)  test_occlusions: a bool per ray, the walk ends at the first hit
  closest_points_meshes(trees, points_list)               compute_closest_points: points, distances, primitive_ids, _uvs, _normals
  distance_to_meshes(trees, points_list)                  compute_distance (unsigned)
  render_meshes(trees, views, view_meshes, height, width, depth_min, depth_max)     depth, points, normals, primitive_ids, mask as ray_cast()'s
  camera_views(intrinsics, extrinsics)                    the table of views that render_meshes and the TSDF ray caster take
  cloud_to_mesh_distances(points_list, vertices_list, triangles_list)               the recipe: build, ask, the distances per cloud
  cast_rays / compute_closest_points / compute_distance   one mesh, numpy in and out

The watertight ray test counts a ray through a shared edge or vertex as a hit of every triangle around it; among equal t (or equal
distances) the lowest triangle number wins.  Every output is bit-identical alone or in a batch, and from run to run, and equal to a brute
force over all triangles."""
import math

import numpy as np
import torch

from . import ops, stacking
from .mesh import _lists, _stacked

_FAMILY = 'mesh queries'


class MeshTrees:
    """The meshes of build_bvh_meshes in chunks of at most PAIR_MAX_PAIRS, each an ops.MeshBVH; .live and .zero_area count every mesh's
    triangles that are in its tree and that were passed over for a zero area."""

    def __init__(self, chunks, bounds):
        self.chunks, self.bounds = chunks, bounds
        self.num_meshes = bounds[-1][1] if bounds else 0
        self.live = [n for c in chunks for n in c.live]
        self.zero_area = [n for c in chunks for n in c.zero_area]
        self.device = chunks[0].meshes.device if chunks else None


def build_bvh_meshes(vertices_list, triangles_list):
    """The bounding volume hierarchies of the meshes (an LBVH over Morton keys of the centroids, built on the device)."""
    what = 'build_bvh_meshes'
    chunks, bounds = [], []
    for a, b in stacking.chunks(_lists(what, vertices_list, triangles_list)):
        S, _ = _stacked(what, vertices_list, triangles_list, a, b)
        chunks.append(ops.mesh_bvh_stack(S))
        bounds.append((a, b))
    return MeshTrees(chunks, bounds)


def _rows_per_chunk(what, trees, rows_list, cols, name):
    """for every chunk of the trees: (its BVH, the stacked rows of its meshes, their owners (rows,) int32, the counts per mesh)"""
    if not isinstance(trees, MeshTrees):
        raise RuntimeError('%s: the trees of build_bvh_meshes expected' % what)
    if len(rows_list) != trees.num_meshes:
        raise RuntimeError('%s: one entry of %s per mesh (%d meshes)' % (what, name, trees.num_meshes))
    for bvh, (a, b) in zip(trees.chunks, trees.bounds):
        dev = bvh.meshes.device
        rows = stacking.gpu_rows_each(rows_list[a:b], dev, '%s: %s' % (what, name), _FAMILY, cols=cols, dtypes=(torch.float64,))
        counts = stacking.lengths(rows)
        owners = torch.repeat_interleave(torch.arange(b - a, dtype=torch.int32, device=dev), stacking.to_device(counts, torch.int64, dev))
        yield bvh, stacking.stack(rows), owners, counts


def cast_rays_meshes(trees, rays_list, t_min=0.0, t_max=math.inf):
    """rays_list: per mesh (r, 6) float64 origin and direction (any length but zero).  Returns a dict of lists per mesh: 't_hit' (r,) float64
    in units of the direction's length, inf on a miss; 'primitive_ids' (r,) int64, -1; 'primitive_uvs' (r, 2), the weights of the
    triangle's second and third vertex; 'primitive_normals' (r, 3), the unit geometric normal."""
    out = {'t_hit': [], 'primitive_ids': [], 'primitive_uvs': [], 'primitive_normals': []}
    for bvh, rays, owners, counts in _rows_per_chunk('cast_rays_meshes', trees, rays_list, 6, 'rays'):
        got = ops.mesh_cast_rays_stack(bvh, rays, owners, t_min, t_max)
        for name in out:
            out[name] += list(torch.split(got[name], counts))
    return out


def test_occlusions_meshes(trees, rays_list, t_min=0.0, t_max=math.inf):
    """Per mesh (r,) bool: whether the ray meets the mesh with t in [t_min, t_max] (equal to cast_rays_meshes' t_hit < inf)."""
    out = []
    for bvh, rays, owners, counts in _rows_per_chunk('test_occlusions_meshes', trees, rays_list, 6, 'rays'):
        out += list(torch.split(ops.mesh_cast_rays_stack(bvh, rays, owners, t_min, t_max, any_hit=True), counts))
    return out


test_occlusions_meshes.__test__ = False          # (a name of Open3D's, not a test)


def closest_points_meshes(trees, points_list):
    """points_list: per mesh (q, 3) float64.  Returns a dict of lists per mesh: 'points' (q, 3), 'distances' (q,), 'primitive_ids' (q,) int64,
    'primitive_uvs' (q, 2), 'primitive_normals' (q, 3).  A mesh without a live triangle answers distance inf and primitive -1."""
    out = {'points': [], 'distances': [], 'primitive_ids': [], 'primitive_uvs': [], 'primitive_normals': []}
    for bvh, q, owners, counts in _rows_per_chunk('closest_points_meshes', trees, points_list, 3, 'points'):
        got = ops.mesh_closest_points_stack(bvh, q, owners)
        for name in out:
            out[name] += list(torch.split(got[name], counts))
    return out


def distance_to_meshes(trees, points_list):
    """Per mesh (q,) float64: the unsigned distance of every point to the mesh."""
    return closest_points_meshes(trees, points_list)['distances']


def camera_views(intrinsics, extrinsics, device=None):
    """(F, 16) float64 on the device: the camera-to-world pose (3 x 4 by rows) of every world-to-camera extrinsic (F, 4, 4), then fx, fy, cx,
    cy of intrinsics (4,), (F, 4), (3, 3) or (F, 3, 3): the views of render_meshes."""
    from .tsdf import _intrinsics
    from .tsdf_sparse import camera_poses
    what = 'camera_views'
    E = stacking.as_tensor(extrinsics).detach().cpu().to(torch.float64).reshape(-1, 4, 4)
    F = int(E.shape[0])
    K = _intrinsics(what, intrinsics, F, torch.float64).cpu()
    if not bool(torch.isfinite(K).all()) or bool((K[:, :2] == 0).any()):
        raise ValueError('%s: an intrinsic is not finite, or a focal length is 0' % what)
    P = camera_poses(E, what)
    return torch.cat([torch.from_numpy(P[:, :3, :].reshape(F, 12)), K], 1).contiguous().to(device or 'cuda')


def render_meshes(trees, views, view_meshes, height, width, depth_min=0.1, depth_max=3.0, maps=('depth', 'mask')):
    """The meshes seen from F cameras: views (F, 16) float64 on the device (camera_views), view_meshes: the mesh of every view (F ints on the
    host, not decreasing).  Returns a dict of device tensors for the names in maps, shaped as ray_cast()'s: 'depth' (F, H, W) float32, camera
    z; 'points' (F, H, W, 3) float64, world coordinates; 'normals' (F, H, W, 3) float64, the unit geometric normal of the triangle;
    'primitive_ids' (F, H, W) int64; 'mask' (F, H, W) bool.  A pixel without a hit holds 0, NaN, NaN, -1 and False."""
    what = 'render_meshes'
    if not isinstance(trees, MeshTrees):
        raise RuntimeError('%s: the trees of build_bvh_meshes expected' % what)
    maps = (maps,) if isinstance(maps, str) else tuple(maps)
    if any(m not in ops.MESH_RENDER_MAPS for m in maps) or len(set(maps)) != len(maps):
        raise ValueError('%s: maps %r must be distinct names among %s' % (what, maps, ', '.join(ops.MESH_RENDER_MAPS)))
    lo, hi = float(depth_min), float(depth_max)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo > 0 and hi > lo):
        raise ValueError('%s: depth_min %r, depth_max %r: 0 < depth_min < depth_max expected' % (what, depth_min, depth_max))
    owners = [int(v) for v in (view_meshes.tolist() if hasattr(view_meshes, 'tolist') else view_meshes)]
    if any(v < 0 or v >= trees.num_meshes for v in owners) or any(a > b for a, b in zip(owners[:-1], owners[1:])):
        raise ValueError('%s: view_meshes must name meshes in [0, %d) and not decrease' % (what, trees.num_meshes))
    if not torch.is_tensor(views) or not views.is_cuda:
        raise RuntimeError('%s: views must be a GPU tensor (%s has no CPU implementation)' % (what, _FAMILY))
    if views.dim() != 2 or views.shape[0] != len(owners):
        raise RuntimeError('%s: one row of views per entry of view_meshes' % what)
    dev = views.device
    H, W = int(height), int(width)
    out = ops.mesh_render_outputs(maps, len(owners), H, W, dev)
    for bvh, (a, b) in zip(trees.chunks, trees.bounds):
        f0, f1 = sum(v < a for v in owners), sum(v < b for v in owners)
        if f0 == f1:
            continue
        ops.mesh_render_stack(bvh, views[f0:f1], stacking.to_device([v - a for v in owners[f0:f1]], torch.int32, dev),
                              {name: x[f0:f1] for name, x in out.items()}, H, W, lo, hi)
    return out


def cloud_to_mesh_distances(points_list, vertices_list, triangles_list):
    """The accuracy figure of a reconstruction: per cloud (q,) float64, the unsigned distance of every point to the mesh of the same place
    in the lists."""
    return distance_to_meshes(build_bvh_meshes(vertices_list, triangles_list), points_list)


# ---- one mesh, numpy in and out -------------------------------------------------------------------------------------------------------------------
def _one(vertices, triangles, device):
    v = stacking.upload(np.array(vertices, dtype=np.float64), device)
    t = torch.from_numpy(np.array(triangles, dtype=np.int64).reshape(-1, 3)).to(v.device)
    return build_bvh_meshes([v], [t]), v.device


def cast_rays(vertices, triangles, rays, t_min=0.0, t_max=math.inf, device=None):
    """RaycastingScene.cast_rays for one mesh: rays (r, 6); a dict of numpy arrays t_hit, primitive_ids, primitive_uvs, primitive_normals."""
    trees, dev = _one(vertices, triangles, device)
    out = cast_rays_meshes(trees, [stacking.upload(np.array(rays, dtype=np.float64), dev, cols=6)], t_min, t_max)
    return {name: x[0].cpu().numpy() for name, x in out.items()}


def compute_closest_points(vertices, triangles, points, device=None):
    """RaycastingScene.compute_closest_points for one mesh: a dict of numpy arrays points, distances, primitive_ids, primitive_uvs,
    primitive_normals."""
    trees, dev = _one(vertices, triangles, device)
    out = closest_points_meshes(trees, [stacking.upload(np.array(points, dtype=np.float64), dev)])
    return {name: x[0].cpu().numpy() for name, x in out.items()}


def compute_distance(vertices, triangles, points, device=None):
    """RaycastingScene.compute_distance for one mesh: (q,) float64 numpy."""
    return compute_closest_points(vertices, triangles, points, device)['distances']
