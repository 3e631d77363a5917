"""TSDF fusion of depth frames on the device: Open3D's UniformTSDFVolume (integrate, extract_point_cloud) for batches of volumes, and depth
images as clouds (the reference's convert_depth_mat_to_points, Open3D's create_from_depth_image), as HIP kernels (csrc/tsdf.hip with
csrc/tsdf_core.h) in place of a host sweep of the volume per frame.

  TSDFVolumes(num_volumes, resolution, voxel_length, sdf_trunc, origins=None, color=False, device=None)
        .tsdf, .weight (V, R, R, R) float32 and, with color, .color (V, 3, R, R, R) float32: plain device tensors, zeros at the start
        .integrate(depths, intrinsics, extrinsics, frame_counts=None, colors=None, depth_scale=1000.0, depth_trunc=3.0)
        .extract_point_clouds()      three lists, one entry per volume: points, normals (n, 3) float64, colours (n, 3) float64 or None
        .extract_triangle_meshes()   four lists: vertices (n, 3) float64, triangles (m, 3) int64, normals, colours or None
        .ray_cast(intrinsics, extrinsics, height, width, frame_counts=None, depth_min=0.1, depth_max=3.0, weight_threshold=1.0,
                  maps=('depth', 'color'))     a dict of device tensors: the model seen from F cameras (contract: ray casting)
  fuse_depth_frames(depths_list, intrinsics, extrinsics_list, resolution, voxel_length, sdf_trunc, ...)
        construct, integrate and extract for a list of fragments: (points_list, normals_list, colors_list or None)
  depth_to_points_clouds(depths, intrinsics, scaling_factor=1000.0, distance_limit=6.0, convention='reference')
        the list of (n, 3) float64 clouds of F depth images, on the device
  convert_depth_mat_to_points      one image, numpy in and out, under the reference's name and signature

The batched calls take GPU tensors only (there is no CPU path), any number of volumes, and chunk internally at the library's
SE3_PAIR_MAX_PAIRS volumes per launch.  What a call refuses is a ValueError raised before any launch: a resolution, an image size or an
sdf_trunc outside ops.TSDF_LIMITS, a non-finite extrinsic or intrinsic, frame_counts that do not sum to the frames given, colours for a
volume without colour (or none for one with).  Open3D is not a dependency: the contract below, restated from it, is the yardstick.

State.  A volume is R^3 voxels of length vl with its corner at origin o (float64).  Voxel [x, y, z] (Open3D's IndexOf) sits at
(x R + y) R + z: planar, z fastest.

Contract: integration (the kernel file carries the same text).  All float32, every operation rounded on its own (no contraction; `/` and
sqrt rounded to nearest).  A volume takes its frames in ascending order.  For voxel (x, y, z) and one frame with extrinsic E (world to
camera, rounded to float32), intrinsics (fx, fy, cx, cy) as float32, an image of H x W:
  1. World position: w_a = f32((vl / 2 + vl i_a) + o_a), evaluated in float64 with that one final rounding.
  2. Camera position: c_a = ((E[a][0] w_x + E[a][1] w_y) + E[a][2] w_z) + E[a][3], evaluated directly for every voxel, never
     incrementally along z.  The frame is skipped unless c_z > 0.
  3. Pixel: u_f = ((c_x fx) / c_z + cx) + 0.5f, v_f likewise with fy, cy.  Skipped unless u_f >= 0.0001f, u_f < f32(W) - 0.0001f and the
     same for v_f with H.  u = (int)u_f, v = (int)v_f.
  4. Depth: d = f32(raw) / f32(depth_scale); d >= f32(depth_trunc) makes d = 0; skipped unless d > 0 (a NaN is skipped this way).
  5. Signed distance: m = sqrtf((xr xr + yr yr) + 1) with xr = (f32(u) - cx) / fx, yr = (f32(v) - cy) / fy; sdf = (d - c_z) m; skipped
     unless sdf > -trunc, trunc = f32(sdf_trunc).
  6. Truncation: t = min(1, sdf (1f / trunc)).
  7. Update: tsdf = (tsdf w + t) / (w + 1); each colour channel likewise with its pixel's value, a uint8 colour loaded as
     f32(c) / 255f, a float32 colour as it is; then w = w + 1.

Contract: extraction.  All float64.  Output order is ascending (x, y, z, axis), Open3D's loop order.
  1. A voxel is usable iff w != 0, t < 0.98f and t >= -0.98f (float32 tests).
  2. For x, y, z in [1, R - 1) and each axis i with idx_i + 1 < R - 1: a point is emitted when the voxel and its neighbour at idx + e_i
     are both usable and their tsdf values f0, f1 are non-zero with opposite signs.
  3. p0_a = vl / 2 + vl idx_a, p1_i = p0_i + vl, r0 = |f0|, r1 = |f1|, p_i = ((p0_i r1) + (p1_i r0)) / (r0 + r1), p_a = p0_a on the other
     two axes.  The returned point is p + origin.  A colour channel is ((c0 r1) + (c1 r0)) / (r0 + r1).
  4. Normal: n_i = T(p + h e_i) - T(p - h e_i), h = 0.99 vl, p without the origin.  T(q): g_a = q_a / vl - 0.5, i_a = floor(g_a),
     r_a = g_a - i_a, s_a = 1 - r_a, f[dx][dy][dz] the stored tsdf of voxel (i_x + dx, i_y + dy, i_z + dz), and
       T = s_x (s_y (s_z f000 + r_z f001) + r_y (s_z f010 + r_z f011)) + r_x (s_y (s_z f100 + r_z f101) + r_y (s_z f110 + r_z f111)),
     every product and sum rounded on its own.  T reads the stored tsdf of every voxel, observed or not (an unobserved one holds 0:
     Open3D's quirk).  n is divided by sqrt((n_x^2 + n_y^2) + n_z^2) when that is positive and returned as it is otherwise.  The reads
     are inside the volume by construction: p_a / vl - 0.5 is in [1, R - 2], so g_a is in [0.01, R - 1.01] and floor(g_a) in [0, R - 2].

Contract: triangle meshes (csrc/tsdf_mesh.hip carries the same text, and the rule of its triangle table).  All float64.
  1. Cubes have their min corner (x, y, z) in [1, R - 3]^3, the range in which every cube edge satisfies the stencil argument of item 4
     above.  A cube is taken iff all eight corner weights are != 0 (there is no 0.98 test); a corner is negative iff t < 0, so an exact
     zero is positive; the cube index has bit i set iff corner i is negative, and indices 0 and 255 emit nothing.
  2. A vertex exists for the edge (owning voxel, axis) iff the edge changes sign and at least one taken cube contains it, so every vertex is
     referenced.  Its point, normal and colour are those of extraction items 3 and 4, bit for bit the row that extract_point_clouds emits
     for the same edge where both exist.
  3. Vertices are numbered in ascending (x, y, z, axis) of the owner; triangles come in ascending (x, y, z) of the cube, then in table
     order, as int64 triples of the volume's own vertex numbers, wound so that the right-hand normal points to the positive side.

Contract: ray casting (csrc/tsdf_raycast.hip carries the same text; SparseTSDFVolumes.ray_cast follows it with its own item 3).  All float64,
every operation rounded on its own, unless said otherwise.  A view has an extrinsic E (world to camera), its inverse P computed on the
host in float64 (tsdf_sparse.camera_poses) and intrinsics (fx, fy, cx, cy).
  1. Ray.  For pixel (u, v): xr = (u - cx) / fx, yr = (v - cy) / fy, dir_a = (P[a][0] xr + P[a][1] yr) + P[a][2], e_a = P[a][3] - o_a,
     q_a(s) = e_a + s dir_a: s is camera depth.  m = sqrt((xr xr + yr yr) + 1) turns a Euclidean step into a step of s.
  2. Interval.  Starting from [depth_min, depth_max], each axis intersects the interval with the ray's stay in the slab
     [1.5 vl, (R - 1.5) vl], both ends computed once as 1.5 vl and (f64(R) - 1.5) vl: t = (end - e_a) / dir_a for both ends, the smaller
     raises the lower end, the larger lowers the upper end.  An axis with dir_a == 0 divides nothing: it leaves the interval alone when
     e_a lies in the slab and empties it otherwise.  An empty interval is no hit.  A sample is read only where the three computed q_a
     themselves lie in the slab (a slab end that rounding moved by an ulp may not: it is an unobserved sample).  For such a q,
     q_a / vl - 0.5 is in [1, R - 2] up to a rounding: the nearest voxel floor(q_a / vl) is in [1, R - 2], T's floor in [0, R - 2] with a
     far corner of at most R - 1, and the normal's g_a -+ 0.99 in [0.01, R - 1.01] up to 2^-40: extraction item 4's argument.  The refined
     s* lies in [s0, s1] (item 5) and q_a(s) is monotone in s as computed, so q(s*) lies between two tested points and is in the slab too.
  3. (Sparse volumes: see se3et_amd/tsdf_sparse.py.)
  4. March.  s starts at the interval's lower end.  The sample at s is the nearest voxel's stored (f, w); it is observed iff
     w >= f32(weight_threshold).  Observed: s advances by max(vl, f64(f) sdf_trunc) / m.  Unobserved: by vl / m.  A crossing is an
     observed sample with f <= 0 whose predecessor on the ray was observed with f > 0: a ray that starts on the negative side has no hit
     until it has seen a positive observed sample, and no crossing is taken across an unobserved sample.  Marching ends at the first
     crossing or when s passes the upper end.  Every step advances s by vl / m at least, so a ray takes at most (hi - lo) / (vl / m) + 1
     samples, and the loop counts them against that number + 1.  (depth_max - depth_min) / vl is at most ops.RAYCAST_LIMITS['max_steps'].
  5. Refinement.  At the crossing between s0 and s1: F0 = T(q(s0)), F1 = T(q(s1)) (extraction item 4's T: stored values, observed or
     not).  If F0 > 0 and F1 <= 0 those are used, otherwise the two nearest-voxel values.  s* = ((s1 F0) - (s0 F1)) / (F0 - F1), then
     limited to [s0, s1], which only rounding can leave.
  6. Outputs at s*: depth = f32(s*); point = q(s*) + o; normal = extraction item 4 at q(s*), which points to the positive side, towards
     the camera; a colour channel is T's sum over that colour plane with T's weights, rounded once to float32.  A pixel without a hit
     holds depth 0, a NaN point and normal, colour 0 and mask False.
  7. Determinism.  No atomics, every pixel independent: a view is bit-identical alone, anywhere in a batch, across chunks, run to run.
ray_cast refuses, as a ValueError before any launch: an image side outside [1, max_image]; depth_min not positive or depth_max <= depth_min;
(depth_max - depth_min) / vl above max_steps; a non-finite intrinsic or a focal length of 0; an extrinsic that camera_poses cannot invert;
counts that do not sum to the views; an unknown or repeated map name; 'color' of volumes made without colour.

Contract: depth images as clouds.  All float64, output in row-major pixel order.  z = raw / scaling_factor; z > distance_limit makes z = 0;
x = ((u - cx) z) / fx, y = ((v - cy) z) / fy.
  'reference'   the reference function, quirks included: v = (row W + u) / W, a true quotient, so the row is fractional; a pixel is kept
                iff raw > 0, so one beyond the limit stays as a (0, 0, 0) row.
  'open3d'      v = row; a pixel is kept iff raw > 0 and not z > distance_limit (create_from_depth_image with an identity extrinsic).

Departures from Open3D.  The surface test of extraction item 2 is a sign test, not the float product f0 f1 < 0 (which underflows to 0 for
two tiny values).  Colours are stored in [0, 1] (Open3D stores 0 .. 255 and divides on extraction).  Weights have no cap.  Depth is
converted per gather, never as a float image; create_from_depth_image's float32 depth image is float64 arithmetic here.  With float32
depth the reference convention divides in float64 (numpy would divide a float32 array in float32).  The mesh leaves out the outer shell
of cubes that Open3D walks, numbers its vertices by position where Open3D numbers them in the order of first use, and resolves an ambiguous
cube face by separating the negative corners, which may not be Open3D's choice.  Ray casting (Open3D's VoxelBlockGrid.ray_cast) has no range
map: every ray marches from depth_min; its step is Euclidean (Open3D advances the ray parameter by the sdf itself); refinement interpolates
the trilinear field, not the two samples; a uniform volume is cast inside its inner box only; observed is a threshold on the stored weight;
colours are in [0, 1].

Determinism.  Every voxel is independent and there are no atomics: a volume's state and clouds are bit-identical alone, anywhere in a
batch, from run to run, and whether its frames arrive in one integrate call or split over several."""
import numpy as np
import torch

from . import ops as _ops
from .stacking import as_tensor, chunks, device_of, exclusive_offsets, to_device, transforms_of

_FAMILY = 'TSDF fusion'
_LIMITS = _ops.TSDF_LIMITS
_DEPTH_DTYPES = (torch.uint16, torch.float32)
_COLOR_DTYPES = (torch.uint8, torch.float32)


def _positive(what, name, value):
    v = float(value)
    if not (np.isfinite(v) and v > 0):
        raise ValueError('%s: %s %r is not a positive finite number' % (what, name, value))
    return v


def _volume_args(what, resolution, voxel_length, sdf_trunc):
    if int(resolution) != resolution or not _LIMITS['min_resolution'] <= int(resolution) <= _LIMITS['max_resolution']:
        raise ValueError('%s: resolution %r is not an integer in [%d, %d]' % (what, resolution, _LIMITS['min_resolution'],
                                                                             _LIMITS['max_resolution']))
    vl = _positive(what, 'voxel_length', voxel_length)
    trunc = float(sdf_trunc)
    if not (np.isfinite(trunc) and trunc > 0 and trunc <= _LIMITS['max_trunc_voxels'] * vl and np.float32(trunc) > 0):
        raise ValueError('%s: sdf_trunc %r is not in (0, %d voxel lengths]' % (what, sdf_trunc, _LIMITS['max_trunc_voxels']))
    return int(resolution), vl, trunc


def _images(what, x, name, dtypes, tail=()):
    """x, contiguous, if it is a tensor (F, H, W) + tail of one of dtypes with sides inside the limits (where it lives: _gpu_only)."""
    if not torch.is_tensor(x) or x.dtype not in dtypes or x.dim() != 3 + len(tail) or tuple(x.shape[3:]) != tuple(tail):
        raise RuntimeError('%s: %s must be a tensor %s %s, got %s' % (what, name, ('F', 'H', 'W') + tuple(tail), ' or '.join(str(d)[6:] for d in dtypes),
                                                                      '%s %s' % (tuple(x.shape), x.dtype) if torch.is_tensor(x) else type(x).__name__))
    H, W = int(x.shape[1]), int(x.shape[2])
    if not (1 <= H <= _LIMITS['max_image'] and 1 <= W <= _LIMITS['max_image']):
        raise ValueError('%s: %s of %d x %d: each side must lie in [1, %d]' % (what, name, H, W, _LIMITS['max_image']))
    return x.contiguous()


def _join(what, images, stack=False):
    """The images of a list in one tensor (cat along the frames, or stack of single images).  uint16 is joined through its int16 bits,
    which every device supports."""
    images = list(images)
    if not all(torch.is_tensor(x) for x in images) or len({(x.dtype, x.device) for x in images}) > 1:
        raise RuntimeError('%s: the images of a list must be tensors of one dtype on one device' % what)
    bits = images[0].dtype == torch.uint16
    joined = (torch.stack if stack else torch.cat)([x.view(torch.int16) if bits else x for x in images], 0)
    return joined.view(torch.uint16) if bits else joined


def _gpu_only(what, dev, **tensors):
    """The last check before a launch, after every ValueError: the state and the images are on the one GPU."""
    for name, x in tensors.items():
        if x is None:
            continue
        if not x.is_cuda:
            raise RuntimeError('%s: %s must be a GPU tensor (%s has no CPU implementation)' % (what, name, _FAMILY))
        if x.device != dev and dev.index is not None:
            raise RuntimeError('%s: %s is on %s, the volumes on %s' % (what, name, x.device, dev))


def _intrinsics(what, intrinsics, F, dtype):
    """(F, 4) of dtype, where it is, from (4,), (F, 4), (3, 3) or (F, 3, 3): fx, fy, cx, cy.  The caller moves it to the device."""
    K = as_tensor(intrinsics).detach().to(torch.float64)
    if K.shape[-2:] == (3, 3):
        K = torch.stack([K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2]], -1)
    if K.dim() == 1 and K.shape[0] == 4:
        K = K.reshape(1, 4).expand(F, 4)
    if K.dim() != 2 or tuple(K.shape) != (F, 4):
        raise ValueError('%s: intrinsics must be (fx, fy, cx, cy) as (4,) or one row per frame (%d, 4), got %s' % (what, F, tuple(K.shape)))
    return K.to(dtype).contiguous()


def _ray_cast_args(what, V, dev, has_color, voxel_length, intrinsics, extrinsics, height, width, frame_counts, depth_min, depth_max, maps):
    """What ray_cast refuses, for both volume types.  Returns (views (F, 16) float64 on the device: the 3 x 4 camera pose by rows, then fx, fy,
    cx, cy; the volume of each view as a host list; the counts; the maps as a tuple; H; W)."""
    from .tsdf_sparse import camera_poses
    if int(height) != height or int(width) != width or not (1 <= int(height) <= _LIMITS['max_image'] and 1 <= int(width) <= _LIMITS['max_image']):
        raise ValueError('%s: an image of %r x %r: each side must be an integer in [1, %d]' % (what, height, width, _LIMITS['max_image']))
    lo, hi = float(depth_min), float(depth_max)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo > 0 and hi > lo):
        raise ValueError('%s: depth_min %r, depth_max %r: 0 < depth_min < depth_max expected' % (what, depth_min, depth_max))
    if not (hi - lo) / voxel_length <= _ops.RAYCAST_LIMITS['max_steps']:
        raise ValueError('%s: (depth_max - depth_min) / voxel_length is %g (at most %d)' % (what, (hi - lo) / voxel_length, _ops.RAYCAST_LIMITS['max_steps']))
    maps = (maps,) if isinstance(maps, str) else tuple(maps)
    if any(m not in _ops.RAYCAST_MAPS for m in maps) or len(set(maps)) != len(maps):
        raise ValueError('%s: maps %r must be distinct names among %s' % (what, maps, ', '.join(_ops.RAYCAST_MAPS)))
    if 'color' in maps and not has_color:
        raise ValueError("%s: the map 'color' of volumes made without colour" % what)
    if isinstance(extrinsics, (list, tuple)):
        extrinsics = [as_tensor(e).detach().cpu().to(torch.float64).reshape(4, 4) for e in extrinsics]
        extrinsics = torch.stack(extrinsics, 0) if extrinsics else torch.zeros((0, 4, 4), dtype=torch.float64)
    E = as_tensor(extrinsics).detach().to(torch.float64).reshape(-1, 4, 4)
    F = int(E.shape[0])
    if frame_counts is None:
        if V != 1:
            raise ValueError('%s: frame_counts is required for %d volumes' % (what, V))
        frame_counts = [F]
    counts = [int(n) for n in (frame_counts.tolist() if hasattr(frame_counts, 'tolist') else frame_counts)]
    if len(counts) != V or any(n < 0 for n in counts) or sum(counts) != F:
        raise ValueError('%s: frame_counts %r must be %d counts >= 0 that sum to the %d views given' % (what, counts, V, F))
    K = _intrinsics(what, intrinsics, F, torch.float64).cpu()
    if not bool(torch.isfinite(K).all()) or bool((K[:, :2] == 0).any()):
        raise ValueError('%s: an intrinsic is not finite, or a focal length is 0' % what)
    P = camera_poses(E, what)
    views = torch.cat([torch.from_numpy(P[:, :3, :].reshape(F, 12)), K], 1).contiguous().to(dev)
    return views, [v for v, n in enumerate(counts) for _ in range(n)], counts, maps, int(height), int(width)


class TSDFVolumes:
    """V uniform TSDF volumes of resolution^3 voxels on the device (the module docstring carries the contract).  The state is the plain
    tensors .tsdf, .weight and .color (None without colour); .origins is (V, 3) float64 on the device."""

    def __init__(self, num_volumes, resolution, voxel_length, sdf_trunc, origins=None, color=False, device=None):
        what = 'TSDFVolumes'
        if int(num_volumes) != num_volumes or int(num_volumes) < 0:
            raise ValueError('%s: num_volumes %r is not an integer >= 0' % (what, num_volumes))
        V = int(num_volumes)
        R, self.voxel_length, self.sdf_trunc = _volume_args(what, resolution, voxel_length, sdf_trunc)
        dev = device_of(device, [origins] if torch.is_tensor(origins) else [])
        o = torch.zeros((V, 3), dtype=torch.float64) if origins is None else as_tensor(origins).detach().to(torch.float64)
        if tuple(o.shape) != (V, 3) or not bool(torch.isfinite(o).all()):
            raise ValueError('%s: origins must be (%d, 3) finite numbers' % (what, V))
        self.num_volumes, self.resolution, self.device = V, R, dev
        self.origins = o.to(dev).contiguous()
        self.tsdf = torch.zeros((V, R, R, R), dtype=torch.float32, device=dev)
        self.weight = torch.zeros((V, R, R, R), dtype=torch.float32, device=dev)
        self.color = torch.zeros((V, 3, R, R, R), dtype=torch.float32, device=dev) if color else None

    @torch.no_grad()
    def integrate(self, depths, intrinsics, extrinsics, frame_counts=None, colors=None, depth_scale=1000.0, depth_trunc=3.0):
        """Integrate F frames: depths (F, H, W) uint16 or float32 on the device, intrinsics (4,) or (F, 4) (fx, fy, cx, cy), extrinsics
        (F, 4, 4) world to camera, frame_counts (V,) on the host: volume v takes the next frame_counts[v] frames, in order (default: all
        frames into volume 0 when V = 1), colors (F, H, W, 3) uint8 or float32 exactly for volumes with colour.  Integration continues
        from the stored state, so frames may arrive over several calls."""
        what = 'TSDFVolumes.integrate'
        V, dev = self.num_volumes, self.device
        d = _images(what, depths, 'depths', _DEPTH_DTYPES)
        F = int(d.shape[0])
        if (colors is not None) != (self.color is not None):
            raise ValueError('%s: colours are %s, but the volumes were made %s colour' % (what, 'given' if colors is not None else 'missing',
                                                                                         'with' if self.color is not None else 'without'))
        c = None
        if colors is not None:
            c = _images(what, colors, 'colors', _COLOR_DTYPES, (3,))
            if tuple(c.shape[:3]) != tuple(d.shape):
                raise ValueError('%s: colors %s do not match depths %s' % (what, tuple(c.shape), tuple(d.shape)))
        if frame_counts is None:
            if V != 1:
                raise ValueError('%s: frame_counts is required for %d volumes' % (what, V))
            frame_counts = [F]
        counts = [int(n) for n in (frame_counts.tolist() if hasattr(frame_counts, 'tolist') else frame_counts)]
        if len(counts) != V or any(n < 0 for n in counts) or sum(counts) != F:
            raise ValueError('%s: frame_counts %r must be %d counts >= 0 that sum to the %d frames given' % (what, counts, V, F))
        scale, far = _positive(what, 'depth_scale', depth_scale), _positive(what, 'depth_trunc', depth_trunc)
        E = transforms_of(extrinsics, F, what, dev)
        table = torch.cat([E[:, :3, :].reshape(F, 12).to(torch.float32), _intrinsics(what, intrinsics, F, torch.float32).to(dev)], 1).contiguous()
        if not bool(torch.isfinite(table).all()):
            raise ValueError('%s: an extrinsic or an intrinsic is not finite in float32' % what)
        _gpu_only(what, dev, volumes=self.tsdf, depths=d, colors=c)
        offsets = exclusive_offsets(counts)
        for a, b in chunks(V):
            f0, f1 = offsets[a], offsets[b]
            if f0 == f1:
                continue
            _ops.tsdf_integrate_stack(self.tsdf[a:b], self.weight[a:b], None if self.color is None else self.color[a:b], self.voxel_length,
                                      self.sdf_trunc, self.origins[a:b], d[f0:f1], table[f0:f1], counts[a:b], None if c is None else c[f0:f1],
                                      scale, far)
        return self

    @torch.no_grad()
    def extract_point_clouds(self):
        """(points_list, normals_list, colors_list): per volume (n, 3) float64 tensors on the device, colours None without colour.  The
        host reads the volumes' counts, nothing else."""
        points, normals, colors = [], [], []
        for a, b in chunks(self.num_volumes):
            p, n, c, counts = _ops.tsdf_extract_stack(self.tsdf[a:b], self.weight[a:b], None if self.color is None else self.color[a:b],
                                                      self.voxel_length, self.origins[a:b])
            points += list(torch.split(p, counts))
            normals += list(torch.split(n, counts))
            colors += list(torch.split(c, counts)) if c is not None else [None] * (b - a)
        return points, normals, colors

    @torch.no_grad()
    def extract_triangle_meshes(self):
        """(vertices_list, triangles_list, normals_list, colors_list): per volume (n, 3) float64 vertices, normals and colours (None without
        colour) and (m, 3) int64 triangles that index the volume's own vertices, on the device.  The host reads the volumes' counts,
        nothing else."""
        vertices, triangles, normals, colors = [], [], [], []
        for a, b in chunks(self.num_volumes):
            v, t, n, c, nv, nt = _ops.tsdf_mesh_stack(self.tsdf[a:b], self.weight[a:b], None if self.color is None else self.color[a:b],
                                                      self.voxel_length, self.origins[a:b])
            vertices += list(torch.split(v, nv))
            triangles += list(torch.split(t, nt))
            normals += list(torch.split(n, nv))
            colors += list(torch.split(c, nv)) if c is not None else [None] * (b - a)
        return vertices, triangles, normals, colors

    @torch.no_grad()
    def ray_cast(self, intrinsics, extrinsics, height, width, frame_counts=None, depth_min=0.1, depth_max=3.0, weight_threshold=1.0,
                 maps=('depth', 'color')):
        """The volumes seen from F cameras (contract: ray casting): extrinsics (F, 4, 4) world to camera, intrinsics as in integrate,
        frame_counts (V,) on the host: volume v renders the next frame_counts[v] views (default: all views of volume 0 when V = 1; zero
        views for a volume is fine).  Returns a dict of device tensors for the names in maps: 'depth' (F, H, W) float32, camera z in metres;
        'points' (F, H, W, 3) float64, world coordinates; 'normals' (F, H, W, 3) float64, unit, towards the positive side; 'color'
        (F, H, W, 3) float32 in [0, 1]; 'mask' (F, H, W) bool.  A pixel without a hit holds 0, NaN, NaN, 0 and False.  Nothing is read back."""
        what = 'TSDFVolumes.ray_cast'
        V, dev = self.num_volumes, self.device
        views, volume_of, counts, maps, H, W = _ray_cast_args(what, V, dev, self.color is not None, self.voxel_length, intrinsics, extrinsics, height,
                                                              width, frame_counts, depth_min, depth_max, maps)
        _gpu_only(what, dev, volumes=self.tsdf)
        out = _ops.raycast_outputs(maps, len(volume_of), H, W, dev)
        offsets = exclusive_offsets(counts)
        for a, b in chunks(V):
            f0, f1 = offsets[a], offsets[b]
            if f0 == f1:
                continue
            _ops.tsdf_raycast_stack(self.tsdf[a:b], self.weight[a:b], None if self.color is None else self.color[a:b], self.voxel_length,
                                    self.sdf_trunc, self.origins[a:b], views[f0:f1], to_device([v - a for v in volume_of[f0:f1]], torch.int32, dev),
                                    {name: x[f0:f1] for name, x in out.items()}, H, W, depth_min, depth_max, weight_threshold)
        return out


@torch.no_grad()
def fuse_depth_frames(depths_list, intrinsics, extrinsics_list, resolution, voxel_length, sdf_trunc, origins=None, colors_list=None,
                      depth_scale=1000.0, depth_trunc=3.0, device=None, mesh=False):
    """One TSDF volume per fragment: construct, integrate and extract in one call.  depths_list: per fragment (F_i, H, W) uint16 or float32
    on the device, all of one image size and dtype; extrinsics_list: per fragment (F_i, 4, 4) world to camera; intrinsics: (4,) for all
    frames or a list of (4,) / (F_i, 4) per fragment; colors_list: per fragment (F_i, H, W, 3), or None.  Returns (points_list,
    normals_list, colors_list or None): (n, 3) float64 tensors on the device, what voxel_downsample_clouds and global_registration_pairs
    take.  mesh=True: (vertices_list, triangles_list, normals_list, colors_list or None) of extract_triangle_meshes instead."""
    what = 'fuse_depth_frames'
    V = len(depths_list)
    if len(extrinsics_list) != V or (colors_list is not None and len(colors_list) != V):
        raise ValueError('%s: one entry per fragment expected in every list (%d fragments)' % (what, V))
    dev = device_of(device, depths_list)
    volumes = TSDFVolumes(V, resolution, voxel_length, sdf_trunc, origins, colors_list is not None, dev)
    if V:
        counts = [int(d.shape[0]) for d in depths_list]
        if isinstance(intrinsics, (list, tuple)) and len(intrinsics) == V and not np.isscalar(intrinsics[0]):
            K = torch.cat([_intrinsics(what, k, n, torch.float64).to(dev) for k, n in zip(intrinsics, counts)], 0)
        else:
            K = intrinsics
        E = torch.cat([transforms_of(e, n, what, dev) for e, n in zip(extrinsics_list, counts)], 0)
        volumes.integrate(_join(what, depths_list), K, E, counts, None if colors_list is None else _join(what, colors_list),
                          depth_scale, depth_trunc)
    if mesh:
        vertices, triangles, normals, colors = volumes.extract_triangle_meshes()
        return vertices, triangles, normals, colors if colors_list is not None else None
    points, normals, colors = volumes.extract_point_clouds()
    return points, normals, colors if colors_list is not None else None


@torch.no_grad()
def depth_to_points_clouds(depths, intrinsics, scaling_factor=1000.0, distance_limit=6.0, convention='reference', device=None):
    """The clouds of F depth images: depths (F, H, W) uint16 or float32 on the device (or a list of (H, W) images of one size), intrinsics
    (4,), (F, 4), (3, 3) or (F, 3, 3).  Returns the list of (n, 3) float64 tensors on the device, rows in row-major pixel order.
    convention 'reference' reproduces convert_depth_mat_to_points, 'open3d' create_from_depth_image (the module docstring has both)."""
    what = 'depth_to_points_clouds'
    if convention not in _ops.DEPTH_CONVENTIONS:
        raise ValueError('%s: convention %r is not one of %s' % (what, convention, ', '.join(sorted(_ops.DEPTH_CONVENTIONS))))
    if isinstance(depths, (list, tuple)):
        depths = _join(what, depths, True) if len(depths) else torch.zeros((0, 1, 1), dtype=torch.float32, device=device_of(device))
    dev = device_of(device, [depths])
    d = _images(what, depths, 'depths', _DEPTH_DTYPES)
    scale = _positive(what, 'scaling_factor', scaling_factor)
    if np.isnan(float(distance_limit)):
        raise ValueError('%s: distance_limit is not a number' % what)
    K = _intrinsics(what, intrinsics, int(d.shape[0]), torch.float64)
    if not bool(torch.isfinite(K).all()):
        raise ValueError('%s: an intrinsic is not finite' % what)
    _gpu_only(what, dev, depths=d)
    points, counts = _ops.depth_points_stack(d, K.to(d.device), scale, float(distance_limit), convention)
    return list(torch.split(points, counts))


def convert_depth_mat_to_points(depth_mat, intrinsics, scaling_factor=1000.0, distance_limit=6.0, device=None):
    """The reference's convert_depth_mat_to_points on one image, numpy in and out: depth_mat (H, W) (uint16 stays, anything else becomes
    float32), intrinsics (3, 3); returns (n, 3) float64."""
    depth = np.asarray(depth_mat)
    depth = np.ascontiguousarray(depth if depth.dtype == np.uint16 else depth.astype(np.float32))
    d = torch.from_numpy(depth).to(device or 'cuda')[None]
    return depth_to_points_clouds(d, np.asarray(intrinsics, dtype=np.float64), scaling_factor, distance_limit, 'reference')[0].cpu().numpy()
