"""RGB-D odometry on the device: Open3D's legacy compute_rgbd_odometry (Odometry.cpp, hybrid and colour Jacobians, with
CreateInformationMatrix) for batches of frame pairs, and the recipe of its make_fragments.py on top of it -- the stage in front of
tsdf.fuse_depth_frames and pose_graph.optimize_pose_graphs, which take camera poses and odometry edges as given
(csrc/rgbd_odometry.hip with csrc/rgbd_odometry_core.h).

  rgbd_odometry_pairs(depths, colors, intrinsics, pairs=None, init_transforms=None, method='hybrid', iterations=(20, 10, 5), ...)
        dict of device tensors for P pairs of the F frames: transforms (P, 4, 4) float64 (source camera -> target camera), success (P,)
        bool, status (P,) int32 (ops.RGBD_STATUS bits), information (P, 6, 6) float64, correspondences (P,) int64
  compute_rgbd_odometry(source_color, source_depth, target_color, target_depth, intrinsics, odo_init=None, ...)
        one pair, numpy in and out: (success, transform, information), Open3D's order
  make_fragments_rgbd(depths_list, colors_list, intrinsics, resolution, voxel_length, sdf_trunc, keyframe_stride=5, ...)
        odometry, loop closures, one pose graph and one TSDF volume per fragment: points, normals, colours and poses

Frames are the unit of preparation: a frame used by several pairs is converted, filtered and given its pyramid once per call, whatever
the number of pairs and of chunks (for the default pairs (i, i + 1) that is half the work and half the memory of per-pair copies).  The
batched call takes GPU tensors only (there is no CPU path), any number of pairs, and chunks at the library's SE3_PAIR_MAX_PAIRS pairs per
C call; a C call issues the whole schedule (3 launches per iteration) on the current stream and nothing is read back.  What a call
refuses is a ValueError raised before any launch.  pairs and intrinsics are host values; a pair's two frames must share their intrinsics.
Open3D is not a dependency: the contract below, restated from it, is the yardstick.

Contract: preparation, per frame.  All float32, every operation rounded on its own.
  1. Depth: d = f32(raw) / f32(depth_scale); d > f32(depth_trunc) makes d = 0; then d <= f32(min_depth), d > f32(max_depth) and a
     non-finite d become NaN.
  2. Intensity: uint8 RGB ((0.2990f R + 0.5870f G) + 0.1140f B) / 255f; uint8 grey c / 255f; float32 alike without the division.
  3. Both images pass Gaussian3: h(x, y) = (0.25f a + 0.5f b) + 0.25f c over in(x - 1, y), in(x, y), in(x + 1, y), then the same taps over
     h(x, y - 1), h(x, y), h(x, y + 1); coordinates are clamped to the image.  A NaN depth spreads to its neighbours (Open3D's behaviour).
  4. Level l + 1 of floor(H / 2) x floor(W / 2): intensity is Gaussian3 of level l, then ((a + b) + (c + d)) 0.25f over the block
     a = (2x, 2y), b = (2x + 1, 2y), c = (2x, 2y + 1), d = (2x + 1, 2y + 1); depth is that mean alone.  Intrinsics of level l: all four
     values times 2^-l.
  5. Sobel images of intensity and depth, per level, of every frame that is some pair's target: e(x, y) = in(x + 1, y) - in(x - 1, y),
     s(x, y) = (in(x - 1, y) + 2f in(x, y)) + in(x + 1, y), dx = (e(x, y - 1) + 2f e(x, y)) + e(x, y + 1), dy = s(x, y + 1) - s(x, y - 1),
     clamped coordinates.  The factor 0.125 is applied where a gradient is used; a NaN depth gradient counts as 0 there.

Contract: correspondences of a pair at level l under T = (R, t).  All float64.
  1. M = K (R K^-1) and K t in this operation order: A = R K^-1 with A[a][0] = R[a][0] (1 / fx), A[a][1] = R[a][1] (1 / fy),
     A[a][2] = (R[a][0] (-(cx / fx)) + R[a][1] (-(cy / fy))) + R[a][2]; M[0][b] = fx A[0][b] + cx A[2][b], M[1][b] = fy A[1][b] + cy A[2][b],
     M[2][b] = A[2][b]; K t = (fx t_x + cx t_z, fy t_y + cy t_z, t_z).
  2. For source pixel (u, v), index s = v W + u, with non-NaN depth d: q_a = d ((M[a][0] u + M[a][1] v) + M[a][2]) + (K t)_a.  Skipped unless
     q_z > 0.  u_t = floor(q_x / q_z + 0.5), v_t likewise; skipped when outside the image, when the target depth d_t there is NaN, or when
     |q_z - d_t| > max_depth_diff.
  3. A target pixel claimed by several source pixels keeps the one with the smallest hi32(q_z), the high 32 bits of q_z's float64 pattern
     (q_z cut to 20 mantissa bits), then the smallest s.

Contract: intensity normalisation of a pair.  Over the correspondences at level 0 under the initial transform: a_s = 0.5 / (sum I_s / n),
a_t = 0.5 / (sum I_t / n); n = 0 fails the pair (status empty).  The factors multiply intensities and intensity gradients where read.

Contract: one iteration.  For a correspondence (s, j): d the source depth, p = (d xr, d yr, d) with xr = (u - cx) / fx, yr = (v - cy) / fy;
(x, y, z)_a = ((R[a][0] p_x + R[a][1] p_y) + R[a][2] p_z) + t_a.  For a gradient g: c0 = (g_x fx) / z, c1 = (g_y fy) / z,
c2 = -((c0 x + c1 y) / z), row(g) = (y c2 - z c1, z c0 - x c2, x c1 - y c0, c0, c1, c2).
  colour row   J = w_I row(a_t (0.125 S_I)),  r = w_I ((a_t I_t) - (a_s I_s))
  depth row    J = w_D (row(0.125 S_D) + (-y, x, 0, 0, 0, -1)),  r = w_D (D_t - z)                      (method 'hybrid' alone)
  'hybrid': w_D = sqrt(0.95), w_I = sqrt(0.05); 'color': w_I = 1.  The 29 sums: the upper triangle of J^T J by rows, J^T r, r^2, the count.
  (J^T J) x = -J^T r by ICP's Cholesky solve with its pivot test; T <- M(x) T, M(x) = [Rz(x_2) Ry(x_1) Rx(x_0) | x_3..5] with ICP's sine
  and cosine.  A pair fails and stays frozen on a non-finite sum (nonfinite), fewer than 6 correspondences (too_few), a refused pivot
  (singular) or a rotation component of 1 rad or more (step_refused).  A failed pair returns success False, the identity, a zero
  information matrix and 0 correspondences, as Open3D returns the identity.  Every iteration runs: there is no convergence test.

Contract: information matrix.  Over the correspondences at level 0 under the final transform, with p = d_t (xr, yr, 1) of the TARGET
pixel: the sum of G^T G, G = [[0, p_z, -p_y, 1, 0, 0], [-p_z, 0, p_x, 0, 1, 0], [p_y, -p_x, 0, 0, 0, 1]].  `correspondences` is their count.

Sums.  Target pixels are cut into chunks of ops.RGBD_LIMITS['chunk'] in index order; a chunk is summed in the order of ICP's sums (lane l
of 256 adds pixels l, l + 256, .. ascending, then the halving tree), and a pair's chunk partials are folded in the same order over the
chunks: the order depends on the level's image size alone.

Departures from Open3D.
  - The tie rule of correspondences item 3 (Open3D's result under ties depends on its thread merge order), and its 20-bit q_z.
  - The intensity factors are applied where intensities are read; Open3D scales the images before it builds the pyramids (equal up to
    rounding).  Unscaled per-frame pyramids are what lets pairs share frames.
  - Sine and cosine are the library's series; the solve is ICP's Cholesky with a pivot test and a step limit, which Open3D has not.
  - depth_trunc of the RGBD image and min_depth / max_depth of the option are one conversion.
  - make_fragments_rgbd initialises its loop closures from the chained odometry poses; Open3D's make_fragments.py matches ORB features
    through OpenCV there.  The odometry pairs of all fragments are one rgbd_odometry_pairs call and the loop closures of all fragments a
    second one, because the second needs the first's poses.

Determinism.  The z-buffer is a 64-bit unsigned minimum, which does not depend on arrival order, and there are no float atomics: a
pair's result is bit-identical alone, anywhere in a batch, whether it shares frames with other pairs or not, and from run to run."""
import numpy as np
import torch

from . import ops as _ops
from .pose_graph import optimize_pose_graphs
from .stacking import chunks, device_of, exclusive_offsets, to_device, transforms_of
from .tsdf import _COLOR_DTYPES, _DEPTH_DTYPES, _gpu_only, _intrinsics, _join, _positive, fuse_depth_frames

_LIMITS = _ops.RGBD_LIMITS
_ODOMETRY_OPTIONS = ('method', 'iterations', 'depth_scale', 'depth_trunc', 'min_depth', 'max_depth', 'max_depth_diff')


def _frames(what, depths, colors, levels):
    """(depths, colors), contiguous, of F frames inside the limits: (F, H, W) uint16 / float32 and (F, H, W, 3) or (F, H, W) uint8 / float32."""
    if not torch.is_tensor(depths) or depths.dtype not in _DEPTH_DTYPES or depths.dim() != 3:
        raise RuntimeError('%s: depths must be a tensor (F, H, W) uint16 or float32' % what)
    if not torch.is_tensor(colors) or colors.dtype not in _COLOR_DTYPES or tuple(colors.shape) not in (tuple(depths.shape), tuple(depths.shape) + (3,)):
        raise RuntimeError('%s: colors must be a tensor %s or %s uint8 or float32' % (what, tuple(depths.shape) + (3,), tuple(depths.shape)))
    H, W = int(depths.shape[1]), int(depths.shape[2])
    if not (1 <= H <= _LIMITS['max_image'] and 1 <= W <= _LIMITS['max_image']):
        raise ValueError('%s: images of %d x %d: each side must lie in [1, %d]' % (what, H, W, _LIMITS['max_image']))
    if min(H, W) >> (levels - 1) < _LIMITS['min_side']:
        raise ValueError('%s: images of %d x %d leave a side below %d at the coarsest of %d levels' % (what, H, W, _LIMITS['min_side'], levels))
    return depths.contiguous(), colors.contiguous()


def _options(what, method, iterations, depth_scale, depth_trunc, min_depth, max_depth, max_depth_diff):
    if method not in _ops.RGBD_METHODS:
        raise ValueError('%s: method %r is not one of %s' % (what, method, ', '.join(sorted(_ops.RGBD_METHODS))))
    try:
        its = [int(n) for n in iterations]
        whole = all(int(n) == n for n in iterations)
    except (TypeError, ValueError):
        its, whole = [], False
    if not whole or not 1 <= len(its) <= _LIMITS['max_levels'] or any(not 0 <= n <= _LIMITS['max_iterations'] for n in its):
        raise ValueError('%s: iterations %r must be 1 to %d integers in [0, %d], coarsest level first' % (what, iterations, _LIMITS['max_levels'],
                                                                                                       _LIMITS['max_iterations']))
    scale, far = _positive(what, 'depth_scale', depth_scale), _positive(what, 'depth_trunc', depth_trunc)
    lo, hi, diff = float(min_depth), float(max_depth), float(max_depth_diff)
    if not (np.isfinite(lo) and lo >= 0 and np.isfinite(hi) and hi > lo):
        raise ValueError('%s: min_depth %r and max_depth %r must be finite with 0 <= min_depth < max_depth' % (what, min_depth, max_depth))
    if not (np.isfinite(diff) and diff >= 0):
        raise ValueError('%s: max_depth_diff %r is not a finite, non-negative number' % (what, max_depth_diff))
    return dict(method=method, iterations=its, depth_scale=scale, depth_trunc=far, min_depth=lo, max_depth=hi, max_depth_diff=diff)


def _host_intrinsics(what, intrinsics, F):
    """(F, 4) float64 numpy (fx, fy, cx, cy), finite with positive focal lengths (a device tensor is read)"""
    K = _intrinsics(what, intrinsics, F, torch.float64).cpu().numpy()
    if not (np.isfinite(K).all() and (K[:, :2] > 0).all()):
        raise ValueError('%s: the intrinsics must be finite with positive focal lengths' % what)
    return K


def _empty(dev, P=0):
    return dict(transforms=torch.empty((P, 4, 4), dtype=torch.float64, device=dev), success=torch.empty((P,), dtype=torch.bool, device=dev),
                status=torch.empty((P,), dtype=torch.int32, device=dev), information=torch.empty((P, 6, 6), dtype=torch.float64, device=dev),
                correspondences=torch.empty((P,), dtype=torch.int64, device=dev))


@torch.no_grad()
def rgbd_odometry_pairs(depths, colors, intrinsics, pairs=None, init_transforms=None, method='hybrid', iterations=(20, 10, 5),
                        depth_scale=1000.0, depth_trunc=3.0, min_depth=0.0, max_depth=4.0, max_depth_diff=0.03, return_information=True,
                        device=None):
    """RGB-D odometry of P pairs of F frames (the module text carries the contract).  depths (F, H, W) uint16 or float32 and colors
    (F, H, W, 3) or (F, H, W) uint8 or float32, GPU tensors; intrinsics (4,), (F, 4), (3, 3) or (F, 3, 3): fx, fy, cx, cy; pairs (P, 2) host
    ints (source frame, target frame), default every (i, i + 1); init_transforms: anything stacking.transforms_of takes, default
    identities; method 'hybrid' or 'color'; iterations: 1 to 4 entries, coarsest level first, their number the number of pyramid levels.
    Returns a dict of device tensors: transforms (P, 4, 4) float64 mapping source camera coordinates to target camera coordinates,
    success (P,) bool, status (P,) int32, information (P, 6, 6) float64 (None without return_information), correspondences (P,) int64."""
    what = 'rgbd_odometry_pairs'
    o = _options(what, method, iterations, depth_scale, depth_trunc, min_depth, max_depth, max_depth_diff)
    d, c = _frames(what, depths, colors, len(o['iterations']))
    F = int(d.shape[0])
    if pairs is None:
        table = [(i, i + 1) for i in range(F - 1)]
    else:
        host = pairs.detach().cpu().numpy() if torch.is_tensor(pairs) else np.asarray(pairs)
        if host.size and (host.ndim != 2 or host.shape[1] != 2 or not np.issubdtype(host.dtype, np.integer)):
            raise ValueError('%s: pairs must be (P, 2) integers (source frame, target frame), got %s %s' % (what, host.shape, host.dtype))
        table = [(int(s), int(t)) for s, t in host.reshape(-1, 2).tolist()]
    if any(not (0 <= s < F and 0 <= t < F) for s, t in table):
        raise ValueError('%s: a pair names a frame outside [0, %d)' % (what, F))
    P = len(table)
    K = _host_intrinsics(what, intrinsics, F)
    if any(not np.array_equal(K[s], K[t]) for s, t in table):
        raise ValueError('%s: the two frames of a pair must share their intrinsics' % what)
    dev = device_of(device, [d, c])
    T0 = transforms_of(init_transforms, P, what, dev)
    _gpu_only(what, dev, depths=d, colors=c)
    dev = d.device
    if c.device != dev:
        raise RuntimeError('%s: colors is on %s, depths on %s' % (what, c.device, dev))
    if P == 0:
        out = _empty(dev)
    else:
        flags = [0] * F
        for _s, t in table:
            flags[t] = 1
        flags = to_device(flags, torch.uint8, dev)
        workspace = _ops.rgbd_frames_workspace(d, len(o['iterations']))
        parts = [_ops.rgbd_odometry_stack(d, c, flags, workspace, a == 0, table[a:b], [K[s] for s, _t in table[a:b]], T0[a:b].contiguous(), **o)
                 for a, b in chunks(P)]
        out = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]} if len(parts) > 1 else parts[0]
    if not return_information:
        out['information'] = None
    return out


def compute_rgbd_odometry(source_color, source_depth, target_color, target_depth, intrinsics, odo_init=None, method='hybrid', device=None,
                          **options):
    """One pair, numpy in and out (the images are uploaded inside the call): (success, transform (4, 4) float64 mapping the source
    camera's coordinates to the target camera's, information (6, 6) float64), Open3D's order.  Depth: uint16 stays, anything else becomes
    float32; colour: uint8 stays, anything else becomes float32; options: those of rgbd_odometry_pairs."""
    def images(a, b, keep):
        a, b = np.asarray(a), np.asarray(b)
        kind = keep if a.dtype == keep and b.dtype == keep else np.float32
        return torch.from_numpy(np.ascontiguousarray(np.stack([a.astype(kind, copy=False), b.astype(kind, copy=False)]))).to(device or 'cuda')
    T0 = None if odo_init is None else np.asarray(odo_init, dtype=np.float64).reshape(1, 4, 4)
    out = rgbd_odometry_pairs(images(source_depth, target_depth, np.uint16), images(source_color, target_color, np.uint8),
                              np.asarray(intrinsics, dtype=np.float64), [(0, 1)], T0, method, **options)
    return bool(out['success'][0]), out['transforms'][0].cpu().numpy(), out['information'][0].cpu().numpy()


def _rigid_inverses(T):
    """(R^T, -R^T t) of (N, 4, 4) rigid device transforms: no factorisation, so nothing waits on the host."""
    out = torch.zeros_like(T)
    Rt = T[:, :3, :3].transpose(1, 2)
    out[:, :3, :3] = Rt
    out[:, :3, 3] = -(Rt @ T[:, :3, 3:4])[:, :, 0]
    out[:, 3, 3] = 1.0
    return out


@torch.no_grad()
def make_fragments_rgbd(depths_list, colors_list, intrinsics, resolution, voxel_length, sdf_trunc, keyframe_stride=5, origins=None,
                        device=None, **options):
    """The recipe of Open3D's make_fragments.py for V fragments.  depths_list / colors_list: per fragment (F_i, H, W) and (F_i, H, W, 3) or
    (F_i, H, W) GPU tensors, all of one image size and dtype; intrinsics: (4,) for all frames or a list of (4,) / (F_i, 4) per fragment.
    Per fragment: odometry edges (i, i + 1), certain, from the identity; loop-closure edges between frames that are both multiples of
    keyframe_stride (and no neighbours), uncertain, initialised from the chained odometry poses X_0 = I, X_(i+1) = X_i T_(i,i+1)^-1 (not
    from ORB features, as Open3D does); a failed pair gives no edge; optimize_pose_graphs with reference node 0, max_correspondence_distance
    = max_depth_diff and preference_loop_closure 0.1 (Open3D's value for fragments); fuse_depth_frames with the inverses of the optimised
    poses, colour passed through when the colours have three channels.  options: those of rgbd_odometry_pairs and of optimize_pose_graphs.
    The odometry pairs of all fragments are one rgbd_odometry_pairs call, the loop closures a second one; the host reads the pairs'
    success flags once, to leave the failed ones out.  Returns a dict: points, normals, colors (lists of (n, 3) float64 device tensors;
    colors None without three-channel colour), poses (list of (F_i, 4, 4): frame i's camera to the fragment's frame, that of its frame 0),
    edges (list of (E_i, 2) int64), uncertain (list of (E_i,) bool), status (V,) int32 of the pose graphs."""
    what = 'make_fragments_rgbd'
    V = len(depths_list)
    if len(colors_list) != V:
        raise ValueError('%s: one entry per fragment expected in every list (%d fragments)' % (what, V))
    stride = int(keyframe_stride)
    if stride != keyframe_stride or stride < 1:
        raise ValueError('%s: keyframe_stride %r is not an integer >= 1' % (what, keyframe_stride))
    odo = {k: options.pop(k) for k in _ODOMETRY_OPTIONS if k in options}
    counts = [int(d.shape[0]) for d in depths_list]
    for g, n in enumerate(counts):
        if n > _ops.PGO_MAX_NODES:
            raise ValueError('%s: fragment %d has %d frames (at most SE3_PGO_MAX_NODES = %d, the nodes of a pose graph)' % (what, g, n,
                                                                                                                           _ops.PGO_MAX_NODES))
    dev = device_of(device, depths_list)
    if V == 0 or sum(counts) == 0:
        points, normals, colors = fuse_depth_frames(depths_list, intrinsics, [torch.zeros((0, 4, 4), dtype=torch.float64, device=dev)] * V, resolution,
                                                    voxel_length, sdf_trunc, origins, device=dev)
        return dict(points=points, normals=normals, colors=colors, poses=[torch.zeros((0, 4, 4), dtype=torch.float64, device=dev)] * V,
                    edges=[torch.zeros((0, 2), dtype=torch.int64, device=dev)] * V, uncertain=[torch.zeros((0,), dtype=torch.bool, device=dev)] * V,
                    status=torch.zeros((V,), dtype=torch.int32, device=dev))
    d, c = _join(what, depths_list), _join(what, colors_list)
    if isinstance(intrinsics, (list, tuple)) and len(intrinsics) == V and not np.isscalar(intrinsics[0]):
        K = np.concatenate([_host_intrinsics(what, k, n) for k, n in zip(intrinsics, counts)], 0)
    else:
        K = _host_intrinsics(what, intrinsics, sum(counts))
    offsets = exclusive_offsets(counts)
    f64 = dict(dtype=torch.float64, device=d.device)
    # 1. odometry between neighbours, all fragments in one call
    steps = [(offsets[g] + i, offsets[g] + i + 1) for g in range(V) for i in range(counts[g] - 1)]
    first = rgbd_odometry_pairs(d, c, K, steps, None, **odo)
    # 2. the chained poses, on the device: X_0 = I, X_(i + 1) = X_i T_i^-1 (a failed pair returns the identity: X_(i + 1) = X_i)
    back = _rigid_inverses(first['transforms'])
    chained, k = [], 0
    for g in range(V):
        X = [torch.eye(4, **f64)]
        for _ in range(counts[g] - 1):
            X.append(X[-1] @ back[k])
            k += 1
        chained.append(torch.stack(X[:counts[g]]) if counts[g] else torch.zeros((0, 4, 4), **f64))
    # 3. loop closures between key frames, initialised from the chain: T_(s,t) = X_t^-1 X_s
    loops = [(g, s, t) for g in range(V) for s in range(0, counts[g], stride) for t in range(s + stride, counts[g], stride) if t - s > 1]
    if loops:
        init = torch.stack([_rigid_inverses(chained[g][t:t + 1])[0] @ chained[g][s] for g, s, t in loops])
        second = rgbd_odometry_pairs(d, c, K, [(offsets[g] + s, offsets[g] + t) for g, s, t in loops], init, **odo)
    else:
        second = _empty(d.device)
    ok = torch.cat([first['success'], second['success']]).cpu().tolist()             # (the one host read: which pairs became edges)
    rows = [(g, i, i + 1) for g in range(V) for i in range(counts[g] - 1)] + loops
    T = torch.cat([first['transforms'], second['transforms']])
    info = torch.cat([first['information'], second['information']])
    graphs = []
    for g in range(V):
        keep = [e for e, (h, _s, _t) in enumerate(rows) if h == g and ok[e]]
        idx = torch.tensor(keep, dtype=torch.int64, device=d.device)
        graphs.append(dict(poses=chained[g], edges=torch.tensor([rows[e][1:] for e in keep], dtype=torch.int64, device=d.device).reshape(-1, 2),
                           transforms=T[idx], informations=info[idx],
                           uncertain=torch.tensor([e >= len(steps) for e in keep], dtype=torch.uint8, device=d.device)))
    pgo = dict(max_correspondence_distance=float(odo.get('max_depth_diff', 0.03)), preference_loop_closure=0.1)
    pgo.update(options)
    solved = optimize_pose_graphs(graphs, [0 if n else -1 for n in counts], d.device, **pgo)
    # 4. one volume per fragment: the extrinsic of a frame is the inverse of its pose
    color = c.dim() == 4
    points, normals, colors = fuse_depth_frames(depths_list, [K[offsets[g]:offsets[g + 1]] for g in range(V)],
                                                [_rigid_inverses(X) for X in solved['poses']], resolution, voxel_length, sdf_trunc, origins,
                                                [x.contiguous() for x in colors_list] if color else None, odo.get('depth_scale', 1000.0),
                                                odo.get('depth_trunc', 3.0), d.device)
    return dict(points=points, normals=normals, colors=colors, poses=solved['poses'], edges=[g['edges'] for g in graphs],
                uncertain=[g['uncertain'].to(torch.bool) for g in graphs], status=solved['status'])
