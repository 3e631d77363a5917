"""Frame-to-model tracking on the device: each new RGB-D frame is registered against a rendering of the model fused so far, then fused
into it -- KinectFusion's loop, Open3D's dense SLAM (slam.Model: synthesize_model_frame, track_frame_to_model, integrate) -- for a batch
of scenes that advance in lockstep.  It composes the public stages and adds no kernel: ray_cast of se3et_amd/tsdf.py /
se3et_amd/tsdf_sparse.py (csrc/tsdf_raycast.hip), rgbd_odometry_pairs of se3et_amd/odometry.py, and the volumes' integrate.

  track_and_integrate_rgbd(depths_list, colors_list, intrinsics, voxel_length, sdf_trunc, init_poses=None, sparse=True, resolution=None,
                           origins=None, depth_scale=1000.0, depth_trunc=3.0, weight_threshold=1.0, stride=4, **odometry_options)
        (poses: list of (F_i, 4, 4) float64, camera to world; success: list of (F_i,) bool; the volumes object)

make_fragments_rgbd chains frame-to-frame odometry, so its drift grows with every frame until the pose graph repairs it; here every frame
is registered against the model, whose surface averages the frames before it."""
import numpy as np
import torch

from .odometry import _ODOMETRY_OPTIONS, _frames, _host_intrinsics, _options, _rigid_inverses, rgbd_odometry_pairs
from .stacking import device_of, transforms_of
from .tsdf import _COLOR_DTYPES, _DEPTH_DTYPES, _gpu_only, _join, _positive, TSDFVolumes
from .tsdf_sparse import SparseTSDFVolumes

_FAMILY = 'frame-to-model tracking'


def _metres(depths, depth_scale):
    """f32(raw) / f32(depth_scale): the one conversion of the source frames (integration item 4's quotient)"""
    raw = depths if depths.dtype == torch.float32 else depths.view(torch.int16).to(torch.int32).bitwise_and(0xffff).to(torch.float32)
    return raw / torch.tensor(depth_scale, dtype=torch.float32, device=depths.device)


def _unit_colors(colors):
    """uint8 colours as f32(c) / 255f (integration item 7's quotient), float32 colours as they are"""
    return colors if colors.dtype == torch.float32 else colors.to(torch.float32) / torch.tensor(255.0, dtype=torch.float32, device=colors.device)


@torch.no_grad()
def track_and_integrate_rgbd(depths_list, colors_list, intrinsics, voxel_length, sdf_trunc, init_poses=None, sparse=True, resolution=None,
                             origins=None, depth_scale=1000.0, depth_trunc=3.0, weight_threshold=1.0, stride=4, device=None, **odometry_options):
    """Track and fuse V scenes, one per list entry, in lockstep: step k handles frame k of every scene that still has one.  depths_list /
    colors_list: per scene (F_i, H, W) uint16 or float32 and (F_i, H, W, 3) uint8 or float32 GPU tensors, all of one image size and
    dtype; intrinsics: (4,) for all frames or a list of (4,) / (F_i, 4) per scene, the same for all frames of a scene; init_poses
    (V, 4, 4), camera to world, of each scene's frame 0 (default: identities); sparse: SparseTSDFVolumes with allocation stride `stride`, else TSDFVolumes of
    `resolution` at `origins`; odometry_options: those of rgbd_odometry_pairs but depth_scale (method, iterations, depth_trunc, min_depth, max_depth,
    max_depth_diff).
    Frame 0 of a scene is integrated at its initial pose.  At step k >= 1 every scene with a frame k renders its volume at its previous
    pose, ray_cast(maps=('depth', 'color'), depth_max=depth_trunc, weight_threshold=weight_threshold): one call for all scenes; one
    rgbd_odometry_pairs call registers the scenes' input frames k (source: depth once converted to float32 metres as f32(raw) /
    f32(depth_scale), uint8 colours as f32(c) / 255f) against the renderings (target) with depth_scale 1 from the identity; the transform
    maps the frame's camera to the rendering's, so pose_k = pose_(k-1) T; frame k is integrated at pose_k, under its rigid inverse
    (R^T, -R^T t) taken scene by scene, one integrate call for all scenes.  A scene whose pair fails keeps its pose and is not integrated at that step; the
    frames after it go on against the same model.  The host reads one success flag per scene and step for this, and nothing else of the
    results (ray_cast and the sparse integrate invert their extrinsics on the host, as they do everywhere).  What the parts refuse is
    refused here before any state changes.
    Returns (poses, success, volumes): per scene (F_i, 4, 4) float64 camera-to-world poses and (F_i,) bool on the device (frame 0 is True),
    and the volumes object, from which extraction, meshes and further ray_cast calls start.
    Departures from Open3D's slam.Model: the odometry is the legacy hybrid RGB-D odometry of this library against the rendered depth and
    colour, not the tensor odometry against a rendered vertex map; the rendering has no range map and the departures of ray_cast; there
    is no tracking-loss handling beyond skipping the frame, no relocalisation and no loop closure; integration is that of the volumes here
    (no weight cap, no block pre-selection from the rendered depth)."""
    what = 'track_and_integrate_rgbd'
    V = len(depths_list)
    if len(colors_list) != V:
        raise ValueError('%s: one entry per scene expected in every list (%d scenes)' % (what, V))
    if 'depth_scale' in odometry_options or any(k not in _ODOMETRY_OPTIONS for k in odometry_options):
        raise ValueError('%s: odometry options are %s' % (what, ', '.join(k for k in _ODOMETRY_OPTIONS if k != 'depth_scale')))
    odo = dict(odometry_options, depth_scale=1.0)
    odo.setdefault('depth_trunc', depth_trunc)
    checked = _options(what, **{**dict(method='hybrid', iterations=(20, 10, 5), min_depth=0.0, max_depth=4.0, max_depth_diff=0.03), **odo})
    scale, far = _positive(what, 'depth_scale', depth_scale), _positive(what, 'depth_trunc', depth_trunc)
    dev = device_of(device, depths_list)
    if not sparse and resolution is None:
        raise ValueError('%s: resolution is required with sparse=False' % what)
    if sparse and (resolution is not None or origins is not None):
        raise ValueError('%s: resolution and origins belong to sparse=False' % what)
    volumes = SparseTSDFVolumes(V, voxel_length, sdf_trunc, True, stride, dev) if sparse else TSDFVolumes(V, resolution, voxel_length, sdf_trunc, origins,
                                                                                                          True, dev)
    counts = [int(d.shape[0]) if torch.is_tensor(d) and d.dim() == 3 else -1 for d in depths_list]
    for g in range(V):
        d, c = depths_list[g], colors_list[g]
        if counts[g] < 0 or d.dtype not in _DEPTH_DTYPES or not torch.is_tensor(c) or c.dtype not in _COLOR_DTYPES or tuple(c.shape) != tuple(d.shape) + (3,):
            raise RuntimeError('%s: scene %d needs depths (F, H, W) uint16 or float32 and colors (F, H, W, 3) uint8 or float32' % (what, g))
        if (d.dtype, c.dtype, tuple(d.shape[1:])) != (depths_list[0].dtype, colors_list[0].dtype, tuple(depths_list[0].shape[1:])):
            raise RuntimeError('%s: the scenes must share their image size and dtypes' % what)
        _frames(what, d, c, len(checked['iterations']))
        _gpu_only(what, dev, depths=d, colors=c)
    if isinstance(intrinsics, (list, tuple)) and len(intrinsics) == V and V and not np.isscalar(intrinsics[0]):
        K = [_host_intrinsics(what, k, max(n, 1))[0:1] for k, n in zip(intrinsics, counts)]
        if any(n and not np.array_equal(_host_intrinsics(what, k, n), np.repeat(K[g], n, 0)) for g, (k, n) in enumerate(zip(intrinsics, counts))):
            raise ValueError('%s: the frames of a scene must share their intrinsics' % what)
    else:
        K = [_host_intrinsics(what, intrinsics, 1)] * V
    pose = transforms_of(init_poses, V, what, dev, finite=True)
    pose = [pose[g:g + 1] for g in range(V)]
    H, W = (int(s) for s in depths_list[0].shape[1:]) if V else (1, 1)
    poses, success = [[] for _ in range(V)], [[] for _ in range(V)]
    for k in range(max(counts, default=0)):
        active = [g for g in range(V) if counts[g] > k]
        ok = [True] * len(active)
        if k:
            views = [1 if g in active else 0 for g in range(V)]
            model = volumes.ray_cast(np.concatenate([K[g] for g in active]), torch.cat([_rigid_inverses(pose[g]) for g in active]), H, W, views,
                                     depth_max=far, weight_threshold=weight_threshold, maps=('depth', 'color'))
            S = len(active)
            d = torch.cat([_metres(_join(what, [depths_list[g][k:k + 1] for g in active]), scale), model['depth']])
            c = torch.cat([_unit_colors(_join(what, [colors_list[g][k:k + 1] for g in active])), model['color']])
            found = rgbd_odometry_pairs(d, c, np.concatenate([K[g] for g in active] * 2), [(i, S + i) for i in range(S)], None,
                                        return_information=False, **odo)
            ok = found['success'].cpu().tolist()                        # (the one host read of the step)
            for i, g in enumerate(active):
                if ok[i]:
                    pose[g] = pose[g] @ found['transforms'][i:i + 1]
        fused = [g for i, g in enumerate(active) if ok[i]]
        if fused:
            volumes.integrate(_join(what, [depths_list[g][k:k + 1] for g in fused]), np.concatenate([K[g] for g in fused]),
                              torch.cat([_rigid_inverses(pose[g]) for g in fused]), [1 if g in fused else 0 for g in range(V)],
                              _join(what, [colors_list[g][k:k + 1] for g in fused]), scale, far)
        for i, g in enumerate(active):
            poses[g].append(pose[g]), success[g].append(bool(ok[i]))
    f64 = dict(dtype=torch.float64, device=dev)
    return ([torch.cat(p) if p else torch.zeros((0, 4, 4), **f64) for p in poses],
            [torch.tensor(s, dtype=torch.bool, device=dev) for s in success], volumes)
