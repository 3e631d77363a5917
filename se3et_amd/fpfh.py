"""FPFH descriptors on the device: Open3D's compute_fpfh_feature (33 bins from the point-pair angles over a point's neighbourhood), the
weights-free descriptor that the reference's make_open3d_registration_feature / registration_with_ransac_from_feats (utils/open3d.py) are
fed with, as batched HIP kernels (csrc/fpfh.hip, csrc/fpfh_core.h) on the searches of csrc/pair_grid.h.

  compute_fpfh_clouds(points_list, normals_list, radius=None, max_nn=None, dtype=torch.float64)   list of (n_c, 33) tensors on the device
  spfh_clouds(points_list, normals_list, radius=None, max_nn=None)                                the first pass alone, float64
  compute_fpfh_feature(points, normals, radius=None, max_nn=None)                                 one cloud, numpy in, (n, 33) numpy out
  global_registration_pairs(src_list, ref_list, voxel_size, ...)                                  (outlier removal,) downsample, (planes out,
                                                                                                  clusters kept,) normals, FPFH, (ISS keypoints,)
                                                                                                  RANSAC or FGR, ICP

The batched calls take GPU tensors only (there is no CPU path): points and normals (n, 3) float32 or float64, promoted on load; any number
of clouds per call, chunked at the library's SE3_PAIR_MAX_PAIRS clouds and, within a chunk, at PAIR_BUDGET neighbour-list entries (16
bytes each) per launch sequence.  One host synchronisation per chunk (the list's size and the status words in one copy); a chunk above the
budget adds one.  dtype=torch.float32 rounds the finished float64 row once: the form feature_matching takes.

Search modes, as Open3D's three KDTreeSearchParams:
  radius only       every point with d^2 < r^2 (strict, as the project's other ball queries), r^2 = r r in float64; no cap on the count
  max_nn = K only   the K nearest INCLUDING the row itself, K in [1, SE3_KNN_MAX = 64]; membership and ties at the K-th place are
                    knn_clouds' rule: (d^2, index) ascending, the lower index wins
  both (hybrid)     the K nearest, then of those the ones with d^2 < r^2
Neither given is a ValueError.  Open3D's tutorial value max_nn = 100 is above the library's limit and is refused.

Contract (csrc/fpfh.hip carries the same text).  The structure is Open3D's (Feature.cpp: ComputePairFeatures, ComputeSPFHFeature,
ComputeFPFHFeature); the arithmetic is the project's own, chosen so that host and device agree bit for bit: float64, contraction off, no
libm call other than the square root and division.
  Neighbours.  The neighbours of row i are the members of its search result other than row i itself, chosen by index; m is their number.
    A duplicate point at d = 0 is a neighbour.
  Pair feature of (p1, n1) and (p2, n2), normals as given (not normalised).  Dot products are (a b + c d) + e f.
    1. dp = p2 - p1, d = sqrt((dx dx + dy dy) + dz dz).          2. d == 0: degenerate.
    3. a1 = n1 . dp / d, a2 = n2 . dp / d.
    4. |a1| < |a2| (strict; Open3D writes acos|a1| > acos|a2|): swap the normals, negate dp, f2 = -a2.  Otherwise f2 = a1.
    5. v = dp x n1; |v| == 0: degenerate.                         6. v /= |v|; w = n1 x v; f1 = v . n2; y = (w . n2) + 0.0; x = n1 . n2.
    A degenerate pair has f1 = f2 = 0 and x = y = 0.
  Bins.  f1 and f2: clamp(floor(11 (f + 1) 0.5), 0, 10).  theta = atan2(y, x) is binned without computing it: with beta_k = -pi +
    2 pi k / 11 and (c_k, s_k) = (cos, sin) beta_k for k = 1..10 as float64 literals, the bin is 5 if x == 0 and y == 0; the number of k
    in 1..5 with c_k y - s_k x >= 0 if y < 0; otherwise 5 plus the number of k in 6..10 with c_k y - s_k x >= 0.  This is
    clamp(floor(11 (theta + pi) / 2 pi), 0, 10) away from the edges; theta = pi gives bin 10; a degenerate pair gives bins 5, 5, 5 and is
    counted, as in Open3D.
  SPFH row.  bin count x (100.0 / m): integer counts and one product, so the order of the neighbours does not matter.  theta at 0-10, f1
    at 11-21, f2 at 22-32.  m == 0 gives a zero row.
  FPFH row.  A_j = sum_k spfh(j, k) / d2_k, a sequential sum over the neighbours k with d2_k != 0 in ascending neighbour index;
    S_g = the sequential sum of the group's eleven A_j in ascending j; F_j = spfh(j, i) + (S_g != 0 ? A_j (100 / S_g) : A_j).  A row with
    a neighbour at d > 0 therefore sums to 600.
  Refusals.  A non-finite point or normal raises ValueError naming the cloud (a device flag, read in the chunk's one synchronisation).  A
    zero normal is not refused: its pairs are degenerate.  n = 0 gives an empty output.
  Determinism.  No float atomics: a cloud's rows are bit-identical alone, anywhere in a batch, and from run to run.

Where this departs from Open3D: the strict radius test and the tie rule of the searches; the swap test on |a| instead of acos|a|; the
sector rule in place of atan2 and a floor; the fixed summation order.  None of them moves a value beyond rounding, or a count except for a
pair within rounding of a bin edge."""
import numpy as np
import torch

from . import ops as _ops
from .stacking import chunks, device_of, exclusive_offsets, gpu_rows_each, identities, lengths, stack, to_device, upload

_FAMILY = 'FPFH'
DIM = _ops.FPFH_DIM
PAIR_BUDGET = 1 << 23          # neighbour-list entries per launch sequence: 16 bytes each, 128 MiB


def _search_mode(radius, max_nn, what):
    """(r or None, K or None) of a call, or ValueError."""
    if radius is None and max_nn is None:
        raise ValueError('%s: give radius, max_nn or both (a radius, k-nearest or hybrid search)' % what)
    r = K = None
    if radius is not None:
        r = float(radius)
        if not (np.isfinite(r) and r > 0):
            raise ValueError('%s: radius %r is not a positive finite number' % (what, radius))
    if max_nn is not None:
        if int(max_nn) != max_nn or int(max_nn) < 1:
            raise ValueError('%s: max_nn %r is not an integer >= 1' % (what, max_nn))
        K = int(max_nn)
        if K > _ops.KNN_MAX:
            raise ValueError("%s: max_nn %d is above the library's limit SE3_KNN_MAX = %d (Open3D's tutorial value 100 among them): give "
                             'max_nn <= %d, or the radius alone, which has no cap' % (what, K, _ops.KNN_MAX, _ops.KNN_MAX))
    return r, K


def _partial(offsets, s, e):
    """The rows of [s, e) that each cloud owns."""
    return [max(0, min(e, offsets[c + 1]) - max(s, offsets[c])) for c in range(len(offsets) - 1)]


def _refuse(what, a, words):
    if words[-1]:
        raise ValueError('%s: ' % what + '; '.join('cloud %d: %s' % (a + c, ', '.join(t for bit, t in _ops.FPFH_STATUS.items() if w & bit))
                                                   for c, w in enumerate(words[:-1]) if w))


def _radius_lists(p, pl, r, words, what, a, budget=None):
    """The chunk's neighbour lists from the ball query: a function that yields (row_begin, row_offsets, pairs) per slice of at most
    PAIR_BUDGET entries (half of it plus one row's, where a chunk is cut), and whether there is more than one slice.  r: one radius, or
    a list of one per cloud; budget: another family's own budget in place of PAIR_BUDGET (se3et_amd/iss.py runs its saliency pass over
    the same lists, with a radius per cloud)."""
    n, offsets = p.shape[0], exclusive_offsets(pl)
    budget = PAIR_BUDGET if budget is None else budget
    grid = _ops.pair_grid_build(p, pl, identities(len(pl)), max(r, default=0.0) if isinstance(r, list) else r)
    ro = _ops.pair_ball_count_stack(grid, p, pl, r)
    host = torch.cat([ro[-1:], words.to(torch.int64)]).cpu().tolist()           # the ONE synchronisation of the chunk: the total, the status
    _refuse(what, a, host[1:])
    total = host[0]
    if total <= budget:
        cuts, at = [0, n], [0, total]
    else:
        half = max(1, budget // 2)
        targets = torch.arange(half, total, half, dtype=torch.int64, device=p.device)
        rows = (torch.searchsorted(ro, targets, right=True) - 1).clamp(1, n)
        rows = torch.unique(torch.cat([rows.new_zeros(1), rows, rows.new_full((1,), n)]))
        both = torch.stack([rows, ro[rows]]).cpu().tolist()                      # (a chunk above the budget: its cuts, one more copy)
        cuts, at = both

    def slices():
        for k in range(len(cuts) - 1):
            s, e = cuts[k], cuts[k + 1]
            ro_s = ro if (s, e) == (0, n) else ro[s:e + 1] - at[k]
            yield s, ro_s, _ops.pair_ball_fill_stack(grid, p[s:e], _partial(offsets, s, e), r, ro_s, at[k + 1] - at[k])
    return slices, len(cuts) > 2


def _knn_lists(p, pl, r, K):
    """The same from the k nearest: every row owns K entries; the columns a small cloud leaves empty, or the radius masks, hold the row's
    own index, which the kernels skip as they skip the row itself."""
    n, offsets, dev = p.shape[0], exclusive_offsets(pl), p.device
    grid = _ops.pair_grid_build(p, pl, identities(len(pl)), 0.0)
    per = max(1, PAIR_BUDGET // K)
    cloud = torch.repeat_interleave(torch.arange(len(pl), device=dev), to_device(pl, torch.int64, dev), output_size=n)
    local = torch.arange(n, dtype=torch.int64, device=dev) - to_device(offsets[:-1], torch.int64, dev)[cloud]

    def slices():
        for s in range(0, n, per):
            e = min(n, s + per)
            idx, d2 = _ops.knn_stack(grid, p[s:e], _partial(offsets, s, e), K)
            keep = idx >= 0
            if r is not None:
                keep &= d2 < r * r
            own = local[s:e, None].expand(e - s, K)
            j = torch.where(keep, idx, own).sort(dim=1).values
            ro = torch.arange(0, (e - s + 1) * K, K, dtype=torch.int64, device=dev)
            yield s, ro, torch.stack([own, j], 2).reshape(-1, 2)
    return slices, n > per


@torch.no_grad()
def _descriptor_clouds(points_list, normals_list, radius, max_nn, device, what, second_pass):
    r, K = _search_mode(radius, max_nn, what)
    if len(points_list) != len(normals_list):
        raise ValueError('%s: one normals tensor per cloud: %d for %d clouds' % (what, len(normals_list), len(points_list)))
    dev = device_of(device, points_list, normals_list)
    pts = gpu_rows_each(points_list, dev, what + ': cloud', _FAMILY)
    nrs = gpu_rows_each(normals_list, dev, what + ': normals: cloud', _FAMILY)
    for c, (p, nr) in enumerate(zip(pts, nrs)):
        if nr.shape != p.shape or nr.device != p.device:
            raise ValueError('%s: cloud %d: normals %s on %s for points %s on %s' % (what, c, tuple(nr.shape), nr.device, tuple(p.shape), p.device))
    out = []
    for a, b in chunks(len(pts)):
        p, nr, pl = stack(pts[a:b]), stack(nrs[a:b]), lengths(pts[a:b])
        words = _ops.fpfh_check_stack(p, nr, pl)
        if K is None:
            slices, several = _radius_lists(p, pl, r, words, what, a)
        else:
            _refuse(what, a, words.cpu().tolist())                               # the ONE synchronisation of the chunk: the status
            slices, several = _knn_lists(p, pl, r, K)
        spfh = torch.empty((p.shape[0], DIM), dtype=torch.float64, device=p.device)
        res = torch.empty_like(spfh) if second_pass else spfh
        for s, ro, pairs in slices():
            _ops.spfh_stack(p, nr, pl, ro, pairs, spfh, s)
            if second_pass and not several:
                _ops.fpfh_stack(p, spfh, pl, ro, pairs, res, s)
        if second_pass and several:                                              # (every SPFH row first: the lists are searched again)
            for s, ro, pairs in slices():
                _ops.fpfh_stack(p, spfh, pl, ro, pairs, res, s)
        out += list(torch.split(res, pl))
    return out


def compute_fpfh_clouds(points_list, normals_list, radius=None, max_nn=None, dtype=torch.float64, device=None):
    """FPFH of a list of clouds: points and normals (n, 3) float32 or float64 GPU tensors.  radius, max_nn or both choose the search (see
    the module text).  Returns the list of (n_c, 33) tensors on the device, float64, or float32 (the float64 row rounded once)."""
    if dtype not in (torch.float32, torch.float64):
        raise ValueError('compute_fpfh_clouds: dtype must be torch.float32 or torch.float64, got %r' % (dtype,))
    out = _descriptor_clouds(points_list, normals_list, radius, max_nn, device, 'compute_fpfh_clouds', True)
    return out if dtype == torch.float64 else [f.to(torch.float32) for f in out]


def spfh_clouds(points_list, normals_list, radius=None, max_nn=None, device=None):
    """The first pass alone (tests and diagnostics): the list of (n_c, 33) float64 SPFH rows, bin count x (100 / m)."""
    return _descriptor_clouds(points_list, normals_list, radius, max_nn, device, 'spfh_clouds', False)


def compute_fpfh_feature(points, normals, radius=None, max_nn=None, device=None):
    """One cloud, numpy in and out: (n, 33) float64, rows are points -- the layout utils/open3d.py's make_open3d_registration_feature takes
    (Open3D's own Feature.data is the transpose)."""
    _search_mode(radius, max_nn, 'compute_fpfh_feature')
    return compute_fpfh_clouds([upload(points, device)], [upload(normals, device)], radius, max_nn)[0].cpu().numpy()


@torch.no_grad()
def global_registration_pairs(src_list, ref_list, voxel_size, normal_knn=33, fpfh_radius=None, fpfh_max_nn=None, distance_threshold=None,
                              ransac_n=3, num_iterations=50000, mutual_filter=True, edge_length_similarity=0.9, check_distance=True,
                              icp_distance=None, icp_estimation='point_to_point', icp_max_iteration=30, seed=0, device=None, icp_loss=None,
                              icp_loss_k=None, coarse='ransac', fgr_distance=None, fgr_options=None, outlier_removal=None, keypoints=None,
                              iss_options=None, remove_planes=0, plane_options=None, keep_clusters=None, dbscan_options=None):
    """The classical global registration of P pairs, a composition of the batched tools (no kernel of its own): voxel_downsample_clouds at
    voxel_size, estimate_normals_clouds (normal_knn), compute_fpfh_clouds (float32), ransac_from_feats_pairs, and with icp_distance
    icp_pairs from the RANSAC result on the downsampled clouds.  src_list / ref_list: (n, 3) float32 or float64 GPU tensors.
    Defaults, as multiples of voxel_size: fpfh_radius None = 5 voxel_size when fpfh_max_nn is None too (a radius search; give fpfh_max_nn
    alone for the k nearest, both for the hybrid); distance_threshold None = 1.5 voxel_size.  icp_distance None: no refinement.
    icp_estimation 'generalized' refines with generalized_icp_pairs on the normals computed here for both clouds; icp_loss / icp_loss_k:
    the robust loss kernel of either refinement (icp.icp_pairs), None for none.
    coarse: 'ransac' (ransac_from_feats_pairs, as above) or 'fgr': fgr.fgr_from_feats_pairs on the same features, mutual matches always,
    with maximum_correspondence_distance = fgr_distance (None: distance_threshold; in normalised units unless fgr_options says
    use_absolute_scale) and fgr_options, a dict of further options of fgr.fgr_pairs; ransac_n, num_iterations, mutual_filter and the
    checkers are then not read.
    outlier_removal: None, ('statistical', nb_neighbors, std_ratio) or ('radius', nb_points, radius): scan_prep's filter of that name on
    the raw clouds before the voxel downsampling.  keypoints: None or 'iss': iss.iss_keypoints_clouds (iss_options: a dict of its
    arguments) on the downsampled clouds; normals and FPFH are still computed on the whole downsampled clouds (the neighbourhoods need
    them), only the keypoint rows of points and features go to the coarse method, and ICP refines on the whole downsampled clouds.
    Returns a dict: transforms (P, 4, 4) float64 on the device (ref ~ T src), coarse_transforms (the coarse method's), ransac_transforms
    (the same tensor under coarse='ransac', else None), src_points / ref_points / src_normals / ref_normals / src_feats / ref_feats (the
    intermediate lists), ransac (the dict of ransac_from_feats_pairs, or None), fgr (the dict of fgr_from_feats_pairs, or None) and icp
    (that of icp_pairs or generalized_icp_pairs, or None).  A call with outlier_removal or keypoints adds four keys: src_keypoints /
    ref_keypoints (the lists of keypoint indices into src_points / ref_points, None without a detector) and src_kept / ref_kept (the
    lists of the raw rows the outlier filter kept, None without one); a call with neither returns exactly the keys above.
    remove_planes: how many dominant planes segmentation.segment_planes_clouds peels off every downsampled cloud (0: none; plane_options:
    a dict of its further arguments, distance_threshold 0.5 voxel_size unless given there).  keep_clusters: None, or the least size of a
    DBSCAN cluster (segmentation.cluster_dbscan_clouds; dbscan_options: eps, 2.5 voxel_size unless given, and min_points, 5 unless given)
    whose rows are kept; noise and smaller clusters are dropped.  Both apply to the downsampled clouds before the normals, the planes
    first, and only the kept rows go on to every later stage.  A call with either adds eight keys: src_segment_rows / ref_segment_rows
    (the lists of the kept rows' indices into the downsampled clouds, int64, ascending), src_plane_labels / ref_plane_labels and
    src_planes / ref_planes (the labels per downsampled row and the (P, remove_planes, 4) planes of segment_planes_clouds; None without
    remove_planes), src_cluster_labels / ref_cluster_labels (the DBSCAN labels of the rows the planes left; None without keep_clusters).
    With both at their defaults the result has exactly the keys above and the same bits."""
    from .icp import generalized_icp_pairs, icp_pairs
    from .ransac import ransac_from_feats_pairs
    from .scan_prep import estimate_normals_clouds, voxel_downsample_clouds
    what = 'global_registration_pairs'
    P = len(src_list)
    if len(ref_list) != P:
        raise ValueError('%s: one source and one reference cloud per pair' % what)
    if coarse not in ('ransac', 'fgr'):
        raise ValueError("%s: coarse %r is not one of 'ransac', 'fgr'" % (what, coarse))
    if keypoints not in (None, 'iss'):
        raise ValueError("%s: keypoints %r is not None or 'iss'" % (what, keypoints))
    if outlier_removal is not None and (len(outlier_removal) != 3 or outlier_removal[0] not in ('statistical', 'radius')):
        raise ValueError("%s: outlier_removal %r is not None, ('statistical', nb_neighbors, std_ratio) or ('radius', nb_points, radius)"
                         % (what, outlier_removal))
    if int(remove_planes) != remove_planes or int(remove_planes) < 0:
        raise ValueError('%s: remove_planes %r is not an integer >= 0' % (what, remove_planes))
    if keep_clusters is not None and (int(keep_clusters) != keep_clusters or int(keep_clusters) < 1):
        raise ValueError('%s: keep_clusters %r is not None or an integer >= 1' % (what, keep_clusters))
    v = float(voxel_size)
    if not (np.isfinite(v) and v > 0):
        raise ValueError('%s: voxel size %r is not a positive finite number' % (what, voxel_size))
    if fpfh_radius is None and fpfh_max_nn is None:
        fpfh_radius = 5.0 * v
    if distance_threshold is None:
        distance_threshold = 1.5 * v
    dev = device_of(device, src_list, ref_list)
    raw, kept = list(src_list) + list(ref_list), None
    if outlier_removal is not None:
        from .scan_prep import remove_radius_outlier_clouds, remove_statistical_outlier_clouds
        remove = remove_statistical_outlier_clouds if outlier_removal[0] == 'statistical' else remove_radius_outlier_clouds
        kept = remove(raw, outlier_removal[1], outlier_removal[2], device=dev)
        raw = [c[k] for c, k in zip(raw, kept)]
    clouds = voxel_downsample_clouds(raw, v, device=dev)
    segment = None
    if remove_planes or keep_clusters is not None:
        from .segmentation import cluster_dbscan_clouds, segment_planes_clouds
        rows = [torch.arange(c.shape[0], dtype=torch.int64, device=c.device) for c in clouds]
        plane_labels = plane_models = cluster_labels = None
        if remove_planes:
            options = dict(plane_options or {})
            options.setdefault('distance_threshold', 0.5 * v)
            options.setdefault('seed', seed)
            plane_labels, plane_models, _ = segment_planes_clouds(clouds, max_planes=int(remove_planes), device=dev, **options)
            rows = [r[lab < 0] for r, lab in zip(rows, plane_labels)]
        if keep_clusters is not None:
            options = dict(dbscan_options or {})
            cluster_labels, _ = cluster_dbscan_clouds([c[r] for c, r in zip(clouds, rows)], options.pop('eps', 2.5 * v),
                                                      options.pop('min_points', 5), device=dev, **options)
            big = [torch.bincount(lab[lab >= 0].to(torch.int64), minlength=1) >= int(keep_clusters) for lab in cluster_labels]
            rows = [r[(lab >= 0) & b[lab.clamp(min=0).to(torch.int64)]] for r, lab, b in zip(rows, cluster_labels, big)]
        clouds = [c[r] for c, r in zip(clouds, rows)]
        segment = (rows, plane_labels, plane_models, cluster_labels)
    normals = estimate_normals_clouds(clouds, normal_knn, device=dev)
    feats = compute_fpfh_clouds(clouds, normals, fpfh_radius, fpfh_max_nn, torch.float32, device=dev)
    src, ref = clouds[:P], clouds[P:]
    keys, full = None, (src, ref, feats)
    if keypoints == 'iss':
        from .iss import iss_keypoints_clouds
        keys = iss_keypoints_clouds(clouds, device=dev, **(iss_options or {}))
        src, ref = [c[k] for c, k in zip(src, keys[:P])], [c[k] for c, k in zip(ref, keys[P:])]
        feats = [f[k] for f, k in zip(feats, keys)]
    ransac, fgr = None, None
    if coarse == 'fgr':
        from .fgr import fgr_from_feats_pairs
        options = dict(fgr_options or {}, maximum_correspondence_distance=distance_threshold if fgr_distance is None else fgr_distance)
        options.setdefault('seed', seed)
        fgr = fgr_from_feats_pairs(src, ref, feats[:P], feats[P:], device=dev, **options)
        coarse_transforms = fgr['transforms']
    else:
        ransac = ransac_from_feats_pairs([c.to(torch.float32) for c in src], [c.to(torch.float32) for c in ref], feats[:P], feats[P:],
                                         distance_threshold, ransac_n, num_iterations, mutual_filter, seed, edge_length_similarity,
                                         check_distance)
        coarse_transforms = ransac['transforms'].to(torch.float64)
    src, ref, feats = full
    icp = None
    if icp_distance is not None and icp_estimation == 'generalized':
        icp = generalized_icp_pairs(src, ref, coarse_transforms, icp_distance, normals[:P], normals[P:], loss=icp_loss, loss_k=icp_loss_k,
                                    max_iteration=icp_max_iteration, device=dev)
    elif icp_distance is not None:
        icp = icp_pairs(src, ref, coarse_transforms, icp_distance, icp_estimation, normals[P:] if icp_estimation == 'point_to_plane' else None,
                        max_iteration=icp_max_iteration, device=dev, loss=icp_loss, loss_k=icp_loss_k)
    out = {'transforms': icp['transforms'] if icp is not None else coarse_transforms, 'coarse_transforms': coarse_transforms,
           'ransac_transforms': coarse_transforms if ransac is not None else None, 'src_points': src, 'ref_points': ref, 'src_normals': normals[:P],
           'ref_normals': normals[P:], 'src_feats': feats[:P], 'ref_feats': feats[P:], 'ransac': ransac, 'fgr': fgr, 'icp': icp}
    if keypoints is not None or outlier_removal is not None:
        out.update(src_keypoints=keys[:P] if keys is not None else None, ref_keypoints=keys[P:] if keys is not None else None,
                   src_kept=kept[:P] if kept is not None else None, ref_kept=kept[P:] if kept is not None else None)
    if segment is not None:
        for key, value in zip(('segment_rows', 'plane_labels', 'planes', 'cluster_labels'), segment):
            out['src_' + key], out['ref_' + key] = (None, None) if value is None else (value[:P], value[P:])
    return out
