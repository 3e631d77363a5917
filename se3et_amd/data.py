"""On-GPU counterpart of the reference's stack-mode collate (geotransformer/utils/data.py:13-97,159-209).

The reference runs grid subsampling and the 3S-2 radius searches on the CPU inside DataLoader workers; here the
whole pyramid is built on the GPU in the main process right after the raw pair was uploaded, with two host
synchronisations (the counts of all subsampling stages; the widths of all neighbour tables + the number of rows with exact distance
ties).  Clouds that hold exact ties (real scans) take one more per support stage: a host copy of the stage's points, from which the
reference's k-d tree is built for the device pass that gives those rows the reference's order (csrc/radius_ties.hip).  List structure,
voxel/radius doubling, the 2000-point cap of the coarsest stage and the column truncation are reproduced exactly
(pinned by tests/golden/precompute_c1.npz).  The reference's third step, the calibration of the neighbour limits from the data
(utils/data.py:212-252), is calibrate_neighbors_stack_mode below: count-only searches, no tables (pinned by tests/golden/calibration.npz)."""
import warnings

import numpy as np
import torch

from . import ops as _ops
from ._lib import CONSTANTS
from .modules.ops import grid_subsample

SE3_MAX_BATCH, SE3_MAX_NEIGHBOR_LIMIT = CONSTANTS['SE3_MAX_BATCH'], CONSTANTS['SE3_MAX_NEIGHBOR_LIMIT']


def cap_coarsest(points, lengths, cap=2000):
    """The reference keeps at most 2000 superpoints per cloud, the first ones in its output order (utils/data.py:40-48); any number of
    stacked clouds here.  -> (points, lengths)"""
    if int(lengths.max()) <= cap:
        return points, lengths
    keep, start = [], 0
    for n in lengths.tolist():
        keep.append(points[start:start + min(n, cap)])
        start += n
    return torch.cat(keep, 0), torch.clamp(lengths, max=cap)


def stage_clouds(points, lengths, num_stages, voxel_size, normals=None):
    """The point pyramid of the reference's precompute_data_stack_mode: stage 0 the clouds as given, stage i > 0 the grid subsampling of
    stage i - 1 at voxel_size * 2^i, the coarsest stage capped at 2000 points per cloud.  points (N, 3) float32 on the GPU, lengths host
    int64.  -> (points_list, lengths_list of host int64 tensors); with normals (N, 3) float32 (carried through every subsampling stage and
    capped with the points, as the reference carries them) also the normals_list."""
    points_list, lengths_list, normals_list = [], [], []
    # the S-1 subsampling stages back to back: every stage takes the per-cloud counts of the one before from DEVICE memory (outputs sized
    # by the stage-0 row count, an upper bound), and ONE synchronisation fetches the counts of all stages
    sub_pts, sub_nrm, sub_len, cur_pts, cur_nrm, cur_len, v = [], [], [], points, normals, lengths, voxel_size
    for i in range(1, num_stages):
        v *= 2
        cur_pts, cur_nrm, cur_len = _ops.grid_subsample(cur_pts, cur_len, cur_nrm, v)
        sub_pts.append(cur_pts)
        sub_nrm.append(cur_nrm)
        sub_len.append(cur_len)
    sub_len = torch.stack(sub_len).cpu() if sub_len else None
    for i in range(num_stages):
        if i > 0:
            lengths = sub_len[i - 1].clone()
            points = sub_pts[i - 1][:int(lengths.sum())]
            if normals is not None:
                normals = sub_nrm[i - 1][:int(lengths.sum())]
        if i == num_stages - 1:
            if normals is not None:
                normals = cap_coarsest(normals, lengths)[0]
            points, lengths = cap_coarsest(points, lengths)
        points_list.append(points.contiguous())
        lengths_list.append(lengths)
        if normals is not None:
            normals_list.append(normals.contiguous())
    return (points_list, lengths_list) if normals is None else (points_list, lengths_list, normals_list)


def precompute_data_stack_mode(points, lengths, num_stages, voxel_size, radius, neighbor_limits, normals=False):
    """points (N, 3) float32 GPU tensor (ref rows then src rows; several pairs may be stacked: ref0, src0, ref1, src1, ...),
    lengths (2 B,) int64 (host).  Returns the dict of lists
    {'points', 'lengths', 'neighbors', 'subsampling', 'upsampling'}; `lengths` entries are host int64 tensors.  normals=True adds the
    reference's 'normals' list of (N_i, 3) float32 (utils/data.py:23-28): stage 0 estimated per cloud on the device (se3et_amd.scan_prep:
    k-NN 33, canonical sign, cast to float32), later stages carried by the grid subsampling, the coarsest capped with its points."""
    assert num_stages == len(neighbor_limits)
    if not points.is_cuda:
        raise RuntimeError('precompute_data_stack_mode: points must be on the GPU')
    lengths = torch.as_tensor(lengths, dtype=torch.int64).cpu()
    normals_list = None
    if normals:
        from .scan_prep import estimate_normals_clouds
        normals0 = torch.cat(estimate_normals_clouds(list(torch.split(points, lengths.tolist()))), 0).float()
        points_list, lengths_list, normals_list = stage_clouds(points, lengths, num_stages, voxel_size, normals0)
    else:
        points_list, lengths_list = stage_clouds(points, lengths, num_stages, voxel_size)

    # a spatial order of every stage's points for the union-staged KPConv (tile membership only; csrc/kpconv_union.hip)
    # (the default policy runs that kernel on the layers whose queries are stage 0 / 1 points: ops._kpconv_union_pays)
    # ... and only on stacked batches: with one pair per forward (10 000 stage-0 points) the order and the plans cost what the kernels gain
    ns = num_stages if _ops.KPCONV_UNION_ALL else min(2, num_stages)
    if _ops.KPCONV_UNION and (_ops.KPCONV_UNION_ALL or points_list[0].shape[0] >= _ops.KPCONV_UNION_MIN_POINTS):
        _ops.register_point_orders(points_list[:ns], lengths_list[:ns], [voxel_size * 2 ** i for i in range(ns)])
    # all 3S-2 searches are launched back to back; their column counts are fetched with ONE synchronisation
    jobs = []
    grids = {}

    def grid_for(stage, r):       # one cell grid per (support stage, radius): shared by up to three searches
        key = (stage, float(r))
        if key not in grids:
            s_pts = points_list[stage]
            grids[key] = (_ops.RadiusGrid(s_pts, lengths_list[stage], r)
                          if s_pts.shape[0] >= _ops.GRID_SEARCH_MIN_SUPPORT else None)
        return grids[key]

    n_jobs, n_clouds = 3 * num_stages - 2, len(lengths_list[0])
    # one fill for the counters of all searches: per job the largest in-radius count of every cloud, then per job the number of rows whose
    # kept columns hold an EXACT distance tie (the reference orders those by its k-d tree walk: csrc/radius_ties.hip)
    words = torch.zeros((n_jobs * n_clouds + n_jobs,), dtype=torch.int32, device=points.device)
    counters, tie_counts = words[:n_jobs * n_clouds].view(n_jobs, n_clouds), words[n_jobs * n_clouds:]
    want_ties = _ops.RADIUS_REFERENCE_TIES
    q_rows = [points_list[i].shape[0] for i in range(num_stages)]
    tie_rows = torch.empty((sum(q_rows) + sum(q_rows[1:]) + sum(q_rows[:-1]),), dtype=torch.int32, device=points.device) if want_ties else None
    tie_at = [0]

    def ties_for(nq):             # this job's slice of the row list + its counter word
        if not want_ties:
            return None
        j, o = len(jobs), tie_at[0]
        tie_at[0] += nq
        return tie_rows[o:o + nq], tie_counts[j:j + 1]

    searches = []                 # per job: (queries, support, q_lengths, s_lengths, radius, support stage, ties)
    for i in range(num_stages):
        cur, cl = points_list[i], lengths_list[i]
        t = ties_for(cur.shape[0])
        searches.append((cur, cur, cl, cl, radius, i, t))
        jobs.append(('neighbors', _ops.radius_neighbors(cur, cur, cl, cl, radius, neighbor_limits[i], grid=grid_for(i, radius),
                                                        zeroed_max_count=counters[len(jobs)], ties=t)))
        if i < num_stages - 1:
            sub, sl = points_list[i + 1], lengths_list[i + 1]
            t = ties_for(sub.shape[0])
            searches.append((sub, cur, sl, cl, radius, i, t))
            jobs.append(('subsampling', _ops.radius_neighbors(sub, cur, sl, cl, radius, neighbor_limits[i],
                                                              grid=grid_for(i, radius), zeroed_max_count=counters[len(jobs)], ties=t)))
            t = ties_for(cur.shape[0])
            searches.append((cur, sub, cl, sl, radius * 2, i + 1, t))
            jobs.append(('upsampling', _ops.radius_neighbors(cur, sub, cl, sl, radius * 2, neighbor_limits[i + 1],
                                                             grid=grid_for(i + 1, radius * 2), zeroed_max_count=counters[len(jobs)], ties=t)))
        radius *= 2
    for j, (_, (_, mc)) in enumerate(jobs):       # (a search on a small support takes the exhaustive kernel, which fills a counter of its own)
        if mc.data_ptr() != counters[j].data_ptr():
            counters[j].copy_(mc)
    words_host = words.cpu()                                                      # the ONE synchronisation of the searches
    counts = words_host[:n_jobs * n_clouds].view(n_jobs, n_clouds)                # (jobs, clouds)
    # rows with exact ties (none on jittered synthetic clouds, most rows of a real scan): the reference's order, support stage by support stage
    trees = {}
    for j, (q_pts, s_pts, q_len, s_len, r, s_stage, t) in enumerate(searches):
        n_tie = int(words_host[n_jobs * n_clouds + j])
        if n_tie > 0:
            trees[s_stage] = _ops.radius_tie_order(jobs[j][1][0], q_pts, s_pts, q_len, s_len, r, t[0], n_tie, max(int(counts[j].max()), 1),
                                                   tree=trees.get(s_stage))
    if trees:
        _ops.tie_overflow_check()              # (one more small copy on the path that already copied the stage's points: a row left behind raises)
    num_pairs = counts.shape[1] // 2
    pair_counts = counts.view(counts.shape[0], num_pairs, 2).amax(2).tolist() if counts.shape[1] % 2 == 0 else None
    out = {'points': points_list, 'lengths': lengths_list, 'neighbors': [], 'subsampling': [], 'upsampling': []}
    if normals_list is not None:
        out['normals'] = normals_list
    stage_of = {'neighbors': lambda k: k, 'subsampling': lambda k: k + 1, 'upsampling': lambda k: k}
    for j, (kind, (full, _)) in enumerate(jobs):
        width = min(full.shape[1], int(counts[j].max()))
        if pair_counts is not None and 1 < num_pairs <= 64 and min(pair_counts[j]) < width and full.is_cuda:
            # several pairs stacked: a pair processed alone would have kept only min(limit, ITS max count) columns; columns
            # beyond that are marked -1 (ignored by every consumer, unlike the padding index Ns which selects the zero row): one launch
            q_lengths = lengths_list[stage_of[kind](len(out[kind]))]
            ends, row = [], 0
            for p in range(num_pairs):
                row += int(q_lengths[2 * p] + q_lengths[2 * p + 1])
                ends.append(row)
            table = _ops.neighbor_table_trim(full, width, ends, pair_counts[j])
        else:
            table = full if width == full.shape[1] else full[:, :width].contiguous()
            if pair_counts is not None and num_pairs > 1 and min(pair_counts[j]) < width:
                q_lengths = lengths_list[stage_of[kind](len(out[kind]))]
                row = 0
                for p in range(num_pairs):
                    rows_p = int(q_lengths[2 * p] + q_lengths[2 * p + 1])
                    if pair_counts[j][p] < width:
                        if table is full:
                            table = full.clone()
                        table[row:row + rows_p, pair_counts[j][p]:] = -1
                    row += rows_p
        out[kind].append(table)
    return out


def registration_collate_fn_stack_mode(data_dicts, num_stages, voxel_size, search_radius, neighbor_limits,
                                       precompute_data=True, device='cuda', normals=False):
    """One-pair version of the reference collate: uploads the pair and builds the pyramid on the device (normals: the 'normals' list of
    precompute_data_stack_mode)."""
    if len(data_dicts) != 1:
        raise NotImplementedError('one registration pair per call (as the reference, batch_size = 1)')
    d = data_dicts[0]
    as_t = lambda a: torch.as_tensor(a)
    ref, src = as_t(d['ref_points']).float(), as_t(d['src_points']).float()
    out = {k: as_t(v).to(device) for k, v in d.items() if k not in ('ref_points', 'src_points', 'ref_feats', 'src_feats')}
    out['features'] = torch.cat((as_t(d['ref_feats']).float(), as_t(d['src_feats']).float()), 0).to(device)
    points = torch.cat((ref, src), 0).to(device)
    lengths = torch.tensor([ref.shape[0], src.shape[0]], dtype=torch.int64)
    if precompute_data:
        out.update(precompute_data_stack_mode(points, lengths, num_stages, voxel_size, search_radius, neighbor_limits, normals=normals))
    else:
        out['points'], out['lengths'] = points, lengths
    out['batch_size'] = 1
    return out


# ---- neighbour-limit calibration (the reference's calibrate_neighbors_stack_mode, utils/data.py:212-252) ----------------------------------
# The reference searches every stage with limit = hist_n (180 / 607: beyond the 64 columns a device search keeps), counts the in-radius
# points of every row of the tables and keeps the histogram of the counts.  Here the counts never become tables: one count-only search per
# stage (ops.radius_count_hist) adds straight into per-(pair, stage) histograms on the device.
def calibration_hist_n(voxel_size, search_radius):
    """Bins of the calibration histogram: the reference's bound of the voxels in a search ball (utils/data.py:217)."""
    return int(np.ceil(4 / 3 * np.pi * (search_radius / voxel_size + 1) ** 3))


def pair_slots(num_pairs, num_stages, stage):
    """Histogram row of every cloud of stage `stage`: the two clouds of pair p share row p * num_stages + stage."""
    return [(c // 2) * num_stages + stage for c in range(2 * num_pairs)]


def neighbor_histograms(points, lengths, num_stages, voxel_size, radius, hist_n=None):
    """Per pair and stage the histogram of the in-radius counts of the stage's self search (what the reference's calibration adds up per
    dataset item), for B <= 16 stacked pairs: points (N, 3) float32 on the GPU (ref0, src0, ref1, ...), lengths (2 B,) host int64.  The
    stage clouds are those of precompute_data_stack_mode; no neighbour table is allocated.  Returns host int32 tensors hist (B, num_stages,
    hist_n), dropped (B, num_stages): rows with hist_n or more in-radius points (in no bin), max_count (B, num_stages): the largest count --
    after ONE device-to-host copy (and the one of the stage sizes)."""
    if not torch.is_tensor(points) or not points.is_cuda:
        raise RuntimeError('neighbor_histograms: points must be on the GPU')
    lengths = torch.as_tensor(lengths, dtype=torch.int64).cpu()
    if lengths.numel() == 0 or lengths.numel() % 2 != 0:
        raise RuntimeError('neighbor_histograms: lengths must hold ref and src of every pair')
    hist_n = calibration_hist_n(voxel_size, radius) if hist_n is None else int(hist_n)
    num_pairs = lengths.numel() // 2
    points_list, lengths_list = stage_clouds(points, lengths, num_stages, voxel_size)
    rows, nh = num_pairs * num_stages, num_pairs * num_stages * hist_n
    words = torch.zeros((nh + rows + num_stages * 2 * num_pairs,), dtype=torch.int32, device=points.device)       # one fill, one copy
    hist, dropped, max_count = words[:nh].view(rows, hist_n), words[nh:nh + rows], words[nh + rows:].view(num_stages, 2 * num_pairs)
    for i in range(num_stages):
        cur, cl = points_list[i], lengths_list[i]
        _ops.radius_count_hist(cur, cur, cl, cl, radius, hist_n, pair_slots(num_pairs, num_stages, i), hist=hist, dropped=dropped,
                               max_count=max_count[i])
        radius *= 2
    host = words.cpu()
    return (host[:nh].view(num_pairs, num_stages, hist_n), host[nh:nh + rows].view(num_pairs, num_stages),
            host[nh + rows:].view(num_stages, num_pairs, 2).amax(2).t().contiguous())


def neighbor_limits_from_histograms(hist, keep_ratio=0.8, sample_threshold=2000):
    """The reference's stop rule and limit rule over per-pair histograms hist (pairs, num_stages, hist_n), pairs in dataset order: pairs
    are added until every stage holds MORE than sample_threshold rows; limit_i = number of bins whose cumulative count lies below keep_ratio
    of the stage's rows.  -> (limits int64 (num_stages,), pairs_used)"""
    hist = np.asarray(hist)
    total, used = np.zeros(hist.shape[1:], dtype=np.int32), 0
    for h in hist:
        total += h.astype(np.int32)
        used += 1
        if np.min(np.sum(total, axis=1)) > sample_threshold:
            break
    # integer cumulative sums against a float64 product, as numpy evaluates the reference's line (utils/data.py:246-250)
    cum_sum = np.cumsum(total.T, axis=0)
    return np.sum(cum_sum < (keep_ratio * cum_sum[total.shape[1] - 1, :]), axis=0), used


def _item_clouds(item):
    return [torch.as_tensor(item[k]).float().contiguous() for k in ('ref_points', 'src_points')]


def calibrate_with(histograms, dataset, collate_fn, num_stages, voxel_size, search_radius, keep_ratio, sample_threshold, pairs_per_call,
                   return_details):
    """The calibration loop over a histogram function (clouds, num_stages, voxel_size, radius, hist_n) -> host (hist, dropped, max_count):
    the device's below, the host's in se3et_amd.ext."""
    if collate_fn is not None and collate_fn is not registration_collate_fn_stack_mode:
        raise NotImplementedError('calibrate_neighbors_stack_mode: collate_fn must be None or se3et_amd.data.registration_collate_fn_stack_mode '
                                  '(no collate is run; with another one, call the reference\'s function over se3et_amd.ext)')
    pairs_per_call = int(pairs_per_call)
    if not 1 <= pairs_per_call <= SE3_MAX_BATCH // 2:
        raise RuntimeError('calibrate_neighbors_stack_mode: pairs_per_call %d not in [1,%d]' % (pairs_per_call, SE3_MAX_BATCH // 2))
    hist_n = calibration_hist_n(voxel_size, search_radius)
    keys = ('histograms', 'dropped', 'max_count')
    kept, total, done = {k: [] for k in keys}, np.zeros((num_stages, hist_n), dtype=np.int64), False
    for first in range(0, len(dataset), pairs_per_call):          # items are read group by group, and no further than the stopping group
        clouds = [c for i in range(first, min(first + pairs_per_call, len(dataset))) for c in _item_clouds(dataset[i])]
        group = histograms(clouds, num_stages, voxel_size, search_radius, hist_n)
        for p in range(len(clouds) // 2):        # pair by pair: what lies behind the stopping pair is dropped, whatever the group size
            for key, t in zip(keys, group):
                kept[key].append(np.asarray(t[p]))
            total += kept['histograms'][-1]
            done = int(np.min(np.sum(total, axis=1))) > sample_threshold
            if done:
                break
        if done:
            break
    details = {k: np.stack(v) if v else np.zeros((0, num_stages) + ((hist_n,) if k == 'histograms' else ()), np.int32) for k, v in kept.items()}
    limits, details['pairs_used'] = neighbor_limits_from_histograms(details['histograms'], keep_ratio, sample_threshold)
    over = [i for i in range(num_stages) if limits[i] > SE3_MAX_NEIGHBOR_LIMIT]
    if over:
        warnings.warn('calibrate_neighbors_stack_mode: stage %s: limit %s is above the %d neighbours per point (SE3_MAX_NEIGHBOR_LIMIT) that the '
                      'radius search and KPConv kernels keep' % (', '.join(map(str, over)), ', '.join(str(int(limits[i])) for i in over),
                                                                 SE3_MAX_NEIGHBOR_LIMIT))
    return (limits, details) if return_details else limits


def _device_histograms(device):
    def run(clouds, num_stages, voxel_size, radius, hist_n):
        points = torch.cat(clouds, 0).to(device)
        lengths = torch.tensor([c.shape[0] for c in clouds], dtype=torch.int64)
        return neighbor_histograms(points, lengths, num_stages, voxel_size, radius, hist_n)
    return run


def calibrate_neighbors_stack_mode(dataset, collate_fn, num_stages, voxel_size, search_radius, keep_ratio=0.8, sample_threshold=2000,
                                   use_normal=False, pairs_per_call=4, device='cuda', return_details=False):
    """The reference's calibrate_neighbors_stack_mode (utils/data.py:212-252) on the device: the per-stage neighbour limits (numpy integer
    array) that keep `keep_ratio` of the points' neighbourhoods whole, from the histograms of the in-radius counts of dataset[0], dataset[1],
    ... (item dicts with 'ref_points' / 'src_points', numpy or tensors) until every stage holds more than sample_threshold points.
    pairs_per_call items are stacked per device pass; the result does not depend on it.  collate_fn: None or this module's
    registration_collate_fn_stack_mode (no collate is run).  use_normal: accepted, without effect on the counts.  A limit above
    SE3_MAX_NEIGHBOR_LIMIT is returned as the reference returns it, with a warning.  return_details: also the dict {'pairs_used',
    'histograms' (pairs, stages, hist_n), 'dropped', 'max_count' (pairs, stages)} of the pairs that entered."""
    return calibrate_with(_device_histograms(device), dataset, collate_fn, num_stages, voxel_size, search_radius, keep_ratio,
                          sample_threshold, pairs_per_call, return_details)
