"""Drop-in for the reference's pybind module `geotransformer.ext` on HOST memory (extensions/pybind.cpp:6-18): the two functions the
collate function calls inside forked DataLoader workers (geotransformer/utils/data.py:159-209), where a GPU context is off limits.
Same signatures, same checks (CPU, contiguous, float32 / int64 -> RuntimeError as the reference's TORCH_CHECKs,
extensions/common/torch_helper.h:6-35), same results bit for bit (tests/test_host_ext.py).  The GPU pipeline
(se3et_amd.data.precompute_data_stack_mode) does not use this module."""
import ctypes

import torch

from ._lib import check, lib


def _chk(t, dtype, name):
    if not torch.is_tensor(t) or t.is_cuda:
        raise RuntimeError('%s must be a CPU tensor' % name)
    if not t.is_contiguous():
        raise RuntimeError('%s must be contiguous' % name)
    if t.dtype != dtype:
        raise RuntimeError('%s must be a %s tensor' % (name, str(dtype).replace('torch.', '')))
    return t


def grid_subsampling(points, lengths, normals, voxel_size):
    """-> [s_points (M, 3), s_lengths (B,), s_normals (M, 3)] (grid_subsampling.cpp:5-83)."""
    _chk(points, torch.float32, 'points'), _chk(lengths, torch.int64, 'lengths'), _chk(normals, torch.float32, 'normals')
    n, b = points.shape[0], lengths.shape[0]
    s_points, s_normals = torch.empty((n, 3), dtype=torch.float32), torch.empty((n, 3), dtype=torch.float32)
    s_lengths = torch.empty((b,), dtype=torch.int64)
    check(lib().se3_grid_subsample_host(points.data_ptr(), normals.data_ptr(), n, lengths.data_ptr(), b, float(voxel_size), s_points.data_ptr(),
                                        s_normals.data_ptr(), s_lengths.data_ptr()), 'se3_grid_subsample_host')
    m = int(s_lengths.sum())
    return [s_points[:m].clone(), s_lengths, s_normals[:m].clone()]


def radius_neighbors(q_points, s_points, q_lengths, s_lengths, radius):
    """-> LongTensor (Nq, max_count), rows ascending in distance, padded with Ns (radius_neighbors.cpp:5-76)."""
    _chk(q_points, torch.float32, 'q_points'), _chk(s_points, torch.float32, 's_points')
    _chk(q_lengths, torch.int64, 'q_lengths'), _chk(s_lengths, torch.int64, 's_lengths')
    nq, ns, b = q_points.shape[0], s_points.shape[0], q_lengths.shape[0]
    mc = ctypes.c_int64(0)
    args = (q_points.data_ptr(), nq, s_points.data_ptr(), ns, q_lengths.data_ptr(), s_lengths.data_ptr(), b, float(radius))
    check(lib().se3_radius_neighbors_host(*args, 0, None, ctypes.byref(mc)), 'se3_radius_neighbors_host')
    width = max(int(mc.value), 0)
    out = torch.empty((nq, width), dtype=torch.int64)
    if width > 0:
        check(lib().se3_radius_neighbors_host(*args, width, out.data_ptr(), ctypes.byref(mc)), 'se3_radius_neighbors_host')
    return out


def radius_count_hist(q_points, s_points, q_lengths, s_lengths, radius, hist_n, slots, hist=None, dropped=None, max_count=None):
    """se3et_amd.ops.radius_count_hist on host tensors (se3_radius_count_hist_host): per query the number of in-radius support points of its
    cloud, kept as the histogram of those counts.  -> (hist (num_slots, hist_n), dropped (num_slots,), max_count (batch,)) int32; the ones
    given are accumulated into."""
    _chk(q_points, torch.float32, 'q_points'), _chk(s_points, torch.float32, 's_points')
    _chk(q_lengths, torch.int64, 'q_lengths'), _chk(s_lengths, torch.int64, 's_lengths')
    slots = [int(v) for v in (slots.tolist() if torch.is_tensor(slots) else slots)]
    b, hist_n = q_lengths.shape[0], int(hist_n)
    if s_lengths.shape[0] != b or len(slots) != b:
        raise RuntimeError('radius_count_hist: q_lengths, s_lengths and slots differ in batch size')
    if hist is None:
        if not 1 <= hist_n <= 4096 or not slots or min(slots) < 0:
            raise RuntimeError('radius_count_hist: hist_n %d not in [1,4096], or no / negative slots' % hist_n)
        hist = torch.zeros((max(slots) + 1, hist_n), dtype=torch.int32)
    _chk(hist, torch.int32, 'hist')
    if hist.dim() != 2 or hist.shape[1] != hist_n:
        raise RuntimeError('radius_count_hist: hist must be (num_slots, hist_n)')
    dropped = torch.zeros((hist.shape[0],), dtype=torch.int32) if dropped is None else _chk(dropped, torch.int32, 'dropped')
    max_count = torch.zeros((b,), dtype=torch.int32) if max_count is None else _chk(max_count, torch.int32, 'max_count')
    if dropped.shape != (hist.shape[0],) or max_count.shape != (b,):
        raise RuntimeError('radius_count_hist: dropped must be (num_slots,), max_count (batch,)')
    check(lib().se3_radius_count_hist_host(q_points.data_ptr(), q_points.shape[0], s_points.data_ptr(), s_points.shape[0], q_lengths.data_ptr(),
                                           s_lengths.data_ptr(), b, float(radius), hist_n, (ctypes.c_int * b)(*slots), hist.shape[0],
                                           hist.data_ptr(), dropped.data_ptr(), max_count.data_ptr()), 'se3_radius_count_hist_host')
    return hist, dropped, max_count


def neighbor_histograms(points, lengths, num_stages, voxel_size, radius, hist_n=None):
    """se3et_amd.data.neighbor_histograms on host tensors: the stage clouds through grid_subsampling as the reference's collate chains it,
    one count call per stage.  -> hist (B, num_stages, hist_n), dropped (B, num_stages), max_count (B, num_stages), int32."""
    from . import data as _data
    _chk(points, torch.float32, 'points'), _chk(lengths, torch.int64, 'lengths')
    if lengths.numel() == 0 or lengths.numel() % 2 != 0:
        raise RuntimeError('neighbor_histograms: lengths must hold ref and src of every pair')
    hist_n = _data.calibration_hist_n(voxel_size, radius) if hist_n is None else int(hist_n)
    num_pairs = lengths.numel() // 2
    hist = torch.zeros((num_pairs * num_stages, hist_n), dtype=torch.int32)
    dropped = torch.zeros((num_pairs * num_stages,), dtype=torch.int32)
    max_count = torch.zeros((num_stages, 2 * num_pairs), dtype=torch.int32)
    for i in range(num_stages):
        if i > 0:
            voxel_size *= 2
            s_points, s_lengths = torch.empty_like(points), torch.empty_like(lengths)
            check(lib().se3_grid_subsample_host(points.data_ptr(), None, points.shape[0], lengths.data_ptr(), lengths.shape[0], float(voxel_size),
                                                s_points.data_ptr(), None, s_lengths.data_ptr()), 'se3_grid_subsample_host')
            points, lengths = s_points[:int(s_lengths.sum())], s_lengths
        if i == num_stages - 1:
            points, lengths = _data.cap_coarsest(points, lengths)
            points = points.contiguous()
        radius_count_hist(points, points, lengths, lengths, radius, hist_n, _data.pair_slots(num_pairs, num_stages, i), hist=hist,
                          dropped=dropped, max_count=max_count[i])
        radius *= 2
    return (hist.view(num_pairs, num_stages, hist_n), dropped.view(num_pairs, num_stages),
            max_count.view(num_stages, num_pairs, 2).amax(2).t().contiguous())


def calibrate_neighbors_stack_mode(dataset, collate_fn, num_stages, voxel_size, search_radius, keep_ratio=0.8, sample_threshold=2000,
                                   use_normal=False, pairs_per_call=4, device='cpu', return_details=False):
    """se3et_amd.data.calibrate_neighbors_stack_mode entirely on host memory (no GPU context: usable before any device work and inside
    worker processes); same arguments, same values."""
    from . import data as _data
    if torch.device(device).type != 'cpu':
        raise RuntimeError('ext.calibrate_neighbors_stack_mode runs on host memory (device %r: se3et_amd.data has the device path)' % (device,))

    def histograms(clouds, stages, voxel, radius, hist_n):
        return neighbor_histograms(torch.cat(clouds, 0), torch.tensor([c.shape[0] for c in clouds], dtype=torch.int64), stages, voxel, radius,
                                   hist_n)
    return _data.calibrate_with(histograms, dataset, collate_fn, num_stages, voxel_size, search_radius, keep_ratio, sample_threshold,
                                pairs_per_call, return_details)
