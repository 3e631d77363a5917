"""Cost of feature-space matching on the device (se3et_amd.feature_matching, csrc/feature_nn.hip) next to the composition the library offered
before it (profiles/feature_matching_probe.txt).

Workloads: planted unit descriptors (tests/feature_matching_twin.planted_features), resident on the device as float32:
  1 pair 5000 x 5000, C = 256;   16 such pairs in one call;   1 pair 20000 x 20000, C = 32.
Two sides, timed with device events in windows of at least --window seconds, the sides ALTERNATING window by window (a drift of the clocks
hits both), after a warm-up of each; per side the median (min .. max) of the windows' per-call times:
  (a) fused    extract_correspondences_from_feats_pairs(mutual=True): the fused search of both directions, count, scan, fill, and the one
               read-back of the list sizes;
  (b) matrix   per pair: ops.pairwise_distance, torch.min(dim=1), torch.min(dim=0) and the mask / nonzero logic of the reference's
               extract_correspondences_from_scores on exp(-d^2) (matching.py:29-61), mutual.
Also: the extraction alone (mutual, and the bilateral union whose rank pass scans nn_ref), the peak device memory each side adds, the search launches alone ((a) without extraction) against the f32-MFMA bound of
4 N M C FLOP (both directions) at 157 TFLOP/s, and whether (b) can hold 16 pairs of 20000 x 20000 (16 matrices of 1.6 GB plus the masks:
recorded as a fact from the sizes, not timed).
Run `python tools/feature_matching_probe.py [--window S] [--windows N] [--out FILE]` on the GPU box."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

WORKLOADS = [('1 x 5000 x 5000, C = 256', 1, 5000, 256), ('16 x 5000 x 5000, C = 256', 16, 5000, 256), ('1 x 20000 x 20000, C = 32', 1, 20000, 32)]
PEAK_F32_MFMA = 157e12


def matrix_route(ops, torch, refs, srcs):
    """The composition available before the fused search: the (N, M) matrix, two reductions and the reference's mask logic (mutual)."""
    out = []
    for r, s in zip(refs, srcs):
        d = ops.pairwise_distance(r, s)
        score = torch.exp(-d)
        n, m = score.shape
        ref_max, ref_arg = torch.max(score, dim=1)
        ref_mat = torch.zeros_like(score)
        ref_mat[torch.arange(n, device=score.device), ref_arg] = ref_max
        src_max, src_arg = torch.max(score, dim=0)
        src_mat = torch.zeros_like(score)
        src_mat[src_arg, torch.arange(m, device=score.device)] = src_max
        out.append(torch.nonzero(torch.logical_and(ref_mat > 0, src_mat > 0), as_tuple=True))
    return out


def window(torch, fn, seconds, calls):
    """Per-call milliseconds of one window of `calls` calls between two device events; calls is grown until a window lasts `seconds`."""
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 1e3 * seconds:
            return ms / calls, calls
        calls = max(calls + 1, int(calls * 1.3e3 * seconds / max(ms, 1e-3)))


def peak(torch, fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import feature_matching_twin as twin
    from se3et_amd import feature_matching as FM, ops
    if not torch.cuda.is_available():
        raise SystemExit('feature_matching_probe needs a GPU: times are not measured anywhere else')
    fmt = lambda t: '%9.3f (%.3f .. %.3f)' % (statistics.median(t), min(t), max(t))          # noqa: E731
    lines = ['feature_matching_probe: %s (%s); per call, ms: median (min .. max) of %d windows of >= %.1f s, the two sides alternating'
             % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, args.windows, args.window)]
    rng = np.random.default_rng(2026)
    for title, count, n, C in WORKLOADS:
        host = [twin.planted_features(rng, n, n, C, n // 2) for _ in range(count)]
        refs, srcs = [torch.from_numpy(h[0]).cuda() for h in host], [torch.from_numpy(h[1]).cuda() for h in host]
        fused = lambda: FM.extract_correspondences_from_feats_pairs(refs, srcs, mutual=True)          # noqa: E731
        search = lambda: FM.nearest_feature_pairs(refs, srcs)                                          # noqa: E731
        matrix = lambda: matrix_route(ops, torch, refs, srcs)                                          # noqa: E731
        got, want = fused(), matrix()
        same = sum(int(torch.equal(got[0][p], want[p][0]) and torch.equal(got[1][p], want[p][1])) for p in range(count))
        lines.append('%s: %d mutual correspondences; the two sides return the same lists on %d of %d pairs'
                     % (title, sum(int(c.shape[0]) for c in got[0]), same, count))
        sides = {'a': (fused, [], 1), 'b': (matrix, [], 1), 's': (search, [], 1)}
        for key in sides:                                   # warm-up, and the number of calls a window needs
            fn, times, _ = sides[key]
            _, calls = window(torch, fn, args.window, 1)
            sides[key] = (fn, times, calls)
        for _ in range(args.windows):
            for key in ('a', 'b', 's'):
                fn, times, calls = sides[key]
                ms, _ = window(torch, fn, args.window, calls)
                times.append(ms)
        ta, tb, ts = sides['a'][1], sides['b'][1], sides['s'][1]
        bound = 4.0 * count * n * n * C / PEAK_F32_MFMA * 1e3
        lines.append('  (a) fused search + mutual extraction %s   peak memory +%.1f MB' % (fmt(ta), peak(torch, fused)))
        lines.append('  (b) matrix, two min, masks, nonzero  %s   peak memory +%.1f MB' % (fmt(tb), peak(torch, matrix)))
        lines.append('      (b) / (a) = %.2f at the medians; spread of (a) %.1f %%, of (b) %.1f %% ((max - min) / median)'
                     % (statistics.median(tb) / statistics.median(ta), 100 * (max(ta) - min(ta)) / statistics.median(ta),
                        100 * (max(tb) - min(tb)) / statistics.median(tb)))
        lines.append('  search alone (3 launches, no read-back) %s   f32-MFMA bound %.3f ms: %.0f %% of it'
                     % (fmt(ts), bound, 100 * bound / statistics.median(ts)))
        # the lists alone, from the search's index arrays: count, scan, read-back, fill (the bilateral union ranks by scanning nn_ref)
        ref, src, ro, so, _nl, _ml = FM.stack_feature_pairs(refs, srcs)
        nn_src, _d, nn_ref, _e = ops.feature_nn_stack(ref, src, ro, so)
        for mode in ('mutual', 'bilateral_mask'):
            lists = lambda: ops.feature_corr_stack(nn_src, nn_ref, ro, so, mode)          # noqa: E731
            _, calls = window(torch, lists, args.window, 1)
            tl = [window(torch, lists, args.window, calls)[0] for _ in range(3)]
            lines.append('  lists alone, %-15s %s   (3 windows)' % (mode, fmt(tl)))
        del refs, srcs, got, want
        torch.cuda.empty_cache()
    total = torch.cuda.get_device_properties(0).total_memory / 2 ** 30
    need = ops.lib().se3_feature_nn_workspace_bytes(16 * 20000, 16 * 20000) + 16 * 2 * 20000 * 12
    lines.append('16 x 20000 x 20000, not timed: on side (b) one float32 matrix is %.2f GB and the 16 of a batch held at once %.1f GB (exp, '
                 'two score matrices and the masks add about 4x of one matrix while a pair is processed); side (a) needs %.1f MB of '
                 'workspace and outputs for the batch.  This device has %.0f GB.'
                 % (20000 * 20000 * 4 / 2 ** 30, 16 * 20000 * 20000 * 4 / 2 ** 30, need / 2 ** 20, total))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
