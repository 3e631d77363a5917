"""Numpy twin of the neighbour-limit calibration, written from its contract and independent of the library:

  count     per query the number of points of the SAME cloud's support with d2 = (dx*dx + dy*dy) + dz*dz < r*r, everything float32 and
            unfused (chunked brute force over all pairs); a NaN never compares below, so a point with a NaN coordinate counts for nobody
  histogram hist[slot][count] += 1 for count < hist_n; a query with count >= hist_n is DROPPED: in no bin, in no total
  stop      pairs are added in order until min over the stages of the rows in the histogram is > sample_threshold (strict)
  limit     limit_i = #{c : cumsum(hist[i])[c] < keep_ratio * sum(hist[i])}: an integer against a float64 product; an empty stage gives 0"""
import numpy as np


def counts(q, s, radius, chunk=512):
    q, s = np.asarray(q, np.float32), np.asarray(s, np.float32)
    r2 = np.float32(radius) * np.float32(radius)
    out = np.zeros((len(q),), np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        for a in range(0, len(q), chunk):
            d = q[a:a + chunk, None, :] - s[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            assert d2.dtype == np.float32
            out[a:a + chunk] = (d2 < r2).sum(1)
    return out


def count_hist(q, s, q_lengths, s_lengths, radius, hist_n, slots, num_slots, hist=None, dropped=None, max_count=None):
    """-> (hist (num_slots, hist_n), dropped (num_slots,), max_count (batch,)) int64; the ones given are the starting values."""
    hist = np.zeros((num_slots, hist_n), np.int64) if hist is None else np.array(hist, np.int64)
    dropped = np.zeros((num_slots,), np.int64) if dropped is None else np.array(dropped, np.int64)
    max_count = np.zeros((len(slots),), np.int64) if max_count is None else np.array(max_count, np.int64)
    q0 = s0 = 0
    for b, (nq, ns) in enumerate(zip(q_lengths, s_lengths)):
        for c in counts(q[q0:q0 + nq], s[s0:s0 + ns], radius).tolist():
            if c < hist_n:
                hist[slots[b], c] += 1
            else:
                dropped[slots[b]] += 1
            max_count[b] = max(max_count[b], c)
        q0, s0 = q0 + nq, s0 + ns
    return hist, dropped, max_count


def limits(hist, keep_ratio):
    out = []
    for row in np.asarray(hist).tolist():
        total, run, n = sum(row), 0, 0
        for v in row:
            run += v
            n += 1 if run < keep_ratio * total else 0
        out.append(n)
    return out


def calibrate(pair_hists, keep_ratio=0.8, sample_threshold=2000):
    """pair_hists (pairs, stages, hist_n) in dataset order -> (limits, pairs used)."""
    pair_hists = np.asarray(pair_hists, np.int64)
    total, used = np.zeros(pair_hists.shape[1:], np.int64), 0
    for h in pair_hists:
        total, used = total + h, used + 1
        if min(int(r.sum()) for r in total) > sample_threshold:
            break
    return limits(total, keep_ratio), used
