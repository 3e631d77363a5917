"""The host-side plumbing of the batched pair tools ("a list of pairs in, stacked launches, a list of results out"), once: pair_geometry,
scan_prep, icp, feature_matching, ransac, benchmark and the stacked wrappers of ops take it from here.

  device_of(device, *lists)                     the device of a call
  gpu_rows(x, dev, name, family)                the STRICT input check: a GPU tensor of the right shape and dtype, or RuntimeError
  gpu_rows_each(lst, dev, what, family)         ... of every entry of a list, named '<what> <index>'
  as_rows(x, device, cols, dtype)               the PERMISSIVE converter: anything array-like becomes (-1, cols) of dtype on the device
  upload(array, device, cols, dtype)            numpy -> device, for the numpy-in, numpy-out wrappers
  exclusive_offsets / device_offsets            [0, n0, n0 + n1, ...] as a Python list / as int64 on the device (to_device)
  lengths / stack / chunks                      stacking a chunk's tensors or joining the chunks' results, and the chunk bounds
  mask_indices(mask, counts)                    a stacked byte mask -> the list of each cloud's ascending local indices (nonzero on the device)
  transforms_of / identities                    one (4, 4) transform per pair from a tensor, an array, a list of either, or None

The two input contracts stay apart: pair ground truth, scan preparation, ICP and feature matching refuse what is not a GPU tensor of the
right dtype (gpu_rows); RANSAC and the benchmark metrics convert what they are given (as_rows)."""
import itertools

import numpy as np
import torch

from ._lib import CONSTANTS

PAIR_MAX_PAIRS = CONSTANTS['SE3_PAIR_MAX_PAIRS']          # pairs per stacked call: chunks() cuts longer lists
_FLOATS = (torch.float32, torch.float64)


def as_tensor(x):
    return x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))


def device_of(device, *lists):
    """The explicit device, else that of the first CUDA tensor in the lists, else 'cuda'."""
    if device is not None:
        return torch.device(device)
    for lst in lists:
        for v in lst:
            if torch.is_tensor(v) and v.is_cuda:
                return v.device
    return torch.device('cuda')


def gpu_rows(x, dev, name, family, cols=3, dtypes=_FLOATS):
    """x, contiguous, if it is a GPU tensor (n, cols) (cols None: any width) of one of dtypes on dev (None, or without an index: any GPU).
    name: what is checked, led by the calling function; family: what has no CPU implementation, in the caller's words."""
    if not torch.is_tensor(x):
        raise RuntimeError('%s must be a tensor on the device (the numpy wrappers upload)' % name)
    if not x.is_cuda:
        raise RuntimeError('%s must be a GPU tensor (%s has no CPU implementation)' % (name, family))
    if (dev is not None and dev.index is not None and x.device != dev) or x.dtype not in dtypes or x.dim() != 2 or x.shape[1] != (cols or x.shape[1]):
        raise RuntimeError('%s must be (n, %s) %s on %s, got %s %s on %s' % (name, cols or 'C', ' or '.join(str(d)[6:] for d in dtypes),
                                                                              dev or 'the GPU', tuple(x.shape), x.dtype, x.device))
    return x.contiguous()


def gpu_rows_each(lst, dev, what, family, cols=3, dtypes=_FLOATS):
    return [gpu_rows(x, dev, '%s %d' % (what, i), family, cols, dtypes) for i, x in enumerate(lst)]


def as_rows(x, device, cols=3, dtype=torch.float32):
    """A tensor or anything array-like as (-1, cols) (cols None: flat) of dtype on the device, contiguous."""
    return as_tensor(x).to(device=device, dtype=dtype).reshape(*((-1, cols) if cols else (-1,))).contiguous()


def upload(array, device, cols=3, dtype=None):
    """A host array on the device (None: 'cuda') as (-1, cols) (cols None: as it is).  dtype None is the rule for points: float32 stays,
    everything else becomes float64; features pass np.float32."""
    a = np.asarray(array)
    a = a.astype(dtype or (np.float32 if a.dtype == np.float32 else np.float64), copy=False)
    return torch.from_numpy(np.ascontiguousarray(a.reshape(-1, cols) if cols else a)).to(device or 'cuda')


def to_device(values, dtype, device):
    """Small host list -> device tensor through pinned memory and an asynchronous copy.  `torch.tensor(values, device=...)`
    copies from pageable memory, which makes the host wait for everything queued on the stream (a full synchronisation per
    index table)."""
    return torch.tensor(values, dtype=dtype).pin_memory().to(device, non_blocking=True)


def exclusive_offsets(counts):
    """[0, n0, n0 + n1, ..., total] as Python ints.  Plain sums: a negative count is the caller's to refuse, each in its own words."""
    return list(itertools.accumulate((int(n) for n in counts), initial=0))


def device_offsets(counts, dev):
    return to_device(exclusive_offsets(counts), torch.int64, dev)


def lengths(tensors):
    return [int(t.shape[0]) for t in tensors]


def stack(tensors, empty=None):
    """The tensors' rows in one tensor: a chunk's clouds, or the results of a call's chunks.  A single tensor is passed as it is (no copy);
    float32 next to float64 is promoted to float64; no tensor at all gives `empty`, which the callers that accept zero pairs pass."""
    if len(tensors) == 1:
        return tensors[0]
    if not tensors:
        if empty is None:
            raise ValueError('nothing to stack')
        return empty
    if any(t.dtype != tensors[0].dtype for t in tensors):
        tensors = [t.to(torch.float64) for t in tensors]
    return torch.cat(tensors, 0)


def mask_indices(mask, counts):
    """The cloud-local indices of the set bytes of a stacked mask, ascending, int64, one tensor per cloud.  The compaction is one nonzero
    on the device (which waits for its size) and one small copy of the clouds' cuts."""
    offsets = exclusive_offsets(counts)
    idx = torch.nonzero(mask).reshape(-1)
    cuts = torch.searchsorted(idx, to_device(offsets, torch.int64, mask.device)).cpu().tolist()
    return [idx[cuts[c]:cuts[c + 1]] - offsets[c] for c in range(len(counts))]


def chunks(P, limit=PAIR_MAX_PAIRS):
    """(a, b) bounds of the runs of at most `limit` pairs (the library's SE3_PAIR_MAX_PAIRS per launch) that cover P pairs."""
    for a in range(0, P, limit):
        yield a, min(P, a + limit)


def identities(P):
    """(P, 4, 4) float64 on the host."""
    return torch.eye(4, dtype=torch.float64).repeat(P, 1, 1)


def transforms_of(x, P, what, device, dtype=torch.float64, finite=False, error=ValueError):
    """(P, 4, 4) of dtype on the device from a tensor, an array, a list of either (each (4, 4)), or None for identities.  A tensor that is
    on the device already stays there (no read-back).  finite: also refuse a NaN or an infinity, which reads the values on the host.
    error: what a refusal raises (the benchmark metrics keep the RuntimeError a wrong count has always given there)."""
    if x is None:
        return identities(P).to(device=device, dtype=dtype)
    if isinstance(x, (list, tuple)):
        x = torch.stack([as_tensor(v).detach().to(device=device, dtype=dtype).reshape(4, 4) for v in x], 0) if len(x) else \
            torch.zeros((0, 4, 4), dtype=dtype, device=device)
    t = as_tensor(x).detach().to(device=device, dtype=dtype).reshape(-1, 4, 4).contiguous()
    if t.shape[0] != P:
        raise error('%s: one (4, 4) transform per pair: %d given for %d pairs' % (what, t.shape[0], P))
    if finite and not bool(torch.isfinite(t).all()):
        raise error('%s: a transform is not finite' % what)
    return t
