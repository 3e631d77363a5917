"""Tensor-level front end of the C ABI: validates tensors the way the reference extension does with TORCH_CHECK
(device / dtype / contiguity -> RuntimeError), allocates outputs with torch (device memory stays owned by
PyTorch) and launches the HIP kernels on the current torch stream."""
import ctypes
import os
import threading

import torch

from .caches import CACHE_EPOCH, Derived, Workspace, _Shared, also_clear, clear_caches, clear_weight_caches, validate_weight_caches  # noqa: F401
from ._lib import CONSTANTS, ENUMS, check, lib
from .stacking import PAIR_MAX_PAIRS, device_offsets, exclusive_offsets, to_device


# Library GEMM dispatch: through torch a GEMM with a bias epilogue goes to hipBLASLt (descriptor set-up + heuristic query,
# ~19 us of host time per call), a plain mm to rocBLAS (~7 us) once rocBLAS is the preferred BLAS -- with ~130 GEMMs per pair
# that is the largest host item.  Callers that can fold the bias into the kernel consuming the product (add+LayerNorm,
# GroupNorm) therefore call linear(x, w) without bias.  Process-wide torch setting, set on import of this package.
_HAS_BLAS_SWITCH = hasattr(torch.backends.cuda, 'preferred_blas_library')
if _HAS_BLAS_SWITCH:
    torch.backends.cuda.preferred_blas_library('cublas')          # 'cublas' = rocBLAS on ROCm
_BLAS_SWITCH_LOCK = threading.Lock()
_BIG_GEMM_FLOP = 2.0e9     # above this the hipBLASLt kernels win (KPConv GEMMs: up to 2.7x faster than rocBLAS's choice)


def mm(a, b):
    """a (M, K) @ b (K, N) through the cheaper-to-dispatch rocBLAS path, or hipBLASLt where its kernels win: the large products
    with a row-major right operand (the KPConv (P*6, 36 Cin) @ (36 Cin, Cout) products) and K <= 32.  For the dense layers
    x @ W^T (transposed view of the (N, K) weight) rocBLAS's kernels are the faster ones at every size measured
    (tools/micro/unary_gemm_backends.py: 1.0-1.4x of the HBM / MFMA bound against 1.1-2.6x)."""
    big = 2.0 * a.shape[0] * a.shape[1] * b.shape[1] > _BIG_GEMM_FLOP
    if _HAS_BLAS_SWITCH and big and (b.stride(-1) == 1 or a.shape[1] <= 32):
        with _BLAS_SWITCH_LOCK:          # the preference is process-global: host threads of `--inflight 2` must not interleave the flips
            torch.backends.cuda.preferred_blas_library('cublaslt')
            try:
                return torch.mm(a, b)
            finally:
                torch.backends.cuda.preferred_blas_library('cublas')
    if _HAS_BLAS_SWITCH and threading.active_count() > 1:
        with _BLAS_SWITCH_LOCK:          # (a small product launched while another thread holds the flipped preference would take its path)
            return torch.mm(a, b)
    return torch.mm(a, b)


# ---- dense layers on the f16 matrix cores (csrc/linear_f16.hip) --------------------------------------------------------------
# The hand-written f16 hi / lo split kernel for the inference GEMMs it wins on MI355X (tools/micro/linear_shapes.py ->
# profiles/r03_linear_shapes.txt: in_features >= 256 and >= 20 000 rows: 1.1-1.55x the library's f32-MFMA-bound kernels; the short-K layers
# are HBM bound and stay on the library, which streams them better), the library otherwise.
LINEAR_F16_MIN_ROWS, LINEAR_F16_MIN_K = 20000, 256
_linear_pieces = Derived(512, weights=True)          # (data_ptr, N, K, row stride, device) -> f16 pieces


def _linear_weight_pieces(weight, stream):
    """f16 hi / lo MFMA fragments of an (N, K) weight, kept while the weight is the same object at the same version (caches.Derived).  A
    column / row block of a Parameter (`weight[:, :k]`: the decoder's split dense layer) is keyed by its own address, shape and row stride
    and owned by its BASE tensor (the view object is a temporary)."""
    N, K = weight.shape
    owner = weight._base if weight._base is not None else weight
    key = (weight.data_ptr(), N, K, weight.stride(0), weight.device.index)
    Wp = _linear_pieces.lookup(owner, key)
    if Wp is not None:
        return Wp
    Wp = torch.empty((lib().se3_linear_weight_pieces_bytes(N, K),), dtype=torch.uint8, device=weight.device)
    w = weight.detach()
    w = w if w.is_contiguous() else w.contiguous()
    check(lib().se3_linear_split_weights_f16(w.data_ptr(), N, K, Wp.data_ptr(), stream), 'se3_linear_split_weights_f16')
    return _linear_pieces.store(owner, key, Wp, fingerprint_of=(weight,))


_stacked_weights = Derived(128, weights=True)


def stacked_weight(weight, groups):
    """(N, K) -> (N, groups * K): the weight repeated along its input dimension, so that a dense layer applied to `groups` partial results
    laid side by side along the channels returns the layer of their SUM (cross_attention_eq_stack with key-anchor groups).  Kept per weight
    version like the f16 pieces."""
    key = (weight.data_ptr(), tuple(weight.shape), int(groups), weight.device.index)
    W = _stacked_weights.lookup(weight, key)
    if W is not None:
        return W
    with torch.no_grad():
        W = torch.cat([weight.detach()] * int(groups), 1).contiguous()
    return _stacked_weights.store(weight, key, W, fingerprint_of=(weight,))


def linear_f16_ok(x, weight):
    """True when linear_f16 applies: inference, f32 GPU tensors, unit-stride rows aligned to 16 bytes, enough rows to fill the chip."""
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad):
        return False
    if not (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and weight.dim() == 2 and weight.is_contiguous()):
        return False
    K = weight.shape[1]
    rows = x.numel() // max(x.shape[-1], 1)
    return (x.shape[-1] == K and K % 32 == 0 and K >= LINEAR_F16_MIN_K and rows >= LINEAR_F16_MIN_ROWS and x.is_contiguous()
            and x.data_ptr() % 16 == 0)


def linear_f16(x, weight, bias=None, relu=False):
    """y = x W^T [+ bias] [ReLU] for x (..., K) contiguous, weight (N, K): csrc/linear_f16.hip."""
    stream = _stream()
    N, K = weight.shape
    rows = x.numel() // K
    Wp = _linear_weight_pieces(weight, stream)      # (the tensor object itself: the cache entry lives as long as it does)
    out = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
    b = None if bias is None else _req(bias.detach().contiguous(), torch.float32, 'bias', 1)
    check(lib().se3_linear_f16(x.data_ptr(), rows, K, K, Wp.data_ptr(), None if b is None else b.data_ptr(), N, 1 if relu else 0,
                               out.data_ptr(), N, stream), 'se3_linear_f16')
    return out


def dense_saturated_rows(reset=True):
    """Rows of the dense launches since the last reset whose values left the headroom of their f16-split scale (csrc/dense_norm.hip: a later
    input channel more than 2^8 times the row's first 32 values) or held NaN / Inf: clamped, counted.  One device synchronisation."""
    return int(lib().se3_debug_dense_saturated_rows(1 if reset else 0))


def attention_saturated(reset=True):
    """NaN / Inf values of K / V^T (and of the cross attention's q) that the operand splits of the f16 attention kernels clamped since the last
    reset (csrc/attention.hip: x6_split_kernel; finite values of any size are scaled, not clamped).  One device synchronisation."""
    return int(lib().se3_debug_attention_saturated(1 if reset else 0))


def linear_stream_ok(x, weight):
    """True when linear_stream applies: inference, f32 GPU tensors, unit-stride rows aligned to 16 bytes, in_features a multiple of 32."""
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad):
        return False
    if not (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and weight.dim() == 2 and weight.stride(1) == 1):
        return False
    K = weight.shape[1]
    return x.shape[-1] == K and K % 32 == 0 and x.stride(-1) == 1 and x.data_ptr() % 16 == 0 and (x.is_contiguous() or (x.dim() == 2 and x.stride(0) % 4 == 0))


def linear_stream(x, weight, bias=None, relu=False, out=None):
    """y = x W^T [+ bias] [ReLU] on the streaming f16-split kernel (csrc/dense_norm.hip, plain mode): any row count; x contiguous (..., K) or
    a 2-D view with a row stride; out: optional 2-D view (rows, N) with unit column stride to write into."""
    stream = _stream()
    N, K = weight.shape
    rows = x.numel() // K
    x_rs = x.stride(0) if (x.dim() == 2 and not x.is_contiguous()) else K
    Wp = _linear_weight_pieces(weight, stream)
    if out is None:
        out = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
        out_rs = N
    else:
        if out.dim() != 2 or out.shape[0] != rows or out.shape[1] != N or out.stride(1) != 1 or out.dtype != torch.float32:
            raise RuntimeError('linear_stream: out must be a (rows, N) float32 view with unit column stride')
        out_rs = out.stride(0)
    b = None if bias is None else _req(bias.detach().contiguous(), torch.float32, 'bias', 1)
    check(lib().se3_linear_stream(x.data_ptr(), rows, K, x_rs, Wp.data_ptr(), None if b is None else b.data_ptr(), N, 1 if relu else 0,
                                  out.data_ptr(), out_rs, stream), 'se3_linear_stream')
    return out


def linear_stream_transposed(x, weight, bias, ld=None):
    """x (A, R, K) contiguous -> (A, N, ld) with [a, :, :R] = (x[a] W^T + bias)^T: the value projection in the attention kernels' operand
    layout V^T, one launch for all anchors (columns R .. ld are left as allocated: callers pass ld = R padded rows)."""
    A, R, K = x.shape
    N = weight.shape[0]
    ld = R if ld is None else int(ld)
    stream = _stream()
    Wp = _linear_weight_pieces(weight, stream)
    out = torch.empty((A, N, ld), dtype=torch.float32, device=x.device)
    b = None if bias is None else _req(bias.detach().contiguous(), torch.float32, 'bias', 1)
    check(lib().se3_linear_stream_transposed(x.data_ptr(), A * R, K, K, Wp.data_ptr(), None if b is None else b.data_ptr(), N, R, out.data_ptr(), ld,
                                             stream), 'se3_linear_stream_transposed')
    return out


# ---- optional per-kernel timing with HIP events on the launch stream (enabled by bench.py) -----------------------------
TIMING_TAG = None             # optional tag (e.g. 'self') set by callers that want a separate bucket
KERNEL_TIMINGS = None          # dict name -> list of (start_event, end_event, algorithmic_bytes) while enabled
_TIMING_LOCK = threading.Lock()


class _timed:
    def __init__(self, name, nbytes, kind=None):
        self.name, self.nbytes, self.kind = name, nbytes, kind

    def __enter__(self):
        if KERNEL_TIMINGS is not None:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if KERNEL_TIMINGS is not None:
            self.e1.record()
            KERNEL_TIMINGS.setdefault(self.name, []).append((self.e0, self.e1, self.nbytes))
            if self.kind is not None:
                KERNEL_TIMINGS.setdefault(self.name + '/' + self.kind, []).append((self.e0, self.e1, self.nbytes))
            if TIMING_TAG is not None:
                KERNEL_TIMINGS.setdefault(self.name + '@' + TIMING_TAG, []).append((self.e0, self.e1, self.nbytes))
        return False


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream():
    """hipStream_t of torch's current stream (torch.cuda.current_stream() costs ~10 us of host time per call; the raw getter
    well under 1 us -- with ~150 launches per pair that is 1.5 ms of the host's 10 ms)."""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(t, dtype, name, ndim=None):
    if not torch.is_tensor(t):
        raise RuntimeError('%s must be a tensor' % name)
    if not t.is_cuda:
        raise RuntimeError('%s must be a GPU tensor (the SE3ET hot path has no CPU implementation)' % name)
    if t.dtype != dtype:
        raise RuntimeError('%s must be %s, got %s' % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise RuntimeError('%s must be contiguous' % name)
    if ndim is not None and t.dim() != ndim:
        raise RuntimeError('%s must have %d dims, got %d' % (name, ndim, t.dim()))
    return t


def _host_lengths(lengths, name):
    """Batch lengths live on the host (as in the reference, where they are CPU LongTensors)."""
    if torch.is_tensor(lengths):
        if lengths.dtype != torch.int64:
            raise RuntimeError('%s must be int64' % name)
        lengths = lengths.tolist()
    arr = (ctypes.c_int64 * len(lengths))(*[int(v) for v in lengths])
    return arr, len(lengths)


GRID_SEARCH_MIN_SUPPORT = 1500        # below this the exhaustive kernel is faster than building a grid


class RadiusGrid:
    """Cell-binned support cloud for repeated radius searches with one radius (csrc/radius_neighbors.hip)."""

    def __init__(self, s_points, s_lengths, radius):
        self.s_points = _req(s_points, torch.float32, 's_points', 2)
        self.lengths, self.batch = _host_lengths(s_lengths, 's_lengths')
        self.radius = float(radius)
        self.ns = s_points.shape[0]
        nbytes = lib().se3_radius_grid_workspace_bytes(self.ns, self.batch)
        self.ws = torch.empty((nbytes,), dtype=torch.uint8, device=s_points.device)
        check(lib().se3_radius_grid_build(self.s_points.data_ptr(), self.ns, self.lengths, self.batch, self.radius,
                                          self.ws.data_ptr(), nbytes, _stream()), 'se3_radius_grid_build')

    def search(self, q_points, q_lengths, limit, zeroed_max_count=None, ties=None):
        """zeroed_max_count: a (batch,) int32 device tensor the caller has already cleared (one fill for all searches of a pyramid).
        ties: None, or (tie_rows (>= Nq,) int32, tie_count (1,) int32 cleared by the caller) -- see radius_neighbors."""
        _req(q_points, torch.float32, 'q_points', 2)
        ql, nb = _host_lengths(q_lengths, 'q_lengths')
        if nb != self.batch:
            raise RuntimeError('q_lengths and s_lengths differ in batch size')
        nq = q_points.shape[0]
        out = torch.empty((nq, limit), dtype=torch.int64, device=q_points.device)
        if zeroed_max_count is not None:
            max_count = _req(zeroed_max_count, torch.int32, 'zeroed_max_count', 1)
            if max_count.shape[0] != nb or not max_count.is_contiguous():
                raise RuntimeError('radius search: zeroed_max_count must be a contiguous (batch,) int32 tensor')
        else:
            max_count = torch.empty((nb,), dtype=torch.int32, device=q_points.device)
        tr, tc = _tie_buffers(ties, nq)
        check(lib().se3_radius_neighbors_grid_ties(q_points.data_ptr(), nq, ql, self.lengths, self.ns, self.batch, self.ws.data_ptr(),
                                                   self.radius, int(limit), out.data_ptr(), max_count.data_ptr(),
                                                   1 if zeroed_max_count is not None else 0, tr, tc, _stream()),
              'se3_radius_neighbors_grid')
        return out, max_count


def _tie_buffers(ties, nq):
    if ties is None:
        return None, None
    rows, count = ties
    _req(rows, torch.int32, 'tie_rows', 1), _req(count, torch.int32, 'tie_count', 1)
    if rows.shape[0] < nq or count.shape[0] != 1:
        raise RuntimeError('radius search: tie_rows needs room for every query row, tie_count is ONE int32 word')
    return rows.data_ptr(), count.data_ptr()


def radius_neighbors(q_points, s_points, q_lengths, s_lengths, radius, limit, grid=None, zeroed_max_count=None, ties=None):
    """Returns (neighbors (Nq, limit) int64 padded with Ns, max_count (batch,) int32 device tensor: per cloud the largest
    in-radius count).  Large supports go through
    a uniform grid (pass a prebuilt RadiusGrid to share it between searches); results are identical either way.
    Exactly tied distances come in index order; `ties` = (tie_rows (>= Nq,) int32, tie_count (1,) int32, CLEARED by the caller) makes the
    search list the rows whose kept columns hold such a tie (radius_tie_order then gives them the reference's order)."""
    _req(q_points, torch.float32, 'q_points', 2)
    _req(s_points, torch.float32, 's_points', 2)
    if grid is None and s_points.shape[0] >= GRID_SEARCH_MIN_SUPPORT:
        grid = RadiusGrid(s_points, s_lengths, radius)
    if grid is not None:
        if grid.s_points.data_ptr() != s_points.data_ptr() or grid.radius != float(radius):
            raise RuntimeError('radius_neighbors: the grid was built for another support cloud / radius')
        return grid.search(q_points, q_lengths, limit, zeroed_max_count, ties)
    ql, nb = _host_lengths(q_lengths, 'q_lengths')
    sl, nb2 = _host_lengths(s_lengths, 's_lengths')
    if nb != nb2:
        raise RuntimeError('q_lengths and s_lengths differ in batch size')
    nq, ns = q_points.shape[0], s_points.shape[0]
    out = torch.empty((nq, limit), dtype=torch.int64, device=q_points.device)
    max_count = torch.empty((nb,), dtype=torch.int32, device=q_points.device)
    tr, tc = _tie_buffers(ties, nq)
    check(lib().se3_radius_neighbors_ties(q_points.data_ptr(), nq, s_points.data_ptr(), ns, ql, sl, nb, float(radius),
                                          int(limit), out.data_ptr(), max_count.data_ptr(), tr, tc, _stream()),
          'se3_radius_neighbors')
    return out, max_count


def radius_count_hist(q_points, s_points, q_lengths, s_lengths, radius, hist_n, slots, hist=None, grid=None, dropped=None, max_count=None):
    """Count-only radius search (csrc/radius_neighbors.hip: se3_radius_count_hist): per query the number of in-radius support points of its
    cloud, of which only the histogram is kept -- no neighbour table, no cap at SE3_MAX_NEIGHBOR_LIMIT.  slots: per cloud the row of `hist`
    it adds into.  Returns (hist (num_slots, hist_n), dropped (num_slots,): queries with hist_n or more, max_count (batch,): per cloud the
    largest count), int32 device tensors.  hist / dropped / max_count given: ACCUMULATED into (cleared by the caller, contiguous int32);
    otherwise fresh, with num_slots = max(slots) + 1.  grid: None takes the uniform grid above GRID_SEARCH_MIN_SUPPORT support points as
    radius_neighbors does, a RadiusGrid of the same support and radius is used as it is, False forces the exhaustive kernel; the numbers
    are the same either way."""
    _req(q_points, torch.float32, 'q_points', 2)
    _req(s_points, torch.float32, 's_points', 2)
    ql, nb = _host_lengths(q_lengths, 'q_lengths')
    sl, nb2 = _host_lengths(s_lengths, 's_lengths')
    slots = [int(v) for v in (slots.tolist() if torch.is_tensor(slots) else slots)]
    if nb != nb2 or nb != len(slots):
        raise RuntimeError('radius_count_hist: q_lengths, s_lengths and slots differ in batch size')
    hist_n = int(hist_n)
    if hist is None:
        if not 1 <= hist_n <= 4096 or not slots or min(slots) < 0:
            raise RuntimeError('radius_count_hist: hist_n %d not in [1,4096], or no / negative slots' % hist_n)
        hist = torch.zeros((max(slots) + 1, hist_n), dtype=torch.int32, device=q_points.device)
    _req(hist, torch.int32, 'hist', 2)
    num_slots = hist.shape[0]
    if hist.shape[1] != hist_n:
        raise RuntimeError('radius_count_hist: hist must be (num_slots, hist_n)')
    dropped = torch.zeros((num_slots,), dtype=torch.int32, device=q_points.device) if dropped is None else _req(dropped, torch.int32, 'dropped', 1)
    max_count = torch.zeros((nb,), dtype=torch.int32, device=q_points.device) if max_count is None else _req(max_count, torch.int32, 'max_count', 1)
    if dropped.shape[0] != num_slots or max_count.shape[0] != nb:
        raise RuntimeError('radius_count_hist: dropped must be (num_slots,), max_count (batch,)')
    if grid is None and s_points.shape[0] >= GRID_SEARCH_MIN_SUPPORT:
        grid = RadiusGrid(s_points, s_lengths, radius)
    ws = None
    if grid is not None and grid is not False:
        if grid.s_points.data_ptr() != s_points.data_ptr() or grid.radius != float(radius) or grid.batch != nb:
            raise RuntimeError('radius_count_hist: the grid was built for another support cloud / radius')
        ws = grid.ws.data_ptr()
    check(lib().se3_radius_count_hist(q_points.data_ptr(), q_points.shape[0], s_points.data_ptr(), s_points.shape[0], ql, sl, nb, float(radius),
                                      ws, hist_n, (ctypes.c_int * nb)(*slots), num_slots, hist.data_ptr(), dropped.data_ptr(),
                                      max_count.data_ptr(), _stream()), 'se3_radius_count_hist')
    return hist, dropped, max_count


# The reference's order of exactly tied distances (csrc/radius_ties.hip).  On by default: clouds without exact ties
# (every jittered synthetic configuration) pay one ballot per row in the search kernels and nothing else.
RADIUS_REFERENCE_TIES = os.environ.get('SE3_RADIUS_REFERENCE_TIES', '1') != '0'       # (0: the kernels' index order; A/B runs)


class ReferenceTree:
    """The reference's k-d tree (nanoflann, leaf size 10) of the support clouds, built on the HOST from a host copy of the points
    (se3_kdtree_build_host: structural preprocessing, 12 + ~6 bytes per point) and uploaded; walked on the GPU by radius_tie_order."""

    def __init__(self, s_points, s_lengths):
        self.s_points = _req(s_points, torch.float32, 's_points', 2)
        self.lengths, self.batch = _host_lengths(s_lengths, 's_lengths')
        self.ns = s_points.shape[0]
        host_pts = s_points.cpu()                                              # (a synchronisation: only ever reached when rows were flagged)
        cap = lib().se3_kdtree_max_bytes(self.ns, self.batch)
        host = torch.empty((cap,), dtype=torch.uint8)                          # (pageable: pinning a fresh buffer per tree costs more than the copy)
        used = ctypes.c_size_t(0)
        check(lib().se3_kdtree_build_host(host_pts.data_ptr(), self.ns, self.lengths, self.batch, host.data_ptr(), cap, ctypes.byref(used)),
              'se3_kdtree_build_host')
        self.tree = host[:int(used.value)].to(s_points.device)


def radius_tie_order(neighbors, q_points, s_points, q_lengths, s_lengths, radius, tie_rows, num_tie_rows, max_hits, tree=None):
    """Rewrites the `num_tie_rows` rows listed in tie_rows (device int32; what a search with `ties` flagged) of the (Nq, limit) table
    `neighbors` IN PLACE with the reference's order / choice of exactly tied distances.  max_hits: the search's largest in-radius count
    (host int).  tree: a ReferenceTree of the same support clouds (built when omitted).  Returns the tree."""
    if num_tie_rows <= 0:
        return tree
    _req(neighbors, torch.int64, 'neighbors', 2)
    tree = tree if tree is not None else ReferenceTree(s_points, s_lengths)
    if tree.s_points.data_ptr() != s_points.data_ptr():
        raise RuntimeError('radius_tie_order: the tree was built for another support cloud')
    ql, nb = _host_lengths(q_lengths, 'q_lengths')
    nbytes = lib().se3_radius_tie_scratch_bytes(int(num_tie_rows), int(max_hits))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=q_points.device)
    check(lib().se3_radius_neighbors_tie_order(q_points.data_ptr(), q_points.shape[0], s_points.data_ptr(), s_points.shape[0], ql, tree.lengths,
                                               nb, tree.tree.data_ptr(), float(radius), neighbors.shape[1], tie_rows.data_ptr(),
                                               int(num_tie_rows), int(max_hits), scratch.data_ptr(), nbytes, neighbors.data_ptr(), _stream()),
          'se3_radius_neighbors_tie_order')
    # the last 256 bytes of the scratch hold the number of rows that did not fit (more matches than max_hits, a tree deeper than the walk's
    # stack): they keep their index order -- callers read the word with their next synchronisation and fail loudly (tie_overflow_check)
    if not hasattr(_tie_tls, 'words'):
        _tie_tls.words = []
    _tie_tls.words.append(scratch[nbytes - 256:nbytes - 252].view(torch.int32))
    return tree


_tie_tls = threading.local()          # per host thread (= per stream): a thread only ever checks the passes it issued itself


def tie_overflow_check():
    """Raises if any row of the tie passes issued since the last check was left in index order (one small device -> host copy; a no-op when
    no tie pass ran)."""
    words = getattr(_tie_tls, 'words', None)
    if not words:
        return
    _tie_tls.words = []
    left = int(torch.cat(words).sum())
    if left:
        raise RuntimeError('radius search: %d row(s) with exactly tied distances could not be given the reference order (more matches than the '
                           'search counted, or a k-d tree deeper than %d levels)' % (left, 48))


def radius_search_reference_order(q_points, s_points, q_lengths, s_lengths, radius, limit):
    """One search with the reference's tie order: (neighbors (Nq, limit), largest in-radius count (host int)).  Two synchronisations when
    rows were flagged (the counts; the host copy of the support points for the tree), one otherwise."""
    nq = q_points.shape[0]
    flags = torch.zeros((nq + 1,), dtype=torch.int32, device=q_points.device) if RADIUS_REFERENCE_TIES else None
    ties = (flags[1:], flags[:1]) if flags is not None else None
    full, max_count = radius_neighbors(q_points, s_points, q_lengths, s_lengths, radius, limit, ties=ties)
    host = torch.cat((max_count.max().reshape(1), flags[:1])).tolist() if flags is not None else [int(max_count.max()), 0]
    if host[1] > 0:
        radius_tie_order(full, q_points, s_points, q_lengths, s_lengths, radius, flags[1:], host[1], max(host[0], 1))
        tie_overflow_check()
    return full, host[0]


def grid_subsample(points, lengths, normals, voxel_size):
    """Returns (s_points (N,3) [first sum(s_lengths) rows valid], s_normals or None, s_lengths (B,) int64 device).  `lengths` on the
    host: they sum to the rows of `points`.  `lengths` a DEVICE int64 tensor (the s_lengths of a previous call): no host synchronisation
    -- the rows of `points` are then an upper bound of their sum (se3_grid_subsample_dev)."""
    _req(points, torch.float32, 'points', 2)
    if normals is not None:
        _req(normals, torch.float32, 'normals', 2)
    if torch.is_tensor(lengths) and lengths.is_cuda:
        ld = _req(lengths.contiguous(), torch.int64, 'lengths', 1)
        n, nb, dev = points.shape[0], ld.shape[0], points.device
        ws_bytes = lib().se3_grid_subsample_workspace_bytes(n, nb)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        s_points = torch.empty((n, 3), dtype=torch.float32, device=dev)
        s_normals = torch.empty((n, 3), dtype=torch.float32, device=dev) if normals is not None else None
        s_lengths = torch.empty((nb,), dtype=torch.int64, device=dev)
        check(lib().se3_grid_subsample_dev(points.data_ptr(), normals.data_ptr() if normals is not None else None, n, ld.data_ptr(), nb,
                                           float(voxel_size), s_points.data_ptr(), s_normals.data_ptr() if s_normals is not None else None,
                                           s_lengths.data_ptr(), ws.data_ptr(), ws_bytes, _stream()), 'se3_grid_subsample_dev')
        return s_points, s_normals, s_lengths
    ln, nb = _host_lengths(lengths, 'lengths')
    n = points.shape[0]
    dev = points.device
    ws_bytes = lib().se3_grid_subsample_workspace_bytes(n, nb)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    s_points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    s_normals = torch.empty((n, 3), dtype=torch.float32, device=dev) if normals is not None else None
    s_lengths = torch.empty((nb,), dtype=torch.int64, device=dev)
    check(lib().se3_grid_subsample(points.data_ptr(), normals.data_ptr() if normals is not None else None, n, ln, nb,
                                   float(voxel_size), s_points.data_ptr(),
                                   s_normals.data_ptr() if s_normals is not None else None, s_lengths.data_ptr(),
                                   ws.data_ptr(), ws_bytes, _stream()), 'se3_grid_subsample')
    return s_points, s_normals, s_lengths


# =====================================================================================================================
# Ops whose gfx950 kernel is not bound yet run as eager torch-on-GPU chains (never on the CPU); each entry of
# INTERIM_TORCH is replaced by a C-ABI call as its kernel lands (DESIGN.md tracks the status per SURVEY row).
# =====================================================================================================================
import math

import torch.nn.functional as F

INTERIM_TORCH = set()


def _interim(fn):
    INTERIM_TORCH.add(fn.__name__)
    return fn


def _gpu(t, name):
    if not t.is_cuda:
        raise RuntimeError('%s must be a GPU tensor (the SE3ET hot path has no CPU implementation)' % name)
    return t


def _split_heads(x, h):
    return x.reshape(*x.shape[:-1], h, -1).transpose(-2, -3)


def _merge_heads(x):
    x = x.transpose(-2, -3)
    return x.reshape(*x.shape[:-2], -1)


def log_optimal_transport(scores, row_masks, col_masks, alpha, num_iterations, inf):
    """HIP: one workgroup per patch pair, score matrix in registers for all iterations (csrc/sinkhorn.hip)."""
    scores = _req(scores.contiguous(), torch.float32, 'scores', 3)
    B, R, C = scores.shape
    rm = _req(row_masks.to(torch.uint8).contiguous(), torch.uint8, 'row_masks', 2)
    cm = _req(col_masks.to(torch.uint8).contiguous(), torch.uint8, 'col_masks', 2)
    al = _req(alpha.detach().reshape(1).contiguous(), torch.float32, 'alpha')
    out = torch.empty((B, R + 1, C + 1), dtype=torch.float32, device=scores.device)
    check(lib().se3_log_sinkhorn_fwd(scores.data_ptr(), rm.data_ptr(), cm.data_ptr(), al.data_ptr(), B, R, C,
                                     int(num_iterations), float(inf), out.data_ptr(), _stream()), 'se3_log_sinkhorn_fwd')
    return out


def log_optimal_transport_bwd(grad_out, scores, row_masks, col_masks, alpha, num_iterations, inf):
    """HIP (csrc/sinkhorn.hip): gradients of log_optimal_transport with respect to (scores, alpha)."""
    scores = _req(scores.contiguous(), torch.float32, 'scores', 3)
    B, R, C = scores.shape
    g = _req(grad_out.contiguous(), torch.float32, 'grad_out', 3)
    rm = _req(row_masks.to(torch.uint8).contiguous(), torch.uint8, 'row_masks', 2)
    cm = _req(col_masks.to(torch.uint8).contiguous(), torch.uint8, 'col_masks', 2)
    al = _req(alpha.detach().reshape(1).contiguous(), torch.float32, 'alpha')
    ds = torch.empty_like(scores)
    da = torch.empty((B,), dtype=torch.float32, device=scores.device)
    check(lib().se3_log_sinkhorn_bwd(scores.data_ptr(), rm.data_ptr(), cm.data_ptr(), al.data_ptr(), g.data_ptr(), B, R, C,
                                     int(num_iterations), float(inf), ds.data_ptr(), da.data_ptr(), _stream()), 'se3_log_sinkhorn_bwd')
    return ds, da.sum().reshape(alpha.shape)


def pairwise_distance(x, y, normalized=False):
    """HIP (csrc/pairwise_distance.hip): squared distances (*, N, M) of x (*, N, C) and y (*, M, C), clamped at 0."""
    x = _req(x.contiguous(), torch.float32, 'x')
    y = _req(y.contiguous(), torch.float32, 'y')
    if x.dim() < 2 or x.dim() != y.dim() or x.shape[:-2] != y.shape[:-2] or x.shape[-1] != y.shape[-1]:
        raise RuntimeError('pairwise_distance: shapes %s and %s' % (tuple(x.shape), tuple(y.shape)))
    N, M, C = x.shape[-2], y.shape[-2], x.shape[-1]
    batch = x.numel() // max(N * C, 1) if N * C else 0
    out = torch.empty(x.shape[:-2] + (N, M), dtype=torch.float32, device=x.device)
    if C == 0:
        return out.zero_()
    check(lib().se3_pairwise_distance(x.data_ptr(), y.data_ptr(), batch, N, M, C, N * C, M * C, 1 if normalized else 0, out.data_ptr(), _stream()),
          'se3_pairwise_distance')
    return out


def add_layer_norm(hidden, residual, weight, bias, eps, hidden_bias=None):
    """HIP (csrc/rowops.hip): LayerNorm(hidden [+ hidden_bias] + residual); residual may lack leading (anchor) dims of hidden;
    hidden_bias (C,) is the bias of the linear layer that produced hidden (its GEMM then runs bias-free)."""
    hidden = _req(hidden.contiguous(), torch.float32, 'hidden')
    C = hidden.shape[-1]
    if residual.shape != hidden.shape:
        # supported broadcast: one (N, C) residual block shared by all leading (anchor) slices of hidden
        if tuple(residual.shape[-2:]) != tuple(hidden.shape[-2:]) or residual.numel() != hidden.shape[-2] * C:
            raise RuntimeError('add_layer_norm: unsupported residual broadcast %s vs %s'
                               % (tuple(residual.shape), tuple(hidden.shape)))
    residual = _req(residual.contiguous(), torch.float32, 'residual')
    rows, res_rows = hidden.numel() // C, residual.numel() // C
    out = torch.empty_like(hidden)
    check(lib().se3_add_layer_norm_fwd(hidden.data_ptr(), hidden_bias.data_ptr() if hidden_bias is not None else None,
                                       residual.data_ptr(), weight.data_ptr(), bias.data_ptr(), rows, res_rows, C, float(eps),
                                       out.data_ptr(), _stream()), 'se3_add_layer_norm_fwd')
    return out


def add_layer_norm_bwd(grad_out, hidden, residual, weight, eps, hidden_bias=None):
    """HIP (csrc/rowops.hip): gradients of add_layer_norm -> (d hidden, d residual, d weight, d bias, d hidden_bias or None)."""
    hidden = _req(hidden.contiguous(), torch.float32, 'hidden')
    g = _req(grad_out.contiguous(), torch.float32, 'grad_out')
    C = hidden.shape[-1]
    res = _req(residual.contiguous(), torch.float32, 'residual')
    rows, res_rows = hidden.numel() // C, res.numel() // C
    dh = torch.empty_like(hidden)
    if TRAINING_DETERMINISTIC:
        # per-workgroup partial sums added in order by one torch reduction (no float atomics: bit-identical runs)
        part = torch.empty((int(lib().se3_add_layer_norm_bwd_blocks(rows)), 3, C), dtype=torch.float32, device=hidden.device)
        check(lib().se3_add_layer_norm_bwd_partials(hidden.data_ptr(), hidden_bias.data_ptr() if hidden_bias is not None else None, res.data_ptr(),
                                                    weight.data_ptr(), g.data_ptr(), rows, res_rows, C, float(eps), dh.data_ptr(), part.data_ptr(),
                                                    _stream()), 'se3_add_layer_norm_bwd_partials')
        params = part.sum(0)
    else:
        params = torch.zeros((3, C), dtype=torch.float32, device=hidden.device)
        check(lib().se3_add_layer_norm_bwd(hidden.data_ptr(), hidden_bias.data_ptr() if hidden_bias is not None else None, res.data_ptr(),
                                           weight.data_ptr(), g.data_ptr(), rows, res_rows, C, float(eps), dh.data_ptr(), params.data_ptr(),
                                           _stream()), 'se3_add_layer_norm_bwd')
    dres = dh if res_rows == rows else dh.reshape(rows // res_rows, res_rows, C).sum(0)
    return dh, dres.reshape(residual.shape), params[0], params[1], (params[2] if hidden_bias is not None else None)


def gather_rows_padded(x, idx):
    """HIP: x[idx] with idx == x.shape[0] addressing an all-zero row; idx of any shape."""
    x = _req(x.contiguous(), torch.float32, 'x')
    idx = _req(idx.contiguous(), torch.int64, 'idx')
    n = x.shape[0]
    width = x.numel() // max(n, 1)
    out = torch.empty(tuple(idx.shape) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    check(lib().se3_gather_rows_padded(x.data_ptr(), idx.data_ptr(), n, idx.numel(), width, out.data_ptr(), _stream()),
          'se3_gather_rows_padded')
    return out


def anchor_max(x, dim):
    """HIP (csrc/rowops.hip): maximum over the anchor axis `dim` of a 3-D float32 tensor with 6 anchors, (A, R, C) -> (R, C) or
    (R, A, C) -> (R, C); other layouts go through torch."""
    if x.dim() != 3 or x.shape[dim] != 6 or dim not in (0, 1) or x.dtype != torch.float32 or not x.is_cuda or x.shape[2] % 4 or \
            x.stride(2) != 1 or x.stride(0) % 4 or x.stride(1) % 4 or x.data_ptr() % 16:
        return x.amax(dim)
    rows, C = x.shape[1 - dim], x.shape[2]
    out = torch.empty((rows, C), dtype=torch.float32, device=x.device)
    check(lib().se3_anchor_max(x.data_ptr(), 6, rows, C, x.stride(dim), x.stride(1 - dim), out.data_ptr(), _stream()), 'se3_anchor_max')
    return out


def neighbor_max_pool(x, idx):
    x = _req(x.contiguous(), torch.float32, 'x')
    idx = _req(idx.contiguous(), torch.int64, 'idx', 2)
    n = x.shape[0]
    width = x.numel() // max(n, 1)
    out = torch.empty((idx.shape[0],) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    check(lib().se3_neighbor_max_pool(x.data_ptr(), idx.data_ptr(), n, idx.shape[0], idx.shape[1], width, out.data_ptr(),
                                      _stream()), 'se3_neighbor_max_pool')
    return out


def neighbor_max_pool_bwd(x, idx, grad_out):
    """HIP (csrc/rowops.hip): gradient of neighbor_max_pool with respect to x (to the arg-max neighbour of every output element)."""
    x = _req(x.contiguous(), torch.float32, 'x')
    idx = _req(idx.contiguous(), torch.int64, 'idx', 2)
    g = _req(grad_out.contiguous(), torch.float32, 'grad_out')
    n = x.shape[0]
    width = x.numel() // max(n, 1)
    if idx.shape[0] == 0 or g.numel() == 0:                  # nothing pooled: no gradient (empty tensors have no address to hand to the C side)
        return torch.zeros_like(x)
    if TRAINING_DETERMINISTIC:
        bound = g.abs().max().reshape(1)
        fixed = torch.zeros(x.shape, dtype=torch.int64, device=x.device)
        dx = torch.empty_like(x)
        check(lib().se3_neighbor_max_pool_bwd_fixed(x.data_ptr(), idx.data_ptr(), g.data_ptr(), n, idx.shape[0], idx.shape[1], width,
                                                    bound.data_ptr(), fixed.data_ptr(), _stream()), 'se3_neighbor_max_pool_bwd_fixed')
        check(lib().se3_fixed_to_float(fixed.data_ptr(), fixed.numel(), bound.data_ptr(), idx.shape[0], 0, dx.data_ptr(), _stream()), 'se3_fixed_to_float')
        return dx
    dx = torch.zeros_like(x)
    check(lib().se3_neighbor_max_pool_bwd(x.data_ptr(), idx.data_ptr(), g.data_ptr(), n, idx.shape[0], idx.shape[1], width, dx.data_ptr(),
                                          _stream()), 'se3_neighbor_max_pool_bwd')
    return dx


def scatter_add_rows(g, idx, n):
    """Transpose of gather_rows_padded (its backward): out[idx[i]] += g[i] for idx[i] in [0, n), as order-independent 64-bit fixed-point sums
    (csrc/rowops.hip: scatter_add_rows_fixed_kernel; bit-identical runs).  g (m.., width..), idx (m..) -> (n, width..)."""
    g = _req(g.contiguous(), torch.float32, 'grad')
    idx = _req(idx.contiguous(), torch.int64, 'idx')
    m = idx.numel()
    width = g.numel() // max(m, 1)
    tail = tuple(g.shape[idx.dim():])
    if m == 0 or g.numel() == 0:
        return torch.zeros((n,) + tail, dtype=torch.float32, device=g.device)
    bound = g.abs().max().reshape(1)
    fixed = torch.zeros((n,) + tail, dtype=torch.int64, device=g.device)
    out = torch.empty((n,) + tail, dtype=torch.float32, device=g.device)
    check(lib().se3_scatter_add_rows_fixed(g.data_ptr(), idx.data_ptr(), n, m, width, bound.data_ptr(), fixed.data_ptr(), _stream()),
          'se3_scatter_add_rows_fixed')
    check(lib().se3_fixed_to_float(fixed.data_ptr(), fixed.numel(), bound.data_ptr(), m, 0, out.data_ptr(), _stream()), 'se3_fixed_to_float')
    return out


# one buffer per launch stream and purpose: Workspace(floor in bytes)
_ws_gn, _ws_gn_bwd = Workspace(1 << 22), Workspace(1 << 22)          # GroupNorm partial statistics
_ws_attn = Workspace(1 << 22)             # f16 hi / lo pieces of K and V^T of a stack-mode attention call
_ws_x6, _ws_emb = Workspace(1 << 24), Workspace(1 << 24)          # operand pieces of the equivariant cross attention; records of the embedding kernels
# ... that begin with arrival counters (in-kernel finalize / split reduction): zero when first used; every call leaves the counters zero
# (COUNTER_BYTES: the length of that prefix, from include/se3et_hip.h; the bytes behind it have no required content)
COUNTER_BYTES = {'_ws_dense': CONSTANTS['SE3_GN_COUNTER_BYTES'], '_ws_kpconv_split': CONSTANTS['SE3_KPCONV_SPLIT_COUNTER_BYTES'],
                 '_ws_kpconv_union_split': CONSTANTS['SE3_KPCONV_SPLIT_COUNTER_BYTES']}
_ws_dense, _ws_kpconv_split, _ws_kpconv_union_split = (Workspace(1 << 20, zeroed=True, counters=n) for n in COUNTER_BYTES.values())


def group_norm_rows(x, weight, bias, groups, eps, leaky_slope, residual, x_bias=None, segments=None):
    """HIP (csrc/rowops.hip): GroupNorm of x [+ x_bias] with statistics over all leading dims, fused residual add + LeakyReLU;
    x_bias (C,) is the bias of the linear layer that produced x (its GEMM then runs bias-free).  segments: optional row
    offsets (S + 1 host ints, rows = all leading dims flattened) of independently normalised row ranges (one per pair)."""
    x = _req(x.contiguous(), torch.float32, 'x')
    C = x.shape[-1]
    rows = x.numel() // C
    if residual is not None:
        residual = _req(residual.contiguous(), torch.float32, 'residual')
        if residual.shape != x.shape:
            raise RuntimeError('group_norm_rows: residual shape mismatch')
    ws_bytes = lib().se3_group_norm_workspace_bytes(rows, C, groups)
    stream = _stream()
    ws = _ws_gn.get(x.device, stream.value, ws_bytes)
    out = torch.empty_like(x)
    nseg = 1 if segments is None else len(segments) - 1
    check(lib().se3_group_norm_segments_fwd(x.data_ptr(), x_bias.data_ptr() if x_bias is not None else None,
                                            residual.data_ptr() if residual is not None else None, weight.data_ptr(),
                                            bias.data_ptr(), rows, C, int(groups), _i64_array(segments) if nseg > 1 else None,
                                            nseg, float(eps), 1 if leaky_slope is not None else 0, float(leaky_slope or 0.0),
                                            out.data_ptr(), ws.data_ptr(), ws.numel(), stream), 'se3_group_norm_segments_fwd')
    return out


def group_norm_rows_bwd(grad_out, x, weight, bias, groups, eps, leaky_slope, residual, x_bias=None, segments=None):
    """HIP (csrc/rowops.hip): gradients of group_norm_rows -> (dx, dweight, dbias, dresidual or None, dx_bias or None)."""
    x = _req(x.contiguous(), torch.float32, 'x')
    g = _req(grad_out.contiguous(), torch.float32, 'grad_out')
    C = x.shape[-1]
    rows = x.numel() // C
    if residual is not None:
        residual = _req(residual.contiguous(), torch.float32, 'residual')
    ws_bytes = lib().se3_group_norm_bwd_workspace_bytes(C)
    stream = _stream()
    ws = _ws_gn_bwd.get(x.device, stream.value, ws_bytes)
    nseg = 1 if segments is None else len(segments) - 1
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if residual is not None else None
    params = torch.empty((nseg, 3, C), dtype=torch.float32, device=x.device)
    check(lib().se3_group_norm_segments_bwd(x.data_ptr(), x_bias.data_ptr() if x_bias is not None else None,
                                            residual.data_ptr() if residual is not None else None, weight.data_ptr(), bias.data_ptr(),
                                            g.data_ptr(), rows, C, int(groups), _i64_array(segments) if nseg > 1 else None, nseg, float(eps),
                                            1 if leaky_slope is not None else 0, float(leaky_slope or 0.0), dx.data_ptr(),
                                            dres.data_ptr() if dres is not None else None, params.data_ptr(), ws.data_ptr(), ws.numel(),
                                            stream), 'se3_group_norm_segments_bwd')
    params = params.sum(0) if nseg > 1 else params[0]
    return dx, params[0], params[1], dres, (params[2] if x_bias is not None else None)


KPCONV_SPLIT = True           # few-tile layers split their input channels over workgroups (False: A/B runs)


def _check_counters(status, what, ws):
    """check() for the calls whose workspace begins with arrival counters: a failed or rejected call may leave them non-zero (every later call on
    the stream would then finalize at the wrong arrival), so the workspace is cleared before the error is raised."""
    if status != 0 and ws is not None:
        ws.zero_()
    check(status, what)


class Pending:
    """An activation in its pending form: `raw` (rows.., C) float32 plus up to two stages v -> lrelu(v * scale + shift, slope) that its
    consumer applies while loading it (the GroupNorm [+ LeakyReLU] of the producer, reduced to per-(segment, channel) affine tables by
    group_norm_stats / dense_norm).  `affines`: list of (nseg, 2, C) tensors; `slopes`: list of floats (1.0 = no LeakyReLU)."""
    __slots__ = ('raw', 'affines', 'slopes', 'segments')

    def __init__(self, raw, affines, slopes, segments):
        self.raw, self.affines, self.slopes, self.segments = raw, list(affines), list(slopes), segments

    def then(self, affine, slope):
        return Pending(self.raw, self.affines + [affine], self.slopes + [slope], self.segments)


class BlockedFeatures:
    """(points, 6, C) features in a layout a fused KPConv kernel reads whole cache lines / rows from (group_norm_apply(blocked=True) writes
    it, kpconv_inter_so3 reads it); `plain()` is the ordinary tensor.
    kind 1: [point][C / 16][anchor pair][16 channels][2 anchors] (csrc/kpconv_mfma.hip: per-lane gathers of 8 bytes)
    kind 2: [point][C / 8][6 anchors][8 channels]                (csrc/kpconv_union.hip: a point's 8-channel chunk is 192 contiguous bytes)"""
    __slots__ = ('data', 'shape', 'kind', 'amax', 'amax_tag')

    def __init__(self, data, shape, kind=1, amax=None, amax_tag=None):
        # amax: one-element device tensor holding the largest |value| (written by the apply pass that produced `data`), or None: the fused
        # kernels scale the features by a power of two from it before their f16 split (csrc/kpconv_sums.h: x_split_scale)
        self.data, self.shape, self.kind, self.amax, self.amax_tag = data, tuple(shape), kind, amax, amax_tag

    def plain(self):
        n, a, c = self.shape
        if self.kind == 2:
            return self.data.view(n, c // 8, a, 8).permute(0, 2, 1, 3).reshape(n, a, c)
        return self.data.view(n, c // 16, a // 2, 16, 2).permute(0, 2, 4, 1, 3).reshape(n, a, c)


# The union-staged fused KPConv (csrc/kpconv_union.hip), wherever a spatial order of the query points is registered (se3et_amd/data.py):
# SE3_KPCONV_UNION = 0 never; 1 (default) where it measured faster than the per-lane-gather kernel alone on the GPU (output widths <= 64 of the
# stride-1 layers and the first strided one: profiles/r05_kpconv_union_check.txt: 18-26 % on those layers with the 128-row cap); all: every
# layer.  With the order and plan launches the forward as a whole reads the same or slightly higher in alternating bench runs (488.1 / 488.6
# against 487.7 / 483.0 pairs/s; with the first form's 160-row cap it read 1-1.5 % lower and was off).
_KPCONV_UNION_ENV = os.environ.get('SE3_KPCONV_UNION', '1')
KPCONV_UNION = _KPCONV_UNION_ENV != '0'
KPCONV_UNION_ALL = _KPCONV_UNION_ENV == 'all'
KPCONV_UNION_MIN_POINTS = 24000           # stage-0 points of a pyramid from which the pyramid builder registers orders (single pairs stay on the gather kernel)


_amax_rings = {}


def _amax_slot(device, stream):
    """A zeroed device word for one apply pass to atomicMax the largest magnitude of its output into: taken from a per-stream ring of 4096
    words that is cleared (one fill, in stream order) every time it wraps."""
    key = (device, stream.value)
    ring = _amax_rings.get(key)
    if ring is None:
        ring = _amax_rings[key] = [torch.zeros((4096,), dtype=torch.float32, device=device), 0, 0]
    if ring[1] == 4096:
        ring[0].zero_()
        ring[1] = 0
        ring[2] += 1                     # generation: words handed out before the wrap are no longer their owners'
    slot = ring[0][ring[1]:ring[1] + 1]
    ring[1] += 1
    return slot, (ring, ring[2], ring[1] - 1)


def _amax_live(blocked):
    """The magnitude word of a BlockedFeatures, or None when the ring it came from has wrapped since (an object kept across a wrap: its word
    was zeroed and may describe another tensor by now -- the kernels then split the features as they are)."""
    if blocked.amax is None or blocked.amax_tag is None:
        return blocked.amax
    ring, gen, pos = blocked.amax_tag
    return blocked.amax if ring[2] == gen else None        # (the wrap zeroes the WHOLE ring: every word of an earlier generation is dead)


def _kpconv_union_pays(Cin, Cout, same_cloud):
    return KPCONV_UNION_ALL or (Cout <= 64 and (same_cloud or Cout <= 32))


def dense_norm_ok(x, weight, groups):
    """True when the fused dense layer + GroupNorm statistics kernel (csrc/dense_norm.hip) takes this layer."""
    raw = x.raw if isinstance(x, Pending) else x
    if torch.is_grad_enabled() and (raw.requires_grad or weight.requires_grad):
        return False
    N, K = weight.shape
    return (raw.is_cuda and raw.dtype == torch.float32 and weight.dtype == torch.float32 and weight.is_contiguous() and raw.is_contiguous()
            and raw.shape[-1] == K and 32 <= K <= 1024 and K & (K - 1) == 0 and (N in (32, 64, 128) or N % 256 == 0) and N % groups == 0
            and N // groups in (1, 2, 4, 8, 16, 32) and N <= 4096
            and raw.data_ptr() % 16 == 0)


def dense_norm(x, weight, linear_bias, norm_weight, norm_bias, groups, eps, segments=None):
    """HIP (csrc/dense_norm.hip): the dense layer of a unary block with the GroupNorm statistics of its output taken from the accumulators.
    x: a tensor or a Pending (its stages are applied on load).  -> Pending(raw = T(x) W^T without the bias, [affine of GroupNorm(raw + bias)],
    slope left to the caller via .slopes[-1])."""
    pend = x if isinstance(x, Pending) else Pending(x, [], [], segments)
    raw = _req(pend.raw, torch.float32, 'x')
    if len(pend.affines) > 2:
        raise RuntimeError('dense_norm: at most two pending stages')
    segments = pend.segments if segments is None else segments
    N, K = weight.shape
    rows = raw.numel() // K
    stream = _stream()
    Wp = _linear_weight_pieces(weight, stream)
    nseg = 1 if segments is None else len(segments) - 1
    out = torch.empty(raw.shape[:-1] + (N,), dtype=torch.float32, device=raw.device)
    affine = torch.empty((nseg, 2, N), dtype=torch.float32, device=raw.device)
    ws = _ws_dense.get(raw.device, stream.value, lib().se3_dense_norm_workspace_bytes(int(groups)))
    aa = pend.affines + [None, None]
    sl = pend.slopes + [1.0, 1.0]
    with _timed('dense', 4.0 * rows * (K + N)):           # (bench.py roofline_dense: activations read + product written)
        _check_counters(lib().se3_dense_norm_fwd(raw.data_ptr(), rows, K, aa[0].data_ptr() if aa[0] is not None else None, float(sl[0]),
                                       aa[1].data_ptr() if aa[1] is not None else None, float(sl[1]), Wp.data_ptr(), N,
                                       linear_bias.data_ptr() if linear_bias is not None else None, norm_weight.data_ptr(), norm_bias.data_ptr(),
                                       int(groups), float(eps), _i64_array(segments) if nseg > 1 else None, nseg, out.data_ptr(),
                                       affine.data_ptr(), ws.data_ptr(), ws.numel(), stream), 'se3_dense_norm_fwd', ws)
    return Pending(out, [affine], [1.0], segments)


def dense_stats(x, weight, linear_bias, norm_weight, norm_bias, groups, eps, segments=None):
    """HIP (csrc/dense_norm.hip, statistics-only mode): the affine table (nseg, 2, N) of GroupNorm(T(x) W^T + linear_bias) -- the GEMM runs and
    is reduced to its statistics, the product is never written.  x: a tensor or a Pending (at most two stages)."""
    pend = x if isinstance(x, Pending) else Pending(x, [], [], segments)
    raw = _req(pend.raw, torch.float32, 'x')
    if len(pend.affines) > 2:
        raise RuntimeError('dense_stats: at most two pending stages')
    segments = pend.segments if segments is None else segments
    N, K = weight.shape
    rows = raw.numel() // K
    stream = _stream()
    Wp = _linear_weight_pieces(weight, stream)
    nseg = 1 if segments is None else len(segments) - 1
    affine = torch.empty((nseg, 2, N), dtype=torch.float32, device=raw.device)
    ws = _ws_dense.get(raw.device, stream.value, lib().se3_dense_norm_workspace_bytes(int(groups)))
    aa = pend.affines + [None, None]
    sl = pend.slopes + [1.0, 1.0]
    with _timed('dense', 4.0 * rows * K):                 # (statistics only: the activations read, nothing written)
        _check_counters(lib().se3_dense_norm_fwd(raw.data_ptr(), rows, K, aa[0].data_ptr() if aa[0] is not None else None, float(sl[0]),
                                       aa[1].data_ptr() if aa[1] is not None else None, float(sl[1]), Wp.data_ptr(), N,
                                       linear_bias.data_ptr() if linear_bias is not None else None, norm_weight.data_ptr(), norm_bias.data_ptr(),
                                       int(groups), float(eps), _i64_array(segments) if nseg > 1 else None, nseg, None,
                                       affine.data_ptr(), ws.data_ptr(), ws.numel(), stream), 'se3_dense_norm_fwd (statistics only)', ws)
    return affine


_nonzero_norms = Derived(256, weights=True)


def norm_weight_nonzero(weight):
    """True when no entry of a GroupNorm weight is zero (one host synchronisation per weight version): dense_residual's shortcut form divides
    by the shortcut norm's scale."""
    key = (weight.data_ptr(), weight.device.index, tuple(weight.shape))
    hit = _nonzero_norms.lookup(weight, key)
    return hit if hit is not None else _nonzero_norms.store(weight, key, bool((weight.detach().abs() > 1e-30).all()))


def dense_residual(x, weight, affine, residual=None, shortcut=None, final_slope=1.0, segments=None):
    """HIP (csrc/dense_norm.hip, final modes): out = lrelu( (T(x) W^T) * scale + shift + R ) with (scale, shift) = `affine` from dense_stats on
    the same operands; R = `residual` (rows.., N) tensor, or the shortcut layer `shortcut` = (x2 tensor, weight2 (N, K2), affine2) evaluated in
    the same kernel, or nothing.  The tail of a bottleneck block with only its output written."""
    pend = x if isinstance(x, Pending) else Pending(x, [], [], segments)
    raw = _req(pend.raw, torch.float32, 'x')
    if len(pend.affines) > 2:
        raise RuntimeError('dense_residual: at most two pending stages')
    segments = pend.segments if segments is None else segments
    N, K = weight.shape
    rows = raw.numel() // K
    stream = _stream()
    Wp = _linear_weight_pieces(weight, stream)
    nseg = 1 if segments is None else len(segments) - 1
    if tuple(affine.shape) != (nseg, 2, N):
        raise RuntimeError('dense_residual: affine table %s for %d segment(s) x %d features' % (tuple(affine.shape), nseg, N))
    out = torch.empty(raw.shape[:-1] + (N,), dtype=torch.float32, device=raw.device)
    x2p = wp2 = aff2 = resp = None
    K2 = 0
    if shortcut is not None:
        x2, w2, aff2t = shortcut
        x2 = _req(x2, torch.float32, 'shortcut input')
        K2 = w2.shape[1]
        if w2.shape[0] != N or x2.numel() != rows * K2 or tuple(aff2t.shape) != (nseg, 2, N) or residual is not None:
            raise RuntimeError('dense_residual: shortcut layer shapes')
        x2p, wp2, aff2 = x2.data_ptr(), _linear_weight_pieces(w2, stream).data_ptr(), aff2t.data_ptr()
    elif residual is not None:
        residual = _req(residual, torch.float32, 'residual')
        if residual.numel() != rows * N:
            raise RuntimeError('dense_residual: residual shape %s' % (tuple(residual.shape),))
        resp = residual.data_ptr()
    aa = pend.affines + [None, None]
    sl = pend.slopes + [1.0, 1.0]
    with _timed('dense', 4.0 * rows * (K + K2 + N + (N if resp is not None else 0))):
        check(lib().se3_dense_residual_fwd(raw.data_ptr(), rows, K, aa[0].data_ptr() if aa[0] is not None else None, float(sl[0]),
                                           aa[1].data_ptr() if aa[1] is not None else None, float(sl[1]), Wp.data_ptr(), affine.data_ptr(),
                                           x2p, K2, wp2, aff2, resp, N, float(final_slope), _i64_array(segments) if nseg > 1 else None, nseg,
                                           out.data_ptr(), stream), 'se3_dense_residual_fwd')
    return out


def group_norm_stats(x, weight, bias, groups, eps, x_bias=None, segments=None):
    """HIP (csrc/rowops.hip): the affine table (nseg, 2, C) of GroupNorm over T(x) (x: tensor, or Pending with ONE stage)."""
    pend = x if isinstance(x, Pending) else Pending(x, [], [], segments)
    raw = _req(pend.raw.contiguous(), torch.float32, 'x')
    if len(pend.affines) > 1:
        raise RuntimeError('group_norm_stats: at most one pending stage')
    segments = pend.segments if segments is None else segments
    C = raw.shape[-1]
    rows = raw.numel() // C
    stream = _stream()
    nseg = 1 if segments is None else len(segments) - 1
    affine = torch.empty((nseg, 2, C), dtype=torch.float32, device=raw.device)
    ws = _ws_dense.get(raw.device, stream.value, lib().se3_group_norm_stats_workspace_bytes(C))
    pa = pend.affines[0] if pend.affines else None
    _check_counters(lib().se3_group_norm_stats(raw.data_ptr(), pa.data_ptr() if pa is not None else None, float(pend.slopes[0]) if pa is not None else 1.0,
                                     x_bias.data_ptr() if x_bias is not None else None, weight.data_ptr(), bias.data_ptr(), rows, C,
                                     int(groups), _i64_array(segments) if nseg > 1 else None, nseg, float(eps), affine.data_ptr(),
                                     ws.data_ptr(), ws.numel(), stream), 'se3_group_norm_stats', ws)
    return affine


def group_norm_apply(x, residual=None, final_slope=1.0, blocked=False):
    """HIP (csrc/rowops.hip): a Pending made concrete: lrelu_f(T_b(T_a(raw)) + R), R = a tensor, a Pending with one stage (slope 1), or None.
    blocked=True (raw (points, 6, C), C % 16 == 0): the result in the fused KPConv's gather layout, as BlockedFeatures."""
    if not x.affines or len(x.affines) > 2:
        raise RuntimeError('group_norm_apply: one or two pending stages')
    raw = _req(x.raw, torch.float32, 'x')
    C = raw.shape[-1]
    rows = raw.numel() // C
    res, res_aff = None, None
    if isinstance(residual, Pending):
        if len(residual.affines) != 1 or residual.slopes[0] != 1.0:
            raise RuntimeError('group_norm_apply: the residual may carry one stage without LeakyReLU')
        res, res_aff = _req(residual.raw, torch.float32, 'residual'), residual.affines[0]
    elif residual is not None:
        res = _req(residual.contiguous(), torch.float32, 'residual')
    if res is not None and res.shape != raw.shape:
        raise RuntimeError('group_norm_apply: residual shape mismatch')
    segments = x.segments
    nseg = 1 if segments is None else len(segments) - 1
    out = torch.empty_like(raw)
    aa = x.affines + [None]
    sl = x.slopes + [1.0]
    stream = _stream()
    amax, amax_tag = _amax_slot(raw.device, stream) if blocked else (None, None)
    check(lib().se3_group_norm_apply_amax(raw.data_ptr(), aa[0].data_ptr(), float(sl[0]), aa[1].data_ptr() if aa[1] is not None else None, float(sl[1]),
                                          res.data_ptr() if res is not None else None, res_aff.data_ptr() if res_aff is not None else None,
                                          float(final_slope), rows, C, _i64_array(segments) if nseg > 1 else None, nseg, int(blocked),
                                          out.data_ptr(), amax.data_ptr() if amax is not None else None, stream),
          'se3_group_norm_apply')
    return BlockedFeatures(out, raw.shape, int(blocked), amax, amax_tag) if blocked else out


_host_tables = Derived(256, weights=True)


def _host_table(t, dtype):
    """Constant module tables (kernel points, permutation indices) as host arrays, cached per view and owned by the module's parameter /
    buffer (for a view, its base)."""
    base = t._base if t._base is not None else t
    key = (t.data_ptr(), t.shape, t.stride(), dtype)
    hit = _host_tables.lookup(base, key)
    return hit if hit is not None else _host_tables.store(base, key, t.detach().to('cpu', dtype).contiguous())


# KPConv path: True / 'auto' = the fused matrix-core kernel (csrc/kpconv_mfma.hip) where the channel counts allow (Cin % 8, Cout % 32),
# 'sums' = the same contraction with the orbit sums written to HBM by a separate gather kernel (A/B runs), False = the round-1 path (slot
# sums G in HBM + library f32 GEMM; also the fallback for other channel counts / slot tables and the operand of the backward pass).
# All paths agree to f32 round-off (tests/test_gpu_ops.py::test_kpconv_matrix_core_path_has_f32_accuracy).
KPCONV_MATRIX_CORE = {'mfma': True, 'fused': True, 'sums': 'sums', 'gemm': False}.get(os.environ.get('SE3_KPCONV_PATH', 'auto'), 'auto')


def _kpconv_use_matrix_core(Cin, Cout, P):
    return True if KPCONV_MATRIX_CORE == 'auto' else KPCONV_MATRIX_CORE


_BUILTIN_KIDX = [[0, 1, 1, 1, 1, 2], [1, 0, 1, 2, 1, 1], [1, 1, 0, 1, 2, 1], [1, 2, 1, 0, 1, 1], [1, 1, 2, 1, 0, 1], [2, 1, 1, 1, 1, 0],
                 [3, 3, 3, 4, 4, 4], [3, 4, 3, 3, 4, 4], [3, 4, 4, 3, 3, 4], [3, 3, 4, 4, 3, 4], [4, 3, 3, 4, 4, 3], [4, 4, 3, 3, 4, 3],
                 [4, 4, 4, 3, 3, 3], [4, 3, 4, 4, 3, 3], [5, 5, 5, 5, 5, 5]]
_BUILTIN_RIDX = [[0, 3, 3, 3, 3, 5], [1, 0, 4, 5, 2, 1], [2, 2, 0, 4, 5, 4], [3, 5, 2, 0, 4, 3], [4, 4, 5, 2, 0, 2], [5, 1, 1, 1, 1, 0]]
def _builtin_slot_tables(kt, rt):
    """True when the module's (k, r) -> s and (a, r) -> t tables are the SE3ET configuration compiled into the matrix-core kernel.  The
    verdict is an attribute of the host copies `_host_table` returns, so it lives and dies with their cache entries (a verdict keyed by the
    host tensors' addresses could outlive them and be inherited by other tables placed at the same addresses)."""
    hit = getattr(kt, '_se3_builtin', None)
    if hit is None or hit[0] is not rt:
        hit = (rt, kt.tolist() == _BUILTIN_KIDX and rt.tolist() == _BUILTIN_RIDX)
        kt._se3_builtin = hit
    return hit[1]


_kpconv_pieces = Derived(256, weights=True)          # (data_ptr, Cin, Cout, device) -> f16 pieces


def _kpconv_weight_pieces(weights, Cin, Cout, stream):
    """f16 hi / lo MFMA fragments of KPConvInterSO3.weights (se3_kpconv_split_weights_f16).  Without autograd (inference) they are kept per
    weight object and version (caches.Derived); under autograd the fragments are rebuilt per call (3 small launches)."""
    w = _req(weights.detach().contiguous(), torch.float32, 'weights', 4)
    cacheable = not torch.is_grad_enabled() and w.data_ptr() == weights.data_ptr()
    key = (w.data_ptr(), Cin, Cout, w.device.index)
    if cacheable:
        Wp = _kpconv_pieces.lookup(weights, key)
        if Wp is not None:
            return Wp
    Wp = torch.empty((lib().se3_kpconv_weight_pieces_bytes(Cin, Cout),), dtype=torch.uint8, device=w.device)
    check(lib().se3_kpconv_split_weights_f16(w.data_ptr(), Cin, Cout, Wp.data_ptr(), stream), 'se3_kpconv_split_weights_f16')
    if cacheable:
        _kpconv_pieces.store(weights, key, Wp, fingerprint_of=(weights,))
    return Wp


def kpconv_slot_sums(x, q_pts, s_pts, idx, kernel_points, kidx, ridx, sigma):
    """HIP (csrc/kpconv_so3.hip): G (P * 6, 36 Cin), the slot-summed neighbourhood features with out = G @ weights.reshape(36 Cin, Cout)."""
    x = _req(x.contiguous(), torch.float32, 'x', 3)
    q_pts, s_pts = _req(q_pts.contiguous(), torch.float32, 'q_pts', 2), _req(s_pts.contiguous(), torch.float32, 's_pts', 2)
    idx = _req(idx.contiguous(), torch.int64, 'neighb_inds', 2)
    P, NN = idx.shape
    Ns, A, Cin = x.shape
    kp, kt, rt = _host_table(kernel_points, torch.float32), _host_table(kidx, torch.int64), _host_table(ridx, torch.int64)
    G = torch.empty((P * 6, 36 * Cin), dtype=torch.float32, device=x.device)
    check(lib().se3_kpconv_so3_gather(q_pts.data_ptr(), s_pts.data_ptr(), idx.data_ptr(), x.data_ptr(), kp.data_ptr(),
                                      kt.data_ptr(), rt.data_ptr(), float(sigma), P, Ns, NN, Cin, G.data_ptr(), _stream()),
          'se3_kpconv_so3_gather')
    return G


def kpconv_inter_so3_bwd(grad_out, x, q_pts, s_pts, idx, kernel_points, weights, kidx, ridx, sigma, need_x=True, need_w=True):
    """Gradients of kpconv_inter_so3 with respect to (x, weights): two library GEMMs on the slot-sum matrix (dW = G^T dout, dG = dout W^T)
    and the HIP transpose of the gather (csrc/kpconv_so3.hip: kpconv_scatter_kernel)."""
    x = _req(x.contiguous(), torch.float32, 'x', 3)
    q_pts, s_pts = _req(q_pts.contiguous(), torch.float32, 'q_pts', 2), _req(s_pts.contiguous(), torch.float32, 's_pts', 2)
    idx = _req(idx.contiguous(), torch.int64, 'neighb_inds', 2)
    P, NN = idx.shape
    Ns, A, Cin = x.shape
    Cout = weights.shape[-1]
    if P == 0:                                                   # no query points: zero gradients (empty tensors have no address for the C side)
        return (torch.zeros_like(x) if need_x else None), (torch.zeros_like(weights) if need_w else None)
    d2 = _req(grad_out.contiguous(), torch.float32, 'grad_out').reshape(P * 6, Cout)
    dx = dw = None
    if need_w:
        G = kpconv_slot_sums(x, q_pts, s_pts, idx, kernel_points, kidx, ridx, sigma)
        dw = mm(G.t(), d2).view(6, 6, Cin, Cout)
        del G
    if need_x:
        kp, kt, rt = _host_table(kernel_points, torch.float32), _host_table(kidx, torch.int64), _host_table(ridx, torch.int64)
        W2 = weights.detach().reshape(36 * Cin, Cout)              # as a dense layer's (N = 36 Cin, K = Cout) weight: dG = dout W2^T
        if Cout % 32 == 0 and d2.data_ptr() % 16 == 0 and P * 6 * max(Cout, 36 * Cin) < 2 ** 31:
            # round 5: on the f16-split streaming kernel (csrc/dense_norm.hip; f32 accurate, ~2x the library's f32-MFMA rate on these shapes);
            # its weight pieces are cached per weight version like every dense layer's (keyed on the view's address / shape, owned by `weights`)
            with torch.no_grad():           # (the view's _base must be `weights` itself -- the cache entry's owner; a view of weights.detach() is owned by a temporary)
                Wv = weights.view(36 * Cin, Cout) if weights.is_contiguous() else W2.contiguous()
            dG = linear_stream(d2, Wv)
        else:
            dG = mm(d2, W2.t())
        if KPCONV_BACKWARD_DETERMINISTIC:
            # order-independent sums (64-bit fixed point at a scale from max |dG|): bit-identical runs (csrc/kpconv_so3.hip)
            # (an upper bound of |dG| = |dout W^T| from the small operands -- max |dout| times the largest absolute row sum of W -- instead of a pass
            # over the (6 P, 36 Cin) product: the scale only has to prevent overflow)
            # (two fused max-magnitude reductions and Cout as the row length -- |dG| <= max |dout| max |W| Cout -- instead of abs / max / abs /
            #  row sums / max: 3 launches for 6 per layer; the looser bound costs the 64-bit sums a few of their ~39 spare bits)
            bound = ((torch.linalg.vector_norm(d2, float('inf')) * torch.linalg.vector_norm(W2, float('inf'))).mul_(float(Cout)).reshape(1)
                     if d2.numel() and W2.numel() else d2.new_zeros(1))
            fixed = torch.zeros(x.shape, dtype=torch.int64, device=x.device)
            dx = torch.empty_like(x)
            check(lib().se3_kpconv_so3_gather_bwd_fixed(q_pts.data_ptr(), s_pts.data_ptr(), idx.data_ptr(), dG.data_ptr(), kp.data_ptr(),
                                                        kt.data_ptr(), rt.data_ptr(), float(sigma), P, Ns, NN, Cin, bound.data_ptr(),
                                                        fixed.data_ptr(), _stream()), 'se3_kpconv_so3_gather_bwd_fixed')
            check(lib().se3_kpconv_fixed_to_float(fixed.data_ptr(), fixed.numel(), bound.data_ptr(), P, dx.data_ptr(), _stream()),
                  'se3_kpconv_fixed_to_float')
        else:
            dx = torch.zeros_like(x)
            check(lib().se3_kpconv_so3_gather_bwd(q_pts.data_ptr(), s_pts.data_ptr(), idx.data_ptr(), dG.data_ptr(), kp.data_ptr(),
                                                  kt.data_ptr(), rt.data_ptr(), float(sigma), P, Ns, NN, Cin, dx.data_ptr(), _stream()),
                  'se3_kpconv_so3_gather_bwd')
    return dx, dw


KPCONV_BACKWARD_DETERMINISTIC = os.environ.get('SE3_KPCONV_BWD', 'fixed') != 'float'      # 64-bit fixed-point scatter (bit-identical runs); 'float': hardware float atomics
TRAINING_DETERMINISTIC = KPCONV_BACKWARD_DETERMINISTIC      # the other scatter-adds of the training step (max-pool, row gather, LayerNorm parameter sums) follow the same switch
_neighbor_tables = Derived(64, share=False)          # stream -> (key, table) of the last geometry seen there


def _kpconv_neighbor_table(q_pts, s_pts, idx, kernel_points, sigma, P, Ns, NN, stream):
    """The neighbour table of the fused KPConv (valid neighbours compacted + 16 orbit weights each): a function of the geometry only, so the
    layers of a pyramid stage (same query / support points, neighbour indices, kernel points and extent) share it.  Kept per stream for the
    LAST geometry seen (the same tensor objects at the same versions)."""
    kpd = _req(kernel_points.detach().contiguous(), torch.float32, 'kernel_points', 2)
    # (the kernel points enter by VALUE -- the bytes of their cached host copy: the layers of a stage own different Parameter objects holding
    # the same 15 points, and shared one table only by accident of the cache's depth before round 5: 10 -> 7 table launches per forward)
    kph = _host_table(kernel_points, torch.float32)
    kp_key = getattr(kph, '_se3_bytes', None)
    if kp_key is None:
        kp_key = kph.numpy().tobytes()
        kph._se3_bytes = kp_key
    key = (kp_key, float(sigma), P, Ns, NN)
    hit = _neighbor_tables.lookup((q_pts, s_pts, idx), stream.value)
    if hit is not None and hit[0] == key:
        return hit[1]
    nbytes = lib().se3_kpconv_neighbor_table_bytes(P, NN)
    tab = torch.empty((nbytes,), dtype=torch.uint8, device=q_pts.device)
    check(lib().se3_kpconv_neighbor_table(q_pts.data_ptr(), s_pts.data_ptr(), idx.data_ptr(), kpd.data_ptr(), float(sigma), P, Ns, NN,
                                          tab.data_ptr(), nbytes, stream), 'se3_kpconv_neighbor_table')
    return _neighbor_tables.store((q_pts, s_pts, idx), stream.value, (key, tab))[1]


_point_orders = Derived(256, prune_dead=True, share=False)          # points.data_ptr() -> (order (G * 16 int32), G), owned by the points tensor
_union_plans = Derived(64, share=False)               # stream -> plan of the last (geometry, order) seen there


def register_point_order(points, lengths, cell):
    """A spatial order of one stage's stacked points (per cloud: Morton order of floor(p / cell)), kept while the `points` tensor lives: the
    union-staged fused KPConv (csrc/kpconv_union.hip) takes its 16-point tiles along it.  Tile membership only -- no tensor is reordered.
    Called by the pyramid builder (se3et_amd/data.py); lengths: the stage's per-cloud counts (host)."""
    lens = [int(v) for v in (lengths.tolist() if hasattr(lengths, 'tolist') else lengths)]
    n = points.shape[0]
    if not KPCONV_UNION or not points.is_cuda or n == 0 or len(lens) > 32 or sum(lens) != n:
        return None
    points = _req(points, torch.float32, 'points', 2)
    stream = _stream()
    la = _i64_array(lens)
    G = int(lib().se3_point_order_groups(la, len(lens)))
    order = torch.empty((G * 16,), dtype=torch.int32, device=points.device)
    if max(lens) <= 8192:
        # one launch: a workgroup per cloud sorts (Morton code, index) in LDS
        check(lib().se3_point_order(points.data_ptr(), n, la, len(lens), float(cell), order.data_ptr(), stream), 'se3_point_order')
    else:
        keys = torch.empty((n,), dtype=torch.int64, device=points.device)
        check(lib().se3_point_order_keys(points.data_ptr(), n, la, len(lens), float(cell), keys.data_ptr(), stream), 'se3_point_order_keys')
        sk, si = torch.sort(keys, stable=True)
        check(lib().se3_point_order_place(sk.data_ptr(), si.data_ptr(), n, la, len(lens), order.data_ptr(), stream), 'se3_point_order_place')
    _point_orders.store(points, points.data_ptr(), (order, G))
    return order


def register_point_orders(points_list, lengths_list, cells):
    """register_point_order for several stages of one pyramid, in ONE launch when every cloud has at most 8192 points."""
    lens = [[int(v) for v in (l.tolist() if hasattr(l, 'tolist') else l)] for l in lengths_list]
    ok = KPCONV_UNION and 1 <= len(points_list) <= 4 and all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.shape[0] > 0
                                                             and len(l) <= 32 and sum(l) == p.shape[0] and max(l) <= 8192
                                                             for p, l in zip(points_list, lens))
    if not ok:
        # (clouds beyond 8192 points -- the KITTI configuration -- would take the keys + torch.sort + placement form, whose launches cost more
        # than the four narrow layers gain there: 142 against 141 pairs/s at C3 with the 160-row cap, 138.6 against 140.4 with the 128-row cap
        # and NN = 38; only with SE3_KPCONV_UNION=all)
        return [register_point_order(p, l, c) for p, l, c in zip(points_list, lengths_list, cells)] if KPCONV_UNION_ALL else [None] * len(points_list)
    S = len(points_list)
    las = [_i64_array(l) for l in lens]
    Gs = [int(lib().se3_point_order_groups(la, len(l))) for la, l in zip(las, lens)]
    orders = [torch.empty((G * 16,), dtype=torch.int32, device=p.device) for G, p in zip(Gs, points_list)]
    vp = ctypes.c_void_p
    check(lib().se3_point_order_stages((vp * S)(*[p.data_ptr() for p in points_list]), _i64_array([p.shape[0] for p in points_list]),
                                       (vp * S)(*[ctypes.cast(la, vp).value for la in las]), (ctypes.c_int * S)(*[len(l) for l in lens]),
                                       (ctypes.c_float * S)(*[float(c) for c in cells]), (vp * S)(*[o.data_ptr() for o in orders]), S, _stream()),
          'se3_point_order_stages')
    for p, o, G in zip(points_list, orders, Gs):
        _point_orders.store(p, p.data_ptr(), (o, G))
    return orders


def point_order(points):
    return _point_orders.lookup(points, points.data_ptr())


def _kpconv_union_plan(tab, q_pts, s_pts, idx, order, G, P, NN, stream):
    """Per group of 16 order positions the distinct support rows of its neighbour lists and every list slot's index into them
    (se3_kpconv_union_plan): a function of (order, neighbour table); kept per stream for the last table seen."""
    # (the plan reads the table's compacted lists and counts only -- the geometry, not the layer's kernel points: layers with tables of
    # their own over the same (queries, supports, neighbour indices) share it)
    plan = _union_plans.lookup((q_pts, s_pts, idx, order), stream.value)
    if plan is not None:
        return plan
    nbytes = lib().se3_kpconv_union_plan_bytes(G, NN)
    plan = torch.empty((nbytes,), dtype=torch.uint8, device=q_pts.device)
    order.record_stream(torch.cuda.current_stream())
    check(lib().se3_kpconv_union_plan(tab.data_ptr(), P, NN, order.data_ptr(), G, plan.data_ptr(), nbytes, stream), 'se3_kpconv_union_plan')
    return _union_plans.store((q_pts, s_pts, idx, order), stream.value, plan)


def _listed_amax(x, idx, Ns):
    """The largest |x| among the support rows that some neighbour list names, as a one-element device tensor (no host sync): the magnitude
    word of a plain input.  A row that no list names stays out -- the kernels never multiply it, and its size must not take the split's
    range away from the rows they do."""
    with torch.no_grad():
        rows = torch.linalg.vector_norm(x.detach().reshape(Ns, -1), float('inf'), dim=1)
        unlisted = torch.ones((Ns + 2,), dtype=torch.bool, device=x.device)          # [below the range | rows | the shadow and beyond]
        unlisted[(idx.reshape(-1) + 1).clamp_(0, Ns + 1)] = False
        return rows.masked_fill_(unlisted[1:Ns + 1], 0.0).amax().reshape(1)


def kpconv_inter_so3(x, q_pts, s_pts, idx, kernel_points, weights, kidx, ridx, sigma):
    """Fused matrix-core kernel (csrc/kpconv_mfma.hip) for channel counts that are multiples of (8, 32); otherwise the HIP gather of
    the slot-summed neighbourhood features (csrc/kpconv_so3.hip) + one library GEMM with the (36 Cin, Cout) weight matrix.
    x: (Ns, 6, Cin) tensor or BlockedFeatures (inference: written by group_norm_apply(blocked=True))."""
    blocked = isinstance(x, BlockedFeatures)
    xb = x.data if blocked else None
    x_amax = _amax_live(x) if blocked else None
    if blocked:
        Ns, A, Cin = x.shape
    else:
        x = _req(x.contiguous(), torch.float32, 'x', 3)
        Ns, A, Cin = x.shape
    q_pts, s_pts = _req(q_pts.contiguous(), torch.float32, 'q_pts', 2), _req(s_pts.contiguous(), torch.float32, 's_pts', 2)
    idx = _req(idx.contiguous(), torch.int64, 'neighb_inds', 2)
    P, NN = idx.shape
    Cout = weights.shape[-1]
    if A != 6 or tuple(weights.shape[:3]) != (6, 6, Cin) or Ns != s_pts.shape[0]:
        raise RuntimeError('kpconv_inter_so3: inconsistent shapes')
    kt, rt = _host_table(kidx, torch.int64), _host_table(ridx, torch.int64)
    path = _kpconv_use_matrix_core(Cin, Cout, P)
    fused_ok = bool(path) and Cin % 8 == 0 and Cout % 32 == 0 and Ns * 6 * Cin < 2 ** 31 and _builtin_slot_tables(kt, rt)
    po = point_order(q_pts) if (fused_ok and path is True and KPCONV_UNION and _kpconv_union_pays(Cin, Cout, q_pts is s_pts)) else None
    want = 0 if not blocked else x.kind
    if blocked and not (fused_ok and path != 'sums' and ((want == 2 and po is not None) or (want == 1 and po is None and Cin % 16 == 0))):
        x, blocked = x.plain().contiguous(), False              # (each fused kernel reads its own blocked layout only; the values, and their amax, stay)
    if fused_ok:
        if blocked:
            x = xb
        stream = _stream()
        Wp = _kpconv_weight_pieces(weights, Cin, Cout, stream)
        out = torch.empty((P, 6, Cout), dtype=torch.float32, device=x.device)
        # neighbour table (valid neighbours + 16 orbit weights each), then ONE kernel in which producer waves form the f16 hi / lo orbit sums
        # of a 16-point tile on the f32 matrix cores into LDS and consumer waves multiply them on the f16 matrix cores (csrc/kpconv_mfma.hip)
        tab = _kpconv_neighbor_table(q_pts, s_pts, idx, kernel_points, sigma, P, Ns, NN, stream)
        if not blocked and x_amax is None and path != 'sums' and P > 0 and Ns > 0:
            # a plain tensor (every call under autograd, a user's tensor through the drop-in modules) carries no magnitude word: the one the
            # kernels scale by before their f16 split (kpsum::x_split_scale) is formed here; the blocked input keeps the word of its apply pass
            x_amax = _listed_amax(x, idx, Ns)
        if path == 'sums':
            # two launches: the orbit sums as tile images in HBM, then the contraction (kept for A/B runs)
            Hs = torch.empty((lib().se3_kpconv_sums_bytes(P, Cin),), dtype=torch.uint8, device=x.device)
            check(lib().se3_kpconv_so3_gather_sums(x.data_ptr(), tab.data_ptr(), P, Ns, NN, Cin, Hs.data_ptr(), stream),
                  'se3_kpconv_so3_gather_sums')
            check(lib().se3_kpconv_so3_contract_f16(Hs.data_ptr(), Wp.data_ptr(), P, Cin, Cout, out.data_ptr(), stream),
                  'se3_kpconv_so3_contract_f16')
            return out
        if po is not None:
            # union-staged form (csrc/kpconv_union.hip): 16 spatial neighbours per workgroup, their distinct support rows read once
            order, G = po
            plan = _kpconv_union_plan(tab, q_pts, s_pts, idx, order, G, P, NN, stream)
            sbytes = lib().se3_kpconv_union_split_workspace_bytes(G, Cin, Cout) if KPCONV_SPLIT else 0
            sws = _ws_kpconv_union_split.get(x.device, stream.value, sbytes) if sbytes else None
            with _timed('kpconv_fused', 2.0 * 6 * P * 36 * Cin * Cout + 2.0 * P * NN * 16 * 6 * Cin):
                _check_counters(lib().se3_kpconv_so3_union(x.data_ptr(), tab.data_ptr(), plan.data_ptr(), G, P, Ns, NN, Cin, Cout, Wp.data_ptr(),
                                                           out.data_ptr(), sws.data_ptr() if sws is not None else None,
                                                           sws.numel() if sws is not None else 0, 1 if blocked else 0,
                                                           x_amax.data_ptr() if x_amax is not None else None, stream),
                                'se3_kpconv_so3_union', sws)
            return out
        sbytes = lib().se3_kpconv_fused_split_workspace_bytes(P, Cin, Cout) if KPCONV_SPLIT else 0
        sws = _ws_kpconv_split.get(x.device, stream.value, sbytes) if sbytes else None
        # (bench.py: event pair around the launch; algorithmic flops = contraction 2.6P.36Cin.Cout + the gather as a product 2.P.NN.16.6Cin)
        with _timed('kpconv_fused', 2.0 * 6 * P * 36 * Cin * Cout + 2.0 * P * NN * 16 * 6 * Cin):
            _check_counters(lib().se3_kpconv_so3_fused_scaled(x.data_ptr(), tab.data_ptr(), P, Ns, NN, Cin, Cout, Wp.data_ptr(), out.data_ptr(),
                                                              sws.data_ptr() if sws is not None else None, sws.numel() if sws is not None else 0,
                                                              1 if blocked else 0, x_amax.data_ptr() if x_amax is not None else None, stream),
                            'se3_kpconv_so3_fused', sws)
        return out
    kp = _host_table(kernel_points, torch.float32)          # (only this path reads the kernel points on the host)
    G = torch.empty((P * 6, 36 * Cin), dtype=torch.float32, device=x.device)
    check(lib().se3_kpconv_so3_gather(q_pts.data_ptr(), s_pts.data_ptr(), idx.data_ptr(), x.data_ptr(), kp.data_ptr(),
                                      kt.data_ptr(), rt.data_ptr(), float(sigma), P, Ns, NN, Cin, G.data_ptr(), _stream()),
          'se3_kpconv_so3_gather')
    Kg = 36 * Cin
    if not torch.is_grad_enabled() and Kg % 4 == 0 and Kg <= 64:
        # (the first layer of the backbone, Cin = 1: K = 36.)  The streaming kernel multiplies K rounded up to 32 wide: the rows of G are read
        # past their end into the next row (finite values) against weight columns that are zero; the last row reads zeros (buffer bounds).
        # Only the first layer: the kernel takes a row's f16-split scale from its FIRST 32 values (csrc/dense_norm.hip) and clamps later values
        # more than 2^8 times those.  The first 32 slot sums of a wider layer (Kg up to 1024 came here before) belong to at most four of
        # the 36 weight slots: a point with one or two neighbours has them at or next to zero beside live later slots, and its rows came out
        # clamped (tests/test_gpu_kpconv_edges.py, count ladder: up to 0.2 of the tensor's maximum).  Wider layers take the library GEMM.
        Kp = (Kg + 31) // 32 * 32
        Wt = _padded_transposed_weight(weights, Kg, Kp, Cout)
        out = torch.empty((P * 6, Cout), dtype=torch.float32, device=x.device)
        stream = _stream()
        check(lib().se3_linear_stream(G.data_ptr(), P * 6, Kp, Kg, _linear_weight_pieces(Wt, stream).data_ptr(), None, Cout, 0, out.data_ptr(), Cout,
                                      stream), 'se3_linear_stream (KPConv slot sums)')
        return out.view(P, 6, Cout)
    return mm(G, weights.reshape(Kg, Cout)).view(P, 6, Cout)


_padded_weights = Derived(64, weights=True)


def _padded_transposed_weight(weights, Kg, Kp, Cout):
    """(6, 6, Cin, Cout) KPConv weights as a dense layer's (Cout, Kp) weight: transposed, zero columns from Kg to Kp; kept per weight version."""
    key = (weights.data_ptr(), Kg, Kp, Cout, weights.device.index)
    Wt = _padded_weights.lookup(weights, key)
    if Wt is not None:
        return Wt
    with torch.no_grad():
        Wt = torch.zeros((Cout, Kp), dtype=torch.float32, device=weights.device)
        Wt[:, :Kg] = weights.detach().reshape(Kg, Cout).t()
    return _padded_weights.store(weights, key, Wt, fingerprint_of=(weights,))


def key_stride(M):
    """Row stride of key-major operands (relative-position logits, transposed values): keys padded to a multiple of 32."""
    return (M + 31) // 32 * 32


def _rows_view(t, name, C=None):
    """([A,] rows, C') float32 GPU view with unit last stride and 16-byte aligned rows -> (tensor3, anchors, rows, row_stride,
    anchor_stride); column blocks / row ranges of a wider tensor are accepted as they are (no copy)."""
    if not t.is_cuda or t.dtype != torch.float32:
        raise RuntimeError('%s must be a float32 GPU tensor' % name)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.stride(-1) != 1 or t.stride(-2) % 4 or (t.shape[0] > 1 and t.stride(0) % 4) or t.data_ptr() % 16:
        t = t.contiguous()
    if C is not None and t.shape[-1] != C:
        raise RuntimeError('%s: last dim %d != %d' % (name, t.shape[-1], C))
    return t, t.shape[0], t.shape[1], t.stride(1), (t.stride(0) if t.shape[0] > 1 else 0)


def attention(q, k, vt, bias, num_heads, out=None, v_shared=False, tag=None):
    """softmax_m((q.k [+ bias]) / sqrt(d)) v through se3_attention_fwd.  q ([A,] N, C), k ([A,] M, C): strided views are
    fine; vt ([A,] C, >= ceil32(M)) transposed values; bias (A*H, N, Mp) or None; out: optional ([A,] N, C) view with
    contiguous rows.  A = number of output anchors = anchors of vt (q/k with one anchor are broadcast)."""
    H = num_heads
    q3, Aq, N, q_rs, q_sa = _rows_view(q, 'q')
    C = q3.shape[-1]
    k3, Ak, M, k_rs, k_sa = _rows_view(k, 'k', C)
    v3 = vt if vt.dim() == 3 else vt.unsqueeze(0)
    if not v3.is_cuda or v3.dtype != torch.float32 or v3.stride(-1) != 1 or v3.stride(-2) % 4 or v3.data_ptr() % 16:
        v3 = v3.contiguous()
    Av, v_rs = v3.shape[0], v3.stride(1)
    if v3.shape[1] != C or v3.shape[2] < M:
        raise RuntimeError('attention: transposed values %s do not match C=%d, M=%d' % (tuple(v3.shape), C, M))
    A = max(Aq, Ak, Av)
    Mp = key_stride(M)
    if bias is not None and (tuple(bias.shape) != (A * H, N, Mp) or not bias.is_contiguous()):
        raise RuntimeError('attention: bias must be a contiguous (A*H, N, %d) tensor' % Mp)
    if out is None:
        out = torch.empty((A, N, C), dtype=torch.float32, device=q3.device)
    o3 = out if out.dim() == 3 else out.unsqueeze(0)
    if tuple(o3.shape) != (A, N, C) or o3.stride(-1) != 1 or o3.stride(-2) != C:
        raise RuntimeError('attention: out must be (A, N, C) with contiguous rows')
    with _timed('attention_kernel' if tag is None else 'attention_kernel@' + tag, 0):
        check(lib().se3_attention_fwd(q3.data_ptr(), k3.data_ptr(), v3.data_ptr(), bias.data_ptr() if bias is not None else None,
                                      A, N, M, C, H, q_rs, k_rs, v_rs, q_sa if Aq > 1 else 0, k_sa if Ak > 1 else 0,
                                      v3.stride(0) if Av > 1 else 0, o3.stride(0) if A > 1 else 0, Mp,
                                      1.0 / math.sqrt(C // H), o3.data_ptr(), _stream()), 'se3_attention_fwd')
    return out


def rpe_bias(qp, qe, emb, eq_emb, num_heads):
    """Relative-position logits (A*H, N, Mp) from the folded queries qp ([A,] N, H*C) [and qe ([A,] N, 4*H)] (strided views
    of one projection are fine: qp and qe must share row / anchor strides) and the embeddings emb (N, M, C), eq_emb (A, N, M, 4)."""
    H = num_heads
    emb = _req(emb, torch.float32, 'embed_qk', 3)
    N, M, C = emb.shape
    qp3, A, Nq, rs, sa = _rows_view(qp, 'qp', H * C)
    if Nq != N:
        raise RuntimeError('rpe_bias: %d folded query rows for an (N=%d, M, C) embedding' % (Nq, N))
    qe_ptr = None
    eq_ptr = None
    if qe is not None:
        qe3, Ae, Ne, rs_e, sa_e = _rows_view(qe, 'qe', 4 * H)
        if (Ae, Ne, rs_e, sa_e) != (A, N, rs, sa):
            raise RuntimeError('rpe_bias: qe must be a column block of the same projection as qp')
        eq_emb = _req(eq_emb, torch.float32, 'embed_eq', 4)
        if tuple(eq_emb.shape) != (A, N, M, 4):
            raise RuntimeError('rpe_bias: equivariant embedding shape %s' % (tuple(eq_emb.shape),))
        qe_ptr, eq_ptr = qe3.data_ptr(), eq_emb.data_ptr()
    if A * H > 32 or C % 16:
        raise RuntimeError('rpe_bias: anchors*heads must be <= 32 and C a multiple of 16')
    Mp = key_stride(M)
    bias = torch.empty((A * H, N, Mp), dtype=torch.float32, device=emb.device)
    # algorithmic bytes of one self-attention call: q, k, v in + out, the embedding, the eq-embedding;
    # booked on this (embedding-streaming) launch, the attention launch of the same call is booked with 0 bytes
    survey_bytes = 4 * (4 * A * N * C + N * M * C + (A * N * M * 4 if qe is not None else 0))
    with _timed('rpe_bias_kernel', survey_bytes, 'eq' if qe is not None else 'inv'):
        check(lib().se3_rpe_bias_fwd(qp3.data_ptr(), qe_ptr, rs, sa, emb.data_ptr(), eq_ptr, N, M, C, A * H, H, Mp,
                                     bias.data_ptr(), _stream()), 'se3_rpe_bias_fwd')
    return bias


def neighbor_table_trim(full, width, pair_row_ends, pair_widths):
    """HIP (csrc/radius_neighbors.hip): full (rows, W) int64 -> (rows, width) with the columns past each pair's own width marked -1."""
    full = _req(full, torch.int64, 'full', 2)
    rows, W = full.shape
    out = torch.empty((rows, width), dtype=torch.int64, device=full.device)
    n = len(pair_row_ends)
    check(lib().se3_neighbor_table_trim(full.data_ptr(), rows, W, int(width), _i64_array(pair_row_ends), (ctypes.c_int * n)(*[int(w) for w in pair_widths]),
                                        n, out.data_ptr(), _stream()), 'se3_neighbor_table_trim')
    return out


def _i64_array(values):
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def stack_bias_offsets(lengths, key_lengths, AH):
    """Float offsets of the per-cloud (A*H, N_c, ceil32(M_c)) logits blocks in one workspace, and its total size."""
    offs, total = [], 0
    for n, m in zip(lengths, key_lengths):
        offs.append(total)
        total += AH * int(n) * key_stride(int(m))
    return offs, total


def _embedding_list(embs, C):
    """(bytes per element, contiguous GPU tensors): the geometric embeddings of a call are all float32 or all bfloat16."""
    dt = embs[0].dtype
    if dt not in (torch.float32, torch.bfloat16) or (dt == torch.bfloat16 and C % 32):
        raise RuntimeError('embed_qk must be float32, or bfloat16 with C a multiple of 32')
    return (4 if dt == torch.float32 else 2), [_req(e, dt, 'embed_qk', 3) for e in embs]


def rpe_bias_stack(qp, qe, embs, eq_embs, starts, lengths, num_heads):
    """Stack mode of rpe_bias: qp ([A,] R, H*C) [qe ([A,] R, 4*H)] hold the folded queries of all clouds (cloud c = rows
    starts[c] .. + lengths[c]); embs[c] (N_c, N_c, C), eq_embs[c] (A, N_c, N_c, 4) or None.  ONE launch; returns the flat
    logits workspace and the per-cloud block offsets (block c: (A*H, N_c, ceil32(N_c)))."""
    H = num_heads
    C = embs[0].shape[-1]
    qp3, A, R, rs, sa = _rows_view(qp, 'qp', H * C)
    has_eq = qe is not None
    qe_ptr = None
    if has_eq:
        qe3, Ae, Re, rs_e, sa_e = _rows_view(qe, 'qe', 4 * H)
        if (Ae, Re, rs_e, sa_e) != (A, R, rs, sa):
            raise RuntimeError('rpe_bias_stack: qe must be a column block of the same projection as qp')
        qe_ptr = qe3.data_ptr()
    if A * H > 32 or C % 16:
        raise RuntimeError('rpe_bias_stack: anchors*heads must be <= 32 and C a multiple of 16')
    esize, embs = _embedding_list(embs, C)
    survey_bytes = 0
    for c, (e, n) in enumerate(zip(embs, lengths)):
        if tuple(e.shape) != (n, n, C) or starts[c] + n > R:
            raise RuntimeError('rpe_bias_stack: cloud %d: embedding %s for %d rows at %d of %d' % (c, tuple(e.shape), n, starts[c], R))
        survey_bytes += 4 * (4 * A * n * C + (A * n * n * 4 if has_eq else 0)) + esize * n * n * C
    eqs = None
    if has_eq:
        eqs = [_req(e, torch.float32, 'embed_eq', 4) for e in eq_embs]
        for e, n in zip(eqs, lengths):
            if tuple(e.shape) != (A, n, n, 4):
                raise RuntimeError('rpe_bias_stack: equivariant embedding shape %s' % (tuple(e.shape),))
    offs, total = stack_bias_offsets(lengths, lengths, A * H)
    bias = torch.empty((total,), dtype=torch.float32, device=qp3.device)
    with _timed('rpe_bias_kernel', survey_bytes, 'eq' if has_eq else 'inv'):
        entry = lib().se3_rpe_bias_stack_fwd if esize == 4 else lib().se3_rpe_bias_stack_bf16_fwd
        check(entry(qp3.data_ptr(), qe_ptr, rs, sa, _ptr_array(embs), _ptr_array(eqs) if has_eq else None, _i64_array(starts),
                    _i64_array(lengths), _i64_array(lengths), _i64_array(offs), len(embs), C, A * H, H, bias.data_ptr(),
                    _stream()), 'se3_rpe_bias_stack_fwd')
    return bias, offs


def attention_stack(q, k, vt, bias, bias_offsets, q_starts, q_lengths, k_starts, k_lengths, num_heads, out, tag=None):
    """Stack mode of attention: q ([A,] R, C), k ([A,] R, C) packed rows, vt ([A,] C, Rk) transposed values addressed by key
    column, out ([A,] R, C) with contiguous rows; cloud c: queries q_starts[c] .. + q_lengths[c], keys k_starts[c] .. +
    k_lengths[c] (k_starts multiples of 4, ceil32(k_lengths[c]) columns readable).  bias: flat workspace of rpe_bias_stack or None."""
    H = num_heads
    q3, Aq, R, q_rs, q_sa = _rows_view(q, 'q')
    C = q3.shape[-1]
    k3, Ak, Rk, k_rs, k_sa = _rows_view(k, 'k', C)
    v3 = vt if vt.dim() == 3 else vt.unsqueeze(0)
    if not v3.is_cuda or v3.dtype != torch.float32 or v3.stride(-1) != 1 or v3.stride(-2) % 4 or v3.data_ptr() % 16:
        v3 = v3.contiguous()
    Av, v_rs = v3.shape[0], v3.stride(1)
    if v3.shape[1] != C:
        raise RuntimeError('attention_stack: transposed values %s do not match C=%d' % (tuple(v3.shape), C))
    A = max(Aq, Ak, Av)
    o3 = out if out.dim() == 3 else out.unsqueeze(0)
    if o3.shape[0] != A or o3.shape[2] != C or o3.stride(-1) != 1 or o3.stride(-2) != C or o3.dtype != torch.float32:
        raise RuntimeError('attention_stack: out must be (A, rows, C) float32 with contiguous rows')
    for c in range(len(q_starts)):
        if q_starts[c] + q_lengths[c] > min(R, o3.shape[1]) or k_starts[c] + k_lengths[c] > Rk or \
                k_starts[c] + key_stride(k_lengths[c]) > v3.shape[2]:
            raise RuntimeError('attention_stack: cloud %d exceeds the packed rows / value columns' % c)
    if bias is not None and (not bias.is_cuda or bias.dtype != torch.float32 or not bias.is_contiguous()):
        raise RuntimeError('attention_stack: bias must be a contiguous float32 GPU workspace')
    with _timed('attention_kernel' if tag is None else 'attention_kernel@' + tag, 0):
        check(lib().se3_attention_stack_fwd(q3.data_ptr(), k3.data_ptr(), v3.data_ptr(), bias.data_ptr() if bias is not None else None,
                                            _i64_array(q_starts), _i64_array(q_lengths), _i64_array(k_starts), _i64_array(k_lengths),
                                            _i64_array(bias_offsets) if bias is not None else None, len(q_starts), A, C, H,
                                            q_rs, k_rs, v_rs, q_sa if Aq > 1 else 0, k_sa if Ak > 1 else 0,
                                            v3.stride(0) if Av > 1 else 0, o3.stride(0) if A > 1 else 0,
                                            1.0 / math.sqrt(C // H), o3.data_ptr(), *_attention_pieces(A, k_starts, k_lengths, C, v_rs, q3.device),
                                            _stream()), 'se3_attention_stack_fwd')
    return out


def rpe_self_attention_stack(proj, offs, vt, embs, eq_embs, starts, lengths, num_heads, out):
    """The stack-mode RPE self-attention call: proj ([A,] R, 2C + HC [+ 4H]) is the stacked projection [q | k | W_p^T q | W_eq^T q]
    of the packed rows (column offsets `offs`), vt ([A,] C, R) the transposed values, embs[c] (N_c, N_c, C), eq_embs[c]
    (A, N_c, N_c, 4) or None; out ([A,] R, C) receives the rows of every cloud.  Both kernels (relative-position logits, then
    softmax.V) are launched back to back from one C call."""
    H = num_heads
    C = embs[0].shape[-1]
    p3, A, R, rs, sa = _rows_view(proj, 'proj')
    has_eq = eq_embs is not None and eq_embs[0] is not None
    if offs['qp'] + H * C > p3.shape[-1] or (has_eq and offs['qe'] + 4 * H > p3.shape[-1]):
        raise RuntimeError('rpe_self_attention_stack: projection narrower than its column offsets')
    if A * H > 32 or C % 16:
        raise RuntimeError('rpe_self_attention_stack: anchors*heads must be <= 32 and C a multiple of 16')
    v3 = vt if vt.dim() == 3 else vt.unsqueeze(0)
    if not v3.is_cuda or v3.dtype != torch.float32 or v3.stride(-1) != 1 or v3.stride(-2) % 4 or v3.data_ptr() % 16 or \
            v3.shape[0] != A or v3.shape[1] != C:
        raise RuntimeError('rpe_self_attention_stack: vt must be a float32 (A, C, rows) GPU tensor with 16-byte aligned rows')
    o3 = out if out.dim() == 3 else out.unsqueeze(0)
    if o3.shape[0] != A or o3.shape[2] != C or o3.stride(-1) != 1 or o3.stride(-2) != C or o3.dtype != torch.float32:
        raise RuntimeError('rpe_self_attention_stack: out must be (A, rows, C) float32 with contiguous rows')
    esize, embs = _embedding_list(embs, C)
    survey_bytes, total = 0, 0
    for c, (e, n) in enumerate(zip(embs, lengths)):
        if tuple(e.shape) != (n, n, C) or starts[c] % 4 or starts[c] + n > min(R, o3.shape[1]) or \
                starts[c] + key_stride(n) > v3.shape[2]:
            raise RuntimeError('rpe_self_attention_stack: cloud %d: embedding %s, %d rows at %d of %d' % (c, tuple(e.shape), n, starts[c], R))
        survey_bytes += 4 * (4 * A * n * C + (A * n * n * 4 if has_eq else 0)) + esize * n * n * C
        total += A * H * n * key_stride(n)
    eqs = None
    if has_eq:
        eqs = [_req(e, torch.float32, 'embed_eq', 4) for e in eq_embs]
        for e, n in zip(eqs, lengths):
            if tuple(e.shape) != (A, n, n, 4):
                raise RuntimeError('rpe_self_attention_stack: equivariant embedding shape %s' % (tuple(e.shape),))
    logits = torch.empty((total,), dtype=torch.float32, device=p3.device)
    base = p3.data_ptr()
    col = lambda name: base + 4 * offs[name]
    entry = lib().se3_rpe_self_attention_stack_fwd if esize == 4 else lib().se3_rpe_self_attention_stack_bf16_fwd
    if KERNEL_TIMINGS is not None:       # bench.py pairs these with the library's per-launch HIP events, in call order
        with _TIMING_LOCK:               # (host threads with one stream each: the record and the launches stay in one order)
            KERNEL_TIMINGS.setdefault('rpe_self_attention_calls', []).append((survey_bytes, ('eq' if has_eq else 'inv') + ('' if esize == 4 else '_bf16')))
            check(entry(col('q'), col('k'), v3.data_ptr(), col('qp'), col('qe') if has_eq else None, rs, sa, v3.stride(1),
                        v3.stride(0) if A > 1 else 0, _ptr_array(embs), _ptr_array(eqs) if has_eq else None, _i64_array(starts),
                        _i64_array(lengths), len(embs), A, C, H, logits.data_ptr(), o3.stride(0) if A > 1 else 0, o3.data_ptr(),
                        *_attention_pieces(A, starts, lengths, C, v3.stride(1), p3.device), _stream()), 'se3_rpe_self_attention_stack_fwd')
        return out
    check(entry(col('q'), col('k'), v3.data_ptr(), col('qp'), col('qe') if has_eq else None, rs, sa, v3.stride(1),
                v3.stride(0) if A > 1 else 0, _ptr_array(embs), _ptr_array(eqs) if has_eq else None, _i64_array(starts),
                _i64_array(lengths), len(embs), A, C, H, logits.data_ptr(), o3.stride(0) if A > 1 else 0, o3.data_ptr(),
                *_attention_pieces(A, starts, lengths, C, v3.stride(1), p3.device), _stream()), 'se3_rpe_self_attention_stack_fwd')
    return out


def _attention_pieces(A, k_starts, k_lengths, C, v_row_stride, device):
    """(workspace pointer, bytes) for the f16 hi / lo pieces of K and V^T of one stack-mode attention call: one buffer per stream."""
    rows = max(int(s) + int(n) for s, n in zip(k_starts, k_lengths))
    nbytes = lib().se3_attention_kv_pieces_bytes(int(A), rows, int(C), int(v_row_stride))
    if nbytes == 0:
        return None, 0
    ws = _ws_attn.get(device, _stream().value, nbytes)
    return ws.data_ptr(), ws.numel()


def cross_attention(q, k, vt, num_heads):
    """HIP: plain cross attention; vt (C, Mp) or (A, C, Mp) transposed values (per-anchor values share the scores)."""
    out = attention(q, k, vt, None, num_heads)
    return out[0] if vt.dim() == 2 else out


def cross_attention_eq(q, k, vt, num_heads, mode, trace_idx):
    """HIP: global anchor-pair statistics (se3_cross_eq_stats) + weighted per-pair softmax.V (se3_cross_eq_apply)."""
    q = _req(q.contiguous(), torch.float32, 'q', 3)
    k = _req(k.contiguous(), torch.float32, 'k', 3)
    vt = _req(vt.contiguous(), torch.float32, 'vt', 3)
    A, N, C = q.shape
    M, H = k.shape[1], num_heads
    scale = 1.0 / math.sqrt(C // H)
    P = (N + 31) // 32
    partial = torch.empty((A * A, P), dtype=torch.float32, device=q.device)
    nparts = ctypes.c_int(0)
    check(lib().se3_cross_eq_stats(q.data_ptr(), k.data_ptr(), A, N, M, C, H, scale, partial.data_ptr(),
                                   ctypes.byref(nparts), _stream()), 'se3_cross_eq_stats')
    if mode not in ('a_soft', 'r_soft'):
        raise RuntimeError('cross_attention_eq: mode %r' % (mode,))
    R = trace_idx.shape[0]
    mix = torch.empty((A, A), dtype=torch.float32, device=q.device)
    ret = torch.empty((A, A) if mode == 'a_soft' else (R,), dtype=torch.float32, device=q.device)
    trace_idx = _req(trace_idx.contiguous(), torch.int64, 'trace_idx', 2)
    check(lib().se3_cross_eq_mix(partial.data_ptr(), P, A, N, M, 0 if mode == 'a_soft' else 1, trace_idx.data_ptr(), R,
                                 mix.data_ptr(), ret.data_ptr(), _stream()), 'se3_cross_eq_mix')
    out = torch.empty((A, N, C), dtype=torch.float32, device=q.device)
    Mp = key_stride(M)
    if tuple(vt.shape) != (A, C, Mp):
        raise RuntimeError('cross_attention_eq: transposed values must be (A, C, %d)' % Mp)
    check(lib().se3_cross_eq_apply(q.data_ptr(), k.data_ptr(), vt.data_ptr(), mix.data_ptr(), A, N, M, C, H,
                                   Mp, scale, out.data_ptr(), _stream()), 'se3_cross_eq_apply')
    return out, ret, mix


# equivariant cross attention of a batch on the bf16 matrix cores at f32 accuracy (SE3_CROSS_EQ=f32 forces the f32 MFMA kernels)
CROSS_EQ_BF16X6 = os.environ.get('SE3_CROSS_EQ', 'bf16x6') != 'f32'
_pair_row_tables = Derived(64)


def _pair_rows(starts, lengths, device):
    """(P * W,) row indices and a (1, P, W, 1) 0/1 mask that cut the packed rows of P clouds into P windows of W rows."""
    key = (tuple(int(s) for s in starts), tuple(int(n) for n in lengths), str(device))
    W = max(key[1])
    hit = _pair_row_tables.lookup((), key)
    if hit is None:
        idx = to_device([s + min(j, n - 1) for s, n in zip(key[0], key[1]) for j in range(W)], torch.int64, device)
        mask = to_device([1.0 if j < n else 0.0 for n in key[1] for j in range(W)], torch.float32, device)
        hit = _pair_row_tables.store((), key, (idx, mask))
    return hit[0], hit[1].view(1, len(key[1]), W, 1), W


GRAM_KERNEL = True            # False: index_select + mask + batched library GEMM (A/B runs, tests)


def _gram_per_pair(x, starts, lengths):
    """x (A, R, C) packed rows -> (A, P, C, C): X_p^T X_p over the rows of every pair (csrc/attention.hip: gram_stack_kernel; other channel
    counts / strided rows: index_select + library GEMM)."""
    A, P, C = x.shape[0], len(starts), x.shape[2]
    if GRAM_KERNEL and C in (128, 256) and P <= 16 and x.dtype == torch.float32 and x.stride(2) == 1 and x.stride(1) == C:
        out = torch.empty((A, P, C, C), dtype=torch.float32, device=x.device)
        check(lib().se3_gram_stack(x.data_ptr(), A, C, x.stride(0) if A > 1 else 0, _i64_array(starts), _i64_array(lengths), P, out.data_ptr(),
                                   _stream()), 'se3_gram_stack')
        return out
    idx, mask, W = _pair_rows(starts, lengths, x.device)
    win = x.index_select(1, idx).view(A, P, W, C)
    win.mul_(mask)                                   # rows past a cloud's length -> 0 (the mask is 0 / 1: masking both operands is masking one)
    win = win.view(A * P, W, C)
    return torch.bmm(win.transpose(1, 2), win).view(A, P, C, C)


def cross_eq_groups(A, q_lengths, num_heads, C, k_starts, vt):
    """Key-anchor groups of cross_attention_eq_stack for this call: with few pairs one workgroup per (128 queries, head, anchor) leaves
    most compute units idle while every wave walks A x key-tiles dependent steps, so the key anchors are divided over 3 (or 2) workgroups
    whose partial results lie side by side along the channels of the output.  1 = the plain form."""
    H = int(num_heads)
    if not CROSS_EQ_BF16X6 or C // H != 64 or C % H or A > 6 or vt.stride(1) % 16 or vt.stride(2) != 1 or any(int(s) % 16 for s in k_starts):
        return 1
    wgs = sum((int(n) + 127) // 128 for n in q_lengths) * H * A
    for G in (3, 2):
        if A % G == 0 and wgs * G <= 320:
            return G
    return 1


def cross_attention_eq_stack(q, k, vt, q_starts, q_lengths, k_starts, k_lengths, num_heads, mode, trace_idx, out, groups=1):
    """HIP: equivariant cross attention of all pairs of a batch (se3_cross_eq_stack_fwd).  q (A, Rq, C), k (A, Rk, C) packed rows,
    vt (A, C, Rk) transposed values, out (A, Rq, C) (rows outside the pairs are left untouched).  Returns the per-pair mixing
    matrices (P, A, A) and weights (P, A*A) ('a_soft') / (P, R) ('r_soft').  groups = G > 1 (cross_eq_groups): out (A, Rq, G * C)
    contiguous, the result is the sum of its G channel blocks (the caller folds it into the next dense layer: stacked_weight)."""
    q = _req(q, torch.float32, 'q', 3)
    k = _req(k, torch.float32, 'k', 3)
    vt = _req(vt, torch.float32, 'vt', 3)
    out = _req(out, torch.float32, 'out', 3)
    A, Rq, C = q.shape
    groups = int(groups)
    if k.shape[0] != A or k.shape[2] != C or tuple(vt.shape[:2]) != (A, C) or tuple(out.shape) != (A, Rq, groups * C):
        raise RuntimeError('cross_attention_eq_stack: shapes q %s k %s vt %s out %s' % (tuple(q.shape), tuple(k.shape), tuple(vt.shape), tuple(out.shape)))
    if groups > 1 and not (CROSS_EQ_BF16X6 and out.is_contiguous()):
        raise RuntimeError('cross_attention_eq_stack: key-anchor groups need the f16 form and a contiguous output')
    if mode not in ('a_soft', 'r_soft'):
        raise RuntimeError('cross_attention_eq_stack: mode %r' % (mode,))
    P = len(q_starts)
    for p in range(P):
        if q_starts[p] + q_lengths[p] > Rq or k_starts[p] + k_lengths[p] > k.shape[1] or k_starts[p] + key_stride(k_lengths[p]) > vt.shape[2]:
            raise RuntimeError('cross_attention_eq_stack: pair %d exceeds the packed rows / value columns' % p)
    trace_idx = _req(trace_idx.contiguous(), torch.int64, 'trace_idx', 2)
    R = trace_idx.shape[0]
    dev = q.device
    # anchor-pair statistics sum_{n,m} (mean_h S[a,e,h,n,m])^2: the head mean of the per-head dot products is the dot product
    # over all C channels, so the sum is (scale / H)^2 <Q_a^T Q_a, K_e^T K_e>_F -- two Gram products per pair instead of the
    # (A*A, N, M) score pass of se3_cross_eq_stats (vanilla_transformer.py:380-389,425-426 computes the scores themselves)
    f = 1.0 / (math.sqrt(C // int(num_heads)) * int(num_heads))
    gq, gk = _gram_per_pair(q, q_starts, q_lengths), _gram_per_pair(k, k_starts, k_lengths)
    partial = torch.empty((P, A, A), dtype=torch.float32, device=dev)
    check(lib().se3_gram_frobenius(gq.data_ptr(), gk.data_ptr(), A, P, C * C, f * f, partial.data_ptr(), _stream()), 'se3_gram_frobenius')
    mix = torch.empty((P, A, A), dtype=torch.float32, device=dev)
    weights = torch.empty((P, A * A if mode == 'a_soft' else R), dtype=torch.float32, device=dev)
    if CROSS_EQ_BF16X6 and q.stride(1) == C and k.stride(1) == C and q.stride(2) == 1 and k.stride(2) == 1 and vt.stride(2) == 1:
        # bf16 matrix cores at f32 accuracy (csrc/attention.hip: cross_eq_apply_stack_x6_kernel); shapes it does not take are forwarded
        # to the f32 kernels by the entry point itself
        stream = _stream()
        ws_bytes = lib().se3_cross_eq_x6_workspace_bytes(A, Rq, k.shape[1], C, vt.stride(1))
        ws = _ws_x6.get(dev, stream.value, ws_bytes)
        check(lib().se3_cross_eq_stack_x6_fwd(q.data_ptr(), k.data_ptr(), vt.data_ptr(), _i64_array(q_starts), _i64_array(q_lengths),
                                              _i64_array(k_starts), _i64_array(k_lengths), P, A, C, int(num_heads), Rq, k.shape[1],
                                              q.stride(0), k.stride(0), vt.stride(1), vt.stride(0), 0 if mode == 'a_soft' else 1,
                                              trace_idx.data_ptr(), R, 1, partial.data_ptr(), mix.data_ptr(), weights.data_ptr(),
                                              out.data_ptr(), groups, out.stride(0), ws.data_ptr(), ws.numel(), stream),
              'se3_cross_eq_stack_x6_fwd')
        return mix, weights
    if groups > 1:
        raise RuntimeError('cross_attention_eq_stack: key-anchor groups with strided q / k rows')
    check(lib().se3_cross_eq_stack_fwd(q.data_ptr(), k.data_ptr(), vt.data_ptr(), _i64_array(q_starts), _i64_array(q_lengths),
                                       _i64_array(k_starts), _i64_array(k_lengths), P, A, C, int(num_heads), q.stride(0), k.stride(0),
                                       vt.stride(1), vt.stride(0), 0 if mode == 'a_soft' else 1, trace_idx.data_ptr(), R, 1,
                                       partial.data_ptr(), mix.data_ptr(), weights.data_ptr(), out.data_ptr(), _stream()),
          'se3_cross_eq_stack_fwd')
    return mix, weights


_EMB_D_RANGE, _EMB_D_PER_UNIT = 64.0, 64.0        # distance-index table: [0, 64) index units, 64 entries per unit
_EMB_A_PER_UNIT = 32.0                             # angle-index table: a 32-channel slice (418 entries x 256 B) fits in LDS; Hermite error h^4 / 384 |f''''| ~ 2.5e-9 |f''''|
_emb_table_cache = {}
also_clear += [_emb_table_cache.clear, _amax_rings.clear]          # (device-side validation state, a ring cursor: own logic, cleared by clear_caches())


def _embedding_table(weight, bias, div_term, x_max, per_unit):
    """(entries, C, 2): f(x) = W emb(x) + b and f'(x) at x = j / per_unit, j = 0 .. x_max * per_unit, built and VALIDATED ON THE
    DEVICE by se3_embedding_table_refresh in front of every use: the kernel hashes the current weight values and rebuilds the
    table when they differ from the ones it was built from.  The host cache below only holds the buffers (keyed by the
    storage addresses): identity / version bookkeeping of the Parameters plays no role, so `p.data.copy_()`, `module.to()`,
    `load_state_dict` and optimizer steps can never leave a stale table behind.  One table + validation state PER LAUNCH STREAM: the
    refresh kernels count their completed workgroups in the state block, which two streams rebuilding the same table at the same time
    (first use under `bench.py --inflight 2`) would mix -- calls on one stream are ordered, so a per-stream table has one writer."""
    weight, bias, div_term = weight.detach(), bias.detach(), div_term.detach()
    for t, name in ((weight, 'weight'), (bias, 'bias'), (div_term, 'div_term')):
        _req(t, torch.float32, 'embedding ' + name)
    C = weight.shape[0]
    n = int(math.ceil(x_max * per_unit)) + 2
    stream = _stream()
    key = (str(weight.device), stream.value, weight.data_ptr(), bias.data_ptr(), div_term.data_ptr(), C, n, float(per_unit))
    hit = _emb_table_cache.get(key)
    if hit is None:
        hit = (torch.empty((n, C, 2), dtype=torch.float32, device=weight.device),
               torch.zeros((lib().se3_embedding_table_state_bytes(),), dtype=torch.uint8, device=weight.device))
        if len(_emb_table_cache) > 32:
            _emb_table_cache.clear()
        _emb_table_cache[key] = hit
    tab, state = hit
    check(lib().se3_embedding_table_refresh(weight.data_ptr(), bias.data_ptr(), div_term.data_ptr(), C, n, float(per_unit),
                                            tab.data_ptr(), state.data_ptr(), stream), 'se3_embedding_table_refresh')
    return tab


def knn3_stack(points, lengths):
    """HIP (csrc/partition.hip): the 3 nearest other points of every point of several stacked clouds, indices local to the cloud."""
    points = _req(points.contiguous(), torch.float32, 'points', 2)
    if sum(lengths) != points.shape[0]:
        raise RuntimeError('knn3_stack: lengths do not add up to the stacked points')
    knn = torch.empty((points.shape[0], 3), dtype=torch.int64, device=points.device)
    check(lib().se3_knn3_stack(points.data_ptr(), _i64_array(lengths), len(lengths), knn.data_ptr(), _stream()), 'se3_knn3_stack')
    return knn


def embedding_tables(div_term, w_d, b_d, w_a, b_a, sigma_a):
    """The two validated tables (distance, angle) of a geometric embedding: pass them as `tables=` to several geometric_embedding calls of
    one forward (all clouds of a batch) to validate the weights once instead of once per cloud."""
    return (_embedding_table(w_d, b_d, div_term, _EMB_D_RANGE, _EMB_D_PER_UNIT),
            _embedding_table(w_a, b_a, div_term, 180.0 / sigma_a + 1.0, _EMB_A_PER_UNIT))


def geometric_embedding(points, div_term, w_d, b_d, w_a, b_a, sigma_d, sigma_a, k, wigner_d1=None, dtype=torch.float32, knn=None, tables=None):
    """HIP (csrc/geo_embedding.hip).  Returns emb (N, N, C), or (emb, eq_emb (A, N, N, 4)) when wigner_d1 is given.
    dtype: torch.float32, or torch.bfloat16 for the 'bf16 attention' mode (emb stored rounded; eq_emb stays float32)."""
    points = _req(points.contiguous(), torch.float32, 'points', 2)
    if k != 3:
        raise RuntimeError('geometric_embedding: angle_k must be 3 on the HIP path')
    N, C = points.shape[0], w_d.shape[0]
    # 3 nearest other points (the reference takes top-(k+1) of the distance map and drops the first column)
    if knn is None:
        knn = torch.empty((N, 3), dtype=torch.int64, device=points.device)
        check(lib().se3_knn3(points.data_ptr(), N, knn.data_ptr(), _stream()), 'se3_knn3')
    else:                            # precomputed for all clouds of a batch (knn3_stack)
        knn = _req(knn, torch.int64, 'knn', 2)
        if tuple(knn.shape) != (N, 3):
            raise RuntimeError('geometric_embedding: knn must be (N, 3)')
    tab_d, tab_a = tables if tables is not None else embedding_tables(div_term, w_d, b_d, w_a, b_a, sigma_a)
    if dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError('geometric_embedding: dtype must be float32 or bfloat16')
    emb = torch.empty((N, N, C), dtype=dtype, device=points.device)
    eq = None
    A = 0
    if wigner_d1 is not None:
        A = wigner_d1.shape[0]
        eq = torch.empty((A, N, N, 4), dtype=torch.float32, device=points.device)
        wigner_d1 = wigner_d1.detach().contiguous()
    entry = lib().se3_geo_embedding_fwd if dtype == torch.float32 else lib().se3_geo_embedding_bf16_fwd
    ws = _ws_emb.get(points.device, _stream().value, lib().se3_geo_embedding_workspace_bytes(N))
    check(entry(points.data_ptr(), knn.data_ptr(), N, C, tab_d.data_ptr(), tab_d.shape[0], _EMB_D_PER_UNIT, tab_a.data_ptr(),
                tab_a.shape[0], _EMB_A_PER_UNIT, float(sigma_d), float(sigma_a), w_d.data_ptr(), b_d.data_ptr(), w_a.data_ptr(),
                b_a.data_ptr(), div_term.data_ptr(), wigner_d1.data_ptr() if eq is not None else None, A, emb.data_ptr(),
                eq.data_ptr() if eq is not None else None, ws.data_ptr(), ws.numel(), _stream()), 'se3_geo_embedding_fwd')
    return emb if eq is None else (emb, eq)


def geometric_embedding_bwd(grad_emb, points, div_term, w_d, b_d, w_a, b_a, sigma_d, sigma_a, knn, tables=None):
    """Gradients of geometric_embedding with respect to (w_d, b_d, w_a, b_a): the HIP kernel writes the GEMM operands (sinusoid embeddings
    of the four indices, gradient masked by the arg-max angle), the products are two library GEMMs (csrc/geo_embedding.hip)."""
    points = _req(points.contiguous(), torch.float32, 'points', 2)
    g = _req(grad_emb.contiguous(), torch.float32, 'grad_emb', 3)
    N, C = points.shape[0], w_d.shape[0]
    knn = _req(knn, torch.int64, 'knn', 2)
    tab_a = (tables if tables is not None else embedding_tables(div_term, w_d, b_d, w_a, b_a, sigma_a))[1]
    S = torch.empty((4, N * N, C), dtype=torch.float32, device=points.device)
    dEk = torch.empty((3 * N * N, C), dtype=torch.float32, device=points.device)
    check(lib().se3_geo_embedding_bwd_operands(points.data_ptr(), knn.data_ptr(), N, C, tab_a.data_ptr(), tab_a.shape[0], _EMB_A_PER_UNIT,
                                               float(sigma_d), float(sigma_a), w_a.data_ptr(), b_a.data_ptr(), div_term.data_ptr(),
                                               g.data_ptr(), S.data_ptr(), dEk.data_ptr(), _stream()), 'se3_geo_embedding_bwd_operands')
    g2 = g.reshape(N * N, C)
    db = g2.sum(0)
    return mm_tn_splitk(g2, S[0]), db, mm_tn_splitk(dEk, S[1:].reshape(3 * N * N, C)), db.clone()


def mm_tn_splitk(a, b, splits=64):
    """a (K, M)^T @ b (K, N) for K >> M, N (the weight gradients of the geometric embedding: K = N^2 .. 3 N^2 = 1.5e5 .. 4.4e5 rows onto a
    256 x 256 result).  As ONE product the library runs 32 workgroups for 0.6 ms per call (2.4 ms of a 42 ms training step,
    profiles/r04_kernel_stats_train.csv); cut into `splits` row blocks it is a batched product that fills the chip, the partial results summed
    in a fixed order."""
    K, M = a.shape
    k = K // splits
    if k < 512:
        return mm(a.t(), b)
    head = splits * k
    out = torch.bmm(a[:head].view(splits, k, M).transpose(1, 2), b[:head].view(splits, k, b.shape[1])).sum(0)
    if head < K:
        out += mm(a[head:].t(), b[head:])
    return out


def point_to_node_partition(points, nodes, point_limit):
    """HIP (csrc/partition.hip): (point_to_node (N,) int64, node_masks (M,) bool, node_knn_indices (M, K) int64 padded with N,
    node_knn_masks (M, K) bool) -- nearest node per point, the K nearest own points per node."""
    points = _req(points.contiguous(), torch.float32, 'points', 2)
    nodes = _req(nodes.contiguous(), torch.float32, 'nodes', 2)
    N, M, K = points.shape[0], nodes.shape[0], int(point_limit)
    dev = points.device
    p2n = torch.empty((N,), dtype=torch.int64, device=dev)
    masks = torch.empty((M,), dtype=torch.bool, device=dev)
    knn = torch.empty((M, K), dtype=torch.int64, device=dev)
    knn_masks = torch.empty((M, K), dtype=torch.bool, device=dev)
    check(lib().se3_point_to_node_partition(points.data_ptr(), nodes.data_ptr(), N, M, K, p2n.data_ptr(), masks.data_ptr(),
                                            knn.data_ptr(), knn_masks.data_ptr(), _stream()), 'se3_point_to_node_partition')
    return p2n, masks, knn, knn_masks


def point_to_node_partition_stack(points, nodes, point_lengths, node_lengths, point_limit):
    """HIP (csrc/partition.hip), all clouds in one launch per kernel: stacked fine points / superpoints with per-cloud lengths
    (host lists).  GLOBAL indices: (point_to_node (P,), node_masks (M,) bool, node_knn_indices (M, K) padded with P,
    node_knn_masks (M, K) bool)."""
    points = _req(points.contiguous(), torch.float32, 'points', 2)
    nodes = _req(nodes.contiguous(), torch.float32, 'nodes', 2)
    if len(point_lengths) != len(node_lengths) or sum(point_lengths) != points.shape[0] or sum(node_lengths) != nodes.shape[0]:
        raise RuntimeError('point_to_node_partition_stack: lengths do not add up to the stacked arrays')
    P, M, K = points.shape[0], nodes.shape[0], int(point_limit)
    dev = points.device
    p2n = torch.empty((P,), dtype=torch.int64, device=dev)
    masks = torch.empty((M,), dtype=torch.bool, device=dev)
    knn = torch.empty((M, K), dtype=torch.int64, device=dev)
    knn_masks = torch.empty((M, K), dtype=torch.bool, device=dev)
    check(lib().se3_point_to_node_partition_stack(points.data_ptr(), nodes.data_ptr(), _i64_array(point_lengths),
                                                  _i64_array(node_lengths), len(point_lengths), K, p2n.data_ptr(), masks.data_ptr(),
                                                  knn.data_ptr(), knn_masks.data_ptr(), _stream()), 'se3_point_to_node_partition_stack')
    return p2n, masks, knn, knn_masks


def superpoint_scores_stack(feats, node_masks, ref_rows, src_rows, ref_lengths, src_lengths, ref_mask_offsets, src_mask_offsets,
                            dual_normalization):
    """HIP (csrc/matching.hip), all pairs in one launch per kernel: feats (rows, C) unit superpoint features, node_masks bool
    (nodes,); per pair (host lists) the first ref / src row, the counts and the first ref / src entry of node_masks.  Returns
    (B, max_p N_p * M_p) scores: pair p's (N_p, M_p) matrix at the start of row p, -1 for absent nodes and beyond."""
    feats = _req(feats.contiguous(), torch.float32, 'feats', 2)
    node_masks = _req(node_masks.contiguous(), torch.bool, 'node_masks', 1)
    B, C = len(ref_rows), feats.shape[1]
    for p in range(B):
        if ref_rows[p] + ref_lengths[p] > feats.shape[0] or src_rows[p] + src_lengths[p] > feats.shape[0] or \
                ref_mask_offsets[p] + ref_lengths[p] > node_masks.shape[0] or src_mask_offsets[p] + src_lengths[p] > node_masks.shape[0]:
            raise RuntimeError('superpoint_scores_stack: pair %d exceeds the feature rows / node masks' % p)
    stride = max(n * m for n, m in zip(ref_lengths, src_lengths))
    scores = torch.empty((B, stride), dtype=torch.float32, device=feats.device)
    ws = torch.empty((sum(ref_lengths) + sum(src_lengths),), dtype=torch.float32, device=feats.device)
    check(lib().se3_superpoint_scores_stack(feats.data_ptr(), node_masks.data_ptr(), _i64_array(ref_rows), _i64_array(src_rows),
                                            _i64_array(ref_lengths), _i64_array(src_lengths), _i64_array(ref_mask_offsets),
                                            _i64_array(src_mask_offsets), B, C, 1 if dual_normalization else 0, stride,
                                            scores.data_ptr(), ws.data_ptr(), _stream()), 'se3_superpoint_scores_stack')
    return scores


def patch_scores(feats, ref_idx, src_idx, scale):
    """HIP (csrc/matching.hip): fine-matching scores (B, K, K) of all patch pairs, scale * <feats[ref_idx[b, n]], feats[src_idx[b, m]]>, the
    two gathers fused (an index outside [0, rows) selects the reference's zero padding row)."""
    feats = _req(feats, torch.float32, 'feats', 2)
    ref_idx, src_idx = _req(ref_idx.contiguous(), torch.int64, 'ref_idx', 2), _req(src_idx.contiguous(), torch.int64, 'src_idx', 2)
    B, K = ref_idx.shape
    if tuple(src_idx.shape) != (B, K):
        raise RuntimeError('patch_scores: index shapes %s and %s' % (tuple(ref_idx.shape), tuple(src_idx.shape)))
    out = torch.empty((B, K, K), dtype=torch.float32, device=feats.device)
    check(lib().se3_patch_scores(feats.data_ptr(), ref_idx.data_ptr(), src_idx.data_ptr(), B, K, feats.shape[0], feats.shape[1], float(scale),
                                 out.data_ptr(), _stream()), 'se3_patch_scores')
    return out


def patch_scores_ok(feats, K):
    return feats.is_cuda and feats.dtype == torch.float32 and feats.is_contiguous() and feats.shape[1] % 64 == 0 and K in (64, 128) and \
        not (torch.is_grad_enabled() and feats.requires_grad)


def anchor_mix_stack(x, mixes, starts, lengths):
    """HIP (csrc/rowops.hip): out[a, r] = sum_e mixes[p][a, e] x[e, r] for the packed rows r of pair p (rows of no pair: zero); x (6, R, C)."""
    x = _req(x, torch.float32, 'x', 3)
    mixes = _req(mixes.contiguous(), torch.float32, 'mixes', 3)
    if x.shape[0] != 6 or tuple(mixes.shape) != (len(starts), 6, 6):
        raise RuntimeError('anchor_mix_stack: x %s, mixes %s for %d pairs' % (tuple(x.shape), tuple(mixes.shape), len(starts)))
    out = torch.empty_like(x)
    check(lib().se3_anchor_mix_stack(x.data_ptr(), x.shape[1], x.shape[2], mixes.data_ptr(), _i64_array(starts), _i64_array(lengths), len(starts),
                                     out.data_ptr(), _stream()), 'se3_anchor_mix_stack')
    return out


def superpoint_scores(ref_feats, src_feats, dual_normalization):
    """HIP (csrc/matching.hip): exp(-||f_r - f_s||^2) on unit features with dual normalisation."""
    ref_feats = _req(ref_feats.contiguous(), torch.float32, 'ref_feats', 2)
    src_feats = _req(src_feats.contiguous(), torch.float32, 'src_feats', 2)
    N, C = ref_feats.shape
    M = src_feats.shape[0]
    scores = torch.empty((N, M), dtype=torch.float32, device=ref_feats.device)
    ws = torch.empty((N + M,), dtype=torch.float32, device=ref_feats.device)
    check(lib().se3_superpoint_scores(ref_feats.data_ptr(), src_feats.data_ptr(), N, M, C, 1 if dual_normalization else 0,
                                      scores.data_ptr(), ws.data_ptr(), _stream()), 'se3_superpoint_scores')
    return scores


def mutual_topk_mask(scores, row_masks, col_masks, k, threshold):
    """HIP (csrc/registration.hip): bool (B, R, C) mask of the entries that are among the k largest of their row and of their
    column, above `threshold`, with valid row and column points."""
    scores = _req(scores.contiguous(), torch.float32, 'scores', 3)
    B, R, C = scores.shape
    rm = row_masks.contiguous()
    cm = col_masks.contiguous()
    if rm.dtype != torch.bool or cm.dtype != torch.bool or tuple(rm.shape) != (B, R) or tuple(cm.shape) != (B, C):
        raise RuntimeError('mutual_topk_mask: masks must be bool (B, R) / (B, C)')
    out = torch.empty((B, R, C), dtype=torch.bool, device=scores.device)
    check(lib().se3_mutual_topk_mask(scores.data_ptr(), rm.data_ptr(), cm.data_ptr(), B, R, C, int(k), float(threshold),
                                     out.data_ptr(), _stream()), 'se3_mutual_topk_mask')
    return out


def weighted_procrustes(src, ref, scores, offsets, gate_transform=None, gate_radius=0.0, eps=1e-5):
    """HIP (csrc/registration.hip): one weighted Kabsch solve per segment of the stacked correspondences -> (S, 4, 4).
    gate_transform: (4, 4) shared by all segments, or (S, 4, 4) one per segment (several pairs at once)."""
    src = _req(src.contiguous(), torch.float32, 'src', 2)
    ref = _req(ref.contiguous(), torch.float32, 'ref', 2)
    scores = _req(scores.contiguous(), torch.float32, 'scores', 1)
    offsets = _req(offsets.contiguous(), torch.int64, 'offsets', 1)
    S = offsets.shape[0] - 1
    T = torch.empty((S, 4, 4), dtype=torch.float32, device=src.device)
    gt = _req(gate_transform.contiguous(), torch.float32, 'gate_transform') if gate_transform is not None else None
    per_segment = gt is not None and gt.dim() == 3
    if per_segment and gt.shape[0] != S:
        raise RuntimeError('weighted_procrustes: %d gate transforms for %d segments' % (gt.shape[0], S))
    check(lib().se3_weighted_procrustes_segments(src.data_ptr(), ref.data_ptr(), scores.data_ptr(), offsets.data_ptr(), S,
                                                 gt.data_ptr() if gt is not None else None, 1 if per_segment else 0,
                                                 float(gate_radius), float(eps), T.data_ptr(), _stream()),
          'se3_weighted_procrustes_segments')
    return T


def count_inliers(src, ref, transforms, radius, range_begin=None, range_end=None):
    """HIP: votes[t] = number of correspondences i (in [range_begin[t], range_end[t]) if given, else all) with
    |ref_i - T_t src_i| < radius."""
    src = _req(src.contiguous(), torch.float32, 'src', 2)
    ref = _req(ref.contiguous(), torch.float32, 'ref', 2)
    transforms = _req(transforms.contiguous(), torch.float32, 'transforms', 3)
    votes = torch.empty((transforms.shape[0],), dtype=torch.int32, device=src.device)
    if range_begin is not None:
        range_begin = _req(range_begin.contiguous(), torch.int64, 'range_begin', 1)
        range_end = _req(range_end.contiguous(), torch.int64, 'range_end', 1)
        if range_begin.shape[0] != transforms.shape[0] or range_end.shape[0] != transforms.shape[0]:
            raise RuntimeError('count_inliers: one range per transform')
    check(lib().se3_count_inliers_ranges(src.data_ptr(), ref.data_ptr(), src.shape[0], transforms.data_ptr(), transforms.shape[0],
                                         range_begin.data_ptr() if range_begin is not None else None,
                                         range_end.data_ptr() if range_end is not None else None, float(radius),
                                         votes.data_ptr(), _stream()), 'se3_count_inliers_ranges')
    return votes


def ransac_stack(src, ref, offsets, distance_threshold, ransac_n, num_iterations, seed=0, hypothesis_indices=None, per_hypothesis=False,
                 edge_length_similarity=None, check_distance=False):
    """HIP (csrc/ransac.hip): RANSAC from correspondences for the P = len(offsets) - 1 pairs of stacked src / ref (total, 3), pair p on
    rows [offsets[p], offsets[p+1]) (offsets int64 on the device), three launches and no host synchronisation.  hypothesis_indices:
    (P, num_iterations, ransac_n) int32 pair-local samples instead of the seeded sampler.  Returns a dict of device tensors: transforms
    (P, 4, 4), fitness (P,), inlier_rmse (P,), best_hypothesis (P,) int32 (-1: identity); with per_hypothesis also counts (P, H) int32
    and err_sums (P, H) float32.  edge_length_similarity (a float in (0, 1]) and check_distance switch on Open3D's correspondence checkers
    (se3_ransac_correspondences_checked_stack; a rejected hypothesis scores 0 inliers); per_hypothesis then also returns passed (P, H)
    bool.  Without them the call and its outputs are the unchecked entry's."""
    src = _req(src.contiguous(), torch.float32, 'src', 2)
    ref = _req(ref.contiguous(), torch.float32, 'ref', 2)
    offsets = _req(offsets.contiguous(), torch.int64, 'offsets', 1)
    if src.shape != ref.shape or src.shape[1] != 3:
        raise RuntimeError('ransac_stack: src and ref must both be (total, 3)')
    P, H, rn = offsets.shape[0] - 1, int(num_iterations), int(ransac_n)
    if P < 0 or H < 0:
        raise RuntimeError('ransac_stack: %d pairs, %d iterations' % (P, H))
    dev = src.device
    if hypothesis_indices is not None:
        hypothesis_indices = _req(hypothesis_indices.contiguous(), torch.int32, 'hypothesis_indices', 3)
        if tuple(hypothesis_indices.shape) != (P, H, rn):
            raise RuntimeError('ransac_stack: hypothesis_indices must be (%d, %d, %d)' % (P, H, rn))
    out = dict(transforms=torch.empty((P, 4, 4), dtype=torch.float32, device=dev),
               fitness=torch.empty((P,), dtype=torch.float32, device=dev),
               inlier_rmse=torch.empty((P,), dtype=torch.float32, device=dev),
               best_hypothesis=torch.empty((P,), dtype=torch.int32, device=dev))
    if per_hypothesis:
        out['counts'] = torch.empty((P, H), dtype=torch.int32, device=dev)
        out['err_sums'] = torch.empty((P, H), dtype=torch.float32, device=dev)
    nbytes = lib().se3_ransac_correspondences_workspace_bytes(P, H)
    ws = torch.empty((max(1, nbytes),), dtype=torch.uint8, device=dev)
    hyp = hypothesis_indices.data_ptr() if hypothesis_indices is not None else None
    # (_dp: a call without pairs, or without rows, has empty tensors, and the library refuses null pointers: such a call raised before it
    # took the dummy pointer, and returns the empty / identity results now; nothing is read or written through it when n = 0)
    results = (_dp(out['transforms']), _dp(out['fitness']), _dp(out['inlier_rmse']), _dp(out['best_hypothesis']),
               out['counts'].data_ptr() if per_hypothesis else None, out['err_sums'].data_ptr() if per_hypothesis else None)
    if edge_length_similarity is None and not check_distance:
        check(lib().se3_ransac_correspondences_stack(_dp(src), _dp(ref), offsets.data_ptr(), P, float(distance_threshold), rn, H,
                                                     int(seed) & 0xFFFFFFFFFFFFFFFF, hyp, ws.data_ptr(), nbytes, *results, _stream()),
              'se3_ransac_correspondences_stack')
        return out
    edge = 0.0 if edge_length_similarity is None else float(edge_length_similarity)
    if edge_length_similarity is not None and not 0.0 < edge <= 1.0:
        raise RuntimeError('ransac_stack: edge_length_similarity = %r outside (0, 1]' % (edge_length_similarity,))
    passed = torch.empty((P, H), dtype=torch.uint8, device=dev) if per_hypothesis else None
    check(lib().se3_ransac_correspondences_checked_stack(_dp(src), _dp(ref), offsets.data_ptr(), P, float(distance_threshold), rn,
                                                         H, int(seed) & 0xFFFFFFFFFFFFFFFF, hyp, edge, 1 if check_distance else 0,
                                                         ws.data_ptr(), nbytes, *results,
                                                         passed.data_ptr() if passed is not None else None, _stream()),
          'se3_ransac_correspondences_checked_stack')
    if passed is not None:
        out['passed'] = passed.bool()
    return out


# ---- feature-space matching (csrc/feature_nn.hip) -----------------------------------------------------------------------------------------
CORR_MODES = {'one_way': 0, 'mutual': 1, 'bilateral_mask': 2, 'bilateral_concat': 3}


def _feature_offsets(ref_offsets, src_offsets, nref, nsrc, what):
    ref_offsets = _req(ref_offsets.contiguous(), torch.int64, 'ref_offsets', 1)
    src_offsets = _req(src_offsets.contiguous(), torch.int64, 'src_offsets', 1)
    P = ref_offsets.shape[0] - 1
    if P < 0 or src_offsets.shape[0] != P + 1 or (P == 0 and nref + nsrc > 0):
        raise RuntimeError('%s: ref_offsets and src_offsets must both hold one entry per pair and the end' % what)
    return ref_offsets, src_offsets, P


def feature_nn_stack(ref_feats, src_feats, ref_offsets, src_offsets):
    """HIP (csrc/feature_nn.hip): the nearest neighbour in feature space of every row in the other cloud of its pair, both directions, with
    O(rows) memory.  ref_feats (sum N_p, C) / src_feats (sum M_p, C) float32, pair p on rows [ref_offsets[p], ref_offsets[p+1]) and
    [src_offsets[p], src_offsets[p+1]) (int64 on the device, from 0 to the row count).  Returns (nn_src_indices (sum N_p,) int64 pair-local,
    -1 without a finite candidate; nn_src_sq_distances float32, recomputed as sum (x - y)^2, +inf for -1; nn_ref_indices (sum M_p,);
    nn_ref_sq_distances).  Three launches, no host synchronisation; deterministic."""
    ref_feats = _req(ref_feats.contiguous(), torch.float32, 'ref_feats', 2)
    src_feats = _req(src_feats.contiguous(), torch.float32, 'src_feats', 2)
    nref, nsrc, C = ref_feats.shape[0], src_feats.shape[0], ref_feats.shape[1]
    if src_feats.shape[1] != C or C < 1:
        raise RuntimeError('feature_nn_stack: features of %d and %d channels' % (C, src_feats.shape[1]))
    ref_offsets, src_offsets, P = _feature_offsets(ref_offsets, src_offsets, nref, nsrc, 'feature_nn_stack')
    dev = ref_feats.device
    _same_device(dev, (src_feats, ref_offsets, src_offsets), 'feature_nn_stack')
    nn_src = torch.empty((nref,), dtype=torch.int64, device=dev)
    d_src = torch.empty((nref,), dtype=torch.float32, device=dev)
    nn_ref = torch.empty((nsrc,), dtype=torch.int64, device=dev)
    d_ref = torch.empty((nsrc,), dtype=torch.float32, device=dev)
    nbytes = lib().se3_feature_nn_workspace_bytes(nref, nsrc)
    ws = torch.empty((max(1, nbytes),), dtype=torch.uint8, device=dev)
    check(lib().se3_feature_nn_stack(ref_feats.data_ptr(), src_feats.data_ptr(), ref_offsets.data_ptr(), src_offsets.data_ptr(), P, nref, nsrc,
                                     C, ws.data_ptr(), nbytes, nn_src.data_ptr(), d_src.data_ptr(), nn_ref.data_ptr(), d_ref.data_ptr(),
                                     _stream()), 'se3_feature_nn_stack')
    return nn_src, d_src, nn_ref, d_ref


def feature_corr_stack(nn_src, nn_ref, ref_offsets, src_offsets, mode):
    """HIP (csrc/feature_nn.hip): the correspondence lists of feature_nn_stack's index arrays for all pairs: count, exclusive scan, fill, and
    ONE host synchronisation (the pair boundaries of the list).  mode: a key of CORR_MODES.  Returns (ref_corr_indices, src_corr_indices)
    int64 pair-local on the device, and the host list of P + 1 boundaries: pair p's entries are [bounds[p], bounds[p+1])."""
    nn_src = _req(nn_src.contiguous(), torch.int64, 'nn_src', 1)
    nn_ref = _req(nn_ref.contiguous(), torch.int64, 'nn_ref', 1)
    nref, nsrc = nn_src.shape[0], nn_ref.shape[0]
    ref_offsets, src_offsets, P = _feature_offsets(ref_offsets, src_offsets, nref, nsrc, 'feature_corr_stack')
    dev = nn_src.device
    _same_device(dev, (nn_ref, ref_offsets, src_offsets), 'feature_corr_stack')
    m = CORR_MODES[mode]
    entry_offsets = torch.empty((nref + nsrc + 1,), dtype=torch.int64, device=dev)
    args = (nn_src.data_ptr(), nn_ref.data_ptr(), ref_offsets.data_ptr(), src_offsets.data_ptr(), P, nref, nsrc, m)
    check(lib().se3_feature_corr_count_stack(*args, entry_offsets.data_ptr(), _stream()), 'se3_feature_corr_count_stack')
    bounds = entry_offsets[ref_offsets + src_offsets].cpu().tolist()      # the one read-back
    total = bounds[-1] if bounds else 0
    ref_idx = torch.empty((total,), dtype=torch.int64, device=dev)
    src_idx = torch.empty((total,), dtype=torch.int64, device=dev)
    check(lib().se3_feature_corr_fill_stack(*args, entry_offsets.data_ptr(), total, ref_idx.data_ptr(), src_idx.data_ptr(), _stream()),
          'se3_feature_corr_fill_stack')
    return ref_idx, src_idx, bounds


# ---- evaluation (csrc/evaluation.hip) ---------------------------------------------------------------------------------------------------
class GroundTruthOverlaps:
    """Result of gt_node_overlaps_stack for B pairs, all on the device: `dense` packs pair p's (N_p, M_p) overlap matrix from entry
    dense_offsets[p] on; `indices` (capacity, 2) / `overlaps` (capacity,) hold pair p's compacted list from the same offset, `counts` (B,)
    its length.  `lists()` reads the counts (one host synchronisation) and returns per pair ((C_p, 2) int64, (C_p,) float32) views."""

    def __init__(self, dense, dense_offsets, shapes, indices, overlaps, counts):
        self.dense, self.dense_offsets, self.shapes = dense, dense_offsets, shapes
        self.indices, self.overlaps, self.counts = indices, overlaps, counts

    def block(self, p):
        n, m = self.shapes[p]
        return self.dense[self.dense_offsets[p]:self.dense_offsets[p] + n * m].view(n, m)

    def lists(self):
        out = []
        for p, c in enumerate(self.counts.tolist()):
            a = self.dense_offsets[p]
            out.append((self.indices[a:a + c], self.overlaps[a:a + c]))
        return out


def gt_node_overlaps_stack(points_f, points_c, node_lengths, knn, knn_masks, node_masks, transforms, pos_radius):
    """HIP (csrc/evaluation.hip): get_node_correspondences for the B = len(node_lengths) / 2 pairs of a stacked batch (clouds ref0, src0,
    ref1, ...) in three launches and no host synchronisation.  knn / knn_masks / node_masks as point_to_node_partition_stack returns them
    (GLOBAL fine-point indices); transforms (B, 4, 4) ground truth.  Returns a GroundTruthOverlaps."""
    points_f = _req(points_f.contiguous(), torch.float32, 'points_f', 2)
    points_c = _req(points_c.contiguous(), torch.float32, 'points_c', 2)
    knn = _req(knn.contiguous(), torch.int64, 'knn', 2)
    knn_masks = _req(knn_masks.contiguous(), torch.bool, 'knn_masks', 2)
    node_masks = _req(node_masks.contiguous(), torch.bool, 'node_masks', 1)
    transforms = _req(transforms.contiguous(), torch.float32, 'transforms', 3)
    lengths = [int(n) for n in (node_lengths.tolist() if torch.is_tensor(node_lengths) else node_lengths)]
    nc, M, K = len(lengths), points_c.shape[0], knn.shape[1]
    B = nc // 2
    if nc % 2 or nc < 2 or sum(lengths) != M or knn.shape[0] != M or knn_masks.shape != knn.shape or node_masks.shape[0] != M:
        raise RuntimeError('gt_node_overlaps_stack: an even number of clouds whose node lengths match the partition')
    if transforms.shape[0] != B or tuple(transforms.shape[1:]) != (4, 4):
        raise RuntimeError('gt_node_overlaps_stack: transforms must be (%d, 4, 4)' % B)
    shapes = [(lengths[2 * p], lengths[2 * p + 1]) for p in range(B)]
    offs = exclusive_offsets(n * m for n, m in shapes)
    dev = points_c.device
    dense = torch.empty((offs[-1],), dtype=torch.float32, device=dev)
    indices = torch.empty((offs[-1], 2), dtype=torch.int64, device=dev)
    overlaps = torch.empty((offs[-1],), dtype=torch.float32, device=dev)
    counts = torch.empty((B,), dtype=torch.int64, device=dev)
    ws = torch.empty((max(1, lib().se3_gt_node_overlaps_workspace_bytes(M)),), dtype=torch.uint8, device=dev)
    pr = float(pos_radius)
    check(lib().se3_gt_node_overlaps_stack(points_f.data_ptr(), points_c.data_ptr(), _i64_array(lengths), nc, knn.data_ptr(),
                                           knn_masks.data_ptr(), node_masks.data_ptr(), K, transforms.data_ptr(), pr, pr ** 2,
                                           ws.data_ptr(), dense.data_ptr(), indices.data_ptr(), overlaps.data_ptr(), counts.data_ptr(),
                                           _stream()), 'se3_gt_node_overlaps_stack')
    return GroundTruthOverlaps(dense, offs[:-1], shapes, indices, overlaps, counts)


def registration_metrics_stack(pairs, gt_transforms, acceptance_overlap, acceptance_radius, rmse_threshold, rre_threshold, rte_threshold,
                               kitti):
    """HIP (csrc/evaluation.hip): the Evaluator's PIR, IR, RRE, RTE, RMSE, RR for B pairs in one launch.  pairs[p] = (overlaps (N, M),
    ref_node_corr_indices, src_node_corr_indices, ref_corr_points, src_corr_points, estimated_transform (4, 4), src_points or None);
    gt_transforms (B, 4, 4).  Returns (B, 6) float32 in that column order (RMSE NaN with kitti)."""
    B = len(pairs)
    gt_transforms = _req(gt_transforms.contiguous(), torch.float32, 'gt_transforms', 3)
    if gt_transforms.shape[0] != B or tuple(gt_transforms.shape[1:]) != (4, 4):
        raise RuntimeError('registration_metrics_stack: gt_transforms must be (%d, 4, 4)' % B)
    dev = gt_transforms.device
    table, keep = [], []        # (keep: the contiguous operands stay referenced until the launch is queued)
    for p, (ov, ri, si, rc, sc, est, sp) in enumerate(pairs):
        ov = _req(ov.contiguous(), torch.float32, 'overlaps', 2)
        ri = _req(ri.contiguous(), torch.int64, 'ref_node_corr_indices', 1)
        si = _req(si.contiguous(), torch.int64, 'src_node_corr_indices', 1)
        rc = _req(rc.contiguous(), torch.float32, 'ref_corr_points', 2)
        sc = _req(sc.contiguous(), torch.float32, 'src_corr_points', 2)
        est = _req(est.contiguous(), torch.float32, 'estimated_transform', 2)
        if ri.shape != si.shape or rc.shape != sc.shape or rc.shape[1] != 3 or tuple(est.shape) != (4, 4):
            raise RuntimeError('registration_metrics_stack: pair %d has mismatched shapes' % p)
        if not kitti:
            sp = _req(sp.contiguous(), torch.float32, 'src_points', 2)
            if sp.shape[1] != 3:
                raise RuntimeError('registration_metrics_stack: src_points must be (n, 3)')
        _same_device(dev, (ov, ri, si, rc, sc, est) + ((sp,) if not kitti else ()), 'registration_metrics_stack')
        keep.append((ov, ri, si, rc, sc, est, sp))
        table += [ov.data_ptr(), ov.shape[0], ov.shape[1], ri.data_ptr(), si.data_ptr(), ri.shape[0], rc.data_ptr(), sc.data_ptr(),
                  rc.shape[0], est.data_ptr(), gt_transforms[p].data_ptr(), 0 if kitti else sp.data_ptr(), 0 if kitti else sp.shape[0],
                  0, 0, 0]
    rows = torch.empty((B, 6), dtype=torch.float32, device=dev)
    if B == 0:
        return rows
    tab = to_device(table, torch.int64, dev)
    check(lib().se3_registration_metrics_stack(tab.data_ptr(), B, float(acceptance_overlap), float(acceptance_radius), float(rmse_threshold),
                                               float(rre_threshold), float(rte_threshold), 1 if kitti else 0, rows.data_ptr(), _stream()),
          'se3_registration_metrics_stack')
    return rows


# ---- eval.py's benchmark metrics (csrc/benchmark.hip) -------------------------------------------------------------------------------------
def _same_device(dev, tensors, what):
    for t in tensors:
        if t.device != dev:
            raise RuntimeError('%s: all tensors on %s' % (what, dev))


def benchmark_correspondences_stack(ref, src, offsets, max_count, transforms, positive_radius):
    """HIP: evaluate_correspondences for the P = len(offsets) - 1 pairs of stacked ref / src correspondence points (total, 3), pair p on
    rows [offsets[p], offsets[p+1]) (offsets int64 on the device); max_count (host int) bounds every pair's count; transforms (P, 4, 4)
    float32 ground truth.  Returns (P, 4) float64: overlap, inlier_ratio, residual, num_corr."""
    ref = _req(ref.contiguous(), torch.float32, 'ref', 2)
    src = _req(src.contiguous(), torch.float32, 'src', 2)
    offsets = _req(offsets.contiguous(), torch.int64, 'offsets', 1)
    transforms = _req(transforms.contiguous(), torch.float32, 'transforms', 3)
    P = offsets.shape[0] - 1
    if ref.shape != src.shape or ref.shape[1] != 3 or tuple(transforms.shape) != (P, 4, 4):
        raise RuntimeError('benchmark_correspondences_stack: ref / src (total, 3) and transforms (%d, 4, 4) expected' % P)
    dev = ref.device
    _same_device(dev, (src, offsets, transforms), 'benchmark_correspondences_stack')
    out = torch.empty((P, 4), dtype=torch.float64, device=dev)
    nbytes = lib().se3_benchmark_correspondences_workspace_bytes(P)
    ws = torch.empty((max(1, nbytes),), dtype=torch.uint8, device=dev)
    check(lib().se3_benchmark_correspondences_stack(ref.data_ptr(), src.data_ptr(), offsets.data_ptr(), P, int(max_count),
                                                    transforms.data_ptr(), float(positive_radius), ws.data_ptr(), nbytes, out.data_ptr(),
                                                    _stream()), 'se3_benchmark_correspondences_stack')
    return out


def benchmark_sparse_stack(ref_idx, src_idx, pred_offsets, gt_idx, gt_offsets, node_counts):
    """HIP: evaluate_sparse_correspondences for P pairs.  ref_idx / src_idx (total,) and gt_idx (total_gt, 2) int64 on the device, pair p's
    on [pred_offsets[p], pred_offsets[p+1]) / [gt_offsets[p], gt_offsets[p+1]) (device int64); node_counts: host list of P (N_p, M_p).
    Returns (P, 3) float64: precision, recall, hit_ratio."""
    ref_idx = _req(ref_idx.contiguous(), torch.int64, 'ref_node_indices', 1)
    src_idx = _req(src_idx.contiguous(), torch.int64, 'src_node_indices', 1)
    gt_idx = _req(gt_idx.contiguous(), torch.int64, 'gt_node_corr_indices', 2)
    pred_offsets = _req(pred_offsets.contiguous(), torch.int64, 'pred_offsets', 1)
    gt_offsets = _req(gt_offsets.contiguous(), torch.int64, 'gt_offsets', 1)
    P = pred_offsets.shape[0] - 1
    if ref_idx.shape != src_idx.shape or gt_idx.shape[1] != 2 or gt_offsets.shape[0] != P + 1 or len(node_counts) != P:
        raise RuntimeError('benchmark_sparse_stack: mismatched shapes')
    dev = ref_idx.device
    _same_device(dev, (src_idx, gt_idx, pred_offsets, gt_offsets), 'benchmark_sparse_stack')
    counts = [(int(n), int(m)) for n, m in node_counts]
    if any(n < 0 or m < 0 for n, m in counts):
        raise RuntimeError('benchmark_sparse_stack: negative node count')
    words = exclusive_offsets(lib().se3_benchmark_sparse_words(n, m) for n, m in counts)
    host_counts = _i64_array([v for c in counts for v in c] or [0])
    nbytes = lib().se3_benchmark_sparse_workspace_bytes(host_counts, P)
    if nbytes != 4 * words[-1]:
        raise RuntimeError('benchmark_sparse_stack: workspace layout mismatch')
    ws = torch.empty((max(4, nbytes),), dtype=torch.uint8, device=dev)
    out = torch.empty((P, 3), dtype=torch.float64, device=dev)
    if P == 0:
        return out
    dev_counts = to_device([v for c in counts for v in c], torch.int64, dev)
    dev_words = to_device(words, torch.int64, dev)
    check(lib().se3_benchmark_sparse_stack(ref_idx.data_ptr(), src_idx.data_ptr(), pred_offsets.data_ptr(), gt_idx.data_ptr(),
                                           gt_offsets.data_ptr(), dev_counts.data_ptr(), dev_words.data_ptr(), P, ws.data_ptr(), nbytes,
                                           out.data_ptr(), _stream()), 'se3_benchmark_sparse_stack')
    return out


def benchmark_transform_error_stack(gt_transforms, est_transforms, covariances=None, has_covariance=None):
    """HIP: compute_transform_error and compute_registration_error for P pairs, float64.  gt / est (P, 4, 4), covariances (P, 6, 6) float64
    and has_covariance (P,) int32 on the device (None: no pair has one).  Returns (P, 3) float64: err (NaN without covariance), rre, rte."""
    gt = _req(gt_transforms.contiguous(), torch.float64, 'gt_transforms', 3)
    est = _req(est_transforms.contiguous(), torch.float64, 'est_transforms', 3)
    P = gt.shape[0]
    if tuple(gt.shape) != (P, 4, 4) or est.shape != gt.shape:
        raise RuntimeError('benchmark_transform_error_stack: gt and est must be (P, 4, 4)')
    if (covariances is None) != (has_covariance is None):
        raise RuntimeError('benchmark_transform_error_stack: covariances and has_covariance go together')
    dev = gt.device
    if covariances is not None:
        covariances = _req(covariances.contiguous(), torch.float64, 'covariances', 3)
        has_covariance = _req(has_covariance.contiguous(), torch.int32, 'has_covariance', 1)
        if tuple(covariances.shape) != (P, 6, 6) or tuple(has_covariance.shape) != (P,):
            raise RuntimeError('benchmark_transform_error_stack: covariances (P, 6, 6) and has_covariance (P,) expected')
        _same_device(dev, (covariances, has_covariance), 'benchmark_transform_error_stack')
    _same_device(dev, (est,), 'benchmark_transform_error_stack')
    out = torch.empty((P, 3), dtype=torch.float64, device=dev)
    check(lib().se3_benchmark_transform_error_stack(gt.data_ptr(), est.data_ptr(), None if covariances is None else covariances.data_ptr(),
                                                    None if has_covariance is None else has_covariance.data_ptr(), P, out.data_ptr(),
                                                    _stream()), 'se3_benchmark_transform_error_stack')
    return out


def benchmark_summary(rows, is_gt, group_lengths, kitti, inlier_ratio_threshold, rmse_threshold, rre_threshold, rte_threshold):
    """HIP: eval.py's summaries.  rows (P, 6) float64 (precision, inlier_ratio, overlap, err, rre, rte), is_gt (P,) int32 on the device;
    group_lengths: host list of the groups' pair counts (consecutive rows).  Returns (groups (G, 14), overall (14,)) float64."""
    rows = _req(rows.contiguous(), torch.float64, 'rows', 2)
    is_gt = _req(is_gt.contiguous(), torch.int32, 'is_gt', 1)
    P, G = rows.shape[0], len(group_lengths)
    lengths = [int(n) for n in group_lengths]
    if rows.shape[1] != 6 or is_gt.shape[0] != P or sum(lengths) != P or any(n < 0 for n in lengths):
        raise RuntimeError('benchmark_summary: rows (P, 6), is_gt (P,) and group lengths summing to P expected')
    dev = rows.device
    _same_device(dev, (is_gt,), 'benchmark_summary')
    offsets = device_offsets(lengths, dev)
    groups = torch.empty((max(G, 1), 14), dtype=torch.float64, device=dev)
    overall = torch.empty((14,), dtype=torch.float64, device=dev)
    check(lib().se3_benchmark_summary(rows.data_ptr(), is_gt.data_ptr(), offsets.data_ptr(), G, max(lengths, default=0), 1 if kitti else 0,
                                      float(inlier_ratio_threshold), float(rmse_threshold), float(rre_threshold), float(rte_threshold),
                                      groups.data_ptr(), overall.data_ptr(), _stream()), 'se3_benchmark_summary')
    return groups[:G], overall


# ---- pair ground truth: nearest neighbour, overlap, correspondences, gt.info covariance (csrc/pair_geometry.hip) ---------------------------
_ws_pair_grid = Workspace(1 << 22)          # the cell grid of the call in flight on a stream


def _pair_points(t, name):
    """(rows, 3) float32 or float64 on the device, as it is (the kernels promote on load); returns (tensor, elem flag)."""
    if torch.is_tensor(t) and t.dtype not in (torch.float32, torch.float64):
        raise RuntimeError('%s must be float32 or float64, got %s' % (name, t.dtype))
    t = _req(t, t.dtype if torch.is_tensor(t) else torch.float32, name, 2)
    if t.shape[1] != 3:
        raise RuntimeError('%s must be (rows, 3)' % name)
    return t, 1 if t.dtype == torch.float64 else 0


def _pair_offsets(lengths, rows, what):
    lengths = [int(n) for n in lengths]
    if len(lengths) > PAIR_MAX_PAIRS or any(n < 0 for n in lengths) or sum(lengths) != rows:
        raise RuntimeError('%s: at most %d pairs per call, with lengths that sum to the %d rows given' % (what, PAIR_MAX_PAIRS, rows))
    return _i64_array(exclusive_offsets(lengths))


def _pair_transforms(transforms, P, what):
    """(P, 4, 4) float64 on the HOST (the library checks it and passes it to the kernels by value)."""
    t = transforms.detach().to(device='cpu', dtype=torch.float64).contiguous()
    if tuple(t.shape) != (P, 4, 4):
        raise RuntimeError('%s: transforms must be (%d, 4, 4)' % (what, P))
    return t


_pair_dummy = {}


def _dp(t):
    """data_ptr of a tensor, or of a small per-device buffer for an empty one (the library refuses null pointers; nothing is read or written
    through the pointer of an array without rows)."""
    if t.numel():
        return t.data_ptr()
    d = _pair_dummy.get(t.device)
    if d is None:
        d = _pair_dummy[t.device] = torch.zeros((64,), dtype=torch.uint8, device=t.device)
    return d.data_ptr()


class PairGrid:
    """The cell grid of a stacked support (pair_grid_build), valid until the next build on the same stream."""
    __slots__ = ('ws', 'nbytes', 'ns_total', 'num_pairs', 'device')

    def __init__(self, ws, nbytes, ns_total, num_pairs):
        self.ws, self.nbytes, self.ns_total, self.num_pairs, self.device = ws, nbytes, ns_total, num_pairs, ws.device


def pair_grid_build(s_points, s_lengths, transforms, cell_hint=0.0):
    """HIP: the float64 cell grid over the transformed support of each pair.  s_points (total, 3) float32 / float64 on the device, pair p on
    the next s_lengths[p] rows (host ints); transforms (P, 4, 4), moved to the host as float64; cell_hint: the ball radius, or 0 for the
    nearest-neighbour grid.  Returns a PairGrid for pair_nearest_neighbor_stack / pair_ball_*_stack."""
    s, elem = _pair_points(s_points, 's_points')
    P = len(s_lengths)
    offsets = _pair_offsets(s_lengths, s.shape[0], 'pair_grid_build')
    T = _pair_transforms(transforms, P, 'pair_grid_build')
    nbytes = lib().se3_pair_grid_workspace_bytes(s.shape[0], P)
    stream = _stream()
    ws = _ws_pair_grid.get(s.device, stream.value, nbytes)
    check(lib().se3_pair_grid_build(_dp(s), elem, offsets, P, T.data_ptr(), float(cell_hint), ws.data_ptr(), nbytes, stream),
          'se3_pair_grid_build')
    return PairGrid(ws, nbytes, s.shape[0], P)


def _pair_query(grid, q_points, q_lengths, what):
    q, elem = _pair_points(q_points, 'q_points')
    if q.device != grid.device or len(q_lengths) != grid.num_pairs:
        raise RuntimeError('%s: %d pairs on %s expected' % (what, grid.num_pairs, grid.device))
    return q, elem, _pair_offsets(q_lengths, q.shape[0], what)


def pair_nearest_neighbor_stack(grid, q_points, q_lengths):
    """HIP: exact nearest support point of every query row in its own pair's transformed support.  Returns (distances (nq,) float64,
    indices (nq,) int64 pair-local; inf / -1 for an empty support)."""
    q, elem, offsets = _pair_query(grid, q_points, q_lengths, 'pair_nearest_neighbor_stack')
    dist = torch.empty((q.shape[0],), dtype=torch.float64, device=q.device)
    idx = torch.empty((q.shape[0],), dtype=torch.int64, device=q.device)
    check(lib().se3_pair_nearest_neighbor_stack(grid.ws.data_ptr(), grid.nbytes, grid.ns_total, _dp(q), elem, offsets, grid.num_pairs,
                                                _dp(dist), _dp(idx), _stream()), 'se3_pair_nearest_neighbor_stack')
    return dist, idx


def _pair_radii(radius, P, what):
    """None for one radius, else the (P,) float64 host array of a radius per pair."""
    if not isinstance(radius, (list, tuple)):
        return None
    if len(radius) != P:
        raise RuntimeError('%s: one radius per pair: %d given for %d pairs' % (what, len(radius), P))
    return (ctypes.c_double * max(P, 1))(*[float(r) for r in radius])


def pair_ball_count_stack(grid, q_points, q_lengths, radius):
    """HIP: pass 1 of the ball query.  radius: one number, or a list of one per pair.  Returns row_offsets (nq + 1,) int64 on the device:
    the exclusive scan of the hits per query row."""
    q, elem, offsets = _pair_query(grid, q_points, q_lengths, 'pair_ball_count_stack')
    row_offsets = torch.empty((q.shape[0] + 1,), dtype=torch.int64, device=q.device)
    radii = _pair_radii(radius, grid.num_pairs, 'pair_ball_count_stack')
    if radii is not None:
        check(lib().se3_pair_ball_count_radii_stack(grid.ws.data_ptr(), grid.nbytes, grid.ns_total, _dp(q), elem, offsets, grid.num_pairs, radii,
                                                    row_offsets.data_ptr(), _stream()), 'se3_pair_ball_count_radii_stack')
        return row_offsets
    check(lib().se3_pair_ball_count_stack(grid.ws.data_ptr(), grid.nbytes, grid.ns_total, _dp(q), elem, offsets, grid.num_pairs,
                                          float(radius), row_offsets.data_ptr(), _stream()), 'se3_pair_ball_count_stack')
    return row_offsets


def pair_ball_fill_stack(grid, q_points, q_lengths, radius, row_offsets, total):
    """HIP: pass 2.  Returns (total, 2) int64: (i, j) pair-local, rows ascending in i, j ascending within a row."""
    q, elem, offsets = _pair_query(grid, q_points, q_lengths, 'pair_ball_fill_stack')
    row_offsets = _req(row_offsets, torch.int64, 'row_offsets', 1)
    if row_offsets.shape[0] != q.shape[0] + 1 or row_offsets.device != q.device:
        raise RuntimeError('pair_ball_fill_stack: row_offsets of pair_ball_count_stack expected')
    out = torch.empty((int(total), 2), dtype=torch.int64, device=q.device)
    radii = _pair_radii(radius, grid.num_pairs, 'pair_ball_fill_stack')
    if radii is not None:
        check(lib().se3_pair_ball_fill_radii_stack(grid.ws.data_ptr(), grid.nbytes, grid.ns_total, _dp(q), elem, offsets, grid.num_pairs, radii,
                                                   row_offsets.data_ptr(), int(total), _dp(out), _stream()), 'se3_pair_ball_fill_radii_stack')
        return out
    check(lib().se3_pair_ball_fill_stack(grid.ws.data_ptr(), grid.nbytes, grid.ns_total, _dp(q), elem, offsets, grid.num_pairs,
                                         float(radius), row_offsets.data_ptr(), int(total), _dp(out), _stream()),
          'se3_pair_ball_fill_stack')
    return out


def pair_overlap_stack(nn_distances, q_lengths, radius):
    """HIP: count(d d < r r) / rows per pair of stacked nearest-neighbour distances (float64).  Returns (P,) float64; NaN without rows."""
    d = _req(nn_distances, torch.float64, 'nn_distances', 1)
    P = len(q_lengths)
    offsets = _pair_offsets(q_lengths, d.shape[0], 'pair_overlap_stack')
    out = torch.empty((P,), dtype=torch.float64, device=d.device)
    check(lib().se3_pair_overlap_stack(_dp(d), offsets, P, float(radius), _dp(out), _stream()), 'se3_pair_overlap_stack')
    return out


def pair_info_covariance_stack(src_points, s_lengths, transforms, selected, selected_lengths):
    """HIP: the gt.info covariance sum G^T G over the transformed src points src[selected] of each pair (selected: pair-local int64 on the
    device, pair p's the next selected_lengths[p] entries).  Returns (P, 6, 6) float64."""
    s, elem = _pair_points(src_points, 'src_points')
    sel = _req(selected, torch.int64, 'selected', 1)
    P = len(s_lengths)
    if len(selected_lengths) != P or sel.device != s.device:
        raise RuntimeError('pair_info_covariance_stack: one selection per pair, on %s' % s.device)
    s_off = _pair_offsets(s_lengths, s.shape[0], 'pair_info_covariance_stack')
    k_off = _pair_offsets(selected_lengths, sel.shape[0], 'pair_info_covariance_stack')
    T = _pair_transforms(transforms, P, 'pair_info_covariance_stack')
    out = torch.empty((P, 6, 6), dtype=torch.float64, device=s.device)
    check(lib().se3_pair_info_covariance_stack(_dp(s), elem, s_off, T.data_ptr(), _dp(sel), k_off, P, _dp(out), _stream()),
          'se3_pair_info_covariance_stack')
    return out


# ---- scan preparation: voxel downsampling, k nearest neighbours, k-NN normals (csrc/voxel_downsample.hip, csrc/knn_normals.hip) ---------------
KNN_MAX = CONSTANTS['SE3_KNN_MAX']                 # one list entry per lane of a wave
_ws_voxel = Workspace(1 << 22)


def voxel_downsample_stack(points, lengths, voxel_size, normals=None):
    """HIP: Open3D's voxel_down_sample of stacked clouds.  points (total, 3) float32 / float64 on the device, cloud c on the next lengths[c]
    rows (host ints); normals: None or the same shape and type.  Returns (out_points (total, 3) float64, out_normals or None, words): the
    clouds' voxel means back to back in out_points[:sum(counts)]; words (len(lengths) + 1,) int32 on the DEVICE holds the counts and, last,
    the status word (0; bit 1: a non-finite value, bit 2: an axis needs 2^21 voxels or more; the count of a refused cloud is minus its bits)
    -- one copy fetches both."""
    p, elem = _pair_points(points, 'points')
    nr = None
    if normals is not None:
        nr, nelem = _pair_points(normals, 'normals')
        if nr.shape != p.shape or nelem != elem or nr.device != p.device:
            raise RuntimeError('voxel_downsample_stack: normals must have the shape, type and device of the points')
    C = len(lengths)
    offsets = _pair_offsets(lengths, p.shape[0], 'voxel_downsample_stack')
    out = torch.empty((p.shape[0], 3), dtype=torch.float64, device=p.device)
    out_n = torch.empty_like(out) if nr is not None else None
    words = torch.empty((C + 1,), dtype=torch.int32, device=p.device)
    nbytes = lib().se3_voxel_downsample_workspace_bytes(p.shape[0], C)
    stream = _stream()
    ws = _ws_voxel.get(p.device, stream.value, nbytes)
    check(lib().se3_voxel_downsample_stack(_dp(p), elem, None if nr is None else _dp(nr), offsets, C, float(voxel_size), _dp(out),
                                           None if out_n is None else _dp(out_n), words.data_ptr(), words[C:].data_ptr(), ws.data_ptr(),
                                           nbytes, stream), 'se3_voxel_downsample_stack')
    return out, out_n, words


def _knn_k(k, what):
    k = int(k)
    if not 1 <= k <= KNN_MAX:
        raise RuntimeError('%s: k %d not in [1, %d]' % (what, k, KNN_MAX))
    return k


def knn_stack(grid, q_points, q_lengths, k):
    """HIP: the k nearest support points of every query row in its own cloud of `grid` (pair_grid_build with identity transforms and
    cell_hint 0).  Returns (idx (nq, k) int64 cloud-local, d2 (nq, k) float64), rows ascending by (d2, index); -1 / inf where the cloud
    has fewer than k points."""
    q, elem, offsets = _pair_query(grid, q_points, q_lengths, 'knn_stack')
    k = _knn_k(k, 'knn_stack')
    idx = torch.empty((q.shape[0], k), dtype=torch.int64, device=q.device)
    d2 = torch.empty((q.shape[0], k), dtype=torch.float64, device=q.device)
    check(lib().se3_knn_stack(grid.ws.data_ptr(), grid.nbytes, grid.ns_total, _dp(q), elem, offsets, grid.num_pairs, k, _dp(idx), _dp(d2),
                              _stream()), 'se3_knn_stack')
    return idx, d2


def knn_normals_stack(grid, q_points, q_lengths, k, viewpoints=None):
    """HIP: the normal of every query row from its k nearest support points, fused (no (nq, k) table is written).  viewpoints: None or
    (clouds, 3), moved to the host as float64.  Returns (nq, 3) float64."""
    q, elem, offsets = _pair_query(grid, q_points, q_lengths, 'knn_normals_stack')
    k = _knn_k(k, 'knn_normals_stack')
    view = None
    if viewpoints is not None:
        view = torch.as_tensor(viewpoints).detach().to(device='cpu', dtype=torch.float64).contiguous()
        if tuple(view.shape) != (grid.num_pairs, 3):
            raise RuntimeError('knn_normals_stack: viewpoints must be (%d, 3)' % grid.num_pairs)
    out = torch.empty((q.shape[0], 3), dtype=torch.float64, device=q.device)
    check(lib().se3_knn_normals_stack(grid.ws.data_ptr(), grid.nbytes, grid.ns_total, _dp(q), elem, offsets, grid.num_pairs, k,
                                      None if view is None or grid.num_pairs == 0 else view.data_ptr(), _dp(out), _stream()),
          'se3_knn_normals_stack')
    return out


# ---- ICP refinement of stacked pairs (csrc/icp.hip) --------------------------------------------------------------------------------------------
ICP_MODES = {'point_to_point': CONSTANTS['SE3_ICP_POINT_TO_POINT'], 'point_to_plane': CONSTANTS['SE3_ICP_POINT_TO_PLANE']}
ICP_STATUS = {name.lower(): CONSTANTS['SE3_ICP_' + name] for name in ('NONFINITE', 'TOO_FEW', 'SINGULAR', 'EMPTY', 'STEP_REFUSED')}
ICP_MAX_ITERATION = CONSTANTS['SE3_ICP_MAX_ITERATION']
_ws_icp = Workspace(1 << 20)


def icp_outputs(P, dev):
    """The uninitialised result tensors of icp_stack for P pairs (P = 0: the result of a call without pairs)."""
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    return {'transforms': torch.empty((P, 4, 4), **f64), 'fitness': torch.empty((P,), **f64), 'inlier_rmse': torch.empty((P,), **f64),
            'iterations': torch.empty((P,), **i32), 'converged': torch.empty((P,), **i32), 'status': torch.empty((P,), **i32)}


def icp_stack(grid, src_points, src_lengths, init_transforms, max_correspondence_distance, mode, ref_normals=None, relative_fitness=1e-6,
              relative_rmse=1e-6, max_iteration=30, return_correspondences=False):
    """HIP: ICP of up to PAIR_MAX_PAIRS stacked pairs, resident on the device.  grid: pair_grid_build over the REFERENCE clouds with identity
    transforms and cell_hint = max_correspondence_distance; src_points (total, 3) float32 / float64, pair p on the next src_lengths[p] rows;
    init_transforms (P, 4, 4) float64 on the DEVICE; mode: a key of ICP_MODES; ref_normals (grid.ns_total, 3) float32 / float64 or None.
    Every launch is enqueued without a host synchronisation.  Returns a dict of device tensors: transforms (P, 4, 4) float64, fitness,
    inlier_rmse (P,) float64, iterations, converged, status (P,) int32 (status: a sum of the ICP_STATUS bits), and with
    return_correspondences the final pair-local reference row of every stacked source row (int64, -1 for none)."""
    s, elem = _pair_points(src_points, 'src_points')
    P = len(src_lengths)
    if s.device != grid.device or P != grid.num_pairs:
        raise RuntimeError('icp_stack: %d pairs on %s expected' % (grid.num_pairs, grid.device))
    if mode not in ICP_MODES:
        raise ValueError('icp_stack: estimation %r is not one of %s' % (mode, ', '.join(sorted(ICP_MODES))))
    offsets = _pair_offsets(src_lengths, s.shape[0], 'icp_stack')
    T0 = _req(init_transforms, torch.float64, 'init_transforms', 3)
    if tuple(T0.shape) != (P, 4, 4) or T0.device != s.device:
        raise RuntimeError('icp_stack: init_transforms must be (%d, 4, 4) on %s' % (P, s.device))
    nr, nelem = None, 1
    if ref_normals is not None:
        nr, nelem = _pair_points(ref_normals, 'ref_normals')
        if nr.shape[0] != grid.ns_total or nr.device != s.device:
            raise RuntimeError('icp_stack: ref_normals must be (%d, 3) on %s' % (grid.ns_total, s.device))
    elif ICP_MODES[mode] == ICP_MODES['point_to_plane']:
        raise RuntimeError('icp_stack: point_to_plane needs the reference normals')
    dev = s.device
    out = icp_outputs(P, dev)
    corr = torch.empty((s.shape[0],), dtype=torch.int64, device=dev) if return_correspondences else None
    nbytes = lib().se3_icp_workspace_bytes(s.shape[0], P)
    stream = _stream()
    ws = _ws_icp.get(dev, stream.value, nbytes)
    check(lib().se3_icp_stack(grid.ws.data_ptr(), grid.nbytes, grid.ns_total, _dp(s), elem, offsets, P, None if nr is None else _dp(nr), nelem,
                              _dp(T0), float(max_correspondence_distance), ICP_MODES[mode], float(relative_fitness), float(relative_rmse),
                              int(max_iteration), _dp(out['transforms']), _dp(out['fitness']), _dp(out['inlier_rmse']), _dp(out['iterations']),
                              _dp(out['converged']), _dp(out['status']), None if corr is None else _dp(corr), ws.data_ptr(), nbytes, stream),
          'se3_icp_stack')
    if corr is not None:
        out['correspondences'] = corr
    return out


# the weighted entry: robust loss kernels and generalized ICP.  ICP_MODES stays the two modes of icp_stack; the third is this entry's own.
ICP_GENERALIZED = ENUMS['se3_icp_option']['SE3_ICP_GENERALIZED']
ICP_WEIGHTED_MODES = dict(ICP_MODES, generalized=ICP_GENERALIZED)
ICP_LOSSES = {name[len('SE3_ICP_LOSS_'):].lower(): value for name, value in ENUMS['se3_icp_option'].items()
              if name.startswith('SE3_ICP_LOSS_') and value >= 0}
_ICP_LOSS_NONE = ENUMS['se3_icp_option']['SE3_ICP_LOSS_NONE']


def icp_weighted_stack(grid, src_points, src_lengths, init_transforms, max_correspondence_distance, mode, ref_normals=None, src_normals=None,
                       loss=None, loss_k=None, gicp_epsilon=1e-3, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30,
                       return_correspondences=False):
    """HIP: icp_stack with a robust loss kernel and / or generalized ICP.  mode: a key of ICP_WEIGHTED_MODES; 'generalized' needs
    ref_normals and src_normals ((total source rows, 3) float32 / float64), unit normals of both clouds, and reads gicp_epsilon in (0, 1].
    loss: None (the instantiation without weight code: for the modes of icp_stack, its kernels and bits) or a key of ICP_LOSSES with its
    width loss_k, finite and positive ('l2' takes none).  Everything else, and the returned dict, as icp_stack."""
    s, elem = _pair_points(src_points, 'src_points')
    P = len(src_lengths)
    if s.device != grid.device or P != grid.num_pairs:
        raise RuntimeError('icp_weighted_stack: %d pairs on %s expected' % (grid.num_pairs, grid.device))
    if mode not in ICP_WEIGHTED_MODES:
        raise ValueError('icp_weighted_stack: estimation %r is not one of %s' % (mode, ', '.join(sorted(ICP_WEIGHTED_MODES))))
    loss_id, k = icp_loss_of(loss, loss_k, 'icp_weighted_stack')
    offsets = _pair_offsets(src_lengths, s.shape[0], 'icp_weighted_stack')
    T0 = _req(init_transforms, torch.float64, 'init_transforms', 3)
    if tuple(T0.shape) != (P, 4, 4) or T0.device != s.device:
        raise RuntimeError('icp_weighted_stack: init_transforms must be (%d, 4, 4) on %s' % (P, s.device))
    nr, nelem, sn, selem = None, 1, None, 1
    if ref_normals is not None:
        nr, nelem = _pair_points(ref_normals, 'ref_normals')
        if nr.shape[0] != grid.ns_total or nr.device != s.device:
            raise RuntimeError('icp_weighted_stack: ref_normals must be (%d, 3) on %s' % (grid.ns_total, s.device))
    elif mode != 'point_to_point':
        raise RuntimeError('icp_weighted_stack: %s needs the reference normals' % mode)
    if mode == 'generalized':
        if src_normals is None:
            raise RuntimeError('icp_weighted_stack: generalized needs the source normals')
        sn, selem = _pair_points(src_normals, 'src_normals')
        if sn.shape[0] != s.shape[0] or sn.device != s.device:
            raise RuntimeError('icp_weighted_stack: src_normals must be (%d, 3) on %s' % (s.shape[0], s.device))
    dev = s.device
    out = icp_outputs(P, dev)
    corr = torch.empty((s.shape[0],), dtype=torch.int64, device=dev) if return_correspondences else None
    nbytes = lib().se3_icp_weighted_workspace_bytes(s.shape[0], P)
    stream = _stream()
    ws = _ws_icp.get(dev, stream.value, nbytes)
    check(lib().se3_icp_weighted_stack(grid.ws.data_ptr(), grid.nbytes, grid.ns_total, _dp(s), elem, offsets, P, None if nr is None else _dp(nr),
                                       nelem, None if sn is None else _dp(sn), selem, _dp(T0), float(max_correspondence_distance),
                                       ICP_WEIGHTED_MODES[mode], loss_id, k, float(gicp_epsilon), float(relative_fitness), float(relative_rmse),
                                       int(max_iteration), _dp(out['transforms']), _dp(out['fitness']), _dp(out['inlier_rmse']),
                                       _dp(out['iterations']), _dp(out['converged']), _dp(out['status']), None if corr is None else _dp(corr),
                                       ws.data_ptr(), nbytes, stream),
          'se3_icp_weighted_stack')
    if corr is not None:
        out['correspondences'] = corr
    return out


def icp_loss_of(loss, loss_k, what):
    """(the library's loss id, its width) of a loss name or None and loss_k; a ValueError for an unknown name or a width that is not
    finite and positive.  None and 'l2' read no width: 1.0 stands in."""
    if loss is not None and loss not in ICP_LOSSES:
        raise ValueError('%s: loss %r is not one of %s' % (what, loss, ', '.join(sorted(ICP_LOSSES))))
    if loss_k is None and loss in (None, 'l2'):
        return (_ICP_LOSS_NONE if loss is None else ICP_LOSSES[loss]), 1.0
    try:
        k = float(loss_k)
    except (TypeError, ValueError):
        k = float('nan')
    if not (math.isfinite(k) and k > 0):
        raise ValueError('%s: loss_k %r is not a finite, positive number' % (what, loss_k))
    return (_ICP_LOSS_NONE if loss is None else ICP_LOSSES[loss]), k


# ---- coloured ICP: colour gradients and the coloured entry (csrc/color_gradient.hip, csrc/icp.hip) ----------------------------------------------
# the coloured mode has an enum and a constant of its own: ICP_MODES and ICP_WEIGHTED_MODES stay the tables of their entries
ICP_COLORED = ENUMS['se3_icp_colored_option']['SE3_ICP_COLORED']
COLOR_GRADIENT_STATUS = {1: 'a point, normal or colour is not finite'}


def color_gradient_stack(points, normals, colors, lengths, knn_idx, knn_d2, radius):
    """HIP: the colour gradient of every row of stacked clouds from the (rows, k) tables of knn_stack over the clouds searched in
    themselves.  points / normals / colors (total, 3) float32 / float64 on the device, cloud c on the next lengths[c] rows (host ints);
    radius finite and >= 0.  Returns (gradients (total, 3) float64, words (len(lengths) + 1,) int32 on the DEVICE: bit 1 of word c for a
    non-finite point, normal or colour of cloud c, the last word for any)."""
    p, elem = _pair_points(points, 'points')
    nr, nelem = _pair_points(normals, 'normals')
    col, celem = _pair_points(colors, 'colors')
    if nr.shape != p.shape or col.shape != p.shape or nr.device != p.device or col.device != p.device:
        raise RuntimeError('color_gradient_stack: normals and colors must have the shape and device of the points')
    idx, d2 = _req(knn_idx, torch.int64, 'knn_idx', 2), _req(knn_d2, torch.float64, 'knn_d2', 2)
    k = _knn_k(idx.shape[1], 'color_gradient_stack')
    if idx.shape != (p.shape[0], k) or d2.shape != idx.shape or idx.device != p.device or d2.device != p.device:
        raise RuntimeError('color_gradient_stack: knn_idx and knn_d2 must be (%d, k) tables of knn_stack on %s' % (p.shape[0], p.device))
    C = len(lengths)
    offsets = _pair_offsets(lengths, p.shape[0], 'color_gradient_stack')
    out = torch.empty((p.shape[0], 3), dtype=torch.float64, device=p.device)
    words = torch.empty((C + 1,), dtype=torch.int32, device=p.device)
    check(lib().se3_color_gradient_stack(_dp(p), elem, _dp(nr), nelem, _dp(col), celem, offsets, C, _dp(idx), _dp(d2), k, float(radius),
                                         _dp(out), words.data_ptr(), _stream()), 'se3_color_gradient_stack')
    return out, words


def icp_colored_stack(grid, src_points, src_lengths, init_transforms, max_correspondence_distance, ref_normals, src_colors, ref_colors,
                      ref_gradients, lambda_geometric=0.968, loss=None, loss_k=None, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30,
                      return_correspondences=False):
    """HIP: coloured ICP of up to PAIR_MAX_PAIRS stacked pairs: icp_stack's grid, source, transforms and results, with ref_normals
    (grid.ns_total, 3), src_colors (total source rows, 3), ref_colors (grid.ns_total, 3), all float32 / float64, ref_gradients
    (grid.ns_total, 3) float64 from color_gradient_stack over the reference clouds, lambda_geometric in [0, 1], and loss / loss_k as
    icp_weighted_stack (None: the instantiation without weight code)."""
    s, elem = _pair_points(src_points, 'src_points')
    P = len(src_lengths)
    if s.device != grid.device or P != grid.num_pairs:
        raise RuntimeError('icp_colored_stack: %d pairs on %s expected' % (grid.num_pairs, grid.device))
    lam = float(lambda_geometric)
    if not 0.0 <= lam <= 1.0:
        raise ValueError('icp_colored_stack: lambda_geometric %r is not in [0, 1]' % (lambda_geometric,))
    loss_id, k = icp_loss_of(loss, loss_k, 'icp_colored_stack')
    offsets = _pair_offsets(src_lengths, s.shape[0], 'icp_colored_stack')
    T0 = _req(init_transforms, torch.float64, 'init_transforms', 3)
    if tuple(T0.shape) != (P, 4, 4) or T0.device != s.device:
        raise RuntimeError('icp_colored_stack: init_transforms must be (%d, 4, 4) on %s' % (P, s.device))
    nr, nelem = _pair_points(ref_normals, 'ref_normals')
    sc, scelem = _pair_points(src_colors, 'src_colors')
    rc, rcelem = _pair_points(ref_colors, 'ref_colors')
    g = _req(ref_gradients, torch.float64, 'ref_gradients', 2)
    for t, rows, name in ((nr, grid.ns_total, 'ref_normals'), (sc, s.shape[0], 'src_colors'), (rc, grid.ns_total, 'ref_colors'),
                          (g, grid.ns_total, 'ref_gradients')):
        if tuple(t.shape) != (rows, 3) or t.device != s.device:
            raise RuntimeError('icp_colored_stack: %s must be (%d, 3) on %s' % (name, rows, s.device))
    dev = s.device
    out = icp_outputs(P, dev)
    corr = torch.empty((s.shape[0],), dtype=torch.int64, device=dev) if return_correspondences else None
    nbytes = lib().se3_icp_colored_workspace_bytes(s.shape[0], P)
    stream = _stream()
    ws = _ws_icp.get(dev, stream.value, nbytes)
    check(lib().se3_icp_colored_stack(grid.ws.data_ptr(), grid.nbytes, grid.ns_total, _dp(s), elem, offsets, P, _dp(nr), nelem, _dp(sc), scelem,
                                      _dp(rc), rcelem, _dp(g), _dp(T0), float(max_correspondence_distance), lam, loss_id, k,
                                      float(relative_fitness), float(relative_rmse), int(max_iteration), _dp(out['transforms']),
                                      _dp(out['fitness']), _dp(out['inlier_rmse']), _dp(out['iterations']), _dp(out['converged']),
                                      _dp(out['status']), None if corr is None else _dp(corr), ws.data_ptr(), nbytes, stream),
          'se3_icp_colored_stack')
    if corr is not None:
        out['correspondences'] = corr
    return out


# ---- Fast Global Registration of stacked pairs (csrc/fgr.hip) ------------------------------------------------------------------------------------
FGR_STATUS = {name[len('SE3_FGR_'):].lower(): value for name, value in ENUMS['se3_fgr_status'].items()}
FGR_MAX_ITERATION = ENUMS['se3_fgr_limit']['SE3_FGR_MAX_ITERATION']
FGR_MAX_CORRESPONDENCES = ENUMS['se3_fgr_limit']['SE3_FGR_MAX_CORRESPONDENCES']
FGR_MAX_TUPLE_COUNT = ENUMS['se3_fgr_limit']['SE3_FGR_MAX_TUPLE_COUNT']
FGR_TUPLE_CHUNK = ENUMS['se3_fgr_limit']['SE3_FGR_TUPLE_CHUNK']
FGR_MAX_ANGLE = ENUMS['se3_fgr_limit']['SE3_FGR_MAX_ANGLE']
_ws_fgr = Workspace(1 << 20)


def fgr_stack(src_points, src_lengths, ref_points, ref_lengths, correspondences, corr_lengths, maximum_correspondence_distance=0.025,
              division_factor=1.4, use_absolute_scale=False, decrease_mu=True, iteration_number=64, tuple_scale=0.95,
              maximum_tuple_count=1000, tuple_test=True, seed=0, return_tuples=False):
    """HIP: Fast Global Registration of up to PAIR_MAX_PAIRS stacked pairs in three launches, nothing read back (se3et_amd/fgr.py has the
    contract).  src_points / ref_points (total, 3) float32 / float64 on the device, pair p on the next src_lengths[p] / ref_lengths[p]
    rows; correspondences (K_total, 2) int64 on the device, pair-local (src row, ref row), pair p on the next corr_lengths[p] rows.
    Returns a dict of device tensors: transforms (P, 4, 4) float64 (ref ~ T src), status (P,) int32 (a sum of the FGR_STATUS bits),
    num_correspondences (|C'|), num_tuples (P,) int32, mu (P,) float64, and with return_tuples under the tuple test tuples
    (P, 3 maximum_tuple_count, 2) and trials (P, maximum_tuple_count) int64, of which pair p's first num_correspondences[p] /
    num_tuples[p] rows are written."""
    s, selem = _pair_points(src_points, 'src_points')
    q, qelem = _pair_points(ref_points, 'ref_points')
    c = _req(correspondences, torch.int64, 'correspondences', 2)
    P = len(src_lengths)
    if c.shape[1] != 2 or q.device != s.device or c.device != s.device or len(ref_lengths) != P or len(corr_lengths) != P:
        raise RuntimeError('fgr_stack: correspondences must be (K, 2), and the clouds and correspondences of %d pairs on %s' % (P, s.device))
    if any(int(k) > FGR_MAX_CORRESPONDENCES for k in corr_lengths):
        raise RuntimeError('fgr_stack: at most %d correspondences per pair' % FGR_MAX_CORRESPONDENCES)
    so, qo = _pair_offsets(src_lengths, s.shape[0], 'fgr_stack'), _pair_offsets(ref_lengths, q.shape[0], 'fgr_stack')
    co = _pair_offsets(corr_lengths, c.shape[0], 'fgr_stack')
    cap, tuple_test = int(maximum_tuple_count), bool(tuple_test)
    dev = s.device
    f64, i32, i64 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    out = {'transforms': torch.empty((P, 4, 4), **f64), 'status': torch.empty((P,), **i32), 'num_correspondences': torch.empty((P,), **i32),
           'num_tuples': torch.empty((P,), **i32), 'mu': torch.empty((P,), **f64)}
    tuples = trials = None
    if return_tuples and tuple_test and 0 <= cap <= FGR_MAX_TUPLE_COUNT:
        tuples, trials = torch.empty((P, 3 * cap, 2), **i64), torch.empty((P, cap), **i64)
    nbytes = lib().se3_fgr_workspace_bytes(P, cap, int(tuple_test))
    stream = _stream()
    ws = _ws_fgr.get(dev, stream.value, nbytes)
    check(lib().se3_fgr_stack(_dp(s), selem, so, _dp(q), qelem, qo, _dp(c), co, P, float(maximum_correspondence_distance), float(division_factor),
                              int(bool(use_absolute_scale)), int(bool(decrease_mu)), int(iteration_number), float(tuple_scale), cap,
                              int(tuple_test), int(seed) & ((1 << 64) - 1), _dp(out['transforms']), _dp(out['status']),
                              _dp(out['num_correspondences']), _dp(out['num_tuples']), _dp(out['mu']),
                              None if tuples is None else _dp(tuples), None if trials is None else _dp(trials), ws.data_ptr(), nbytes, stream),
          'se3_fgr_stack')
    if tuples is not None:
        out['tuples'], out['trials'] = tuples, trials
    return out


# ---- multiway registration: information matrices and pose graphs (csrc/pose_graph.hip) ---------------------------------------------------------------
PGO_STATUS = {name[len('SE3_PGO_'):].lower(): value for name, value in ENUMS['se3_pgo_status'].items()}
PGO_STOP = {name[len('SE3_PGO_STOP_'):].lower(): value for name, value in ENUMS['se3_pgo_stop'].items()}
PGO_MAX_NODES = ENUMS['se3_pgo_limit']['SE3_PGO_MAX_NODES']
PGO_MAX_EDGES = ENUMS['se3_pgo_limit']['SE3_PGO_MAX_EDGES']
PGO_MAX_ITERATION = ENUMS['se3_pgo_limit']['SE3_PGO_MAX_ITERATION']
PGO_MAX_ITERATION_LM = ENUMS['se3_pgo_limit']['SE3_PGO_MAX_ITERATION_LM']
_ws_pair_information, _ws_pose_graph = Workspace(1 << 20), Workspace(1 << 22)


def pair_information_stack(grid, src_points, src_lengths, transforms, max_correspondence_distance):
    """HIP: the information matrix of up to PAIR_MAX_PAIRS stacked pairs (se3et_amd/pose_graph.py has the contract).  grid:
    pair_grid_build over the REFERENCE clouds with identity transforms and cell_hint = max_correspondence_distance; src_points (total, 3)
    float32 / float64, pair p on the next src_lengths[p] rows; transforms (P, 4, 4) float64 on the DEVICE, ref ~ T src.  Returns a dict of
    device tensors: information (P, 6, 6) float64, count (P,) float64, status (P,) int32 (0, or the nonfinite / empty bit of PGO_STATUS)."""
    s, elem = _pair_points(src_points, 'src_points')
    P = len(src_lengths)
    if s.device != grid.device or P != grid.num_pairs:
        raise RuntimeError('pair_information_stack: %d pairs on %s expected' % (grid.num_pairs, grid.device))
    offsets = _pair_offsets(src_lengths, s.shape[0], 'pair_information_stack')
    T = _req(transforms, torch.float64, 'transforms', 3)
    if tuple(T.shape) != (P, 4, 4) or T.device != s.device:
        raise RuntimeError('pair_information_stack: transforms must be (%d, 4, 4) on %s' % (P, s.device))
    dev = s.device
    out = {'information': torch.empty((P, 6, 6), dtype=torch.float64, device=dev), 'count': torch.empty((P,), dtype=torch.float64, device=dev),
           'status': torch.empty((P,), dtype=torch.int32, device=dev)}
    nbytes = lib().se3_pair_information_workspace_bytes(s.shape[0], P)
    stream = _stream()
    ws = _ws_pair_information.get(dev, stream.value, nbytes)
    check(lib().se3_pair_information_stack(grid.ws.data_ptr(), grid.nbytes, grid.ns_total, _dp(s), elem, offsets, P, _dp(T),
                                           float(max_correspondence_distance), _dp(out['information']), _dp(out['count']), _dp(out['status']),
                                           ws.data_ptr(), nbytes, stream), 'se3_pair_information_stack')
    return out


def pose_graph_optimize_stack(poses, node_lengths, edges, transforms, informations, uncertain, edge_lengths, reference_nodes=None,
                              max_iteration=100, max_iteration_lm=20, min_relative_increment=1e-6, min_relative_residual_increment=1e-6,
                              min_right_term=1e-6, min_residual=1e-6, upper_scale_factor=2.0 / 3.0, lower_scale_factor=1.0 / 3.0,
                              max_correspondence_distance=0.075, edge_prune_threshold=0.25, preference_loop_closure=1.0):
    """HIP: the global optimisation of up to PAIR_MAX_PAIRS stacked pose graphs in ONE launch, one workgroup per graph, nothing read back
    (se3et_amd/pose_graph.py has the contract).  poses (nodes, 4, 4) float64, graph g on the next node_lengths[g] rows; edges (E, 2) int64
    graph-local (source node, target node), transforms (E, 4, 4) and informations (E, 6, 6) float64, uncertain (E,) uint8, graph g on the
    next edge_lengths[g] rows; all on the device.  reference_nodes: None, or one node per graph (-1 for none).  Returns a dict of device
    tensors: poses (nodes, 4, 4), confidence (2, E) (the line process after each pass), kept (E,) uint8, status (G,) int32 (a sum of the
    PGO_STATUS bits), info (G, 6) int32 (stop reason -- a value of PGO_STOP --, iterations, trials of pass 1, then of pass 2), residuals
    (G, 2) float64."""
    what = 'pose_graph_optimize_stack'
    X = _req(poses, torch.float64, 'poses', 3)
    e = _req(edges, torch.int64, 'edges', 2)
    T = _req(transforms, torch.float64, 'transforms', 3)
    L = _req(informations, torch.float64, 'informations', 3)
    u = _req(uncertain, torch.uint8, 'uncertain', 1)
    G, E, dev = len(node_lengths), e.shape[0], X.device
    if tuple(X.shape[1:]) != (4, 4) or tuple(e.shape) != (E, 2) or tuple(T.shape) != (E, 4, 4) or tuple(L.shape) != (E, 6, 6) or u.shape[0] != E \
            or len(edge_lengths) != G or any(t.device != dev for t in (e, T, L, u)):
        raise RuntimeError('%s: poses (nodes, 4, 4), edges (E, 2), transforms (E, 4, 4), informations (E, 6, 6) and uncertain (E,) of %d '
                           'graphs on %s expected' % (what, G, dev))
    if any(int(n) > PGO_MAX_NODES for n in node_lengths) or any(int(n) > PGO_MAX_EDGES for n in edge_lengths):
        raise RuntimeError('%s: at most %d nodes and %d edges per graph' % (what, PGO_MAX_NODES, PGO_MAX_EDGES))
    no, eo = _pair_offsets(node_lengths, X.shape[0], what), _pair_offsets(edge_lengths, E, what)
    ref = None
    if reference_nodes is not None:
        if len(reference_nodes) != G:
            raise RuntimeError('%s: one reference node per graph' % what)
        ref = (ctypes.c_int * max(G, 1))(*[int(r) for r in reference_nodes])
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    out = {'poses': torch.empty((X.shape[0], 4, 4), **f64), 'confidence': torch.empty((2, E), **f64),
           'kept': torch.empty((E,), dtype=torch.uint8, device=dev), 'status': torch.empty((G,), **i32), 'info': torch.empty((G, 6), **i32),
           'residuals': torch.empty((G, 2), **f64)}
    nbytes = lib().se3_pose_graph_workspace_bytes(no, eo, G)
    if nbytes == 0:
        raise RuntimeError('%s: the library refuses these graph sizes' % what)
    stream = _stream()
    ws = _ws_pose_graph.get(dev, stream.value, nbytes)
    check(lib().se3_pose_graph_optimize_stack(_dp(X), no, _dp(e), _dp(T), _dp(L), _dp(u), eo, G, ref, int(max_iteration), int(max_iteration_lm),
                                              float(min_relative_increment), float(min_relative_residual_increment), float(min_right_term),
                                              float(min_residual), float(upper_scale_factor), float(lower_scale_factor),
                                              float(max_correspondence_distance), float(edge_prune_threshold), float(preference_loop_closure),
                                              _dp(out['poses']), _dp(out['confidence']), _dp(out['kept']), _dp(out['status']), _dp(out['info']),
                                              _dp(out['residuals']), ws.data_ptr(), nbytes, stream), 'se3_pose_graph_optimize_stack')
    return out


# ---- keypoint selection: radius NMS in score order (csrc/keypoint_nms.hip) -----------------------------------------------------------------------
_ws_keypoint_nms = Workspace(1 << 20)


def keypoint_nms_stack(grid, order, lengths, radius, max_keep=0):
    """HIP: greedy radius NMS of up to PAIR_MAX_PAIRS stacked clouds, one workgroup per cloud.  grid: pair_grid_build over the clouds
    themselves with identity transforms and cell_hint = radius; order (total,) int64 on the device, cloud-local, rank -> index; max_keep:
    keypoints wanted per cloud, <= 0 for all survivors.  Returns (out (total,) int64: cloud c's kept indices in rank order from its row
    offset on, words (len(lengths) + 1,) int32 on the DEVICE: the counts and, last, the status word (0; bit 1: a non-finite point, bit 2:
    an order that is no permutation; the count of a refused cloud is minus its bits) -- one copy fetches both."""
    o = _req(order, torch.int64, 'order', 1)
    C = len(lengths)
    if o.device != grid.device or C != grid.num_pairs or o.shape[0] != grid.ns_total:
        raise RuntimeError('keypoint_nms_stack: an order of %d rows for %d clouds on %s expected' % (grid.ns_total, grid.num_pairs, grid.device))
    offsets = _pair_offsets(lengths, o.shape[0], 'keypoint_nms_stack')
    out = torch.empty((o.shape[0],), dtype=torch.int64, device=o.device)
    words = torch.empty((C + 1,), dtype=torch.int32, device=o.device)
    nbytes = lib().se3_keypoint_nms_workspace_bytes(o.shape[0], C)
    stream = _stream()
    ws = _ws_keypoint_nms.get(o.device, stream.value, nbytes)
    check(lib().se3_keypoint_nms_stack(grid.ws.data_ptr(), grid.nbytes, grid.ns_total, _dp(o), offsets, C, float(radius), int(max_keep), _dp(out),
                                       words.data_ptr(), words[C:].data_ptr(), ws.data_ptr(), nbytes, stream), 'se3_keypoint_nms_stack')
    return out, words


# ---- FPFH descriptors of stacked clouds (csrc/fpfh.hip) --------------------------------------------------------------------------------------------
FPFH_DIM = 33
FPFH_STATUS = {1: 'a point or normal is not finite'}


def _fpfh_cloud(points, normals, lengths, what):
    p, elem = _pair_points(points, 'points')
    nr, nelem = _pair_points(normals, 'normals')
    if nr.shape != p.shape or nr.device != p.device:
        raise RuntimeError('%s: normals must have the shape and device of the points' % what)
    return p, elem, nr, nelem, _pair_offsets(lengths, p.shape[0], what)


def fpfh_check_stack(points, normals, lengths):
    """HIP: the finite check of stacked clouds.  Returns words (len(lengths) + 1,) int32 on the DEVICE: bit 1 of word c for a non-finite
    point or normal of cloud c, the last word the OR of all (FPFH_STATUS)."""
    p, elem, nr, nelem, offsets = _fpfh_cloud(points, normals, lengths, 'fpfh_check_stack')
    words = torch.empty((len(lengths) + 1,), dtype=torch.int32, device=p.device)
    check(lib().se3_fpfh_check_stack(_dp(p), elem, _dp(nr), nelem, offsets, len(lengths), words.data_ptr(), _stream()), 'se3_fpfh_check_stack')
    return words


def _fpfh_list(row_offsets, pairs, row_begin, n_total, dev, what):
    ro = _req(row_offsets, torch.int64, 'row_offsets', 1)
    pr = _req(pairs, torch.int64, 'pairs', 2)
    rows = ro.shape[0] - 1
    if rows < 0 or row_begin < 0 or row_begin + rows > n_total or pr.shape[1] != 2 or ro.device != dev or pr.device != dev:
        raise RuntimeError('%s: row_offsets (rows + 1,) and pairs (total, 2) on %s for a slice of the %d rows expected' % (what, dev, n_total))
    return ro, pr, rows


def spfh_stack(points, normals, lengths, row_offsets, pairs, out, row_begin=0):
    """HIP: the SPFH rows [row_begin, row_begin + len(row_offsets) - 1) of stacked clouds into out (total rows, 33) float64, from the
    neighbour list (row_offsets from 0, pairs (total, 2) int64 with the neighbour's cloud-local index in column 1, as pair_ball_fill_stack
    leaves them).  A list entry outside its cloud is skipped."""
    p, elem, nr, nelem, offsets = _fpfh_cloud(points, normals, lengths, 'spfh_stack')
    ro, pr, rows = _fpfh_list(row_offsets, pairs, row_begin, p.shape[0], p.device, 'spfh_stack')
    if tuple(out.shape) != (p.shape[0], FPFH_DIM) or out.dtype != torch.float64 or not out.is_contiguous() or out.device != p.device:
        raise RuntimeError('spfh_stack: out must be (%d, %d) float64 on %s' % (p.shape[0], FPFH_DIM, p.device))
    check(lib().se3_spfh_stack(_dp(p), elem, _dp(nr), nelem, offsets, len(lengths), int(row_begin), rows, ro.data_ptr(), _dp(pr), pr.shape[0],
                               _dp(out), _stream()), 'se3_spfh_stack')
    return out


def fpfh_stack(points, spfh, lengths, row_offsets, pairs, out, row_begin=0):
    """HIP: the FPFH rows of the same slice into out (total rows, 33) float64 from spfh (total rows, 33), which holds every row of the
    clouds the slice touches."""
    p, elem = _pair_points(points, 'points')
    offsets = _pair_offsets(lengths, p.shape[0], 'fpfh_stack')
    ro, pr, rows = _fpfh_list(row_offsets, pairs, row_begin, p.shape[0], p.device, 'fpfh_stack')
    for t in (spfh, out):
        if tuple(t.shape) != (p.shape[0], FPFH_DIM) or t.dtype != torch.float64 or not t.is_contiguous() or t.device != p.device:
            raise RuntimeError('fpfh_stack: spfh and out must be (%d, %d) float64 on %s' % (p.shape[0], FPFH_DIM, p.device))
    check(lib().se3_fpfh_stack(_dp(p), elem, _dp(spfh), offsets, len(lengths), int(row_begin), rows, ro.data_ptr(), _dp(pr), pr.shape[0], _dp(out),
                               _stream()), 'se3_fpfh_stack')
    return out


# ---- ISS keypoints of stacked clouds (csrc/iss.hip) --------------------------------------------------------------------------------------------------
def points_check_stack(points, lengths):
    """HIP: the finite check of stacked clouds without normals (se3_fpfh_check_stack with the points in both places).  Returns words
    (len(lengths) + 1,) int32 on the DEVICE: bit 1 of word c for a non-finite point of cloud c, the last word the OR of all."""
    return fpfh_check_stack(points, points, lengths)


def iss_saliency_stack(points, lengths, row_offsets, pairs, gamma_21, gamma_32, min_neighbors, out, row_begin=0):
    """HIP: the ISS saliencies of rows [row_begin, row_begin + len(row_offsets) - 1) of stacked clouds into out (total rows,) float64, from
    the ball lists at the salient radius (row_offsets from 0, pairs (total, 2) int64 as pair_ball_fill_stack leaves them)."""
    p, elem = _pair_points(points, 'points')
    offsets = _pair_offsets(lengths, p.shape[0], 'iss_saliency_stack')
    ro, pr, rows = _fpfh_list(row_offsets, pairs, row_begin, p.shape[0], p.device, 'iss_saliency_stack')
    if tuple(out.shape) != (p.shape[0],) or out.dtype != torch.float64 or not out.is_contiguous() or out.device != p.device:
        raise RuntimeError('iss_saliency_stack: out must be (%d,) float64 on %s' % (p.shape[0], p.device))
    check(lib().se3_iss_saliency_stack(_dp(p), elem, offsets, len(lengths), int(row_begin), rows, ro.data_ptr(), _dp(pr), pr.shape[0],
                                       float(gamma_21), float(gamma_32), int(min_neighbors), _dp(out), _stream()), 'se3_iss_saliency_stack')
    return out


def iss_select_stack(grid, points, lengths, radii, saliency, min_neighbors):
    """HIP: the ISS selection.  grid: pair_grid_build over the clouds themselves with identity transforms and cell_hint = the largest
    radius; radii: each cloud's non_max_radius (a list), or one number for all.  Returns the mask (total rows,) uint8: 1 for a keypoint."""
    q, elem, offsets = _pair_query(grid, points, lengths, 'iss_select_stack')
    s = _req(saliency, torch.float64, 'saliency', 1)
    if s.shape[0] != q.shape[0] or s.device != q.device or grid.ns_total != q.shape[0]:
        raise RuntimeError('iss_select_stack: one saliency per row, on %s, and a grid over the same %d rows expected' % (q.device, q.shape[0]))
    mask = torch.empty((q.shape[0],), dtype=torch.uint8, device=q.device)
    check(lib().se3_iss_select_stack(grid.ws.data_ptr(), grid.nbytes, grid.ns_total, _dp(q), elem, offsets, grid.num_pairs,
                                     _pair_radii(list(radii) if isinstance(radii, (list, tuple)) else [radii] * grid.num_pairs, grid.num_pairs, 'iss_select_stack'), _dp(s),
                                     int(min_neighbors), _dp(mask), _stream()), 'se3_iss_select_stack')
    return mask


# ---- outlier removal and model resolution of stacked clouds (csrc/outliers.hip) -----------------------------------------------------------------
DISTANCE_STATS = 4          # per cloud: mean, std, thr, model resolution


def knn_distance_stack(grid, q_points, q_lengths, k, column=-1):
    """HIP: one float64 per row from its k nearest in its own cloud of `grid` (pair_grid_build with identity transforms and cell_hint 0):
    column < 0: the mean of the list's distances (the row itself at 0 among them); column >= 0: the distance of that column, 0 where the
    list is shorter."""
    q, elem, offsets = _pair_query(grid, q_points, q_lengths, 'knn_distance_stack')
    k = _knn_k(k, 'knn_distance_stack')
    if int(column) >= k:
        raise RuntimeError('knn_distance_stack: column %d not below k = %d' % (column, k))
    out = torch.empty((q.shape[0],), dtype=torch.float64, device=q.device)
    check(lib().se3_knn_distance_stack(grid.ws.data_ptr(), grid.nbytes, grid.ns_total, _dp(q), elem, offsets, grid.num_pairs, k, int(column),
                                       _dp(out), _stream()), 'se3_knn_distance_stack')
    return out


def distance_stats_stack(a, lengths, std_ratio=1.0):
    """HIP: (stats (clouds, 4) float64: mean, std, thr = mean + std_ratio std, model resolution; mask (total rows,) uint8: a > 0 and
    a < thr) of the stacked row values a, in the fixed summation shape of csrc/fixed_sum.h."""
    a = _req(a, torch.float64, 'a', 1)
    offsets = _pair_offsets(lengths, a.shape[0], 'distance_stats_stack')
    stats = torch.empty((len(lengths), DISTANCE_STATS), dtype=torch.float64, device=a.device)
    mask = torch.empty((a.shape[0],), dtype=torch.uint8, device=a.device)
    check(lib().se3_distance_stats_stack(_dp(a), offsets, len(lengths), float(std_ratio), _dp(stats), _dp(mask), _stream()),
          'se3_distance_stats_stack')
    return stats, mask


# ---- plane segmentation and DBSCAN clustering of stacked clouds (csrc/plane.hip, csrc/dbscan.hip) ------------------------------------------------
PLANE_STATUS = {name[len('SE3_PLANE_'):].lower(): value for name, value in ENUMS['se3_plane_status'].items()}
PLANE_MAX_SAMPLE = ENUMS['se3_plane_limit']['SE3_PLANE_MAX_SAMPLE']
PLANE_TILE = ENUMS['se3_plane_limit']['SE3_PLANE_TILE']
PLANE_SEGMENT = ENUMS['se3_plane_limit']['SE3_PLANE_SEGMENT']
PLANE_MAX_ITERATIONS = ENUMS['se3_plane_limit']['SE3_PLANE_MAX_ITERATIONS']
_ws_plane, _ws_dbscan = Workspace(1 << 22), Workspace(1 << 20)


def plane_segment_stack(points, lengths, distance_threshold, ransac_n=3, num_iterations=100, seed=0, per_hypothesis=False):
    """HIP (csrc/plane.hip): the dominant plane of each of the stacked clouds, three launches and nothing read back.  Returns a dict of
    device tensors: planes (P, 4) float64, mask (rows,) uint8, counts (P,) int32, fitness and inlier_rmse (P,) float64, status (P,) int32
    (PLANE_STATUS), best_hypothesis (P,) int32 (-1: none); with per_hypothesis also hyp_counts (P, H) int32 and hyp_errs (P, H) float64."""
    p, elem = _pair_points(points, 'points')
    P, H = len(lengths), int(num_iterations)
    offsets = _pair_offsets(lengths, p.shape[0], 'plane_segment_stack')
    dev = p.device
    out = dict(planes=torch.empty((P, 4), dtype=torch.float64, device=dev), mask=torch.empty((p.shape[0],), dtype=torch.uint8, device=dev),
               counts=torch.empty((P,), dtype=torch.int32, device=dev), fitness=torch.empty((P,), dtype=torch.float64, device=dev),
               inlier_rmse=torch.empty((P,), dtype=torch.float64, device=dev), status=torch.empty((P,), dtype=torch.int32, device=dev),
               best_hypothesis=torch.empty((P,), dtype=torch.int32, device=dev))
    if per_hypothesis:
        out['hyp_counts'] = torch.empty((P, max(H, 0)), dtype=torch.int32, device=dev)
        out['hyp_errs'] = torch.empty((P, max(H, 0)), dtype=torch.float64, device=dev)
    nbytes = lib().se3_plane_segment_workspace_bytes(offsets, P, H)
    stream = _stream()
    ws = _ws_plane.get(dev, stream.value, max(nbytes, 256))
    check(lib().se3_plane_segment_stack(_dp(p), elem, offsets, P, float(distance_threshold), int(ransac_n), H, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                        _dp(out['planes']), _dp(out['mask']), _dp(out['counts']), _dp(out['fitness']), _dp(out['inlier_rmse']),
                                        _dp(out['status']), _dp(out['best_hypothesis']), _dp(out['hyp_counts']) if per_hypothesis else None,
                                        _dp(out['hyp_errs']) if per_hypothesis else None, ws.data_ptr(), nbytes, stream), 'se3_plane_segment_stack')
    return out


def dbscan_stack(grid, points, lengths, eps, min_points):
    """HIP (csrc/dbscan.hip): DBSCAN labels of the stacked clouds.  grid: pair_grid_build over the clouds themselves with identity
    transforms and cell_hint = eps.  Returns (labels (rows,) int32: -1 noise, clusters 0 .. k - 1 per cloud; num_clusters (P,) int64), on
    the device."""
    q, elem, offsets = _pair_query(grid, points, lengths, 'dbscan_stack')
    labels = torch.empty((q.shape[0],), dtype=torch.int32, device=q.device)
    num = torch.empty((len(lengths),), dtype=torch.int64, device=q.device)
    nbytes = lib().se3_dbscan_workspace_bytes(q.shape[0])
    stream = _stream()
    ws = _ws_dbscan.get(q.device, stream.value, nbytes)
    check(lib().se3_dbscan_stack(grid.ws.data_ptr(), grid.nbytes, grid.ns_total, _dp(q), elem, offsets, grid.num_pairs, float(eps), int(min_points),
                                 _dp(labels), _dp(num), ws.data_ptr(), nbytes, stream), 'se3_dbscan_stack')
    return labels, num


# ---- TSDF fusion of depth frames and depth images as clouds (csrc/tsdf.hip) ------------------------------------------------------------------------
TSDF_LIMITS = {name[len('SE3_TSDF_'):].lower(): value for name, value in ENUMS['se3_tsdf_limit'].items()}
DEPTH_CONVENTIONS = {name[len('SE3_DEPTH_'):].lower(): value for name, value in ENUMS['se3_depth_convention'].items()}
_DEPTH_ELEM = {torch.uint16: 0, torch.float32: 1}
_COLOR_ELEM = {torch.uint8: 1, torch.float32: 2}


def _tsdf_images(depths, colors, what):
    """(depths, depth_elem, colors or None, color_elem) of (F, H, W) uint16 / float32 depths and (F, H, W, 3) uint8 / float32 colours."""
    if not torch.is_tensor(depths) or depths.dtype not in _DEPTH_ELEM:
        raise RuntimeError('%s: depths must be a uint16 or float32 tensor' % what)
    d = _req(depths, depths.dtype, 'depths', 3)
    if colors is None:
        return d, _DEPTH_ELEM[d.dtype], None, 0
    if not torch.is_tensor(colors) or colors.dtype not in _COLOR_ELEM:
        raise RuntimeError('%s: colors must be a uint8 or float32 tensor' % what)
    c = _req(colors, colors.dtype, 'colors', 4)
    if tuple(c.shape) != tuple(d.shape) + (3,) or c.device != d.device:
        raise RuntimeError('%s: colors must be %s on %s, got %s on %s' % (what, tuple(d.shape) + (3,), d.device, tuple(c.shape), c.device))
    return d, _DEPTH_ELEM[d.dtype], c, _COLOR_ELEM[c.dtype]


def _tsdf_state(tsdf, weight, color, what):
    t = _req(tsdf, torch.float32, 'tsdf', 4)
    V, R = t.shape[0], t.shape[1]
    w = _req(weight, torch.float32, 'weight', 4)
    if tuple(t.shape) != (V, R, R, R) or w.shape != t.shape or w.device != t.device or V > PAIR_MAX_PAIRS:
        raise RuntimeError('%s: tsdf and weight must both be (V, R, R, R) on one device, V at most %d' % (what, PAIR_MAX_PAIRS))
    if color is not None:
        color = _req(color, torch.float32, 'color', 5)
        if tuple(color.shape) != (V, 3, R, R, R) or color.device != t.device:
            raise RuntimeError('%s: color must be (V, 3, R, R, R) on %s' % (what, t.device))
    return t, w, color, V, R


def tsdf_integrate_stack(tsdf, weight, color, voxel_length, sdf_trunc, origins, depths, frames, frame_counts, colors=None, depth_scale=1000.0,
                         depth_trunc=3.0):
    """HIP (csrc/tsdf.hip): the frames' depth images integrated into the volumes, in place, one launch.  tsdf, weight (V, R, R, R) float32,
    color (V, 3, R, R, R) float32 or None, origins (V, 3) float64, depths (F, H, W) uint16 or float32, colors (F, H, W, 3) uint8 or float32
    (exactly when color is given), frames (F, TSDF_LIMITS['frame_words']) float32: the 3 x 4 extrinsic by rows, then fx, fy, cx, cy;
    frame_counts: the number of frames of each volume, in order."""
    what = 'tsdf_integrate_stack'
    t, w, color, V, R = _tsdf_state(tsdf, weight, color, what)
    d, depth_elem, c, color_elem = _tsdf_images(depths, colors, what)
    o = _req(origins, torch.float64, 'origins', 2)
    fr = _req(frames, torch.float32, 'frames', 2)
    F = d.shape[0]
    if tuple(o.shape) != (V, 3) or tuple(fr.shape) != (F, TSDF_LIMITS['frame_words']) or any(x.device != t.device for x in (o, fr, d)):
        raise RuntimeError('%s: origins (V, 3), frames (F, %d) and depths (F, H, W) on %s expected' % (what, TSDF_LIMITS['frame_words'], t.device))
    offsets = _pair_offsets(frame_counts, F, what)
    if len(frame_counts) != V:
        raise RuntimeError('%s: one frame count per volume' % what)
    check(lib().se3_tsdf_integrate_stack(_dp(t), _dp(w), None if color is None else _dp(color), V, R, float(voxel_length), float(sdf_trunc), _dp(o),
                                         _dp(d), depth_elem, None if c is None else _dp(c), color_elem, int(d.shape[1]), int(d.shape[2]), _dp(fr),
                                         offsets, float(depth_scale), float(depth_trunc), _stream()), 'se3_tsdf_integrate_stack')


def tsdf_extract_stack(tsdf, weight, color, voxel_length, origins):
    """HIP (csrc/tsdf.hip): the surface points of the volumes: a count pass, a scan, one host read of the volumes' counts, a write pass.
    Returns (points (n, 3) float64, normals (n, 3) float64, colors (n, 3) float64 or None, counts: a list of V ints); volume v owns the
    next counts[v] rows."""
    what = 'tsdf_extract_stack'
    t, w, color, V, R = _tsdf_state(tsdf, weight, color, what)
    o = _req(origins, torch.float64, 'origins', 2)
    if tuple(o.shape) != (V, 3) or o.device != t.device:
        raise RuntimeError('%s: origins (V, 3) on %s expected' % (what, t.device))
    dev = t.device
    rows = torch.empty((V * R * R + 1,), dtype=torch.int64, device=dev)
    stream = _stream()
    cptr = None if color is None else _dp(color)
    check(lib().se3_tsdf_extract_stack(_dp(t), _dp(w), cptr, V, R, float(voxel_length), _dp(o), _dp(rows), 0, None, None, None, stream),
          'se3_tsdf_extract_stack')
    cuts = rows[::R * R].cpu().tolist()          # (the one host read: the volumes' offsets)
    total = cuts[-1]
    out = [torch.empty((total, 3), dtype=torch.float64, device=dev) for _ in range(2 if color is None else 3)]
    if total:
        check(lib().se3_tsdf_extract_stack(_dp(t), _dp(w), cptr, V, R, float(voxel_length), _dp(o), _dp(rows), total, _dp(out[0]), _dp(out[1]),
                                           None if color is None else _dp(out[2]), stream), 'se3_tsdf_extract_stack')
    return out[0], out[1], None if color is None else out[2], [cuts[v + 1] - cuts[v] for v in range(V)]


def depth_points_stack(depths, intrinsics, scaling_factor=1000.0, distance_limit=6.0, convention='reference'):
    """HIP (csrc/tsdf.hip): the points of F depth images.  depths (F, H, W) uint16 or float32, intrinsics (F, 4) float64 (fx, fy, cx, cy).
    Returns (points (n, 3) float64 in image order, row-major pixel order within an image; counts: a list of F ints)."""
    what = 'depth_points_stack'
    d, elem, _, _ = _tsdf_images(depths, None, what)
    K = _req(intrinsics, torch.float64, 'intrinsics', 2)
    F, H, W = (int(s) for s in d.shape)
    if tuple(K.shape) != (F, 4) or K.device != d.device:
        raise RuntimeError('%s: intrinsics (F, 4) on %s expected' % (what, d.device))
    if convention not in DEPTH_CONVENTIONS:
        raise RuntimeError('%s: convention %r is not one of %s' % (what, convention, ', '.join(sorted(DEPTH_CONVENTIONS))))
    conv = DEPTH_CONVENTIONS[convention]
    rows = torch.empty((F * H + 1,), dtype=torch.int64, device=d.device)
    stream = _stream()
    check(lib().se3_depth_points_stack(_dp(d), elem, F, H, W, _dp(K), float(scaling_factor), float(distance_limit), conv, _dp(rows), 0, None, stream),
          'se3_depth_points_stack')
    cuts = rows[::H].cpu().tolist()
    total = cuts[-1]
    out = torch.empty((total, 3), dtype=torch.float64, device=d.device)
    if total:
        check(lib().se3_depth_points_stack(_dp(d), elem, F, H, W, _dp(K), float(scaling_factor), float(distance_limit), conv, _dp(rows), total,
                                           _dp(out), stream), 'se3_depth_points_stack')
    return out, [cuts[i + 1] - cuts[i] for i in range(F)]


# ---- block-sparse TSDF volumes (csrc/tsdf_sparse.hip) ------------------------------------------------------------------------------------------------
STSDF_LIMITS = {name[len('SE3_STSDF_'):].lower(): value for name, value in ENUMS['se3_stsdf_limit'].items()}
STSDF_BLOCK = STSDF_LIMITS['block']


def _stsdf_storage(tsdf, weight, color, what):
    t = _req(tsdf, torch.float32, 'tsdf', 4)
    w = _req(weight, torch.float32, 'weight', 4)
    B = STSDF_BLOCK
    if tuple(t.shape[1:]) != (B, B, B) or w.shape != t.shape or w.device != t.device:
        raise RuntimeError('%s: tsdf and weight must both be (S, %d, %d, %d) on one device' % (what, B, B, B))
    if color is not None:
        color = _req(color, torch.float32, 'color', 5)
        if tuple(color.shape) != (t.shape[0], 3, B, B, B) or color.device != t.device:
            raise RuntimeError('%s: color must be (S, 3, %d, %d, %d) on %s' % (what, B, B, B, t.device))
    return t, w, color


def _stsdf_directory(keys, slots, what, device):
    k, s = _req(keys, torch.int64, 'keys', 1), _req(slots, torch.int32, 'slots', 1)
    if k.shape != s.shape or k.device != device or s.device != device:
        raise RuntimeError('%s: keys (B,) int64 and slots (B,) int32 on %s expected' % (what, device))
    return k, s


def stsdf_touch_stack(depths, poses, frame_counts, voxel_length, sdf_trunc, stride=4, depth_scale=1000.0, depth_trunc=3.0):
    """HIP (csrc/tsdf_sparse.hip): the blocks that the frames touch (contract A).  depths (F, H, W) uint16 or float32, poses
    (F, STSDF_LIMITS['pose_words']) float64: the 3 x 4 camera pose by rows, then fx, fy, cx, cy; frame_counts: the frames of each volume.
    A count pass, one host read (the records and the first frame out of range), a write pass; then a stable sort by key and the removal
    of duplicates in torch.  Returns (keys (n,) int64, frames (n,) int32, bad_frame): the records ascending in (key, frame), each once;
    bad_frame is -1, or the first frame that touches a block coordinate out of range (the records are empty then)."""
    what = 'stsdf_touch_stack'
    d, depth_elem, _, _ = _tsdf_images(depths, None, what)
    P = _req(poses, torch.float64, 'poses', 2)
    F, H, W = (int(s) for s in d.shape)
    if tuple(P.shape) != (F, STSDF_LIMITS['pose_words']) or P.device != d.device:
        raise RuntimeError('%s: poses (F, %d) on %s expected' % (what, STSDF_LIMITS['pose_words'], d.device))
    offsets = _pair_offsets(frame_counts, F, what)
    dev = d.device
    groups = lib().se3_stsdf_touch_groups(F, H, W, int(stride))
    rows = torch.empty((groups + 1,), dtype=torch.int64, device=dev)
    bad = torch.zeros((F + 1,), dtype=torch.int32, device=dev)
    stream = _stream()
    args = (_dp(d), depth_elem, F, H, W, _dp(P), offsets, len(frame_counts), float(voxel_length), float(sdf_trunc), int(stride), float(depth_scale),
            float(depth_trunc), _dp(rows))
    check(lib().se3_stsdf_touch_stack(*args, _dp(bad), 0, None, None, stream), 'se3_stsdf_touch_stack')
    bad[F] = 1
    total, first_bad = torch.stack([rows[groups], torch.argmax(bad).to(torch.int64)]).cpu().tolist()          # (the one host read)
    keys = torch.empty((0 if first_bad < F else total,), dtype=torch.int64, device=dev)
    frames = torch.empty((keys.shape[0],), dtype=torch.int32, device=dev)
    if first_bad < F or total == 0:
        return keys, frames, (first_bad if first_bad < F else -1)
    check(lib().se3_stsdf_touch_stack(*args, None, total, _dp(keys), _dp(frames), stream), 'se3_stsdf_touch_stack')
    keys, order = torch.sort(keys, stable=True)          # (the records come in frame order: each key's frames stay ascending)
    frames = frames[order]
    first = torch.ones_like(keys, dtype=torch.bool)
    first[1:] = (keys[1:] != keys[:-1]) | (frames[1:] != frames[:-1])
    return keys[first].contiguous(), frames[first].contiguous(), -1


def stsdf_neighbors(keys, slots):
    """HIP (csrc/tsdf_sparse.hip): (B, 27) int32, the slots of the 27 blocks around each block of the sorted directory, -1 where absent."""
    k, s = _stsdf_directory(keys, slots, 'stsdf_neighbors', keys.device)
    out = torch.empty((k.shape[0], 27), dtype=torch.int32, device=k.device)
    check(lib().se3_stsdf_neighbors(_dp(k), _dp(s), int(k.shape[0]), _dp(out), _stream()), 'se3_stsdf_neighbors')
    return out


def stsdf_integrate_stack(tsdf, weight, color, keys, slots, frame_offsets, frame_ids, voxel_length, sdf_trunc, depths, frames, colors=None,
                          depth_scale=1000.0, depth_trunc=3.0):
    """HIP (csrc/tsdf_sparse.hip): the touched blocks integrate their frames, in place, one launch (contract B).  tsdf, weight
    (S, 16, 16, 16), color (S, 3, 16, 16, 16) or None: the storage; keys, slots (n,): the touched blocks; block i takes the frames
    frame_ids[frame_offsets[i]:frame_offsets[i + 1]] (int64 (n + 1,), int32); depths, frames, colors as tsdf_integrate_stack."""
    what = 'stsdf_integrate_stack'
    t, w, color = _stsdf_storage(tsdf, weight, color, what)
    k, s = _stsdf_directory(keys, slots, what, t.device)
    d, depth_elem, c, color_elem = _tsdf_images(depths, colors, what)
    fr = _req(frames, torch.float32, 'frames', 2)
    csr, ids = _req(frame_offsets, torch.int64, 'frame_offsets', 1), _req(frame_ids, torch.int32, 'frame_ids', 1)
    F, n = int(d.shape[0]), int(k.shape[0])
    if tuple(fr.shape) != (F, TSDF_LIMITS['frame_words']) or csr.shape[0] != n + 1 or any(x.device != t.device for x in (fr, d, csr, ids)):
        raise RuntimeError('%s: frames (F, %d), frame_offsets (n + 1,) and frame_ids on %s expected' % (what, TSDF_LIMITS['frame_words'], t.device))
    check(lib().se3_stsdf_integrate_stack(_dp(t), _dp(w), None if color is None else _dp(color), int(t.shape[0]), _dp(k), _dp(s), n, _dp(csr),
                                          _dp(ids), float(voxel_length), float(sdf_trunc), _dp(d), depth_elem, None if c is None else _dp(c),
                                          color_elem, F, int(d.shape[1]), int(d.shape[2]), _dp(fr), float(depth_scale), float(depth_trunc),
                                          _stream()), 'se3_stsdf_integrate_stack')


def stsdf_extract_stack(tsdf, weight, color, keys, neighbors, voxel_length, block_cuts):
    """HIP (csrc/tsdf_sparse.hip): the surface points of the blocks in key order (contract C): a count pass, a scan, one host read, a write
    pass.  neighbors: stsdf_neighbors of the directory; block_cuts (V + 1,) int64 on the device: volume v owns the blocks
    [block_cuts[v], block_cuts[v + 1]).  Returns (points, normals, colors or None, counts: a list of V ints)."""
    what = 'stsdf_extract_stack'
    t, w, color = _stsdf_storage(tsdf, weight, color, what)
    k, nb = _req(keys, torch.int64, 'keys', 1), _req(neighbors, torch.int32, 'neighbors', 2)
    n = int(k.shape[0])
    if tuple(nb.shape) != (n, 27) or k.device != t.device or nb.device != t.device:
        raise RuntimeError('%s: keys (B,) and neighbors (B, 27) on %s expected' % (what, t.device))
    dev = t.device
    rows = torch.empty((n * STSDF_BLOCK + 1,), dtype=torch.int64, device=dev)
    stream = _stream()
    cptr = None if color is None else _dp(color)
    check(lib().se3_stsdf_extract_stack(_dp(t), _dp(w), cptr, _dp(k), _dp(nb), n, float(voxel_length), _dp(rows), 0, None, None, None, stream),
          'se3_stsdf_extract_stack')
    cuts = rows[block_cuts * STSDF_BLOCK].cpu().tolist()          # (the one host read: the volumes' offsets)
    total = cuts[-1]
    out = [torch.empty((total, 3), dtype=torch.float64, device=dev) for _ in range(2 if color is None else 3)]
    if total:
        check(lib().se3_stsdf_extract_stack(_dp(t), _dp(w), cptr, _dp(k), _dp(nb), n, float(voxel_length), _dp(rows), total, _dp(out[0]),
                                            _dp(out[1]), None if color is None else _dp(out[2]), stream), 'se3_stsdf_extract_stack')
    return out[0], out[1], None if color is None else out[2], [cuts[v + 1] - cuts[v] for v in range(len(cuts) - 1)]


# ---- triangle meshes from the TSDF volumes (csrc/tsdf_mesh.hip) -------------------------------------------------------------------------------------
MESH_LIMITS = {name[len('SE3_MESH_'):].lower(): value for name, value in ENUMS['se3_mesh_limit'].items()}


def _mesh_outputs(vertices, triangles, has_color, dev):
    out = [torch.empty((vertices, 3), dtype=torch.float64, device=dev) for _ in range(3 if has_color else 2)]
    return out, torch.empty((triangles, 3), dtype=torch.int64, device=dev)


def tsdf_mesh_stack(tsdf, weight, color, voxel_length, origins):
    """HIP (csrc/tsdf_mesh.hip): the triangle meshes of the volumes: a count pass, two scans, one host read of the volumes' counts, a write
    pass; no workspace.  Returns (vertices (n, 3) float64, triangles (m, 3) int64, normals (n, 3) float64, colors (n, 3) float64 or None,
    vertex_counts, triangle_counts: lists of V ints); volume v owns the next vertex_counts[v] vertices and triangle_counts[v] triangles,
    and its triangles name its own vertices from 0."""
    what = 'tsdf_mesh_stack'
    t, w, color, V, R = _tsdf_state(tsdf, weight, color, what)
    o = _req(origins, torch.float64, 'origins', 2)
    if tuple(o.shape) != (V, 3) or o.device != t.device:
        raise RuntimeError('%s: origins (V, 3) on %s expected' % (what, t.device))
    dev = t.device
    rows = torch.empty((2, V * R * R + 1), dtype=torch.int64, device=dev)
    stream = _stream()
    cptr = None if color is None else _dp(color)
    args = (_dp(t), _dp(w), cptr, V, R, float(voxel_length), _dp(o), _dp(rows[0]), _dp(rows[1]))
    check(lib().se3_tsdf_mesh_stack(*args, 0, 0, None, None, None, None, stream), 'se3_tsdf_mesh_stack')
    vcuts, tcuts = rows[:, ::R * R].cpu().tolist()          # (the one host read: the volumes' offsets)
    out, tri = _mesh_outputs(vcuts[-1], tcuts[-1], color is not None, dev)
    if vcuts[-1]:
        check(lib().se3_tsdf_mesh_stack(*args, vcuts[-1], tcuts[-1], _dp(out[0]), _dp(out[1]), None if color is None else _dp(out[2]), _dp(tri),
                                        stream), 'se3_tsdf_mesh_stack')
    return (out[0], tri, out[1], None if color is None else out[2], [vcuts[v + 1] - vcuts[v] for v in range(V)],
            [tcuts[v + 1] - tcuts[v] for v in range(V)])


def stsdf_mesh_stack(tsdf, weight, color, keys, neighbors, voxel_length, block_cuts):
    """HIP (csrc/tsdf_mesh.hip): the triangle meshes of the blocks in key order, as tsdf_mesh_stack; the arguments of stsdf_extract_stack.
    The write pass takes an int32 plane of S x 4096 entries (the blocks' first vertex numbers: as many bytes as the tsdf storage), which
    lives for the call."""
    what = 'stsdf_mesh_stack'
    t, w, color = _stsdf_storage(tsdf, weight, color, what)
    k, nb = _req(keys, torch.int64, 'keys', 1), _req(neighbors, torch.int32, 'neighbors', 2)
    n = int(k.shape[0])
    if tuple(nb.shape) != (n, 27) or k.device != t.device or nb.device != t.device:
        raise RuntimeError('%s: keys (B,) and neighbors (B, 27) on %s expected' % (what, t.device))
    dev = t.device
    rows = torch.empty((2, n * STSDF_BLOCK + 1), dtype=torch.int64, device=dev)
    stream = _stream()
    cptr = None if color is None else _dp(color)
    args = (_dp(t), _dp(w), cptr, _dp(k), _dp(nb), n, float(voxel_length), _dp(rows[0]), _dp(rows[1]))
    check(lib().se3_stsdf_mesh_stack(*args, 0, 0, None, None, None, None, None, stream), 'se3_stsdf_mesh_stack')
    vcuts, tcuts = rows[:, block_cuts * STSDF_BLOCK].cpu().tolist()          # (the one host read: the volumes' offsets)
    out, tri = _mesh_outputs(vcuts[-1], tcuts[-1], color is not None, dev)
    if vcuts[-1]:
        plane = torch.empty((int(t.shape[0]) * STSDF_BLOCK ** 3,), dtype=torch.int32, device=dev)
        check(lib().se3_stsdf_mesh_stack(*args, vcuts[-1], tcuts[-1], _dp(plane), _dp(out[0]), _dp(out[1]), None if color is None else _dp(out[2]),
                                         _dp(tri), stream), 'se3_stsdf_mesh_stack')
    V = len(vcuts) - 1
    return (out[0], tri, out[1], None if color is None else out[2], [vcuts[v + 1] - vcuts[v] for v in range(V)],
            [tcuts[v + 1] - tcuts[v] for v in range(V)])


# ---- RGB-D odometry of frame pairs (csrc/rgbd_odometry.hip) -----------------------------------------------------------------------------------------
RGBD_LIMITS = {name[len('SE3_RGBD_'):].lower(): value for name, value in ENUMS['se3_rgbd_limit'].items()}
RGBD_STATUS = {name[len('SE3_RGBD_'):].lower(): value for name, value in ENUMS['se3_rgbd_status'].items()}
RGBD_METHODS = {name[len('SE3_RGBD_'):].lower(): value for name, value in ENUMS['se3_rgbd_method'].items()}
RGBD_STOPS = {name[len('SE3_RGBD_STOP_'):].lower(): value for name, value in ENUMS['se3_rgbd_stop'].items()}
_ws_rgbd = Workspace(1 << 20)


def rgbd_frames_workspace(depths, num_levels):
    """The tensor that holds the pyramids of the frames of depths (F, H, W) for rgbd_odometry_stack: one per call of the public function,
    shared by its chunks of pairs."""
    F, H, W = (int(s) for s in depths.shape)
    nbytes = lib().se3_rgbd_frames_workspace_bytes(F, H, W, int(num_levels))
    return torch.empty((max(nbytes, 256),), dtype=torch.uint8, device=depths.device)


def rgbd_odometry_stack(depths, colors, target_flags, frames_workspace, prepare, pairs, intrinsics, init_transforms, method, iterations,
                        depth_scale=1000.0, depth_trunc=3.0, min_depth=0.0, max_depth=4.0, max_depth_diff=0.03):
    """HIP (csrc/rgbd_odometry.hip): RGB-D odometry of up to PAIR_MAX_PAIRS pairs of the F frames, the whole schedule from one C call and
    nothing read back.  depths (F, H, W) uint16 or float32, colors (F, H, W, 3) or (F, H, W) uint8 or float32, target_flags (F,) uint8 on
    the device, frames_workspace: rgbd_frames_workspace(depths, len(iterations)); prepare: build the pyramids first (False: they are there
    from the call before).  pairs: P host tuples (source frame, target frame); intrinsics: P host rows (fx, fy, cx, cy);
    init_transforms (P, 4, 4) float64 on the device; method: a key of RGBD_METHODS; iterations: per level, coarsest first.  Returns a dict
    of device tensors: transforms (P, 4, 4) float64, success (P,) bool, status (P,) int32 (RGBD_STATUS bits), information (P, 6, 6)
    float64, correspondences (P,) int64."""
    what = 'rgbd_odometry_stack'
    d, depth_elem, c, color_elem = _rgbd_images(depths, colors, what)
    F, H, W = (int(s) for s in d.shape)
    dev = d.device
    flags = _req(target_flags, torch.uint8, 'target_flags', 1)
    T0 = _req(init_transforms, torch.float64, 'init_transforms', 3)
    P, L = len(pairs), len(iterations)
    if method not in RGBD_METHODS:
        raise RuntimeError('%s: method %r is not one of %s' % (what, method, ', '.join(sorted(RGBD_METHODS))))
    if P > PAIR_MAX_PAIRS or tuple(T0.shape) != (P, 4, 4) or len(intrinsics) != P or flags.shape[0] != F or any(x.device != dev for x in (flags, T0)):
        raise RuntimeError('%s: at most %d pairs per call, with init_transforms (P, 4, 4), P rows of intrinsics and target_flags (F,) on %s'
                           % (what, PAIR_MAX_PAIRS, dev))
    pair_table = (ctypes.c_int * max(2 * P, 1))(*[int(f) for pair in pairs for f in pair])
    K = (ctypes.c_double * max(4 * P, 1))(*[float(k) for row in intrinsics for k in row])
    its = (ctypes.c_int * max(L, 1))(*[int(n) for n in iterations])
    out = dict(transforms=torch.empty((P, 4, 4), dtype=torch.float64, device=dev), success=torch.empty((P,), dtype=torch.uint8, device=dev),
               status=torch.empty((P,), dtype=torch.int32, device=dev), information=torch.empty((P, 6, 6), dtype=torch.float64, device=dev),
               correspondences=torch.empty((P,), dtype=torch.int64, device=dev))
    nbytes = lib().se3_rgbd_pairs_workspace_bytes(P, H, W)
    stream = _stream()
    ws = _ws_rgbd.get(dev, stream.value, max(nbytes, 256))
    check(lib().se3_rgbd_odometry_stack(_dp(d), depth_elem, _dp(c), color_elem, 3 if c.dim() == 4 else 1, F, H, W, _dp(flags), 1 if prepare else 0,
                                        pair_table, K, P, _dp(T0), RGBD_METHODS[method], its, L, float(depth_scale), float(depth_trunc),
                                        float(min_depth), float(max_depth), float(max_depth_diff), _dp(out['transforms']), _dp(out['success']),
                                        _dp(out['status']), _dp(out['information']), _dp(out['correspondences']), frames_workspace.data_ptr(),
                                        frames_workspace.numel(), ws.data_ptr(), nbytes, stream), 'se3_rgbd_odometry_stack')
    out['success'] = out['success'].to(torch.bool)
    return out


def _rgbd_images(depths, colors, what):
    """(depths, depth_elem, colors, color_elem) of (F, H, W) uint16 / float32 depths and (F, H, W, 3) or (F, H, W) uint8 / float32 colours."""
    if not torch.is_tensor(depths) or depths.dtype not in _DEPTH_ELEM:
        raise RuntimeError('%s: depths must be a uint16 or float32 tensor' % what)
    d = _req(depths, depths.dtype, 'depths', 3)
    if not torch.is_tensor(colors) or colors.dtype not in _COLOR_ELEM or colors.dim() not in (3, 4):
        raise RuntimeError('%s: colors must be a uint8 or float32 tensor (F, H, W, 3) or (F, H, W)' % what)
    c = _req(colors, colors.dtype, 'colors', colors.dim())
    if tuple(c.shape) not in (tuple(d.shape), tuple(d.shape) + (3,)) or c.device != d.device:
        raise RuntimeError('%s: colors must be %s or %s on %s, got %s on %s' % (what, tuple(d.shape) + (3,), tuple(d.shape), d.device, tuple(c.shape),
                                                                              c.device))
    return d, _DEPTH_ELEM[d.dtype], c, _COLOR_ELEM[c.dtype]


# ---- ray casting of the TSDF volumes (csrc/tsdf_raycast.hip) -------------------------------------------------------------------------------------------
RAYCAST_LIMITS = {name[len('SE3_RAYCAST_'):].lower(): value for name, value in ENUMS['se3_raycast_limit'].items()}
RAYCAST_MAPS = {'depth': (torch.float32, ()), 'points': (torch.float64, (3,)), 'normals': (torch.float64, (3,)), 'color': (torch.float32, (3,)),
                'mask': (torch.bool, ())}


def raycast_outputs(maps, F, H, W, dev):
    """The maps of a call, uninitialised: the kernels write every pixel of every map."""
    return {name: torch.empty((F, H, W) + RAYCAST_MAPS[name][1], dtype=RAYCAST_MAPS[name][0], device=dev) for name in maps}


def _raycast_views(views, view_volumes, out, height, width, dev, what):
    v, vv = _req(views, torch.float64, 'views', 2), _req(view_volumes, torch.int32, 'view_volumes', 1)
    F, H, W = int(v.shape[0]), int(height), int(width)
    if tuple(v.shape) != (F, RAYCAST_LIMITS['view_words']) or vv.shape[0] != F or v.device != dev or vv.device != dev:
        raise RuntimeError('%s: views (F, %d) float64 and view_volumes (F,) int32 on %s expected' % (what, RAYCAST_LIMITS['view_words'], dev))
    ptrs = []
    for name, (dtype, tail) in RAYCAST_MAPS.items():
        t = out.get(name)
        if t is not None and (t.dtype != dtype or tuple(t.shape) != (F, H, W) + tail or t.device != dev or not t.is_contiguous()):
            raise RuntimeError('%s: map %r must be %s %s on %s, contiguous' % (what, name, (F, H, W) + tail, dtype, dev))
        ptrs.append(None if t is None else _dp(t))
    if set(out) - set(RAYCAST_MAPS):
        raise RuntimeError('%s: maps %s are not among %s' % (what, sorted(set(out) - set(RAYCAST_MAPS)), ', '.join(RAYCAST_MAPS)))
    return v, vv, F, H, W, ptrs


def tsdf_raycast_stack(tsdf, weight, color, voxel_length, sdf_trunc, origins, views, view_volumes, out, height, width, depth_min=0.1, depth_max=3.0,
                       weight_threshold=1.0):
    """HIP (csrc/tsdf_raycast.hip): the views ray-cast into the maps of `out`, in place, one launch, nothing read back.  The state of
    tsdf_extract_stack; views (F, RAYCAST_LIMITS['view_words']) float64: the 3 x 4 camera pose by rows, then fx, fy, cx, cy; view_volumes
    (F,) int32 on the device: the volume of each view; out: raycast_outputs of any of RAYCAST_MAPS ('color' only with color)."""
    what = 'tsdf_raycast_stack'
    t, w, color, V, R = _tsdf_state(tsdf, weight, color, what)
    o = _req(origins, torch.float64, 'origins', 2)
    if tuple(o.shape) != (V, 3) or o.device != t.device:
        raise RuntimeError('%s: origins (V, 3) on %s expected' % (what, t.device))
    v, vv, F, H, W, ptrs = _raycast_views(views, view_volumes, out, height, width, t.device, what)
    check(lib().se3_tsdf_raycast_stack(_dp(t), _dp(w), None if color is None else _dp(color), V, R, float(voxel_length), float(sdf_trunc), _dp(o),
                                       _dp(v), _dp(vv), F, H, W, float(depth_min), float(depth_max), float(weight_threshold), *ptrs, _stream()),
          'se3_tsdf_raycast_stack')
    return out


def stsdf_raycast_stack(tsdf, weight, color, keys, slots, num_volumes, voxel_length, sdf_trunc, views, view_volumes, out, height, width,
                        depth_min=0.1, depth_max=3.0, weight_threshold=1.0):
    """HIP (csrc/tsdf_raycast.hip): tsdf_raycast_stack for the block-sparse volumes: the storage with its directory (keys ascending, slots)."""
    what = 'stsdf_raycast_stack'
    t, w, color = _stsdf_storage(tsdf, weight, color, what)
    k, s = _stsdf_directory(keys, slots, what, t.device)
    v, vv, F, H, W, ptrs = _raycast_views(views, view_volumes, out, height, width, t.device, what)
    check(lib().se3_stsdf_raycast_stack(_dp(t), _dp(w), None if color is None else _dp(color), _dp(k), _dp(s), int(k.shape[0]), int(t.shape[0]),
                                        int(num_volumes), float(voxel_length), float(sdf_trunc), _dp(v), _dp(vv), F, H, W, float(depth_min),
                                        float(depth_max), float(weight_threshold), *ptrs, _stream()), 'se3_stsdf_raycast_stack')
    return out


# ---- mesh post-processing of stacked triangle meshes (csrc/mesh_ops.hip) ---------------------------------------------------------------------------
MESH_OPS_LIMITS = {name[len('SE3_MESH_OPS_'):].lower(): value for name, value in ENUMS['se3_mesh_ops_limit'].items()}
MESH_OPS_STATUS = {name[len('SE3_MESH_OPS_'):].lower(): value for name, value in ENUMS['se3_mesh_ops_status'].items()}
MESH_SMOOTH_METHODS = {name[len('SE3_MESH_SMOOTH_'):].lower(): value for name, value in ENUMS['se3_mesh_smooth_method'].items()}
_MESH_WORDS = MESH_OPS_LIMITS['count_words']


class StackedMeshes:
    """The meshes of one call end to end: vertices (N, 3) float64, triangles (M, 3) int64 naming vertices by their number within their own
    mesh, the host offsets of both.  At most PAIR_MAX_PAIRS meshes, each below 2^31 vertices and triangles."""

    def __init__(self, vertices, triangles, vertex_counts, triangle_counts, what='StackedMeshes'):
        self.vertices, self.triangles = _req(vertices, torch.float64, 'vertices', 2), _req(triangles, torch.int64, 'triangles', 2)
        if vertices.shape[1] != 3 or triangles.shape[1] != 3 or triangles.device != vertices.device:
            raise RuntimeError('%s: vertices (N, 3) and triangles (M, 3) on one device expected' % what)
        if len(vertex_counts) != len(triangle_counts):
            raise RuntimeError('%s: one vertex count and one triangle count per mesh' % what)
        if any(int(n) >= 1 << 31 for n in list(vertex_counts) + list(triangle_counts)):
            raise ValueError('%s: a mesh has 2^31 vertices or triangles or more' % what)
        self.vertex_counts, self.triangle_counts = [int(n) for n in vertex_counts], [int(m) for m in triangle_counts]
        self.voff, self.toff = _pair_offsets(vertex_counts, vertices.shape[0], what), _pair_offsets(triangle_counts, triangles.shape[0], what)
        self.B, self.N, self.M, self.device = len(self.vertex_counts), int(vertices.shape[0]), int(triangles.shape[0]), vertices.device

    def attribute(self, x, name):
        if x is None:
            return None
        x = _req(x, torch.float64, name, 2)
        if tuple(x.shape) != (self.N, 3) or x.device != self.device:
            raise RuntimeError('%s must be (%d, 3) on %s' % (name, self.N, self.device))
        return x

    def counts(self):
        return torch.empty((self.B, _MESH_WORDS), dtype=torch.int64, device=self.device)

    def read(self, counts, what):
        """the counts on the host (the one read of a pass); ValueError for a mesh whose status word is set"""
        rows = counts.cpu().tolist()
        bad = [b for b, row in enumerate(rows) if row[0] & MESH_OPS_STATUS['bad_triangle']]
        if bad:
            raise ValueError('%s: a triangle of mesh %s names a vertex outside [0, n) of its mesh' % (what, ', '.join(map(str, bad))))
        bad = [b for b, row in enumerate(rows) if row[0] & MESH_QUERY_STATUS['nonfinite_vertex']]          # (set by csrc/mesh_query.hip alone)
        if bad:
            raise ValueError('%s: a triangle of mesh %s has a vertex that is not finite' % (what, ', '.join(map(str, bad))))
        return rows


def _mesh_bytes(nbytes, dev):
    return torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=dev)


def _optr(t):
    return None if t is None else _dp(t)


class MeshIncidence:
    """The two CSR tables of mesh_incidence_stack: tri_offsets, nbr_offsets (N + 1) int64, tri_rows, nbr_rows int32 (mesh-local numbers)."""


def mesh_incidence_stack(meshes):
    """HIP (csrc/mesh_ops.hip): the vertex -> incident triangles and vertex -> neighbours tables of the stacked meshes: the count pass, one
    host read of the totals and the status, the write pass.  ValueError for a triangle out of range."""
    what, S, dev = 'mesh_incidence_stack', meshes, meshes.device
    inc = MeshIncidence()
    inc.tri_offsets = torch.empty((S.N + 1,), dtype=torch.int64, device=dev)
    inc.nbr_offsets = torch.empty((S.N + 1,), dtype=torch.int64, device=dev)
    inc.tri_rows = torch.empty((3 * S.M,), dtype=torch.int32, device=dev)
    counts = S.counts()
    nbytes = lib().se3_mesh_incidence_workspace_bytes(S.N)
    ws, stream = _mesh_bytes(nbytes, dev), _stream()
    args = (_dp(S.triangles), S.voff, S.toff, S.B, _dp(inc.tri_offsets), _dp(inc.tri_rows), _dp(inc.nbr_offsets))
    check(lib().se3_mesh_incidence_stack(*args, 0, None, _dp(counts), ws.data_ptr(), nbytes, stream), 'se3_mesh_incidence_stack')
    rows = S.read(counts, what)
    inc.incidences, inc.neighbors = sum(r[1] for r in rows), sum(r[2] for r in rows)
    inc.tri_rows = inc.tri_rows[:inc.incidences]
    inc.nbr_rows = torch.empty((inc.neighbors,), dtype=torch.int32, device=dev)
    if inc.neighbors:
        check(lib().se3_mesh_incidence_stack(*args, inc.neighbors, _dp(inc.nbr_rows), _dp(counts), ws.data_ptr(), nbytes, stream),
              'se3_mesh_incidence_stack')
    return inc


def mesh_components_stack(meshes, inc):
    """HIP (csrc/mesh_ops.hip): the connected components of the triangles under shared edges.  Returns (clusters (M,) int64, cluster
    n_triangles (M,) int64, cluster area (M,) float64, k: a list of B ints); cluster c of mesh b stands in slot triangle offset of b + c.
    The areas need each cluster's triangles in ascending order: one stable sort of the slots (torch.sort) between the two entries."""
    what, S, dev = 'mesh_components_stack', meshes, meshes.device
    clusters = torch.empty((S.M,), dtype=torch.int64, device=dev)
    n_triangles = torch.empty((S.M,), dtype=torch.int64, device=dev)
    area = torch.zeros((S.M,), dtype=torch.float64, device=dev)
    counts = S.counts()
    nbytes = lib().se3_mesh_components_workspace_bytes(S.M)
    ws, stream = _mesh_bytes(nbytes, dev), _stream()
    check(lib().se3_mesh_components_stack(_dp(S.triangles), S.voff, S.toff, S.B, _dp(inc.tri_offsets), _dp(inc.tri_rows), _dp(clusters), _dp(n_triangles),
                                          _dp(counts), ws.data_ptr(), nbytes, stream), 'se3_mesh_components_stack')
    if S.M:
        first = torch.repeat_interleave(to_device(list(S.toff)[:S.B], torch.int64, dev), to_device(S.triangle_counts, torch.int64, dev))
        order = torch.sort(clusters + first, stable=True).indices
        nbytes = lib().se3_mesh_cluster_area_workspace_bytes(S.M)
        ws = _mesh_bytes(nbytes, dev)
        check(lib().se3_mesh_cluster_area_stack(_dp(S.vertices), _dp(S.triangles), S.voff, S.toff, S.B, _dp(n_triangles), _dp(order), _dp(area),
                                                ws.data_ptr(), nbytes, stream), 'se3_mesh_cluster_area_stack')
    return clusters, n_triangles, area, [r[1] for r in S.read(counts, what)]


def mesh_select_stack(meshes, keep, normals=None, colors=None):
    """HIP (csrc/mesh_ops.hip): the triangles whose keep byte is set and the vertices they name, in their order, renumbered.  Returns
    (vertices, triangles, normals, colors, vertex_map (N,) int64 with -1 for a dropped vertex, vertex_counts, triangle_counts)."""
    what, S, dev = 'mesh_select_stack', meshes, meshes.device
    keep = _req(keep, torch.uint8, 'keep', 1)
    if keep.shape[0] != S.M or keep.device != dev:
        raise RuntimeError('%s: keep must be (%d,) uint8 on %s' % (what, S.M, dev))
    nrm, col = S.attribute(normals, 'normals'), S.attribute(colors, 'colors')
    vmap = torch.empty((S.N,), dtype=torch.int64, device=dev)
    counts = S.counts()
    nbytes = lib().se3_mesh_select_workspace_bytes(S.N, S.M)
    ws, stream = _mesh_bytes(nbytes, dev), _stream()
    head = (_dp(S.vertices), _optr(nrm), _optr(col), _dp(S.triangles), _dp(keep), S.voff, S.toff, S.B)
    check(lib().se3_mesh_select_stack(*head, None, None, None, None, None, None, _dp(vmap), _dp(counts), ws.data_ptr(), nbytes, stream),
          'se3_mesh_select_stack')
    rows = S.read(counts, what)
    vc, tc = [r[1] for r in rows], [r[2] for r in rows]
    out = [None if x is None else torch.empty((sum(vc), 3), dtype=torch.float64, device=dev) for x in (S.vertices, nrm, col)]
    tri = torch.empty((sum(tc), 3), dtype=torch.int64, device=dev)
    check(lib().se3_mesh_select_stack(*head, _i64_array(exclusive_offsets(vc)), _i64_array(exclusive_offsets(tc)), _dp(out[0]), _optr(out[1]),
                                      _optr(out[2]), _dp(tri), _dp(vmap), _dp(counts), ws.data_ptr(), nbytes, stream), 'se3_mesh_select_stack')
    return out[0], tri, out[1], out[2], vmap, vc, tc


def mesh_normals_stack(meshes, inc=None, normalized=True, triangle_normals=True, vertex_normals=True):
    """HIP (csrc/mesh_ops.hip): (triangle normals (M, 3), vertex normals (N, 3)) float64, either None when not asked for; the vertex normals
    gather the incidence rows `inc`.  Without `inc` (whose build checks the triangles) the status words are read here."""
    S, dev = meshes, meshes.device
    counts = S.counts() if inc is None and triangle_normals else None
    if vertex_normals and inc is None:
        raise RuntimeError('mesh_normals_stack: the vertex normals need the incidence tables')
    tn = torch.empty((S.M, 3), dtype=torch.float64, device=dev) if triangle_normals else None
    vn = torch.empty((S.N, 3), dtype=torch.float64, device=dev) if vertex_normals else None
    check(lib().se3_mesh_normals_stack(_dp(S.vertices), _dp(S.triangles), S.voff, S.toff, S.B, _dp(inc.tri_offsets) if vertex_normals else None,
                                       _dp(inc.tri_rows) if vertex_normals else None, int(bool(normalized)), _optr(tn), _optr(vn), _optr(counts), _stream()),
          'se3_mesh_normals_stack')
    if counts is not None:
        S.read(counts, 'mesh_normals_stack')
    return tn, vn


def mesh_smooth_stack(meshes, inc, method, iterations, lambda_filter=0.5, mu=-0.53, normals=None, colors=None):
    """HIP (csrc/mesh_ops.hip): `iterations` iterations of the filter over the neighbour rows of `inc`, every step issued by one call.
    Returns (vertices, normals, colors) as new tensors (None where none was given)."""
    what, S, dev = 'mesh_smooth_stack', meshes, meshes.device
    if method not in MESH_SMOOTH_METHODS:
        raise ValueError('%s: method %r is none of %s' % (what, method, ', '.join(MESH_SMOOTH_METHODS)))
    if int(iterations) < 0 or int(iterations) > MESH_OPS_LIMITS['max_iterations']:
        raise ValueError('%s: %d iterations (0 .. %d)' % (what, iterations, MESH_OPS_LIMITS['max_iterations']))
    src = [S.vertices, S.attribute(normals, 'normals'), S.attribute(colors, 'colors')]
    out = [None if x is None else torch.empty_like(x) for x in src]
    nbytes = lib().se3_mesh_smooth_workspace_bytes(S.N, sum(x is not None for x in src))
    ws = _mesh_bytes(nbytes, dev)
    check(lib().se3_mesh_smooth_stack(_dp(src[0]), _optr(src[1]), _optr(src[2]), S.voff, S.B, _dp(inc.nbr_offsets), _dp(inc.nbr_rows),
                                      MESH_SMOOTH_METHODS[method], int(iterations), float(lambda_filter), float(mu), _dp(out[0]), _optr(out[1]),
                                      _optr(out[2]), ws.data_ptr(), nbytes, _stream()), 'se3_mesh_smooth_stack')
    return tuple(out)


MESH_CLUSTER_PASSES = {name[len('SE3_MESH_CLUSTER_'):].lower(): value for name, value in ENUMS['se3_mesh_cluster_pass'].items()}


def _sorted_rows(columns, cuts):
    """the stacked rows sorted mesh by mesh by their columns (the first the most significant), equal rows in their order: stable sorts from
    the last column to the first"""
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        o = torch.arange(b - a, device=columns[0].device)
        for col in reversed(columns):
            o = o[torch.sort(col[a:b][o], stable=True).indices]
        parts.append(o + a)
    return torch.cat(parts) if parts else torch.zeros((0,), dtype=torch.int64, device=columns[0].device)


def mesh_cluster_vertices_stack(meshes, voxel_size, normals=None, colors=None):
    """HIP (csrc/mesh_ops.hip): simplify_vertex_clustering with the mean as contraction: the four passes of se3_mesh_cluster_vertices_stack with
    the two orders (vertices by cell, triangles by their rotated triple) sorted in between (torch.sort, stable) and one host read of the
    counts.  Returns (vertices, triangles, normals, colors, vertex_map (N,) int64, vertex_counts, triangle_counts).  ValueError for a voxel
    size that is not positive and finite, a mesh that is not finite or needs 2^21 cells or more on an axis, a triangle out of range."""
    what, S, dev = 'mesh_cluster_vertices_stack', meshes, meshes.device
    vs = float(voxel_size)
    if not (math.isfinite(vs) and vs > 0.0):
        raise ValueError('%s: voxel_size %r is not a positive finite number' % (what, voxel_size))
    nrm, col = S.attribute(normals, 'normals'), S.attribute(colors, 'colors')
    keys = torch.empty((S.N,), dtype=torch.int64, device=dev)
    vmap = torch.empty((S.N,), dtype=torch.int64, device=dev)
    rotated = torch.empty((S.M, 3), dtype=torch.int64, device=dev)
    counts = S.counts()
    nbytes = lib().se3_mesh_cluster_vertices_workspace_bytes(S.N, S.M)
    ws, stream = _mesh_bytes(nbytes, dev), _stream()

    def run(name, sorted_keys=None, vorder=None, torder=None, out=(None,) * 6):
        check(lib().se3_mesh_cluster_vertices_stack(MESH_CLUSTER_PASSES[name], _dp(S.vertices), _optr(nrm), _optr(col), _dp(S.triangles), S.voff, S.toff, S.B,
                                                    vs, _dp(keys), _optr(sorted_keys), _optr(vorder), _dp(vmap), _dp(rotated), _optr(torder), out[0], out[1],
                                                    _optr(out[2]), _optr(out[3]), _optr(out[4]), _optr(out[5]), _dp(counts), ws.data_ptr(), nbytes, stream),
              'se3_mesh_cluster_vertices_stack')
    run('keys')
    vorder = _sorted_rows([keys], list(S.voff)[:S.B + 1])
    run('vertices', keys[vorder], vorder)
    torder = _sorted_rows([rotated[:, 0], rotated[:, 1], rotated[:, 2]], list(S.toff)[:S.B + 1])
    run('triangles', None, None, torder)
    rows = counts.cpu().tolist()
    for bit, why in (('nonfinite', 'has a vertex or an attribute that is not finite'), ('too_many_cells', 'needs 2^21 cells or more on an axis: voxel_size is too small')):
        bad = [b for b, row in enumerate(rows) if row[0] & MESH_OPS_STATUS[bit]]
        if bad:
            raise ValueError('%s: mesh %s %s' % (what, ', '.join(map(str, bad)), why))
    rows = S.read(counts, what)
    vc, tc = [r[1] for r in rows], [r[2] for r in rows]
    out = [None if x is None else torch.empty((sum(vc), 3), dtype=torch.float64, device=dev) for x in (S.vertices, nrm, col)]
    tri = torch.empty((sum(tc), 3), dtype=torch.int64, device=dev)
    run('write', None, vorder, torder, (_i64_array(exclusive_offsets(vc)), _i64_array(exclusive_offsets(tc)), out[0], out[1], out[2], tri))
    return out[0], tri, out[1], out[2], vmap, vc, tc


# ---- ray casting and closest points on stacked triangle meshes (csrc/mesh_query.hip) -------------------------------------------------------------------
MESH_QUERY_LIMITS = {name[len('SE3_MESH_QUERY_'):].lower(): value for name, value in ENUMS['se3_mesh_query_limit'].items()}
MESH_QUERY_STATUS = {name[len('SE3_MESH_QUERY_'):].lower(): value for name, value in ENUMS['se3_mesh_query_status'].items()}
MESH_BVH_PASSES = {name[len('SE3_MESH_BVH_'):].lower(): value for name, value in ENUMS['se3_mesh_bvh_pass'].items()}
MESH_RENDER_MAPS = {'depth': (torch.float32, ()), 'points': (torch.float64, (3,)), 'normals': (torch.float64, (3,)), 'primitive_ids': (torch.int64, ()),
                    'mask': (torch.bool, ())}


class MeshBVH:
    """The trees of mesh_bvh_stack over the stacked `meshes`: nodes (2 max(M, 1), MESH_QUERY_LIMITS['node_bytes']) uint8, counts (B, 4) int64 on
    the device (status, live triangles, zero-area triangles, root), and the host's copy of the live and zero-area counts."""


def mesh_bvh_stack(meshes, strict=True):
    """HIP (csrc/mesh_query.hip): the bounding volume hierarchies of the stacked meshes: the key pass, one stable sort per mesh by
    (key < 0, key) (torch.sort), the tree pass, one host read of the counts.  ValueError for a triangle out of range or not finite
    (strict=False: no error, the status words stay in .status and the inert triangles are in no tree)."""
    what, S, dev = 'mesh_bvh_stack', meshes, meshes.device
    bvh = MeshBVH()
    bvh.meshes = S
    bvh.nodes = torch.empty((2 * max(S.M, 1), MESH_QUERY_LIMITS['node_bytes']), dtype=torch.uint8, device=dev)
    bvh.counts = S.counts()
    keys = torch.empty((S.M,), dtype=torch.int64, device=dev)
    nbytes = lib().se3_mesh_bvh_workspace_bytes(S.M)
    ws, stream = _mesh_bytes(nbytes, dev), _stream()
    head = (_dp(S.vertices), _dp(S.triangles), S.voff, S.toff, S.B)
    check(lib().se3_mesh_bvh_stack(MESH_BVH_PASSES['keys'], *head, _dp(keys), None, None, None, _dp(bvh.counts), ws.data_ptr(), nbytes, stream),
          'se3_mesh_bvh_stack')
    order = _sorted_rows([(keys < 0).to(torch.int64), keys], list(S.toff)[:S.B + 1])
    sorted_keys = keys[order]
    check(lib().se3_mesh_bvh_stack(MESH_BVH_PASSES['tree'], *head, None, _dp(sorted_keys), _dp(order), bvh.nodes.data_ptr(), _dp(bvh.counts),
                                   ws.data_ptr(), nbytes, stream), 'se3_mesh_bvh_stack')
    rows = S.read(bvh.counts, what) if strict else bvh.counts.cpu().tolist()
    bvh.status, bvh.live, bvh.zero_area = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    return bvh


def _query_rows(x, owners, cols, name, what, dev):
    x, o = _req(x, torch.float64, name, 2), _req(owners, torch.int32, name + ' meshes', 1)
    if x.shape[1] != cols or o.shape[0] != x.shape[0] or x.device != dev or o.device != dev:
        raise RuntimeError('%s: %s (R, %d) float64 and their meshes (R,) int32 on %s expected' % (what, name, cols, dev))
    return x, o, int(x.shape[0])


def _bvh_head(bvh):
    S = bvh.meshes
    return (_dp(S.vertices), _dp(S.triangles), S.voff, S.toff, S.B, bvh.nodes.data_ptr(), _dp(bvh.counts))


def mesh_cast_rays_stack(bvh, rays, ray_meshes, t_min=0.0, t_max=math.inf, any_hit=False):
    """HIP (csrc/mesh_query.hip): rays (R, 6) float64 origin and direction against the mesh ray_meshes (R,) int32 names (outside [0, B): a
    miss).  Returns {'t_hit' (R,) float64, inf on a miss; 'primitive_ids' (R,) int64, -1; 'primitive_uvs' (R, 2); 'primitive_normals'
    (R, 3)}, or with any_hit the hit flags (R,) bool alone: the walk of a ray ends at its first hit."""
    what, dev = 'mesh_cast_rays_stack', bvh.meshes.device
    r, o, R = _query_rows(rays, ray_meshes, 6, 'rays', what, dev)
    if math.isnan(float(t_min)) or math.isnan(float(t_max)):
        raise ValueError('%s: t_min %r, t_max %r' % (what, t_min, t_max))
    if any_hit:
        hit = torch.empty((R,), dtype=torch.uint8, device=dev)
        outs = (None, None, None, None, _dp(hit))
    else:
        out = {'t_hit': torch.empty((R,), dtype=torch.float64, device=dev), 'primitive_ids': torch.empty((R,), dtype=torch.int64, device=dev),
               'primitive_uvs': torch.empty((R, 2), dtype=torch.float64, device=dev),
               'primitive_normals': torch.empty((R, 3), dtype=torch.float64, device=dev)}
        outs = tuple(_dp(x) for x in out.values()) + (None,)
    check(lib().se3_mesh_cast_rays_stack(*_bvh_head(bvh), _dp(r), _dp(o), R, float(t_min), float(t_max), int(bool(any_hit)), *outs, _stream()),
          'se3_mesh_cast_rays_stack')
    return hit.to(torch.bool) if any_hit else out


def mesh_closest_points_stack(bvh, queries, query_meshes):
    """HIP (csrc/mesh_query.hip): the closest point of mesh query_meshes (Q,) int32 to every row of queries (Q, 3) float64.  Returns {'points'
    (Q, 3), 'distances' (Q,), 'primitive_ids' (Q,) int64, 'primitive_uvs' (Q, 2), 'primitive_normals' (Q, 3)}; a mesh without a live
    triangle answers inf and -1, a query point that is not finite NaN and -1."""
    what, dev = 'mesh_closest_points_stack', bvh.meshes.device
    q, o, Q = _query_rows(queries, query_meshes, 3, 'queries', what, dev)
    out = {'points': torch.empty((Q, 3), dtype=torch.float64, device=dev), 'distances': torch.empty((Q,), dtype=torch.float64, device=dev),
           'primitive_ids': torch.empty((Q,), dtype=torch.int64, device=dev), 'primitive_uvs': torch.empty((Q, 2), dtype=torch.float64, device=dev),
           'primitive_normals': torch.empty((Q, 3), dtype=torch.float64, device=dev)}
    check(lib().se3_mesh_closest_points_stack(*_bvh_head(bvh), _dp(q), _dp(o), Q, *(_dp(x) for x in out.values()), _stream()),
          'se3_mesh_closest_points_stack')
    return out


def mesh_render_outputs(maps, F, H, W, dev):
    """The maps of a rendering, uninitialised: the kernel writes every pixel of every map."""
    return {name: torch.empty((F, H, W) + MESH_RENDER_MAPS[name][1], dtype=MESH_RENDER_MAPS[name][0], device=dev) for name in maps}


def mesh_render_stack(bvh, views, view_meshes, out, height, width, depth_min=0.1, depth_max=3.0):
    """HIP (csrc/mesh_query.hip): the meshes seen from the views of tsdf_raycast_stack (F, RAYCAST_LIMITS['view_words']) float64, view_meshes
    (F,) int32 on the device, into the maps of `out` (mesh_render_outputs of any of MESH_RENDER_MAPS), in place."""
    what, dev = 'mesh_render_stack', bvh.meshes.device
    v, vm = _req(views, torch.float64, 'views', 2), _req(view_meshes, torch.int32, 'view_meshes', 1)
    F, H, W = int(v.shape[0]), int(height), int(width)
    if tuple(v.shape) != (F, RAYCAST_LIMITS['view_words']) or vm.shape[0] != F or v.device != dev or vm.device != dev:
        raise RuntimeError('%s: views (F, %d) float64 and view_meshes (F,) int32 on %s expected' % (what, RAYCAST_LIMITS['view_words'], dev))
    if set(out) - set(MESH_RENDER_MAPS):
        raise RuntimeError('%s: maps %s are not among %s' % (what, sorted(set(out) - set(MESH_RENDER_MAPS)), ', '.join(MESH_RENDER_MAPS)))
    ptrs = []
    for name, (dtype, tail) in MESH_RENDER_MAPS.items():
        t = out.get(name)
        if t is not None and (t.dtype != dtype or tuple(t.shape) != (F, H, W) + tail or t.device != dev or not t.is_contiguous()):
            raise RuntimeError('%s: map %r must be %s %s on %s, contiguous' % (what, name, (F, H, W) + tail, dtype, dev))
        ptrs.append(None if t is None else _dp(t))
    check(lib().se3_mesh_render_stack(*_bvh_head(bvh), _dp(v), _dp(vm), F, H, W, float(depth_min), float(depth_max), *ptrs, _stream()),
          'se3_mesh_render_stack')
    return out
