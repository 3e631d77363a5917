"""Seeded pose graphs of the multiway-registration tests, the twin's run over them, and the calls of the library's host entries.

A graph is a scene of N fragments with known poses X_i (node frame -> scene frame).  Edge (s, t) measures T = X_t^-1 X_s composed with
a 0.5 degree / 5 mm error; its information matrix is part A's formula (sum G^T G) on a few hundred random points of a unit cube; edges
(i, i + 1) are certain (odometry), the rest uncertain (loop closures), and a tenth of the uncertain edges are FALSE: 40 degrees / 0.8 m
added.  The start is the odometry chain X_0 = gt_0, X_(i+1) = X_i T_(i,i+1)^-1, or for the `identity` families all-identity poses on the
complete graph: those reject trials and end in a poor local minimum, so they are compared with the twin only, never with the truth.

case(name) returns the graph, the options and the twin's result, and asserts on the twin alone the margins under which the library must
follow the twin's path:
  - no pass-1 confidence within 1e-3 of the prune threshold,
  - no |rho| below 1e-6,
  - no stop test within 1 % of its threshold, at any trial.
A seed that misses a margin fails here, loudly.

MARGINS: how far the library may be from the twin, per quantity and case: 16 times the largest difference between two float64
evaluations OF THE TWIN that differ only in the solver (LU against Cholesky) and in the direction of the edge sums (ascending against
descending), with a floor of 1e-13; measured by tools/pose_graph_probe.py and copied from profiles/pose_graph_probe.txt."""
import ctypes
import functools

import numpy as np

import pose_graph_twin as twin
from icp_fixture import rigid

PRUNE_MARGIN, RHO_MARGIN, STOP_MARGIN = 1e-3, 1e-6, 1e-2
FLOOR = 1e-13

# name -> (nodes, seed, loop closures: 'all' or the number per node, start, largest pose angle in degrees, largest pose shift)
FAMILIES = {'chain3': (3, 11, 'all', 'odometry', 70.0, 2.0), 'ring6': (6, 12, 'all', 'odometry', 70.0, 2.0),
            'sparse12': (12, 13, 3, 'odometry', 70.0, 2.0), 'sparse42': (42, 14, 3, 'odometry', 70.0, 2.0),
            'sparse43': (43, 15, 3, 'odometry', 70.0, 2.0), 'complete64': (64, 16, 'all', 'odometry', 70.0, 2.0),
            'identity6': (6, 17, 'all', 'identity', 60.0, 2.0), 'identity12': (12, 21, 'all', 'identity', 60.0, 2.0)}

# profiles/pose_graph_probe.txt: 16 x the twin's own spread, floored at 1e-13 (poses, confidence, residuals)
MARGINS = {
    'chain3': {'poses': 2.10e-13, 'confidence': 1.00e-13, 'residuals': 1.00e-13},
    'complete64': {'poses': 4.46e-12, 'confidence': 2.01e-13, 'residuals': 1.55e-11},
    'identity12': {'poses': 4.69e-13, 'confidence': 1.00e-13, 'residuals': 1.31e-13},
    'identity6': {'poses': 4.06e-13, 'confidence': 1.00e-13, 'residuals': 1.00e-13},
    'ring6': {'poses': 2.33e-12, 'confidence': 1.00e-13, 'residuals': 1.00e-13},
    'sparse12': {'poses': 4.25e-12, 'confidence': 1.17e-13, 'residuals': 1.00e-13},
    'sparse42': {'poses': 1.96e-12, 'confidence': 1.00e-13, 'residuals': 1.71e-13},
    'sparse43': {'poses': 3.40e-12, 'confidence': 1.01e-13, 'residuals': 1.14e-13},
}
INFORMATION_MARGIN = 5.64e-11        # the information matrix: the twin's rows summed from either end, over the ICP fixture's cases


def margin(name, quantity):
    return MARGINS.get(name, {}).get(quantity, FLOOR)


def spread_margins(graph, **options):
    """The margin rule on a graph that has no recorded constant: 16 times the twin's spread over the solver and the direction of the edge
    sums, floored, per quantity.  -> (the twin's base result, {quantity: margin})."""
    base = twin.global_optimization(graph, **options)
    out = dict.fromkeys(('poses', 'confidence', 'residuals'), FLOOR)
    for solver, descending in (('lu', False), ('cholesky', True), ('lu', True)):
        other = twin.global_optimization(graph, solver, descending, **options)
        for q in out:
            out[q] = max(out[q], 16.0 * float(np.abs(other[q] - base[q]).max()) if base[q].size else 0.0)
    return base, out


def information_of(rng, n):
    """Part A's formula on n random points of the unit cube."""
    q = rng.random((n, 3))
    G = np.zeros((n, 3, 6))
    G[:, 0, 1], G[:, 0, 2], G[:, 1, 0], G[:, 1, 2], G[:, 2, 0], G[:, 2, 1] = q[:, 2], -q[:, 1], -q[:, 2], q[:, 0], q[:, 1], -q[:, 0]
    G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1.0
    return np.einsum('nra,nrb->ab', G, G)


def scene(N, seed, closures='all', start='odometry', degrees=70.0, shift=2.0):
    """-> (graph dict, ground-truth poses (N, 4, 4), false (E,) bool)."""
    rng = np.random.default_rng(seed)
    gt = np.stack([rigid(rng, rng.uniform(0.0, degrees), rng.uniform(0.0, shift)) for _ in range(N)]) if N else np.zeros((0, 4, 4))
    pairs = [(i, i + 1) for i in range(N - 1)]
    if closures == 'all':
        pairs += [(i, j) for i in range(N) for j in range(i + 2, N)]
    else:
        for i in range(N):
            for j in sorted(rng.choice(N, min(closures, N), replace=False)):
                if abs(i - j) > 1 and (min(i, j), max(i, j)) not in pairs:
                    pairs.append((min(i, j), max(i, j)))
    edges = np.array(pairs, np.int64).reshape(-1, 2)
    uncertain = np.array([t - s != 1 for s, t in pairs], bool)
    false = np.zeros(len(pairs), bool)
    loops = np.nonzero(uncertain)[0]
    false[rng.permutation(loops)[:max(len(loops) // 10, 1 if len(loops) >= 3 else 0)]] = True
    T = np.zeros((len(pairs), 4, 4))
    info = np.zeros((len(pairs), 6, 6))
    for k, (s, t) in enumerate(pairs):
        T[k] = rigid(rng, 0.5, 0.005) @ np.linalg.inv(gt[t]) @ gt[s]
        if false[k]:
            T[k] = rigid(rng, 40.0, 0.8) @ T[k]
        info[k] = information_of(rng, int(rng.integers(200, 400)))
    poses = np.tile(np.eye(4), (N, 1, 1))
    if start == 'odometry' and N:
        poses[0] = gt[0]
        for i in range(N - 1):
            poses[i + 1] = poses[i] @ np.linalg.inv(T[i])            # (the first N - 1 edges are the odometry edges, in order)
    return {'poses': poses, 'edges': edges, 'transforms': T, 'informations': info, 'uncertain': uncertain}, gt, false


def relative_error(poses, gt):
    """The largest |X_0^-1 X_i - gt_0^-1 gt_i| over the nodes: the error up to the free common frame."""
    rel = lambda X: np.stack([np.linalg.inv(X[0]) @ x for x in X])
    return float(np.abs(rel(np.asarray(poses)) - rel(gt)).max())


def check_margins(name, result):
    assert result['prune_margin'] >= PRUNE_MARGIN, '%s: a pass-1 confidence is %.1e from the prune threshold (another seed)' % (
        name, result['prune_margin'])
    assert result['rho_margin'] >= RHO_MARGIN, '%s: a trial has |rho| = %.1e (another seed)' % (name, result['rho_margin'])
    assert result['stop_margin'] >= STOP_MARGIN, '%s: a stop test is within %.1e of its threshold (another seed)' % (name, result['stop_margin'])


def rejected_trials(passes):
    """The trials (lambda, rho, accepted, residual) of the passes that formed a residual and were turned down: rho <= 0."""
    return sum(1 for p in passes for t in (p['trials'] if isinstance(p, dict) else p) if t[3] == t[3] and not t[1] > 0)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(graph, gt, false, options, twin), read-only."""
    N, seed, closures, start, degrees, shift = FAMILIES[name]
    graph, gt, false = scene(N, seed, closures, start, degrees, shift)
    options = {}
    result = twin.global_optimization(graph, **options)
    check_margins(name, result)
    if start == 'identity':
        assert rejected_trials(result['passes']) > 0, '%s: the twin rejects no trial' % name
    for a in list(graph.values()) + [gt, false]:
        a.setflags(write=False)
    return {'graph': graph, 'gt': gt, 'false': false, 'options': options, 'twin': result}


# ---- the host entries ------------------------------------------------------------------------------------------------------------------------
_dummy = (ctypes.c_double * 64)()


def _ptr(a):
    return None if a is None else a.ctypes.data if a.size else ctypes.addressof(_dummy)


def host_pgo(graph, trace_rows=4096, **options):
    """se3_debug_pose_graph_host on a graph dict.  -> dict(poses, confidence (2, E), kept (E,) bool, status, info (6,), residuals (2,),
    trials: per pass the list of (lambda, rho, accepted, residual))."""
    from se3et_amd._lib import check, lib
    o = dict(twin.DEFAULTS, **options)
    X = np.ascontiguousarray(graph['poses'], np.float64).reshape(-1, 4, 4)
    edges = np.ascontiguousarray(graph['edges'], np.int64).reshape(-1, 2)
    T = np.ascontiguousarray(graph['transforms'], np.float64).reshape(-1, 4, 4)
    info = np.ascontiguousarray(graph['informations'], np.float64).reshape(-1, 6, 6)
    unc = np.ascontiguousarray(np.asarray(graph['uncertain']).reshape(-1).astype(np.uint8))
    N, E = len(X), len(edges)
    assert len(T) == len(info) == len(unc) == E
    poses, conf, kept = np.full((N, 4, 4), -7.0), np.zeros((2, E)), np.zeros((E,), np.uint8)
    status, out_info, res = ctypes.c_int(-1), np.zeros((6,), np.int32), np.zeros((2,))
    trace, counts = np.full((trace_rows, 4), np.nan), np.zeros((2,), np.int32)
    check(lib().se3_debug_pose_graph_host(_ptr(X), N, _ptr(edges), _ptr(T), _ptr(info), _ptr(unc), E, int(o['reference_node']),
                                          int(o['max_iteration']), int(o['max_iteration_lm']), o['min_relative_increment'],
                                          o['min_relative_residual_increment'], o['min_right_term'], o['min_residual'],
                                          o['upper_scale_factor'], o['lower_scale_factor'], o['max_correspondence_distance'],
                                          o['edge_prune_threshold'], o['preference_loop_closure'], _ptr(poses), _ptr(conf), _ptr(kept),
                                          ctypes.byref(status), _ptr(out_info), _ptr(res), _ptr(trace), trace_rows, _ptr(counts)),
          'se3_debug_pose_graph_host')
    rows = [tuple(r) for r in trace[:counts.sum()]]
    return {'poses': poses, 'confidence': conf, 'kept': kept.astype(bool), 'status': status.value, 'info': out_info, 'residuals': res,
            'trials': (rows[:counts[0]], rows[counts[0]:])}


def host_information(src, ref, T, r):
    """se3_debug_pair_information_host on numpy arrays of one dtype.  -> dict(information (6, 6), count, status, corr (n,))."""
    from se3et_amd._lib import check, lib
    src, ref = np.ascontiguousarray(src).reshape(-1, 3), np.ascontiguousarray(ref).reshape(-1, 3)
    assert src.dtype == ref.dtype and src.dtype in (np.float32, np.float64)
    T = np.ascontiguousarray(T, np.float64).reshape(4, 4)
    out, count, status, corr = np.zeros((6, 6)), ctypes.c_double(), ctypes.c_int(-1), np.full((len(src),), -2, np.int64)
    check(lib().se3_debug_pair_information_host(_ptr(src), len(src), _ptr(ref), len(ref), int(src.dtype == np.float64), _ptr(T), float(r),
                                                _ptr(out), ctypes.byref(count), ctypes.byref(status), _ptr(corr)),
          'se3_debug_pair_information_host')
    return {'information': out, 'count': count.value, 'status': status.value, 'corr': corr}


def host_atan2(y, x):
    from se3et_amd._lib import check, lib
    y, x = np.ascontiguousarray(y, np.float64), np.ascontiguousarray(x, np.float64)
    out = np.zeros_like(y)
    check(lib().se3_debug_pgo_atan2_host(_ptr(y), _ptr(x), y.size, _ptr(out)), 'se3_debug_pgo_atan2_host')
    return out
