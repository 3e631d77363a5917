"""An independent float64 twin of the multiway-registration contract (csrc/pose_graph.hip, se3et_amd/pose_graph.py), written from the
contract and not from the library's text: numpy matrix products, np.arctan2, np.sin / np.cos, np.linalg for the solve (Cholesky, or LU
for the margin probe), scipy's cKDTree for the information matrix.  Besides the result it records, per trial, lambda, rho, whether the
trial was accepted and its residual, and the margins under which the library must follow the same path: the distance of every pass-1
confidence from the prune threshold, the smallest |rho|, and the relative distance of every stop test from its threshold at the trial
where it fires or first fails to fire."""
import numpy as np

NONFINITE, SINGULAR, EMPTY, STEP_REFUSED, BAD_INDEX = 1, 4, 8, 16, 32
STOP_NONE, STOP_RIGHT_TERM, STOP_RELATIVE_INCREMENT, STOP_RELATIVE_RESIDUAL, STOP_RESIDUAL, STOP_MAX_ITERATION, STOP_MAX_ITERATION_LM, \
    STOP_REFUSED = range(8)
DEFAULTS = dict(max_iteration=100, max_iteration_lm=20, min_relative_increment=1e-6, min_relative_residual_increment=1e-6,
                min_right_term=1e-6, min_residual=1e-6, upper_scale_factor=2.0 / 3.0, lower_scale_factor=1.0 / 3.0,
                max_correspondence_distance=0.075, edge_prune_threshold=0.25, preference_loop_closure=1.0, reference_node=-1)


# ---- part A ---------------------------------------------------------------------------------------------------------------------------------
def information_matrix(src, ref, T, r, descending=False, workers=1):
    """-> dict(information (6, 6), count, corr (n,) with -1 for none, threshold_margin, gap_margin) for non-empty finite clouds.
    descending: the rows are summed from the far end (the margin probe); workers: the threads of the tree query."""
    from scipy.spatial import cKDTree
    src, ref, T = np.asarray(src, np.float64), np.asarray(ref, np.float64), np.asarray(T, np.float64)
    p = src @ T[:3, :3].T + T[:3, 3]
    k = min(2, len(ref))
    d, j = cKDTree(ref).query(p, k=k, workers=workers)
    d, j = d.reshape(len(p), k), j.reshape(len(p), k)
    keep = d[:, 0] < r
    q = ref[j[keep, 0]][::-1] if descending else ref[j[keep, 0]]
    G = np.zeros((len(q), 3, 6))
    G[:, 0, 1], G[:, 0, 2], G[:, 1, 0], G[:, 1, 2], G[:, 2, 0], G[:, 2, 1] = q[:, 2], -q[:, 1], -q[:, 2], q[:, 0], q[:, 1], -q[:, 0]
    G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1.0
    return {'information': np.einsum('nra,nrb->ab', G, G), 'count': int(keep.sum()), 'corr': np.where(keep, j[:, 0], -1).astype(np.int64),
            'threshold_margin': float(np.abs(d[:, 0] - r).min()), 'gap_margin': float((d[:, 1] - d[:, 0]).min()) if k == 2 else np.inf}


# ---- part B ---------------------------------------------------------------------------------------------------------------------------------
def inverse(X):
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = X[:3, :3].T, -X[:3, :3].T @ X[:3, 3]
    return out


def vec6(M):
    sy = np.sqrt(M[0, 0] ** 2 + M[1, 0] ** 2)
    if not sy < 1e-6:
        a, b, c = np.arctan2(M[2, 1], M[2, 2]), np.arctan2(-M[2, 0], sy), np.arctan2(M[1, 0], M[0, 0])
    else:
        a, b, c = np.arctan2(-M[1, 2], M[1, 1]), np.arctan2(-M[2, 0], sy), 0.0
    return np.array([a, b, c, M[0, 3], M[1, 3], M[2, 3]])


def update_matrix(x):
    sx, cx, sy, cy, sz, cz = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = Rz @ Ry @ Rx, x[3:]
    return out


def _generators():
    D = np.zeros((6, 4, 4))
    D[0, 1, 2], D[0, 2, 1] = -1, 1
    D[1, 2, 0], D[1, 0, 2] = -1, 1
    D[2, 0, 1], D[2, 1, 0] = -1, 1
    D[3, 0, 3] = D[4, 1, 3] = D[5, 2, 3] = 1
    return D


_D = _generators()


def _lin6(M):
    return np.array([(M[2, 1] - M[1, 2]) / 2, (M[0, 2] - M[2, 0]) / 2, (M[1, 0] - M[0, 1]) / 2, M[0, 3], M[1, 3], M[2, 3]])


class _Pass:
    """One pass over the edges `ids` (ascending) of a graph; solver 'cholesky' / 'lu', descending: the edges are summed from the far end."""

    def __init__(self, graph, ids, opt, solver, descending):
        self.g, self.ids, self.o, self.solver = graph, list(ids), opt, solver
        self.order = self.ids[::-1] if descending else self.ids
        info = graph['informations']
        self.mu = opt['preference_loop_closure'] * opt['max_correspondence_distance'] ** 2 * \
            (sum(info[k][5, 5] for k in self.order) / len(self.ids)) if self.ids else 0.0

    def residuals(self, X):
        g = self.g
        return {k: vec6(inverse(g['transforms'][k]) @ inverse(X[g['edges'][k][1]]) @ X[g['edges'][k][0]]) for k in self.ids}

    def quad(self, e):
        return {k: float(e[k] @ self.g['informations'][k] @ e[k]) for k in self.ids}

    def line(self, q):
        return {k: (self.mu / (self.mu + q[k])) ** 2 if self.g['uncertain'][k] else 1.0 for k in self.ids}

    def total(self, l, q):
        return sum(l[k] * q[k] + (self.mu * (np.sqrt(l[k]) - 1.0) ** 2 if self.g['uncertain'][k] else 0.0) for k in self.order)

    def system(self, X, e, l):
        g, N = self.g, len(X)
        H, b = np.zeros((6 * N, 6 * N)), np.zeros(6 * N)
        for k in self.order:
            s, t = g['edges'][k]
            A = inverse(g['transforms'][k]) @ inverse(X[t])
            Js = np.stack([_lin6(A @ _D[i] @ X[s]) for i in range(6)], 1)
            J = {s: Js, t: -Js}
            L = g['informations'][k]
            for a in (s, t):
                b[6 * a:6 * a + 6] += l[k] * (J[a].T @ L @ e[k])
                for c in (s, t):
                    H[6 * a:6 * a + 6, 6 * c:6 * c + 6] += l[k] * (J[a].T @ L @ J[c])
        return H, b

    def solve(self, H, b, lam):
        A = H + lam * np.eye(len(b))
        if self.solver == 'lu':
            return np.linalg.solve(A, -b)
        C = np.linalg.cholesky(A)
        return np.linalg.solve(C.T, np.linalg.solve(C, -b))

    def run(self, X):
        o = self.o
        X = [x.copy() for x in X]
        rec = {'trials': [], 'margins': {'rho': np.inf, 'stop': np.inf}, 'status': 0}
        margins = rec['margins']

        def test(value, threshold):
            """value < threshold, with the relative distance between the two recorded for the tests that decide the path."""
            if threshold > 0:
                margins['stop'] = min(margins['stop'], abs(value - threshold) / threshold)
            return value < threshold

        e = self.residuals(X)
        q = self.quad(e)
        l = self.line(q)
        F = self.total(l, q)
        H, b = self.system(X, e, l)
        lam, nu = 1e-5 * (np.abs(np.diag(H)).max() if len(b) else 0.0), 2.0
        reason, stop = STOP_NONE, False

        def fire(why):
            nonlocal reason, stop
            if not stop:
                reason = why
            stop = True

        if (np.abs(b).max() if len(b) else 0.0) == 0.0:
            fire(STOP_RIGHT_TERM)                                       # (an exact zero: no margin to record)
        elif test(np.abs(b).max(), o['min_right_term']):
            fire(STOP_RIGHT_TERM)
        it = trials = 0
        while not stop:
            lm, rho = 0, 0.0
            while True:
                left, accepted, Fn, used = False, False, np.nan, lam
                rho = 0.0
                trials += 1
                d = self.solve(H, b, lam)
                x = np.concatenate([vec6(p) for p in X])
                if test(np.linalg.norm(d), o['min_relative_increment'] * (np.linalg.norm(x) + o['min_relative_increment'])):
                    fire(STOP_RELATIVE_INCREMENT)
                if not stop:
                    angles = d.reshape(-1, 6)[:, :3]
                    if not np.all(np.abs(angles) < 4.0):
                        rec['status'] |= STEP_REFUSED
                        fire(STOP_REFUSED)
                        left = True
                    else:
                        Xn = [update_matrix(d[6 * i:6 * i + 6]) @ X[i] for i in range(len(X))]
                        en = self.residuals(Xn)
                        qn = self.quad(en)
                        Fn = self.total(l, qn)
                        rho = (F - Fn) / (d @ (lam * d - b) + 1e-3)
                        margins['rho'] = min(margins['rho'], abs(rho))
                        if rho > 0:
                            if test(F - Fn, o['min_relative_residual_increment'] * F):
                                fire(STOP_RELATIVE_RESIDUAL)
                                left = True
                            else:
                                c = 2 * rho - 1
                                lam *= max(o['lower_scale_factor'], min(1 - c * c * c, o['upper_scale_factor']))
                                nu = 2.0
                                accepted = True
                                F, e, q, X = Fn, en, qn, Xn
                                l = self.line(q)
                                H, b = self.system(X, e, l)
                                if test(np.abs(b).max(), o['min_right_term']):
                                    fire(STOP_RIGHT_TERM)
                                    left = True
                        else:
                            lam *= nu
                            nu *= 2
                rec['trials'].append((used, rho, accepted, Fn))
                if left:
                    break
                lm += 1
                if lm >= o['max_iteration_lm']:
                    fire(STOP_MAX_ITERATION_LM)
                if rho > 0 or stop:
                    break
            if test(F, o['min_residual']):
                fire(STOP_RESIDUAL)
            if it + 1 >= o['max_iteration']:
                fire(STOP_MAX_ITERATION)
            it += 1
        rec.update(poses=X, line=l, residual=F, stop=reason, iterations=it, num_trials=trials)
        return rec


def global_optimization(graph, solver='cholesky', descending=False, **options):
    """graph: dict(poses (N, 4, 4), edges (E, 2), transforms (E, 4, 4), informations (E, 6, 6), uncertain (E,)); options: those of
    DEFAULTS.  -> dict(poses (N, 4, 4), confidence (2, E), kept (E,) bool, status, info (6,), residuals (2,), passes: the two records).
    The twin covers graphs that are not refused (the refusals have known answers)."""
    o = dict(DEFAULTS, **options)
    g = {'poses': np.asarray(graph['poses'], np.float64).reshape(-1, 4, 4), 'edges': np.asarray(graph['edges'], np.int64).reshape(-1, 2),
         'transforms': np.asarray(graph['transforms'], np.float64).reshape(-1, 4, 4),
         'informations': np.asarray(graph['informations'], np.float64).reshape(-1, 6, 6),
         'uncertain': np.asarray(graph['uncertain']).reshape(-1).astype(bool)}
    E = len(g['edges'])
    one = _Pass(g, range(E), o, solver, descending).run(list(g['poses']))
    conf = np.zeros((2, E))
    conf[0] = [one['line'][k] for k in range(E)]
    kept = ~g['uncertain'] | (conf[0] > o['edge_prune_threshold'])
    ids = [k for k in range(E) if kept[k]]
    two = _Pass(g, ids, o, solver, descending).run(one['poses'])
    for k in ids:
        conf[1, k] = two['line'][k]
    X = np.stack(two['poses']) if len(two['poses']) else np.zeros((0, 4, 4))
    ref = o['reference_node']
    if ref >= 0:
        C = g['poses'][ref] @ inverse(X[ref])
        X = np.stack([g['poses'][ref] if i == ref else C @ X[i] for i in range(len(X))])
    prune_margin = float(np.abs(conf[0][g['uncertain']] - o['edge_prune_threshold']).min()) if g['uncertain'].any() else np.inf
    return {'poses': X, 'confidence': conf, 'kept': kept, 'status': one['status'] | two['status'],
            'info': np.array([one['stop'], one['iterations'], one['num_trials'], two['stop'], two['iterations'], two['num_trials']]),
            'residuals': np.array([one['residual'], two['residual']]), 'passes': (one, two), 'prune_margin': prune_margin,
            'rho_margin': min(one['margins']['rho'], two['margins']['rho']), 'stop_margin': min(one['margins']['stop'], two['margins']['stop'])}
