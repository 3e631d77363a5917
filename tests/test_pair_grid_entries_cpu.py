"""CPU: what the seven entries that search a built pair grid refuse before they touch memory or launch anything (csrc/pair_grid.h's
pg_grid_call and each entry's own conditions), through the C ABI: the return code, and that se3_last_error() names the entry and the
offending quantity.  One table drives every entry; a small host buffer stands in for every pointer, so nothing here needs a GPU."""
import ctypes

import numpy as np
import pytest

N, CLOUDS, K = 4, 1, 3                       # rows and clouds of the valid call that every case below breaks in ONE place


def _base():
    from se3et_amd import _lib
    buf = np.zeros(4096, np.float64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    ws_bytes = _lib.lib().se3_pair_grid_workspace_bytes(N, CLOUDS)
    assert ws_bytes > 0
    return dict(buf=buf, grid=p, grid_bytes=ws_bytes, ns=N, q=p, elem=1, off=(ctypes.c_int64 * 34)(0, N), clouds=CLOUDS, out=p, k=K,
                radius=0.1, total=1, mode=0, max_iteration=2, ws_bytes=1 << 20)


# name -> (the call from the arguments above, the entry's word for a pair, has it an elem argument)
ENTRIES = {
    'pair_nearest_neighbor_stack': (lambda L, a: L.se3_pair_nearest_neighbor_stack(
        a['grid'], a['grid_bytes'], a['ns'], a['q'], a['elem'], a['off'], a['clouds'], a['out'], a['out'], None), b'pairs', True),
    'pair_ball_count_stack': (lambda L, a: L.se3_pair_ball_count_stack(
        a['grid'], a['grid_bytes'], a['ns'], a['q'], a['elem'], a['off'], a['clouds'], a['radius'], a['out'], None), b'pairs', True),
    'pair_ball_fill_stack': (lambda L, a: L.se3_pair_ball_fill_stack(
        a['grid'], a['grid_bytes'], a['ns'], a['q'], a['elem'], a['off'], a['clouds'], a['radius'], a['out'], a['total'], a['out'], None),
        b'pairs', True),
    'knn_stack': (lambda L, a: L.se3_knn_stack(
        a['grid'], a['grid_bytes'], a['ns'], a['q'], a['elem'], a['off'], a['clouds'], a['k'], a['out'], a['out'], None), b'clouds', True),
    'knn_normals_stack': (lambda L, a: L.se3_knn_normals_stack(
        a['grid'], a['grid_bytes'], a['ns'], a['q'], a['elem'], a['off'], a['clouds'], a['k'], None, a['out'], None), b'clouds', True),
    'icp_stack': (lambda L, a: L.se3_icp_stack(
        a['grid'], a['grid_bytes'], a['ns'], a['q'], a['elem'], a['off'], a['clouds'], None, 1, a['out'], a['radius'], a['mode'], 1e-6, 1e-6,
        a['max_iteration'], a['out'], a['out'], a['out'], a['out'], a['out'], a['out'], None, a['out'], a['ws_bytes'], None), b'pairs', True),
    # (the keypoints' query is `order`; the entry has no elem: its points are the grid's)
    'keypoint_nms_stack': (lambda L, a: L.se3_keypoint_nms_stack(
        a['grid'], a['grid_bytes'], a['ns'], a['q'], a['off'], a['clouds'], a['radius'], 0, a['out'], a['out'], a['out'], a['out'], a['ws_bytes'],
        None), b'clouds', False),
}

INVALID, UNSUPPORTED, WORKSPACE = 1, 2, 4      # SE3_ERR_INVALID_ARG, SE3_ERR_UNSUPPORTED, SE3_ERR_WORKSPACE

# case -> (what it changes, the code, the words the message must hold besides the entry's name; None: the entry's word for a pair)
SHARED = {
    '33 pairs': (dict(clouds=33), INVALID, [b'33 ', None, b'at most 32']),
    'offsets start at 1': (dict(off=(ctypes.c_int64 * 34)(1, N)), INVALID, [b'offsets must start at 0']),
    'offsets decrease': (dict(off=(ctypes.c_int64 * 34)(0, N, N - 1), clouds=2), INVALID, [b'offsets', b'not decrease']),
    'workspace one byte short': (dict(short=1), WORKSPACE, [b'grid workspace of ', b'bytes is too small']),
    'elem 2': (dict(elem=2), INVALID, [b'elem 2']),
    'null query': (dict(q=None), INVALID, [b'null pointer']),
}
OWN = {
    'knn_stack': {'k 0': (dict(k=0), INVALID, [b'k 0 not in [1, 64]']), 'k 65': (dict(k=65), INVALID, [b'k 65 not in [1, 64]'])},
    'knn_normals_stack': {'k 0': (dict(k=0), INVALID, [b'k 0 not in [1, 64]']), 'k 65': (dict(k=65), INVALID, [b'k 65 not in [1, 64]'])},
    'pair_ball_count_stack': {'negative radius': (dict(radius=-1.0), INVALID, [b'radius -1'])},
    'pair_ball_fill_stack': {'negative radius': (dict(radius=-1.0), INVALID, [b'radius -1'])},
    'keypoint_nms_stack': {'negative radius': (dict(radius=-1.0), INVALID, [b'radius -1', b'positive finite']),
                           'offsets end short of n_total': (dict(off=(ctypes.c_int64 * 34)(0, N - 1)), INVALID, [b'end at n_total = 4'])},
    'icp_stack': {'negative radius': (dict(radius=-1.0), INVALID, [b'distance -1']), 'mode 7': (dict(mode=7), INVALID, [b'mode 7'])},
    'pair_nearest_neighbor_stack': {},
}
CASES = [(entry, case) for entry in ENTRIES for case in list(SHARED) + list(OWN[entry]) if not (case == 'elem 2' and not ENTRIES[entry][2])]


def test_the_table_covers_the_seven_entries():
    assert len(ENTRIES) == 7 and set(OWN) == set(ENTRIES)
    assert len(CASES) == 7 * len(SHARED) - 1 + sum(len(v) for v in OWN.values())


def test_the_unbroken_call_passes_every_check_that_needs_no_gpu():
    """The base arguments are valid: with zero rows (nothing to launch) the entries that stop there return SE3_OK."""
    from se3et_amd import _lib
    L = _lib.lib()
    a = _base()
    a.update(off=(ctypes.c_int64 * 34)(0, 0))
    for entry in ('pair_nearest_neighbor_stack', 'knn_stack'):
        assert ENTRIES[entry][0](L, a) == 0, L.se3_last_error()


@pytest.mark.parametrize('entry,case', CASES, ids=['%s-%s' % (e, c.replace(' ', '_')) for e, c in CASES])
def test_refusal(entry, case):
    from se3et_amd import _lib
    L = _lib.lib()
    call, unit, _ = ENTRIES[entry]
    change, code, words = (SHARED[case] if case in SHARED else OWN[entry][case])
    a = _base()
    a.update(change)
    if a.pop('short', 0):
        a['grid_bytes'] -= 1
    status = call(L, a)
    message = L.se3_last_error()
    assert status == code, (status, message)
    assert message.startswith(entry.encode() + b': '), message
    for w in words:
        assert (unit if w is None else w) in message, message
