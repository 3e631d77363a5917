"""CPU: the C-ABI library loads and exports every symbol include/se3et_hip.h declares, and the binding reads its signatures and limits from
that header (no compute without a GPU)."""
import ctypes
import os
import re

import pytest


def _declared():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'se3et_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(se3_[a-z0-9_]+)\s*\(', text)))


def test_library_exports_every_declared_symbol():
    from se3et_amd import _lib
    L = _lib.lib()
    names = _declared()
    assert len(names) >= 10
    for n in names:
        assert hasattr(L, n), 'missing symbol %s' % n
        assert n in _lib.SIGNATURES, 'no ctypes signature for %s' % n
    assert set(_lib.SIGNATURES) == set(names)
    assert b'gfx950' in L.se3_version()


def test_signatures_are_the_headers_prototypes():
    """One prototype per branch of the binding's type map, written out from include/se3et_hip.h: a char* / uint64 / void / size_t return,
    float, double, uint64_t and size_t among pointers, a struct pointer, T* const*."""
    from se3et_amd._lib import SIGNATURES
    vp, i32, i64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    f32, f64, u64 = ctypes.c_float, ctypes.c_double, ctypes.c_uint64
    want = {
        'se3_version': (ctypes.c_char_p, []),
        'se3_debug_dense_saturated_rows': (u64, [i32]),
        'se3_debug_kernel_timing': (None, [i32]),
        'se3_radius_grid_workspace_bytes': (sz, [i64, i32]),
        'se3_radius_neighbors': (i32, [vp, i64, vp, i64, vp, vp, i32, f32, i32, vp, vp, vp]),
        'se3_ransac_correspondences_checked_stack': (i32, [vp, vp, vp, i32, f32, i32, i32, u64, vp, f64, i32, vp, sz,
                                                           vp, vp, vp, vp, vp, vp, vp, vp]),
        'se3_benchmark_summary': (i32, [vp, vp, vp, i32, i64, i32, f64, f64, f64, f64, vp, vp, vp]),
        'se3_transformer_forward': (i32, [vp, vp, vp, vp, sz, vp]),
        'se3_point_order_stages': (i32, [vp, vp, vp, vp, vp, vp, i32, vp]),
    }
    for name, (res, args) in want.items():
        assert SIGNATURES[name][0] is res, name
        assert SIGNATURES[name][1] == args, name


def test_header_reader_on_synthetic_text():
    from se3et_amd._lib import read_header
    sigs, consts = read_header('#define SE3_A 7 /* seven */\n#define SE3_S "text"\n#define OTHER 1\n// int se3_hidden(int);\n'
                               'const char *se3_a(void);\nvoid se3_b(unsigned long long, const float* const* p,\n  int32_t n);')
    assert consts == {'SE3_A': 7}
    assert sigs == {'se3_a': (ctypes.c_char_p, []), 'se3_b': (None, [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int])}


@pytest.mark.parametrize('text, offender', [('int se3_f(const float* x, short n);', 'short n'),            # an unknown scalar type
                                            ('long se3_f(int n);', 'long'),
                                            ('int se3_f(se3_linear_t w, int n);', 'se3_linear_t w'),        # a struct by value
                                            ('int se3_f(int n, float x[3]);', r'float x\[3\]'),             # an array
                                            ('int se3_f(void (*done)(int), int n);', r'void \(\*done\)\(int\)')])
def test_header_reader_refuses_what_it_cannot_map(text, offender):
    from se3et_amd._lib import read_header
    with pytest.raises(RuntimeError, match='se3_f.*%s' % offender):
        read_header(text)


def test_limits_are_the_headers_defines():
    from se3et_amd import _lib, cdriver, data, ops
    assert _lib.CONSTANTS == {'SE3_OK': 0, 'SE3_ERR_INVALID_ARG': 1, 'SE3_ERR_UNSUPPORTED': 2, 'SE3_ERR_LAUNCH': 3, 'SE3_ERR_WORKSPACE': 4,
                              'SE3_MAX_BATCH': 32, 'SE3_MAX_NEIGHBOR_LIMIT': 64, 'SE3_MAX_BLOCKS': 16, 'SE3_PAIR_MAX_PAIRS': 32,
                              'SE3_KNN_MAX': 64, 'SE3_GN_COUNTER_BYTES': 1024, 'SE3_KPCONV_SPLIT_COUNTER_BYTES': 65536,
                              # the enumerators of the header's enum block, with the values it spells (ops.ICP_MODES / ICP_STATUS / ICP_MAX_ITERATION)
                              'SE3_ICP_POINT_TO_POINT': 0, 'SE3_ICP_POINT_TO_PLANE': 1, 'SE3_ICP_NONFINITE': 1, 'SE3_ICP_TOO_FEW': 2,
                              'SE3_ICP_SINGULAR': 4, 'SE3_ICP_EMPTY': 8, 'SE3_ICP_STEP_REFUSED': 16, 'SE3_ICP_MAX_ITERATION': 1000}
    assert ops.ICP_MODES == {'point_to_point': 0, 'point_to_plane': 1} and ops.ICP_MAX_ITERATION == 1000
    assert ops.ICP_STATUS == {'nonfinite': 1, 'too_few': 2, 'singular': 4, 'empty': 8, 'step_refused': 16}
    got = {'SE3_MAX_BATCH': data.SE3_MAX_BATCH, 'SE3_MAX_NEIGHBOR_LIMIT': data.SE3_MAX_NEIGHBOR_LIMIT, 'SE3_MAX_BLOCKS': cdriver.MAX_BLOCKS,
           'SE3_PAIR_MAX_PAIRS': ops.PAIR_MAX_PAIRS, 'SE3_KNN_MAX': ops.KNN_MAX, 'SE3_GN_COUNTER_BYTES': ops.COUNTER_BYTES['_ws_dense'],
           'SE3_KPCONV_SPLIT_COUNTER_BYTES': ops.COUNTER_BYTES['_ws_kpconv_split']}
    assert ops.COUNTER_BYTES['_ws_kpconv_union_split'] == ops.COUNTER_BYTES['_ws_kpconv_split'] and len(ops.COUNTER_BYTES) == 3
    for name, value in got.items():
        assert type(value) is int and value == _lib.CONSTANTS[name], name
    assert type(cdriver.MAX_BATCH) is int and cdriver.MAX_BATCH == _lib.CONSTANTS['SE3_MAX_BATCH']


def test_missing_header_fails_loudly(monkeypatch, tmp_path):
    from se3et_amd import _lib
    monkeypatch.setattr(_lib, 'HEADER', str(tmp_path / 'se3et_hip.h'))
    with pytest.raises(RuntimeError, match='se3et_hip.h is missing'):
        _lib._read()


def test_plan_structs_match_the_library():
    """The ctypes mirror of se3_linear_t / se3_layer_t / se3_transformer_plan_t (se3et_amd/cdriver.py) has the library's sizes and offsets."""
    from se3et_amd import cdriver
    cdriver.check_layout()
    assert ctypes.sizeof(cdriver.Plan) > 16 * ctypes.sizeof(cdriver.Layer)


def test_argument_validation_without_gpu():
    from se3et_amd import _lib
    L = _lib.lib()
    # invalid arguments are rejected on the host before any launch
    assert L.se3_radius_neighbors(None, 0, None, 0, None, None, 0, 0.1, 10, None, None, None) != 0
    assert b'radius_neighbors' in L.se3_last_error()
    assert L.se3_grid_subsample_workspace_bytes(10000, 2) > 0
    assert L.se3_group_norm_workspace_bytes(1000, 64, 32) > 0
    assert L.se3_attention_fwd(None, None, None, None, 1, 1, 1, 32, 4, 32, 32, 32, 0, 0, 0, 0, 0, 1.0, None, None) != 0


def test_product_refuses_cpu_tensors():
    import torch
    from se3et_amd.modules.ops import radius_search
    with pytest.raises(RuntimeError):
        radius_search(torch.zeros(4, 3), torch.zeros(4, 3), torch.tensor([4]), torch.tensor([4]), 0.1, 8)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from se3et_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(RuntimeError, match='no CPU / eager fallback'):
        _lib.lib()


def test_cdriver_supported_mirrors_the_drivers_scheduler():
    """cdriver.supported() must refuse every block list se3_transformer_forward would refuse (csrc/transformer_driver.hip:
    SE3_REQUIREs on the X_is_eq / Xeq state), so that such models keep the Python schedule instead of raising."""
    from se3et_amd.cdriver import _schedule_ok
    e = ['self_eq', 'cross_a_soft', 'self_eq', 'cross_r_soft', 'self', 'cross', 'self', 'cross', 'self', 'cross']
    i = ['self_eq', 'cross', 'self_eq', 'cross', 'self_eq', 'cross']
    assert _schedule_ok(e, True) and _schedule_ok(i, True)
    assert not _schedule_ok(e, False)                                   # eq2inv without the rotcompress layer
    assert not _schedule_ok(['self_eq', 'cross_a_soft'], True)          # ends on anchor features
    assert not _schedule_ok(['self_eq', 'cross_r_soft'], True)
    assert not _schedule_ok(['self_eq', 'self', 'cross'], True)         # plain cross attention on anchor features
    assert not _schedule_ok(['self_eq', 'cross', 'cross_a_soft'], True)  # equivariant cross attention on invariant features
    assert _schedule_ok(['self_eq', 'cross_r_soft', 'self', 'cross'], True)
