"""The C oracle (oracle/c/grid_radius_oracle.c) against the reference's own binary at the geometric edges of grid subsampling and the
radius search: the seeded cases of precompute_edge_fixture.py, the reference's results in tests/golden/precompute_edges.npz
(generate_precompute_edges_golden.py: lengths, shapes and checksums).  The oracle is what tests/test_gpu_precompute_edges.py holds the
HIP kernels to, so this file closes the chain HIP kernel == C oracle == reference binary on these cases.  Every case is also held to the
property it exists for (check_grid_case / check_radius_case)."""
import numpy as np
import pytest
import torch

import precompute_edge_fixture as F
from helpers import index_checksum, tie_canonical


@pytest.fixture(scope='module')
def want(golden_dir):
    return np.load(golden_dir + '/precompute_edges.npz')


def _t(a):
    return torch.from_numpy(np.array(a))                                    # (a copy: the fixture's arrays are read-only)


def _bits(t):
    return index_checksum(np.ascontiguousarray(t.numpy()).view(np.uint32))


def oracle_radius(case, limit=None):
    from oracle import native
    return native.radius_search(_t(case['q']), _t(case['s']), torch.tensor(case['q_lengths'], dtype=torch.int64),
                                torch.tensor(case['s_lengths'], dtype=torch.int64), case['radius'], case['limit'] if limit is None else limit)


@pytest.mark.parametrize('name', list(F.grid_cases()))
def test_grid_case_holds_its_property(name):
    F.check_grid_case(name, F.grid_cases()[name])


@pytest.mark.parametrize('name', list(F.radius_cases()))
def test_radius_case_holds_its_property(name):
    F.check_radius_case(name, F.radius_cases()[name])


def test_fixture_and_cases_name_the_same_cases(want):
    assert {k.split('/')[1] for k in want.files if k.startswith('grid/')} == set(F.grid_cases())
    assert {k.split('/')[1] for k in want.files if k.startswith('radius/')} == set(F.radius_cases())


@pytest.mark.parametrize('name', list(F.grid_cases()))
def test_c_oracle_grid_subsample_equals_the_reference_binary(name, want):
    from oracle import native
    case = F.grid_cases()[name]
    p, n, l = _t(case['points']), _t(case['normals']), torch.tensor(case['lengths'], dtype=torch.int64)
    for k in range(F.CHAIN_STAGES):
        p, l, n = native.grid_subsample(p, l, n, case['voxel'] * 2 ** k)
        assert l.tolist() == want['grid/%s/lengths' % name][k].tolist(), 'stage %d counts' % k
        assert _bits(p) == int(want['grid/%s/points' % name][k]), 'stage %d points (selection or emission order)' % k
        assert _bits(n) == int(want['grid/%s/normals' % name][k]), 'stage %d normals' % k


@pytest.mark.parametrize('name', list(F.radius_cases()))
def test_c_oracle_radius_search_equals_the_reference_binary(name, want):
    case = F.radius_cases()[name]
    t = oracle_radius(case)
    assert list(t.shape) == want['radius/%s/shape' % name].tolist()
    with np.errstate(invalid='ignore'):                                     # (NaN / infinite query rows hold padding only)
        canon = tie_canonical(case['q'], case['s'], t)[0]
    assert index_checksum(canon) == int(want['radius/%s/tiecanon' % name]), 'differs beyond exactly tied entries'
    counts = (oracle_radius(case, 0) < len(case['s'])).sum(1).numpy()
    assert index_checksum(counts) == int(want['radius/%s/counts' % name])
    np.testing.assert_array_equal(counts, F.radius_counts(case)[0])


def test_c_oracle_gives_awkward_queries_padding_only():
    case = F.radius_cases()['awkward']
    t = oracle_radius(case)
    assert (t[case['awkward_rows']] == len(case['s'])).all()
    base, keep = F.without_awkward_rows(case)
    assert torch.equal(t[keep], oracle_radius(base))
