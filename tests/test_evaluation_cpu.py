"""CPU: the evaluation configuration (make_cfg's cfg.eval) and the provenance of tests/golden/eval_metrics.npz."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# experiments/se3ete.3dmatch/config.py:54-59 and experiments/se3eti.kitti/config.py:58-62
EVAL_3DMATCH = dict(acceptance_overlap=0.0, acceptance_radius=0.1, inlier_ratio_threshold=0.05, rmse_threshold=0.2, rre_threshold=15.0,
                    rte_threshold=0.3)
EVAL_KITTI = dict(acceptance_overlap=0.0, acceptance_radius=1.0, inlier_ratio_threshold=0.05, rre_threshold=5.0, rte_threshold=2.0)


def test_make_cfg_carries_the_reference_eval_section():
    from se3et_amd.model import VARIANTS, make_cfg
    for variant in VARIANTS:
        e = make_cfg(variant).eval
        want = EVAL_KITTI if variant.endswith('kitti') else EVAL_3DMATCH
        assert vars(e) == want, (variant, vars(e))


@pytest.mark.reference
def test_fixture_c2_pair0_reproduces_from_the_reference(golden_dir):
    """The generator's C2 pair-0 section re-run in process equals what eval_metrics.npz stores."""
    sys.path.insert(0, golden_dir)
    import generate_eval_golden as GE
    from se3et_amd.synthetic import make_pair
    stored = np.load(os.path.join(golden_dir, 'eval_metrics.npz'))
    res = {}
    ref, src, T = make_pair('c2_5k', 0)
    GE.gen_pair(res, '3dmatch', 'c2/p0/', ref, src, T, 100, 3.0, 0.05)
    assert res
    for k, v in res.items():
        assert k in stored.files, k
        w = stored[k]
        assert v.shape == w.shape and v.dtype == w.dtype, k
        assert np.array_equal(v, w, equal_nan=v.dtype.kind == 'f'), k
