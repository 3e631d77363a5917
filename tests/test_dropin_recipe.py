"""The drop-in recipe of INTEGRATION.md section 1 without the reference tree: the documented text is the helper
call, the aliases resolve, and the EPN toolkit constants equal the reference's stored values.  The recipe in front of the reference's own
experiment directories is tests/dropin_probe.py, run by hand where the reference tree exists (it reads the recipe out of INTEGRATION.md, as
the test below does, so the documentation cannot drift)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def test_recipe_text_is_the_helper_call():
    """The documented block is the two-line call of se3et_amd.dropin (no hand-maintained module list in the text)."""
    sys.path.insert(0, HERE)
    import dropin_probe
    lines = [l for l in dropin_probe.recipe_text().strip().splitlines() if l.strip()]
    assert lines == ['import se3et_amd.dropin', 'se3et_amd.dropin.install_aliases()']


def test_aliases_without_a_reference_tree():
    """On a machine without the reference (the GPU box): the aliases install, the mirrored names import under the reference's module
    names, names that are not mirrored raise AttributeError / ImportError instead of resolving to anything else."""
    code = '''
import sys
import se3et_amd.dropin as d
sys.path = [p for p in sys.path if "reference" not in p]
names = d.install_aliases()
from geotransformer.modules.geotransformer import GeometricTransformer, SuperPointMatching, SuperPointTargetGenerator, LocalGlobalRegistration
from geotransformer.modules.registration import get_node_correspondences
from geotransformer.modules.ops import point_to_node_partition, index_select, apply_transform, pairwise_distance
from geotransformer.modules.ops.transformation import apply_transform as at2
from geotransformer.modules.ops.pairwise_distance import pairwise_distance as pd2
from geotransformer.modules.sinkhorn import LearnableLogOptimalTransport
from geotransformer.modules.kpconv import UnaryBlock, LastUnaryBlock, nearest_upsample
from geotransformer.modules.e2pn.blocks_epn import LiftBlockEPN, SimpleBlockEPN, ResnetBottleneckBlockEPN, UnaryBlockEPN, LastUnaryBlockEPN, InvOutBlockEPN
from geotransformer.modules.transformer.rotation_supervision import RotationAttentionLayer
from geotransformer.modules.transformer.permutation_invariant import PermutationInvariantLayer
import vgtk.functional as fr, vgtk.so3conv as sptk
import geotransformer.modules.ops as ops
try:
    ops.rodrigues_rotation_matrix
    raise SystemExit("unmirrored name resolved without a reference tree")
except AttributeError:
    pass
import torch
T = torch.eye(4); T[:3, 3] = torch.tensor([1., 2., 3.])
p = torch.arange(12.).reshape(4, 3)
assert torch.equal(apply_transform(p, T), p + T[:3, 3])
assert torch.allclose(ops.inverse_transform(T) @ T, torch.eye(4))
print("ok", len(names))
'''
    env = dict(os.environ, SE3_BLOCKING_SYNC='0', PYTHONPATH=os.path.dirname(HERE))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, timeout=600, cwd='/tmp')
    assert r.returncode == 0 and r.stdout.strip().startswith('ok'), r.stderr[-3000:]


def test_toolkit_constants_match_the_reference(golden_dir):
    """get_octahedron_vertices / get_relativeV_index / label_relative_rotation_simple of se3et_amd.vgtk (what the reference's loss.py:88-145
    takes from the EPN toolkit at construction time) against the genuine toolkit's values (tests/golden/vgtk_constants.npz, generate_golden.py
    toolkit: imported through oracle/ref_shims, whose trimesh is a stand-in: the edge centres are compared as a set)."""
    import numpy as np
    import torch
    import se3et_amd.vgtk as own
    a = np.load(os.path.join(golden_dir, 'vgtk_constants.npz'))
    b = own.get_octahedron_vertices()
    for i, name in ((0, 'vs'), (1, 'v_adjs'), (2, 'vRs'), (4, 'face_normals')):
        assert a[name].shape == np.asarray(b[i]).shape and np.allclose(a[name], b[i], atol=1e-6), name
    key = lambda e: sorted(map(tuple, np.round(np.asarray(e, np.float64), 5).tolist()))
    assert key(a['ecs']) == key(b[3]), 'ecs'
    tb = own.get_relativeV_index(b[2], b[0])
    assert np.array_equal(a['relative_index0'], tb[0]) and np.array_equal(a['relative_index1'], tb[1])
    g = np.random.default_rng(0)
    anchors = torch.tensor(a['vRs'], dtype=torch.float32)
    for j in range(20):
        q, _r = np.linalg.qr(g.normal(size=(3, 3)))
        q = torch.tensor(q * np.sign(np.linalg.det(q)), dtype=torch.float32)
        rb, lb = own.label_relative_rotation_simple(anchors, q)
        assert int(a['labels'][j]) == int(lb) and torch.allclose(torch.from_numpy(a['label_rotations'][j]), rb), j
