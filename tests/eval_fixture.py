"""Checksums that tie tests/golden/eval_metrics.npz to the clouds it was made from (shared by tests/golden/generate_eval_golden.py and
tests/test_gpu_evaluation.py).  The fixture stores the reference's ground truth, predictions and metrics, not the clouds: the tests rebuild
the pyramid and the node partition on the device from se3et_amd.synthetic.make_pair and hold them to these checksums of the reference's
own collate and point_to_node_partition before they compare anything else."""
import numpy as np

P61 = np.uint64(2 ** 61 - 1)


def index_checksum(a):
    """Order-sensitive: sum of value * ((flat position mod 65521) + 1) mod 2^61 - 1 (the formula of tests/helpers.py)."""
    v = np.asarray(a).astype(np.uint64).reshape(-1)
    w = (np.arange(v.size, dtype=np.uint64) % np.uint64(65521)) + np.uint64(1)
    return int((v * w).sum() % P61)


def float_checksum(a):
    """index_checksum of the float32 bit patterns: equal only for bit-identical arrays in the same order."""
    return index_checksum(np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32))


def knn_set_checksum(knn, masks, num_points):
    """Checksum of every node's SET of patch points (local indices; masked entries as num_points): the overlaps depend on the sets,
    not on the order inside a row."""
    masks = np.asarray(masks).astype(bool)
    rows = np.where(masks, np.asarray(knn).astype(np.int64), num_points)
    return index_checksum(np.sort(rows, 1))


def pair_checksums(rec):
    """rec: numpy arrays ref/src_points_f, ref/src_points_c, src_points (stage 0), ref/src_knn (local indices), ref/src_knn_masks,
    ref/src_node_masks of one pair.  -> {name: int64}."""
    out = {}
    for k in ('ref_points_f', 'src_points_f', 'ref_points_c', 'src_points_c', 'src_points'):
        out['points/' + k] = float_checksum(rec[k])
    for side in ('ref', 'src'):
        out['knn_sets/' + side] = knn_set_checksum(rec[side + '_knn'], rec[side + '_knn_masks'], len(rec[side + '_points_f']))
        out['node_masks/' + side] = index_checksum(np.asarray(rec[side + '_node_masks']).astype(np.uint8))
    return {k: np.int64(v) for k, v in out.items()}
