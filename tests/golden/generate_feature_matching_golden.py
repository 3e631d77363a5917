"""Fixture generator of the feature-space matching (runs ONLY where the reference tree exists; data only travels).

Imports the genuine reference through oracle/ref_shims.py and runs geotransformer.utils.registration.extract_corr_indices_from_feats (a
float64 cKDTree search in feature space) on planted descriptor sets: 400 ref and 350 src rows at C = 256 and at C = 32, 200 of the src rows
noisy copies of ref rows, the rest distractors (feature_matching_twin.planted_features).

Writes tests/golden/feature_matching.npz, per case c256 / c32:
  <case>/ref_feats, src_feats                    float32 inputs
  <case>/one_way_ref, one_way_src                extract_corr_indices_from_feats(ref, src)
  <case>/mutual_ref, mutual_src                  ... mutual=True
  <case>/bilateral_ref, bilateral_src            ... bilateral=True (the concatenated form)
and asserts that no row of either direction is a near-tie row (feature_matching_twin.near_ties), so the lists do not depend on a tie rule
or on float32 rounding of the ranking value.  Re-run with:  python tests/golden/generate_feature_matching_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_shims  # noqa: E402
import feature_matching_twin as twin  # noqa: E402

OUT = os.path.join(HERE, 'feature_matching.npz')
# (seeds whose inputs have no near-tie row: main() asserts it)
CASES = {'c256': (256, 20260115), 'c32': (32, 20260101)}
N_REF, N_SRC, MATCHES = 400, 350, 200


def main():
    ref_shims.install()
    from geotransformer.utils import registration as R
    store = {}
    for name, (C, seed) in CASES.items():
        ref, src = twin.planted_features(np.random.default_rng(seed), N_REF, N_SRC, C, MATCHES)
        for x, y, what in ((ref, src, 'ref -> src'), (src, ref, 'src -> ref')):
            near = twin.near_ties(x, y)[2]
            assert not near.any(), '%s %s: %d near-tie rows' % (name, what, int(near.sum()))
        p = name + '/'
        store[p + 'ref_feats'], store[p + 'src_feats'] = ref, src
        ref64, src64 = ref.astype(np.float64), src.astype(np.float64)
        for key, kwargs in (('one_way', {}), ('mutual', dict(mutual=True)), ('bilateral', dict(bilateral=True))):
            i, j = R.extract_corr_indices_from_feats(ref64, src64, **kwargs)
            store[p + key + '_ref'], store[p + key + '_src'] = np.asarray(i, np.int32), np.asarray(j, np.int32)
        print('%-5s one-way %d, mutual %d, bilateral %d' % (name, len(store[p + 'one_way_ref']), len(store[p + 'mutual_ref']),
                                                           len(store[p + 'bilateral_ref'])))
    np.savez_compressed(OUT, **store)
    size = os.path.getsize(OUT)
    assert size < (1 << 20), '%d bytes: above the size limit of a committed file' % size
    print('wrote', OUT, size, 'bytes')


if __name__ == '__main__':
    main()
