"""Fixture generator of the neighbour-limit calibration (runs ONLY where the reference tree and oracle/_ref exist; data only travels).

Imports the genuine reference through oracle/ref_shims.py and runs ITS calibrate_neighbors_stack_mode with ITS
registration_collate_fn_stack_mode over the in-memory datasets of tests/calibration_fixture.py.  Writes tests/golden/calibration.npz:

  <case>/limits       the reference's return value
  <case>/pairs_used   the number of items it collated before it stopped
  <case>/hist         (pairs_used, stages, hist_n) int32: per item the histogram its loop added, recomputed here from the collate's output
                      with the reference's two lines (utils/data.py:232,235)
  <case>/dropped      (pairs_used, stages): rows with hist_n or more neighbours, which those lines cut

Re-run with:  python tests/golden/generate_calibration_golden.py [case ...]"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_shims  # noqa: E402
import calibration_fixture as F  # noqa: E402  (tests/calibration_fixture.py)


def run_case(name):
    ref_shims.install()
    from geotransformer.utils.data import calibrate_neighbors_stack_mode, registration_collate_fn_stack_mode
    params, kwargs, want_limits, want_pairs = F.CASES[name]
    hist_n = int(np.ceil(4 / 3 * np.pi * (params['search_radius'] / params['voxel_size'] + 1) ** 3))
    hists, dropped = [], []

    def collate(data_dicts, *args, **kw):
        dd = registration_collate_fn_stack_mode(data_dicts, *args, **kw)
        counts = [np.sum(neighbors.numpy() < neighbors.shape[0], axis=1) for neighbors in dd['neighbors']]
        hists.append(np.vstack([np.bincount(c, minlength=hist_n)[:hist_n] for c in counts]).astype(np.int32))
        dropped.append(np.array([int((c >= hist_n).sum()) for c in counts], np.int32))
        return dd

    limits = calibrate_neighbors_stack_mode(F.dataset(name), collate, params['num_stages'], params['voxel_size'], params['search_radius'],
                                            **kwargs)
    print(name, 'hist_n', hist_n, 'limits', limits.tolist(), 'pairs used', len(hists), 'rows', np.sum(hists, axis=(0, 2)).tolist(),
          'dropped', np.sum(dropped, axis=0).tolist(), flush=True)
    assert limits.tolist() == want_limits and len(hists) == want_pairs, (name, limits.tolist(), len(hists))
    if name == 'dense':       # the case of the dropped bin: it must neither lose that bin nor empty the histogram
        share = dropped[0][0] / float(dropped[0][0] + hists[0][0].sum())
        print('dense: share of stage-0 rows with %d or more neighbours %.3f' % (hist_n, share))
        assert 0.1 < share < 0.9
    return {name + '/limits': np.asarray(limits, np.int64), name + '/pairs_used': np.int64(len(hists)), name + '/hist': np.stack(hists),
            name + '/dropped': np.stack(dropped)}


if __name__ == '__main__':
    which = sys.argv[1:] or list(F.CASES)
    res = dict(np.load(F.FIXTURE)) if os.path.exists(F.FIXTURE) else {}
    torch.set_num_threads(8)
    for name in which:
        res.update(run_case(name))
    np.savez_compressed(F.FIXTURE, **res)
    print(F.FIXTURE, os.path.getsize(F.FIXTURE) // 1024, 'KiB')
