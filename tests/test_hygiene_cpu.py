"""tests/hygiene.py judged on fake ops with CPU tensors: a clean op passes, each planted fault -- an output element never written, a
workspace word read before it is written, a counter left at 1 on an early return, an error return that leaves a counter set -- fails; and
the case table of tests/test_gpu_hygiene.py answers for every Workspace of the package."""
import pytest
import torch

import hygiene
from se3et_amd import caches

PREFIX = 16          # bytes of arrival counters at the start of the fake workspace


class FakeOp:
    """y = 2 x + 1 through a counter workspace, the way the real ops use theirs: partials behind the counter prefix, an arrival counter
    that goes up while the call runs and back to zero when it completes, a `torch.empty` output.  `fault` plants one defect."""

    def __init__(self, fault=None):
        self.fault = fault
        self.ws = caches.Workspace(64, zeroed=True, counters=PREFIX)
        self.spaces = [('fake._ws', self.ws, PREFIX)]

    def __call__(self, x):
        n = x.numel()
        buf = self.ws.get('cpu', 0, PREFIX + 4 * n)
        counter, part = buf[:PREFIX].view(torch.int32), buf[PREFIX:PREFIX + 4 * n].view(torch.float32)
        if n > 12:
            if self.fault == 'error return':
                counter[1] += 1
            raise RuntimeError('fake op: at most 12 elements')
        counter[0] += 1
        if n < 4 and self.fault == 'early return':
            return (torch.zeros(n),)
        written = n - 1 if self.fault == 'workspace word' else n
        part[:written] = 2 * x[:written]
        out = torch.empty(n)
        filled = n - 1 if self.fault == 'output element' else n
        out[:filled] = part[:filled] + 1
        counter[0] = 0
        return (out,)


def _judge(op, **kw):
    x, big, small = torch.arange(8.0), torch.arange(11.0), torch.arange(3.0)
    return hygiene.judge(lambda: op(x), stale=[('the larger problem', lambda: op(big)), ('the smaller problem', lambda: op(small))], spaces=op.spaces, clear=op.ws.clear,
                         refusals=[lambda: op(torch.arange(13.0))], **kw)


@pytest.fixture(autouse=True)
def _poison_cpu_tensors(monkeypatch):
    monkeypatch.setattr(hygiene, '_POISON_DEVICES', ['cuda', 'cpu'])


def test_a_clean_op_passes():
    report = []
    (out,) = _judge(FakeOp(), report=report)
    assert torch.equal(out, 2 * torch.arange(8.0) + 1) and report == [(0, 8, 8)]


@pytest.mark.parametrize('fault, message', [('output element', r'filled with 0x(FF|00): output 0: element \(7,\)'),
                                            ('workspace word', r'filled with 0xFF: output 0: element \(7,\)'),
                                            ('early return', r'the smaller problem: fake\._ws: arrival counter at byte offset 0 holds 1'),
                                            ('error return', r'after a refused call: fake\._ws: arrival counter at byte offset 4 holds 1')])
def test_a_planted_fault_fails_the_judge(fault, message):
    with pytest.raises(hygiene.Dirty, match=message):
        _judge(FakeOp(fault))


def test_a_region_outside_the_contract_is_not_compared_and_is_counted():
    op, report = FakeOp('output element'), []
    _judge(op, regions=lambda o0: [(slice(0, 7),)], report=report)
    assert report == [(0, 7, 8)]
    mask = torch.ones(8, dtype=torch.bool)
    mask[7] = False
    _judge(op, regions=lambda o0: [mask])


def test_poison_spares_the_counter_prefix_and_reaches_every_other_byte():
    op = FakeOp()
    op(torch.arange(8.0))
    (buf,) = op.ws.buffers.values()
    assert hygiene.poison(0xFF, op.spaces) == buf.numel() - PREFIX
    assert not buf[:PREFIX].any() and bool((buf[PREFIX:] == 0xFF).all())
    assert hygiene.counters_are_zero(op.spaces)
    buf[9] = 2
    with pytest.raises(AssertionError, match=r'fake\._ws: arrival counter at byte offset 8 holds 512'):
        hygiene.counters_are_zero(op.spaces)


def test_poisoned_empty_fills_and_restores_also_on_error():
    originals = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    with pytest.raises(ZeroDivisionError):
        with hygiene.poisoned_empty(0xFF):
            a = torch.empty((3, 5), dtype=torch.int64)
            b = torch.empty_like(torch.zeros(4, dtype=torch.float16))
            c = torch.empty_strided((2, 3), (1, 2))          # (not contiguous: filled through the pattern of its dtype)
            d = torch.zeros(2, dtype=torch.int32).new_empty((6,))
            e = torch.empty((0, 4))
            assert bool((a == -1).all()) and bool(b.isnan().all()) and bool(c.isnan().all()) and bool((d == -1).all()) and e.numel() == 0
            1 / 0
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == originals
    with hygiene.poisoned_empty(0x00):
        assert not torch.empty(64).any()
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == originals


def test_bitwise_comparison_takes_nan_for_nan_and_tells_the_zeros_apart():
    a = torch.tensor([float('nan'), 0.0, 1.0])
    assert hygiene.first_difference(a, a.clone())[0] is None
    text, compared, total = hygiene.first_difference(a, torch.tensor([float('nan'), -0.0, 1.0]))
    assert 'element (1,)' in text and (compared, total) == (3, 3)
    assert hygiene.first_difference(a, a.double())[0].startswith('shape / dtype')
    with pytest.raises(hygiene.Dirty, match='1 outputs, expected 2'):
        hygiene.compare('x', (a,), (a, a))


def test_every_workspace_of_the_package_has_a_gpu_case():
    import test_gpu_hygiene as gpu
    names = [name for name, _, _ in hygiene.workspaces()]
    assert len(names) == len(set(names)) and len(names) >= 19
    with_counters = {name: prefix for name, _, prefix in hygiene.workspaces() if prefix}
    from se3et_amd import ops
    assert with_counters == {'ops.' + k: v for k, v in ops.COUNTER_BYTES.items()}
    covered = {name for case in gpu.CASES for name in case.workspaces}
    assert covered <= set(names), 'cases name workspaces that do not exist: %s' % sorted(covered - set(names))
    missing = sorted(set(names) - covered)
    assert not missing, 'no case of tests/test_gpu_hygiene.py runs on %s' % ', '.join(missing)
    ids = [case.name for case in gpu.CASES]
    assert len(ids) == len(set(ids))
