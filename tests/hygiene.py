"""Memory hygiene of the ops ("What a call may assume about memory"): no op may read a workspace word or an output
element that it did not write in the same call, and every op leaves the arrival counters of its workspace zero.  The parity tests cannot
see either: they start from fresh or zero memory and compare one call with a twin.  The tools here hand an op the memory of a long-running
process instead -- workspaces and `torch.empty` results filled with a byte, or with the leftovers of another shape -- and `judge` compares
what it returns, bit for bit, with what it returned in a cold process.  Imports torch alone; tests/test_hygiene_cpu.py drives it with CPU
tensors and planted faults, tests/test_gpu_hygiene.py with the real ops."""
import contextlib
import importlib
import pkgutil
import sys

import torch

from se3et_amd import caches

POISON_BYTES = (0xFF, 0x00)          # all ones: NaN as float32 / float16, -1 as an integer (an index outside everything); all zeros: the
#                                      value that the fresh memory of every other test happens to hold most of the time


def import_all():
    """Import every module of se3et_amd, so that every module-level Workspace exists."""
    import se3et_amd
    for m in pkgutil.walk_packages(se3et_amd.__path__, 'se3et_amd.'):
        importlib.import_module(m.name)


def workspaces(modules=None):
    """[(name, Workspace, counter prefix in bytes)] of every caches.Workspace alive, named 'module.attribute' after the module-level name it
    is bound to (modules: where to look; default: all of se3et_amd, imported first)."""
    if modules is None:
        import_all()
        modules = [m for name, m in sorted(sys.modules.items()) if m is not None and (name == 'se3et_amd' or name.startswith('se3et_amd.'))]
    found, seen = [], set()
    for m in modules:
        for attr, value in sorted(vars(m).items()):
            if isinstance(value, caches.Workspace) and id(value) not in seen:
                seen.add(id(value))
                found.append(('%s.%s' % (m.__name__.split('.')[-1], attr), value, int(value.counters)))
    return found


def _bytes(buffer):
    return buffer.reshape(-1).view(torch.uint8)


def poison(byte, spaces=None):
    """Fill every live buffer of every workspace with `byte`; of a counter workspace everything behind its prefix only (the prefix is
    contractual: zero between calls).  -> the number of bytes written."""
    total = 0
    for _, ws, prefix in (workspaces() if spaces is None else spaces):
        for buf in list(ws.buffers.values()):
            tail = _bytes(buf)[prefix:]
            tail.fill_(byte)
            total += tail.numel()
    return total


def counters_are_zero(spaces=None):
    """True when the counter prefix of every live buffer of every counter workspace holds zeros only; raises AssertionError naming the
    workspace and the first non-zero byte offset otherwise."""
    for name, ws, prefix in (workspaces() if spaces is None else spaces):
        if not prefix:
            continue
        for key, buf in list(ws.buffers.items()):
            head = _bytes(buf)[:prefix]
            bad = torch.nonzero(head)
            if bad.numel():
                off = int(bad[0, 0])
                word = int(head[off - off % 4:off - off % 4 + 4].cpu().view(torch.int32)[0]) if prefix >= 4 else int(head[off])
                raise AssertionError('%s: arrival counter at byte offset %d holds %d (buffer of %s): a call did not leave it zero'
                                     % (name, off - off % 4, word, key))
    return True


_POISON_DEVICES = ['cuda']          # (tests/test_hygiene_cpu.py adds 'cpu' for its fake ops)


def _fill(t, byte):
    """Fill the memory that a freshly made tensor `t` covers with `byte` (dense, or strided without overlap: every element is reached)."""
    if not (torch.is_tensor(t) and t.numel() and t.device.type in _POISON_DEVICES):
        return t
    if t.is_contiguous():
        _bytes(t).fill_(byte)
    else:
        with torch.no_grad():
            t.fill_(torch.full((t.element_size(),), byte, dtype=torch.uint8, device=t.device).view(t.dtype)[0])
    return t


@contextlib.contextmanager
def poisoned_empty(byte):
    """While the block runs, torch.empty, torch.empty_like, torch.empty_strided and Tensor.new_empty return memory filled with `byte`
    (non-empty device results, through a uint8 view).  The originals are put back on exit, also on error."""
    originals = [(torch, 'empty', torch.empty), (torch, 'empty_like', torch.empty_like), (torch, 'empty_strided', torch.empty_strided),
                 (torch.Tensor, 'new_empty', torch.Tensor.new_empty)]

    def wrap(fn):
        def poisoned(*args, **kwargs):
            return _fill(fn(*args, **kwargs), byte)
        poisoned.__name__ = getattr(fn, '__name__', 'empty')
        return poisoned
    try:
        for owner, name, fn in originals:
            setattr(owner, name, wrap(fn))
        yield
    finally:
        for owner, name, fn in originals:
            setattr(owner, name, fn)


def bits(t):
    """The integer view of a tensor's values (NaN equals NaN, -0.0 differs from 0.0): what two results are compared through."""
    t = t.detach().contiguous()
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    if t.dtype == torch.bool:
        return t.to(torch.uint8)
    return t.view(view) if t.dtype != view else t


def first_difference(got, want, region=None):
    """None when `got` equals `want` bit for bit on `region` (a bool mask of the output's shape, or an index / slice tuple; None: all of
    it), else a text naming the first differing element.  -> (text or None, elements compared, elements in all)."""
    if tuple(got.shape) != tuple(want.shape) or got.dtype != want.dtype:
        return 'shape / dtype %s %s, expected %s %s' % (tuple(got.shape), got.dtype, tuple(want.shape), want.dtype), 0, want.numel()
    a, b = bits(got), bits(want)
    if region is None:
        mask = None
        compared = want.numel()
    elif torch.is_tensor(region):
        mask = region.to(device=a.device, dtype=torch.bool).expand(a.shape)
        compared = int(mask.sum())
    else:
        mask = torch.zeros(a.shape, dtype=torch.bool, device=a.device)
        mask[region] = True
        compared = int(mask.sum())
    diff = a != b
    if mask is not None:
        diff &= mask
    if not bool(diff.any()):
        return None, compared, want.numel()
    at = tuple(int(i) for i in torch.nonzero(diff)[0])
    return 'element %s of shape %s: %r, expected %r (%d of %d compared elements differ)' % (
        at, tuple(want.shape), got[at].item(), want[at].item(), int(diff.sum()), compared), compared, want.numel()


class Dirty(AssertionError):
    """An op returned something that depends on memory it did not write, or left a counter set."""


def compare(what, got, want, regions=None, report=None):
    """Bitwise comparison of two tuples of outputs on their contractual regions (regions[i] as in first_difference; None entries and a
    missing `regions`: the whole output).  report: a list that receives (output index, compared, total) per output."""
    got, want = (x if isinstance(x, (tuple, list)) else (x,) for x in (got, want))
    if len(got) != len(want):
        raise Dirty('%s: %d outputs, expected %d' % (what, len(got), len(want)))
    for i, (g, w) in enumerate(zip(got, want)):
        if g is None or w is None:
            if g is not w:
                raise Dirty('%s: output %d is %s, expected %s' % (what, i, type(g).__name__, type(w).__name__))
            continue
        text, compared, total = first_difference(g, w, None if regions is None else regions[i])
        if report is not None:
            report.append((i, compared, total))
        if text is not None:
            raise Dirty('%s: output %d: %s' % (what, i, text))


def judge(case, stale=(), regions=None, spaces=None, clear=caches.clear_caches, refusals=(), before_poisoned=None, report=None, log=None):
    """Run the whole protocol on `case` (a callable without arguments -> tuple of output tensors):
      (a) cold: clear(), one call -> O0;
      (b) poisoned: workspaces and torch.empty* filled with 0xFF, then with 0x00, one call each -> equal to O0 (before_poisoned: called
          first, e.g. caches.clear_weight_caches, so that buffers derived from long-lived weights are built anew in poisoned memory);
      (c) stale: for every (label, callable) of `stale` -- the same op on a larger problem, on a smaller one, another op on the same
          workspace -- that call, then the case -> equal to O0;
      (d) the counter prefixes are zero after every call above;
      (e) refusals: callables that must raise RuntimeError / ValueError; afterwards the counters are zero and the case equals O0.
    regions: a function O0 -> per-output contractual regions (or None).  Raises Dirty on the first violation.  -> O0."""
    spaces = workspaces() if spaces is None else spaces

    def call(fn, what):
        out = fn()
        try:
            counters_are_zero(spaces)
        except AssertionError as e:
            raise Dirty('%s: %s' % (what, e)) from None
        return out

    clear()
    o0 = call(case, 'cold run')
    o0 = tuple(o0) if isinstance(o0, (tuple, list)) else (o0,)
    reg = None if regions is None else regions(o0)
    rep = []
    compare('cold run against itself', o0, o0, reg, rep)          # (the share of every output that the contract covers)
    if report is not None:
        report.extend(rep)
    if log is not None:
        for i, compared, total in rep:
            log('  output %d: %d of %d elements compared (%.1f %%)' % (i, compared, total, 100.0 * compared / max(total, 1)))
    for byte in POISON_BYTES:
        if before_poisoned is not None:
            before_poisoned()
        poison(byte, spaces)
        with poisoned_empty(byte):
            out = call(case, 'run on memory filled with 0x%02X' % byte)
        compare('run on memory filled with 0x%02X' % byte, out, o0, reg)
    for label, other in stale:
        call(other, label)
        compare('run after %s' % label, call(case, 'run after %s' % label), o0, reg)
    for refused in refusals:
        try:
            refused()
        except (RuntimeError, ValueError):
            pass
        else:
            raise Dirty('a documented refusal did not raise')
        try:
            counters_are_zero(spaces)
        except AssertionError as e:
            raise Dirty('after a refused call: %s' % e) from None
        compare('run after a refused call', call(case, 'run after a refused call'), o0, reg)
    return o0
