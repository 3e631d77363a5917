"""The rules of se3et_amd/caches.py ("Host-side caches"), driven with CPU tensors: no GPU and no built library needed."""
import gc
import threading

import torch

from se3et_amd import caches


def _param(*shape, seed=0):
    return torch.nn.Parameter(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)), requires_grad=False)


def test_entry_is_valid_for_the_same_object_at_the_same_version_only():
    cache = caches.Derived(8, weights=True)
    w = _param(4, 6)
    key = (w.data_ptr(), 4, 6)
    assert cache.lookup(w, key) is None
    value = cache.store(w, key, w.detach() * 2, fingerprint_of=(w,))
    assert cache.lookup(w, key) is value and cache.entry(key)[0] == (w,)
    # another Parameter on the same storage at the same version: same key, not the owner
    other = torch.nn.Parameter(torch.empty_like(w), requires_grad=False)
    other.data = w.data
    assert other.data_ptr() == w.data_ptr() and other._version == w._version
    assert cache.lookup(other, key) is None and cache.lookup((w, other), key) is None and cache.lookup((other,), key) is None
    # an in-place update bumps the version
    with torch.no_grad():
        w.mul_(2.0)
    assert cache.lookup(w, key) is None
    cache.store(w, key, 'again')
    assert cache.lookup(w, key) == 'again'


def test_dead_owner_is_a_miss_and_is_dropped():
    cache = caches.Derived(8, weights=True)
    w, x = _param(3, 3), _param(3, 3, seed=1)
    cache.store(w, 'k', True)               # host value, no fingerprint: only checked for a dead owner
    cache.store(x, 'x', False)
    assert cache.lookup(w, 'k') is True and cache.lookup(x, 'x') is False
    assert caches.validate_weight_caches() == 0
    del w
    gc.collect()
    assert cache.lookup(x, 'k') is None and cache.entry('k')[0] == (None,)
    epoch = caches.CACHE_EPOCH[0]
    assert caches.validate_weight_caches() == 1
    assert cache.entry('k') is None and cache.lookup(x, 'x') is False and caches.CACHE_EPOCH[0] == epoch + 1


def test_view_entry_is_owned_by_its_base():
    w = _param(4, 6)
    assert w.detach().view(24)._base is not w
    with torch.no_grad():
        flat, block = w.view(24), w[:, :2]
    assert flat._base is w and block._base is w
    cache = caches.Derived(8, weights=True)
    key = (block.data_ptr(), 4, 2, block.stride(0))
    cache.store(block._base, key, 'pieces', fingerprint_of=(block,))
    del flat, block
    gc.collect()
    with torch.no_grad():
        again = w[:, :2]
    assert cache.lookup(again._base, key) == 'pieces'          # a new view object of the same base
    w.data[:, 2:].mul_(3.0)                                     # outside the block, behind the version counter
    assert caches.validate_weight_caches() == 0 and cache.lookup(w, key) == 'pieces'
    w.data[:, :2].mul_(3.0)                                     # inside the block
    assert caches.validate_weight_caches() == 1 and cache.lookup(w, key) is None


def test_validate_drops_exactly_the_entries_rewritten_behind_the_version_counter():
    cache, second = caches.Derived(8, weights=True), caches.Derived(8, weights=True)
    geometry = caches.Derived(8)
    ws = [_param(5, 5, seed=i) for i in range(4)]
    for i, w in enumerate(ws):
        cache.store(w, i, w.detach().clone(), fingerprint_of=(w,))
    second.store(ws[1], 'derived', 1.0, fingerprint_of=(ws[1],))
    geometry.store(ws[1], 'order', 2.0, fingerprint_of=(ws[1],))            # not weight-derived: validate leaves it alone
    several = caches.Derived(1, weights=True)
    several.store(tuple(ws), 'composed', 'c', fingerprint_of=tuple(ws))
    assert several.lookup(tuple(ws), 'composed') == 'c' and several.lookup(tuple(ws[:3]), 'composed') is None
    assert caches.validate_weight_caches() == 0
    versions = [w._version for w in ws]
    ws[1].data.copy_(ws[1].data * -2.0)
    ws[3].data.copy_(ws[3].data + 1.0)
    assert [w._version for w in ws] == versions
    assert cache.lookup(ws[1], 1) is not None                  # the version rule cannot see the write
    epoch = caches.CACHE_EPOCH[0]
    assert caches.validate_weight_caches() == 4                 # entries 1 and 3, the one of `second`, the entry with several owners
    assert caches.CACHE_EPOCH[0] == epoch + 1
    assert [cache.lookup(w, i) is not None for i, w in enumerate(ws)] == [True, False, True, False]
    assert second.lookup(ws[1], 'derived') is None and several.lookup(tuple(ws), 'composed') is None
    assert geometry.lookup(ws[1], 'order') == 2.0
    assert caches.validate_weight_caches() == 0 and caches.CACHE_EPOCH[0] == epoch + 1


def test_capacity_and_clear():
    cache = caches.Derived(3, weights=True)
    ws = [_param(2, 2, seed=i) for i in range(6)]
    for i in range(4):
        cache.store(ws[i], i, i)
    assert len(cache.entries) == 4                              # an insert clears the cache when it FINDS more than `capacity` entries
    cache.store(ws[4], 4, 4)
    assert list(cache.entries) == [4]
    pruned = caches.Derived(3, prune_dead=True)
    for i in range(4):
        pruned.store(ws[i], i, i)
    del ws[0], ws[0]                                            # the owners of entries 0 and 1
    gc.collect()
    pruned.store(ws[3], 5, 5)
    assert sorted(pruned.entries) == [2, 3, 5]
    shapes = caches.Derived(2)                                  # no owners: constant tables keyed by shape
    assert shapes.store((), (3, 4), 'rows') == 'rows' and shapes.lookup((), (3, 4)) == 'rows'
    space = caches.Workspace(16)
    space.get('cpu', 0, 8)
    called = []
    caches.also_clear.append(lambda: called.append(1))
    try:
        epoch = caches.CACHE_EPOCH[0]
        caches.clear_weight_caches()
        assert not cache.entries and pruned.entries and shapes.entries and space.buffers and not called and caches.CACHE_EPOCH[0] == epoch + 1
        caches.clear_caches()
        assert not pruned.entries and not shapes.entries and not space.buffers and called == [1]
    finally:
        caches.also_clear.pop()


def test_workspace_is_per_purpose_and_stream_and_grows():
    a, b, z = caches.Workspace(64), caches.Workspace(64), caches.Workspace(32, zeroed=True)
    grow = caches.Workspace(lambda n: int(n * 1.1) + 256)
    w0 = a.get('cpu', 7, 10)
    assert w0.dtype == torch.uint8 and w0.numel() == 64
    assert a.get('cpu', 7, 64) is w0 and a.get('cpu', 7, 1) is w0
    assert a.get('cpu', 8, 10) is not w0                        # another stream
    assert b.get('cpu', 7, 10) is not w0 and b.get('cpu', 7, 10).data_ptr() != w0.data_ptr()        # another purpose
    w1 = a.get('cpu', 7, 65)
    assert w1 is not w0 and w1.numel() == 65 and a.get('cpu', 7, 10) is w1
    zz = z.get('cpu', 7, 100)
    assert zz.numel() == 100 and not zz.any()
    zz.fill_(1)
    assert z.get('cpu', 7, 50) is zz and bool(zz.all())         # never re-zeroed by the cache
    assert grow.get('cpu', 0, 1000).numel() == 1356


def test_threads_on_overlapping_keys():
    cache = caches.Derived(5, weights=True)
    ws = [_param(2, 2, seed=i) for i in range(8)]
    failed = []

    def work(t):
        try:
            for n in range(2000):
                k = (n * (t + 1) + t) % 8
                hit = cache.lookup(ws[k], k)
                if hit is None:
                    hit = cache.store(ws[k], k, ('value of', k), fingerprint_of=(ws[k],))
                assert hit == ('value of', k)
                if n % 500 == 499:
                    caches.validate_weight_caches() if t % 2 else cache.clear()
        except BaseException as e:
            failed.append(e)

    pool = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in pool:
        th.start()
    for th in pool:
        th.join()
    assert not failed, failed[0]
