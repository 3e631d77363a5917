"""The host-side caches and per-stream workspaces of se3et_amd: the one place that states their rules ("Host-side caches").  Imports torch
alone and touches no GPU until a device tensor is stored, so the rules are tested with CPU tensors.  Inserts, evictions, clear and validate
take LOCK; the hit paths take none (one dict read of an immutable entry)."""
import threading
import weakref

import torch

LOCK = threading.RLock()
CACHE_EPOCH = [0]          # bumped whenever weight-derived entries are dropped: part of the key of plans that hold raw pointers into them (cdriver)
_registered = weakref.WeakSet()      # every Derived and Workspace alive
also_clear = []                     # clear() of per-stream state that keeps its own logic (ops: embedding tables, amax rings)


class _Shared:
    """Device tensors built asynchronously on one stream and read from others (weight pieces, index tables: caches shared by the host
    threads of `--inflight N`, one HIP stream each).  A reader on another stream waits -- on the GPU, not the host -- for the event recorded
    behind the kernels that fill them, and tells the caching allocator that its stream uses the memory too.  (Without this the second
    thread's first GEMM could read weight pieces the first thread's split kernel had not written yet.)"""
    __slots__ = ('tensors', 'stream', 'event', 'raw')

    def __init__(self, *tensors):
        self.tensors = tensors
        self.stream = torch.cuda.current_stream()
        self.event = torch.cuda.Event()
        self.event.record(self.stream)
        self.raw = self.stream.cuda_stream

    def get(self):
        raw = getattr(torch._C, '_cuda_getCurrentRawStream', None)
        if raw is not None and raw(self.stream.device.index) == self.raw and torch.cuda.current_device() == self.stream.device.index:
            return self.tensors                              # the builder's own stream: nothing to wait for (and 2.6 us less host time)
        cur = torch.cuda.current_stream()
        if cur != self.stream:
            if not self.event.query():
                cur.wait_event(self.event)
            for t in self.tensors:
                t.record_stream(cur)
        return self.tensors


def _fingerprint(tensors):
    """Device-side content fingerprint (wrapping int64 sum of the bit patterns; one small launch per tensor, no host synchronisation)."""
    with torch.no_grad():
        sums = [t.detach().reshape(-1).view(torch.int32).sum(dtype=torch.int64) for t in tensors]
        return sums[0] if len(sums) == 1 else torch.stack(sums).sum()


def _current(recipes):
    """The fingerprint as it is now (each tensor found again through its base: a view object is a temporary), or None when one is gone."""
    bases = [(r(), view) for r, view in recipes]
    try:
        return _fingerprint([b if view is None else torch.as_strided(b, *view) for b, view in bases]) if all(b is not None for b, _ in bases) else None
    except RuntimeError:          # (the base was given a smaller storage: the view no longer exists)
        return None


_no_owner = type(None)          # (called like a dead weak reference: the `ref` slot of an entry with several owners)


def _owners(entry):
    return tuple(r() for r in (entry[:1] if entry[5] is None else entry[5]))


class Derived:
    """key -> value computed from tensors (the owners), shared by all host threads.  An entry is valid only while every owner IS the object
    it was stored for (weak reference compared by identity: a freed tensor's address and version can be inherited by another) at an unchanged
    `_version` (bumped by every in-place update).  An insert that finds more than `capacity` entries clears the cache (prune_dead: only the
    entries with a dead owner).  weights=True: clear_weight_caches() and validate_weight_caches() reach it (writes behind the version counter)."""

    def __init__(self, capacity, weights=False, prune_dead=False, share=True):
        self.entries, self.capacity, self.weights, self.prune_dead, self.share = {}, capacity, weights, prune_dead, share
        _registered.add(self)

    def lookup(self, owners, key):
        """The value stored for `key` if it is valid for `owners` (one tensor, or a tuple of them: the form it was stored with), else None."""
        hit = self.entries.get(key)
        if hit is None:
            return None
        if type(owners) is tuple:
            refs = hit[5]
            if refs is None or len(refs) != len(owners) or not all(r() is o and v == o._version for r, v, o in zip(refs, hit[1], owners)):
                return None
        elif hit[0]() is not owners or hit[1] != owners._version:          # (the single-owner path: most lookups of a forward)
            return None
        if hit[3] is not None:
            hit[3]()
        return hit[2]

    def store(self, owners, key, value, fingerprint_of=None):
        """The device tensors in `value` (itself, or members of a tuple) are handed to readers on other streams through _Shared (share=False:
        a cache whose values stay on their stream).  fingerprint_of: the tensors validate_weight_caches() holds the entry to."""
        tensors = [t for t in (value if type(value) is tuple else (value,)) if torch.is_tensor(t) and t.is_cuda] if self.share else []
        wait = _Shared(*tensors).get if tensors else None
        fp = None if fingerprint_of is None else (_fingerprint(fingerprint_of), [
            (weakref.ref(t), None) if t._base is None else (weakref.ref(t._base), (tuple(t.shape), t.stride(), t.storage_offset())) for t in fingerprint_of])
        with LOCK:
            if len(self.entries) > self.capacity:
                for k in [k for k, e in self.entries.items() if not self.prune_dead or None in _owners(e)]:
                    del self.entries[k]
            if type(owners) is tuple:          # (ref, version, value, wait, fingerprint, refs): `ref` of several owners never matches one
                self.entries[key] = (_no_owner, tuple(o._version for o in owners), value, wait, fp, tuple(weakref.ref(o) for o in owners))
            else:
                self.entries[key] = (weakref.ref(owners), owners._version, value, wait, fp, None)
        return value

    def entry(self, key):
        """(owner objects -- a dead one as None --, value) stored for `key`, valid or not, or None: for tests and tools."""
        hit = self.entries.get(key)
        return None if hit is None else (_owners(hit), hit[2])

    def clear(self):
        with LOCK:
            self.entries.clear()


class Workspace:
    """get(device, stream, nbytes): the grow-only uint8 buffer of ONE purpose on that stream (calls on a stream are ordered: one user at a
    time), at least nbytes long; allocated anew (size: a floor in bytes, or a function of nbytes) when there is none or it is too small.
    zeroed: zero when first handed out, never cleared again by the cache (its users leave it zero; ops._check_counters after an error).
    counters: the bytes at the start that hold arrival counters -- the only part whose content one call owes the next (zero); no call
    may depend on what any other byte of a workspace held when it began (tests/hygiene.py poisons them)."""
    weights = False

    def __init__(self, size, zeroed=False, counters=0):
        self.buffers, self.size, self.new, self.counters = {}, size, (torch.zeros if zeroed else torch.empty), counters
        _registered.add(self)

    def get(self, device, stream, nbytes):
        ws = self.buffers.get((device, stream))
        if ws is None or ws.numel() < nbytes:
            n = self.size(nbytes) if callable(self.size) else max(nbytes, self.size)
            ws = self.buffers[(device, stream)] = self.new((n,), dtype=torch.uint8, device=device)
        return ws

    def clear(self):
        self.buffers.clear()


def clear_caches(weights_only=False):
    """Everything registered, workspaces and per-stream state included (a cold process, for tests and tools), or the weight-derived only."""
    with LOCK:
        CACHE_EPOCH[0] += 1
        for c in list(_registered):
            if c.weights or not weights_only:
                c.clear()
        for clear in ([] if weights_only else also_clear):
            clear()


def clear_weight_caches():          # after writes behind torch's version counter (SE3ET.load_state_dict / ._apply call it)
    clear_caches(weights_only=True)


def validate_weight_caches():
    """Compares the content fingerprint of every weight-derived entry with the CURRENT values of the tensors it names (all sums on the
    device, one host synchronisation in all), drops the entries that no longer match or whose owner is gone and returns their number.  For
    code that writes weights behind torch's version counter (`p.data.copy_()`, EMA swaps through `.data`, hand-written checkpoint loaders)."""
    with LOCK:
        drop, live = [], []
        for c in [c for c in _registered if c.weights]:
            for key, hit in list(c.entries.items()):
                dead = None in _owners(hit)
                now = None if dead or hit[4] is None else _current(hit[4][1])
                if now is not None:
                    live.append((c, key, hit[4][0], now))
                elif dead or hit[4] is not None:          # (an entry without a fingerprint is only checked for a dead owner)
                    drop.append((c, key))
        if live:
            then, now = (torch.stack([e[i].to(live[0][2].device) for e in live]) for i in (2, 3))
            drop += [e[:2] for ok, e in zip((then == now).tolist(), live) if not ok]
        for c, key in drop:
            c.entries.pop(key, None)
        if drop:
            CACHE_EPOCH[0] += 1          # plans holding pointers to the dropped pieces (cdriver._static_plan) are rebuilt
    return len(drop)
