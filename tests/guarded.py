"""Guard zones and poison for every buffer a kernel of libaivc_hip.so touches: the software stand-in for an address sanitizer.
Not a test module and not a conftest: tests/test_guarded_harness.py proves it on the CPU, tests/test_gpu_memory_discipline.py runs
every device entry point of aivc_amd.ops under it.

The library allocates no device memory of its own: every buffer comes from a torch call in aivc_amd/ops.py or from the test.  So

  guarded_empty(shape, dtype, device, fill)   one arena `front guard | payload | back guard`, all of it the byte `fill`.  The
                                              payload starts on a 256-byte boundary, the back guard at the payload's last byte + 1
                                              (no rounding gap: an overrun of ONE element is seen), each guard is GUARD = 1 MiB
                                              (the largest output tile, 256 x 128 fp32, is 128 KiB: a whole stray tile lands inside).
                                              The tensor shares the arena's storage through Tensor.set_: it is no view (_base is None).
  guarded(array_or_tensor, device, fill)      the same for an input: payload = the data.
  guard_ops(fill)                             context manager: every torch.empty / empty_like / zeros of a CUDA tensor inside
                                              aivc_amd.ops goes through guarded_empty (zeros keeps a zero payload).  The product has
                                              no test-only branch for this: the module's `torch` global is replaced by a proxy that
                                              forwards everything else, host and pinned allocations included.  On exit it puts the real
                                              module back (also after an exception), synchronizes and checks every arena made since
                                              entry, those of guarded() / guarded_empty() calls in the body included: a guard byte that
                                              is not `fill` raises GuardError with the allocation site, the shape and the first
                                              offending byte offset relative to the payload.  It keeps no arena alive afterwards.
  both_fills(case)                            case(fill) inside guard_ops(fill) for each of FILLS; what the two runs return must be
                                              equal byte for byte.

The two fills.  0xFF makes every fp32 / fp64 word a NaN: a read outside an input that reaches the result poisons it, and so does
"multiply the stray value by a zero mask".  0xA5 is a second pattern: an output byte the kernel never wrote holds the fill, and an
integer result that a guard read influenced follows the fill; neither can equal the oracle under both.  Every guarded case
therefore runs once per fill and both runs are compared with the oracle.

ops.range_encode looks at _base and storage_offset() of its inputs to find bounds that already sit back to back in one tensor.
Its inputs may therefore stay plain tensors (slices of what the batched bounds kernels returned), so that this logic runs as in the
product; its outputs are guarded like every other allocation of ops.

Limits of the method:
  * a stray read whose value a select then discards is invisible (no fault, no effect on the result);
  * a stray access more than 1 MiB outside the payload is invisible;
  * the 4 GB sub-batching path of conv2d_mfma cannot be reached at test sizes and stays uncovered."""
import contextlib
import os
import sys

import numpy as np
import torch

GUARD = 1 << 20
ALIGN = 256
FILLS = (0xFF, 0xA5)

_HERE = os.path.abspath(__file__)
_SESSIONS = []  # the open guard_ops() (at most one)


class GuardError(AssertionError):
    pass


class _Arena:
    """one allocation: the uint8 arena, where the payload sits in it and who asked for it"""

    def __init__(self, arena, off, nbytes, shape, dtype, fill, site):
        self.arena, self.off, self.nbytes, self.shape, self.dtype, self.fill, self.site = arena, off, nbytes, shape, dtype, fill, site

    def guards(self):
        return self.arena[:self.off], self.arena[self.off + self.nbytes:]

    def first_bad(self):
        """byte offset, relative to the payload's first byte, of the first guard byte that is not the fill; None: intact"""
        front, back = self.guards()
        bad = (front != self.fill).nonzero()
        if bad.numel():
            return int(bad[0]) - self.off
        bad = (back != self.fill).nonzero()
        if bad.numel():
            return self.nbytes + int(bad[0])
        return None

    def describe(self, at):
        side = 'before the payload' if at < 0 else '%d past its last byte' % (at - self.nbytes + 1)
        return ('guard of the %s %s allocated at %s was written: first at byte offset %d relative to the payload (%s; payload %d bytes, fill 0x%02X)'
                % (tuple(self.shape), str(self.dtype).replace('torch.', ''), self.site, at, side, self.nbytes, self.fill))


def _site():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:
        return '?'
    return '%s:%d (%s)' % (os.path.basename(f.f_code.co_filename), f.f_lineno, f.f_code.co_name)


def guarded_empty(shape, dtype=torch.float32, device='cpu', fill=0xFF):
    shape = tuple(int(s) for s in ((shape,) if isinstance(shape, int) else shape))
    item = torch.empty(0, dtype=dtype).element_size()
    nbytes = int(np.prod(shape, dtype=np.int64)) * item
    arena = torch.empty(GUARD + ALIGN + nbytes + GUARD, dtype=torch.uint8, device=device)
    arena.fill_(fill)
    off = GUARD + (-(arena.data_ptr() + GUARD)) % ALIGN
    assert (arena.data_ptr() + off) % ALIGN == 0 and off % item == 0
    arena = arena[:off + nbytes + GUARD]  # the back guard: exactly GUARD bytes from the payload's last byte + 1
    strides, acc = [], 1
    for s in reversed(shape):
        strides.append(acc)
        acc *= max(s, 1)
    t = torch.empty(0, dtype=dtype, device=device).set_(arena.untyped_storage(), off // item, shape, tuple(reversed(strides)))
    assert t._base is None and t.is_contiguous() and (nbytes == 0 or t.data_ptr() == arena.data_ptr() + off)
    rec = _Arena(arena, off, nbytes, shape, dtype, fill, _site())
    t._guard = rec  # (check_guards(t) outside a guard_ops(); the storage is shared, so this keeps nothing extra alive)
    if _SESSIONS:
        _SESSIONS[-1].append(rec)
    return t


def guarded(a, device='cpu', fill=0xFF):
    src = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    t = guarded_empty(tuple(src.shape), src.dtype, device, fill)
    t.copy_(src)
    return t


def check_guards(*tensors_or_arenas):
    """raises GuardError for the first of the given guarded tensors whose guard no longer holds its fill"""
    for t in tensors_or_arenas:
        rec = t if isinstance(t, _Arena) else t._guard
        if rec.arena.is_cuda:
            torch.cuda.synchronize(rec.arena.device)
        at = rec.first_bad()
        if at is not None:
            raise GuardError(rec.describe(at))


class _TorchProxy:
    """stands in for the `torch` global of aivc_amd.ops: empty / empty_like / zeros of a tensor on a guarded device type come
    from guarded_empty, everything else is the real module's"""

    def __init__(self, real, fill, device_types):
        self.__dict__.update(_real=real, _fill=fill, _types=tuple(device_types))

    def __getattr__(self, name):
        return getattr(self._real, name)

    def __setattr__(self, name, value):
        raise AttributeError('the torch proxy of guard_ops is read-only')

    def _guarded_or_none(self, shape, dtype, device, pin_memory, zero, extra):
        dev = self._real.device('cpu' if device is None else device)
        if pin_memory or dev.type not in self._types:
            return None
        if extra:  # (an argument this harness has not been taught: say so, never hand out an unguarded buffer silently)
            raise NotImplementedError('guard_ops: torch allocation with %s' % sorted(extra))
        t = guarded_empty(shape, self._real.get_default_dtype() if dtype is None else dtype, dev, self._fill)
        if zero:
            t.zero_()
        return t

    def _alloc(self, name, size, kw, zero):
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        extra = {k: v for k, v in kw.items() if k not in ('dtype', 'device', 'pin_memory')}
        t = self._guarded_or_none(shape, kw.get('dtype'), kw.get('device'), kw.get('pin_memory', False), zero, extra)
        return getattr(self._real, name)(*size, **kw) if t is None else t

    def empty(self, *size, **kw):
        return self._alloc('empty', size, kw, False)

    def zeros(self, *size, **kw):
        return self._alloc('zeros', size, kw, True)

    def empty_like(self, x, **kw):
        extra = {k: v for k, v in kw.items() if k not in ('dtype', 'device', 'pin_memory')}
        t = self._guarded_or_none(tuple(x.shape), kw.get('dtype', x.dtype), kw.get('device', x.device), kw.get('pin_memory', False),
                                  False, extra)
        return self._real.empty_like(x, **kw) if t is None else t


@contextlib.contextmanager
def guard_ops(fill, device_types=('cuda',)):
    """see the module docstring.  device_types: which allocations of aivc_amd.ops are guarded (the CPU self-tests pass ('cpu',))"""
    from aivc_amd import ops
    assert not _SESSIONS, 'guard_ops does not nest'
    real = ops.torch
    assert real is torch, 'aivc_amd.ops.torch is not the torch module: an earlier guard_ops leaked'
    session = []
    _SESSIONS.append(session)
    ops.torch = _TorchProxy(real, fill, device_types)
    try:
        yield session
        ok = True
    except BaseException:
        ok = False
        raise
    finally:
        ops.torch = real
        _SESSIONS.remove(session)
        arenas, session[:] = list(session), []  # nothing stays alive through the harness
        if ok:  # (a failing body is reported as what it is)
            check_guards(*arenas)
        del arenas


def _as_bytes(v):
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().contiguous().view(torch.uint8).numpy() if v.numel() else np.zeros(0, np.uint8)
        return v.tobytes()
    if isinstance(v, np.ndarray):
        return np.ascontiguousarray(v).tobytes()
    if isinstance(v, dict):
        return {k: _as_bytes(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_as_bytes(x) for x in v]
    return v


def both_fills(case, device_types=('cuda',)):
    """case(fill) under guard_ops(fill) for each fill -> what the first run returned.  The results (tensors, arrays, nested in lists /
    tuples / dicts) of the two runs must be equal byte for byte: an output byte that was never written, or one that depends on a
    byte outside an input, follows the fill."""
    results = []
    for fill in FILLS:
        with guard_ops(fill, device_types):
            out = case(fill)
            results.append(_as_bytes(out))
        del out
    if results[0] != results[1]:
        raise GuardError('the result depends on the fill (0x%02X against 0x%02X): an output that was not written, or a read outside '
                         'an input that reaches the result' % FILLS)
    return results[0]
