"""tests/guarded.py proved on the CPU: arenas on device='cpu', plain torch operations in the place of kernels.  Every check the
GPU suite (tests/test_gpu_memory_discipline.py) relies on is shown to fire -- a store one element past either end of a payload, a
store at the far end of a guard, an output that is partly unwritten, a read of a guard -- and a clean run to pass."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402

CPU = ('cpu',)


def _bytes_from(t, start, n):
    """n bytes of t's storage from byte `start` relative to its payload (what a kernel's stray pointer arithmetic reaches)"""
    rec = t._guard
    return rec.arena[rec.off + start:rec.off + start + n]


def _stray_store(t, elem):
    """one element of t's dtype stored at element index `elem` of the payload, in or out of bounds"""
    item = t.element_size()
    _bytes_from(t, elem * item, item).copy_(torch.zeros(item, dtype=torch.uint8))


@pytest.mark.parametrize('fill', G.FILLS)
@pytest.mark.parametrize('shape,dtype', [((3, 5, 7), torch.float32), ((13,), torch.uint8), ((2, 3), torch.float64), ((5, 1), torch.int16),
                                         (7, torch.float32)])
def test_layout_of_an_arena(shape, dtype, fill):
    t = G.guarded_empty(shape, dtype, 'cpu', fill)
    rec = t._guard
    assert t._base is None and t.is_contiguous() and t.dtype == dtype
    assert tuple(t.shape) == ((shape,) if isinstance(shape, int) else shape)
    assert t.data_ptr() % 256 == 0
    front, back = rec.guards()
    assert front.numel() >= G.GUARD == back.numel() == 1 << 20
    assert back.data_ptr() == t.data_ptr() + t.numel() * t.element_size()  # no gap behind the payload
    assert front.data_ptr() + front.numel() == t.data_ptr()
    assert bool((front == fill).all()) and bool((back == fill).all())
    assert bool((t.contiguous().view(-1).view(torch.uint8) == fill).all())  # the payload is poisoned too
    G.check_guards(t)
    empty = G.guarded_empty((0,), torch.int32, 'cpu', fill)  # (nothing to write to: the guards meet)
    assert empty.numel() == 0 and empty._guard.nbytes == 0
    G.check_guards(empty)


@pytest.mark.parametrize('fill', G.FILLS)
def test_guarded_input_holds_the_data(fill):
    a = np.arange(35, dtype=np.float32).reshape(5, 7)
    t = G.guarded(a, 'cpu', fill)
    assert t._base is None and torch.equal(t, torch.from_numpy(a))
    u = G.guarded(torch.arange(9, dtype=torch.int16), 'cpu', fill)
    assert u.dtype == torch.int16 and u.tolist() == list(range(9))
    G.check_guards(t, u)
    assert 'test_guarded_harness.py' in t._guard.site and 'test_guarded_input_holds_the_data' in t._guard.site


def _op_that_allocates(n, dtype=torch.float32):
    """an `operation` the way aivc_amd.ops writes them: the output comes from the module's torch global"""
    from aivc_amd import ops
    return ops.torch.empty((n,), dtype=dtype, device='cpu')


@pytest.mark.parametrize('fill', G.FILLS)
@pytest.mark.parametrize('dtype', [torch.float32, torch.uint8, torch.float64])
def test_store_one_element_past_the_end_is_seen(dtype, fill):
    with pytest.raises(G.GuardError) as e:
        with G.guard_ops(fill, CPU):
            out = _op_that_allocates(10, dtype)
            out.fill_(1)
            _stray_store(out, 10)
    item = torch.empty(0, dtype=dtype).element_size()
    msg = str(e.value)
    assert 'byte offset %d relative' % (10 * item) in msg and '1 past its last byte' in msg
    assert '(10,)' in msg and '_op_that_allocates' in msg and 'test_guarded_harness.py' in msg


@pytest.mark.parametrize('fill', G.FILLS)
def test_store_one_element_before_the_start_is_seen(fill):
    with pytest.raises(G.GuardError) as e:
        with G.guard_ops(fill, CPU):
            out = _op_that_allocates(10)
            out.fill_(1)
            _stray_store(out, -1)
    assert 'byte offset -4 relative' in str(e.value) and 'before the payload' in str(e.value)


@pytest.mark.parametrize('fill', G.FILLS)
def test_store_at_the_far_end_of_the_guard_is_seen(fill):
    with pytest.raises(G.GuardError) as e:
        with G.guard_ops(fill, CPU):
            out = _op_that_allocates(10, torch.uint8)
            out.fill_(1)
            _bytes_from(out, 10 + G.GUARD - 2, 1).fill_(fill ^ 0x01)  # 1 MiB - 1 past the last byte
    assert 'byte offset %d relative' % (10 + G.GUARD - 2) in str(e.value) and '%d past its last byte' % (G.GUARD - 1) in str(e.value)
    with pytest.raises(G.GuardError):
        with G.guard_ops(fill, CPU):
            out = _op_that_allocates(10, torch.uint8)
            _bytes_from(out, -G.GUARD, 1).fill_(fill ^ 0x80)  # and the first byte of the front guard


@pytest.mark.parametrize('fill', G.FILLS)
def test_guards_of_inputs_made_in_the_body_are_checked_too(fill):
    with pytest.raises(G.GuardError) as e:
        with G.guard_ops(fill, CPU):
            x = G.guarded(np.ones(6, np.float32), 'cpu', fill)
            _stray_store(x, 6)
    assert 'byte offset 24 relative' in str(e.value)


def test_partly_unwritten_output_fails_the_two_fill_comparison():
    def skips_the_last_element(fill):
        out = _op_that_allocates(8)
        out[:7] = torch.arange(7, dtype=torch.float32)  # the "kernel" forgets its tile edge
        return out

    def complete(fill):
        out = _op_that_allocates(8)
        out[:] = torch.arange(8, dtype=torch.float32)
        return {'y': out, 'more': [out.numpy().copy(), None, 3]}
    with pytest.raises(G.GuardError, match='depends on the fill'):
        G.both_fills(skips_the_last_element, CPU)
    got = G.both_fills(complete, CPU)
    assert got['y'] == np.arange(8, dtype=np.float32).tobytes()
    # an unwritten element equals neither fill's run of the other, whatever a stale allocator block would have held
    a, b = (np.frombuffer(bytes([f]) * 4, np.float32)[0] for f in G.FILLS)
    assert a.tobytes() != b.tobytes()


def test_integer_result_that_depends_on_a_guard_fails_the_two_fill_comparison():
    def reads_one_past(fill):
        x = G.guarded(np.arange(5, dtype=np.uint8), 'cpu', fill)
        out = _op_that_allocates(1, torch.int64)
        out[0] = int(x.sum()) + int(_bytes_from(x, 5, 1)[0])
        return out
    with pytest.raises(G.GuardError, match='depends on the fill'):
        G.both_fills(reads_one_past, CPU)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_reading_one_element_of_a_float_guard_gives_nan(dtype):
    x = G.guarded(torch.ones(6, dtype=dtype), 'cpu', 0xFF)
    item = x.element_size()
    for elem in (6, -1):
        stray = _bytes_from(x, elem * item, item).view(dtype)
        assert bool(torch.isnan(stray).all())
        assert bool(torch.isnan(x.sum() + stray[0]))
        assert bool(torch.isnan(stray[0] * 0.0))  # "multiply by a zero mask" does not clean it
    unwritten = G.guarded_empty((4,), dtype, 'cpu', 0xFF)
    assert bool(torch.isnan(unwritten).all())


@pytest.mark.parametrize('fill', G.FILLS)
def test_clean_run_passes_and_zeros_keeps_a_zero_payload(fill):
    from aivc_amd import ops
    with G.guard_ops(fill, CPU) as arenas:
        a = ops.torch.empty((3, 4), dtype=torch.float32, device='cpu')
        b = ops.torch.empty(5, 2, dtype=torch.int16, device=torch.device('cpu'))
        z = ops.torch.zeros((2, 3), dtype=torch.float64, device='cpu')
        like = ops.torch.empty_like(a)
        like8 = ops.torch.empty_like(a, dtype=torch.uint8)
        for t in (a, b, z, like, like8):
            assert hasattr(t, '_guard') and t._base is None
        assert tuple(b.shape) == (5, 2) and tuple(like.shape) == (3, 4) and like8.dtype == torch.uint8
        assert not z.any() and bool((z._guard.guards()[1] == fill).all())
        a.fill_(2.0), b.fill_(3), like.copy_(a), like8.fill_(1)
        assert len(arenas) == 5
        # everything else is the real module's
        assert ops.torch.float32 is torch.float32 and ops.torch.cat is torch.cat and ops.torch.cuda is torch.cuda
        assert ops.torch.ones(3).tolist() == [1.0, 1.0, 1.0]
    assert arenas == []  # no arena is kept alive


def test_other_device_types_and_pinned_requests_pass_through():
    from aivc_amd import ops
    with G.guard_ops(0xFF) as arenas:  # the product's setting: CUDA allocations only
        host = ops.torch.empty((4,), dtype=torch.uint8)
        host2 = ops.torch.zeros(3, dtype=torch.float32, device='cpu')
        like = ops.torch.empty_like(host2)
        assert not any(hasattr(t, '_guard') for t in (host, host2, like)) and arenas == []
    with G.guard_ops(0xFF, CPU):
        with pytest.raises(NotImplementedError):  # an allocation the harness cannot guard is refused, never handed out unguarded
            ops.torch.empty((4,), dtype=torch.float32, device='cpu', requires_grad=True)


def test_guard_ops_restores_the_module_exactly():
    from aivc_amd import ops
    before = dict(vars(ops))
    with G.guard_ops(0xA5, CPU):
        assert ops.torch is not torch
        ops.torch.empty((2,), dtype=torch.float32, device='cpu').fill_(0)
    assert ops.torch is torch and dict(vars(ops)) == before
    with pytest.raises(ZeroDivisionError):
        with G.guard_ops(0xA5, CPU):
            out = _op_that_allocates(4)
            _stray_store(out, 4)  # (the body's own failure is what is reported)
            1 / 0
    assert ops.torch is torch and dict(vars(ops)) == before and G._SESSIONS == []
    with pytest.raises(G.GuardError):
        with G.guard_ops(0xA5, CPU):
            _stray_store(_op_that_allocates(4), 4)
    assert ops.torch is torch and dict(vars(ops)) == before and G._SESSIONS == []
