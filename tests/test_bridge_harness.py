"""The helpers of tests/bridge.py do what the GPU tests of the ops bridge rely on -- checked here, without a GPU and without the
library -- and the case list of tests/test_gpu_ops_arguments.py names every public function of aivc_amd.ops that reaches it."""
import inspect

import numpy as np
import pytest
import torch

import bridge
from op_cases import Case


def test_placer_reaches_every_leaf_once_and_names_it():
    a = [np.full(2, i, np.int16) for i in range(7)]
    inputs = {'x': a[0], 'none': None, 'parts': [{'y': a[1], 'u': a[2]}, None, a[3]], 'syms': (a[4], None, a[5]), 'deep': {'er': {'z': a[6]}}}
    names = ['x', 'parts[0].y', 'parts[0].u', 'parts[2]', 'syms[0]', 'syms[2]', 'deep.er.z']
    assert [nm for nm, _ in bridge.leaves(inputs)] == names
    assert all(arr is a[i] for i, (_, arr) in enumerate(bridge.leaves(inputs)))
    case = Case(inputs, None, None)
    seen = []
    case.place(lambda arr: seen.append(int(arr[0])))
    assert seen == list(range(7))  # leaves() numbers them as Case.place visits them
    for k in range(7):
        put = bridge.Target(lambda arr: ('plain', int(arr[0])), k, lambda t: ('changed', t[1]))
        d = case.place(put)
        flat = [d['x'], d['parts'][0]['y'], d['parts'][0]['u'], d['parts'][2], d['syms'][0], d['syms'][2], d['deep']['er']['z']]
        assert flat == [('changed' if i == k else 'plain', i) for i in range(7)] and put.hit and put.n == 7
        assert d['none'] is None and d['parts'][1] is None and d['syms'][1] is None
    put = bridge.Target(lambda arr: 0, 7, lambda t: 1)
    case.place(put)
    assert not put.hit


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.uint8, torch.int16, torch.int32, torch.int64])
@pytest.mark.parametrize('shape', [(7,), (5, 1), (3, 5, 4), (1, 1, 9, 1), (2, 3, 5, 7)])
def test_changed_tensors_are_what_they_claim(shape, dtype):
    n = int(np.prod(shape))
    t = (torch.arange(n, dtype=torch.float64) - 3).to(dtype).reshape(shape)
    s = bridge.strided(t)
    assert s.shape == t.shape and s.dtype == t.dtype and torch.equal(s, t) and not s.is_contiguous() and s.data_ptr() % 16 == 0
    short = bridge.one_short(t)
    assert short.dim() == 1 and short.numel() == n - 1 and torch.equal(short, t.reshape(-1)[:-1])
    other = bridge.other_dtype(t)
    assert other.shape == t.shape and other.dtype != t.dtype
    if dtype == torch.float32:
        assert other.dtype == torch.float64
    if not dtype.is_floating_point and dtype != torch.int64:
        assert not other.dtype.is_floating_point and other.element_size() > t.element_size() and torch.equal(other.to(dtype), t)
    assert bridge.on_cpu(t).device.type == 'cpu'


def test_one_element_has_no_strided_form():
    assert bridge.strided(torch.zeros(1)) is None and bridge.strided(torch.zeros((1, 1, 1))) is None


class FakeOps:
    """what the recorder touches of aivc_amd.ops, over a fake function table (no library)"""

    class AivcNativeError(RuntimeError):
        pass

    def __init__(self):
        self.launched = []

        def fn(name, rc=0):
            def f(*args):
                self.launched.append((name, args))
                return rc
            return f
        self.table = {nm: fn(nm) for nm in ('aivc_conv2d', 'aivc_conv_images', 'aivc_warp') + bridge.HOST_ONLY}
        self.table['aivc_fails'] = fn('aivc_fails', 3)
        self.call = self.real_call = lambda name, *args: self.table[name](*args)
        self.load = self.real_load = lambda: self.table


def test_recorder_stands_in_for_every_launching_function_and_never_calls_it():
    ops = FakeOps()
    with bridge.recording(ops, table=ops.table):
        for name in ('aivc_conv2d', 'aivc_warp'):
            with pytest.raises(bridge.Reached) as r:
                ops.call(name, 1, 2)
            assert r.value.name == name and repr(r.value) == 'Reached(%r)' % name
        stand_in = ops.load()['aivc_conv_images']  # (reached through load()[...], not call)
        assert stand_in is not ops.table['aivc_conv_images']
        with pytest.raises(bridge.Reached) as r:
            stand_in(None, 1)
        assert r.value.name == 'aivc_conv_images'
        assert ops.launched == []  # nothing got through
        for name in bridge.HOST_ONLY:  # the host-only queries stay real
            assert ops.load()[name] is ops.table[name]
            ops.load()[name](7)
        ops.call('aivc_abi_version')
        assert [nm for nm, _ in ops.launched] == list(bridge.HOST_ONLY) + ['aivc_abi_version']


def test_recorder_restores_call_and_load_after_an_exception():
    ops = FakeOps()
    for forward in (False, True):
        with pytest.raises(bridge.Reached if not forward else KeyError):
            with bridge.recording(ops, forward=forward, table=ops.table):
                assert ops.call is not ops.real_call and ops.load is not ops.real_load
                ops.call('aivc_conv2d') if not forward else ops.load()['no such function']
        assert ops.call is ops.real_call and ops.load is ops.real_load


def test_forwarding_recorder_calls_the_function_then_probes():
    ops = FakeOps()
    state = []
    with bridge.recording(ops, forward=True, probe=lambda: len(ops.launched), table=ops.table) as rec:
        ops.call('aivc_conv2d', 5)
        assert ops.load()['aivc_conv_images'](6) == 0
        ops.load()['aivc_conv2d_variant'](1)  # host only: real, not recorded
        with pytest.raises(FakeOps.AivcNativeError):
            ops.call('aivc_fails')
        state = list(rec.calls)
    # (the probe ran after each call: it saw that call among the launched)
    assert state == [('aivc_conv2d', 1), ('aivc_conv_images', 2), ('aivc_fails', 4)]
    assert [nm for nm, _ in ops.launched] == ['aivc_conv2d', 'aivc_conv_images', 'aivc_conv2d_variant', 'aivc_fails']


def test_raises_before_the_library():
    from aivc_amd._lib import AivcNativeError
    for exc in (ValueError('x'), AivcNativeError('x')):
        with bridge.raises_before_the_library('ok'):
            raise exc
    with pytest.raises(AssertionError, match=r"leaf: handed to the library \(Reached\('aivc_conv2d'\)\)"):
        with bridge.raises_before_the_library('leaf'):
            raise bridge.Reached('aivc_conv2d')
    with pytest.raises(AssertionError, match='leaf: accepted'):
        with bridge.raises_before_the_library('leaf'):
            pass
    with pytest.raises(RuntimeError):  # (any other exception is not a rejection: it passes through)
        with bridge.raises_before_the_library('leaf'):
            raise RuntimeError('x')


def reaches_the_library():
    """the public functions of aivc_amd.ops whose source calls the library: call( or load()[ """
    from aivc_amd import ops
    names = []
    for name, fn in vars(ops).items():
        if name.startswith('_') or not inspect.isfunction(fn) or fn.__module__ != ops.__name__:
            continue
        src = inspect.getsource(fn)
        if 'call(' in src or 'load()[' in src:
            names.append(name)
    return sorted(names)


def test_every_wrapper_that_reaches_the_library_has_an_entry():
    """a wrapper added to aivc_amd.ops without an entry in the case list fails here"""
    import test_gpu_ops_arguments as args
    from aivc_amd import ops
    wrappers = reaches_the_library()
    assert len(wrappers) > 40 and {'conv2d', 'md5_planes', 'range_encode', 'slab_contract', 'inflate_launch'} <= set(wrappers)
    covered = {fn for e in args.ENTRIES for fn in e.covers}
    assert all(hasattr(ops, fn) for fn in covered), sorted(fn for fn in covered if not hasattr(ops, fn))
    missing = [w for w in wrappers if w not in covered]
    assert not missing, 'aivc_amd.ops wrappers without an entry in tests/test_gpu_ops_arguments.py: %s' % missing
