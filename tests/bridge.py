"""Helpers of the tests of the ops bridge (tests/test_bridge_harness.py, test_gpu_ops_arguments.py, test_gpu_ops_streams.py):
aivc_amd/ops.py is the one place where a tensor becomes a raw pointer and torch's current stream a hipStream_t.  Not a test module.

  recording()   a context manager that replaces ops.call and ops.load for its body and puts them back afterwards, also after an
                exception.  The host-only queries (HOST_ONLY) stay real.  In the default mode every other native function is a
                stand-in that raises Reached(name) WITHOUT calling the library: a defective argument that gets this far would have
                been handed to a kernel.  With forward=True the real function is called and (name, probe()) is appended to
                the recorder's `calls` after it returns.

  Target        a placer that hands ONE leaf of a case's inputs a changed tensor.  Case.place(put) (tests/op_cases.py, place_all)
                walks the inputs depth first, dicts in insertion order, lists by index, and calls put on every array; a None is no
                leaf.  Leaf k is the k-th such call, and its NAME is the path of dict keys and list indices that leads to it:
                'bias', 'parts[0].y', 'syms[3]'.  leaves(inputs) -> [(name, array)] in that order.

  the changed tensors, each made from the plain device tensor t:
    on_cpu        t.cpu()
    other_dtype   float32 -> float64, every integer type -> the next wider one (int64 -> float64, float64 -> float32)
    one_short     t.reshape(-1)[:-1]: one dimension, one element too few; never a valid form of the same call
    strided       the shape and values of t, not contiguous, data_ptr() on a 16-byte boundary: every second element of a buffer twice
                  the size.  A tensor of one element has no such form (torch calls it contiguous whatever its strides): None
"""
import contextlib

import torch

HOST_ONLY = ('aivc_conv2d_variant', 'aivc_metrics_workspace', 'aivc_abi_version', 'aivc_last_error')


class Reached(Exception):
    """a native function that launches was called: .name says which"""

    def __init__(self, name):
        Exception.__init__(self, name)
        self.name = name

    def __repr__(self):
        return 'Reached(%r)' % self.name

    __str__ = __repr__


class _Table:
    """what ops.load() returns under the recorder: name -> the real function (host-only queries), a stand-in or a forwarder"""

    def __init__(self, rec):
        self.rec = rec

    def __getitem__(self, name):
        return self.rec.function(name)

    def __contains__(self, name):
        return name in self.rec.real_load()


class Recorder:
    def __init__(self, ops, forward=False, probe=None, table=None):
        """table: the function table to stand in for (default: the library's, asked for on first use)"""
        self.ops, self.forward, self.probe, self.table = ops, forward, probe, table
        self.calls = []

    def real_load(self):
        return self.table if self.table is not None else self._load()

    def function(self, name):
        if name in HOST_ONLY:
            return self.real_load()[name]
        if not self.forward:
            def stand_in(*args):
                raise Reached(name)
            return stand_in
        real = self.real_load()[name]

        def forwarder(*args):
            rc = real(*args)
            self.calls.append((name, None if self.probe is None else self.probe()))
            return rc
        return forwarder

    def call(self, name, *args):
        if name not in HOST_ONLY and not self.forward:
            raise Reached(name)
        if self.table is None and name not in HOST_ONLY:
            self._call(name, *args)  # (the real call(): it words a failure)
            self.calls.append((name, None if self.probe is None else self.probe()))
            return
        rc = self.function(name)(*args)
        if rc != 0:
            raise self.ops.AivcNativeError('%s failed (%s)' % (name, rc))

    def __enter__(self):
        self._call, self._load = self.ops.call, self.ops.load
        self.ops.call, self.ops.load = self.call, lambda: _Table(self)
        return self

    def __exit__(self, *exc):
        self.ops.call, self.ops.load = self._call, self._load
        return False


def recording(ops, forward=False, probe=None, table=None):
    return Recorder(ops, forward, probe, table)


# ---- leaves ------------------------------------------------------------------------------------------------------------------------
def leaves(inputs):
    """[(name, array)] of every array leaf, in the order Case.place calls its placer"""
    out = []

    def walk(v, path):
        if v is None:
            return
        if isinstance(v, dict):
            for k, x in v.items():
                walk(x, '%s.%s' % (path, k) if path else str(k))
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk(x, '%s[%d]' % (path, i))
        else:
            out.append((path, v))
    walk(inputs, '')
    return out


class Target:
    """put for every leaf but number k, change(put(a)) for that one; .hit: whether leaf k was placed"""

    def __init__(self, put, k, change):
        self.put, self.k, self.change, self.n, self.hit = put, k, change, 0, False

    def __call__(self, a):
        t = self.put(a)
        i, self.n = self.n, self.n + 1
        if i != self.k:
            return t
        self.hit = True
        return self.change(t)


# ---- the changed tensors -----------------------------------------------------------------------------------------------------------
WIDER = {torch.float32: torch.float64, torch.float64: torch.float32, torch.uint8: torch.int16, torch.int8: torch.int16,
         torch.int16: torch.int32, torch.int32: torch.int64, torch.int64: torch.float64}


def on_cpu(t):
    return t.cpu()


def other_dtype(t):
    return t.to(WIDER[t.dtype])


def one_short(t):
    return t.reshape(-1)[:-1]


def strided(t):
    """-> the strided form of t, or None where there is none: torch calls every tensor of one element contiguous"""
    if t.numel() <= 1:
        return None
    big = torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype, device=t.device)  # (zero: a valid value of every type in the gaps)
    v = big[..., 0]
    v.copy_(t)
    return v


DEFECTS = {'on_cpu': on_cpu, 'other_dtype': other_dtype, 'one_short': one_short}


@contextlib.contextmanager
def raises_before_the_library(what):
    """the body raises ValueError or AivcNativeError; a Reached (the argument got as far as the library) or no exception fails,
    named by `what`"""
    from aivc_amd._lib import AivcNativeError
    try:
        yield
    except Reached as r:
        raise AssertionError('%s: handed to the library (%r)' % (what, r)) from None
    except (ValueError, AivcNativeError):
        return
    raise AssertionError('%s: accepted' % what)
