"""Every wrapper of aivc_amd/ops.py issues ALL its work on torch's current stream: each entry of tests/test_gpu_ops_arguments.py runs
once on a side stream behind a delay, on buffers that hold a DECOY until a copy behind that delay puts the real inputs there.

  1. the case and its decoy (the same call on other values: every leaf the real leaf's shape and dtype, other content -- a valid
     input, so no kernel ever sees bytes that are not one) are placed on the device; torch.cuda.synchronize()
  2. on `side`: ops.diag_hold_lds(1024, ITERATIONS), an event `done` behind it, copy_ of the real inputs over the decoy's buffers,
     then the case's call under the forwarding recorder with probe = done.query
  3. after side.synchronize(): the result is the case's want by its own compare, and every native call was issued while the delay
     was still running (its probe value False).  A call issued after the delay ended proves nothing and FAILS the case.

A launch (or a staged table's copy) that went to any other stream does not wait for the delay: it reads the decoy and gives the
decoy's result, or it reads an output that is not written yet.  Nothing here waits for the host (several wrappers synchronise: a
gate the host opens would deadlock them), and no launch reads anything but a valid input.

FIRST_CALL_ONLY: the wrappers that read back in the middle; the requirement covers their calls up to the first host
synchronisation.  PREPARED: conv2d derives a transformed copy of a weight once per tensor and version, between two device-wide
waits (ops._derived_weights: the codec's side streams read it too); the case prepares it by a plain call first, and its weight leaf
holds the real weights from the start -- the copy would bump the tensor's version and the wait would end the delay.

Read before run (the wrappers that stage a pointer table: the _plane_batch users md5_planes / pair_sad_u8 / resize_u8, raw video,
inflate, png_unfilter, png_encode, frame_maps_to_device): each table goes through ops._stage, whose copy_ is issued on the current
stream and whose event is recorded on torch.cuda.current_stream(); each launch passes ops._stream(), the same stream.

ITERATIONS = 600000.  Measured on the MI355X over all entries and the further cases (copies included in the issue time):
  the delay, between its two events: 39.26 ... 39.46 ms (65.6 ns per iteration; 19.66 ... 20.23 ms at 300000), under the 50 ms asked for
  the longest issue time: 12.85 ms, range_encode forked over two fresh HIP streams (12.25 ms in another run); every other case
  0.03 ... 0.43 ms -- the delay is 3 times the longest and 90 times the next
  (the four FIRST_CALL_ONLY wrappers and the range_encode entry, which reads its bytes back, return after the delay: 39.3 ... 40.2 ms)
"""
import hashlib
import time

import numpy as np
import pytest
import torch

import bridge
import op_cases as oc
import test_gpu_ops_arguments as args
from aivc_amd import abi
from op_cases import on

pytestmark = pytest.mark.gpu

ITERATIONS = 600000
DELAY_MAX_MS = 50.0

FIRST_CALL_ONLY = {
    'png_encode': 'reads the segments\' lengths back before it gathers',
    'inflate': 'one launch, then the status rows come back',
    'png_unfilter': 'one launch, then the status words come back',
    'selfcheck_gdn_math': 'one launch, then the two counts come back',
}
PREPARED = {nm: 'w' for nm in ('conv2d-wino-301', 'conv2d-wino-302', 'conv2d-wino-303', 'conv2d-bf16x3', 'conv2d-slab')}


def _pairs(a, b, out):
    """the tensors of two placed input structures, leaf by leaf"""
    if a is None:
        assert b is None
    elif isinstance(a, dict):
        for k in a:
            _pairs(a[k], b[k], out)
    elif isinstance(a, (list, tuple)):
        for x, y in zip(a, b):
            _pairs(x, y, out)
    else:
        out.append((a, b))
    return out


def behind_a_delay(cuda, bufs, real, call, skip=()):
    """steps 2 and 3 of the module's docstring -> (result, [(native call, whether the delay had ended)], issue ms, delay ms)"""
    from aivc_amd import ops
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        t0, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        ops.diag_hold_lds(1024, ITERATIONS)
        done.record()
        host0 = time.perf_counter()
        for i, (dst, src) in enumerate(_pairs(bufs, real, [])):
            if i not in skip:
                dst.copy_(src)
        with bridge.recording(ops, forward=True, probe=done.query) as rec:
            got = call(ops, bufs)
        issue_ms = (time.perf_counter() - host0) * 1e3
    side.synchronize()
    return got, rec.calls, issue_ms, t0.elapsed_time(done)


def check_calls(name, calls, issue_ms, delay_ms, first_only=False):
    print('%s: %d native calls, issued in %.3f ms, delay %.3f ms' % (name, len(calls), issue_ms, delay_ms))
    assert calls, '%s: no native call' % name
    assert delay_ms < DELAY_MAX_MS, '%s: the delay took %.1f ms' % (name, delay_ms)
    late = [nm for nm, ended in (calls[:1] if first_only else calls) if ended is not False]
    assert not late, '%s: issued after the delay had ended (this proves nothing): %s' % (name, late)


@pytest.mark.parametrize('entry', args.ENTRIES, ids=[e.name for e in args.ENTRIES])
def test_every_launch_waits_for_the_stream(entry, cuda, oracle, golden):
    from aivc_amd import ops
    with args.contract_of(entry, oracle):
        case, decoy = entry.build(oracle, golden, False), entry.build(oracle, golden, True)
        la, lb = bridge.leaves(case.inputs), bridge.leaves(decoy.inputs)
        assert [(nm, a.shape, a.dtype) for nm, a in la] == [(nm, b.shape, b.dtype) for nm, b in lb]
        for (nm, a), (_, b) in zip(la, lb):  # (an output's content is a fill: the same either way)
            assert nm in entry.outputs or not np.array_equal(a, b), '%s: the decoy\'s %s is the real one' % (entry.name, nm)
        names = [nm for nm, _ in la]
        real, skip, want = case.place(on(cuda)), (), case.want
        if entry.name in PREPARED:
            k = names.index(PREPARED[entry.name])
            bufs = decoy.place(bridge.Target(on(cuda), k, lambda t: _pairs(real, real, [])[k][0]))
            skip = (k,)
            plain = case.call(ops, real)  # (derives the weights, device-wide waits included)
            if want is None:  # the precision mode has no oracle: the plain call's bits
                want, case.compare = plain, lambda got, w: args.same_bits(got, w, entry.name)
        else:
            bufs = decoy.place(on(cuda))
        got, calls, issue_ms, delay_ms = behind_a_delay(cuda, bufs, real, case.call, skip)
        case.compare(got, want)
        check_calls(entry.name, calls, issue_ms, delay_ms, first_only=entry.name in FIRST_CALL_ONLY)


def test_range_encode_forks_behind_the_stream_and_joins_it(cuda, oracle):
    """more streams than one launch takes, forked over two HIP streams from the side stream: both launches wait for the fork's
    event, which lies behind the delay and the copies; the join makes the side stream wait for both"""
    lens = [5 + i % 13 for i in range(abi.RC_MAX_STREAMS + 6)]
    case, decoy = (oc.range_encode_case(oracle, seed, lens, 0, 2, False) for seed in (7, 8))
    assert all(a.shape == b.shape and not np.array_equal(a, b) for a, b in zip(case.inputs['streams'], decoy.inputs['streams']))
    forks = [torch.cuda.Stream(), torch.cuda.Stream()]
    got, calls, issue_ms, delay_ms = behind_a_delay(cuda, decoy.place(on(cuda)), case.place(on(cuda)),
                                                    lambda ops, d: ops.range_encode(d['streams'], streams=forks))
    case.check(got)  # (stream_bytes copies on the side stream's successor: torch's default stream after side.synchronize())
    assert [nm for nm, _ in calls] == ['aivc_range_encode'] * 2
    check_calls('range_encode, forked', calls, issue_ms, delay_ms)


def test_two_staged_tables_in_a_row_keep_their_buffers(cuda):
    """md5_planes twice on the side stream: the first table's pinned buffer goes back to the pool behind an event of THAT stream,
    which has not completed while the delay runs, so the second call must not be handed the same buffer (it would overwrite the
    first table before its copy has read it)"""
    rng = np.random.default_rng(5)
    first, second, decoy_a, decoy_b = ([rng.integers(0, 256, 65 + 7 * k, dtype=np.uint8) for _ in range(3)] for k in (0, 1, 0, 1))

    def call(ops, d):
        return ops.md5_planes(d['a']), ops.md5_planes(d['b'])
    got, calls, issue_ms, delay_ms = behind_a_delay(cuda, oc.place_all({'a': decoy_a, 'b': decoy_b}, on(cuda)),
                                                    oc.place_all({'a': first, 'b': second}, on(cuda)), call)
    for g, planes in zip(got, (first, second)):
        assert [bytes(row).hex() for row in g.cpu().numpy()] == [hashlib.md5(p.tobytes()).hexdigest() for p in planes]
    assert [nm for nm, _ in calls] == ['aivc_md5_batch'] * 2
    check_calls('md5_planes twice', calls, issue_ms, delay_ms)
