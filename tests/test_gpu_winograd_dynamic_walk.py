"""The Winograd kernels' persistent workgroups claim the entries of the block list at run time, from per-XCD ticket counters that
the last workgroup out leaves zeroed (aivc_amd/csrc/wino_dynamic_walk.h; tests/test_winograd_dynamic_walk.py runs the protocol
itself without a GPU).  Here the kernel walks the lists on which the claims can go wrong:
  * the shortest list of each form (one pixel block: 2 entries, 4 in the transposed form): a workgroup's only block is its
    first, and its one claim finds nothing;
  * lists just below, at and just above the CU count, and 2 * CUs + 8: a list is whole pixel blocks, 2 entries each (4 in the
    transposed form), so CUs - 1 and CUs + 1 do not exist and the nearest lengths that do stand for them;
  * 10 entries on 10 workgroups: the ranges of XCDs 5, 6 and 7 are empty and a workgroup sits on each of them;
  * 17 x 30 images, an odd number of them; stride-1 form 128 -> 128 and 64 -> 128; polyphase form c_in 64 on 30 x 62 outputs;
    transposed form c_out 64 / 128 / 192;
  * two streams launching different shapes at the same time (each stream has counters of its own);
  * a launch beside a workgroup of another kernel that holds 100 KB of LDS on a side stream (aivc_diag_hold_lds: a bounded loop,
    no flag, about a millisecond): a Winograd workgroup cannot start on that CU and starts late or claims nothing.
Every output starts as NaN between guard zones (guard_ops of tests/guarded.py, fill 0xFF): an entry that no workgroup claimed
stays NaN, one claimed after its time would be computed from the wrong descriptor.  HIP == CPU oracle BIT FOR BIT, three launches
in a row on one stream -- the second and third find the counters as the launch before left them.  Bits only, never a time."""
import pytest
import torch

from conv_cases import fp32w, wino_blocks, wino_case, wino_three_launches  # noqa: F401 (fp32w: a fixture)
from guarded import guard_ops
from numeric_regimes import assert_bits
from op_cases import on, profiled

pytestmark = pytest.mark.gpu

# variant -> the row of a one-pixel-block image (n = None: the number of images comes from the list length asked for)
UNIT = {
    301: (None, 16, 16, 32, 128, 0, 0, True, False, False),
    302: (None, 32, 32, 32, 128, 0, 0, True, False),
    303: (None, 16, 16, 32, 64, 0, 0, True, False),
}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _sized(variant, row, blocks_wanted, below=False, odd=False):
    """the row with as many images as make the list blocks_wanted long, or the nearest length above (below) that exists"""
    per_image = wino_blocks(variant, row, n=1)
    n = max(1, blocks_wanted // per_image if below else -(-blocks_wanted // per_image))
    n += odd and n % 2 == 0
    return (n,) + row[1:], wino_blocks(variant, row, n=n)


def _run(oracle, cuda, variant, row, seed):
    case = wino_case(oracle, variant, row, seed)
    with guard_ops(0xFF):
        wino_three_launches(variant, case, cuda)


@pytest.mark.parametrize('variant', list(UNIT))
def test_one_pixel_block(variant, cuda, oracle, fp32w):
    row, total = _sized(variant, UNIT[variant], 1)
    assert total == (4 if variant == 303 else 2)
    _run(oracle, cuda, variant, row, 1200 + variant)


# the list length against the CU count: name -> (CUs -> blocks wanted, nearest existing length below instead of above)
AROUND = {'below-CUs': (lambda c: c - 1, True), 'CUs': (lambda c: c, False), 'above-CUs': (lambda c: c + 1, False),
          'two-and-three-each': (lambda c: 2 * c + 8, False)}


@pytest.mark.parametrize('name', list(AROUND))
@pytest.mark.parametrize('variant', [301, 303])
def test_list_length_around_the_cu_count(variant, name, cuda, oracle, fp32w):
    wanted, below = AROUND[name]
    cus = _cus()
    row, total = _sized(variant, UNIT[variant], wanted(cus), below=below)
    per = 4 if variant == 303 else 2
    assert (wanted(cus) - per < total <= wanted(cus)) if below else (wanted(cus) <= total < wanted(cus) + per), (cus, total)
    _run(oracle, cuda, variant, row, 1210 + 10 * list(AROUND).index(name) + variant % 10)


def test_workgroups_on_xcds_whose_range_is_empty(cuda, oracle, fp32w):
    row, total = _sized(301, UNIT[301], 10)
    per_xcd = (total + 7) >> 3
    assert total == 10 and total <= _cus() and [x for x in range(8) if x * per_xcd >= total] == [5, 6, 7]
    _run(oracle, cuda, 301, row, 1260)


SHAPES = {  # variant, row (n = None: sized to 2 * CUs + 8 blocks), odd image count
    '17x30-odd-images-3x3': (301, (None, 17, 30, 32, 128, 0, 0, True, False, False), True),
    '17x30-odd-images-transposed': (303, (None, 17, 30, 32, 64, 0, 0, True, False), True),
    '3x3-128-to-128': (301, (None, 16, 32, 128, 128, 1, 0, True, False, True), False),
    '3x3-64-to-128': (301, (None, 16, 32, 64, 128, 0, 2, True, False, True), False),
    'polyphase-c_in-64-30x62': (302, (None, 60, 124, 64, 128, 0, 0, True, True), False),
    'transposed-c_out-64': (303, (None, 16, 32, 32, 64, 0, 0, True, True), False),
    'transposed-c_out-128': (303, (None, 16, 32, 32, 128, 0, 0, True, False), False),
    'transposed-c_out-192': (303, (None, 16, 32, 32, 192, 0, 0, True, False), False),
}


@pytest.mark.parametrize('name', list(SHAPES))
def test_forms_and_shapes_on_two_and_three_blocks_per_workgroup(name, cuda, oracle, fp32w):
    variant, row, odd = SHAPES[name]
    cus = _cus()
    row, total = _sized(variant, row, 2 * cus + 8, odd=odd)
    assert total >= 2 * cus + 8 and (not odd or row[0] % 2 == 1), (cus, total, row)
    _run(oracle, cuda, variant, row, 1270 + list(SHAPES).index(name))


def test_two_streams_launch_different_shapes_at_the_same_time(cuda, oracle, fp32w):
    from aivc_amd import ops
    cus = _cus()
    row_a, _ = _sized(301, (None, 16, 32, 32, 128, 0, 0, True, False, False), 2 * cus + 8)
    row_b, _ = _sized(303, (None, 16, 16, 32, 64, 0, 0, True, False), 3 * cus + 4)
    cases = [(301, wino_case(oracle, 301, row_a, 1290)), (303, wino_case(oracle, 303, row_b, 1291))]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with guard_ops(0xFF):
        placed = [c.place(on(cuda)) for _, c in cases]
        torch.cuda.synchronize()

        def launches():
            out = [[], []]
            for _ in range(3):  # launch by launch in turn: the two streams' kernels meet on the device
                for k, (_, c) in enumerate(cases):
                    with torch.cuda.stream(streams[k]):
                        out[k].append(c.call(ops, placed[k]))
            return out
        got, variants = profiled(launches)
        assert variants == [301, 303] * 3, variants
        for k, (_, c) in enumerate(cases):
            for launch, y in enumerate(got[k]):
                assert_bits(y.cpu().numpy(), c.want, 'stream %d launch %d' % (k, launch))


def test_beside_a_workgroup_that_holds_lds(cuda, oracle, fp32w):
    from aivc_amd import ops
    row, _ = _sized(302, (None, 32, 32, 32, 128, 0, 0, True, False), 2 * _cus() + 8)
    case = wino_case(oracle, 302, row, 1295)
    side = torch.cuda.Stream()
    with guard_ops(0xFF):
        d = case.place(on(cuda))
        torch.cuda.synchronize()
        for launch in range(3):
            with torch.cuda.stream(side):
                held = ops.diag_hold_lds(100 * 1024, 20000)  # 1.3 ms at 67 ns per iteration; the launch below takes a fraction of that
            got, variants = profiled(lambda: case.call(ops, d))
            assert variants == [302], (launch, variants)
            assert_bits(got.cpu().numpy(), case.want, 'launch %d' % launch)
            assert int(held.max()) < 100 * 1024 // 4 and int(held.min()) >= 0
