"""The transposed Winograd form deals the (class, channel block) pairs of a pixel block round among the workgroups
(aivc_amd/csrc/wino_class_walk.h; tests/test_winograd_class_walk.py checks the mapping itself without a GPU).  Here the kernel
walks lists on which that mapping does everything it can do:
  * c_out 64 (4 entries per pixel block), 4 * CUs + 8 blocks: a workgroup hands over through all four classes and starts over;
  * c_out 128 (8 entries), 8 * CUs + 8 blocks: the rotation runs over class x channel block;
  * c_out 192 (12 entries, no divisor of the 32 workgroups of an XCD): the rotation on top of the walk's own drift;
  * 17 x 30 inputs (2 x 2 pixel blocks with right and bottom edges) and an odd image count: an XCD's share of the list is no
    multiple of 4, a pixel block's entries lie in two XCDs' ranges;
  * fewer blocks than CUs, down to a single pixel block: every workgroup's only block.
Every output tensor starts as NaN (guard_ops of tests/guarded.py, fill 0xFF, which also checks the guard zones around every
buffer of the launch): a (pixel block, class, channel block) that no workgroup computed stays NaN.  HIP == CPU oracle BIT FOR BIT,
three launches in a row on the same buffers, the variant code asserted."""
import math

import pytest
import torch

from conv_cases import fp32w, wino_blocks, wino_case, wino_three_launches  # noqa: F401 (fp32w: a fixture)
from guarded import guard_ops

pytestmark = pytest.mark.gpu


def _walks(total, gyc, cus):
    """the kernel's block walk and its reading of an entry: per persistent workgroup the (pixel block, cb) pairs in walking order"""
    nwg = min(cus, total)
    per_xcd = (total + 7) >> 3

    def entry(e):
        pb = e // gyc
        w = (nwg + 7 - pb * gyc // per_xcd) >> 3
        q = w // math.gcd(w, gyc) if w else 1
        return pb, (e % gyc + pb // q) % gyc
    out = []
    for b in range(nwg):
        xcd, slot = b & 7, b >> 3
        x_lo = xcd * per_xcd
        out.append([entry(e) for e in range(x_lo + slot, min(x_lo + per_xcd, total), (nwg + 7 - xcd) >> 3)])
    return out


def _sized(row, blocks_wanted, odd=False):
    n = -(-blocks_wanted // wino_blocks(303, row, n=1))
    n += odd and n % 2 == 0
    return (n,) + row[1:], wino_blocks(303, row, n=n)


def _run(oracle, cuda, row, seed):
    case = wino_case(oracle, 303, row, seed)
    with guard_ops(0xFF):
        wino_three_launches(303, case, cuda)


# c_out, multiple of the CU count in the block list
MANY = {'c_out-64': (64, 4), 'c_out-128': (128, 8), 'c_out-192': (192, 4)}


@pytest.mark.parametrize('name', list(MANY))
def test_a_workgroup_hands_over_through_the_classes(name, cuda, oracle, fp32w):
    c_out, mult = MANY[name]
    gyc = c_out // 16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    row, total = _sized((None, 16, 16, 32, c_out, 0, 0, True, False), mult * cus + 8)
    walks = _walks(total, gyc, cus)
    assert sorted(p for w in walks for p in w) == [(pb, cb) for pb in range(total // gyc) for cb in range(gyc)]
    longest = max(walks, key=len)
    classes = [cb // (gyc // 4) for _, cb in longest]
    assert len(set(classes)) >= 3, (cus, total, classes)  # the shape has to hand a workgroup blocks of different classes
    if cus % (8 * gyc) == 0:  # the walk's stride is a multiple of gyc: cb advances by one per block, through every class, and starts over
        assert len(longest) > gyc and all((b - a) % gyc == 1 for (_, a), (_, b) in zip(longest, longest[1:])), (cus, longest)
    _run(oracle, cuda, row, 1100 + list(MANY).index(name))


def test_pixel_blocks_across_xcd_ranges_and_image_borders(cuda, oracle, fp32w):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    row, total = _sized((None, 17, 30, 32, 64, 0, 0, True, False), 2 * cus + 8, odd=True)
    assert ((total + 7) >> 3) % 4 != 0 and max(len(w) for w in _walks(total, 4, cus)) >= 2, (cus, total)
    _run(oracle, cuda, row, 1110)


FEW = {'one-pixel-block-c_out-64': (1, 16, 16, 64), 'one-pixel-block-c_out-192': (1, 16, 16, 192), 'twelve-pixel-blocks': (3, 17, 30, 64)}


@pytest.mark.parametrize('name', list(FEW))
def test_fewer_blocks_than_workgroups(name, cuda, oracle, fp32w):
    n, h, w, c_out = FEW[name]
    row = (n, h, w, 32, c_out, 0, 0, True, False)
    assert wino_blocks(303, row) <= torch.cuda.get_device_properties(0).multi_processor_count
    _run(oracle, cuda, row, 1120 + list(FEW).index(name))
