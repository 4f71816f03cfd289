"""The Winograd kernels' pipeline ACROSS blocks (csrc/conv_wino.hip): no row of WINO_CASES, POLY_CASES or TC_CASES has more blocks
than the device has CUs, so there every persistent workgroup runs one block.  Here the block list is 2 * CUs + 8 long (rounded up to
whole images): workgroups own 2 and 3 blocks, unevenly over the XCDs, and the parts that only exist between two blocks run -- the
next block's patch, U image and first transform under this block's last chunk, the pair exchange through V stage 1 while V stage 0
already holds the next block's chunk 0, and the descriptor hand-over (`nxt`).  Plus one launch per form in which every workgroup's
only block is its first and its last.  HIP == CPU oracle BIT FOR BIT, three launches in a row on the same buffers."""
import pytest
import torch

from conv_cases import fp32w, wino_blocks, wino_case, wino_three_launches  # noqa: F401 (fp32w: a fixture)

pytestmark = pytest.mark.gpu


# variant, row of the form's table with n = None: the number of images comes from the device's CU count
MANY = {
    '3x3': (301, (None, 48, 64, 32, 128, 0, 0, True, False, False)),            # 12 pixel blocks x 2 channel blocks per image
    'polyphase': (302, (None, 96, 128, 32, 128, 0, 0, True, False)),            # 48 x 64 outputs: the same 24 blocks per image
    'transposed': (303, (None, 32, 32, 32, 64, 0, 0, True, False)),             # 4 pixel blocks x 4 classes per image
    '3x3-residual': (301, (None, 48, 64, 64, 128, 0, 2, True, False, True)),    # residual + relu epilogue
}
# one block per workgroup, 16 x 16 grid pixels: the only block's first chunk and its last, nothing rides along behind it
SINGLE = {
    '3x3': (301, (1, 16, 16, 32, 128, 0, 0, True, False, False)),
    'polyphase': (302, (1, 32, 32, 32, 128, 0, 0, True, False)),
    'transposed': (303, (1, 16, 16, 32, 64, 0, 0, True, False)),
}


@pytest.mark.parametrize('name', list(MANY))
def test_workgroups_walk_two_and_three_blocks(name, cuda, oracle, fp32w):
    variant, row = MANY[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_image = wino_blocks(variant, row, n=1)
    n = -(-(2 * cus + 8) // per_image)
    row = (n,) + row[1:]
    blocks = wino_blocks(variant, row)
    assert 2 * cus + 8 <= blocks < 3 * cus, (cus, blocks)  # some workgroups own 2 blocks, some 3
    wino_three_launches(variant, wino_case(oracle, variant, row, 900 + list(MANY).index(name)), cuda)


@pytest.mark.parametrize('name', list(SINGLE))
def test_a_workgroup_with_one_block(name, cuda, oracle, fp32w):
    variant, row = SINGLE[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert wino_blocks(variant, row) <= cus
    wino_three_launches(variant, wino_case(oracle, variant, row, 950 + list(SINGLE).index(name)), cuda)
