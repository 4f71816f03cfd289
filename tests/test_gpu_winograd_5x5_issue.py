"""The issue stream of the two 5x5 Winograd forms (csrc/conv_wino.hip: which descriptor, which phase / class, which addresses a
chunk's LDS-DMAs take) at the places no other row reaches:
  * transposed form, consecutive blocks of a workgroup in DIFFERENT classes: with 4 or 8 list entries per pixel block a step of 32
    entries (32 workgroups per XCD) always lands in the same class; c_out = 192 gives 12 entries per pixel block;
  * transposed form, block entry across image borders (odd sizes: zero-page addresses recomputed under the previous block's last chunks);
  * polyphase form with 8 and 16 chunks per phase, odd input sizes, block lists of 2 * CUs + 8 and 4 * CUs + 8;
  * one block per workgroup at c_in 128 (polyphase) and c_out 192 (transposed): the only block's last chunk.
HIP == CPU oracle BIT FOR BIT, three launches in a row on the same buffers, the variant code asserted."""
import pytest
import torch

from conv_cases import fp32w, wino_blocks, wino_case, wino_three_launches  # noqa: F401 (fp32w: a fixture)

pytestmark = pytest.mark.gpu


def _owned(total, cus):
    """the kernel's block_of: the list entries of every persistent workgroup, in the order it walks them"""
    nwg = min(cus, total)
    per_xcd = (total + 7) >> 3
    out = []
    for b in range(nwg):
        xcd, slot = b & 7, b >> 3
        wg_per_xcd = (nwg + 7 - xcd) >> 3
        x_lo = xcd * per_xcd
        x_hi = min(x_lo + per_xcd, total)
        out.append(list(range(x_lo + slot, x_hi, wg_per_xcd)))
    return out


def _sized(variant, row, blocks_wanted):
    n = -(-blocks_wanted // wino_blocks(variant, row, n=1))
    return (n,) + row[1:], wino_blocks(variant, row, n=n)


def test_transposed_class_changes_between_a_workgroups_blocks(cuda, oracle, fp32w):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    row, total = _sized(303, (None, 16, 16, 32, 192, 0, 0, True, False), 2 * cus + 8)  # 12 entries per pixel block: class = (entry % 12) // 3
    changes = sum(1 for mine in _owned(total, cus) for a, b in zip(mine, mine[1:]) if (a % 12) // 3 != (b % 12) // 3)
    assert changes > 0, (cus, total)  # the shape has to hand a workgroup two blocks of different classes
    wino_three_launches(303, wino_case(oracle, 303, row, 1000), cuda)


def test_transposed_block_entry_across_image_borders(cuda, oracle, fp32w):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    row, total = _sized(303, (None, 17, 30, 64, 64, 0, 0, True, False), 2 * cus + 8)
    assert max(len(m) for m in _owned(total, cus)) >= 2
    wino_three_launches(303, wino_case(oracle, 303, row, 1001), cuda)


# c_in, multiple of the CU count in the block list
POLY = {'8-chunks': (64, 2), '16-chunks': (128, 2), '8-chunks-4x': (64, 4)}


@pytest.mark.parametrize('name', list(POLY))
def test_polyphase_many_chunks_per_phase(name, cuda, oracle, fp32w):
    c_in, mult = POLY[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # 30 x 62 inputs -> 15 x 31 outputs: the clamp into the other phase and the right-edge column
    row, total = _sized(302, (None, 30, 62, c_in, 128, 0, 0, True, False), mult * cus + 8)
    assert max(len(m) for m in _owned(total, cus)) >= mult + 1  # nxt is handed over `mult` times or more
    wino_three_launches(302, wino_case(oracle, 302, row, 1010 + list(POLY).index(name)), cuda)


SINGLE = {
    'polyphase-c_in-128': (302, (1, 32, 32, 128, 128, 0, 0, True, False)),
    'transposed-c_out-192': (303, (1, 16, 16, 32, 192, 0, 0, True, False)),
}


@pytest.mark.parametrize('name', list(SINGLE))
def test_a_workgroup_with_one_block(name, cuda, oracle, fp32w):
    variant, row = SINGLE[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert wino_blocks(variant, row) <= cus
    wino_three_launches(variant, wino_case(oracle, variant, row, 1020 + list(SINGLE).index(name)), cuda)
