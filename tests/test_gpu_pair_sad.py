"""aivc_pair_sad_u8 / ops.pair_sad_u8 (include/aivc_hip_scene.h) against numpy, each case plain and under the guard-zone and
poison harness of tests/guarded.py with both fills: every plane between guard zones, and every buffer aivc_amd.ops allocates --
the pointer table, the partial sums, the result -- an arena whose untouched payload is poison.  Integer arithmetic: the sums
must EQUAL np.abs(a.astype(np.int64) - b).sum(), and the three runs must agree byte for byte.

Sizes.  A workgroup's stripe is 256 chunks of 16 bytes = 4096 bytes, the 128 workgroups of a pair cover 524288 bytes per pass,
a thread has four passes in flight, so a round of the loop covers 2097152 bytes:
  1, 15, 16, 17, 63, 64, 65             less than a chunk, one chunk, heads and tails around it
  4095, 4096, 4097                      one stripe: the second workgroup gets nothing, one chunk, one byte
  524287, 524288, 524304, 524289        one pass: the second unrolled load of thread 0 gets nothing / its first chunk
  2097152 + 16 + 5                      the loop's second round, with a tail
  2^24 + 17, all 0 against all 255      255 x (2^24 + 17) > 2^31; with 2^17 bytes more > 2^32: the 64-bit totals
Planes start `offset` bytes into their buffers, the bytes in front hold the guard's fill: offsets 0 ... 15, different inside
one table (a pair then reads its second plane through the byte funnel), one table with a single misaligned plane (the pairs
around it take the funnel, the others the aligned path), and tables with one offset for all (heads, but the aligned path)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import FILLS, both_fills, guarded  # noqa: E402
from scene_cases import pair_sad_numpy  # noqa: E402

pytestmark = pytest.mark.gpu


def make(rng, n, length, kind='random'):
    if kind == 'random':
        return [rng.integers(0, 256, length, dtype=np.uint8) for _ in range(n)]
    return [np.full(length, (0, 255)[(i + (kind == '255-0')) % 2], np.uint8) for i in range(n)]  # '0-255' / '255-0', alternating


def run_both_ways(planes, offsets, cuda):
    """ops.pair_sad_u8 on the planes, plane i starting offsets[i] bytes into its buffer: plain, then under guard_ops with both
    fills -> the plain result as a numpy array; all three must be equal bytes"""
    from aivc_amd import ops

    def call(fill):
        placed = []
        for a, off in zip(planes, offsets):
            buf = np.concatenate([np.full(off, FILLS[0] if fill is None else fill, np.uint8), a])
            t = (torch.from_numpy(buf).to(cuda) if fill is None else guarded(buf, cuda, fill))[off:]
            assert t.is_contiguous() and t.data_ptr() % 16 == off % 16 and t.numel() == a.size
            placed.append(t)
        got = ops.pair_sad_u8(placed)
        assert got.dtype == torch.int64 and tuple(got.shape) == (max(len(planes) - 1, 0),) and got.is_cuda
        return got
    plain = call(None).cpu().numpy()
    assert both_fills(call) == plain.tobytes()
    return plain


LENGTHS = [1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 524287, 524288, 524289, 524304, 2097152 + 21]


@pytest.mark.parametrize('length', LENGTHS)
def test_pair_sad_lengths(length, cuda):
    """three planes, aligned / 5 bytes in / 5 bytes in: the first pair takes the funnel, the second the shared-alignment path"""
    rng = np.random.default_rng(length)
    planes = make(rng, 3, length)
    want = pair_sad_numpy(planes)
    for offsets in ((0, 0, 0), (0, 5, 5)):
        got = run_both_ways(planes, offsets, cuda)
        assert got.tolist() == want, (offsets, got.tolist(), want)


@pytest.mark.parametrize('n', [1, 2, 3, 70])
def test_pair_sad_plane_counts(n, cuda):
    rng = np.random.default_rng(n)
    planes = make(rng, n, 1024)
    got = run_both_ways(planes, [0] * n, cuda)
    assert got.tolist() == pair_sad_numpy(planes) and len(got) == max(n - 1, 0)


@pytest.mark.parametrize('length', [200, 4096 + 33])
def test_pair_sad_every_offset(length, cuda):
    """17 planes at the offsets 0, 1, ..., 15, 0: every shift of the funnel 1 ... 15 between neighbours (offset i + 1 against i is
    shift 1 whatever the head; so a second table pairs offset 0 with every other one in turn)"""
    rng = np.random.default_rng(length + 1)
    planes = make(rng, 17, length)
    want = pair_sad_numpy(planes)
    assert run_both_ways(planes, list(range(16)) + [0], cuda).tolist() == want
    zig = [(k // 2 + 1) % 16 if k % 2 else 0 for k in range(17)]  # 0, 1, 0, 2, 0, 3, ...: shifts 1 ... 8 and 16 - them
    assert sorted(set(zig)) == list(range(9))
    assert run_both_ways(planes, zig, cuda).tolist() == want
    zag = [0 if k % 2 else 8 + k // 2 for k in range(17)]  # 8, 0, 9, 0, ..., 15, 0, 16 = aligned again
    assert run_both_ways(planes, zag, cuda).tolist() == want
    assert run_both_ways(planes, [7] * 17, cuda).tolist() == want  # one alignment for all: heads, no funnel


def test_pair_sad_one_misaligned_plane(cuda):
    """five planes, only the third off the 16-byte grid: pairs 0 and 3 run the aligned path, pairs 1 and 2 the funnel"""
    rng = np.random.default_rng(99)
    planes = make(rng, 5, 4096 * 3 + 7)
    want = pair_sad_numpy(planes)
    for off in (1, 3, 4, 9, 15):
        assert run_both_ways(planes, [0, 0, off, 0, 0], cuda).tolist() == want


@pytest.mark.parametrize('kind', ['0-255', '255-0'])
def test_pair_sad_extremes(kind, cuda):
    planes = make(None, 3, 5000, kind)
    for offsets in ((0, 0, 0), (3, 0, 11)):
        got = run_both_ways(planes, offsets, cuda)
        assert got.tolist() == [255 * 5000] * 2
    same = [planes[0], planes[0].copy()]
    assert run_both_ways(same, (0, 6), cuda).tolist() == [0]


@pytest.mark.parametrize('length', [(1 << 24) + 17, (1 << 24) + (1 << 17) + 17])
def test_pair_sad_totals_are_64_bit(length, cuda):
    """all 0 against all 255.  2^24 + 17 bytes: 4 278 194 415, past 2^31 (a signed 32-bit total is negative) and 16.8 million
    short of 2^32; 2^24 + 2^17 + 17 bytes: 4 311 617 775, past 2^32 (an unsigned 32-bit total wraps)"""
    planes = make(None, 2, length, '0-255')
    want = 255 * length
    assert want > 1 << 31 and (want > 1 << 32) == (length > (1 << 24) + 17)
    for offsets in ((0, 0), (0, 13)):
        assert run_both_ways(planes, offsets, cuda).tolist() == [want]


def test_pair_sad_does_not_depend_on_batching(cuda):
    from aivc_amd import ops
    rng = np.random.default_rng(4)
    planes = [torch.from_numpy(a).to(cuda) for a in make(rng, 9, 33 * 47)]
    whole = ops.pair_sad_u8(planes)
    parts = torch.cat([ops.pair_sad_u8(planes[s:s + 3]) for s in (0, 2, 4, 6)])
    assert torch.equal(whole, parts)
    stack = torch.stack(planes)  # views into one stack: plane i starts 1551 i bytes in, every alignment
    assert torch.equal(ops.pair_sad_u8(list(stack)), whole)


def test_nothing_is_written_for_fewer_than_two_planes(cuda):
    """the C entry with n = 0 and n = 1: AIVC_OK, and scratch and output keep every byte"""
    from aivc_amd import _lib, ops
    fn = _lib.load()['aivc_pair_sad_u8']
    plane = torch.zeros(64, dtype=torch.uint8, device=cuda)
    table = torch.tensor([plane.data_ptr()], dtype=torch.int64, device=cuda)
    for fill in FILLS:
        partials = guarded(np.full(256, fill, np.uint8), cuda, fill)
        sad = guarded(np.full(64, fill, np.uint8), cuda, fill)
        for n in (0, 1):
            assert fn(table.data_ptr(), n, 64, partials.data_ptr(), sad.data_ptr(), ops._stream()) == 0
        torch.cuda.synchronize()
        assert bool((partials == fill).all()) and bool((sad == fill).all())
        from guarded import check_guards
        check_guards(partials, sad)
    assert ops.pair_sad_u8([plane]).numel() == 0 and ops.pair_sad_u8([]).numel() == 0


def test_pair_sad_rejections(cuda):
    from aivc_amd import ops
    from aivc_amd._lib import AivcNativeError
    a = torch.zeros(8, dtype=torch.uint8, device=cuda)
    with pytest.raises(AivcNativeError):
        ops.pair_sad_u8([a, torch.zeros(8, dtype=torch.uint8)])  # CPU tensors are rejected like everywhere in ops
    with pytest.raises(AivcNativeError):
        ops.pair_sad_u8([a, torch.zeros(8, dtype=torch.float32, device=cuda)])
    with pytest.raises(ValueError):
        ops.pair_sad_u8([a, torch.zeros(9, dtype=torch.uint8, device=cuda)])
    with pytest.raises(ValueError):
        ops.pair_sad_u8(torch.zeros(2, 8, dtype=torch.uint8, device=cuda))
