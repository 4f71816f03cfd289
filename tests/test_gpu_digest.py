"""aivc_md5_batch / ops.md5_planes (include/aivc_hip_digest.h) against hashlib on seeded random bytes, plain and under the
guard-zone and poison harness of tests/guarded.py (every input between guard zones, every output and the pointer table of
aivc_amd.ops allocated between them, each case under both fills: the kernel reads whole aligned 16-byte chunks, so bytes of a
guard zone do enter its registers next to a message's first and last bytes, and must not reach a digest).

Each case is stated once (CASES) and runs plain and guarded.
  lengths  the padding boundaries of RFC 1321, where implementations go wrong: the 0x80 byte and the bit count fit the last data
           block up to 55 bytes, need a block of their own from 56 on; 63 / 64 / 65 and 127 / 128 / 129 around a full block;
           119 / 120 / 121 the same boundary one block later; 561 and 4097 walk the three-slot chunk ring more than once
           (9 and 65 blocks) with a one-byte tail; 0 is the empty string and reads nothing.
  counts   1, a wavefront less one, a full one, one more (two workgroups, the second with one lane), 130 (three).
  offsets  the messages are rows of ONE buffer starting 0 .. 3 bytes into an allocation: row i starts at offset + i * length, so
           with an odd length the lanes of a wavefront have every shift 0 .. 15 at once, with length % 16 == 0 and offset 0 all
           are aligned (the kernel's branch without the byte funnel)."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import both_fills, guard_ops, guarded  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 3, 55, 56, 57, 63, 64, 65, 119, 120, 121, 127, 128, 129, 561, 4097]
COUNTS = [1, 63, 64, 65, 130]
OFFSETS = [0, 1, 2, 3]


def message_bytes(length, count, offset):
    """`offset` bytes of lead, then `count` messages of `length` bytes back to back, seeded by the case"""
    rng = np.random.default_rng(1000003 * length + 1009 * count + offset)
    return rng.integers(0, 256, offset + count * length, dtype=np.uint8)


def expected(flat, length, count, offset):
    return b''.join(hashlib.md5(flat[offset + i * length:offset + (i + 1) * length].tobytes()).digest() for i in range(count))


def run_case(flat, length, count, offset, dev, fill=None):
    """the stacked form: a contiguous [count, length] view `offset` bytes into the buffer"""
    from aivc_amd import ops
    buf = torch.from_numpy(flat).to(dev) if fill is None else guarded(flat, dev, fill)
    stack = buf[offset:].view(count, length)
    assert stack.is_contiguous() and (length == 0 or stack.data_ptr() % 4 == offset)
    out = ops.md5_planes(stack)
    assert out.shape == (count, 16) and out.dtype == torch.uint8 and out.is_cuda
    return out


@pytest.mark.parametrize('length', LENGTHS)
def test_md5_against_hashlib(cuda, length):
    for count in COUNTS:
        for offset in OFFSETS:
            flat = message_bytes(length, count, offset)
            got = run_case(flat, length, count, offset, cuda).cpu().numpy().tobytes()
            assert got == expected(flat, length, count, offset), (length, count, offset)


@pytest.mark.parametrize('length', LENGTHS)
def test_md5_between_guard_zones(cuda, length):
    for count in COUNTS:
        for offset in OFFSETS:
            flat = message_bytes(length, count, offset)
            got = both_fills(lambda fill: run_case(flat, length, count, offset, cuda, fill))
            assert got == expected(flat, length, count, offset), (length, count, offset)


def test_md5_hex_is_hashlib_hexdigest(cuda):
    from aivc_amd import ops
    msg = np.frombuffer(b'The quick brown fox jumps over the lazy dog', np.uint8)
    out = ops.md5_planes(torch.from_numpy(msg.copy()).to(cuda).view(1, -1))
    assert bytes(out[0].cpu().numpy()).hex() == '9e107d9d372bb6826bd81d3542a419d6' == hashlib.md5(msg.tobytes()).hexdigest()
    assert bytes(ops.md5_planes(torch.empty((1, 0), dtype=torch.uint8, device=cuda))[0].cpu().numpy()).hex() \
        == 'd41d8cd98f00b204e9800998ecf8427e'


@pytest.mark.parametrize('n,h,w', [(5, 7, 9), (65, 16, 24), (3, 270, 480)])
def test_md5_of_a_plane_stack_and_of_separate_tensors(cuda, n, h, w):
    """[n, h, w] as one stack and as a list: separate allocations, and views into a stack of frames in which the planes of one
    kind are NOT back to back (the decoder's frames: y, u, v of a frame follow each other).  (3, 270, 480) is 2025 blocks per
    lane; its size is a multiple of 16 and the allocation is aligned, the kernel's aligned branch."""
    from aivc_amd import ops
    rng = np.random.default_rng(n * h * w)
    a = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    want = b''.join(hashlib.md5(a[i].tobytes()).digest() for i in range(n))

    def stacked(fill):
        return ops.md5_planes(guarded(a, cuda, fill))

    def separate(fill):
        return ops.md5_planes([guarded(a[i], cuda, fill) for i in range(n)])

    def interleaved(fill):
        frames = guarded(np.concatenate([a.reshape(n, -1), np.zeros((n, 5), np.uint8)], axis=1), cuda, fill)  # 5 bytes between
        planes = [frames[i, :h * w].view(1, h, w) for i in range(n)]
        assert all(p.is_contiguous() for p in planes)
        return ops.md5_planes(planes)
    for case in (stacked, separate, interleaved):
        assert both_fills(case) == want, case.__name__
    assert ops.md5_planes(torch.from_numpy(a).to(cuda)).cpu().numpy().tobytes() == want


def test_md5_of_nothing(cuda):
    from aivc_amd import ops
    for planes in (torch.empty((0, 4, 4), dtype=torch.uint8, device=cuda), []):
        out = ops.md5_planes(planes)
        assert out.shape == (0, 16) and out.is_cuda


def test_md5_unaligned_digest_pointer(cuda):
    """the C entry with an output that is not 16-byte aligned (ops.md5_planes always hands it an aligned one): byte stores"""
    from aivc_amd import _lib
    flat = message_bytes(129, 65, 0)
    with guard_ops(0xA5):
        msgs = guarded(flat, cuda, 0xA5)
        out = guarded(np.full(3 + 65 * 16, 0xA5, np.uint8), cuda, 0xA5)
        table = torch.tensor([msgs.data_ptr() + 129 * i for i in range(65)], dtype=torch.int64).to(cuda)
        _lib.call('aivc_md5_batch', table.data_ptr(), 129, 65, out.data_ptr() + 3, None)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
    assert got[3:].tobytes() == expected(flat, 129, 65, 0) and (got[:3] == 0xA5).all()


def test_md5_argument_errors(cuda):
    from aivc_amd import _lib, ops
    from aivc_amd._lib import AivcNativeError
    md5_batch = _lib.load()['aivc_md5_batch']
    msgs = torch.zeros(64, dtype=torch.uint8, device=cuda)
    table = torch.tensor([msgs.data_ptr()], dtype=torch.int64).to(cuda)
    out = torch.zeros(16, dtype=torch.uint8, device=cuda)
    assert md5_batch(table.data_ptr(), 64, 0, out.data_ptr(), None) == 0  # n == 0: nothing
    assert md5_batch(None, 64, 0, None, None) == 0
    assert md5_batch(table.data_ptr(), 64, -1, out.data_ptr(), None) == -1
    assert md5_batch(None, 64, 1, out.data_ptr(), None) == -1
    assert md5_batch(table.data_ptr(), 64, 1, None, None) == -1
    assert md5_batch(table.data_ptr(), -1, 1, out.data_ptr(), None) == -1
    assert md5_batch(table.data_ptr(), 1 << 31, 1, out.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert int(out.sum()) == 0  # none of them wrote
    with pytest.raises(AivcNativeError):
        ops.md5_planes(torch.zeros(2, 8, dtype=torch.uint8))  # CPU tensors are rejected like everywhere in ops
    with pytest.raises(AivcNativeError):
        ops.md5_planes(torch.zeros(2, 8, dtype=torch.float32, device=cuda))
    with pytest.raises(ValueError):
        ops.md5_planes([torch.zeros(8, dtype=torch.uint8, device=cuda), torch.zeros(9, dtype=torch.uint8, device=cuda)])
