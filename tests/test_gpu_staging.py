"""ops._stage on the device: the one place small host tables are put on the device (pinned staging buffer, asynchronous copy, the
buffer back in the pool behind an event on the copy's stream).  ops._plane_batch, the one reader of a list of planes or a stack,
has its cases in the files of its three ops: list against stack, misaligned views, rejections (tests/test_gpu_digest.py,
tests/test_gpu_pair_sad.py, tests/test_gpu_resize.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 15, 16, 17]


def test_staged_arrays_sit_at_their_offsets_in_zeros(cuda):
    from aivc_amd import ops
    arrays = [np.arange(1 + 40 * i, 1 + 40 * i + n, dtype=np.uint8) for i, n in enumerate(SIZES)]  # distinct, never 0
    blob, offs = ops._stage(cuda, arrays)
    assert blob.dtype == torch.uint8 and blob.device == cuda and (offs, blob.numel()) == ops._stage_layout(SIZES)
    got = blob.cpu().numpy()
    want = np.zeros(blob.numel(), np.uint8)
    for o, a in zip(offs, arrays):
        want[o:o + a.size] = a
    assert int((want != 0).sum()) == sum(SIZES) and np.array_equal(got, want)
    # a pointer table as its bytes; the range decoder's layout (4-byte boundaries, 8 spare bytes behind each)
    words = np.array([0x0102030405060708, 2 ** 64 - 1], np.uint64)
    blob, offs = ops._stage(cuda, [words.view(np.uint8), np.array([7, 8, 9], np.uint8)], align=4, slack=8)
    assert offs == [0, 24] and blob.numel() == 36
    assert blob.cpu().numpy().tobytes() == words.tobytes() + bytes(8) + bytes([7, 8, 9]) + bytes(9)


@pytest.mark.parametrize('nbytes', [64, (1 << 20) + 16])
def test_staging_buffers_are_not_refilled_under_a_copy(cuda, nbytes):
    """three blobs of one size staged back to back with nothing between them: a pinned buffer that went back to the pool before
    its copy had finished would be refilled by the next call, and an earlier blob would hold a later one's bytes.  The second
    size is more than the pool's smallest buffer."""
    from aivc_amd import ops
    rng = np.random.default_rng(nbytes)
    host = [rng.integers(0, 256, nbytes, dtype=np.uint8) for _ in range(3)]
    blobs = [ops._stage(cuda, [a])[0] for a in host]
    torch.cuda.synchronize()
    for a, blob in zip(host, blobs):
        assert np.array_equal(blob.cpu().numpy(), a)
    # the pool afterwards: pinned buffers, one of them large enough for these, every one free again after the synchronise
    assert all(buf.is_pinned() for _, buf in ops._STAGING) and any(buf.numel() >= nbytes for _, buf in ops._STAGING)
    assert all(ev.query() for ev, _ in ops._STAGING)
