"""aivc_resize_u8 / ops.resize_u8 (include/aivc_hip_resize.h) against Pillow's Image.resize, BY BYTE, on every shape of
tests/resize_cases.py under every filter; each case plain and under the guard-zone and poison harness of tests/guarded.py with
both fills: every plane between guard zones, and every buffer aivc_amd.ops allocates -- the tables, the intermediate, the result
-- an arena whose untouched payload is poison.  Integer arithmetic: no tolerance anywhere, and the three runs agree byte for byte.

A case is two calls: three planes of different content that start 0, 1 and 7 bytes into their buffers (the bytes in front hold
the guard's fill; every row of the second and third plane is off the 16-byte grid, each differently), and one plane alone, 7 bytes
in."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_cases as rc  # noqa: E402
from guarded import FILLS, both_fills, guarded  # noqa: E402

pytestmark = pytest.mark.gpu

OFFSETS = (0, 1, 7)


def place(a, off, cuda, fill):
    """the plane a as a [h, w] tensor that starts `off` bytes into its buffer"""
    buf = np.concatenate([np.full(off, FILLS[0] if fill is None else fill, np.uint8), a.reshape(-1)])
    t = (torch.from_numpy(buf).to(cuda) if fill is None else guarded(buf, cuda, fill))[off:].view(a.shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == off % 16
    return t


def run_both_ways(planes, offsets, h_out, w_out, name, cuda):
    """ops.resize_u8 on the planes, plane i starting offsets[i] bytes into its buffer: plain, then under guard_ops with both
    fills -> the plain result as a numpy array; all three must be equal bytes"""
    from aivc_amd import ops

    def call(fill):
        got = ops.resize_u8([place(a, off, cuda, fill) for a, off in zip(planes, offsets)], h_out, w_out, name)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (len(planes), h_out, w_out) and got.is_cuda and got.is_contiguous()
        return got
    plain = call(None).cpu().numpy()
    assert both_fills(call) == plain.tobytes()
    return plain


@pytest.mark.parametrize('name', rc.FILTER_NAMES)
@pytest.mark.parametrize('shape', rc.SHAPES, ids=rc.shape_id)
def test_resize_equals_pillow(shape, name, cuda):
    h_out, w_out = shape[2:4]
    planes, want = rc.planes(shape, 3), rc.pil_planes(shape, 3, name)
    got = run_both_ways(planes, OFFSETS, h_out, w_out, name, cuda)
    for i in range(3):
        assert np.array_equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()))
    alone = run_both_ways(planes[2:], OFFSETS[2:], h_out, w_out, name, cuda)
    assert np.array_equal(alone[0], want[2])


@pytest.mark.parametrize('name', ['bilinear', 'lanczos'])
def test_a_420_frame_with_odd_sides(name, cuda):
    """33 x 47 (w x h) to 21 x 29 and to 61 x 95 through func_util.img_processing.resize_frames: y to h x w, u and v to the ceil
    half size, each plane what Pillow makes of it on its own; two frames, so the u and v planes of a clip share one call"""
    from aivc_amd.func_util.img_processing import resize_frames
    rng = np.random.default_rng(7)
    w0, h0 = 33, 47
    host = [{'y': rng.integers(0, 256, (1, h0, w0), dtype=np.uint8), 'u': rng.integers(0, 256, (1, 24, 17), dtype=np.uint8),
             'v': rng.integers(0, 256, (1, 24, 17), dtype=np.uint8)} for _ in range(2)]
    for w, h in ((21, 29), (61, 95)):
        def call(fill):
            frames = [{k: place(fr[k], off, cuda, fill) for k, off in zip('yuv', OFFSETS)} for fr in host]
            return resize_frames(frames, w, h, name, cuda)
        plain = call(None)
        for got, fr in zip(plain, host):
            want = rc.pil_resize_frame(fr, w, h, name)
            assert tuple(got['y'].shape) == (1, h, w) and tuple(got['u'].shape) == (1, (h + 1) // 2, (w + 1) // 2) == tuple(got['v'].shape)
            for k in 'yuv':
                assert got[k].dtype == torch.uint8 and np.array_equal(got[k].cpu().numpy(), want[k]), k
        assert both_fills(call) == [{k: fr[k].cpu().numpy().tobytes() for k in 'yuv'} for fr in plain]
    same = resize_frames([{k: torch.from_numpy(v) for k, v in host[0].items()}], w0, h0, name, cuda)  # the size it has: no launch
    assert all(np.array_equal(same[0][k].cpu().numpy(), host[0][k]) for k in 'yuv')


def test_a_stack_and_a_list_are_one_input(cuda):
    from aivc_amd import ops
    shape = rc.SHAPES[4]
    planes = rc.planes(shape, 5)
    stack = torch.from_numpy(np.stack(planes)).to(cuda)  # plane i starts 33 * 61 * i bytes in: every alignment
    want = ops.resize_u8([torch.from_numpy(p).to(cuda) for p in planes], 17, 30, 'bicubic')
    assert torch.equal(ops.resize_u8(stack, 17, 30, 'bicubic'), want)
    assert torch.equal(ops.resize_u8([p[None] for p in stack], 17, 30, 'bicubic'), want)  # [1, h, w], as read_yuv's


def test_result_does_not_depend_on_batching(cuda):
    """7 planes in one call, and in calls of 3, 3 and 1"""
    from aivc_amd import ops
    shape = rc.SHAPES[7]
    planes = [torch.from_numpy(p).to(cuda) for p in rc.planes(shape, 7)]
    whole = ops.resize_u8(planes, 68, 120, 'lanczos')
    parts = torch.cat([ops.resize_u8(planes[s:s + 3], 68, 120, 'lanczos') for s in (0, 3, 6)])
    assert torch.equal(whole, parts)


def test_unsupported_shapes_raise(cuda):
    """what no launch can express raises with the sizes named, and nothing is computed: a tile of the horizontal pass that needs
    more input columns than it holds in LDS (the C entry: AIVC_ERR_UNSUPPORTED), and grids past their limits"""
    from aivc_amd import _lib, abi, ops
    wide = torch.zeros((1, 70000), dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError, match=r'70000 x 1 -> 7 x 1.*holds at most %d' % abi.RESIZE_MAX_SPAN):
        ops.resize_u8([wide], 1, 7, 'bilinear')
    small = torch.zeros((4, 4), dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError, match=r'4 x 4 -> 16777216 x 4'):
        ops.resize_u8([small], 4, 65536 * abi.RESIZE_TILE_W, 'box')
    with pytest.raises(ValueError, match='filter'):
        ops.resize_u8([small], 8, 8, 'nearest')
    with pytest.raises(ValueError):
        ops.resize_u8([small, torch.zeros((4, 5), dtype=torch.uint8, device=cuda)], 8, 8)
    with pytest.raises(ValueError):
        ops.resize_u8([small], 0, 8)
    # the C entry itself, with real buffers: the code, and the output keeps every byte
    fn = _lib.load()['aivc_resize_u8']
    table = torch.tensor([wide.data_ptr()], dtype=torch.int64, device=cuda)
    out = torch.full((7,), 0xA5, dtype=torch.uint8, device=cuda)
    tabs = torch.zeros(64, dtype=torch.int32, device=cuda)
    rc_ = fn(table.data_ptr(), 1, 1, 70000, 1, 7, tabs.data_ptr(), tabs.data_ptr(), 8, abi.RESIZE_MAX_SPAN + 1, None, None, None,
             out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert rc_ == abi.ERR_UNSUPPORTED and bool((out == 0xA5).all())
    # the widest tile that does fit: 4064 input columns into one output column under the box filter
    edge = rc.planes((1, abi.RESIZE_MAX_SPAN, 1, 1, 'random'), 1)[0]
    got = ops.resize_u8([torch.from_numpy(edge).to(cuda)], 1, 1, 'box')
    assert np.array_equal(got[0].cpu().numpy(), rc.pil_resize(edge, 1, 1, 'box'))
