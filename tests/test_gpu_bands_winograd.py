"""Row bands (aivc_amd/bands.py) in the DEFAULT arithmetic contract (version 2, Winograd F(2x2, 3x3) chains): one frame's
transforms over R ranks reproduce the single-rank frame bit for bit -- finalized bytes and reconstructed planes, encoder
and decoder -- because every slab starts on the frame's tile grid and every slab launch is routed by the size of the map
it was cut from (ops.slab_contract).  Thread ranks on the one GPU (bands.ThreadComm), real gloo processes, and bench.py's
multi-rank flow with bands switched on.  Nothing here switches to version 1 (tests/test_gpu_bands.py does)."""
import json
import os
import socket
import subprocess
import sys
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINO = (301, 302, 303)


def _run_ranks(R, fn):
    """fn(bands_ctx) in R threads -> list of results (exceptions re-raised)"""
    from aivc_amd.bands import BandCtx, ThreadComm
    shared = ThreadComm.Shared(R)
    out, err = [None] * R, []

    def work(r):
        try:
            with torch.no_grad():
                out[r] = fn(BandCtx(ThreadComm(shared, r), torch.device('cuda:0')))
        except BaseException as e:  # noqa: BLE001 -- a dead rank must not leave the others at the barrier
            err.append(e)
            shared.barrier.abort()
    ts = [threading.Thread(target=work, args=(r,)) for r in range(R)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if err:
        raise next((e for e in err if not isinstance(e, threading.BrokenBarrierError)), err[0])
    return out


class _Launches:
    """records (layer key, variant code) of every aivc_conv2d launch while active: the key is the layer's shape without
    its row count (mode, ksize, stride, real input channels, output channels, width, fused gdn, tail channels)"""

    def __init__(self, monkeypatch):
        from aivc_amd import ops
        self.on, self.seen = False, []
        inner = ops._profiled

        def profiled(launch, variant, mode, k, stride, c_real, co, n, h, w, ho, wo, fused_gdn=False, co2=0):
            if self.on:
                self.seen.append(((mode, k, stride, c_real, co, w, fused_gdn, co2), variant))
            return inner(launch, variant, mode, k, stride, c_real, co, n, h, w, ho, wo, fused_gdn, co2)
        monkeypatch.setattr(ops, '_profiled', profiled)

    def take(self):
        s, self.seen = self.seen, []
        return s


def _family(launches):
    """{layer key: set of Winograd codes, or 'tap' for any kernel of the tap chain}"""
    out = {}
    for key, v in launches:
        out.setdefault(key, set()).add(v if v in WINO else 'tap')
    return out


def _check(model, frames, R, cuda, rec):
    """I, P, B frames (cur = 1, prev = 0, next = 2): banded over R ranks == one rank, encoder and decoder.
    -> (Winograd codes taken on slabs, per frame type {layer key: families} of the single rank and of the bands)"""
    from aivc_amd.codec import FrameCodec
    from aivc_amd.func_util.GOP_structure import FRAME_B, FRAME_I, FRAME_P
    from aivc_amd.real_life.bitstream import finalize_frames
    fc = FrameCodec(model)
    slab_codes, families = set(), {}
    with torch.no_grad():
        ref0 = fc.encode_batch([frames[0]], [None], [None], FRAME_I)
        ref2 = fc.encode_batch([frames[2]], [ref0['rec'][0]], [None], FRAME_P)
        prev, nxt = ref0['rec'][0], ref2['rec'][0]
        for ftype, cur, p, n in ((FRAME_I, frames[0], None, None), (FRAME_P, frames[2], prev, None), (FRAME_B, frames[1], prev, nxt)):
            rec.on = True
            ref = fc.encode_batch([cur], [p], [n], ftype)
            one = rec.take()
            ref_bytes = finalize_frames(ref['sections'])[0]
            outs = _run_ranks(R, lambda b: (fc.encode_banded(cur, p, n, ftype, 0., b), b))
            banded = rec.take()
            rec.on = False
            for r, (o, b) in enumerate(outs):
                for k in 'yuv':
                    assert torch.equal(o['rec'][0][k], ref['rec'][0][k]), (ftype, r, k)
                assert o['data_dim'] == ref['data_dim']
            assert sum(b.launches for _, b in outs) > 0  # (a rank may own no rows: more ranks than the y grid has rows)
            for r in range(R):  # every rank holds the same latents
                assert finalize_frames(outs[r][0]['sections'])[0] == ref_bytes, (ftype, r)
            yh = fc.entropy_decode([ref_bytes], ftype, ref['data_dim'], 0., cuda)
            torch.cuda.synchronize()
            dec = _run_ranks(R, lambda b: fc.synthesise_banded(yh, p, n, ftype, ref['data_dim'], b))
            for r, d in enumerate(dec):
                for k in 'yuv':
                    assert torch.equal(d[k], ref['rec'][0][k]), ('decode', ftype, r, k)
            slab_codes |= {v for _, v in banded if v in WINO}
            families[ftype] = (_family(one), _family(banded))
    return slab_codes, families


def _model(cuda):
    from aivc_amd import synth
    from aivc_amd.models import arch
    model = synth.make_model(arch.DEFAULT_WIDTHS, seed=1234, device=cuda)
    synth.calibrate_operating_point(model, cuda)
    return model


@pytest.fixture
def any_size():
    from aivc_amd import ops
    prev = ops.WINO_ANY_SIZE
    ops.WINO_ANY_SIZE = True
    yield
    ops.WINO_ANY_SIZE = prev


@pytest.mark.parametrize('w,h,R', [(256, 144, 2), (250, 130, 3), (416, 240, 4), (160, 112, 8)])
def test_banded_frame_equals_single_rank_every_winograd_form(w, h, R, cuda, any_size, monkeypatch):
    """default widths, version 2 at any size: the 3x3, polyphase 5x5 and transposed 5x5 Winograd kernels all run on slabs,
    odd frame sizes, more ranks than the latent has rows"""
    from aivc_amd import synth
    rec = _Launches(monkeypatch)
    frames = synth.to_device_frames(synth.synthetic_video(w, h, 3, seed=5), cuda)
    codes, _ = _check(_model(cuda), frames, R, cuda, rec)
    assert codes == set(WINO), codes


@pytest.mark.parametrize('w,h,R', [(1920, 1080, 4), (3840, 2160, 8)])
def test_banded_frame_routed_like_the_frame_full_size(w, h, R, cuda, monkeypatch):
    """no any-size flag: the slabs are far below the size rules the frame passes, and only the routing by frame size keeps
    them in the frame's kernel family -- layer by layer, the banded launches take the single rank's Winograd code (the tap
    kernels' tiles may differ: version 1 bits do not depend on the tile)"""
    from aivc_amd import ops, synth
    assert not ops.WINO_ANY_SIZE
    rec = _Launches(monkeypatch)
    frames = synth.to_device_frames(synth.synthetic_video(w, h, 3, seed=6), cuda)
    codes, families = _check(_model(cuda), frames, R, cuda, rec)
    assert codes and codes == {c for one, _ in families.values() for f in one.values() for c in f if c in WINO}, codes
    for ftype, (one, banded) in families.items():
        for key in set(one) & set(banded):
            assert banded[key] == one[key], (ftype, key, banded[key], one[key])
        assert all(key in banded for key, fam in one.items() if fam & set(WINO)), ftype


# ---- real processes --------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _setup(gop, w, h):
    from aivc_amd import synth
    from aivc_amd.func_util.GOP_structure import generate_gop_struct
    dev = torch.device('cuda:0')
    model = _model(dev)
    frames = synth.to_device_frames(synth.synthetic_video(w, h, len(generate_gop_struct(gop)), seed=4), dev)
    return model, [frames], dev


def _planes(frs):
    return [bytes(torch.cat([fr[k].reshape(-1) for k in 'yuv']).cpu().numpy()) for fr in frs]


def _worker(rank, world, port, q, gop, w, h, any_size):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      AIVC_DIST_BACKEND='gloo', AIVC_BAND_LEVELS='1')
    os.environ.pop('AIVC_CONTRACT', None)
    import torch.distributed as dist
    from aivc_amd import abi, ops, parallel
    assert ops.PRECISION == abi.PREC_FP32_WINO
    ops.WINO_ANY_SIZE = any_size
    parallel.init_process_group()
    model, units, dev = _setup(gop, w, h)
    parallel.broadcast_model(model)
    fc = model.frame_codec()
    shard = parallel.ClipShard(1, dev)
    with torch.no_grad():
        blobs, dd = parallel.encode_clip(fc, units, gop, shard=shard)
        recs = parallel.decode_clip(fc, blobs, dd, dev, shard=shard)
    torch.cuda.synchronize()
    bands = getattr(shard, '_bands', None)
    q.put((rank, blobs, {u: _planes(frs) for u, frs in recs.items()}, None if bands is None else bands.launches))
    dist.destroy_process_group()


@pytest.mark.parametrize('gop,w,h,world,any_size', [('1_GOP_8', 256, 144, 2, True), ('1_GOP_8', 256, 144, 4, True),
                                                     ('1_GOP_2', 1920, 1080, 2, False)])
def test_processes_in_row_bands_match_single_process(gop, w, h, world, any_size, cuda):
    """ONE unit over `world` gloo processes on the one GPU with AIVC_BAND_LEVELS=1 in the default contract: its levels
    narrower than the group are coded in row bands; blobs and decoded planes are the single process's"""
    import torch.multiprocessing as mp
    from aivc_amd import ops
    port = _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, gop, w, h, any_size)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=600) for _ in procs], key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(timeout=60)
    assert all(p.exitcode == 0 for p in procs)
    assert all(r[1] == res[0][1] for r in res)
    assert all(r[3] is not None and r[3] > 0 for r in res)  # row bands were used
    model, units, dev = _setup(gop, w, h)
    fc = model.frame_codec()
    prev = ops.WINO_ANY_SIZE
    ops.WINO_ANY_SIZE = any_size
    try:
        with torch.no_grad():
            ref_blobs, ref_recs, dd = fc.encode_units(units, gop)
            ref_dec = fc.decode_units(ref_blobs, dd, dev)
    finally:
        ops.WINO_ANY_SIZE = prev
    assert res[0][1] == ref_blobs
    for r in res:
        for u, got in r[2].items():
            assert got == _planes(ref_dec[u])
            assert got == _planes(ref_recs[u])  # decoder == encoder reconstruction


# ---- bench.py ----------------------------------------------------------------------------------------------------------
def test_bench_one_unit_over_four_ranks_in_row_bands_in_the_default_contract(cuda):
    """bench.py's multi-rank flow (as tests/test_gpu_bench_rehearsal.py drives it) with AIVC_BAND_LEVELS=1 in version 2 at
    a size its Winograd kernels cover: one unit over 4 ranks, the narrow levels in row bands, bytes still one rank's"""
    env = dict(os.environ, AIVC_BENCH_SINGLE_DEVICE='1', AIVC_DIST_BACKEND='gloo', AIVC_NO_QUALITY='1',
               HSA_ENABLE_IPC_MODE_LEGACY='0', PYTHONDONTWRITEBYTECODE='1', AIVC_BAND_LEVELS='1')
    env.pop('WORLD_SIZE', None)
    env.pop('RANK', None)
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '4', '--steps', '1', '--warmup', '1',
           '--width', '1280', '--height', '720', '--frames', '8', '--gop', '1_GOP_8', '--contract', 'fp32w', '--no-cpu-baseline',
           '--no-roofline', '--no-high-rate', '--no-lean-encoder', '--no-precision-mode']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, 'bench.py --gpus 4 exited %d\n%s' % (r.returncode, r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out['n_gpus'] == 4 and out['arithmetic_contract'] == 'fp32w'
    assert out['bytes_equal_single_rank'] is True and out['closed_loop_ok'] is True
    assert out['stream_errors_rank0'] == 0
    assert out['config']['units_per_step'] == 1
    assert 'row bands' in out['config']['parallelism'], out['config']['parallelism']
