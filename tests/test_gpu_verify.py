"""Verified decodes: the encoder's sidecar manifest (--digests), the decoder's comparison on the device (--verify), the exit
statuses, and the arithmetic contract taken from the manifest or found by a trial decode (--contract auto).  The default-width
synthetic model of the command line, as in tests/test_gpu_configs.py.

The always-on detector of a foreign stream is the range decoder's bit count, which sees the entropy stage only (z -> h_s ->
(mu, sigma) -> y).  Test (c) builds the case it cannot see: a 1024x576 I frame, whose y grid of 64 x 36 positions keeps the 3x3
layer of h_s below AIVC_WINO_MIN_PIXELS in both contracts, while the transposed 128 -> 64 layer of g_s (128 x 72 -> 256 x 144,
36 864 outputs) is a Winograd launch under fp32w and a tap chain under fp32: a decode in the wrong contract is clean for the bit
count and wrong in its samples.  Test (d) builds the case it can see: 1440x1424, a y grid of 90 x 89 = 8010 positions, where
h_s itself differs between the contracts."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def model(cuda):
    """what aivc_amd.cli_common.get_model builds when the assets are absent (same seeds, same calibration)"""
    from aivc_amd import synth
    m = synth.make_model(device=cuda)
    synth.calibrate_operating_point(m, cuda)
    return m


@pytest.fixture
def clis(model, monkeypatch):
    from aivc_amd import decode as dec_cli
    from aivc_amd import encode as enc_cli
    monkeypatch.setattr(dec_cli, 'get_model', lambda name, dev: model)
    monkeypatch.setattr(enc_cli, 'get_model', lambda name, dev: model)
    return enc_cli, dec_cli


def write_clip(tmp_path, w, h, n, **kw):
    from aivc_amd import synth
    frames = synth.synthetic_video(w, h, n, **kw)
    raw = tmp_path / ('clip_%dx%d_30_420.yuv' % (w, h))
    with open(raw, 'wb') as f:
        for fr in frames:
            for k in 'yuv':
                f.write(np.ascontiguousarray(fr[k]).tobytes())
    return frames, str(raw)


def hashlib_rows(recs, first=0):
    return {first + i: tuple(hashlib.md5(r[k].cpu().numpy().tobytes()).hexdigest() for k in 'yuv') for i, r in enumerate(recs)}


def library_encode(model, frames, gop, cuda, contract=None):
    """FrameCodec alone -> (bitstream, reconstructions of the real frames)"""
    from aivc_amd import ops, synth
    from aivc_amd.codec import FrameCodec
    prev = ops.set_precision(contract) if contract else None
    try:
        fc = FrameCodec(model)
        with torch.no_grad():
            enc = fc.encode_video(synth.to_device_frames(frames, cuda), gop)
        return fc.assemble_video(enc), [r for g in enc['recs'] for r in g][:len(frames)]
    finally:
        if prev:
            ops.set_precision(prev)


def library_decode(model, blob, cuda, contract):
    """-> (frames, number of sections whose bit count does not account for their payload)"""
    from aivc_amd import ops
    from aivc_amd.codec import FrameCodec
    prev = ops.set_precision(contract)
    try:
        fc = FrameCodec(model)
        with torch.no_grad():
            frames = fc.decode_video(blob, cuda)[0]
        return frames, len(fc.stream_errors())
    finally:
        ops.set_precision(prev)


def planes_differ(a, b):
    return sum(int((x[k] != y[k]).sum()) for x, y in zip(a, b) for k in 'yuv')


def read_planes(path, w, h, n):
    hc, wc = (h + 1) // 2, (w + 1) // 2
    raw = np.fromfile(path, np.uint8).reshape(n, h * w + 2 * hc * wc)
    return [{'y': raw[i, :h * w].reshape(1, h, w), 'u': raw[i, h * w:h * w + hc * wc].reshape(1, hc, wc),
             'v': raw[i, h * w + hc * wc:].reshape(1, hc, wc)} for i in range(n)]


def flip_one_payload_byte(blob):
    """as tests/test_gpu_configs.py::test_decode_cli_status_is_returned_by_main: a byte a third into the y payload of frame 0"""
    from aivc_amd.real_life import cat_binary_files as cont
    from aivc_amd.real_life.bitstream import split_sections
    f0 = cont.unpack_gop(cont.unpack_video(blob)[3][0])[2][0]
    sy = split_sections(f0)[3]
    pos = f0.index(sy) + 1 + sy[0] + (len(sy) - 1 - sy[0]) // 3
    bad = bytearray(f0)
    bad[pos] ^= 0x5A
    return blob.replace(f0, bytes(bad), 1)


@pytest.fixture(scope='module')
def small_loop(model, cuda, tmp_path_factory):
    """96x64, 3 frames, 1_GOP_2, coded once with and once without digests through real_life.encode.encode"""
    from aivc_amd.real_life.encode import encode
    tmp = tmp_path_factory.mktemp('verify_small')
    frames, raw = write_clip(tmp, 96, 64, 3, noise=2.0)
    common = {'model': model, 'sequence_path': raw, 'GOP_struct_name': '1_GOP_2'}
    encode(dict(common, final_file=str(tmp / 'with.bin'), digests=True))
    encode(dict(common, final_file=str(tmp / 'without.bin')))
    return tmp, frames


def test_manifest_is_hashlib_of_the_reconstructions_and_leaves_the_bitstream_alone(small_loop, model, cuda, clis, capsys):
    from aivc_amd import digests, ops
    tmp, frames = small_loop
    _, dec_cli = clis
    blob = (tmp / 'with.bin').read_bytes()
    assert blob == (tmp / 'without.bin').read_bytes()
    assert os.path.exists(tmp / 'with.bin.md5') and not os.path.exists(tmp / 'without.bin.md5')
    lib_blob, recs = library_encode(model, frames, '1_GOP_2', cuda)
    assert lib_blob == blob and len(recs) == 3
    m = digests.read_manifest(str(tmp / 'with.bin.md5'))
    assert m.contract == ops.precision_name() and m.rows == hashlib_rows(recs)
    capsys.readouterr()
    assert dec_cli.main(['-i', str(tmp / 'with.bin'), '-o', str(tmp / 'ok.yuv'), '--verify']) == 0
    assert '[VERIFY] 3 frames, 0 planes differ' in capsys.readouterr().out
    assert dec_cli.main(['-i', str(tmp / 'without.bin'), '-o', str(tmp / 'ok2.yuv'), '--verify', str(tmp / 'with.bin.md5')]) == 0
    assert planes_differ(read_planes(tmp / 'ok.yuv', 96, 64, 3), [{k: r[k].cpu().numpy() for k in 'yuv'} for r in recs]) == 0


def test_status_4_for_other_digests_and_3_for_a_stream_error(small_loop, clis, capsys):
    tmp, _ = small_loop
    _, dec_cli = clis
    blob = (tmp / 'with.bin').read_bytes()
    assert dec_cli.main(['-i', str(tmp / 'with.bin'), '-o', str(tmp / 'ref.yuv')]) == 0
    # one hexadecimal digit of the manifest: the u plane of frame 1
    lines = (tmp / 'with.bin.md5').read_text().split('\n')
    tok = lines[2].split(' ')
    tok[2] = tok[2][:5] + ('0' if tok[2][5] != '0' else '1') + tok[2][6:]
    lines[2] = ' '.join(tok)
    (tmp / 'changed.md5').write_text('\n'.join(lines))
    capsys.readouterr()
    assert dec_cli.main(['-i', str(tmp / 'with.bin'), '-o', str(tmp / 'four.yuv'), '--verify', str(tmp / 'changed.md5')]) == 4
    out = capsys.readouterr().out
    assert '[VERIFY] 3 frames, 1 planes differ' in out and '1_u' in out
    assert (tmp / 'four.yuv').read_bytes() == (tmp / 'ref.yuv').read_bytes()  # the frames are written regardless
    # a damaged payload: the stream error takes precedence over the digests that differ with it
    (tmp / 'bad.bin').write_bytes(flip_one_payload_byte(blob))
    assert dec_cli.main(['-i', str(tmp / 'bad.bin'), '-o', str(tmp / 'bad.yuv'), '--verify', str(tmp / 'with.bin.md5')]) == 3
    assert '[VERIFY] 3 frames' in capsys.readouterr().out
    assert os.path.getsize(tmp / 'bad.yuv') == os.path.getsize(tmp / 'ref.yuv')
    assert dec_cli.main(['-i', str(tmp / 'with.bin'), '-o', str(tmp / 'ref.yuv')]) == 0  # (and nothing of it outlives the call)


def test_contract_from_the_manifest(model, cuda, clis, tmp_path, capsys):
    from aivc_amd import digests, ops
    enc_cli, dec_cli = clis
    default = ops.precision_name()
    w, h = 1024, 576
    frames, raw = write_clip(tmp_path, w, h, 1, seed=31)
    bits = str(tmp_path / 'v1.bin')
    enc_cli.main(['-i', raw, '--gop', '1_GOP_0', '-o', bits, '--digests', '--contract', 'fp32'])
    assert ops.precision_name() == default
    blob = open(bits, 'rb').read()
    lib_blob, recs = library_encode(model, frames, '1_GOP_0', cuda, 'fp32')
    assert blob == lib_blob
    m = digests.read_manifest(bits + '.md5')
    assert m.contract == 'fp32' and m.rows == hashlib_rows(recs)
    # the precondition: the two contracts decode this stream to different samples, and the bit count sees neither
    in_v1, errors_v1 = library_decode(model, blob, cuda, 'fp32')
    in_v2, errors_v2 = library_decode(model, blob, cuda, 'fp32w')
    differing = planes_differ(in_v1, in_v2)
    print('1024x576 I frame coded under fp32: %d samples differ between an fp32 and an fp32w decode; sections with a bit-count '
          'error: %d and %d' % (differing, errors_v1, errors_v2))
    assert differing >= 1 and planes_differ(in_v1, recs) == 0
    assert errors_v1 == 0 and errors_v2 == 0
    capsys.readouterr()
    # auto: the manifest names the contract, verification is implied
    assert dec_cli.main(['-i', bits, '-o', str(tmp_path / 'auto.yuv'), '--contract', 'auto']) == 0
    out = capsys.readouterr().out
    assert 'arithmetic contract: fp32 ' in out and '[VERIFY] 1 frames, 0 planes differ' in out
    assert planes_differ(read_planes(tmp_path / 'auto.yuv', w, h, 1), [{k: r[k].cpu().numpy() for k in 'yuv'} for r in recs]) == 0
    assert ops.precision_name() == default
    # the wrong contract by name: clean for the bit count, caught by the digests
    assert dec_cli.main(['-i', bits, '-o', str(tmp_path / 'v2.yuv'), '--contract', 'fp32w', '--verify']) == 4
    out = capsys.readouterr().out
    assert '[WARN]' not in out and '[VERIFY] 1 frames, ' in out and '0 planes differ' not in out
    assert ops.precision_name() == default


def test_contract_from_a_trial_decode(model, cuda, clis, tmp_path, capsys):
    from aivc_amd import _lib, abi, ops
    enc_cli, dec_cli = clis
    default = ops.precision_name()
    other = 'fp32' if default == 'fp32w' else 'fp32w'
    w, h = 1440, 1424
    # the 3x3 layer of h_s on the 90 x 89 y grid is a Winograd launch under fp32w: the entropy stage depends on the contract
    wd = 128
    p = abi.ConvParams(abi.MODE_CONV, 3, 1, 1, 1, h // 16, w // 16, wd, h // 16, w // 16, wd, 0, 0, abi.ALGO_AUTO, 0, 0,
                       1 << 20, 2 << 20, 3 << 20, None, None, 6 << 20, None, None)
    p.precision = abi.PREC_FP32_WINO
    assert (h // 16) * (w // 16) >= abi.WINO_MIN_PIXELS and _lib.load()['aivc_conv2d_variant'](ctypes.byref(p)) == 301
    frames, raw = write_clip(tmp_path, w, h, 1, seed=32)
    bits = str(tmp_path / 'other.bin')
    enc_cli.main(['-i', raw, '--gop', '1_GOP_0', '-o', bits, '--contract', other])
    assert not os.path.exists(bits + '.md5') and ops.precision_name() == default
    _, recs = library_encode(model, frames, '1_GOP_0', cuda, other)
    capsys.readouterr()
    assert dec_cli.main(['-i', bits, '-o', str(tmp_path / 'plain.yuv')]) == 3
    assert '[WARN]' in capsys.readouterr().out
    assert dec_cli.main(['-i', bits, '-o', str(tmp_path / 'auto.yuv'), '--contract', 'auto']) == 0
    out = capsys.readouterr().out
    assert '[INFO] arithmetic contract: %s (detected on unit 0)' % other in out and '[WARN]' not in out
    assert planes_differ(read_planes(tmp_path / 'auto.yuv', w, h, 1), [{k: r[k].cpu().numpy() for k in 'yuv'} for r in recs]) == 0
    assert ops.precision_name() == default


def test_trial_decode_for_a_request_that_does_not_touch_unit_0(model, cuda, clis, tmp_path, capsys):
    """two units (two I frames of the stream above) without a manifest: a request inside unit 1 still probes unit 0, read
    through the index, and prints the note of the whole decode"""
    from aivc_amd import ops
    enc_cli, dec_cli = clis
    default = ops.precision_name()
    other = 'fp32' if default == 'fp32w' else 'fp32w'
    w, h = 1440, 1424
    frames, raw = write_clip(tmp_path, w, h, 2, seed=32)
    bits = str(tmp_path / 'two.bin')
    enc_cli.main(['-i', raw, '--gop', '1_GOP_0', '-o', bits, '--contract', other])
    assert not os.path.exists(bits + '.md5')
    _, recs = library_encode(model, frames, '1_GOP_0', cuda, other)
    note = '[INFO] arithmetic contract: %s (detected on unit 0)' % other
    capsys.readouterr()
    assert dec_cli.main(['-i', bits, '-o', str(tmp_path / 'whole.yuv'), '--contract', 'auto']) == 0
    out = capsys.readouterr().out
    assert note in out and '[WARN]' not in out and '[INFO] partial decode' not in out
    assert dec_cli.main(['-i', bits, '-o', str(tmp_path / 'part.yuv'), '--contract', 'auto', '--frames', '1']) == 0
    out = capsys.readouterr().out
    assert note in out and '[WARN]' not in out and '[INFO] partial decode: 1 frames written, 1 of 2 coded frames decoded' in out
    assert planes_differ(read_planes(tmp_path / 'whole.yuv', w, h, 2), [{k: r[k].cpu().numpy() for k in 'yuv'} for r in recs]) == 0
    assert planes_differ(read_planes(tmp_path / 'part.yuv', w, h, 1), [{k: recs[1][k].cpu().numpy() for k in 'yuv'}]) == 0
    assert ops.precision_name() == default


def test_encode_stages_write_the_bytes_of_the_one_body(model, cuda, golden, tmp_path, capsys):
    """encode() with the quality log, the manifest, scene cuts and flag_bitstream_debug all on: the bitstream, the manifest and
    detailed.txt are the bytes the commit before the stages wrote for the same call without the debug flag
    (tests/golden/encode_stages.npz, tools/gen_golden_encode_stages.py); the debug digests -- one per reconstructed plane, of
    every frame that is not padding -- are accepted by check_debug_md5 against the decode of that bitstream"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import gen_golden_encode_stages as gen
    from aivc_amd.real_life.decode import Decoder, check_debug_md5, debug_dir, decode_one_video
    fx = golden('encode_stages')
    out, files = gen.encode_case(model, str(tmp_path), flag_bitstream_debug=True)
    blob = open(files['bitstream'], 'rb').read()
    assert blob == fx['bitstream'].tobytes()
    assert open(files['manifest']).read() == str(fx['manifest'])
    assert open(files['detailed']).read() == str(fx['detailed'])
    assert out['real_rate_byte'] == len(blob) and out['nb_frames_to_code'] == gen.N
    assert sorted(os.listdir(debug_dir(files['bitstream']))) == sorted('%d_%s.md5' % (i, c) for i in range(gen.N) for c in 'yuv')
    frames = decode_one_video({'decoder': Decoder({'full_net': model}).eval(), 'bitstream_path': files['bitstream'], 'device': str(cuda)})
    capsys.readouterr()
    assert len(frames) == gen.N and check_debug_md5(frames, 0, debug_dir(files['bitstream'])) == 0
    assert capsys.readouterr().out.count('Identical reconstruction!') == 3 * gen.N


def test_two_ranks_write_the_manifest_of_one_process(model, cuda, tmp_path):
    """aivc.py --digests under `torch.distributed.run` with two ranks on the one GPU over gloo (as
    tests/test_gpu_multi_process.py::test_cli_two_ranks_equals_one_process): every rank digests the units it coded, the 48-byte
    rows travel to rank 0, which writes ONE manifest -- hashlib of a single process's reconstructions -- and verifies the
    planes it collected."""
    import socket
    import subprocess
    import sys
    from aivc_amd import digests, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    w, h, n = 96, 64, 10  # RA 2/4: three intra-period units of 5, 4 and (padded) 1 frames
    frames, raw = write_clip(tmp_path, w, h, n)
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''), AIVC_DIST_BACKEND='gloo', AIVC_SINGLE_DEVICE='1')
    two = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                          '--master-port', str(port), '-m', 'aivc_amd.aivc', '-i', raw, '--coding_config', 'RA', '--gop_size', '2',
                          '--intra_period', '4', '--start_frame', '0', '--end_frame', str(n - 1), '--digests',
                          '--bitstream_out', str(tmp_path / 'b.bin'), '-o', str(tmp_path / 'b.yuv')],
                         cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert two.returncode == 0, two.stdout[-2000:] + two.stderr[-2000:]
    assert two.stdout.count('[VERIFY] 10 frames, 0 planes differ') == 1
    blob, recs = library_encode(model, frames, '2_GOP_2', cuda)
    assert (tmp_path / 'b.bin').read_bytes() == blob
    m = digests.read_manifest(str(tmp_path / 'b.bin.md5'))
    assert m.contract == ops.precision_name() and m.rows == hashlib_rows(recs)
