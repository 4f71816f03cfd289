"""CPU-side checks: the C ABI library exports every symbol the header declares, module aliases make
full-module pickles loadable, CLI mapping, product path fails loudly without a GPU."""
import ctypes
import io
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, 'include', 'aivc_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = re.sub(r'static inline[^{]*\{.*?\n\}', '', src, flags=re.S)  # (inline rules shared with the oracle: not exports)
    return sorted(set(re.findall(r'\b(?:int|const char \*)\s*(aivc_\w+)\s*\(', src)))


def test_hip_library_exports_every_declared_symbol():
    lib_path = os.path.join(ROOT, 'aivc_amd', 'lib', 'libaivc_hip.so')
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build_hip()
    lib = ctypes.CDLL(lib_path)  # loads without a GPU (no compute call is made)
    names = header_functions()
    assert len(names) >= 24
    for n in names:
        assert hasattr(lib, n), 'libaivc_hip.so does not export %s' % n
    lib.aivc_abi_version.restype = ctypes.c_int
    from aivc_amd import abi
    assert lib.aivc_abi_version() == abi.ABI_VERSION
    # every prototype bound by abi.py is declared in the header and vice versa
    assert set(abi.PROTOTYPES) | {'aivc_abi_version', 'aivc_last_error', 'aivc_conv2d_variant', 'aivc_selfcheck_gdn_math',
                                  'aivc_detmath_eval'} == set(names)


def test_oracle_exports_ref_twins(oracle):
    lib = ctypes.CDLL(os.path.join(ROOT, 'oracle', 'libaivc_oracle.so'))
    from aivc_amd import abi
    for n in abi.PROTOTYPES:
        assert hasattr(lib, n + '_ref')
    assert hasattr(lib, 'aivc_detmath_eval_ref')  # (a diagnostic outside PROTOTYPES whose twin the accuracy tests run on)


def test_argument_validation_without_gpu():
    """error paths return codes instead of crashing (no kernel is launched)."""
    from aivc_amd import _lib, abi
    fns = _lib.load()
    assert fns['aivc_conv2d'](None, None) == -1
    p = abi.ConvParams(abi.MODE_CONV, 7, 1, 3, 1, 8, 8, 4, 8, 8, 4, 0, 0, 0, 0, 0, 1, 1, None, None, None, 1, None, None)
    assert fns['aivc_conv2d'](ctypes.byref(p), None) == -2  # ksize 7 unsupported
    p = abi.ConvParams(abi.MODE_CONV, 3, 1, 1, 1, 8, 8, 3, 8, 8, 4, 0, 0, 0, 0, 0, 1, 1, None, None, None, 1, None, None)
    assert fns['aivc_conv2d'](ctypes.byref(p), None) == -1  # c_in not a multiple of 4
    p = abi.ConvParams(abi.MODE_CONV, 3, 2, 1, 1, 9, 9, 4, 4, 5, 4, 0, 0, 0, 0, 0, 1, 1, None, None, None, 1, None, None)
    assert fns['aivc_conv2d'](ctypes.byref(p), None) == -1  # wrong output size
    assert fns['aivc_conv2d_variant'](ctypes.byref(abi.ConvParams(
        abi.MODE_CONV, 3, 1, 1, 1, 270, 480, 128, 270, 480, 128, 0, 0, 0, 0, 0, 1, 1, None, None, None, 1, None, None))) == 105  # 64x128 (round-3 tile rules)
    # aivc_detmath_eval: an unknown function, null a / out, null b of a two-operand function; n == 0 does nothing
    ev = fns['aivc_detmath_eval']
    assert ev(abi.DETMATH_COUNT, 1, 1, 4, 1, None) == -1 and ev(-1, 1, 1, 4, 1, None) == -1
    assert ev(abi.DETMATH_COUNT, None, None, 0, None, None) == -1
    for fn in range(abi.DETMATH_COUNT):
        assert ev(fn, None, 1, 4, 1, None) == -1 and ev(fn, 1, 1, 4, None, None) == -1
        if abi.detmath_operands(fn) == 2:  # (a one-operand function would take this call: never made with stand-in pointers)
            assert ev(fn, 1, None, 4, 1, None) == -1
        assert ev(fn, None, None, 0, None, None) == 0


def test_conv_dispatch_of_the_default_model_at_1080p():
    """aivc_conv2d_variant on every conv parameter set of a `bench.py --full` run (default widths, 1920x1080: every
    dependency level's batch, the fused and the unfused GDN / tail requests, the side measurements' shapes) under fp32,
    fp32w and bf16x3 (weights split in the K loop, and split ahead): the kernel each launch takes, checked without a GPU.
    The expected codes are what the library answered before its dispatch became one routing function
    (tests/golden/conv_variants_1080p.npz; x / w 16-byte aligned, bias always given, as the codec launches them)."""
    import numpy as np
    from aivc_amd import _lib, abi
    fns = _lib.load()
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'conv_variants_1080p.npz'))
    assert list(g['columns'][16:]) == ['fp32', 'fp32w', 'bf16x3', 'bf16x3_split']
    rows = g['rows']
    assert len(rows) == 247
    a = 1 << 20
    for r in rows.tolist():
        mode, k, s, pad, n, h, w, ci, co, act1, act2, gdn, flags, mul, res, tail = r[:16]
        ho, wo = abi.conv_out_size(mode, h, w, k, s, pad)
        p = abi.ConvParams(mode, k, s, pad, n, h, w, ci, ho, wo, co, act1, act2, abi.ALGO_AUTO, gdn, flags, a, 2 * a, 3 * a,
                           4 * a if mul else None, 5 * a if res else None, 6 * a, 7 * a if gdn else None, 8 * a if gdn else None)
        if tail:
            p.tail_w, p.tail_bias, p.tail_c_out = 9 * a, 10 * a, tail
        got = []
        for prec, split in ((abi.PREC_FP32, False), (abi.PREC_FP32_WINO, False), (abi.PREC_BF16X3, False), (abi.PREC_BF16X3, True)):
            p.precision, p.w_bf16x3 = prec, 11 * a if split else None
            got.append(fns['aivc_conv2d_variant'](ctypes.byref(p)))
        assert got == r[16:], (r[:16], got, r[16:])


def _variant(mode, k, s, pad, n, h, w, ci, co, gdn=0, tail=0, algo=None, precision=None, flags=0):
    """aivc_conv2d_variant of one launch (fp32 unless precision says otherwise) with stand-in pointers (nothing is allocated, nothing
    launched)"""
    from aivc_amd import _lib, abi
    a = 1 << 20
    ho, wo = abi.conv_out_size(mode, h, w, k, s, pad)
    p = abi.ConvParams(mode, k, s, pad, n, h, w, ci, ho, wo, co, 0, 0, abi.ALGO_AUTO if algo is None else algo, gdn, flags, a, 2 * a, 3 * a,
                       None, None, 6 * a, 7 * a if gdn else None, 8 * a if gdn else None)
    if tail:
        p.tail_w, p.tail_bias, p.tail_c_out = 9 * a, 10 * a, tail
    p.precision = abi.PREC_FP32 if precision is None else precision
    return _lib.load()['aivc_conv2d_variant'](ctypes.byref(p))


def test_conv_dispatch_at_the_loaders_4_gib_limit():
    """The LDS-DMA K loop (conv; transposed conv with c_in % 32 == 0) addresses ONE image's input and the weights with 32-bit
    byte offsets, and no other MFMA kernel is built for these modes: at 4 GiB per image a plain launch takes the scalar kernel
    (64-bit indexing, same bits) and a fused request is declined (the caller issues two launches).  A batch beyond 4 GiB
    of smaller images is sub-batched as before, and the register-staged families keep their 2^32-ELEMENT limit."""
    from aivc_amd import abi
    conv = (abi.MODE_CONV, 3, 1, 1)
    at = conv + (1, 4096, 4096, 64, 64)  # 4096 * 4096 * 64 * 4 bytes = 4 GiB exactly
    assert 4096 * 4096 * 64 * 4 == 1 << 32
    assert _variant(*at) == 0
    assert _variant(*at, gdn=1) == abi.ERR_UNSUPPORTED
    assert _variant(*at, tail=128) == abi.ERR_UNSUPPORTED
    assert _variant(*at, algo=abi.ALGO_MFMA) == abi.ERR_UNSUPPORTED
    below = conv + (1, 4095, 4096, 64, 64)
    assert 100 <= _variant(*below) <= 109
    assert 150 <= _variant(*below, gdn=1) <= 159
    assert _variant(*below, tail=128) == 190
    # two images of 2.5 GiB: sub-batches of one image each, the same kernel as ever
    assert _variant(*conv, 2, 2560, 4096, 64, 64) == 102
    # transposed conv, c_in % 32 == 0: the same limit
    tconv = (abi.MODE_TCONV, 5, 2, 0)
    assert _variant(*tconv, 1, 4095, 4096, 64, 64) == 111
    assert _variant(*tconv, 1, 4096, 4096, 64, 64) == 0
    assert _variant(*tconv, 1, 4096, 4096, 64, 64, gdn=2) == abi.ERR_UNSUPPORTED
    # transposed conv with a generic reduction is register-staged: element offsets, no byte limit
    assert _variant(*tconv, 1, 4096, 4096, 48, 64) == 111
    assert 4096 * 8192 * 48 * 4 > 1 << 32 and 4096 * 8192 * 48 < (1 << 32) - 1
    assert _variant(*tconv, 1, 4096, 8192, 48, 64) == 111
    assert _variant(*tconv, 1, 4096, 8192, 48, 64, gdn=2) == 161


def test_conv_dispatch_limits_of_winograd_thin_and_resident_gdn():
    """The addressing limits the other families declare, at the limit and just below it (stand-in pointers, nothing launched).
    Winograd chain (conv2d_wino_supported): 32-bit byte offsets inside ONE image's input (below 0xFFFF0000 bytes), a block list an
    int counts (below 2^31 - 1 entries), the transposed form's 4 KB zero page (c_in <= 960).  A covered layer beyond a limit is
    AIVC_ERR_UNSUPPORTED, never a version-1 code: the header says it is computed by the Winograd chain or not at all.
    Thin transposed layers (thin_mfma_ok): an image below 0x7FFFFFC0 bytes goes through the MFMA kernel's buffer descriptor (2), a
    larger one to the VALU kernel (1), which indexes with size_t throughout and has no limit of its own.
    Resident (I)GDN (gdn_resident_supported): an int counts the pixels (below 0x7FFFFFC0); from there the launch is version 1's
    GDN mode, which at 128 channels and that many pixels is the scalar kernel (0: the MFMA family stops at 2^32 - 1 elements)."""
    from aivc_amd import abi
    w2, unsupported = abi.PREC_FP32_WINO, abi.ERR_UNSUPPORTED
    conv3, conv5, tconv5 = (abi.MODE_CONV, 3, 1, 1), (abi.MODE_CONV, 5, 2, 2), (abi.MODE_TCONV, 5, 2, 0)
    forms = ((conv3, 128, 301), (conv5, 128, 302), (tconv5, 64, 303))
    # one image's input: c_in 32 = 128 bytes per pixel, 0xFFFF0000 / 128 = 33553920 = 65535 * 512 pixels
    assert 33553920 * 128 == 0xFFFF0000 and 33553919 == 7 * 4793417
    for form, co, code in forms:
        assert _variant(*form, 1, 4793417, 7, 32, co, precision=w2) == code      # 128 bytes below the limit
        assert _variant(*form, 1, 65535, 512, 32, co, precision=w2) == unsupported
        assert _variant(*form, 1, 65535, 512, 32, co) not in (code, unsupported)  # (version 1 has kernels for it)
    # the block list: images x blocks of 16 x 16 grid pixels x blocks of 64 output channels (x 4 classes, transposed form).
    # conv forms, c_out 128: an even count; 2^31 - 2 = 2 * 17043521 * 7 * 9 (100 x 130 grid pixels: 7 x 9 blocks)
    assert 2 * 17043521 * 63 == 0x7FFFFFFE
    assert _variant(*conv3, 17043521, 100, 130, 32, 128, precision=w2) == 301
    assert _variant(*conv5, 17043521, 200, 260, 32, 128, precision=w2) == 302
    for form in (conv3, conv5):  # 2^31 entries
        g = 2 if form is conv5 else 1
        assert _variant(*form, 1 << 24, 128 * g, 128 * g, 32, 128, precision=w2) == unsupported
    # transposed form, c_out 64: a multiple of 4; 2^31 - 4 = 4 * 2304167 * 233 (3728 x 16 grid pixels: 233 x 1 blocks)
    assert 4 * 2304167 * 233 == 0x7FFFFFFC
    assert _variant(*tconv5, 2304167, 3728, 16, 32, 64, precision=w2) == 303
    assert _variant(*tconv5, 1 << 21, 4096, 16, 32, 64, precision=w2) == unsupported
    # the transposed form's zero page
    assert _variant(*tconv5, 1, 270, 480, 960, 64, precision=w2) == 303
    assert _variant(*tconv5, 1, 270, 480, 992, 64, precision=w2) == unsupported
    assert _variant(*tconv5, 1, 270, 480, 992, 64) == 111
    # thin transposed layer, c_in 64 = 256 bytes per pixel: 2^23 - 1 = 47 * 178481 pixels are 192 bytes below 0x7FFFFFC0
    assert 47 * 178481 * 256 == 0x7FFFFFC0 - 192 and 2048 * 4096 * 256 == 0x7FFFFFC0 + 64
    for prec in (abi.PREC_FP32, w2):
        assert _variant(*tconv5, 1, 47, 178481, 64, 3, precision=prec) == 2
        assert _variant(*tconv5, 1, 2048, 4096, 64, 3, precision=prec) == 1
        assert _variant(*tconv5, 2, 2048, 4096, 64, 3, precision=prec) == 1
    # stand-alone (I)GDN of 128 channels: the pixels of the whole batch
    for mode in (abi.MODE_GDN, abi.MODE_IGDN):
        for prec in (abi.PREC_FP32, w2):
            assert _variant(mode, 1, 1, 0, 1, 1, 0x7FFFFFBF, 128, 128, precision=prec) == 400
            assert _variant(mode, 1, 1, 0, 243, 7, 1262483, 128, 128, precision=prec) == 400  # 3^5 * 7 * 1262483 = 0x7FFFFFBF
            assert _variant(mode, 1, 1, 0, 1, 1, 0x7FFFFFC0, 128, 128, precision=prec) == 0
            assert _variant(mode, 1, 1, 0, 64, 31 * 601, 1801, 128, 128, precision=prec) == 0  # 2^6 * 31 * 601 * 1801 = 0x7FFFFFC0


def test_product_path_refuses_cpu_tensors():
    from aivc_amd import ops
    from aivc_amd._lib import AivcNativeError
    with pytest.raises(AivcNativeError):
        ops.conv2d(torch.zeros(1, 4, 4, 4), torch.zeros(4, 3, 3, 4))
    from aivc_amd.layers.misc.custom_conv_layers import CustomConvLayer
    with pytest.raises(AivcNativeError):
        CustomConvLayer(3, 4, 4)(torch.zeros(1, 4, 8, 8))
    from aivc_amd.cli_common import resolve_device
    with pytest.raises(SystemExit):
        resolve_device(True)


def test_full_module_pickle_round_trip_through_reference_module_names():
    """A reference .pt is a pickle of the whole nn.Module whose classes live in `layers.*`,
    `models.*`: the aliases must resolve them to this package."""
    import aivc_amd
    from aivc_amd import synth
    from aivc_amd.models import arch
    aivc_amd.install_aliases()
    model = synth.make_model(arch.TINY_WIDTHS, seed=3)
    for net in (model.codec_net.codec_net, model.mode_net.mode_net):
        net.ac = None  # not pickled upstream either

    # write the pickle with the REFERENCE's module paths (what a real .pt contains)
    classes = {type(m) for m in model.modules() if type(m).__module__.startswith('aivc_amd.')}
    saved = {c: c.__module__ for c in classes}
    try:
        for c in classes:
            c.__module__ = c.__module__[len('aivc_amd.'):]
        buf = io.BytesIO()
        torch.save(model, buf)
    finally:
        for c, m in saved.items():
            c.__module__ = m
    raw = buf.getvalue()
    assert b'layers.misc.custom_conv_layers' in raw and b'aivc_amd.layers' not in raw
    loaded = torch.load(io.BytesIO(raw), map_location='cpu', weights_only=False)
    assert type(loaded).__name__ == 'FullNet'
    sd_a, sd_b = model.state_dict(), loaded.state_dict()
    assert sd_a.keys() == sd_b.keys()
    assert all(torch.equal(sd_a[k], sd_b[k]) for k in sd_a)
    # the attribute contract the reference's decoder reads (src/real_life/decode.py:447-453,770-795)
    cn = loaded.codec_net.codec_net
    for attr in ('g_s', 'h_s', 'g_a_ref', 'pdf_y', 'pdf_z', 'pdf_parameterizer', 'out_c_shortcut_y', 'nb_ft_y',
                 'nb_ft_z', 'gain_I', 'flag_gain_p_b', 'gain_P', 'gain_B'):
        assert hasattr(cn, attr)
    for attr in ('codec_net', 'mode_net', 'motion_compensation', 'in_layer', 'out_layer', 'model_param'):
        assert hasattr(loaded, attr)
    assert 'lambda_tradeoff' in loaded.model_param


def test_cli_gop_mapping():
    from aivc_amd.aivc import gop_name
    assert gop_name('AI', 32, 32) == '1_GOP_0'
    assert gop_name('LDP', 32, 8) == 'LDP_8'
    assert gop_name('RA', 16, 32) == '2_GOP_16'   # the reference's sanity_script.sh setting
    assert gop_name('RA', 32, 32) == '1_GOP_32'
    with pytest.raises(SystemExit):
        gop_name('RA', 16, 24)


def test_section_framing_without_gpu():
    from aivc_amd.real_life.bitstream import split_sections
    frame = (0).to_bytes(4, 'big') * 2 + (3).to_bytes(4, 'big') + b'abc' + (1).to_bytes(4, 'big') + b'\x00'
    assert split_sections(frame) == [b'', b'', b'abc', b'\x00']


def test_md5_debug_digest_is_the_reference_procedure(tmp_path):
    """flag_md5sum (src/real_life/bitstream.py:229-234): md5 of the np.savetxt text of the NCHW-flattened latent"""
    import hashlib

    import numpy as np
    import torch
    from aivc_amd.real_life.bitstream import latent_md5
    rng = np.random.default_rng(3)
    q = torch.from_numpy(rng.integers(-256, 256, (1, 5, 7, 3)).astype(np.int16))  # NHWC
    q[0, 0, 0, 0], q[0, 0, 0, 1] = -256, 255
    x_nchw = q.permute(0, 3, 1, 2).to(torch.int16).numpy().astype(int)
    path = tmp_path / 'tmp_tensor.npy'
    np.savetxt(path, x_nchw.flatten())
    want = hashlib.md5(open(path, 'rb').read()).hexdigest().encode()
    assert latent_md5(q) == want and len(want) == 32


def test_debug_digest_kinds(tmp_path, capsys):
    """flag_bitstream_debug: a bare digest is the md5 of the PNG file (the reference's), 'raw:<md5>' that of the 8-bit
    plane; the decoder compares like with like (src/real_life/decode.py:304-326)"""
    import hashlib
    import numpy as np
    import torch
    from aivc_amd.real_life import decode as dec
    rng = np.random.default_rng(1)
    frames = [{k: torch.from_numpy(rng.integers(0, 256, (1, 6, 8) if k == 'y' else (1, 3, 4), dtype=np.uint8)) for k in 'yuv'}]
    d = str(tmp_path / 'dbg')
    dec.write_debug_md5(frames, 5, d)
    assert dec.check_debug_md5(frames, 5, d) == 0
    raw = hashlib.md5(frames[0]['y'].numpy().tobytes()).hexdigest()
    assert dec.plane_md5(frames[0]['y'], 'raw') == raw
    with open(tmp_path / 'dbg' / '5_y.md5', 'w') as f:  # an encoder without Pillow wrote this one
        f.write('raw:' + raw)
    assert dec.check_debug_md5(frames, 5, d) == 0
    with open(tmp_path / 'dbg' / '5_u.md5', 'w') as f:
        f.write('raw:' + raw)  # wrong plane
    assert dec.check_debug_md5(frames, 5, d) == 1
    assert 'Incorrect reconstruction' in capsys.readouterr().out


def test_clip_shard_is_built_once():
    """clip_shard() keeps one ClipShard per (units, world, device): constructing one allocates communicators"""
    import torch
    from aivc_amd import parallel
    a = parallel.clip_shard(4, torch.device('cpu'))
    assert parallel.clip_shard(4, torch.device('cpu')) is a and parallel.clip_shard(3, torch.device('cpu')) is not a
    assert (a.G, a.R, a.units) == (1, 1, [0, 1, 2, 3])


def test_bench_cli_parses():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--help'], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and '--gpus' in (out.stdout + out.stderr) and '--active-y' in (out.stdout + out.stderr)


def test_package_import_asks_for_eight_hardware_queues():
    """the codec's 8 entropy side streams need as many hardware queues: the package sets the runtime's
    variable at import unless the user already did -- checked in a fresh interpreter"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = 'import os, sys; sys.path.insert(0, %r); import aivc_amd; print(os.environ["GPU_MAX_HW_QUEUES"])' % root
    env = {k: v for k, v in os.environ.items() if k != 'GPU_MAX_HW_QUEUES'}
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120, env=env)
    assert out.stdout.strip() == '8', out.stderr
    env['GPU_MAX_HW_QUEUES'] = '4'
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120, env=env)
    assert out.stdout.strip() == '4', out.stderr


def test_encode_batch_hands_sections_over_before_the_synthesis():
    """FrameCodec.encode_batch(on_sections=...) exists and encode_units uses it (the flags of a batch leave for the
    host before its CodecNet synthesis is queued): a source-level check, the behaviour is covered by the GPU tests"""
    import inspect
    from aivc_amd import codec
    src = inspect.getsource(codec.FrameCodec.encode_batch)
    assert src.index('on_sections(sections)') < src.index('self.cod.synthesise(')
    assert 'on_sections=' in inspect.getsource(codec.FrameCodec.encode_units)


def _save_under_foreign_module_names(model, rename):
    """torch.save(model) as a pickle whose classes live at other dotted paths: rename(cls) -> module name"""
    import types
    classes = {type(m) for m in model.modules() if type(m).__module__.startswith('aivc_amd.')}
    saved = {c: c.__module__ for c in classes}
    fake = {}
    try:
        for c in classes:
            new = rename(c)
            if new not in sys.modules:
                fake[new] = sys.modules[new] = types.ModuleType(new)
            if new in fake:
                setattr(fake[new], c.__name__, c)
            c.__module__ = new
        buf = io.BytesIO()
        torch.save(model, buf)
    finally:
        for c, m in saved.items():
            c.__module__ = m
        for k in fake:
            del sys.modules[k]
    return buf.getvalue()


def test_load_model_resolves_unknown_module_paths_by_class_name(tmp_path, monkeypatch):
    """The dotted paths of the pickled `models.*` classes are unknown (the package is missing from the reference
    snapshot): a file that puts FullNet at models.net and the conditional coders at models.cond.sub
    loads through load_model's class-name fallback (src/model_mngt/model_management.py:341-361 is a plain torch.load),
    the inspector lists what it asks for without unpickling, and an unknown class is reported by name up front."""
    import aivc_amd
    from aivc_amd import synth
    from aivc_amd.model_mngt import model_management, pickle_compat
    from aivc_amd.models import arch
    aivc_amd.install_aliases()
    model = synth.make_model(arch.TINY_WIDTHS, seed=5)
    for net in (model.codec_net.codec_net, model.mode_net.mode_net):
        net.ac = None

    def rename(c):
        ref = c.__module__[len('aivc_amd.'):]
        if not ref.startswith('models.'):
            return ref  # layer classes: the reference's own paths
        return 'models.net' if c.__name__ == 'FullNet' else 'models.cond.sub'
    raw = _save_under_foreign_module_names(model, rename)
    names = pickle_compat.pickle_globals(raw)
    assert ('models.net', 'FullNet') in names and ('models.cond.sub', 'ConditionalNet') in names
    assert ('layers.misc.custom_conv_layers', 'CustomConvLayer') in names
    assert pickle_compat.unresolved(raw) == []
    (tmp_path / '0_model.pt').write_bytes(raw)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(model_management, 'attach_arithmetic_coders', lambda m, d=None: m)  # (the coder's tables are GPU work)
    loaded = model_management.load_model(prefix='0_', on_cpu=True)
    assert type(loaded).__module__ == 'aivc_amd.models.full_net'
    sd_a, sd_b = model.state_dict(), loaded.state_dict()
    assert sd_a.keys() == sd_b.keys() and all(torch.equal(sd_a[k], sd_b[k]) for k in sd_a)
    # the command-line inspector over the same file
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'inspect_pickle.py'), '0_model.pt'],
                         capture_output=True, text=True)
    assert out.returncode == 0 and 'models.net.FullNet' in out.stdout and 'by NAME -> aivc_amd.models.full_net.FullNet' in out.stdout
    # a class this build does not define: named in the error, before anything is unpickled
    foo = type('FooBNet', (type(model),), {'__module__': 'aivc_amd.models.full_net'})
    model.__class__ = foo
    raw2 = _save_under_foreign_module_names(model, lambda c: 'models.net' if c is foo else rename(c))
    (tmp_path / '1_model.pt').write_bytes(raw2)
    with pytest.raises(ImportError, match='models.net.FooBNet'):
        model_management.load_model(prefix='1_', on_cpu=True)
    # protocol-4 qualified names of nested classes resolve by walking the attributes ...
    import collections
    assert pickle_compat.resolve('collections', 'OrderedDict.fromkeys') == collections.OrderedDict.fromkeys
    # ... and the by-name fallback only applies under the reference's own packages: a third-party module that happens
    # to name a class like one of ours stays unresolved instead of binding to the local class
    assert pickle_compat.resolve('models.anything', 'FullNet') is type(loaded)
    assert pickle_compat.resolve('src.models.anything', 'FullNet') is type(loaded)
    with pytest.raises(AttributeError):
        pickle_compat.resolve('somebody_elses_pkg.nets', 'FullNet')


def test_distributed_watchdog_names_the_wait(capfd, monkeypatch):
    """a host-side wait on communication that lasts longer than AIVC_DIST_WARN_S is reported once, with the wait's name
    and the collectives issued before it (aivc_amd/parallel.py: under RCCL a missing peer only shows at the next host
    synchronisation, far from its cause)"""
    import time
    from aivc_amd import parallel
    monkeypatch.setenv('AIVC_DIST_WARN_S', '0.2')
    monkeypatch.setitem(parallel._WATCH, 'thread', None)
    parallel._start_watchdog()
    parallel._note('all_gather level reconstructions')
    with parallel._host_wait('level reconstructions'):
        time.sleep(0.8)
    err = capfd.readouterr().err
    assert err.count('[aivc_amd.parallel]') == 1 and '"level reconstructions"' in err and 'all_gather level reconstructions' in err
    with parallel._host_wait('quick'):
        pass
    time.sleep(0.3)
    assert '[aivc_amd.parallel]' not in capfd.readouterr().err


def test_unit_lengths_of_a_container_with_mixed_coding_structures():
    """decode_video_sharded places the gathered frames by every unit's OWN length (a container may mix GOP structures:
    decode_video / decode_units accept that) -- partial.unit_lengths has them from the names in the GOP headers"""
    from aivc_amd import partial
    from aivc_amd.real_life import cat_binary_files as container
    from aivc_amd.real_life import header as hdr
    frame = (0).to_bytes(4, 'big') * 2 + (1).to_bytes(4, 'big') + b'z' + (1).to_bytes(4, 'big') + b'\x00'
    gops = [container.pack_gop(hdr.gop_header_bytes(name, 0.), [frame] * n) for name, n in (('1_GOP_2', 3), ('1_GOP_4', 5), ('LDP_2', 3))]
    dd = {'x': (48, 80), 'y': (3, 5), 'z': (1, 2)}
    blob = container.pack_video(hdr.video_header_bytes(dd, len(gops), 0, 10), gops)
    assert partial.unit_lengths(partial.indexed_from_blob(blob).names) == [3, 5, 3]


def test_truncated_container_is_an_error_not_garbage():
    """every length prefix of the container is checked against the data at hand: a short file raises ContainerError naming
    the record (the reference's fixed-size reads would carry on with what they got, src/real_life/decode.py:329-426)"""
    from aivc_amd.real_life import cat_binary_files as container
    from aivc_amd.real_life import header as hdr
    from aivc_amd.real_life.bitstream import split_sections
    frame = (0).to_bytes(4, 'big') * 2 + (3).to_bytes(4, 'big') + b'abc' + (1).to_bytes(4, 'big') + b'\x00'
    gop = container.pack_gop(hdr.gop_header_bytes('1_GOP_2', 0.), [frame] * 3)
    blob = container.pack_video(hdr.video_header_bytes({'x': (48, 80), 'y': (3, 5), 'z': (1, 2)}, 2, 0, 5), [gop, gop])
    assert len(container.unpack_video(blob)[3]) == 2 and len(container.unpack_gop(gop)[2]) == 3
    for cut in (5, 17, 20, len(blob) - 1, len(blob) - len(gop) + 3):
        with pytest.raises(container.ContainerError):
            container.unpack_video(blob[:cut])
    with pytest.raises(container.ContainerError, match='frame 2 of 3'):
        container.unpack_gop(gop[:-4])
    with pytest.raises(container.ContainerError, match='codecnet_y'):
        split_sections(frame[:-1])
    assert split_sections(frame) == [b'', b'', b'abc', b'\x00']
    # the path API reads a section back while the later ones are not written yet (src/real_life/bitstream.py:333-350)
    assert split_sections(frame[:-5], upto=3) == [b'', b'', b'abc']


def test_rows_of_is_a_view_for_consecutive_rows():
    """codec._rows_of: the decoded latents of a synthesis batch are a view of the entropy stage's batch tensor when its
    frames sit in consecutive rows, a copy otherwise -- the same values either way"""
    import torch
    from aivc_amd.codec import _rows_of
    t = torch.arange(5 * 2 * 3 * 4, dtype=torch.float32).reshape(5, 2, 3, 4)
    u = torch.arange(100, 100 + 2 * 2 * 3 * 4, dtype=torch.float32).reshape(2, 2, 3, 4)
    v = _rows_of([(t, 1), (t, 2), (t, 3)])
    assert v.data_ptr() == t[1:].data_ptr() and v.shape == (3, 2, 3, 4) and torch.equal(v, t[1:4])
    c = _rows_of([(t, 3), (t, 1)])
    assert torch.equal(c, torch.stack([t[3], t[1]])) and c.data_ptr() != t[3:].data_ptr()
    m = _rows_of([(t, 4), (u, 0)])
    assert torch.equal(m, torch.stack([t[4], u[0]]))
    assert _rows_of([(u, 1)]).data_ptr() == u[1:].data_ptr()


def _fake_codec(c_y=8, md5=False):
    """what FrameCodec.check_sections / _entropy_bytes read of a codec: two networks with an ArithmeticCoder each"""
    from types import SimpleNamespace
    from aivc_amd.real_life.bitstream import ArithmeticCoder
    ac = SimpleNamespace(flag_md5sum=md5, _parse_maps=ArithmeticCoder._parse_maps)
    net = SimpleNamespace(ac=ac, nb_ft_y=c_y)
    return SimpleNamespace(mof=net, cod=SimpleNamespace(ac=ac, nb_ft_y=c_y))


def _frame(mof_y, cod_y):
    return b''.join(len(s).to_bytes(4, 'big') + s for s in (b'z', mof_y, b'z', cod_y))


def test_map_lists_of_every_frame_are_checked_before_any_rank_starts():
    """FrameCodec.check_sections: a y section whose map list is malformed is a ContainerError for the WHOLE container on
    the host (every rank holds the bitstream and fails alike) -- not only on the rank that decodes the frame"""
    from aivc_amd.codec import FrameCodec
    from aivc_amd.real_life import cat_binary_files as container
    good = _frame(b'\x02\x00\x03ab', b'\x01\x07c')
    parsed = [('1_GOP_2', 0., [_frame(b'', b'\x00'), good, good])]
    FrameCodec.check_sections(_fake_codec(), parsed)
    for bad in (_frame(b'\x02\x00', b'\x00'),          # two maps announced, one listed
                _frame(b'\x01\x09x', b'\x00'),         # map 9 of 8
                _frame(b'\x00', b''),                  # no map count at all
                _frame(b'\x00', b'\x09' + bytes(9))):  # more maps than the latent has
        with pytest.raises(container.ContainerError):
            FrameCodec.check_sections(_fake_codec(), [('1_GOP_2', 0., [_frame(b'', b'\x00'), good, bad])])
    # the I frame's MOFNet section is not read (nothing decodes it)
    FrameCodec.check_sections(_fake_codec(), [('1_GOP_2', 0., [_frame(b'\x63', b'\x00'), good, good])])
    # under flag_md5sum the list sits behind the 32 characters of the digest
    md5 = b'0' * 32
    FrameCodec.check_sections(_fake_codec(md5=True), [('1_GOP_2', 0., [_frame(b'', md5 + b'\x00')] + [_frame(md5 + b'\x01\x02q', md5 + b'\x00')] * 2)])


def test_entropy_memory_estimate_reads_the_map_count_behind_the_md5_text():
    from aivc_amd.codec import FrameCodec
    dd = {'x': (64, 64), 'y': (4, 4), 'z': (1, 1)}
    plain = [('1_GOP_0', 0., [_frame(b'', b'\x03\x00\x01\x02xyz')])]
    md5 = b'f' * 32  # ('f' = 102 as a map count)
    tagged = [('1_GOP_0', 0., [_frame(b'', md5 + b'\x03\x00\x01\x02xyz')])]
    a = FrameCodec._entropy_bytes(_fake_codec(), plain, [0], dd)
    b = FrameCodec._entropy_bytes(_fake_codec(md5=True), tagged, [0], dd)
    assert a == b == 3 * 16 * 134 + 16 * 4 * 640


def test_estimating_rate_restores_the_flag_when_the_body_raises():
    """encode() switches bitstream.ESTIMATE_RATE on through estimating_rate(): a body that raises leaves the flag at its
    previous value (for both previous values), so a failed encode does not leave every later launch_finalize of the
    process paying the rate kernels"""
    from aivc_amd.real_life import bitstream
    before = bitstream.ESTIMATE_RATE
    try:
        for previous in (False, True):
            bitstream.ESTIMATE_RATE = previous
            with pytest.raises(ZeroDivisionError):
                with bitstream.estimating_rate():
                    assert bitstream.ESTIMATE_RATE is True
                    1 / 0
            assert bitstream.ESTIMATE_RATE is previous
            with bitstream.estimating_rate():  # and on the success path
                assert bitstream.ESTIMATE_RATE is True
            assert bitstream.ESTIMATE_RATE is previous
    finally:
        bitstream.ESTIMATE_RATE = before


@pytest.mark.parametrize('sizes, align, slack', [([0, 1, 15, 16, 17], 16, 0), ([0, 3, 4, 5], 4, 8)])
def test_stage_layout(sizes, align, slack):
    """where ops._stage puts its arrays: each on an `align` boundary, `slack` spare bytes behind each, nothing overlapping.  The
    second case is the layout the range decoder's kernels were written against (they read past a payload's end): each payload
    padded to 4 bytes plus 8 spare ones, stated here with the formula range_decode used before it called the helper"""
    from aivc_amd import ops
    offs, total = ops._stage_layout(sizes, align, slack)
    if (align, slack) == (16, 0):
        assert offs == [0, 0, 16, 32, 48] and total == 80
    else:
        want, pos = [], 0
        for n in sizes:
            want.append(pos)
            pos += n + (-n) % 4 + 8
        assert offs == want == [0, 8, 20, 32] and total == max(pos, 4) == 48
    assert all(o % align == 0 for o in offs)
    ends = [o + n for o, n in zip(offs, sizes)]
    assert all(e + slack <= nxt for e, nxt in zip(ends, offs[1:] + [total]))  # in order, so: no two ranges share a byte
    assert ops._stage_layout([], 4, 8) == ([], 4)  # (range_decode of no stream still hands the kernels a buffer)


DECLARED_WITH_A_REF_TWIN = [
    'aivc_ssim_means', 'aivc_pool2x2', 'aivc_sq_err', 'aivc_conv2d', 'aivc_gdn_reparam', 'aivc_split_weights_bf16x3',
    'aivc_winograd_weights', 'aivc_winograd_weights_poly5', 'aivc_winograd_weights_tconv5', 'aivc_pad_channels',
    'aivc_yuv420_to_444', 'aivc_yuv420u8_to_444', 'aivc_pack_images', 'aivc_conv_images', 'aivc_frame_to_yuv420',
    'aivc_downsample2x', 'aivc_warp_blend', 'aivc_warp_blend_rows', 'aivc_warp', 'aivc_hyper_params', 'aivc_channel_gain',
    'aivc_gain_interp', 'aivc_quantize_center', 'aivc_dequantize', 'aivc_balle_cdf_table', 'aivc_nonzero_maps',
    'aivc_nonzero_maps_batch', 'aivc_laplace_cdf_rows', 'aivc_laplace_cdf_windows', 'aivc_laplace_bounds', 'aivc_table_bounds',
    'aivc_range_encode', 'aivc_range_decode', 'aivc_range_decode_windows', 'aivc_scatter_symbols',
    'aivc_laplace_cdf_windows_batch', 'aivc_laplace_bounds_batch', 'aivc_table_bounds_batch', 'aivc_scatter_symbols_batch',
    'aivc_bounds_rate', 'aivc_rate_bits', 'aivc_laplace_prob', 'aivc_table_prob', 'aivc_metrics_workspace', 'aivc_abi_version']
DECLARED_ON_THE_DEVICE_ONLY = [
    'aivc_conv2d_variant', 'aivc_selfcheck_gdn_math', 'aivc_detmath_eval', 'aivc_diag_hold_lds', 'aivc_warp_modes',
    'aivc_rgb8_to_yuv420u8', 'aivc_yuv8_to_rgb8', 'aivc_frame_sse_u8', 'aivc_frame_aux_stats', 'aivc_channel_gain_rows',
    'aivc_quantize_center_rows', 'aivc_dequantize_rows', 'aivc_md5_batch', 'aivc_pair_sad_u8', 'aivc_resize_u8']


def test_declare_binds_these_names_and_no_others():
    """abi.declare on a stand-in library that records what is looked up: the device library is asked for every name of the two
    lists, the oracle ('_ref') for the first list's twins only, and each bound entry carries its stream argument"""
    from aivc_amd import abi

    class Fn:
        pass

    class Lib:
        def __init__(self):
            self.asked = {}

        def __getattr__(self, name):
            return self.asked.setdefault(name, Fn())

    for suffix, names in (('', DECLARED_WITH_A_REF_TWIN + DECLARED_ON_THE_DEVICE_ONLY), ('_ref', DECLARED_WITH_A_REF_TWIN)):
        lib = Lib()
        fns = abi.declare(lib, suffix)
        assert sorted(fns) == sorted(names) and len(set(names)) == len(names)
        assert sorted(lib.asked) == sorted(n + suffix for n in names)
        assert all(fns[n] is lib.asked[n + suffix] for n in names)
    assert fns['aivc_conv2d'].argtypes == [ctypes.POINTER(abi.ConvParams), ctypes.c_void_p] and fns['aivc_conv2d'].restype is ctypes.c_int
    assert fns['aivc_metrics_workspace'].argtypes == [ctypes.c_int32] * 3 and fns['aivc_metrics_workspace'].restype is ctypes.c_size_t
    assert fns['aivc_abi_version'].argtypes == []
    dev = abi.declare(Lib())
    assert dev['aivc_conv2d_variant'].argtypes == [ctypes.POINTER(abi.ConvParams)]  # (no stream: nothing is launched)
    assert dev['aivc_detmath_eval'].argtypes == abi.DETMATH_EVAL_ARGS + [ctypes.c_void_p]
    assert dev['aivc_md5_batch'].argtypes == abi.DIGEST_PROTOTYPES['aivc_md5_batch'] + [ctypes.c_void_p]
