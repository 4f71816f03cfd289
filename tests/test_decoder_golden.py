"""Decoder dataflow, section framing and the md5 debug format pinned against fixtures produced by RUNNING the
reference's own code (tools/gen_golden_decoder.py): ArithmeticCoder.encode wrote every section
(src/real_life/bitstream.py:186-304), cat_one_gop / cat_one_video wrapped them, decode_one_video ->
decode_one_GOP -> Decoder.decode (src/real_life/decode.py:44-898) produced the PNG planes.  The only part not
from the reference is the torchac arithmetic (oracle coder behind a stub: "parity unpinned") and the
motion-compensation one-liner of the missing models package.

CPU half: the oracle against the fixtures.  GPU half (-m gpu): the HIP product path against the same fixtures,
with no oracle in between."""
import ast
import hashlib

import numpy as np
import pytest
import torch

from oracle import codec as ocodec
from oracle import spec as ospec

# decoder_big_gop8: 200 x 136, hierarchical 1_GOP_8, 16 + 5 coded maps, z 3 x 4, h_s output cropped; the variants:
# no shortcut transform + empty MOFNet y sections, no P / B gain matrices (tests/decoder_variants.py)
# decoder_b_*: a second draw of the small model (another seed, 3 + 4 coded maps): 1_GOP_4 with a fractional rate index,
# LDP_8 from frame 3 on an odd-sized frame, and 1_GOP_8 at 128 x 96 decoded FREE-RUNNING (the second seed tried: the first
# desynchronised, which the fixture's search log records)
CASES = ['decoder_ra', 'decoder_ra_chained', 'decoder_ldp_odd', 'decoder_big_gop8', 'decoder_noref_empty_y',
         'decoder_gain_i', 'decoder_b_gop4', 'decoder_b_ldp8', 'decoder_b_mid_gop8', 'decoder_mid_gop8',
         'decoder_default_gop2', 'decoder_default_i']
# decoder_mid_gop8: MID widths (n2 32, n 64, c_y = c_short = c_z = 32, n_h 64: c_in % 32 == 0 on every layer behind the
# image layers, i.e. the LDS-DMA K loop, fused-GDN / fused-tail tiles and the thin MFMA kernel carry the decode), 1_GOP_8 at
# 128 x 96, 20 + 6 coded maps, writer's sigma; its 3.2 M parameters are seeded (decoder_variants.seeded_init), not stored
# decoder_default_*: the DEFAULT widths (aivc_amd.models.arch.DEFAULT_WIDTHS, seeded, 2 + 3 coded maps) at sizes where version 2 of
# the contract (fp32w) routes launches to the Winograd chains with its size rule in force: 1_GOP_2 at 448 x 320 (I, P, B: 301 on the
# 3x3 128 -> 128 convs at 1/4 resolution, 302 on g_a_ref's 5x5 stride-2 64 -> 128 layer) and one intra frame at 1024 x 576 (303 on
# the UpscalingLayer(5, 128 -> 64) at 1/4 resolution, and 301).  Writer's sigma (both desynchronise free-running); q and sigma are
# stored on the coded maps only (lat_*_maps)
WINO_LIVE = {'decoder_default_gop2': {301, 302}, 'decoder_default_i': {301, 303}}
TEACHER_CASES = ['decoder_big_gop8', 'decoder_mid_gop8', 'decoder_default_gop2', 'decoder_default_i']
NAMES = ('mofnet', 'codecnet')


def _meta(g):
    return ast.literal_eval(str(g['meta']))


def _model(golden, case='decoder_ra', device=None):
    """this repo's FullNet carrying the weights of the reference model the case was written with (strict state_dict
    load: the names match), then the case's variant edits"""
    from aivc_amd.model_mngt.model_management import attach_arithmetic_coders
    from aivc_amd.models.full_net import FullNet
    from decoder_variants import apply_variant
    cm = _meta(golden(case))
    g = golden(cm.get('model', 'decoder_model'))
    m = _meta(g)
    model = FullNet({'widths': m['widths'], 'nb_rates': m['nb_rates']})
    if m.get('seeded'):
        from decoder_variants import seeded_init
        assert seeded_init(model, m['seed'], m['active_y'], m['weight_grid']) == m['sha256'], \
            'the seeded draw no longer reproduces the parameters the reference ran on'
    else:
        sd = {k[3:]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith('sd.')}
        missing, unexpected = model.load_state_dict(sd, strict=True)
        assert not missing and not unexpected
    model = apply_variant(model, cm.get('variant', {})).eval()
    if device is not None:
        model = attach_arithmetic_coders(model.to(device))
    return model


def _lat(g, idx, name, what, fill=1.0):
    """latent `what` (z, q, sigma) of frame idx's `name`, NCHW as the reference computed it.  Fixtures written with
    lat_*_maps store q and sigma only on the maps the y section codes: q is 0 on the others, sigma (which the stream does not
    use there) is set to `fill` (a scalar, or an NCHW array of the full shape to take those maps from)"""
    a = np.asarray(g['lat_%d_%s_%s' % (idx, name, what)])
    key = 'lat_%d_%s_maps' % (idx, name)
    if what == 'z' or key not in g.files:
        return a
    maps = np.asarray(g[key])
    shape = (a.shape[0], _meta(g)['coded_maps_of'], a.shape[2], a.shape[3])  # (coded_maps_of: the model's c_y)
    full = np.zeros(shape, a.dtype) if what == 'q' else np.broadcast_to(np.asarray(fill, a.dtype), shape).copy()
    full[:, maps] = a
    return full


def _coded(g, idx, name):
    """indices of the y maps frame idx's section of `name` codes, or None where the fixture stores every map"""
    key = 'lat_%d_%s_maps' % (idx, name)
    return np.asarray(g[key]) if key in g.files else None


def _ref_sigma(g, idx, name, own=None):
    """sigma the reference wrote frame idx's y section of `name` with, NHWC; on maps the fixture does not store (not coded),
    the decoder's own sigma `own` (NHWC)"""
    fill = 1.0 if own is None else np.transpose(own, (0, 3, 1, 2))
    return np.ascontiguousarray(np.transpose(_lat(g, idx, name, 'sigma', fill), (0, 2, 3, 1)))


def _pixel_budget(m, frames):
    """differing pixels tolerated (all within 1 LSB): rounding ties only on the small cases (0 as generated); the
    200 x 136 GOP8 case accumulates last-bit differences of the two conv arithmetics over 9 frames (251 pixels of
    367 200 as generated)"""
    total = sum(f[k].size for f in frames for k in 'yuv')
    # free-running: rounding ties (0 as generated on the small cases, 4 of 165 888 on the 128 x 96 GOP8 one)
    return max(4, total // 20000) if not m.get('teacher_sigma') else total // 500


def _frames(g, m, prefix):
    return [{k: np.asarray(g['%s_%d_%s' % (prefix, m['first'] + i, k)]) for k in 'yuv'} for i in range(m['n'])]


def _sections_from_latents(g, idx, net_spec, name, md5=False):
    """restated framing of one conditional coder's two sections from the reference's own latents"""
    from oracle import oracle as O
    z, q, sigma = (_lat(g, idx, name, what) for what in ('z', 'q', 'sigma'))
    nhwc = lambda a: np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))
    table, _ = O.balle_cdf_table(net_spec['balle'])
    sz = ocodec._z_section(table, nhwc(z).astype(np.int16))
    sy = ocodec._y_section(nhwc(sigma), nhwc(q).astype(np.int16))
    if md5:
        sz = _savetxt_md5(z) + sz
        sy = _savetxt_md5(q) + sy
    return sz, sy


def _savetxt_md5(x_nchw):
    """what the reference computes under flag_md5sum (bitstream.py:229-234): md5 of np.savetxt of the latent"""
    import io
    buf = io.BytesIO()
    np.savetxt(buf, x_nchw.astype(np.int16).astype(int).flatten())
    return hashlib.md5(buf.getvalue()).hexdigest().encode()


# ---- CPU: oracle vs reference -----------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_reference_said_lossless(case, golden):
    g = golden(case)
    m = _meta(g)
    gop = ocodec.gop_struct(m['gop'])
    n_sections = sum(2 if gop[i % len(gop)][0] == 0 else 4 for i in range(m['n']))
    # every section was written twice (plain + md5 variant), each decode-back said "lossless"
    assert int(g['ref_log_counts'][0]) == 2 * n_sections and int(g['ref_log_counts'][1]) == n_sections
    assert int(g['cdf_stats'][3]) == 0  # same sigma: both CDF arithmetics agree on every coded bound


@pytest.mark.parametrize('case', CASES)
def test_container_holds_reference_frames(case, golden):
    g = golden(case)
    m = _meta(g)
    blob = np.asarray(g['video_file']).tobytes()
    v = [int.from_bytes(blob[i:i + 2], 'big') for i in range(0, 18, 2)]
    dd = m['data_dim']
    assert tuple(v[:6]) == dd['x'] + dd['y'] + dd['z'] and v[7] == m['first'] and v[8] == m['first'] + m['n'] - 1
    unit = len(ocodec.gop_struct(m['gop']))
    idx = m['first']
    for gb in ocodec.split_lp(blob, 18, v[6]):
        assert gb[:6] == ocodec.gop_header(m['gop'], m['idx_rate'])
        for fb in ocodec.split_lp(gb, 6, unit):
            assert fb == np.asarray(g['frame_%d' % idx]).tobytes()
            idx += 1


@pytest.mark.parametrize('case', CASES)
def test_oracle_framing_equals_reference_encode(case, oracle, golden):
    """sections restated from the reference's latents == bytes its ArithmeticCoder.encode wrote, plain and md5"""
    g = golden(case)
    m = _meta(g)
    spec = ospec.export_model(_model(golden, case))
    gop = ocodec.gop_struct(m['gop'])
    for i in range(m['n']):
        idx = m['first'] + i
        ftype = gop[i % len(gop)][0]
        for md5, key in ((False, 'frame_%d'), (True, 'md5frame_%d')):
            secs = [None, None]
            if ftype != ocodec.FRAME_I:
                secs = list(_sections_from_latents(g, idx, spec['mof'], 'mofnet', md5))
            secs += list(_sections_from_latents(g, idx, spec['cod'], 'codecnet', md5))
            frame = b''.join(ocodec.be(0, 4) if s is None else ocodec.lp(s) for s in secs)
            assert frame == np.asarray(g[key % idx]).tobytes(), (case, idx, md5)


@pytest.mark.parametrize('case', CASES)
def test_oracle_decode_equals_reference_decoder(case, oracle, golden):
    g = golden(case)
    m = _meta(g)
    spec = ospec.export_model(_model(golden, case))
    hook, worst = None, [0.0]
    if m.get('teacher_sigma'):
        # streams of this size written on torch's conv arithmetic: the CDFs are built from the writer's sigma, the
        # oracle's own sigma is held against it (oracle/codec.py cond_decode)
        def hook(idx, name, sigma):
            ref = _ref_sigma(g, idx, name, sigma)
            worst[0] = max(worst[0], float(np.abs(sigma / ref - 1).max()))
            return ref
    dec = ocodec.decode_video(spec, np.asarray(g['video_file']).tobytes(), hook)
    assert worst[0] < 2e-6
    want = _frames(g, m, 'dec')
    assert len(dec) == m['n']
    n_off = 0
    for d, w in zip(dec, want):
        for k in 'yuv':
            diff = np.abs(d[k].astype(np.int32) - w[k].astype(np.int32))
            assert diff.max() <= 1, (case, k)  # north_star: within 1 LSB of the reference
            n_off += int((diff != 0).sum())
    assert n_off <= _pixel_budget(m, want)


@pytest.mark.parametrize('case', TEACHER_CASES)
def test_free_running_statistic_of_teacher_sigma_cases(case, oracle, golden):
    """The writer's-sigma cases, decoded WITHOUT the writer's sigma: the outcome (desynchronised: how many pixels
    differ, by how much) was recorded by the generator in the model fixture's search log; the deterministic oracle must
    reproduce exactly that record, so a change of the sigma path that makes free-running decodes better or worse
    shows up here instead of hiding behind the teacher"""
    g = golden(case)
    m = _meta(g)
    assert m['teacher_sigma']
    log = ast.literal_eval(str(golden(m['model'])['search_log']))
    rec = [st for seed, name, ok, st in log if name == case and ok][-1]['free_running']
    spec = ospec.export_model(_model(golden, case))
    try:
        dec = ocodec.decode_video(spec, np.asarray(g['video_file']).tobytes(), None)
    except Exception as e:  # a desynchronised stream can run the coder out of its alphabet
        assert 'error' in rec, (rec, repr(e))
        return
    want = _frames(g, m, 'dec')
    worst = n_diff = n_equal = 0
    for d, w in zip(dec, want):
        same = True
        for k in 'yuv':
            diff = np.abs(d[k].astype(np.int32) - w[k].astype(np.int32))
            worst = max(worst, int(diff.max()))
            n_diff += int((diff != 0).sum())
            same &= not diff.any()
        n_equal += same
    assert {'max_abs_lsb': worst, 'n_pixels_differ': n_diff, 'frames_equal': n_equal} == rec


@pytest.mark.parametrize('case', CASES)
def test_oracle_latents_equal_reference(case, oracle, golden):
    """entropy stage alone: z, then q_y through the oracle's own h_s / sigma / CDF rows"""
    from oracle import oracle as O
    g = golden(case)
    m = _meta(g)
    spec = ospec.export_model(_model(golden, case))
    gop = ocodec.gop_struct(m['gop'])
    dy, dz = m['data_dim']['y'], m['data_dim']['z']
    for i in range(m['n']):
        idx = m['first'] + i
        sec = ocodec.split_lp(np.asarray(g['frame_%d' % idx]).tobytes(), 0, 4)
        for k, name in enumerate(NAMES):
            if name == 'mofnet' and gop[i % len(gop)][0] == ocodec.FRAME_I:
                assert sec[0] == b'' and sec[1] == b''
                continue
            net = spec['mof' if name == 'mofnet' else 'cod']
            table, _ = O.balle_cdf_table(net['balle'])
            npz, npy = dz[0] * dz[1], dy[0] * dy[1]
            sym = O.range_decode(sec[2 * k], table, net['c_z'] * npz, plane=npz)
            q_z = O.scatter_symbols(sym, npz, net['c_z'], list(range(net['c_z']))).reshape(1, dz[0], dz[1], -1)
            np.testing.assert_array_equal(np.transpose(q_z, (0, 3, 1, 2)), g['lat_%d_%s_z' % (idx, name)])
            mu, sigma = O.hyper_params(O.run_layer(net['h_s'], O.dequantize(q_z)), net['c_y'], dy[0], dy[1])
            coded = _coded(g, idx, name)
            own = np.transpose(sigma, (0, 3, 1, 2))
            np.testing.assert_allclose(own if coded is None else own[:, coded], g['lat_%d_%s_sigma' % (idx, name)], rtol=2e-6)
            if m.get('teacher_sigma'):
                sigma = _ref_sigma(g, idx, name, sigma)
            sy = sec[2 * k + 1]
            maps = list(sy[1:1 + sy[0]])
            q_y = np.zeros((npy, net['c_y']), np.int16)
            if maps:
                sym = O.range_decode(sy[1 + sy[0]:], O.laplace_cdf_rows(sigma, maps), len(maps) * npy)
                q_y = O.scatter_symbols(sym, npy, net['c_y'], maps)
            if coded is not None:
                assert list(coded) == maps  # the fixture's coded maps are the ones the section lists
            np.testing.assert_array_equal(np.transpose(q_y.reshape(1, dy[0], dy[1], -1), (0, 3, 1, 2)),
                                          _lat(g, idx, name, 'q'))



def _oracle_conv_launches(monkeypatch):
    """record the parameters of every oracle.conv2d call (the whole conv family of a decode: oracle.run_layer) as a
    list of abi.ConvParams with stand-in pointers, shaped as aivc_amd.ops.conv2d issues the same layer (stored channel
    counts; x, w 16-byte aligned, bias given)"""
    from aivc_amd import abi
    from oracle import oracle as O
    seen, orig = [], O.conv2d

    def rec(x, w_ohwi, bias=None, mode=abi.MODE_CONV, stride=1, pad=0, act1=0, act2=0, mul=None, res=None, gdn=None,
            cmap=None, tail=None):
        n, h, w, c = x.shape
        c = (max(cmap) + 4) // 4 * 4 if cmap is not None else (c + 3) // 4 * 4
        co, k = w_ohwi.shape[0], w_ohwi.shape[1]
        ho, wo = abi.conv_out_size(mode, h, w, k, stride, pad)
        a = 1 << 20
        p = abi.ConvParams(mode, k, stride, pad, n, h, w, c, ho, wo, co, act1, act2, abi.ALGO_AUTO,
                           0 if gdn is None else (2 if gdn[2] else 1), 0, a, 2 * a, 3 * a, 4 * a if mul is not None else None,
                           5 * a if res is not None else None, 6 * a, 7 * a if gdn is not None else None,
                           8 * a if gdn is not None else None)
        if tail is not None:
            p.tail_w, p.tail_bias, p.tail_c_out = 9 * a, 10 * a, tail[0].shape[0]
        p.precision = abi.PREC_FP32_WINO
        seen.append(p)
        return orig(x, w_ohwi, bias, mode=mode, stride=stride, pad=pad, act1=act1, act2=act2, mul=mul, res=res, gdn=gdn,
                    cmap=cmap, tail=tail)
    monkeypatch.setattr(O, 'conv2d', rec)
    return seen


def _variant_codes(launches):
    """the aivc_conv2d_variant code of each launch; a fused gdn / tail the kernels decline is asked again as the first of
    the two launches the product issues instead (aivc_amd/ops.py _two_launches)"""
    import ctypes
    from aivc_amd import _lib, abi
    variant = _lib.load()['aivc_conv2d_variant']
    codes = []
    for p in launches:
        v = variant(ctypes.byref(p))
        if v < 0 and (p.gdn or p.tail_c_out):
            h = abi.ConvParams.from_buffer_copy(p)
            h.gdn, h.gdn_beta, h.gdn_gamma = 0, None, None
            if p.tail_c_out:
                h.tail_w, h.tail_bias, h.tail_c_out, h.res, h.act2 = None, None, 0, None, 0
            v = variant(ctypes.byref(h))
        codes.append(v)
    return codes


@pytest.mark.parametrize('case', sorted(WINO_LIVE))
def test_winograd_variants_are_live_in_the_default_cases(case, oracle, golden, monkeypatch):
    """The default-width cases exist to run the decode through version 2's Winograd chains with the size rule in force: the
    conv launches of the oracle's decode, asked of the library's own routing (aivc_conv2d_variant, no WINO_ANY_SIZE), take
    exactly the expected Winograd codes.  Raising AIVC_WINO_MIN_PIXELS*, or shrinking a case, fails here, not silently."""
    g = golden(case)
    m = _meta(g)
    assert m['teacher_sigma'] and not oracle.WINO_ANY_SIZE
    spec = ospec.export_model(_model(golden, case))
    launches = _oracle_conv_launches(monkeypatch)
    dec = ocodec.decode_video(spec, np.asarray(g['video_file']).tobytes(), lambda idx, name, sigma: _ref_sigma(g, idx, name, sigma))
    assert len(dec) == m['n'] and launches
    codes = _variant_codes(launches)
    assert all(c >= 0 for c in codes), codes
    assert set(codes) & {301, 302, 303} == WINO_LIVE[case], sorted(set(codes))

def test_md5_text_format(golden):
    """the product's latent_md5 == the 32 bytes the reference's compute_md5sum put in front of the sections"""
    from aivc_amd.real_life.bitstream import latent_md5
    g = golden('decoder_ra')
    m = _meta(g)
    for i in range(m['n']):
        idx = m['first'] + i
        sec = ocodec.split_lp(np.asarray(g['md5frame_%d' % idx]).tobytes(), 0, 4)
        for k, name in enumerate(NAMES):
            if not sec[2 * k]:
                continue
            for s, lat in ((sec[2 * k], 'z'), (sec[2 * k + 1], 'q')):
                x = torch.from_numpy(np.asarray(g['lat_%d_%s_%s' % (idx, name, lat)]))
                assert latent_md5(x.permute(0, 2, 3, 1).to(torch.int16)) == s[:32]


# ---- GPU: HIP product path vs reference (no oracle involved) --------------------------------------------------
def _teach_sigma(model, g, m, monkeypatch):
    """teacher_sigma cases: ArithmeticCoder.decode_y gets the sigma the reference wrote each y section with (found
    by the section's payload), after the product's own sigma has been held against it"""
    if not m.get('teacher_sigma'):
        return
    gop_len = len(ocodec.gop_struct(m['gop']))
    for k, (name, net) in enumerate((('mofnet', model.mode_net.mode_net), ('codecnet', model.codec_net.codec_net))):
        table = {}
        for i in range(m['n']):
            idx = m['first'] + i
            sy = ocodec.split_lp(np.asarray(g['frame_%d' % idx]).tobytes(), 0, 4)[2 * k + 1]
            if len(sy) > 1:  # (the writer's sigma, NHWC, on the maps the fixture stores: all, or the coded ones)
                table[bytes(sy)] = (np.transpose(np.asarray(g['lat_%d_%s_sigma' % (idx, name)]), (0, 2, 3, 1)),
                                    _coded(g, idx, name))
        assert len(table) == m['n'] - (m['n'] // gop_len if name == 'mofnet' else 0)
        orig = net.ac.decode_y

        def patched(payloads, sigma, _orig=orig, _table=table):
            sigma = sigma.clone()
            for j, p in enumerate(payloads):
                entry = _table.get(bytes(p))
                if entry is not None:
                    ref = torch.from_numpy(np.ascontiguousarray(entry[0])).to(sigma.device)
                    maps = slice(None) if entry[1] is None else torch.from_numpy(entry[1].astype(np.int64)).to(sigma.device)
                    assert float((sigma[j:j + 1, :, :, maps] / ref - 1).abs().max()) < 2e-6
                    sigma[j:j + 1, :, :, maps] = ref
            return _orig(payloads, sigma)
        monkeypatch.setattr(net.ac, 'decode_y', patched)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_hip_decode_video_equals_reference_decoder(case, cuda, golden, monkeypatch):
    g = golden(case)
    m = _meta(g)
    model = _model(golden, case, cuda)
    _teach_sigma(model, g, m, monkeypatch)
    fc = model.frame_codec()
    with torch.no_grad():
        dec, data_dim, first, last = fc.decode_video(np.asarray(g['video_file']).tobytes(), cuda)
    assert (first, last) == (m['first'], m['first'] + m['n'] - 1)
    assert {k: tuple(v) for k, v in data_dim.items()} == m['data_dim']
    n_off = 0
    for d, w in zip(dec, _frames(g, m, 'dec')):
        for k in 'yuv':
            diff = np.abs(d[k][0].cpu().numpy().astype(np.int32) - w[k].astype(np.int32))
            assert diff.max() <= 1, (case, k)
            n_off += int((diff != 0).sum())
    assert n_off <= _pixel_budget(m, _frames(g, m, 'dec'))
    assert fc.stream_errors() == []  # every section's bit count accounts for its payload: decoded on the writer's track


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(WINO_LIVE))
def test_hip_decode_in_version_2_where_it_is_live(case, cuda, golden, monkeypatch):
    """The shipped decode path in the default contract (fp32w, size rule in force) on the reference-written default-width
    streams: the launches take the Winograd kernels the case is sized for (301 / 302 / 303; union over the cases: all three),
    and the planes still meet the reference within 1 LSB inside the pixel budget, on the writer's track."""
    from aivc_amd import abi, ops
    assert ops.PRECISION == abi.PREC_FP32_WINO and not ops.WINO_ANY_SIZE
    g = golden(case)
    m = _meta(g)
    model = _model(golden, case, cuda)
    _teach_sigma(model, g, m, monkeypatch)
    fc = model.frame_codec()
    ops.PROFILE = []
    try:
        with torch.no_grad():
            dec, _, first, last = fc.decode_video(np.asarray(g['video_file']).tobytes(), cuda)
        torch.cuda.synchronize()
        codes = [rec[0] for rec in ops.PROFILE]
    finally:
        ops.PROFILE = None
    wino = {c: codes.count(c) for c in sorted(set(codes) & set(ops._WINO_VARIANTS))}
    print('\n%s: Winograd launches %s of %d conv launches' % (case, wino, len(codes)))
    assert set(wino) == WINO_LIVE[case]
    assert (first, last) == (m['first'], m['first'] + m['n'] - 1)
    want = _frames(g, m, 'dec')
    n_off = 0
    for d, w in zip(dec, want):
        for k in 'yuv':
            diff = np.abs(d[k][0].cpu().numpy().astype(np.int32) - w[k].astype(np.int32))
            assert diff.max() <= 1, (case, k)
            n_off += int((diff != 0).sum())
    assert n_off <= _pixel_budget(m, want)
    assert fc.stream_errors() == []


def test_default_cases_make_every_winograd_variant_live():
    assert set().union(*WINO_LIVE.values()) == {301, 302, 303}

@pytest.mark.gpu
@pytest.mark.parametrize('case', TEACHER_CASES)
def test_hip_free_running_desync_is_reported(case, cuda, golden):
    """The reference-written streams of the writer's-sigma cases decoded WITHOUT the writer's sigma: this build's h_s
    differs from torch's in the last bits of sigma, some coded symbol meets a flipped CDF bound and the range decoder
    leaves the writer's track (tests above: test_free_running_statistic_of_teacher_sigma_cases) -- silently, as with
    torchac.  The product's length check must say so."""
    g = golden(case)
    model = _model(golden, case, cuda)
    fc = model.frame_codec()
    with torch.no_grad():
        fc.decode_video(np.asarray(g['video_file']).tobytes(), cuda)
    errs = fc.stream_errors()
    assert errs and all(e[1] == 'y latent' for e in errs)  # z sections (integer table) always decode


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_hip_frame_decoder_per_frame(case, cuda, golden, monkeypatch):
    """Decoder.decode one frame at a time with the REFERENCE's reconstructions as references (no drift)"""
    from aivc_amd.func_util.GOP_structure import generate_gop_struct
    g = golden(case)
    m = _meta(g)
    model = _model(golden, case, cuda)
    _teach_sigma(model, g, m, monkeypatch)
    fc = model.frame_codec()
    gop = generate_gop_struct(m['gop'])
    want = _frames(g, m, 'dec')
    dd = dict(m['data_dim'])
    dev = lambda p: None if p is None else {k: torch.from_numpy(p[k])[None].to(cuda) for k in 'yuv'}
    for i in range(m['n']):
        u0 = i - i % len(gop)
        d = gop['frame_%d' % (i % len(gop))]
        ref = lambda nm: None if nm is None else want[u0 + int(nm.split('_')[-1])]
        with torch.no_grad():
            out = fc.decode_frame(np.asarray(g['frame_%d' % (m['first'] + i)]).tobytes(), dev(ref(d['prev_ref'])),
                                  dev(ref(d['next_ref'])), d['type'], dd, m['idx_rate'], cuda)
        for k in 'yuv':
            diff = np.abs(out[k][0].cpu().numpy().astype(np.int32) - want[i][k].astype(np.int32))
            assert diff.max() <= 1, (case, i, k)


@pytest.mark.gpu
@pytest.mark.parametrize('md5', [False, True])
@pytest.mark.parametrize('case', CASES)
def test_hip_arithmetic_coder_path_api(case, md5, cuda, golden, tmp_path, capsys):
    """ArithmeticCoder.encode / .decode with the reference's signatures: the files this repo writes from the
    reference's latents are byte-identical to the ones the reference wrote, and decode back to them."""
    from aivc_amd.func_util.GOP_structure import generate_gop_struct
    g = golden(case)
    m = _meta(g)
    model = _model(golden, case, cuda)
    gop = generate_gop_struct(m['gop'])
    nets = {'mofnet': model.mode_net.mode_net, 'codecnet': model.codec_net.codec_net}
    for i in range(m['n']):
        idx = m['first'] + i
        path = str(tmp_path / str(idx))
        lat = lambda name, what: torch.from_numpy(np.ascontiguousarray(_lat(g, idx, name, what))).to(cuda)
        names = NAMES if gop['frame_%d' % (i % len(gop))]['type'] != 0 else NAMES[1:]
        for name in names:
            common = {'bitstream_path': path, 'flag_debug': True, 'flag_md5sum': md5}
            nets[name].ac.encode(dict(common, x=lat(name, 'z'), mode='pmf', latent_name=name + '_z'))
            nets[name].ac.encode(dict(common, x=lat(name, 'q'), mode='laplace', sigma=lat(name, 'sigma'),
                                      latent_name=name + '_y'))
        with open(path, 'rb') as f:
            assert f.read() == np.asarray(g[('md5frame_%d' if md5 else 'frame_%d') % idx]).tobytes(), (case, idx)
        for name in names:
            z = nets[name].ac.decode({'mode': 'pmf', 'bitstream_path': path, 'data_dim': tuple(lat(name, 'z').shape),
                                      'device': cuda, 'latent_name': name + '_z', 'flag_md5sum': md5})
            assert torch.equal(z, lat(name, 'z'))
            q = nets[name].ac.decode({'mode': 'laplace', 'bitstream_path': path, 'sigma': lat(name, 'sigma'),
                                      'data_dim': tuple(lat(name, 'q').shape), 'device': cuda,
                                      'latent_name': name + '_y', 'flag_md5sum': md5})
            assert torch.equal(q, lat(name, 'q'))
    out = capsys.readouterr().out
    assert 'Ko!' not in out and '[Error]' not in out and 'Ok! Entropy coding is lossless' in out


@pytest.mark.parametrize('case', CASES)
def test_debug_plane_digest_is_the_reference_png_md5(case, golden):
    """flag_bitstream_debug (src/real_life/decode.py:304-326) compares md5 sums of the PNG FILES of the decoded
    planes: the product's in-memory PNG gives the digest the reference computed for the file it wrote."""
    pytest.importorskip('PIL')
    from aivc_amd.real_life.decode import plane_md5
    g = golden(case)
    m = _meta(g)
    for i in range(m['n']):
        for c in 'yuv':
            assert plane_md5(np.asarray(g['dec_%d_%s' % (m['first'] + i, c)])) == str(g['pngmd5_%d_%s' % (m['first'] + i, c)])


def test_fixture_variants_exercise_what_they_claim(golden):
    """all 16 CodecNet maps coded on the I frame of the GOP8 case (+ z larger than one position and a cropping h_s);
    EMPTY MOFNet y sections and no g_a_ref in the noref case; no gain_P / gain_B in the gain_i case"""
    g = golden('decoder_big_gop8')
    m = _meta(g)
    assert m['gop'] == '1_GOP_8' and m['data_dim']['x'] == (136, 200) and m['data_dim']['y'] == (9, 13) and m['data_dim']['z'] == (3, 4)
    sy = ocodec.split_lp(np.asarray(g['frame_0']).tobytes(), 0, 4)[3]
    assert sy[0] == 16 and list(sy[1:17]) == list(range(16))
    assert 4 * m['data_dim']['z'][0] > m['data_dim']['y'][0]  # h_s yields 12 x 16: the [:h_y, :w_y] crop does work
    g = golden('decoder_noref_empty_y')
    m = _meta(g)
    for i in (1, 2):
        sec = ocodec.split_lp(np.asarray(g['frame_%d' % i]).tobytes(), 0, 4)
        assert sec[1] == b'\x00' and len(sec[0]) > 0 and sec[3][0] > 0  # MOFNet: z coded, y section = "0 maps"
    model = _model(golden, 'decoder_noref_empty_y')
    assert model.mode_net.mode_net.g_a_ref is None and model.codec_net.codec_net.g_a_ref is None
    model = _model(golden, 'decoder_gain_i')
    assert not model.codec_net.codec_net.flag_gain_p_b and not hasattr(model.codec_net.codec_net, 'gain_P')
