"""HIP kernels vs the CPU oracle, through the C ABI, on seeded inputs: bit exact."""
import numpy as np
import pytest
import torch

from aivc_amd import abi
from conv_cases import (ATTENTION_GATE_CASES, CONV_CASES, CONV_IMAGES_CASES, FUSED_GDN_CASES, FUSED_TAIL_CASES, STAGED_CASES, STAGED_FUSED_GDN_CASES, THIN_WALK_CASES,
                        THIN_WALK_GRIDS, attention_gate_case, conv_case, conv_images_cases, fused_gdn_case, fused_tail_case, pack_images_cases, thin_walk_case)
from op_cases import (FORCED, FRAME_BATCH_CASES, FRAME_SIZES, RANGE_CODER_CASES, WARP_SHAPES, T, cdf_case, eq, frame_batch_case, forced_case, frame_sources,
                      frame_to_yuv420_case, latent_ops_case, on, profiled, range_coder_case, range_coder_pmf_case, range_encode_case,
                      straddle_stream, warp_blend_case, warp_blend_sources, warp_case, yuv420_to_444_case, yuv_planes)

pytestmark = pytest.mark.gpu

ALGOS = [abi.ALGO_DIRECT, abi.ALGO_AUTO, abi.ALGO_MFMA]


@pytest.mark.parametrize('case', CONV_CASES)
@pytest.mark.parametrize('algo', ALGOS)
def test_conv_family_bit_exact(case, algo, oracle, cuda):
    from aivc_amd import ops
    c = conv_case(oracle, case, hash(case) % (2 ** 31))
    c.check(c.run(ops, on(cuda), algo=algo))


@pytest.mark.parametrize('row,tiles', STAGED_CASES + STAGED_FUSED_GDN_CASES)
def test_register_staged_k_loop_on_every_tile(row, tiles, oracle, cuda, monkeypatch):
    """The register-staged K loop is what the (I)GDN mode and transposed conv with c_in % 32 != 0 run on (conv and transposed
    conv with whole K tiles have the LDS-DMA loop only): each of them through ALGO_MFMA on every tile it is instantiated for,
    the launch's variant code asserted, bit exact against the oracle (computed once per row)."""
    from aivc_amd import ops
    fused = len(row) == 10
    c = (fused_gdn_case if fused else conv_case)(oracle, row, abs(hash(row)) % (2 ** 31))
    digit = {abi.MODE_CONV: 0, abi.MODE_TCONV: 1, abi.MODE_GDN: 2, abi.MODE_IGDN: 2}[row[0]]
    for tile in tiles:
        monkeypatch.setenv('AIVC_FORCE_TILE', str(tile))
        got, codes = profiled(lambda: c.run(ops, on(cuda), algo=abi.ALGO_MFMA))
        assert codes == [100 + 10 * digit + tile + (50 if fused else 0)], (tile, codes)
        c.check(got)


@pytest.mark.parametrize('grid', THIN_WALK_GRIDS)
@pytest.mark.parametrize('co,k,ci,h,w', THIN_WALK_CASES)
def test_thin_layer_tile_walk(grid, co, k, ci, h, w, oracle, cuda, monkeypatch):
    """The thin output layer's persistent groups walk several tiles each (origins advanced without divisions across tile
    rows and images, double-buffered patches, epilogue of the previous tile inside the next chain): forced here at
    small sizes with AIVC_THIN_GRID_MAX groups over 3 images, bit exact against the oracle -- with and without bias."""
    from aivc_amd import ops
    monkeypatch.setenv('AIVC_THIN_GRID_MAX', str(grid))
    for with_bias in (True, False):
        c = thin_walk_case(oracle, (co, k, ci, h, w), grid * 100 + co, with_bias)
        c.check(c.run(ops, on(cuda)))


def test_frame_ops_bit_exact(oracle, cuda):
    from aivc_amd import ops
    rng = np.random.default_rng(5)
    for (h, w) in FRAME_SIZES:
        planes = yuv_planes(rng, h, w)
        for u8 in (True, False):
            c = yuv420_to_444_case(oracle, planes, u8)
            c.check(c.run(ops, on(cuda)))
        x, skip, x3 = frame_sources(rng, h, w)
        # x3: the synthesis output as the codec hands it over: 3 channels, padded to an even row length (the 8-byte /
        # 16-byte load path of the kernel when the frame sides are even, the scalar one otherwise)
        for src, want_float in ((x, True), (x3, True), (x3, False)):
            for sk in (None, skip):
                c = frame_to_yuv420_case(oracle, src, h, w, sk, want_float)
                c.check(c.run(ops, on(cuda)))


def test_warp_bit_exact(oracle, cuda):
    from aivc_amd import ops
    rng = np.random.default_rng(6)
    for (h, w, s) in WARP_SHAPES + [(32, 48, 1.0)]:
        c = warp_case(oracle, rng, h, w, s)
        c.check(c.run(ops, on(cuda)))
        sources = warp_blend_sources(rng, h, w, s)
        for ft in (1, 2):
            fast, general = (warp_blend_case(oracle, sources, h, w, ft, g) for g in (False, True))
            for c in (fast, general):
                c.check(c.run(ops, on(cuda)))
            # the general kernel (3 stored reference channels, 3 output channels, 7 mask / flow channels) against
            # the 16-byte fast path (4 / 4 / 8)
            for kk in ('pred', 'skip', 'x_warp'):
                np.testing.assert_array_equal(general.want[kk], fast.want[kk][..., :3])


def test_latent_ops_bit_exact(oracle, cuda):
    from aivc_amd import ops
    c = latent_ops_case(oracle, 7)
    c.check(c.run(ops, on(cuda)))


def test_cdf_kernels_bit_exact(oracle, cuda):
    from aivc_amd import ops
    c = cdf_case(oracle, 8, (1, 6, 7, 8))
    d = c.place(on(cuda))
    c.check(c.call(ops, d))
    flags = ops.nonzero_flags(d['q']).cpu().numpy()[0]
    assert [i for i in range(8) if flags[i]] == oracle.nonzero_maps(c.inputs['q'])


@pytest.mark.parametrize('n_sym,scale', RANGE_CODER_CASES)
def test_range_coder_bit_exact(n_sym, scale, oracle, cuda):
    """(70000 symbols: the encoder launch that asks for a CU of its own, csrc/entropy.hip aivc_range_encode)"""
    from aivc_amd import ops
    c = range_coder_case(oracle, n_sym, scale)
    c.check(c.run(ops, on(cuda)))


def test_range_encoder_batches_ragged_streams_and_long_straddle_runs(oracle, cuda):
    """A batch of streams in ONE launch (the stream-per-lane encoder codes them side by side in one wavefront): ragged
    lengths incl. empty, 1, 7, 8, 9 symbols (chunk edges), more than 64 streams (two launches), ordinary Laplace symbols
    and adversarial straddle runs (pending count up to hundreds: the output of one symbol is longer than a word) -- every
    stream's bytes == the oracle's."""
    from aivc_amd import ops
    c = range_encode_case(oracle, 77, [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 500, 2049], 60, 3000, straddle=True)
    c.check(c.run(ops, on(cuda)))


def test_range_encoder_output_capacity_contract(oracle, cuda):
    """include/aivc_hip.h aivc_rc_stream.out_cap: whole 32-bit words, at least one -- anything else is AIVC_ERR_ARG at the
    entry point (the stream-per-lane packer clamps its stores to word out_cap / 4 - 1); a capacity the stream does not
    fit reports out_len 0xFFFFFFFF and writes nothing beyond it"""
    import ctypes as C
    from aivc_amd import abi, ops
    from aivc_amd._lib import AivcNativeError, call
    rng = np.random.default_rng(5)
    bounds = straddle_stream(rng, 400, burst=3)
    want = oracle.range_encode(bounds)
    assert len(want) > 64
    b = T(np.ascontiguousarray(bounds).view(np.int32), cuda)
    guard = 0xA5
    for cap, ok in ((0, False), (3, False), (6, False), (8, True), (64, True), ((len(want) + 3) // 4 * 4, True)):
        out = torch.full((4096,), guard, dtype=torch.uint8, device=cuda)
        ln = torch.zeros(1, dtype=torch.int32, device=cuda)
        batch = abi.RcBatch()
        batch.n_streams = 1
        batch.s[0].in_off, batch.s[0].out_off, batch.s[0].n_sym, batch.s[0].out_cap = 0, 0, b.numel(), cap
        args = ('aivc_range_encode', C.c_void_p(b.data_ptr()), C.byref(batch), C.c_void_p(out.data_ptr()),
                C.c_void_p(ln.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if not ok:
            with pytest.raises(AivcNativeError):
                call(*args)
            continue
        call(*args)
        torch.cuda.synchronize()
        n = int(ln.cpu().numpy().view(np.uint32)[0])
        out_h = out.cpu().numpy()
        assert (out_h[cap:] == guard).all(), (kernel, cap)  # nothing beyond the capacity
        if cap >= len(want):
            assert n == len(want) and out_h[:n].tobytes() == want
        else:
            assert n == 0xFFFFFFFF, (kernel, cap, n)


@pytest.mark.parametrize('scale', [0.4, 3.0, 40.0, 150.0])
def test_range_decode_from_windows(scale, oracle, cuda):
    """64-entry CDF windows + sigma per position (what the codec's decoder reads) give the symbols of the full rows,
    in and outside the window; the windows equal the oracle's and the slice of the full rows"""
    from aivc_amd import ops
    rng = np.random.default_rng(int(scale * 10))
    h, w, c = 9, 13, 6
    maps = [0, 2, 5]
    sig = (np.abs(rng.standard_normal((1, h, w, c))) * scale + 0.05).astype(np.float32)
    q = np.clip(np.rint(rng.standard_normal((1, h, w, c)) * sig), -256, 255).astype(np.int16)
    bounds = oracle.laplace_bounds(sig, q, maps)
    payload = oracle.range_encode(bounds)
    rows = oracle.laplace_cdf_rows(sig, maps)
    n_sym = len(maps) * h * w
    want = oracle.range_decode(payload, rows, n_sym)
    win_o, sp_o = oracle.laplace_cdf_windows(sig, maps)
    np.testing.assert_array_equal(win_o, rows[:, abi.CDF_WIN0:abi.CDF_WIN0 + abi.CDF_WIN])
    np.testing.assert_array_equal(oracle.range_decode_windows(payload, win_o, sp_o, n_sym), want)
    win, sp = ops.laplace_cdf_windows(T(sig, cuda), maps)
    eq(win, win_o)
    eq(sp, sp_o)
    got, bits = ops.range_decode([payload], win, [0], [n_sym], [0], sigma_pos=sp, want_bits=True)
    eq(got[0], want)
    assert len(payload) == (int(bits.cpu()[0]) + 2 + 7) // 8
    if scale >= 40.0:
        assert (np.abs(q[..., maps]) > 32).any(), 'the slow path (symbol outside the window) must be exercised'


@pytest.mark.timeout(120)
@pytest.mark.parametrize('sigma', [0.7, 30.0, 148.0, 600.0])
def test_range_decode_from_windows_of_a_foreign_stream(sigma, oracle, cuda):
    """Bytes no encoder of these CDFs wrote (a corrupt or foreign stream): the decoder's rare path must end its search
    whatever the stream asks for -- at large sigma entry 0 of a row is not 0 and the stream can ask for less -- and
    return what the kernel that searches full rows returns (and the oracle, where every count has a symbol: once a
    stream asks for less than entry 0 the interval is invalid and torchac's own arithmetic is undefined)."""
    from aivc_amd import ops
    rng = np.random.default_rng(int(sigma * 10))
    n_sym = 3000
    sig = np.full((1, 1, n_sym, 1), sigma, np.float32)
    payload = bytes(rng.integers(0, 256, 6000, dtype=np.uint8)) if sigma != 30.0 else bytes(6000)
    rows = oracle.laplace_cdf_rows(sig, [0])
    want = oracle.range_decode(payload, rows, n_sym)
    win, sp = ops.laplace_cdf_windows(T(sig, cuda), [0])
    got_w = ops.range_decode([payload], win, [0], [n_sym], [0], sigma_pos=sp)[0]
    got_r = ops.range_decode([payload], ops.laplace_cdf_rows(T(sig, cuda), [0]), [0], [n_sym], [0])[0]
    assert torch.equal(got_w, got_r)
    if int(rows[0, 0]) == 0:
        eq(got_w, want)


@pytest.mark.parametrize('sigma', [1e-4, 0.3, 5.0, 148.0])
def test_range_coder_forced_symbols(sigma, oracle, cuda):
    """Deterministic visit of the decoder's corners: symbols 0, 1 (octet 0), 223 / 224 and 287 / 288 (either side of
    the 64-entry window), 286, 510, 511 (octet 63: reads CDF entry 512 through lane 8) and 512 (value +256, torchac's
    max_symbol, upper bound 2^16 packed as c_hi = 0) -- HIP bounds / bytes / symbols == oracle, from full rows and
    from windows, at a sigma where everything sits in the window's tail and one where nothing does."""
    from aivc_amd import ops
    sig, q = forced_case(sigma, repeat=11)
    n = q.size
    want = (q.reshape(-1).astype(np.int32) + 256).astype(np.uint16)
    b_ref = oracle.laplace_bounds(sig, q, [0])
    b = ops.laplace_bounds(T(sig, cuda), T(q, cuda), [0])
    eq(b, b_ref.view(np.int32))
    ref_bytes = oracle.range_encode(b_ref)
    out, lens, _ = ops.range_encode([b])
    assert out.cpu().numpy()[:int(lens.cpu()[0])].tobytes() == ref_bytes
    rows = ops.laplace_cdf_rows(T(sig, cuda), [0])
    eq(rows, oracle.laplace_cdf_rows(sig, [0]).view(np.int16))
    eq(ops.range_decode([ref_bytes], rows, [0], [n], [0])[0], want)
    win, sp = ops.laplace_cdf_windows(T(sig, cuda), [0])
    eq(ops.range_decode([ref_bytes], win, [0], [n], [0], sigma_pos=sp)[0], want)


def test_range_coder_symbol_512_table_mode(oracle, cuda):
    from aivc_amd import ops
    rng = np.random.default_rng(5)
    params = (rng.standard_normal((2, abi.BALLE_PARAMS)) * 0.8).astype(np.float32)
    table, _ = oracle.balle_cdf_table(params)
    qz = np.array(FORCED * 2, np.int16).reshape(1, 2, 5, 2)
    b_ref = oracle.table_bounds(table, qz)
    b = ops.table_bounds(T(table.view(np.int16), cuda), T(qz, cuda))
    eq(b, b_ref.view(np.int32))
    ref_bytes = oracle.range_encode(b_ref)
    out, lens, _ = ops.range_encode([b])
    assert out.cpu().numpy()[:int(lens.cpu()[0])].tobytes() == ref_bytes
    sym = ops.range_decode([ref_bytes], T(table.view(np.int16), cuda), [0], [qz.size], [10])[0]
    eq(ops.scatter_symbols(sym, 10, 2, [0, 1]), qz.reshape(10, 2))


def test_range_coder_pmf_and_scatter(oracle, cuda):
    from aivc_amd import ops
    c = range_coder_pmf_case(oracle, 11)
    c.check(c.run(ops, on(cuda)))
    # partial map list
    maps = [1, 4]
    s2 = T((c.qz.reshape(42, 5)[:, maps].T.reshape(-1).astype(np.int32) + 256).astype(np.uint16).view(np.int16), cuda)
    eq(ops.scatter_symbols(s2, 42, 5, maps), oracle.scatter_symbols(s2.cpu().numpy().view(np.uint16), 42, 5, maps))


def test_range_coder_many_streams_concurrently(oracle, cuda):
    """70 independent streams (> 64 per launch) with different lengths: batched == one by one."""
    from aivc_amd import ops
    rng = np.random.default_rng(21)
    c, bl, pl, rows_all, offs, ns, want = 1, [], [], [], [], [], []
    total = 0
    for i in range(70):
        n = int(rng.integers(1, 700))
        sig = np.exp(rng.uniform(-3, 3, (1, 1, n, 1))).clip(1e-4, 148).astype(np.float32)
        q = np.clip(np.rint(rng.laplace(0, 1, sig.shape) * sig), -256, 255).astype(np.int16)
        b = oracle.laplace_bounds(sig, q, [0])
        bl.append(T(b.view(np.int32), cuda))
        pl.append(oracle.range_encode(b))
        rows_all.append(oracle.laplace_cdf_rows(sig, [0]))
        offs.append(total)
        total += n
        ns.append(n)
        want.append((q.reshape(-1).astype(np.int32) + 256).astype(np.uint16))
    out, lens, o = ops.range_encode(bl)
    out_h, lens_h = out.cpu().numpy(), lens.cpu().numpy()
    for i in range(70):
        assert out_h[o[i][0]:o[i][0] + lens_h[i]].tobytes() == pl[i]
    rows = T(np.concatenate(rows_all).view(np.int16), cuda)
    dec = ops.range_decode(pl, rows, offs, ns, [0] * 70)
    for i in range(70):
        eq(dec[i], want[i])


@pytest.mark.parametrize('case', FUSED_GDN_CASES)
def test_fused_gdn_bit_exact(case, oracle, cuda):
    """conv + (I)GDN fused in one launch == oracle fused == oracle conv followed by oracle GDN"""
    from aivc_amd import ops
    mode, k, s, pad, _, _, _, _, inv, _ = case
    c = fused_gdn_case(oracle, case, abs(hash(case)) % (2 ** 31))
    i = c.inputs
    two = oracle.gdn(oracle.conv2d(i['x'], i['w'], i['bias'], mode=mode, stride=s, pad=pad), i['beta'], i['gamma'], inverse=inv, res=i['res'])
    np.testing.assert_array_equal(c.want, two)
    c.check(c.run(ops, on(cuda)))


def test_gdn_lean_math_selfcheck(cuda):
    """the lean square root / division of the fused GDN epilogues (csrc/common.h) == the compiler's IEEE sequences:
    every float of the safe range for the square root, 2^39 random operand pairs (two seeds) for the division"""
    from aivc_amd import ops
    for seed in (20260929, 7):
        bad_sqrt, bad_div = ops.selfcheck_gdn_math(1 << 38, seed=seed)
        assert (bad_sqrt, bad_div) == (0, 0), seed


@pytest.mark.parametrize('scale,zero_bias', [(1.0, False), (2.0 ** 70, False), (2.0 ** -70, True), (0.0, True), (2.0 ** 40, False)])
@pytest.mark.parametrize('inv', [False, True])
def test_fused_gdn_operand_range_fallback(scale, zero_bias, inv, oracle, cuda):
    """operands far outside [2^-60, 2^60] (huge, tiny, exactly zero outputs) next to ordinary ones: the image layer
    (5x5 s2 -> 64, aivc_conv_images) takes the full IEEE sequences for the wavefronts that see them and the lean ones
    (csrc/common.h) for the others; the 3x3 128 -> 128 layer always the full ones: either way == oracle, bit for bit"""
    from aivc_amd import ops
    rng = np.random.default_rng(77)
    x = (rng.standard_normal((2, 16, 32, 128), dtype=np.float32) * np.float32(scale)).astype(np.float32)
    x[0, :8] *= np.float32(1.0 if scale >= 1 else 2.0 ** 60)  # mixed: some tiles in range, some not
    wt = (rng.standard_normal((128, 3, 3, 128), dtype=np.float32) / 34.0).astype(np.float32)
    bias = np.zeros(128, np.float32) if zero_bias else rng.standard_normal(128, dtype=np.float32)
    beta = (np.abs(rng.standard_normal(128)) + 0.2).astype(np.float32)
    gamma = (np.abs(rng.standard_normal((128, 128))) * 0.05).astype(np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        want = oracle.conv2d(x, wt, bias, stride=1, pad=1, gdn=(beta, gamma, inv))
    got = ops.conv2d(T(x, cuda), T(wt, cuda), T(bias, cuda), stride=1, pad=1, gdn=(T(beta, cuda), T(gamma, cuda), inv))
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # the first analysis layer from float sources (aivc_conv_images)
    img = (rng.random((2, 16, 128, 4), dtype=np.float32) * np.float32(scale)).astype(np.float32)
    img[..., 3] = 0
    wi = np.zeros((64, 5, 5, 4), np.float32)
    wi[..., :3] = rng.standard_normal((64, 5, 5, 3), dtype=np.float32) * 0.1
    bi = np.zeros(64, np.float32) if zero_bias else rng.standard_normal(64, dtype=np.float32)
    b64, g64 = beta[:64].copy(), gamma[:64, :64].copy()
    with np.errstate(over='ignore', invalid='ignore'):
        want_i = oracle.conv2d(img, wi, bi, stride=2, pad=2, gdn=(b64, g64, inv))
    stack = ops.ImageStack([T(img, cuda)], 16, 128, cuda)
    got_i = ops.conv2d(stack, T(wi, cuda), T(bi, cuda), stride=2, pad=2, gdn=(T(b64, cuda), T(g64, cuda), inv))
    np.testing.assert_array_equal(got_i.cpu().numpy().view(np.uint32), want_i.view(np.uint32))


@pytest.mark.parametrize('case', FUSED_TAIL_CASES)
def test_fused_tail_bit_exact(case, oracle, cuda):
    """conv + activation + 1x1 conv (+ residual, activation) in one launch == the oracle's two convolutions; a tail leaves the
    contract version of its conv unchanged (the Winograd chain where version 2 covers the conv, else none)"""
    from aivc_amd import ops
    c = fused_tail_case(oracle, case, abs(hash(case)) % (2 ** 31))
    i = c.inputs
    if i['w3'].shape[-1] == case[3]:  # the oracle's own fused twin
        np.testing.assert_array_equal(oracle.conv2d(i['x'], i['w'], i['bias'], res=i['res'], tail=(i['w3'], i['b3']), **c.fixed), c.want)
    assert not ops.WINO_ANY_SIZE and not oracle.WINO_ANY_SIZE
    got, codes = profiled(lambda: c.run(ops, on(cuda)))
    c.check(got)
    if ops.PRECISION == abi.PREC_FP32_WINO and c.covered:
        assert len(codes) == 2 and codes[0] == 301 and codes[1] not in ops._WINO_VARIANTS, codes
    else:
        assert not set(codes) & set(ops._WINO_VARIANTS), codes


def test_attention_res_block_256_bit_exact_in_version_2(oracle, cuda):
    """AttentionResBlock(256) (what bench.py --widths n=256 builds: a 128-wide bottleneck) at a 1/4-resolution size past
    AIVC_WINO_MIN_PIXELS, default contract, size rule in force: its 3x3 128 -> 128 with the fused-tail request runs 301 in two
    launches, and forward_nhwc == the oracle's run_layer on the exported spec, bit for bit"""
    from aivc_amd import ops
    from aivc_amd.layers.misc.attention import AttentionResBlock
    from oracle import spec as ospec
    assert ops.PRECISION == abi.PREC_FP32_WINO and not ops.WINO_ANY_SIZE and not oracle.WINO_ANY_SIZE
    torch.manual_seed(256)
    m = AttentionResBlock(256).eval()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape) / (p[0].numel() ** 0.5 if p.dim() > 1 else 10.0))
    rng = np.random.default_rng(256)
    x = rng.standard_normal((1, 90, 100, 256), dtype=np.float32)  # 9000 pixels
    want = oracle.run_layer(ospec.export_spec(m), x)
    m = m.to(cuda)
    ops.PROFILE = []
    try:
        with torch.no_grad():
            got = m.forward_nhwc(T(x, cuda))
        torch.cuda.synchronize()
        codes = [rec[0] for rec in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert codes.count(301) == 1 and len(codes) == 3, codes  # 1x1, the 3x3 on the chain, the 1x1 tail
    eq(got, want)


@pytest.mark.parametrize('n,h,w,c,scale', [pytest.param(*r, id='-'.join(str(v) for v in r[:4]) + ('' if r[4] == 1.0 else '-x%g' % r[4]))
                                           for r in ATTENTION_GATE_CASES])
def test_attention_gate_epilogue_bit_exact(n, h, w, c, scale, oracle, cuda):
    """x + trunk * sigmoid(conv1x1(a)) in the conv epilogue (whole 64x64 tiles take the inlined-sigmoid path, ragged ones
    the general one): both equal the oracle, through every algo; the scaled row's pre-activations reach beyond +-88, where
    exp(-v) overflows fp32 or is subnormal"""
    from aivc_amd import ops
    case = attention_gate_case(oracle, n, h, w, c, scale)
    if scale != 1.0:
        assert case.pre_activation.min() < -88 and case.pre_activation.max() > 88
    for algo in ALGOS:
        case.check(case.run(ops, on(cuda), algo=algo))


def test_fused_tail_is_one_launch(cuda):
    """the bottleneck-block shape takes the fused kernel (variant 190), others are declined by the library"""
    import ctypes as C
    from aivc_amd._lib import load
    x = torch.zeros((1, 16, 16, 64), device=cuda)
    w = torch.zeros((64, 3, 3, 64), device=cuda)
    b = torch.zeros(64, device=cuda)
    y = torch.zeros((1, 16, 16, 128), device=cuda)
    w3 = torch.zeros((128, 1, 1, 64), device=cuda)
    b3 = torch.zeros(128, device=cuda)
    ptr = lambda t: t.data_ptr()
    p = abi.ConvParams(abi.MODE_CONV, 3, 1, 1, 1, 16, 16, 64, 16, 16, 64, abi.ACT_LEAKY, abi.ACT_LEAKY, abi.ALGO_AUTO, 0, 0,
                       ptr(x), ptr(w), ptr(b), None, None, ptr(y), None, None, ptr(w3), ptr(b3), 128, 0)
    assert load()['aivc_conv2d_variant'](C.byref(p)) == 190
    p.tail_c_out = 64
    assert load()['aivc_conv2d_variant'](C.byref(p)) < 0
    p.tail_c_out = 128
    p.algo = abi.ALGO_DIRECT
    assert load()['aivc_conv2d_variant'](C.byref(p)) < 0


@pytest.mark.parametrize('h,w,n', CONV_IMAGES_CASES)
@pytest.mark.parametrize('use_gdn', [True, False])
def test_conv_images_bit_exact(h, w, n, use_gdn, cuda, oracle, monkeypatch):
    """aivc_conv_images (first analysis layer straight from the image sources) == oracle conv over the packed tensor
    == the HIP pack + conv pair, for 1 / 2 / 3 images, 8-bit 4:2:0 and float sources, ragged tiles"""
    from aivc_amd import ops
    from aivc_amd._lib import load
    monkeypatch.setattr(ops, '_CONV_IMAGES_MAX', 3)  # the codec sends 3-image stacks down the pack + conv path (faster)
    for c in conv_images_cases(oracle, h, w, n, use_gdn, ('a', 'f', 'ab', 'af', 'aba', ('f', 'a', None))):
        i = c.inputs
        g = (i['beta'], i['gamma'], False) if use_gdn else None
        np.testing.assert_array_equal(oracle.conv_images(i['parts'], h, w, i['w'], i['bias'], act1=c.act1, gdn=g), c.want)
        before = load()['aivc_abi_version']()
        c.check(c.run(ops, on(cuda)))
        c.check(c.run(ops, on(cuda), packed=True))  # the two-call path it replaces
        assert before == abi.ABI_VERSION


def test_conv_images_declines_other_layers(cuda):
    """layers outside the kernel's coverage fall back to pack + conv (same result path as before)"""
    from aivc_amd import ops
    rng = np.random.default_rng(5)
    f = torch.from_numpy(rng.standard_normal((1, 12, 12, 4)).astype(np.float32)).to(cuda)
    stack = ops.ImageStack([f], 12, 12, cuda)
    w = torch.from_numpy(rng.standard_normal((32, 3, 3, 4)).astype(np.float32)).to(cuda)
    y = ops.conv2d(stack, w, None, stride=1, pad=1)
    assert stack._packed is not None and tuple(y.shape) == (1, 12, 12, 32)


@pytest.mark.parametrize('h,w', [(9, 13), (16, 32), (35, 1030)])
def test_pack_images_bit_exact(h, w, cuda, oracle):
    """aivc_pack_images (padded multi-image input of the first convs) == oracle twin == per-image conversion"""
    from aivc_amd import ops
    for c in pack_images_cases(oracle, h, w, 2, ('a', ('a', None), ('a', 'b', None), 'af', 'aba', (None, 'f', 'b'))):
        parts_np, parts_t = c.inputs['parts'], c.place(on(cuda))['parts']
        got = c.check(c.call(ops, {'parts': parts_t}))
        assert got._aivc_cmap == tuple(4 * i + ch for i in range(len(parts_np)) for ch in range(3))
        # and the same as the per-image kernels
        for i, p in enumerate(parts_np):
            if isinstance(p, dict):
                ref = ops.yuv420_to_444(parts_t[i]['y'], parts_t[i]['u'], parts_t[i]['v'], c_store=4)
                assert torch.equal(got[..., 4 * i:4 * i + 4], ref)
            elif p is None:
                assert not got[..., 4 * i:4 * i + 4].any()
            else:
                assert torch.equal(got[..., 4 * i:4 * i + 3], parts_t[i][..., :3]) and not got[..., 4 * i + 3].any()


def test_frame_batch_entropy_kernels_equal_per_frame_calls(oracle, cuda):
    """aivc_laplace_cdf_windows_batch / laplace_bounds_batch / table_bounds_batch / scatter_symbols_batch (one launch per
    frame batch, per-frame map lists in a device table) == the oracle's own implementation of every step, frame by frame
    (the independent check: the single-frame entry points are the one-frame case of the same kernels), and == the
    single-frame entry points (the map list passed by value against the one read from the table), incl. frames with no
    coded map.  Second shape: c % 8 != 0 (the scatter's scalar tail), a frame with every map coded next to frames with
    fewer (grid sized for the longest list) and one with none.  Exact equality throughout."""
    from aivc_amd import ops
    rng = np.random.default_rng(21)
    for (n, h, w, c), maps in FRAME_BATCH_CASES:
        npix = h * w
        case = frame_batch_case(oracle, rng, (n, h, w, c), maps)
        d = case.place(on(cuda))
        win = torch.zeros((case.total, abi.CDF_WIN), dtype=torch.int16, device=cuda)
        sp = torch.zeros(case.total, dtype=torch.float32, device=cuda)
        r = case.check(case.call(ops, d, out=(win, sp)))
        # == the single-frame entry points
        sd, qd = d['sig'], d['q']
        for f, m in enumerate(maps):
            sl = slice(r['offs'][f], r['offs'][f] + len(m) * npix)
            if m:
                eq(r['b'][sl], ops.laplace_bounds(sd[f:f + 1], qd[f:f + 1], m))
                w1, s1 = ops.laplace_cdf_windows(sd[f:f + 1], m)
                eq(win[sl], w1)
                eq(sp[sl], s1)
            eq(r['tb'][f], ops.table_bounds(d['table'], qd[f:f + 1]))
            eq(ops.scatter_symbols(d['syms'][f], npix, c, m).view(h, w, c), case.want['q'][f])
