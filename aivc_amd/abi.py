"""ctypes mirror of include/aivc_hip.h, include/aivc_hip_warp.h, include/aivc_hip_color.h, include/aivc_hip_quality.h,
include/aivc_hip_rates.h, include/aivc_hip_digest.h, include/aivc_hip_scene.h, include/aivc_hip_resize.h,
include/aivc_hip_rawvideo.h, include/aivc_hip_png.h, include/aivc_hip_png_read.h and include/aivc_hip_color_matrix.h (struct
layouts, constants, prototypes).

The same prototypes are bound twice: on libaivc_hip.so (device pointers, product path) by
aivc_amd/_lib.py, and -- with the ``_ref`` suffix, host pointers -- on the CPU oracle by
oracle/oracle.py (tests only).
"""
import ctypes as C

ABI_VERSION = 26
PREC_FP32, PREC_BF16X3, PREC_FP32_WINO = 0, 1, 2  # aivc_conv_params.precision

AIVC_OK = 0
ERR_UNSUPPORTED = -2
ERRORS = {0: 'AIVC_OK', -1: 'AIVC_ERR_ARG', -2: 'AIVC_ERR_UNSUPPORTED', -3: 'AIVC_ERR_LAUNCH',
          -4: 'AIVC_ERR_WORKSPACE'}

MODE_CONV, MODE_TCONV, MODE_GDN, MODE_IGDN = 0, 1, 2, 3
ACT_NONE, ACT_LEAKY, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3
ALGO_AUTO, ALGO_DIRECT, ALGO_MFMA = 0, 1, 2

AC_MAX_VAL = 256
LP = 514
CDF_ROW = 520
CDF_WIN0, CDF_WIN = 224, 64  # the decoder's fast-path window of a CDF row
BALLE_PARAMS = 43
MAX_MAPS = 256
RC_MAX_STREAMS = 64
RATE_LANES = 16384
SSE_BLOCKS = 64  # include/aivc_hip_quality.h: AIVC_SSE_BLOCKS
SAD_BLOCKS = 128  # include/aivc_hip_scene.h: AIVC_SAD_BLOCKS
RESIZE_TILE_W, RESIZE_MAX_SPAN = 256, 4064  # include/aivc_hip_resize.h: AIVC_RESIZE_TILE_W, AIVC_RESIZE_MAX_SPAN
WINO_MIN_PIXELS = 8000  # include/aivc_hip.h: AIVC_WINO_MIN_PIXELS
WINO_MIN_PIXELS_TCONV = 32768  # ... AIVC_WINO_MIN_PIXELS_TCONV

FRAME_I, FRAME_P, FRAME_B = 0, 1, 2

# include/aivc_hip_warp.h: aivc_warp_modes
WARP_BILINEAR, WARP_NEAREST, WARP_BICUBIC = 0, 1, 2
WARP_BORDER, WARP_ZEROS, WARP_REFLECTION = 0, 1, 2

_f = C.c_void_p  # every buffer pointer travels as an integer address


CONV_SPARSE4 = 1  # aivc_conv_params.flags: every 4th stored input channel is zero (images padded 3 -> 4)
CONV_WINO_ANY_SIZE = 2  # ... version 2 of the fp32 contract whatever the image size (tests)


class ConvParams(C.Structure):
    _fields_ = [('mode', C.c_int32), ('ksize', C.c_int32), ('stride', C.c_int32), ('pad', C.c_int32),
                ('n', C.c_int32), ('h_in', C.c_int32), ('w_in', C.c_int32), ('c_in', C.c_int32),
                ('h_out', C.c_int32), ('w_out', C.c_int32), ('c_out', C.c_int32),
                ('act1', C.c_int32), ('act2', C.c_int32), ('algo', C.c_int32), ('gdn', C.c_int32),
                ('flags', C.c_int32),
                ('x', _f), ('w', _f), ('bias', _f), ('mul', _f), ('res', _f), ('y', _f),
                ('gdn_beta', _f), ('gdn_gamma', _f),
                ('tail_w', _f), ('tail_bias', _f), ('tail_c_out', C.c_int32), ('precision', C.c_int32),
                ('w_bf16x3', C.c_void_p), ('w_wino', _f)]


MAX_IMAGES = 3


class ImageSrc(C.Structure):
    _fields_ = [('y', _f), ('u', _f), ('v', _f), ('f', _f), ('f_channels', C.c_int32), ('reserved', C.c_int32)]


class MapList(C.Structure):
    _fields_ = [('n_maps', C.c_int32), ('idx', C.c_uint8 * MAX_MAPS)]

    @classmethod
    def make(cls, idx):
        m = cls()
        m.n_maps = len(idx)
        for i, v in enumerate(idx):
            m.idx[i] = int(v)
        return m


def frame_maps_table(maps_list, npix):
    """numpy image of an aivc_frame_maps[len(maps_list)] array (include/aivc_hip.h): frame f codes the channels
    maps_list[f], its positions start where the previous frames' end.  -> (uint8 array [n, 272], [pos_off per frame], total)"""
    import numpy as np
    dt = np.dtype([('pos_off', '<u8'), ('n_maps', '<i4'), ('reserved', '<i4'), ('idx', 'u1', (MAX_MAPS,))])
    t = np.zeros(len(maps_list), dt)
    offs, pos = [], 0
    for f, m in enumerate(maps_list):
        offs.append(pos)
        t['pos_off'][f] = pos
        t['n_maps'][f] = len(m)
        if len(m):
            t['idx'][f, :len(m)] = np.asarray(list(m), np.uint8)
        pos += len(m) * npix
    return t.view(np.uint8).reshape(len(maps_list), dt.itemsize), offs, pos


class RcStream(C.Structure):
    _fields_ = [('in_off', C.c_uint64), ('out_off', C.c_uint64), ('row_off', C.c_uint64),
                ('n_sym', C.c_uint32), ('in_len', C.c_uint32), ('out_cap', C.c_uint32),
                ('plane', C.c_uint32)]


class RcBatch(C.Structure):
    _fields_ = [('n_streams', C.c_int32), ('reserved', C.c_int32), ('s', RcStream * RC_MAX_STREAMS)]


_i32, _sz, _fl = C.c_int32, C.c_size_t, C.c_float
_P = C.POINTER

# name -> argtypes (without the trailing stream argument, which every entry takes)
PROTOTYPES = {
    'aivc_ssim_means': [_f, _f, _i32, _i32, _i32, _f, _i32, C.c_double, C.c_double, _f, _f],
    'aivc_pool2x2': [_f, _i32, _i32, _i32, _i32, _f],
    'aivc_sq_err': [_f, _f, _sz, _f, _f],
    'aivc_conv2d': [_P(ConvParams)],
    'aivc_gdn_reparam': [_f, _f, _i32, _fl, _fl, _fl, _f, _f],
    'aivc_split_weights_bf16x3': [_f, _i32, _i32, C.c_void_p],
    'aivc_winograd_weights': [_f, _i32, _i32, _f],
    'aivc_winograd_weights_poly5': [_f, _i32, _i32, _f],
    'aivc_winograd_weights_tconv5': [_f, _i32, _i32, _f],
    'aivc_pad_channels': [_f, _sz, _i32, _f, _i32],
    'aivc_yuv420_to_444': [_f, _f, _f, _i32, _i32, _i32, _f, _i32, _i32, _i32],
    'aivc_yuv420u8_to_444': [_f, _f, _f, _i32, _i32, _i32, _f, _i32, _i32, _i32],
    'aivc_pack_images': [C.POINTER(ImageSrc), _i32, _i32, _i32, _i32, _f],
    'aivc_conv_images': [C.POINTER(ImageSrc), _i32, C.POINTER(ConvParams)],
    'aivc_frame_to_yuv420': [_f, _i32, _i32, _i32, _i32, _f, _i32, _i32, _i32, _f, _f, _f, _f, _f, _f],
    'aivc_downsample2x': [_f, _i32, _i32, _i32, _i32, _i32, _i32, _f],
    'aivc_warp_blend': [_f, _i32, _i32, _i32, _f, _f, _i32, _i32, _i32, _i32, _i32, _f, _f, _f, _i32, _f, _f],
    'aivc_warp_blend_rows': [_f, _i32, _i32, _i32, _f, _f, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f, _f, _f, _i32, _f, _f],
    'aivc_warp': [_f, _f, _i32, _i32, _i32, _i32, _f],
    'aivc_hyper_params': [_f, _i32, _i32, _i32, _i32, _i32, _i32, _f, _f],
    'aivc_channel_gain': [_f, _f, _sz, _i32, _f],
    'aivc_gain_interp': [_f, _f, _i32, _fl, _f],
    'aivc_quantize_center': [_f, _f, _f, _sz, _i32, _f, _f],
    'aivc_dequantize': [_f, _f, _f, _sz, _i32, _f],
    'aivc_balle_cdf_table': [_f, _i32, _f, _f],
    'aivc_nonzero_maps': [_f, _sz, _i32, _f],
    'aivc_nonzero_maps_batch': [_f, _i32, _sz, _i32, _f],
    'aivc_laplace_cdf_rows': [_f, _sz, _i32, _P(MapList), _f],
    'aivc_laplace_cdf_windows': [_f, _sz, _i32, _P(MapList), _f, _f],
    'aivc_laplace_bounds': [_f, _f, _sz, _i32, _P(MapList), _f],
    'aivc_table_bounds': [_f, _f, _sz, _i32, _f],
    'aivc_range_encode': [_f, _P(RcBatch), _f, _f],
    'aivc_range_decode': [_f, _f, _P(RcBatch), _f, _f],
    'aivc_range_decode_windows': [_f, _f, _f, _P(RcBatch), _f, _f],
    'aivc_scatter_symbols': [_f, _sz, _i32, _P(MapList), _f],
    'aivc_laplace_cdf_windows_batch': [_f, _i32, _sz, _i32, _f, _i32, _f, _f],
    'aivc_laplace_bounds_batch': [_f, _f, _i32, _sz, _i32, _f, _i32, _f],
    'aivc_table_bounds_batch': [_f, _f, _i32, _sz, _i32, _f],
    'aivc_scatter_symbols_batch': [_f, _i32, _sz, _i32, _f, _f],
    'aivc_bounds_rate': [_f, _sz, _f, _f],
    'aivc_rate_bits': [_f, _sz, _fl, _fl, _f, _f, _f],
    'aivc_laplace_prob': [_f, _f, _f, _sz, _f],
    'aivc_table_prob': [_f, _f, _sz, _sz, _i32, _f],
}

# aivc_detmath_eval is a diagnostic like aivc_selfcheck_gdn_math and is bound like it: by declare() on the device library only.
# PROTOTYPES is the list that declare() REQUIRES of an oracle library before it binds anything, and the oracle is test
# infrastructure that is not always of this package's revision: the suite and oracle of an earlier revision, run against this
# package to show that it still computes what it computed, have no twin of a newer diagnostic, and a name in PROTOTYPES would fail
# every one of their oracle calls instead of none.  So oracle.detmath_eval binds `aivc_detmath_eval_ref` itself, and
# tests/test_host_logic.py::test_oracle_exports_ref_twins asserts that twin by name.
DETMATH_EVAL_ARGS = [_i32, _f, _f, _sz, _f]

# aivc_detmath_eval's function ids (include/aivc_hip.h: AIVC_DETMATH_*)
DETMATH_EXP, DETMATH_EXPM1, DETMATH_LOG, DETMATH_LOG1P = 0, 1, 2, 3  # fp64 cores
DETMATH_EXPF, DETMATH_EXPM1F, DETMATH_SIGMOIDF, DETMATH_TANHF, DETMATH_SOFTPLUSF = 4, 5, 6, 7, 8  # fp32 wrappers
DETMATH_POWF, DETMATH_LAPLACE_CDF = 9, 10  # fp32, two operands
DETMATH_COUNT = 11


def detmath_is_fp64(fn):
    return DETMATH_EXP <= fn <= DETMATH_LOG1P


def detmath_operands(fn):
    return 2 if fn in (DETMATH_POWF, DETMATH_LAPLACE_CDF) else 1

# include/aivc_hip_color.h: device only, like aivc_warp_modes (the CPU oracle has no `_ref` twin of these; their CPU statement is
# Pillow itself, tests/test_color_tables.py)
COLOR_PROTOTYPES = {
    'aivc_rgb8_to_yuv420u8': [_f, _i32, _i32, _i32, _f, _f, _f],
    'aivc_yuv8_to_rgb8': [_f, _f, _f, _i32, _i32, _i32, _i32, _i32, _i32, _f],
}

# include/aivc_hip_quality.h: device only as well (their CPU statement is numpy, tests/test_gpu_quality_stats.py)
QUALITY_PROTOTYPES = {
    'aivc_frame_sse_u8': [_f, _f, _f, _f, _f, _f, _i32, _i32, _i32, _f, _f],
    'aivc_frame_aux_stats': [_f, _f, _f, _f, _i32, _i32, _i32, _i32, _i32, _i32, _f, _f],
}

# include/aivc_hip_rates.h: one gain row per image of a batch; device only (their statement is the single-gain entry points above,
# image by image, tests/test_gpu_latent_rows.py)
RATES_PROTOTYPES = {
    'aivc_channel_gain_rows': [_f, _f, _i32, _sz, _i32, _f],
    'aivc_quantize_center_rows': [_f, _f, _f, _i32, _sz, _i32, _f, _f],
    'aivc_dequantize_rows': [_f, _f, _f, _i32, _sz, _i32, _f],
}

# include/aivc_hip_digest.h: device only (its statement is RFC 1321, i.e. hashlib: tests/test_gpu_digest.py)
DIGEST_PROTOTYPES = {
    'aivc_md5_batch': [_f, C.c_int64, _i32, _f],
}

# include/aivc_hip_scene.h: device only (its statement is numpy: tests/test_gpu_pair_sad.py)
SCENE_PROTOTYPES = {
    'aivc_pair_sad_u8': [_f, _i32, C.c_int64, _f, _f],
}

# include/aivc_hip_resize.h: device only (its statement is Pillow: tests/resize_cases.py, tests/test_gpu_resize.py)
RESIZE_PROTOTYPES = {
    'aivc_resize_u8': [_f, _i32, _i32, _i32, _i32, _i32, _f, _f, _i32, _i32, _f, _f, _f, _f],
}

# include/aivc_hip_rawvideo.h: aivc_rawvideo_chroma
CHROMA_NONE, CHROMA_PLANAR, CHROMA_UV, CHROMA_VU = 0, 1, 2, 3


class RawVideoFmt(C.Structure):
    _fields_ = [('w', C.c_int32), ('h', C.c_int32), ('bytes_per_sample', C.c_int32), ('depth', C.c_int32),
                ('msb_aligned', C.c_int32), ('shift_x', C.c_int32), ('shift_y', C.c_int32), ('chroma', C.c_int32),
                ('offset', C.c_int64 * 3), ('pitch', C.c_int64 * 3)]


# include/aivc_hip_rawvideo.h: device only (their statement is numpy: tests/rawvideo_cases.py, tests/test_gpu_rawvideo.py)
RAWVIDEO_PROTOTYPES = {
    'aivc_rawvideo_to_yuv420u8': [_f, _i32, _P(RawVideoFmt), _f, _f, _f],
    'aivc_yuv420u8_to_rawvideo': [_f, _f, _f, _i32, _P(RawVideoFmt), _f],
}


# Everything declare() binds: (name, argtypes, restype, whether the stream argument is appended, whether the CPU oracle has a
# `_ref` twin).  The diagnostics, aivc_warp_modes (include/aivc_hip_diag.h, include/aivc_hip_warp.h) and the *_PROTOTYPES of the
# headers above are device only.
_BINDINGS = [(name, args, C.c_int, True, True) for name, args in PROTOTYPES.items()]
_BINDINGS += [
    ('aivc_conv2d_variant', [_P(ConvParams)], C.c_int, False, False),
    ('aivc_selfcheck_gdn_math', [C.c_uint64, C.c_uint32, _f], C.c_int, True, False),  # the device arithmetic against IEEE
    ('aivc_detmath_eval', DETMATH_EVAL_ARGS, C.c_int, True, False),  # the deterministic transcendentals, element by element
    ('aivc_diag_hold_lds', [C.c_uint32, C.c_uint32, _f], C.c_int, True, False),  # a workgroup that holds LDS for a bounded time
    ('aivc_warp_modes', [_f, _f, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f], C.c_int, True, False),
]
for _protos in (COLOR_PROTOTYPES, QUALITY_PROTOTYPES, RATES_PROTOTYPES, DIGEST_PROTOTYPES, SCENE_PROTOTYPES, RESIZE_PROTOTYPES):
    _BINDINGS += [(name, args, C.c_int, True, False) for name, args in _protos.items()]
_BINDINGS += [
    ('aivc_metrics_workspace', [_i32, _i32, _i32], C.c_size_t, False, True),
    ('aivc_abi_version', [], C.c_int, False, True),
]


def declare(lib, suffix=''):
    """Attach argtypes/restype for every entry of the header; raises AttributeError when the
    library does not export one of them."""
    fns = {}
    for name, args, restype, stream, twin in _BINDINGS:
        if twin or not suffix:
            fn = getattr(lib, name + suffix)
            fn.argtypes = list(args) + ([C.c_void_p] if stream else [])
            fn.restype = restype
            fns[name] = fn
    return fns


# RAWVIDEO_PROTOTYPES is bound by declare_rawvideo, not by the loop above: what declare() binds is pinned name by name
# (tests/test_host_logic.py: test_declare_binds_these_names_and_no_others), and that list stays as it is.  aivc_amd/_lib.py calls
# both on the device library, and a library that lacks either entry fails to load like one that lacks any other.
def declare_rawvideo(lib):
    """Attach argtypes/restype for the entries of include/aivc_hip_rawvideo.h (device library only); raises AttributeError when
    the library does not export one of them."""
    fns = {}
    for name, args in RAWVIDEO_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes = list(args) + [C.c_void_p]
        fn.restype = C.c_int
        fns[name] = fn
    return fns


# include/aivc_hip_png.h: device only (their statement is Pillow and zlib reading the result: tests/test_gpu_png.py)
PNG_RUN, PNG_SEG_WORDS = 32, 4  # AIVC_PNG_RUN, AIVC_PNG_SEG_WORDS
PNG_PROTOTYPES = {
    'aivc_png_deflate': [_f, _i32, _i32, _i32, _i32, _i32, _i32, _f, _f, _f],
    'aivc_png_gather': [_f, _f, _f, _i32, _i32, _i32, _i32, _i32, _f],
}


def declare_png(lib):
    """Attach argtypes/restype for the entries of include/aivc_hip_png.h (device library only), beside declare() for the reason
    declare_rawvideo states; raises AttributeError when the library does not export one of them."""
    fns = {}
    for name, args in PNG_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes = list(args) + [C.c_void_p]
        fn.restype = C.c_int
        fns[name] = fn
    return fns


# include/aivc_hip_png_read.h: device only (their statement is zlib.decompress and Pillow: tests/test_gpu_png_read.py)
INFLATE_OK = 0
INFLATE_STATUS = {0: 'ok', 1: 'the source ends inside the stream', 2: 'bad zlib header', 3: 'reserved block type',
                  4: 'stored block: NLEN is not ~LEN', 5: 'bad set of code lengths', 6: 'invalid symbol',
                  7: 'a match that starts before the output', 8: 'more output than expected', 9: 'less output than expected',
                  10: 'Adler-32 mismatch', 11: 'a stream of 2^31 bytes or more'}  # AIVC_INFLATE_*
PNG_UNFILTER_STATUS = {0: 'ok', 1: 'a filter type above 4', 2: 'a shape the kernel does not take'}  # AIVC_PNG_UNFILTER_*
PNG_READ_PROTOTYPES = {
    'aivc_inflate': [_f, _f, _i32, C.c_uint64, C.c_uint64, _f, _f],
    'aivc_png_unfilter': [_f, _f, _i32, C.c_uint64, _f, _f],
}


def declare_png_read(lib):
    """Attach argtypes/restype for the entries of include/aivc_hip_png_read.h (device library only), beside declare() for the
    reason declare_rawvideo states; raises AttributeError when the library does not export one of them."""
    fns = {}
    for name, args in PNG_READ_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes = list(args) + [C.c_void_p]
        fn.restype = C.c_int
        fns[name] = fn
    return fns


# include/aivc_hip_color_matrix.h: device only (their statement is numpy: aivc_amd/color.py, tests/test_gpu_colour_matrix.py)
COLOR_MATRIX_SHIFT, COLOR_MATRIX_MAX_COEF = 14, 65536  # AIVC_COLOR_MATRIX_SHIFT, AIVC_COLOR_MATRIX_MAX_COEF


class ColorMatrix(C.Structure):
    _fields_ = [('fwd', (C.c_int32 * 3) * 3), ('fwd_off', C.c_int32 * 3), ('inv', C.c_int32 * 5), ('inv_yoff', C.c_int32)]


COLOR_MATRIX_PROTOTYPES = {
    'aivc_rgb8_to_yuv420u8_matrix': [_f, _i32, _i32, _i32, _P(ColorMatrix), _i32, _f, _f, _f],
    'aivc_yuv8_to_rgb8_matrix': [_f, _f, _f, _i32, _i32, _i32, _i32, _i32, _i32, _P(ColorMatrix), _f],
}


def declare_color_matrix(lib):
    """Attach argtypes/restype for the entries of include/aivc_hip_color_matrix.h (device library only), beside declare() for the
    reason declare_rawvideo states; raises AttributeError when the library does not export one of them."""
    fns = {}
    for name, args in COLOR_MATRIX_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes = list(args) + [C.c_void_p]
        fn.restype = C.c_int
        fns[name] = fn
    return fns


def conv_out_size(mode, h, w, k, stride, pad):
    if mode == MODE_CONV:
        return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    if mode == MODE_TCONV:
        return 2 * h, 2 * w
    return h, w
