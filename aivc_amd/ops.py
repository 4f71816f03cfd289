"""Tensor-level wrappers over the C ABI (include/aivc_hip.h).

PyTorch is used for device memory and streams only: every function takes CUDA tensors, hands raw
device pointers to libaivc_hip.so on torch's current stream and returns freshly allocated CUDA
tensors.  Feature maps are NHWC fp32 ([n, h, w, c], contiguous).  CPU tensors are rejected: the
product has no CPU execution path (the CPU restatement lives in oracle/ and is test-only).
"""
import ctypes as C
import os

import numpy as np
import torch

from . import abi
from ._lib import AivcNativeError, call, load

FRAME_I, FRAME_P, FRAME_B = abi.FRAME_I, abi.FRAME_P, abi.FRAME_B

# when bench.py sets this to a list, every aivc_conv2d launch is bracketed by HIP events
PROFILE = None
PROFILE_DIRECT_EQUIVALENT = [0.0, 0.0]  # Winograd launches while PROFILE is on: [tap-chain FLOPs they replace, FLOPs they execute]
# likewise for the HBM-bound stages: (name, algorithmic bytes, event, event) per launch
PROFILE_HBM = None


def _hbm_profiled(name, nbytes, launch):
    if PROFILE_HBM is None:
        return launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    PROFILE_HBM.append((name, float(nbytes), e0, e1))


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream():
    # hipStream_t of torch's current stream on the current device (the raw getter avoids ~7 us of
    # Python per launch)
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype=None, name='tensor'):
    if t is None:
        return None
    if isinstance(t, ImageStack):  # used as anything but the input of the first conv: materialise
        t = t.tensor()
    if not t.is_cuda:
        raise AivcNativeError('aivc_amd.ops: %s is on %s; the HIP path needs CUDA tensors '
                              '(no CPU fallback)' % (name, t.device))
    if dtype is not None and t.dtype != dtype:
        raise AivcNativeError('aivc_amd.ops: %s has dtype %s, expected %s' % (name, t.dtype, dtype))
    return t if t.is_contiguous() else t.contiguous()


def _shaped(t, dtype, shape, name='tensor'):
    """_dev of a tensor of this dtype and EXACTLY this shape (None on an axis: any size; t None stays None).  The kernels see an
    address and the integers of the call: what the two say about each other is checked here, from the tensor's attributes alone."""
    if t is None:
        return None
    t = _dev(t, dtype, name)
    if t.shape != shape and (t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape))):
        raise ValueError('aivc_amd.ops: %s has shape %s, expected [%s]'
                         % (name, tuple(t.shape), ', '.join('any' if s is None else str(int(s)) for s in shape)))
    return t


def _out(t, dtype, shape, name, device=None, at_least=False):
    """a caller's output, which the kernel writes in place: nothing can be converted or copied for it, so it IS a contiguous
    tensor of this dtype on this device (None: any GPU), of exactly this shape or (at_least) of at least shape[0] rows of it -> t"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or (device is not None and t.device != device):
        raise AivcNativeError('aivc_amd.ops: %s is %s; an output is a CUDA tensor on %s'
                              % (name, 'on %s' % t.device if isinstance(t, torch.Tensor) else type(t).__name__, device or 'the GPU'))
    if t.dtype != dtype:
        raise AivcNativeError('aivc_amd.ops: %s has dtype %s, expected %s' % (name, t.dtype, dtype))
    if not t.is_contiguous():
        raise ValueError('aivc_amd.ops: %s is not contiguous (a copy would lose the result)' % name)
    ok = t.dim() == len(shape) and tuple(t.shape[1:]) == tuple(int(s) for s in shape[1:]) \
        and (t.shape[0] >= shape[0] if at_least else t.shape[0] == shape[0])
    if not ok:
        raise ValueError('aivc_amd.ops: %s has shape %s, expected %s%s' % (name, tuple(t.shape), 'at least ' if at_least else '',
                                                                         tuple(int(s) for s in shape)))
    return t


def _p(t):
    return None if t is None else t.data_ptr()


# NCHW (logical, torch module API) <-> NHWC (physical, kernels) -------------------------------
def to_nhwc(x):
    """[n,c,h,w] tensor (any strides) -> contiguous [n,h,w,c] (free when x is channels_last)."""
    return x.permute(0, 2, 3, 1).contiguous()


def to_nchw_view(x):
    """[n,h,w,c] contiguous -> logical [n,c,h,w] view (channels_last strides, no copy)."""
    return x.permute(0, 3, 1, 2)


def pad_channels(x, c_out):
    x = _dev(x, torch.float32, 'x')
    c_in = x.shape[-1]
    if c_in == c_out:
        return x
    if c_out < c_in:
        raise ValueError('pad_channels: %d channels cannot be padded to %d' % (c_in, c_out))
    out = torch.empty(x.shape[:-1] + (c_out,), dtype=torch.float32, device=x.device)
    call('aivc_pad_channels', _p(x), x.numel() // c_in, c_in, _p(out), c_out, _stream())
    return out


def pack_weight(w, c_store=None, transposed=False):
    """torch Conv2d weight [O,I,kh,kw] (ConvTranspose2d: [I,O,kh,kw]) -> OHWI fp32 contiguous with
    the input-channel axis zero padded to c_store (pure data movement, done once per layer)."""
    w = w.detach()
    if transposed:
        w = w.permute(1, 0, 2, 3)
    w = w.permute(0, 2, 3, 1)
    ci = w.shape[3]
    c_store = ci if c_store is None else c_store
    if c_store != ci:
        wp = torch.zeros(w.shape[:3] + (c_store,), dtype=torch.float32, device=w.device)
        wp[..., :ci] = w
        return wp
    return w.contiguous().float()


# The arithmetic contract the conv family computes in (see set_precision()).  Default since round 6: VERSION 2 of the fp32
# contract ('fp32w': Winograd F(2x2, 3x3) chains for the stride-1 3x3 layers it covers) -- as exact as version 1 in the sense
# that matters (HIP == CPU oracle bit for bit, bitstreams reproducible on every GPU), closer to the reference's outputs on the
# layer fixtures, and 1.4 ... 1.6x faster on the layers it covers.  AIVC_CONTRACT=fp32 in the environment selects version 1
# (an encoder and a decoder must run the same version: their bits differ).
_PRECISION_NAMES = {'fp32': abi.PREC_FP32, 'bf16x3': abi.PREC_BF16X3, 'fp32w': abi.PREC_FP32_WINO}  # what set_precision() takes
_CONTRACT_NAMES = {k: _PRECISION_NAMES[k] for k in ('fp32', 'fp32w')}  # ... of which the versions of the contract
DEFAULT_CONTRACT = os.environ.get('AIVC_CONTRACT', 'fp32w')
if DEFAULT_CONTRACT not in _CONTRACT_NAMES:
    raise ValueError('AIVC_CONTRACT=%r: expected fp32 or fp32w' % DEFAULT_CONTRACT)
PRECISION = _CONTRACT_NAMES[DEFAULT_CONTRACT]


def precision_name():
    """the name set_precision() knows the current mode by"""
    return next(k for k, v in _PRECISION_NAMES.items() if v == PRECISION)


def set_precision(mode):
    """'fp32': version 1 of the arithmetic contract (9-tap chains) -- HIP == CPU oracle bit for bit, bitstreams reproducible on every GPU.
    'bf16x3': the precision MODE of the wide convolutions (include/aivc_hip.h, aivc_conv_params.precision): fp32 operands
    as three bf16 terms, six bf16 MFMA products per fp32 product, fp32 accumulation.  Results are within fp32
    summation-order noise of the contract's, not its bits: an encoder and a decoder must run the same mode.
    'fp32w' (the default, DEFAULT_CONTRACT): version 2 of the fp32 contract (AIVC_PREC_FP32_WINO): the stride-1 3x3 layers with c_in % 32 == 0 and
    c_out % 64 == 0 accumulate along Winograd F(2x2, 3x3) chains (16 instead of 36 multiplications per 2x2 outputs);
    everything else as 'fp32'.  HIP == CPU oracle bit for bit in this version too; its bits are not version 1's.
    -> the previous mode's name.  Process-wide (the codec's side streams read it too)."""
    global PRECISION
    if mode not in _PRECISION_NAMES:
        raise ValueError('precision %r: expected one of %s' % (mode, sorted(_PRECISION_NAMES)))
    prev = precision_name()
    PRECISION = _PRECISION_NAMES[mode]
    return prev


_DERIVED_WEIGHTS = {}  # (id(weight tensor), transform) -> (weak reference, (data_ptr, version), image); dies with the weight


def _derived_weights(w_ohwi, fn, numel, dtype, *dims):
    """fn(w_ohwi, *dims, out) into a fresh tensor of numel elements, once per weight tensor and version.  The codec's side
    streams launch convolutions too, so the (one-off) transform is closed with a device-wide wait like every other
    kernel-ready parameter (layers/_cache.py)."""
    import weakref
    key = (id(w_ohwi), fn)
    stamp = (w_ohwi.data_ptr(), w_ohwi._version)
    hit = _DERIVED_WEIGHTS.get(key)
    if hit is not None and hit[0]() is w_ohwi and hit[1] == stamp:
        return hit[2]
    out = torch.empty(numel, dtype=dtype, device=w_ohwi.device)
    torch.cuda.synchronize(w_ohwi.device)
    call(fn, _p(w_ohwi), *dims, _p(out), _stream())
    torch.cuda.synchronize(w_ohwi.device)
    _DERIVED_WEIGHTS[key] = (weakref.ref(w_ohwi, lambda _r, k=key: _DERIVED_WEIGHTS.pop(k, None)), stamp, out)
    return out


def split_weights_bf16x3(w_ohwi):
    """aivc_split_weights_bf16x3 of an OHWI weight, once per tensor and version (aivc_conv_params.w_bf16x3)"""
    co = w_ohwi.shape[0]
    k_total = w_ohwi.numel() // co
    return _derived_weights(w_ohwi, 'aivc_split_weights_bf16x3', co * k_total * 6, torch.uint8, co, k_total)


def winograd_weights(w_ohwi, transposed=False):
    """aivc_winograd_weights of an OHWI 3x3 weight ([co, 3, 3, ci] -> co * 16 * ci floats), aivc_winograd_weights_poly5 of a 5x5
    stride-2 one (4 ci virtual input channels) or, transposed, aivc_winograd_weights_tconv5 (4 co virtual output channels), once per
    tensor and version (aivc_conv_params.w_wino), in the kernels' staging order (AIVC_WINO_U_INDEX)"""
    co, k, _, ci = w_ohwi.shape
    fn = 'aivc_winograd_weights_tconv5' if transposed else ('aivc_winograd_weights_poly5' if k == 5 else 'aivc_winograd_weights')
    return _derived_weights(w_ohwi, fn, co * 16 * ci * (4 if k == 5 else 1), torch.float32, co, ci)


WINO_ANY_SIZE = False  # tests: fp32w on images below AIVC_WINO_MIN_PIXELS too (aivc_conv_params.flags, AIVC_CONV_WINO_ANY_SIZE)
PRESPLIT_WEIGHTS = True  # bf16x3 mode: hand the kernels the split weights (False: they split in their K loop; same bits)
# Winograd codes of aivc_conv2d_variant -> (multiplications per 2 x 2 tile and channel pair, whether the tiles cover the OUTPUT
# pixel grid rather than the input's)
_WINO_VARIANTS = {301: (16, False), 302: (49, True), 303: (49, False)}


def _profiled(launch, variant, mode, k, stride, c_real, co, n, h, w, ho, wo, fused_gdn=False, co2=0):
    """launch() of one conv kernel -> what it returned.  While PROFILE is on (bench.py), HIP events on the launch stream
    bracket it and a launch that succeeded appends (variant, algorithmic FLOPs, e0, e1, shape) to PROFILE."""
    if PROFILE is None:
        return launch()
    pix = n * h * w if mode == abi.MODE_TCONV else n * ho * wo
    flops = 2.0 * k * k * c_real * co * pix + (2.0 * co * co * n * ho * wo if fused_gdn else 0.0) + 2.0 * co * co2 * n * ho * wo
    if variant in _WINO_VARIANTS:
        # version 2 of the contract: what the matrix pipe EXECUTES (3x3: 16 multiplications per tile of 2 x 2 outputs and
        # channel pair instead of 36; 5x5 stride 2 in polyphase form / transposed by classes: 49 instead of 100, the
        # transposed form on its grid of input pixels) -- a roofline fraction is priced on issued work; the tap chain's count
        # is kept beside it
        mults, on_output = _WINO_VARIANTS[variant]
        gh, gw = (ho, wo) if on_output else (h, w)
        PROFILE_DIRECT_EQUIVALENT[0] += flops
        flops = 2.0 * mults * c_real * co * n * ((gh + 1) // 2) * ((gw + 1) // 2)
        PROFILE_DIRECT_EQUIVALENT[1] += flops
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = launch()
    e1.record()
    if not rc:
        PROFILE.append((variant, flops, e0, e1, (mode, k, stride, c_real, co, n, h, w, fused_gdn)))
    return rc


def _two_launches(x, w_ohwi, bias, mode, stride, pad, act1, act2, mul, res, algo, g, tail, frame_h):
    """a fused (I)GDN or 1x1 tail the kernels cannot take for this shape: the same arithmetic in two launches"""
    if tail is not None:
        t = conv2d(x, w_ohwi, bias, stride=stride, pad=pad, act1=act1, algo=algo, frame_h=frame_h)
        return conv2d(t, tail[0], tail[1], res=res, act2=act2, algo=algo,
                      frame_h=None if frame_h is None else abi.conv_out_size(abi.MODE_CONV, frame_h, 1, w_ohwi.shape[1], stride, pad)[0])
    if act1 or act2 or mul is not None:
        raise AivcNativeError('conv2d: fused gdn with act/mul epilogue needs a fusable shape')
    t = conv2d(x, w_ohwi, bias, mode=mode, stride=stride, pad=pad, algo=algo, frame_h=frame_h)
    return gdn(t, g[0], g[1], inverse=g[2], res=res, algo=algo,
               frame_h=None if frame_h is None else abi.conv_out_size(mode, frame_h, 1, w_ohwi.shape[1], stride, pad)[0])


def slab_contract(p, frame_h):
    """-> (precision, flags) for the launch p on a row slab (aivc_amd/bands.py) cut from a map of frame_h rows, under
    version 2 of the contract.  Version 2 decides on the size of the tensor a launch is given (aivc_winograd_covers) and a slab
    is much smaller than its map, so the library is asked which family the WHOLE map's launch takes (aivc_conv2d_variant on p
    with the map's rows: the rule still lives in one place) and the slab follows it:
      * a Winograd code -> version 2 whatever the slab's size (AIVC_CONV_WINO_ANY_SIZE);
      * no code (a covered layer with a fused gdn, which the map splits into two launches) -> the same, so the slab's
        launch is split too, and each half decides again;
      * any other code -> version 1, which is what version 2 computes outside the covered set.
    Only p's copy is changed; p itself is the caller's to update."""
    f = abi.ConvParams.from_buffer_copy(p)
    f.h_in, f.h_out = frame_h, abi.conv_out_size(p.mode, frame_h, p.w_in, p.ksize, p.stride, p.pad)[0]
    f.precision = abi.PREC_FP32_WINO
    variant = load()['aivc_conv2d_variant'](C.byref(f))
    if variant in _WINO_VARIANTS or variant < 0:
        return abi.PREC_FP32_WINO, p.flags | abi.CONV_WINO_ANY_SIZE
    return abi.PREC_FP32, p.flags


def conv2d(x, w_ohwi, bias=None, mode=abi.MODE_CONV, stride=1, pad=0, act1=0, act2=0, mul=None,
           res=None, algo=abi.ALGO_AUTO, gdn=None, tail=None, frame_h=None):
    """x [n,h,w,c] -> y [n,ho,wo,co]; semantics of aivc_conv2d (include/aivc_hip.h).
    gdn = (beta_eff, gamma_eff, inverse) fuses the (inverse) GDN into the conv epilogue when the
    kernels can (all channels of a pixel in one tile), else it is issued as a second launch --
    bit-identical either way.
    tail = (w3 [co2,1,1,co], b3): a 1x1 conv applied to act1(conv + bias) in the same launch when the kernels
    can, else as a second launch (bit-identical); res / act2 then belong to the tail and y is [n,ho,wo,co2].
    frame_h: x is a row slab (n = 1) of a map of frame_h rows (aivc_amd/bands.py); the launch then computes in the
    version of the contract the whole map's would (slab_contract)."""
    if not isinstance(x, ImageStack) and getattr(x, '_aivc_cmap', None) == (0, 1, 2) and x.dim() == 4 and x.shape[-1] == 4 \
            and mode == abi.MODE_CONV and tail is None:
        st = ImageStack([x], x.shape[1], x.shape[2], x.device)  # a single float image (the prediction fed to g_a_ref)
        st._packed = x
        x = st
    # every tensor against the integers of the launch, before the first kernel of the call (packing, padding, a first half)
    if not isinstance(x, ImageStack):
        x = _shaped(x, torch.float32, (None,) * 4, 'x')
    n, h, w_, c = x.shape
    w_ohwi = _shaped(w_ohwi, torch.float32, (None,) * 4, 'weight')
    co, k, k2, cw = w_ohwi.shape
    if k2 != k:
        raise ValueError('conv2d: a %d x %d kernel; the kernels are square' % (k, k2))
    if cw != (c + 3) // 4 * 4:
        raise AivcNativeError('conv2d: weight packed for %d stored channels, input has %d' % (cw, (c + 3) // 4 * 4))
    co2, w3, b3 = 0, None, None
    if tail is not None:
        w3 = _shaped(tail[0], torch.float32, (None, 1, 1, (co + 3) // 4 * 4), 'tail weight')
        co2 = w3.shape[0]
        b3 = _shaped(tail[1], torch.float32, (co2,), 'tail bias')
        tail = (w3, b3)
    ho, wo = abi.conv_out_size(mode, h, w_, k, stride, pad)
    bias = _shaped(bias, torch.float32, (co,), 'bias')
    mul = _shaped(mul, torch.float32, (n, ho, wo, co2 or co), 'mul')
    res = _shaped(res, torch.float32, (n, ho, wo, co2 or co), 'res')
    if gdn is not None:  # (the fused epilogue reads them as they lie: contiguous fp32 on the device, like every other operand)
        gdn = (_shaped(gdn[0], torch.float32, (co,), 'gdn beta'), _shaped(gdn[1], torch.float32, (co, co), 'gdn gamma'), gdn[2])
    if isinstance(x, ImageStack):
        y = None
        if tail is None and mode == abi.MODE_CONV:
            y = _conv_images(x, w_ohwi, bias, stride, pad, act1, act2, mul, res, algo, gdn)
        if y is not None:
            return y
        x = x.tensor()
    if tail is not None:
        if not (c % 4 == 0 and co % 4 == 0 and bias is not None and b3 is not None):
            return _two_launches(x, w_ohwi, bias, mode, stride, pad, act1, act2, mul, res, algo, gdn, tail, frame_h)
        c_real, flags = c, 0  # (a tail launch counts stored channels)
    else:
        cmap = getattr(x, '_aivc_cmap', None)
        c_real = c if cmap is None else len(cmap)  # algorithmic FLOPs count real channels, not zero padding
        if c % 4:
            x = pad_channels(x, (c + 3) // 4 * 4)
            c = x.shape[-1]
        # 3-channel images stored as 4: the zero pad channels are exact no-ops the MFMA kernels may skip
        flags = abi.CONV_SPARSE4 if cmap is not None and all(ci % 4 != 3 for ci in cmap) else 0
        if WINO_ANY_SIZE:
            flags |= abi.CONV_WINO_ANY_SIZE
    y = torch.empty((n, ho, wo, co2 or co), dtype=torch.float32, device=x.device)
    g_beta, g_gamma, gflag = (None, None, 0) if gdn is None else (gdn[0], gdn[1], 2 if gdn[2] else 1)
    p = abi.ConvParams(mode, k, stride, pad, n, h, w_, c, ho, wo, co, act1, act2, algo, gflag, flags,
                       _p(x), _p(w_ohwi), _p(bias), _p(mul), _p(res), _p(y), _p(g_beta), _p(g_gamma))
    if co2:
        p.tail_w, p.tail_bias, p.tail_c_out = _p(w3), _p(b3), co2
    p.precision = PRECISION
    if frame_h is not None and PRECISION == abi.PREC_FP32_WINO:
        p.precision, p.flags = slab_contract(p, frame_h)
    # which kernel the library will launch (aivc_conv2d_variant): the one place the dispatch rule lives
    variant = load()['aivc_conv2d_variant'](C.byref(p))
    if variant < 0 and (gdn is not None or co2):  # no fused kernel for this shape
        return _two_launches(x, w_ohwi, bias, mode, stride, pad, act1, act2, mul, res, algo, gdn, tail, frame_h)
    w_derived = None  # (referenced until the launch has been issued)
    if variant in _WINO_VARIANTS:  # version 2 of the contract: the kernel reads the transformed weights
        w_derived = winograd_weights(w_ohwi, transposed=mode == abi.MODE_TCONV)
        p.w_wino = _p(w_derived)
    elif variant >= 1000 and PRESPLIT_WEIGHTS:  # a launch the precision mode covers
        w_derived = split_weights_bf16x3(w_ohwi)
        p.w_bf16x3 = _p(w_derived)
        variant = load()['aivc_conv2d_variant'](C.byref(p))  # (the mode's tile depends on the split weights)
    _profiled(lambda: call('aivc_conv2d', C.byref(p), _stream()), variant, mode, k, stride, c_real, co, n, h, w_, ho, wo,
              gdn is not None, co2)
    return y


def gdn_reparam(beta, gamma, beta_bound, gamma_bound, pedestal):
    beta = _shaped(beta.detach(), torch.float32, (None,), 'beta')
    c = beta.shape[0]
    gamma = _shaped(gamma.detach(), torch.float32, (c, c), 'gamma')
    be = torch.empty_like(beta)
    ge = torch.empty_like(gamma)
    call('aivc_gdn_reparam', _p(beta), _p(gamma), c, float(beta_bound), float(gamma_bound),
         float(pedestal), _p(be), _p(ge), _stream())
    return be, ge


def selfcheck_gdn_math(n_div_pairs=1 << 34, seed=1, device=None):
    """-> (sqrt mismatches over every float of the safe range, division mismatches over n_div_pairs random pairs):
    the lean sequences of the fused GDN epilogues against the compiler's IEEE sqrt / division (aivc_selfcheck_gdn_math)"""
    out = torch.zeros(2, dtype=torch.int64, device=device or torch.device('cuda'))
    call('aivc_selfcheck_gdn_math', int(n_div_pairs), int(seed), _p(out), _stream())
    return tuple(int(v) for v in out.cpu())


def diag_hold_lds(lds_bytes, iterations, out=None):
    """one workgroup that holds lds_bytes of LDS on the current stream for `iterations` dependent LDS reads
    (aivc_diag_hold_lds, a diagnostic for the tests and tools of the persistent kernels) -> the 64 chain ends, int32"""
    if out is None:
        out = torch.empty(64, dtype=torch.int32, device=torch.device('cuda'))
    else:
        _out(out, torch.int32, (64,), 'out')
    call('aivc_diag_hold_lds', int(lds_bytes), int(iterations), _p(out), _stream())
    return out


def detmath_eval(fn, a, b=None):
    """out[i] = fn(a[i]) or fn(a[i], b[i]) for one function of include/aivc_detmath.h on the device (aivc_detmath_eval, a
    diagnostic): fn one of abi.DETMATH_*, a / b / out float64 for the fp64 cores and float32 for everything else"""
    dt = torch.float64 if abi.detmath_is_fp64(fn) else torch.float32
    a, b = _dev(a, dt, 'a'), _dev(b, dt, 'b')
    if abi.detmath_operands(fn) == 2 and (b is None or b.shape != a.shape):
        raise AivcNativeError('aivc_amd.ops.detmath_eval: function %d takes two operands of one shape' % fn)
    out = torch.empty_like(a)
    call('aivc_detmath_eval', int(fn), _p(a), _p(b), a.numel(), _p(out), _stream())
    return out


def gdn(x, beta_eff, gamma_eff, inverse=False, res=None, algo=abi.ALGO_AUTO, frame_h=None):
    c = x.shape[-1]
    mode = abi.MODE_IGDN if inverse else abi.MODE_GDN
    beta_eff, gamma_eff = _shaped(beta_eff, torch.float32, (c,), 'beta'), _shaped(gamma_eff, torch.float32, (c, c), 'gamma')
    if c % 4 == 0:
        return conv2d(x, gamma_eff.reshape(c, 1, 1, c), beta_eff, mode=mode, res=res, algo=algo, frame_h=frame_h)
    # channel counts that are not a multiple of 4 (never the case in a real model): run on a zero
    # padded copy (extra channels: x = 0, gamma = 0, beta = 1) and drop the padding
    c4 = (c + 3) // 4 * 4
    g = torch.zeros((c4, c4), dtype=torch.float32, device=x.device)
    g[:c, :c] = gamma_eff
    b = torch.ones(c4, dtype=torch.float32, device=x.device)
    b[:c] = beta_eff
    y = conv2d(pad_channels(x, c4), g.reshape(c4, 1, 1, c4), b, mode=mode,
               res=None if res is None else pad_channels(res, c4), algo=algo, frame_h=frame_h)
    return y[..., :c].contiguous()


def yuv420_to_444(y, u, v, c_store=4, c_off=0, out=None):
    """planes [n,h,w] / [n,ceil(h/2),ceil(w/2)] (fp32 levels or uint8) -> NHWC [n,h,w,c_store]"""
    u8 = y.dtype == torch.uint8
    dt = torch.uint8 if u8 else torch.float32
    y = _shaped(y, dt, (None,) * 3, 'y')
    n, h, w = y.shape
    u, v = (_shaped(t, dt, (n, (h + 1) // 2, (w + 1) // 2), nm) for t, nm in ((u, 'u'), (v, 'v')))
    if out is not None:
        _out(out, torch.float32, (n, h, w, c_store), 'out', y.device)
    if not 0 <= c_off <= c_store - 3:
        raise ValueError('yuv420_to_444: channels %d .. %d of %d stored ones' % (c_off, c_off + 2, c_store))
    if out is None:
        # the kernel writes channels c_off .. c_off + 2 (+ the zero pad channel): nothing else to clear when that is all
        full = c_off == 0 and c_store <= 4
        out = (torch.empty if full else torch.zeros)((n, h, w, c_store), dtype=torch.float32, device=y.device)
    zero_pad = 1 if out.shape[-1] >= c_off + 4 else 0
    hc, wc = (h + 1) // 2, (w + 1) // 2
    _hbm_profiled('yuv420_to_444', n * ((h * w + 2 * hc * wc) * (1 if u8 else 4) + h * w * 4 * (3 + zero_pad)),
                  lambda: call('aivc_yuv420u8_to_444' if u8 else 'aivc_yuv420_to_444', _p(y), _p(u), _p(v), n, h, w,
                               _p(out), out.shape[-1], c_off, zero_pad, _stream()))
    return out


# three images (K = 300, 113 KB of LDS: one workgroup per CU) measured slower than pack + generic conv (5.2 vs ~4.3 ms at
# 16 x 1080p), one and two images at par with the conv alone and without the packed tensor
_CONV_IMAGES_MAX = 2


def _n_frames(parts):
    return next(p['y'].shape[0] if isinstance(p, dict) else p.shape[0] for p in parts if p is not None)


def _image_sources(parts, h, w):
    """up to 3 image sources of h x w pixels (plane dicts, float NHWC tensors, None)
    -> (frames per image, ImageSrc array, tensors to keep alive)"""
    if not 1 <= len(parts) <= abi.MAX_IMAGES or all(p is None for p in parts):
        raise ValueError('image sources: %d of them (1 ... %d, not all absent)' % (len(parts), abi.MAX_IMAGES))
    n = _n_frames(parts)
    arr = (abi.ImageSrc * abi.MAX_IMAGES)()
    keep = []
    for i, p in enumerate(parts):
        if isinstance(p, dict):
            y = _shaped(p['y'], torch.uint8, (n, h, w), 'y')
            u, v = (_shaped(p[k], torch.uint8, (n, (h + 1) // 2, (w + 1) // 2), k) for k in 'uv')
            keep += [y, u, v]
            arr[i].y, arr[i].u, arr[i].v = y.data_ptr(), u.data_ptr(), v.data_ptr()
        elif p is not None:
            f = _shaped(p, torch.float32, (n, h, w, None), 'image')
            if f.shape[-1] < 3:
                raise ValueError('image sources: a float image of %d channels, at least 3' % f.shape[-1])
            keep.append(f)
            arr[i].f, arr[i].f_channels = f.data_ptr(), f.shape[-1]
    return n, arr, keep


class ImageStack:
    """The concatenation of up to 3 images (each stored as 3 real channels + a zero) as the first analysis conv sees
    it -- NOT materialised: conv2d() runs aivc_conv_images straight on the sources when the kernel covers the layer,
    and falls back to tensor() (aivc_pack_images) otherwise.  Quacks like the packed NHWC tensor for the few
    attributes the layers read (shape, device, _aivc_cmap)."""

    def __init__(self, parts, h, w, device):
        self.parts, self.h, self.w, self.device = list(parts), h, w, device
        self.n = _n_frames(parts)
        self.shape = (self.n, h, w, 4 * len(self.parts))
        self.dtype = torch.float32
        self._aivc_cmap = tuple(4 * i + c for i in range(len(self.parts)) for c in range(3))
        self._packed = None

    def sources(self):
        """(ImageSrc array, tensors to keep alive)"""
        return _image_sources(self.parts, self.h, self.w)[1:]

    def tensor(self):
        if self._packed is None:
            self._packed = pack_images(self.parts, self.h, self.w, self.device)
        return self._packed


def _conv_images(x, w_ohwi, bias, stride, pad, act1, act2, mul, res, algo, gdn):
    """aivc_conv_images on an ImageStack; None when the library declines the layer (caller packs and convolves)"""
    if mul is not None or res is not None or act2 or algo != abi.ALGO_AUTO or len(x.parts) > _CONV_IMAGES_MAX:
        return None
    w_ohwi = _dev(w_ohwi, torch.float32, 'weight')
    co, k, _, cw = w_ohwi.shape
    n, h, w_, c = x.shape
    if cw != c:
        return None
    ho, wo = abi.conv_out_size(abi.MODE_CONV, h, w_, k, stride, pad)
    y = torch.empty((n, ho, wo, co), dtype=torch.float32, device=x.device)
    bias = _dev(bias, torch.float32, 'bias')
    g_beta, g_gamma, gflag = (None, None, 0) if gdn is None else (gdn[0], gdn[1], 2 if gdn[2] else 1)
    p = abi.ConvParams(abi.MODE_CONV, k, stride, pad, n, h, w_, c, ho, wo, co, act1, 0, algo, gflag, abi.CONV_SPARSE4,
                       None, _p(w_ohwi), _p(bias), None, None, _p(y), _p(g_beta), _p(g_gamma))
    arr, keep = x.sources()
    rc = _profiled(lambda: load()['aivc_conv_images'](arr, len(x.parts), C.byref(p), _stream()), 191, abi.MODE_CONV, k, stride,
                   len(x._aivc_cmap), co, n, h, w_, ho, wo, gdn is not None)
    if rc == abi.ERR_UNSUPPORTED:
        return None
    if rc != 0:
        raise AivcNativeError('aivc_conv_images failed (%d)' % rc)
    del keep
    return y


def pack_images(parts, h, w, device):
    """parts: up to 3 sources, each a dict of uint8 planes {'y','u','v'} ([n,h,w] / [n,ceil(h/2),ceil(w/2)]), a
    float NHWC tensor [n,h,w,c>=3] (its first 3 channels are taken) or None (zeros) -> NHWC [n,h,w,4*len(parts)]
    with every image stored as (c0, c1, c2, 0); carries the stored position of the real channels for the conv."""
    n, arr, keep = _image_sources(parts, h, w)
    out = torch.empty((n, h, w, 4 * len(parts)), dtype=torch.float32, device=device)
    nb = n * h * w * (16 * len(parts) + sum(1.5 if isinstance(p, dict) else (12 if p is not None else 0) for p in parts))
    _hbm_profiled('pack_images', nb, lambda: call('aivc_pack_images', arr, len(parts), n, h, w, _p(out), _stream()))
    out._aivc_cmap = tuple(4 * i + c for i in range(len(parts)) for c in range(3))
    return out


def frame_to_yuv420(x, h, w, skip=None, want_float=True, want_u8=True):
    x = _shaped(x, torch.float32, (None,) * 4, 'x')
    n, hx, wx, cx = x.shape
    if not (0 <= h <= hx and 0 <= w <= wx and cx >= 3):
        raise ValueError('frame_to_yuv420: a frame of %d x %d (w x h) from x %s (at least that size, 3 channels)' % (w, h, tuple(x.shape)))
    skip = _shaped(skip, torch.float32, (n, h, w, None), 'skip')
    if skip is not None and skip.shape[-1] < 3:
        raise ValueError('frame_to_yuv420: skip has %d channels, at least 3' % skip.shape[-1])
    hc, wc = (h + 1) // 2, (w + 1) // 2
    dev = x.device
    f = [None] * 3
    b = [None] * 3
    if want_float:
        f = [torch.empty((n, h, w), dtype=torch.float32, device=dev),
             torch.empty((n, hc, wc), dtype=torch.float32, device=dev),
             torch.empty((n, hc, wc), dtype=torch.float32, device=dev)]
    if want_u8:
        b = [torch.empty((n, h, w), dtype=torch.uint8, device=dev),
             torch.empty((n, hc, wc), dtype=torch.uint8, device=dev),
             torch.empty((n, hc, wc), dtype=torch.uint8, device=dev)]
    # algorithmic bytes: the 3 real channels of x (and of skip) over the frame, the 4:2:0 planes out
    nb = n * (h * w * 3 * 4 * (2 if skip is not None else 1) + (h * w + 2 * hc * wc) * ((4 if want_float else 0) + (1 if want_u8 else 0)))
    _hbm_profiled('frame_to_yuv420', nb,
                  lambda: call('aivc_frame_to_yuv420', _p(x), n, hx, wx, cx, _p(skip), 0 if skip is None else skip.shape[-1],
                               h, w, _p(f[0]), _p(f[1]), _p(f[2]), _p(b[0]), _p(b[1]), _p(b[2]), _stream()))
    return tuple(f), tuple(b)


def rgb8_to_yuv420u8(rgb):
    """interleaved uint8 RGB [n,h,w,3] -> uint8 planes y [n,h,w], u and v [n,h//2,w//2]: Pillow's convert('YCbCr') bit for bit,
    chroma from sample (2i, 2j) alone (include/aivc_hip_color.h).  The chroma planes have the reference's FLOOR size, not the
    ceil size of the planar .yuv path (yuv420_to_444, frame_to_yuv420); the two agree for even h and w."""
    rgb = _dev(rgb, torch.uint8, 'rgb')
    if rgb.dim() != 4 or rgb.shape[-1] != 3:
        raise ValueError('rgb8_to_yuv420u8: expected [n, h, w, 3], got %s' % (tuple(rgb.shape),))
    n, h, w, _ = rgb.shape
    y = torch.empty((n, h, w), dtype=torch.uint8, device=rgb.device)
    u = torch.empty((n, h // 2, w // 2), dtype=torch.uint8, device=rgb.device)
    v = torch.empty((n, h // 2, w // 2), dtype=torch.uint8, device=rgb.device)
    empty = u.numel() == 0
    _hbm_profiled('rgb8_to_yuv420u8', n * (h * w * 4 + 2 * (h // 2) * (w // 2)),
                  lambda: call('aivc_rgb8_to_yuv420u8', _p(rgb), n, h, w, _p(y), None if empty else _p(u), None if empty else _p(v),
                               _stream()))
    return y, u, v


def yuv8_to_rgb8(y, u, v, chroma_shift=1):
    """uint8 planes y [n,h,w], u and v [n,ch,cw] -> interleaved uint8 RGB [n,h,w,3]: Pillow's YCbCr -> RGB bit for bit.
    chroma_shift = 1: half-resolution chroma of the floor or the ceil size, nearest x 2 and cropped; 0: full resolution."""
    y, u, v = _dev(y, torch.uint8, 'y'), _dev(u, torch.uint8, 'u'), _dev(v, torch.uint8, 'v')
    if y.dim() != 3 or u.dim() != 3 or u.shape != v.shape or u.shape[0] != y.shape[0]:
        raise ValueError('yuv8_to_rgb8: planes %s / %s / %s' % (tuple(y.shape), tuple(u.shape), tuple(v.shape)))
    n, h, w = y.shape
    ch, cw = u.shape[1:]
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=y.device)
    _hbm_profiled('yuv8_to_rgb8', n * (h * w * 4 + 2 * ch * cw),
                  lambda: call('aivc_yuv8_to_rgb8', _p(y), _p(u), _p(v), n, h, w, ch, cw, chroma_shift, _p(rgb), _stream()))
    return rgb


def _plane_batch(planes, op, dims=None, stack=True, empty=True):
    """The planes of one call of `op`: a list of contiguous uint8 CUDA tensors of one size on one device (views into a larger
    tensor as they are: a plane may start at any byte) or, with stack, one tensor [n, ...] whose rows are the planes.
    dims: the names of a plane's axes, ('h', 'w'): a plane of a list has that rank, or a leading 1 more, a stack [n, h, w];
    None: any shape, the planes of a list then only share their byte count.  empty: whether n = 0 is a batch.
    -> (tensors to keep alive, [address of each plane], shape of a plane, its bytes, device)"""
    if isinstance(planes, (list, tuple)):
        keep = [_dev(t, torch.uint8, 'planes[%d]' % i) for i, t in enumerate(planes)]
        sizes = sorted({t.numel() if dims is None else tuple(t.shape) for t in keep})
        if len(sizes) > 1:
            raise ValueError('%s: the planes of one call have one size, got %s' % (op, sizes))
        if len({t.device for t in keep}) > 1:
            raise ValueError('%s: planes on several devices' % op)
        shape = (tuple(keep[0].shape) if dims is not None else (keep[0].numel(),)) if keep else (0,)
        if dims is not None and keep and not (len(shape) == len(dims) or (len(shape) == len(dims) + 1 and shape[0] == 1)):
            raise ValueError('%s: expected planes [%s] or [1, %s], got %s' % (op, ', '.join(dims), ', '.join(dims), shape))
        ptrs, device = [t.data_ptr() for t in keep], keep[0].device if keep else None
    elif not stack:
        raise ValueError('%s: expected a list of planes, got %s' % (op, type(planes).__name__))
    else:
        planes = _dev(planes, torch.uint8, 'planes')
        if planes.dim() < 1 or (dims is not None and planes.dim() != len(dims) + 1):
            raise ValueError('%s: expected [n, %s], got %s' % (op, '...' if dims is None else ', '.join(dims), tuple(planes.shape) or 'a scalar'))
        n = planes.shape[0]
        shape = tuple(planes.shape[1:]) if dims is not None else (planes.numel() // n if n else 0,)
        keep, device = [planes], planes.device
        ptrs = [planes.data_ptr() + i * (planes.numel() // n) for i in range(n)]
    if not ptrs:
        if not empty:
            raise ValueError('%s: no planes' % op)
        device = device or torch.device('cuda', torch.cuda.current_device())
    return keep, ptrs, shape, int(np.prod(shape, dtype=np.int64)), device


def _stage_layout(sizes, align=16, slack=0):
    """where _stage puts arrays of these byte sizes: each on an `align` boundary with `slack` spare bytes behind its padded end
    -> ([offset of each], bytes of the blob: never none, at least `align`)"""
    offs, total = [], 0
    for s in sizes:
        offs.append(total)
        total += -(-s // align) * align + slack
    return offs, max(total, align)


_STAGING = []  # [(event recorded behind a pinned buffer's last copy, the buffer: a pinned uint8 tensor)]


def _stage(device, arrays, align=16, slack=0):
    """Small host tables (flat uint8 numpy arrays; range_decode hands in thousands of them a step, so nothing is done per array
    beyond the copy) -> (uint8 CUDA tensor holding their bytes laid out by _stage_layout and zeros everywhere else, [byte offset of
    each]).  One pinned staging buffer and one asynchronous copy on the device's current
    stream: the host never waits.
    THE RULE OF THE POOL: a pinned buffer goes back to _STAGING only behind an event recorded AFTER its copy, ON THE STREAM the
    copy was issued on, and is handed out again only once that event has completed.  Released any earlier, or behind an event of
    another stream, the next call would fill the buffer while the copy still reads it.  Both halves are here and nowhere else."""
    offs, total = _stage_layout([a.size for a in arrays], align, slack)
    for i, (ev, buf) in enumerate(_STAGING):
        if buf.numel() >= total and ev.query():
            _STAGING.pop(i)
            break
    else:
        buf = torch.empty(max(1 << 20, 1 << (total - 1).bit_length()), dtype=torch.uint8, pin_memory=True)
    host = buf.numpy()[:total]
    host[:] = 0
    for o, a in zip(offs, arrays):
        host[o:o + a.size] = a
    blob = torch.empty(total, dtype=torch.uint8, device=device)
    blob.copy_(buf[:total], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(blob.device))
    _STAGING.append((ev, buf))
    return blob, offs


def md5_planes(planes):
    """MD5 of n equal-sized uint8 buffers on the device (include/aivc_hip_digest.h): one message per lane, one launch.
    planes: a contiguous uint8 CUDA tensor [n, ...] (message i is planes[i]), or a list of n contiguous uint8 CUDA tensors of one
    size (views into a batch stack as they are: a message may start at any byte).  -> uint8 [n, 16] on the device, row i the
    digest of message i in RFC 1321 byte order (bytes(row).hex() == hashlib.md5(message).hexdigest()).  No synchronisation: the
    pointer table is one small host-to-device copy, the launch goes on the current stream."""
    keep, ptrs, _, length, device = _plane_batch(planes, 'md5_planes')
    n = len(ptrs)
    if length >= 1 << 31:
        raise ValueError('md5_planes: %d bytes per plane, the kernel takes less than 2^31' % length)
    out = torch.empty((n, 16), dtype=torch.uint8, device=device)
    if n == 0:
        return out
    table, _ = _stage(device, [np.asarray(ptrs, np.uint64).view(np.uint8)])
    _hbm_profiled('md5_planes', n * (length + 16), lambda: call('aivc_md5_batch', _p(table), length, n, _p(out), _stream()))
    del keep
    return out


def pair_sad_u8(planes):
    """Sums of absolute differences between consecutive planes (include/aivc_hip_scene.h): the scene-cut detector's input.
    planes: a list of n contiguous uint8 CUDA tensors of one size (the luma planes of a clip as read_yuv leaves them: separate
    tensors, any alignment).  -> int64 CUDA tensor [max(n - 1, 0)], entry i the exact sum of |planes[i + 1] - planes[i]|.
    No synchronisation: the pointer table is one small host-to-device copy, the two launches go on the current stream.
    n <= 1 launches nothing."""
    keep, ptrs, _, length, device = _plane_batch(planes, 'pair_sad_u8', stack=False)
    n = len(ptrs)
    sad = torch.empty((max(n - 1, 0),), dtype=torch.int64, device=device)
    if n <= 1:
        return sad
    if length == 0:
        raise ValueError('pair_sad_u8: empty planes')
    table, _ = _stage(device, [np.asarray(ptrs, np.uint64).view(np.uint8)])
    partials = torch.empty((n - 1, abi.SAD_BLOCKS), dtype=torch.int64, device=device)
    _hbm_profiled('pair_sad_u8', n * length, lambda: call('aivc_pair_sad_u8', _p(table), n, length, _p(partials), _p(sad), _stream()))
    del keep
    return sad


def resize_u8(planes, h_out, w_out, filter='bicubic'):
    """Pillow's Image.resize of 8-bit single-channel planes, byte for byte (include/aivc_hip_resize.h; filter: box, bilinear,
    hamming, bicubic or lanczos).  planes: a list of n contiguous uint8 CUDA tensors of one size, [h, w] or [1, h, w] (the planes
    of a clip as read_yuv leaves them: separate tensors, any alignment), or one uint8 CUDA tensor [n, h, w].
    -> uint8 CUDA tensor [n, h_out, w_out].  The coefficient tables come from the host (aivc_amd/resize.py, cached per axis and
    filter) in the same small host-to-device copy as the pointer table; the launches go on the current stream, no synchronisation.
    A shape the kernels cannot take raises ValueError with the sizes named, before anything is allocated."""
    from . import resize as rs
    rs.check_filter(filter)
    keep, ptrs, shape, _, device = _plane_batch(planes, 'resize_u8', ('h', 'w'), empty=False)
    n, (h_in, w_in), h_out, w_out = len(ptrs), shape[-2:], int(h_out), int(w_out)
    if min(h_in, w_in, h_out, w_out) < 1:
        raise ValueError('resize_u8: %d x %d -> %d x %d (w x h): every side must be at least 1' % (w_in, h_in, w_out, h_out))
    what = '%d planes of %d x %d -> %d x %d (w x h, %s)' % (n, w_in, h_in, w_out, h_out, filter)
    tiles = -(-w_out // abi.RESIZE_TILE_W)
    if tiles > 65535 or -(-n * h_in // 16) > 0x7fffffff or n * -(-h_out // 16) > 0x7fffffff \
            or ((h_in, w_in) == (h_out, w_out) and n > 65535):
        raise ValueError('resize_u8: %s is more than one launch can express (65535 tiles of %d columns, 2^31 - 1 tiles of 16 rows; '
                         '65535 planes where nothing changes size)' % (what, abi.RESIZE_TILE_W))
    xt = rs.device_tables(w_in, w_out, filter, abi.RESIZE_TILE_W) if w_out != w_in else None
    yt = rs.device_tables(h_in, h_out, filter, 16) if h_out != h_in else None
    if xt is not None and xt[2] > abi.RESIZE_MAX_SPAN:
        raise ValueError('resize_u8: %s: a tile of %d output columns reads %d input columns with %d taps, the horizontal pass holds '
                         'at most %d per row' % (what, abi.RESIZE_TILE_W, xt[2], xt[1].shape[0], abi.RESIZE_MAX_SPAN))
    # one blob: the pointer table, then the tables of the passes, each on a 16-byte boundary
    blob, offs = _stage(device, [np.asarray(ptrs, np.uint64).view(np.uint8)]
                         + [np.ascontiguousarray(a).reshape(-1).view(np.uint8) for t in (xt, yt) if t is not None for a in t[:2]])
    base = blob.data_ptr()
    at = iter(offs[1:])
    xb, xk = (base + next(at), base + next(at)) if xt is not None else (None, None)
    yb, yk = (base + next(at), base + next(at)) if yt is not None else (None, None)
    out = torch.empty((n, h_out, w_out), dtype=torch.uint8, device=device)
    tmp = None
    if xt is not None and yt is not None:  # the horizontal pass's result, rows padded to 4 bytes
        tmp = torch.empty(n * h_in * (-(-w_out // 4) * 4), dtype=torch.uint8, device=device)

    def launch():
        call('aivc_resize_u8', base, n, h_in, w_in, h_out, w_out, xb, xk, 0 if xt is None else xt[1].shape[0],
             0 if xt is None else xt[2], yb, yk, _p(tmp), _p(out), _stream())
    _hbm_profiled('resize_u8', n * (h_in * w_in + h_out * w_out), launch)
    del keep
    return out


def _rawvideo_layout(fmt, w, h, layout, op):
    from . import rawvideo
    fmt = rawvideo.PixFmt(fmt)
    w, h = int(w), int(h)
    if w < 1 or h < 1:
        raise ValueError('%s: a frame of %d x %d (w x h): every side must be at least 1' % (op, w, h))
    offsets, pitches, nbytes = fmt.layout(w, h) if layout is None else layout
    if nbytes >= 1 << 31:
        raise ValueError('%s: a %s frame of %d x %d is %d bytes, the kernel takes less than 2^31' % (op, fmt.name, w, h, nbytes))
    return fmt, fmt.struct(w, h, offsets, pitches), nbytes


def raw_to_yuv420u8(blob, offsets, fmt, w, h, layout=None):
    """Frames of a raw video layout -> the codec's 8-bit 4:2:0 planes (include/aivc_hip_rawvideo.h, where the arithmetic is stated).
    blob: a uint8 CUDA tensor that holds the frames, e.g. a stretch of a file as it is; offsets: the byte offset of each of the n
    frames in it -- ANY offsets: the frames of a .y4m lie behind `FRAME` lines; fmt: an aivc_amd.rawvideo.PixFmt or its name;
    w, h: the luma size; layout: (plane offsets, row pitches, bytes per frame) where the rows are not tight (pitched surfaces), default
    fmt.layout(w, h).  -> (y [n, h, w], u, v [n, ceil(h/2), ceil(w/2)]) uint8 CUDA tensors.  One launch for all frames and planes on
    the current stream; the pointer table is one small host-to-device copy; no synchronisation."""
    blob = _dev(blob, torch.uint8, 'blob').reshape(-1)
    fmt, st, nbytes = _rawvideo_layout(fmt, w, h, layout, 'raw_to_yuv420u8')
    offsets = [int(o) for o in offsets]
    n, hc, wc = len(offsets), (st.h + 1) // 2, (st.w + 1) // 2
    if offsets and (min(offsets) < 0 or max(offsets) + nbytes > blob.numel()):
        raise ValueError('raw_to_yuv420u8: %s frames of %d bytes at offsets %d ... %d do not lie inside a blob of %d bytes'
                         % (fmt.name, nbytes, min(offsets), max(offsets), blob.numel()))
    y = torch.empty((n, st.h, st.w), dtype=torch.uint8, device=blob.device)
    u = torch.empty((n, hc, wc), dtype=torch.uint8, device=blob.device)
    v = torch.empty((n, hc, wc), dtype=torch.uint8, device=blob.device)
    if n == 0:
        return y, u, v
    table, _ = _stage(blob.device, [(np.asarray(offsets, np.uint64) + np.uint64(blob.data_ptr())).view(np.uint8)])
    _hbm_profiled('raw_to_yuv420u8', n * (nbytes + st.h * st.w + 2 * hc * wc),
                  lambda: call('aivc_rawvideo_to_yuv420u8', _p(table), n, C.byref(st), _p(y), _p(u), _p(v), _stream()))
    return y, u, v


def yuv420u8_to_raw(y, u, v, fmt, lead=b''):
    """The codec's 8-bit 4:2:0 planes -> frames of a raw video layout (4:2:0 and grey layouts: include/aivc_hip_rawvideo.h).
    y: uint8 CUDA tensor [n, h, w]; u, v: [n, ceil(h/2), ceil(w/2)] (ignored by a grey layout); fmt: a PixFmt or its name;
    lead: bytes to put in front of every frame (a .y4m file's b'FRAME\\n': the frames then lie at any byte).
    -> uint8 CUDA tensor [n, len(lead) + bytes per frame], the frames tight.  One launch on the current stream, no synchronisation."""
    y = _dev(y, torch.uint8, 'y')
    if y.dim() != 3:
        raise ValueError('yuv420u8_to_raw: expected y [n, h, w], got %s' % (tuple(y.shape),))
    n, h, w = y.shape
    fmt, st, nbytes = _rawvideo_layout(fmt, w, h, None, 'yuv420u8_to_raw')
    if fmt.chroma != abi.CHROMA_NONE and not (fmt.shift_x == 1 and fmt.shift_y == 1):
        raise ValueError('yuv420u8_to_raw: %s: only 4:2:0 and grey layouts are written (4:2:2 and 4:4:4 need an upsampling filter)'
                         % fmt.name)
    if fmt.chroma != abi.CHROMA_NONE:
        u, v = _dev(u, torch.uint8, 'u'), _dev(v, torch.uint8, 'v')
        want = (n, (h + 1) // 2, (w + 1) // 2)
        if tuple(u.shape) != want or tuple(v.shape) != want:
            raise ValueError('yuv420u8_to_raw: expected u and v %s, got %s and %s' % (want, tuple(u.shape), tuple(v.shape)))
    else:
        u = v = None
    lead = bytes(lead)
    out = torch.empty((n, len(lead) + nbytes), dtype=torch.uint8, device=y.device)
    if n == 0:
        return out
    ptrs = out.data_ptr() + len(lead) + np.arange(n, dtype=np.uint64) * np.uint64(len(lead) + nbytes)
    table, offs = _stage(y.device, [ptrs.astype(np.uint64).view(np.uint8), np.frombuffer(lead, np.uint8)])
    if lead:
        out[:, :len(lead)] = table[offs[1]:offs[1] + len(lead)]
    _hbm_profiled('yuv420u8_to_raw', n * (nbytes + h * w + (0 if u is None else 2 * u[0].numel())),
                  lambda: call('aivc_yuv420u8_to_rawvideo', _p(y), _p(u), _p(v), n, C.byref(st), _p(table), _stream()))
    return out


def png_encode(pix, filter=5):
    """8-bit pictures -> one zlib stream each, the payload of a PNG's IDAT chunk (include/aivc_hip_png.h; the container is
    aivc_amd.png.assemble).  pix: uint8 CUDA tensor [n, h, w, c], c = 1 (grey) or 3 (RGB); filter: 0 ... 4 for every row, 5 the
    smallest sum of absolute residuals per row.  -> a list of n bytes objects.  A picture's bytes depend on its pixels and the
    filter alone.  Batches of at most 256 MiB of pixels; per batch three launches and two host synchronisations: the segments'
    lengths and Adler sums, then the bytes."""
    from . import png, rawvideo
    pix = _dev(pix, torch.uint8, 'pix')
    if pix.dim() != 4:
        raise ValueError('png_encode: expected [n, h, w, c], got %s' % (tuple(pix.shape),))
    n, h, w, c = pix.shape
    if filter not in png.FILTERS:
        raise ValueError('png_encode: filter %r, expected 0 ... 5' % (filter,))
    if n == 0:
        return []
    rows, nseg, seg_stride, slot_bytes = png.segment_plan(h, w, c)
    lengths = png.segment_lengths(h, w, c)
    if rows * (1 + w * c) >= 1 << 31:
        raise ValueError('png_encode: a row of %d bytes, the kernel takes segments of less than 2^31' % (1 + w * c))
    per = max(1, rawvideo.BATCH_BYTES // (h * w * c))
    streams = []
    for i0 in range(0, n, per):
        part = pix[i0:i0 + per]
        k = part.shape[0]
        filt = torch.empty(k * nseg * seg_stride, dtype=torch.uint8, device=pix.device)
        slots = torch.empty(k * nseg * slot_bytes, dtype=torch.uint8, device=pix.device)
        info = torch.empty((k * nseg, abi.PNG_SEG_WORDS), dtype=torch.int32, device=pix.device)
        _hbm_profiled('png_deflate', k * h * (2 * w * c + 1),
                      lambda: call('aivc_png_deflate', _p(part), k, h, w, c, filter, rows, _p(filt), _p(slots), _p(info), _stream()))
        seg = info.cpu().numpy().view(np.uint32).astype(np.int64)  # (synchronises: the lengths)
        sizes = seg[:, 0].reshape(k, nseg)
        totals = 2 + sizes.sum(1) + 5 + 4  # header, segments, the final empty block, the Adler-32
        starts = np.concatenate([[0], np.cumsum(totals)[:-1]])
        dst = (starts[:, None] + 2 + np.cumsum(sizes, 1) - sizes).astype(np.uint64)
        table, _ = _stage(pix.device, [dst.reshape(-1).view(np.uint8)])
        out = torch.empty(int(totals.sum()), dtype=torch.uint8, device=pix.device)
        _hbm_profiled('png_gather', 2 * int(sizes.sum()),
                      lambda: call('aivc_png_gather', _p(slots), _p(info), _p(table), k, h, w, c, rows, _p(out), _stream()))
        host = out.cpu().numpy()  # (synchronises: the bytes)
        for j in range(k):
            adler = png.adler_fold(zip(lengths, seg[j * nseg:(j + 1) * nseg, 1].tolist(), seg[j * nseg:(j + 1) * nseg, 2].tolist()))
            lo, hi = int(starts[j]), int(starts[j] + totals[j])
            streams.append(host[lo:hi - 4].tobytes() + adler.to_bytes(4, 'big'))
    return streams


def _byte_pieces(stream):
    """a stream given as one bytes-like object or as a list of them (a PNG's IDAT payloads) -> [flat uint8 arrays]"""
    parts = stream if isinstance(stream, (list, tuple)) else (stream,)
    return [np.frombuffer(p, np.uint8) for p in parts]


def inflate_launch(streams, sizes, device, gap=0):
    """inflate() without the wait: -> ([the output of each stream: uint8 views into dst], info: int32 CUDA tensor [n, 4], dst).
    gap: bytes left untouched in front of every destination range and behind the last (tests)."""
    n = len(streams)
    sizes = [int(s) for s in sizes]
    if len(sizes) != n or n < 1:
        raise ValueError('inflate: %d streams, %d sizes (at least one stream)' % (n, len(sizes)))
    pieces = [_byte_pieces(s) for s in streams]
    src_n = [sum(p.size for p in ps) for ps in pieces]
    for i in range(n):
        if not (0 <= sizes[i] < 1 << 31 and src_n[i] < 1 << 31):
            raise ValueError('inflate: stream %d: %d bytes to %d bytes, the kernel takes less than 2^31' % (i, src_n[i], sizes[i]))
    device = torch.device(device)
    dst_off = np.cumsum([gap] + [s + gap for s in sizes])
    dst = torch.empty(max(int(dst_off[-1]), 1), dtype=torch.uint8, device=device)
    # one blob: the table, then every piece of every stream back to back -- a stream starts at whatever byte it falls on
    flat = [p for ps in pieces for p in ps]
    offs, _ = _stage_layout([32 * n] + [p.size for p in flat], 1)
    table = np.zeros((n, 4), np.uint64)
    table[:, 0] = np.cumsum([offs[1] if flat else 32 * n] + src_n)[:-1]
    table[:, 1], table[:, 2], table[:, 3] = src_n, dst_off[:-1], sizes
    blob, _ = _stage(device, [table.reshape(-1).view(np.uint8)] + flat, 1)
    info = torch.empty((n, 4), dtype=torch.int32, device=device)
    _hbm_profiled('inflate', sum(src_n) + sum(sizes),
                  lambda: call('aivc_inflate', _p(blob), _p(blob), n, max(src_n), max(sizes), _p(dst), _p(info), _stream()))
    return [dst[int(o):int(o) + s] for o, s in zip(dst_off[:-1], sizes)], info, dst


def inflate(streams, sizes, device, check=True, gap=0):
    """zlib streams -> their bytes on the device, all in ONE launch, a workgroup per stream (include/aivc_hip_png_read.h).
    streams: the n streams on the host, each a bytes-like object or a list of them that are taken back to back (the IDAT payloads of
    a PNG); sizes: the bytes each inflates to, EXACTLY.  One pinned staging buffer, one host-to-device copy, one copy of the status
    rows back.  -> a list of n uint8 CUDA tensors, views into one buffer where they lie back to back.  A stream that fails raises
    ValueError naming the first such stream and its status in words; with check=False nothing is raised and the call returns
    (the tensors, the status rows as a uint32 array [n, 4]: status, bytes produced, source bytes consumed, 0; the buffer)."""
    outs, info, dst = inflate_launch(streams, sizes, device, gap)
    rows = info.cpu().numpy().view(np.uint32)  # (synchronises)
    if not check:
        return outs, rows, dst
    for i in np.flatnonzero(rows[:, 0]):
        raise ValueError('inflate: stream %d: %s' % (i, abi.INFLATE_STATUS.get(int(rows[i, 0]), 'status %d' % rows[i, 0])))
    return outs


def png_unfilter_launch(filt, shapes):
    """png_unfilter() without the wait: -> ([pictures: uint8 views [h, w, c]], status: int32 CUDA tensor [n])"""
    from . import png
    shapes = [png.check_size(*s) for s in shapes]
    keep = [_dev(t, torch.uint8, 'filt[%d]' % i).reshape(-1) for i, t in enumerate(filt)]
    n = len(keep)
    if n < 1 or len(shapes) != n:
        raise ValueError('png_unfilter: %d filtered streams, %d shapes (at least one picture)' % (n, len(shapes)))
    need = [h * (1 + w * c) for h, w, c in shapes]
    for i in range(n):
        if keep[i].numel() != need[i] or need[i] >= 1 << 31:
            raise ValueError('png_unfilter: picture %d: %d filtered bytes for %d x %d x %d (w x h x c), expected %d, less than 2^31'
                             % (i, keep[i].numel(), shapes[i][1], shapes[i][0], shapes[i][2], need[i]))
    device = keep[0].device
    base = min(t.data_ptr() for t in keep)
    pix_off = np.cumsum([0] + [h * w * c for h, w, c in shapes])
    table = np.zeros((n, 4), np.uint64)
    table[:, 0] = [t.data_ptr() - base for t in keep]
    table[:, 1] = pix_off[:-1]
    table[:, 2] = [(h << 32) | w for h, w, _ in shapes]
    table[:, 3] = [c for _, _, c in shapes]
    blob, _ = _stage(device, [table.reshape(-1).view(np.uint8)])
    pix = torch.empty(int(pix_off[-1]), dtype=torch.uint8, device=device)
    status = torch.empty((n,), dtype=torch.int32, device=device)
    _hbm_profiled('png_unfilter', sum(need) + int(pix_off[-1]),
                  lambda: call('aivc_png_unfilter', base, _p(blob), n, max(need), _p(pix), _p(status), _stream()))
    del keep
    return [pix[int(o):int(o) + h * w * c].view(h, w, c) for o, (h, w, c) in zip(pix_off[:-1], shapes)], status


def png_unfilter(filt, shapes, check=True):
    """The filtered streams of PNG pictures (what inflate() gives for their IDAT payloads) -> the pixels, all in ONE launch, a
    wavefront per picture (include/aivc_hip_png_read.h).  filt: a list of n uint8 CUDA tensors on one device, any alignment;
    shapes: [(h, w, c)], c = 1 (grey) or 3 (RGB); picture i has h (1 + w c) filtered bytes.  -> a list of uint8 CUDA tensors
    [h, w, c], views into one buffer.  A filter type above 4 raises ValueError naming the picture; with check=False the call
    returns (the pictures, the status words as a uint32 array [n])."""
    pics, status = png_unfilter_launch(filt, shapes)
    words = status.cpu().numpy().view(np.uint32)  # (synchronises)
    if not check:
        return pics, words
    for i in np.flatnonzero(words):
        raise ValueError('png_unfilter: picture %d: %s' % (i, abi.PNG_UNFILTER_STATUS.get(int(words[i]), 'status %d' % words[i])))
    return pics


def downsample2x(x, ch0, nch):
    """NHWC x -> planar [n, nch, h//2, w//2] 2x2 means of channels ch0..ch0+nch-1 (OutputLayer)."""
    x = _shaped(x, torch.float32, (None,) * 4, 'x')
    n, h, w, c = x.shape
    if ch0 < 0 or nch < 0 or ch0 + nch > c:
        raise ValueError('downsample2x: channels %d .. %d of %d' % (ch0, ch0 + nch - 1, c))
    out = torch.empty((n, nch, h // 2, w // 2), dtype=torch.float32, device=x.device)
    call('aivc_downsample2x', _p(x), n, h, w, c, ch0, nch, _p(out), _stream())
    return out


WARP_INTERP = {'bilinear': abi.WARP_BILINEAR, 'nearest': abi.WARP_NEAREST, 'bicubic': abi.WARP_BICUBIC}
WARP_PAD = {'border': abi.WARP_BORDER, 'zeros': abi.WARP_ZEROS, 'reflection': abi.WARP_REFLECTION}


def warp(x, flow, interp='bilinear', pad='border', align_corners=True):
    """NHWC x [n, h, w, c], flow [n, h, w, 2] -> the reference's warp() in any of its sampling modes (include/aivc_hip_warp.h).
    The default call is the codec's mode on aivc_warp, as ever; every other mode runs warp_modes_kernel, which works on groups
    of 4 channels (other channel counts are zero padded for the call)."""
    if interp not in WARP_INTERP or pad not in WARP_PAD:
        raise ValueError('warp: interp %r / pad %r: expected one of %s and one of %s' % (interp, pad, sorted(WARP_INTERP), sorted(WARP_PAD)))
    x = _shaped(x, torch.float32, (None,) * 4, 'x')
    n, h, w, c = x.shape
    flow = _shaped(flow, torch.float32, (n, h, w, 2), 'flow')
    if interp == 'bilinear' and pad == 'border' and align_corners:
        out = torch.empty_like(x)
        call('aivc_warp', _p(x), _p(flow), n, h, w, c, _p(out), _stream())
        return out
    c4 = (c + 3) // 4 * 4
    x = pad_channels(x, c4)
    out = torch.empty_like(x)
    # algorithmic bytes: the frame in, the flow, the frame out (the footprints overlap: each input value counts once)
    _hbm_profiled('warp_modes', n * h * w * 4 * (2 * c4 + 2),
                  lambda: call('aivc_warp_modes', _p(x), _p(flow), n, h, w, c4, WARP_INTERP[interp], WARP_PAD[pad],
                               1 if align_corners else 0, _p(out), _stream()))
    return out if c4 == c else out[..., :c].contiguous()


def warp_blend(mof, prev, nxt, h, w, frame_type, co=4, want_aux=False, rows=None):
    """rows = (row0, n_rows): only that band of the frame -- mof is then the band of the MOFNet output (its row 0 =
    frame row row0), prev / nxt stay whole frames, the outputs are [n, n_rows, w, co] (aivc_warp_blend_rows)."""
    mof = _shaped(mof, torch.float32, (None,) * 4, 'mof')
    n, hm, wm, cm = mof.shape
    prev = _shaped(prev, torch.float32, (n, h, w, None), 'prev')
    nxt = _shaped(nxt, torch.float32, (n, h, w, prev.shape[-1]), 'next')
    dev = mof.device
    row0, nr = (0, h) if rows is None else rows
    if not (0 <= row0 and 0 <= nr <= hm and row0 + nr <= h and w <= wm and cm >= 6 and prev.shape[-1] >= 3 and co >= 3):
        raise ValueError('warp_blend: rows %d .. %d of a %d x %d frame (w x h), %d reference channels, %d output channels from a '
                         'MOFNet band %s' % (row0, row0 + nr - 1, w, h, prev.shape[-1], co, tuple(mof.shape)))
    pred = torch.empty((n, nr, w, co), dtype=torch.float32, device=dev)
    skip = torch.empty_like(pred)
    xw = alpha = beta = None
    if want_aux:
        xw = torch.empty_like(pred)
        alpha = torch.empty((n, nr, w), dtype=torch.float32, device=dev)
        beta = torch.empty((n, nr, w), dtype=torch.float32, device=dev)
    # algorithmic bytes: the 6 MOFNet maps, 3 channels of each reference used, pred + skip out
    n_ref = 2 if int(frame_type) == FRAME_B else 1
    nb = n * nr * w * 4 * (6 + 3 * n_ref + 2 * co + ((co + 2) if want_aux else 0))
    _hbm_profiled('warp_blend', nb,
                  lambda: call('aivc_warp_blend_rows', _p(mof), hm, wm, cm, _p(prev), _p(nxt), prev.shape[-1], n, h, w,
                               int(row0), int(nr), int(frame_type), _p(pred), _p(skip), _p(xw), co, _p(alpha), _p(beta),
                               _stream()))
    return {'pred': pred, 'skip': skip, 'x_warp': xw, 'alpha': alpha, 'beta': beta}


def hyper_params(hs, c, h, w):
    hs = _shaped(hs, torch.float32, (None,) * 4, 'hs')
    n, hh, wh, c2 = hs.shape
    if c2 != 2 * c:
        raise AivcNativeError('hyper_params: expected %d channels, got %d' % (2 * c, c2))
    if not (0 <= h <= hh and 0 <= w <= wh):
        raise ValueError('hyper_params: a crop of %d x %d (w x h) from a map of %d x %d' % (w, h, wh, hh))
    mu = torch.empty((n, h, w, c), dtype=torch.float32, device=hs.device)
    sigma = torch.empty_like(mu)
    call('aivc_hyper_params', _p(hs), n, hh, wh, c, h, w, _p(mu), _p(sigma), _stream())
    return mu, sigma


def _gain_vector(gain, t):
    """one gain per channel of t [..., c] (any shape of c elements; None stays None)"""
    if t.dim() < 1:
        raise ValueError('aivc_amd.ops: a tensor [..., c], got a scalar')
    return None if gain is None else _shaped(gain.detach().reshape(-1), torch.float32, (t.shape[-1],), 'gain')


def channel_gain(x, gain):
    x = _dev(x, torch.float32, 'x')
    gain = _gain_vector(gain, x)
    out = torch.empty_like(x)
    call('aivc_channel_gain', _p(x), _p(gain), x.numel() // x.shape[-1], x.shape[-1], _p(out), _stream())
    return out


def gain_interp(g_r, g_t, lam):
    g_r = _dev(g_r.detach().reshape(-1), torch.float32, 'g_r')
    g_t = _shaped(g_t.detach().reshape(-1), torch.float32, (g_r.numel(),), 'g_t')
    out = torch.empty_like(g_r)
    call('aivc_gain_interp', _p(g_r), _p(g_t), g_r.numel(), float(lam), _p(out), _stream())
    return out


def quantize_center(y, mu=None, gain_dec=None, want_yhat=True):
    y = _dev(y, torch.float32, 'y')
    mu = _shaped(mu, torch.float32, y.shape, 'mu')
    gain_dec = _gain_vector(gain_dec, y)
    q = torch.empty(y.shape, dtype=torch.int16, device=y.device)
    y_hat = torch.empty_like(y) if want_yhat else None
    call('aivc_quantize_center', _p(y), _p(mu), _p(gain_dec), y.numel() // y.shape[-1], y.shape[-1],
         _p(q), _p(y_hat), _stream())
    return q, y_hat


def dequantize(q, mu=None, gain_dec=None):
    q = _dev(q, torch.int16, 'q')
    mu = _shaped(mu, torch.float32, q.shape, 'mu')
    gain_dec = _gain_vector(gain_dec, q)
    out = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    call('aivc_dequantize', _p(q), _p(mu), _p(gain_dec), q.numel() // q.shape[-1], q.shape[-1], _p(out),
         _stream())
    return out


# ... with one gain row per image of the batch (include/aivc_hip_rates.h): x [n, ..., c], gains [n, c]
def _gain_rows(gains, n, c):
    if gains is None:
        return None
    gains = _dev(gains.detach(), torch.float32, 'gains')
    if tuple(gains.shape) != (n, c):
        raise AivcNativeError('gain rows: expected [%d, %d] (one row per image), got %s' % (n, c, list(gains.shape)))
    return gains


def _rows_dims(t):
    """a batch [n, ..., c] -> (n, positions per image, c)"""
    if t.dim() < 2:
        raise AivcNativeError('a batch is [n, ..., c] (with gain rows: one per image), got %s' % list(t.shape))
    n, c = t.shape[0], t.shape[-1]
    return n, (t.numel() // (n * c) if n * c else 0), c


def channel_gain_rows(x, gains):
    x = _dev(x, torch.float32, 'x')
    n, npix, c = _rows_dims(x)
    gains = _gain_rows(gains, n, c)
    out = torch.empty_like(x)
    call('aivc_channel_gain_rows', _p(x), _p(gains), n, npix, c, _p(out), _stream())
    return out


def quantize_center_rows(y, mu, gains_dec, want_yhat=True, want_q=True):
    y = _dev(y, torch.float32, 'y')
    mu = _shaped(mu, torch.float32, y.shape, 'mu')
    n, npix, c = _rows_dims(y)
    gains_dec = _gain_rows(gains_dec, n, c)
    q = torch.empty(y.shape, dtype=torch.int16, device=y.device) if want_q else None
    y_hat = torch.empty_like(y) if want_yhat else None
    call('aivc_quantize_center_rows', _p(y), _p(mu), _p(gains_dec), n, npix, c, _p(q), _p(y_hat), _stream())
    return q, y_hat


def dequantize_rows(q, mu, gains_dec):
    q = _dev(q, torch.int16, 'q')
    mu = _shaped(mu, torch.float32, q.shape, 'mu')
    n, npix, c = _rows_dims(q)
    gains_dec = _gain_rows(gains_dec, n, c)
    out = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    call('aivc_dequantize_rows', _p(q), _p(mu), _p(gains_dec), n, npix, c, _p(out), _stream())
    return out


# entropy model ---------------------------------------------------------------------------------
def balle_cdf_table(params, want_float=False):
    params = _shaped(params, torch.float32, (None, abi.BALLE_PARAMS), 'params')
    c = params.shape[0]
    table = torch.empty((c, abi.CDF_ROW), dtype=torch.int16, device=params.device)  # uint16 payload
    cdf = torch.empty((c, abi.LP), dtype=torch.float32, device=params.device) if want_float else None
    call('aivc_balle_cdf_table', _p(params), c, _p(table), _p(cdf), _stream())
    return (table, cdf) if want_float else table


def nonzero_flags(q):
    """q [n,h,w,c] int16 -> device uint8 [n, c] flags, one row per image (no host sync)"""
    q = _dev(q, torch.int16, 'q')
    n, npix, c = _rows_dims(q)
    flags = torch.empty((n, c), dtype=torch.uint8, device=q.device)
    for i0 in range(0, n, 65535):  # one launch for the whole batch (grid.y = image)
        m = min(65535, n - i0)
        call('aivc_nonzero_maps_batch', q.data_ptr() + 2 * i0 * npix * c, m, npix, c, flags.data_ptr() + i0 * c, _stream())
    return flags


def _one_image(sigma, maps, name='sigma'):
    """sigma [1,h,w,c] (one image) and the coded channels of it -> (sigma, npix, c, aivc_map_list)"""
    sigma = _shaped(sigma, torch.float32, (1, None, None, None), name)
    c = sigma.shape[-1]
    _check_maps(maps, c)
    return sigma, sigma.numel() // c if c else 0, c, abi.MapList.make(maps)


def _check_maps(maps, c):
    if any(not 0 <= int(m) < c for m in maps):
        raise ValueError('aivc_amd.ops: coded maps %s of a latent of %d channels' % (list(maps), c))


def _row_range(row_off, n_rows):
    if row_off < 0:
        raise ValueError('aivc_amd.ops: row_off %d' % row_off)
    return row_off + n_rows


def laplace_cdf_rows(sigma, maps, out=None, row_off=0):
    """sigma [1,h,w,c] (one image) -> rows [(len(maps)*npix), CDF_ROW]; with `out` given the rows are
    written starting at row `row_off` of that (larger) tensor."""
    sigma, npix, c, ml = _one_image(sigma, maps)
    if out is None:
        out = torch.empty((len(maps) * npix, abi.CDF_ROW), dtype=torch.int16, device=sigma.device)
        row_off = 0
    else:
        _out(out, torch.int16, (_row_range(row_off, len(maps) * npix), abi.CDF_ROW), 'out', sigma.device, at_least=True)
    # fp64-VALU bound, not HBM bound: 514 expm1 evaluations per coded position; the profile counts CDF POINTS
    _hbm_profiled('cdf_points:laplace_cdf_rows', len(maps) * npix * abi.LP,
                  lambda: call('aivc_laplace_cdf_rows', _p(sigma), npix, c, C.byref(ml),
                               out.data_ptr() + 2 * row_off * abi.CDF_ROW, _stream()))
    return out


def laplace_cdf_windows(sigma, maps, out=None, row_off=0):
    """Like laplace_cdf_rows, restricted to the decoder's fast-path window: -> (win [n_pos, CDF_WIN] int16,
    sigma_pos [n_pos] float32); with `out` = (win, sigma_pos) given, written from position `row_off` on."""
    sigma, npix, c, ml = _one_image(sigma, maps)
    if out is None:
        out = (torch.empty((len(maps) * npix, abi.CDF_WIN), dtype=torch.int16, device=sigma.device),
               torch.empty(len(maps) * npix, dtype=torch.float32, device=sigma.device))
        row_off = 0
    else:
        _out(out[0], torch.int16, (_row_range(row_off, len(maps) * npix), abi.CDF_WIN), 'out[0]', sigma.device, at_least=True)
        _out(out[1], torch.float32, (row_off + len(maps) * npix,), 'out[1]', sigma.device, at_least=True)
    win, sp = out
    _hbm_profiled('cdf_points:laplace_cdf_windows', len(maps) * npix * abi.CDF_WIN,
                  lambda: call('aivc_laplace_cdf_windows', _p(sigma), npix, c, C.byref(ml),
                               win.data_ptr() + 2 * row_off * abi.CDF_WIN, sp.data_ptr() + 4 * row_off, _stream()))
    return out


def frame_maps_to_device(maps_list, npix, device):
    """device image of the aivc_frame_maps table of a frame batch (pinned staging, asynchronous copy)
    -> (uint8 CUDA tensor [n, 272], [pos_off per frame], total coded positions)"""
    tab, offs, total = abi.frame_maps_table(maps_list, npix)
    # a frame's 272 bytes are a multiple of 16, so the blob is the table; of no frames it is _stage's least blob, 16 zero bytes
    return _stage(device, [tab.reshape(-1)])[0], offs, total


def laplace_cdf_windows_batch(sigma, maps_list, out, table=None):
    """the windows + sigma of every coded position of a frame batch in ONE launch: sigma [n,h,w,c], maps_list[f] the coded
    channels of frame f, out = (win [>= total, CDF_WIN] int16, sigma_pos [>= total]) -> ([pos_off per frame], table)"""
    sigma = _dev(sigma, torch.float32, 'sigma')
    n, npix, c = _rows_dims(sigma)
    table = table or frame_maps_to_device(maps_list, npix, sigma.device)
    dev, offs, total = table
    for m in maps_list:
        _check_maps(m, c)
    win, sp = out
    _out(win, torch.int16, (total, abi.CDF_WIN), 'out[0]', sigma.device, at_least=True)
    _out(sp, torch.float32, (total,), 'out[1]', sigma.device, at_least=True)
    mx = max((len(m) for m in maps_list), default=0)
    if total:
        _hbm_profiled('cdf_points:laplace_cdf_windows', total * abi.CDF_WIN,
                      lambda: call('aivc_laplace_cdf_windows_batch', _p(sigma), n, npix, c, _p(dev), mx, _p(win), _p(sp), _stream()))
    return offs, table


def laplace_bounds_batch(sigma, q, maps_list):
    """-> (bounds int32 [total], [pos_off per frame]) of a frame batch in one launch"""
    sigma = _dev(sigma, torch.float32, 'sigma')
    q = _shaped(q, torch.int16, sigma.shape, 'q')
    n, npix, c = _rows_dims(sigma)
    for m in maps_list:
        _check_maps(m, c)
    dev, offs, total = frame_maps_to_device(maps_list, npix, sigma.device)
    bounds = torch.empty(max(total, 1), dtype=torch.int32, device=sigma.device)
    mx = max((len(m) for m in maps_list), default=0)
    if total:
        call('aivc_laplace_bounds_batch', _p(sigma), _p(q), n, npix, c, _p(dev), mx, _p(bounds), _stream())
    return bounds, offs


def table_bounds_batch(table, q):
    """q [n,h,w,c] -> bounds int32 [n, c * npix] (every channel of every frame, pmf mode) in one launch"""
    q = _dev(q, torch.int16, 'q')
    n, npix, c = _rows_dims(q)
    table = _shaped(table, torch.int16, (c, abi.CDF_ROW), 'table')
    bounds = torch.empty((n, c * npix), dtype=torch.int32, device=q.device)
    call('aivc_table_bounds_batch', _p(table), _p(q), n, npix, c, _p(bounds), _stream())
    return bounds


def _symbols(sym, total):
    """decoded symbols in stream order: an int16 CUDA vector of at least `total` of them"""
    sym = _shaped(sym, torch.int16, (None,), 'sym')
    if sym.shape[0] < total:
        raise ValueError('aivc_amd.ops: %d symbols, the maps hold %d' % (sym.shape[0], total))
    return sym


def scatter_symbols_batch(sym, maps_list, n, npix, c, table=None):
    """sym: the decoded symbols of the batch in stream order (frame f's at its pos_off) -> q int16 [n, npix, c]"""
    sym = _symbols(sym, sum(len(m) for m in maps_list) * npix)
    for m in maps_list:
        _check_maps(m, c)
    if len(maps_list) != n:
        raise ValueError('scatter_symbols_batch: %d map lists for %d frames' % (len(maps_list), n))
    dev_ = sym.device
    table = table or frame_maps_to_device(maps_list, npix, dev_)
    q = torch.empty((n, npix, c), dtype=torch.int16, device=dev_)
    call('aivc_scatter_symbols_batch', _p(sym), n, npix, c, _p(table[0]), _p(q), _stream())
    return q


def laplace_bounds(sigma, q, maps):
    """sigma / q [1,h,w,c] (one image) -> bounds int32 [len(maps) * npix]: aivc_laplace_bounds, the one-frame case of the
    batch kernel with the map list passed by value.  Nothing under aivc_amd/ calls it (the codec goes through
    laplace_bounds_batch); the tests, the oracle comparisons and tools/bench_rangecoder.py do."""
    sigma, npix, c, ml = _one_image(sigma, maps)
    q = _shaped(q, torch.int16, sigma.shape, 'q')
    bounds = torch.empty(len(maps) * npix, dtype=torch.int32, device=sigma.device)
    call('aivc_laplace_bounds', _p(sigma), _p(q), npix, c, C.byref(ml), _p(bounds), _stream())
    return bounds


def table_bounds(table, q):
    """q [1,h,w,c] (one image) -> bounds int32 [c * npix]: aivc_table_bounds = aivc_table_bounds_batch with n = 1.
    Nothing under aivc_amd/ calls it (the codec goes through table_bounds_batch); the tests, the oracle comparisons and
    tools/bench_rangecoder.py do."""
    q = _shaped(q, torch.int16, (1, None, None, None), 'q')
    c = q.shape[-1]
    npix = q.numel() // c if c else 0
    table = _shaped(table, torch.int16, (c, abi.CDF_ROW), 'table')
    bounds = torch.empty(c * npix, dtype=torch.int32, device=q.device)
    call('aivc_table_bounds', _p(table), _p(q), npix, c, _p(bounds), _stream())
    return bounds


# ---- rate estimation (logging only; csrc/rate.hip) ---------------------------------------------------------
def _rate_scratch(device, out=None):
    lanes = torch.empty(abi.RATE_LANES, dtype=torch.float64, device=device)
    return lanes, (torch.empty(1, dtype=torch.float64, device=device) if out is None else out)


def bounds_rate(bounds, out=None):
    """packed CDF bounds (laplace_bounds / table_bounds) -> device fp64 [1]: the bits the range coder pays for them
    (sum of -log2((c_hi - c_lo) / 2^16), fixed summation order).  No sync.  out: a 1-element fp64 view to fill."""
    bounds = _dev(bounds, torch.int32, 'bounds')
    if out is not None:
        _out(out, torch.float64, (1,), 'out', bounds.device)
    lanes, out = _rate_scratch(bounds.device, out)
    call('aivc_bounds_rate', _p(bounds), bounds.numel(), _p(lanes), _p(out), _stream())
    return out


def rate_bits(prob, p_min, p_max):
    """EntropyCoder.forward (src/layers/entropy_coding/entropy_coder.py:25-30): -log2(clamp(prob)) -> (rate like prob,
    device fp64 [1] sum)"""
    prob = _dev(prob, torch.float32, 'prob')
    rate = torch.empty_like(prob)
    lanes, out = _rate_scratch(prob.device)
    call('aivc_rate_bits', _p(prob), prob.numel(), float(p_min), float(p_max), _p(rate), _p(lanes), _p(out), _stream())
    return rate, out


def laplace_prob(y, mu, sigma):
    """P(bin of y) under Laplace(mu, sigma / sqrt(2)) elementwise (mu None = 0), ParametricPdf.forward"""
    y = _dev(y, torch.float32, 'y')
    sigma = _dev(sigma, torch.float32, 'sigma')
    mu = _dev(mu, torch.float32, 'mu')
    if sigma.shape != y.shape or (mu is not None and mu.shape != y.shape):
        raise AivcNativeError('aivc_amd.ops.laplace_prob: y, mu and sigma must have one shape')
    prob = torch.empty_like(y)
    call('aivc_laplace_prob', _p(y), _p(mu), _p(sigma), y.numel(), _p(prob), _stream())
    return prob


def table_prob(x, cdf_f32):
    """x [b, c, h, w] integer-valued in [-256, 256], cdf_f32 [c, 514] (balle_cdf_table(want_float=True)) -> P(bin of x)"""
    x = _dev(x, torch.float32, 'x')
    cdf_f32 = _dev(cdf_f32, torch.float32, 'cdf_f32')
    b, c, h, w = x.shape
    if tuple(cdf_f32.shape) != (c, abi.LP):
        raise AivcNativeError('aivc_amd.ops.table_prob: cdf table %s for %d channels' % (tuple(cdf_f32.shape), c))
    prob = torch.empty_like(x)
    call('aivc_table_prob', _p(x), _p(cdf_f32), x.numel(), h * w, c, _p(prob), _stream())
    return prob


def _rc_batches(n, fill):
    """n range-coder streams, abi.RC_MAX_STREAMS to a launch -> (index of its first stream, aivc_rc_batch) per launch;
    fill(s, i) sets the aivc_rc_stream s of stream i"""
    for start in range(0, n, abi.RC_MAX_STREAMS):
        batch = abi.RcBatch()
        batch.n_streams = min(n - start, abi.RC_MAX_STREAMS)
        for k in range(batch.n_streams):
            fill(batch.s[k], start + k)
        yield start, batch


def range_encode(bounds_list, streams=None):
    """bounds_list: int32 CUDA tensors, one independent stream each (any number; launched 64 at a
    time: one workgroup per launch, one stream per lane).  Returns (out uint8 tensor, lens int32 tensor [n], [(offset,
    capacity)]) -- all on device, no sync.
    streams: optional HIP streams; the launches (a kernel lasts as long as its longest stream) then
    run concurrently on them, forked from / joined back into the current stream with events."""
    n = len(bounds_list)
    for i, b in enumerate(bounds_list):  # (looked at as they are: a view into a packed tensor stays that view)
        if not b.is_cuda or b.dtype != torch.int32 or b.dim() != 1 or b.device != bounds_list[0].device:
            raise AivcNativeError('aivc_amd.ops: bounds_list[%d] is %s %s on %s; a stream is an int32 CUDA vector'
                                  % (i, b.dtype, tuple(b.shape), b.device))
    bounds_list = [b if b.is_contiguous() else b.contiguous() for b in bounds_list]
    dev = bounds_list[0].device
    # views that already sit back to back in one tensor (the batched bounds kernels) need no concatenation
    base = bounds_list[0]._base if bounds_list[0]._base is not None else bounds_list[0]
    pos, packed = bounds_list[0].storage_offset(), True
    for b in bounds_list:
        packed = packed and (b._base if b._base is not None else b) is base and b.storage_offset() == pos and b.is_contiguous()
        pos += b.numel()
    if packed:
        allb = base.reshape(-1)[bounds_list[0].storage_offset():pos]
    else:
        allb = bounds_list[0] if n == 1 else torch.cat(bounds_list)
    in_offs, out_offs, in_off, out_off = [], [], 0, 0
    for b in bounds_list:
        cap = (16 + 3 * b.numel() + 3) // 4 * 4
        in_offs.append(in_off)
        out_offs.append((out_off, cap))
        in_off += b.numel()
        out_off += cap
    out = torch.empty(out_off, dtype=torch.uint8, device=dev)
    lens = torch.empty(n, dtype=torch.int32, device=dev)
    fork = streams is not None and len(streams) > 0 and n > abi.RC_MAX_STREAMS
    cur, ev0 = None, None
    if fork:
        cur = torch.cuda.current_stream()
        ev0 = torch.cuda.Event()
        ev0.record(cur)
        for t in (allb, out, lens):
            for st in streams:
                t.record_stream(st)

    def fill(s_, i):
        s_.in_off, s_.out_off, s_.n_sym, s_.out_cap = in_offs[i], out_offs[i][0], bounds_list[i].numel(), out_offs[i][1]
    for gi, (start, batch) in enumerate(_rc_batches(n, fill)):
        if fork:
            st = streams[gi % len(streams)]
            st.wait_event(ev0)
            call('aivc_range_encode', _p(allb), C.byref(batch), _p(out), lens.data_ptr() + 4 * start, st.cuda_stream)
            ev = torch.cuda.Event()
            ev.record(st)
            cur.wait_event(ev)
        else:
            call('aivc_range_encode', _p(allb), C.byref(batch), _p(out), lens.data_ptr() + 4 * start, _stream())
    return out, lens, out_offs


def range_decode(payloads, rows, row_offs, n_syms, planes, sigma_pos=None, want_bits=False, flat=False):
    """Decode len(payloads) independent streams concurrently (one wavefront each, <= 64 per launch).
    rows: ONE int16 CUDA tensor [n_rows, CDF_ROW] holding every stream's CDF rows; stream i starts at
    row row_offs[i] and uses one row per symbol (planes[i] == 0) or row i // planes[i] (pmf tables).
    With sigma_pos (float32 [n_rows]) `rows` holds the 64-entry windows of laplace_cdf_windows instead
    ([n_rows, CDF_WIN]; planes must be 0).
    Returns a list of int16 CUDA tensors (uint16 payload: symbols 0..512); with want_bits also an int32 CUDA tensor [n]
    of the bits each stream consumed (include/aivc_hip.h: len(payload) == (bits + 2 + 7) // 8 for an intact stream)."""
    n = len(payloads)
    if not len(row_offs) == len(n_syms) == len(planes) == n:
        raise ValueError('range_decode: %d payloads, %d row offsets, %d symbol counts, %d planes' % (n, len(row_offs), len(n_syms), len(planes)))
    rows = _shaped(rows, torch.int16, (None, abi.CDF_ROW if sigma_pos is None else abi.CDF_WIN), 'rows')
    sigma_pos = _shaped(sigma_pos, torch.float32, (rows.shape[0],), 'sigma_pos')
    for i in range(n):  # the rows stream i reads: one per symbol, or one per `plane` symbols
        used = n_syms[i] if planes[i] == 0 else -(-n_syms[i] // planes[i])
        if row_offs[i] < 0 or n_syms[i] < 0 or planes[i] < 0 or row_offs[i] + used > rows.shape[0] or (planes[i] and sigma_pos is not None):
            raise ValueError('range_decode: stream %d reads rows %d .. %d of %d (plane %d)'
                             % (i, row_offs[i], row_offs[i] + used - 1, rows.shape[0], planes[i]))
    dev = rows.device
    # the decoder kernels read past a payload's end by design: every payload is padded to 4 bytes and followed by 8 spare ones,
    # zeros everywhere outside the payloads, at least 4 bytes in all
    dbytes, offs = _stage(dev, [np.frombuffer(pl, np.uint8) for pl in payloads], align=4, slack=8)
    sym_offs = [0]
    for k in n_syms:
        sym_offs.append(sym_offs[-1] + k)
    sym = torch.empty(max(sym_offs[-1], 1), dtype=torch.int16, device=dev)
    outs = [sym[sym_offs[i]:sym_offs[i + 1]] for i in range(n)]
    bits = torch.empty(n, dtype=torch.int32, device=dev) if want_bits else None

    def fill(s_, i):
        s_.in_off, s_.out_off, s_.row_off = offs[i], sym_offs[i], row_offs[i]
        s_.n_sym, s_.in_len, s_.plane = n_syms[i], len(payloads[i]), planes[i]
    for start, batch in _rc_batches(n, fill):
        bp = None if bits is None else bits.data_ptr() + 4 * start
        if sigma_pos is None:
            call('aivc_range_decode', _p(dbytes), _p(rows), C.byref(batch), _p(sym), bp, _stream())
        else:
            call('aivc_range_decode_windows', _p(dbytes), _p(rows), _p(sigma_pos), C.byref(batch), _p(sym), bp, _stream())
    if flat:  # the one tensor the streams' symbols sit in, back to back in stream order
        outs = sym
    return (outs, bits) if want_bits else outs


def scatter_symbols(sym, npix, c, maps):
    _check_maps(maps, c)
    ml = abi.MapList.make(maps)
    sym = None if sym is None else _symbols(sym, len(maps) * npix)
    dev = sym.device if sym is not None else torch.device('cuda')
    q = torch.empty((npix, c), dtype=torch.int16, device=dev)
    call('aivc_scatter_symbols', _p(sym), npix, c, C.byref(ml), _p(q), _stream())
    return q


# ---- quality metrics (fp64 planes [n, h, w]) ------------------------------------------------------
def _metrics_ws(n, h, w, dev):
    nbytes = load()['aivc_metrics_workspace'](int(n), int(h), int(w))
    return torch.empty(nbytes // 8, dtype=torch.float64, device=dev)


def ssim_means(a, b, win, c1, c2):
    """a, b: float64 CUDA planes [n,h,w]; win: 1-D normalised window (host sequence, len <= 11).
    -> float64 CUDA tensor [n, 2]: (mean SSIM, mean contrast-structure) of one scale."""
    a = _shaped(a, torch.float64, (None,) * 3, 'a')
    b = _shaped(b, torch.float64, a.shape, 'b')
    n, h, w = a.shape
    wn = np.ascontiguousarray(np.asarray(win, np.float64))
    out = torch.empty((n, 2), dtype=torch.float64, device=a.device)
    ws = _metrics_ws(n, h, w, a.device)
    call('aivc_ssim_means', _p(a), _p(b), n, h, w, wn.ctypes.data, len(wn), float(c1), float(c2), _p(ws), _p(out), _stream())
    return out


def pool2x2(x, edge):
    """float64 planes [n,h,w] -> [n, ceil(h/2), ceil(w/2)] 2x2 means; edge 0: mirror past the end without
    repeating the border (torch ReflectionPad2d), 1: repeat it (scipy 'reflect')."""
    x = _shaped(x, torch.float64, (None,) * 3, 'x')
    n, h, w = x.shape
    out = torch.empty((n, (h + 1) // 2, (w + 1) // 2), dtype=torch.float64, device=x.device)
    call('aivc_pool2x2', _p(x), n, h, w, int(edge), _p(out), _stream())
    return out


def sq_err(a, b):
    """-> float64 CUDA tensor [1]: sum of squared differences of two float64 tensors of equal size"""
    a = _dev(a, torch.float64, 'a')
    b = _shaped(b, torch.float64, a.shape, 'b')
    out = torch.empty(1, dtype=torch.float64, device=a.device)
    ws = _metrics_ws(1, 16, 16, a.device)
    call('aivc_sq_err', _p(a), _p(b), a.numel(), _p(ws), _p(out), _stream())
    return out


# ---- per-frame statistics of the encoder's quality log (include/aivc_hip_quality.h) -------------------------------------
def frame_sse_u8(src, rec):
    """src, rec: dicts of the uint8 planes of n frames stacked per plane, 'y' [n,h,w], 'u' and 'v' [n,ceil(h/2),ceil(w/2)]
    -> int64 CUDA tensor [n, 3]: the exact sum of (src - rec)^2 per frame and plane (y, u, v).  No sync."""
    a = [_dev(src[k], torch.uint8, 'src ' + k) for k in 'yuv']
    b = [_dev(rec[k], torch.uint8, 'rec ' + k) for k in 'yuv']
    if a[0].dim() != 3:
        raise ValueError('frame_sse_u8: expected planes [n, h, w], got %s' % (tuple(a[0].shape),))
    n, h, w = a[0].shape
    shapes = [(n, h, w)] + [(n, (h + 1) // 2, (w + 1) // 2)] * 2
    if [tuple(t.shape) for t in a] != shapes or [tuple(t.shape) for t in b] != shapes:
        raise ValueError('frame_sse_u8: planes %s against %s: expected %s'
                         % ([tuple(t.shape) for t in a], [tuple(t.shape) for t in b], shapes))
    partials = torch.empty((n, 3, abi.SSE_BLOCKS), dtype=torch.int64, device=a[0].device)
    sse = torch.empty((n, 3), dtype=torch.int64, device=a[0].device)
    _hbm_profiled('frame_sse_u8', 2 * n * (h * w + 2 * shapes[1][1] * shapes[1][2]),
                  lambda: call('aivc_frame_sse_u8', _p(a[0]), _p(a[1]), _p(a[2]), _p(b[0]), _p(b[1]), _p(b[2]), n, h, w,
                               _p(partials), _p(sse), _stream()))
    return sse


def _nhwc_store(t, c, name):
    """t: fp32 [n,h,w,c'] holding its channels innermost with any pixel pitch (a contiguous tensor, or the leading channels of
    one: x[..., :3]) -> (tensor whose data_ptr is pixel 0, stored channels per pixel)"""
    if t.dim() != 4 or t.shape[-1] < c:
        raise ValueError('%s: expected [n, h, w, >= %d channels], got %s' % (name, c, tuple(t.shape)))
    n, h, w, _ = t.shape
    cs = t.stride(2)
    if t.stride(3) != 1 or cs < t.shape[-1] or t.stride(1) != w * cs or t.stride(0) != h * w * cs:
        t = t.contiguous()
        cs = t.shape[-1]
    return t, cs


def frame_aux_stats(alpha, beta, warping, code, c=3):
    """The auxiliary outputs of a batch of n frames (FrameCodec.encode_batch(want_aux=True)): alpha, beta fp32 [n,h,w],
    warping and code fp32 NHWC with the first c channels used (a channel slice of a wider tensor is read in place).
    alpha / beta / warping None: an I frame's (maps of ones, ones, zeros).
    -> float64 CUDA tensor [n, 3]: sum alpha, sum beta, sum (warping - code)^2 per frame, fixed summation order.  No sync."""
    code = _dev_strided(code, 'code')
    code, cs_code = _nhwc_store(code, c, 'code')
    n, h, w, _ = code.shape
    cs_warp = 0
    if warping is not None:
        warping, cs_warp = _nhwc_store(_dev_strided(warping, 'warping'), c, 'warping')
        if tuple(warping.shape[:3]) != (n, h, w):
            raise ValueError('frame_aux_stats: warping %s does not go with code %s' % (tuple(warping.shape), tuple(code.shape)))
    alpha, beta = _dev(alpha, torch.float32, 'alpha'), _dev(beta, torch.float32, 'beta')
    for t, nm in ((alpha, 'alpha'), (beta, 'beta')):
        if t is not None and tuple(t.shape) != (n, h, w):
            raise ValueError('frame_aux_stats: %s %s does not go with code %s' % (nm, tuple(t.shape), tuple(code.shape)))
    lanes = torch.empty((n, 3, abi.RATE_LANES), dtype=torch.float64, device=code.device)
    out = torch.empty((n, 3), dtype=torch.float64, device=code.device)
    n_maps = (alpha is not None) + (beta is not None)
    _hbm_profiled('frame_aux_stats', n * h * w * 4 * (n_maps + c * (2 if warping is not None else 1)),
                  lambda: call('aivc_frame_aux_stats', _p(alpha), _p(beta), _p(warping), _p(code), n, h, w, int(c), int(cs_warp),
                               int(cs_code), _p(lanes), _p(out), _stream()))
    return out


def _dev_strided(t, name):
    """_dev without the copy of a non-contiguous tensor (the caller looks at the strides itself)"""
    if not t.is_cuda:
        raise AivcNativeError('aivc_amd.ops: %s is on %s; the HIP path needs CUDA tensors (no CPU fallback)' % (name, t.device))
    if t.dtype != torch.float32:
        raise AivcNativeError('aivc_amd.ops: %s has dtype %s, expected %s' % (name, t.dtype, torch.float32))
    return t
