"""warp() with the reference's signature (src/func_util/optical_flow.py:14-55) on the HIP kernels: every interpol_mode,
padding_mode and align_corners that grid_sample accepts (include/aivc_hip_warp.h)."""
from .. import ops


def warp(x, flo, interpol_mode='bilinear', padding_mode='border', align_corners=True):
    """x [B,C,H,W], flo [B,2,H,W] (pixel units, channel 0 horizontal) -> warped [B,C,H,W]."""
    if interpol_mode not in ops.WARP_INTERP:
        raise ValueError("warp: interpol_mode %r: expected 'bilinear', 'nearest' or 'bicubic'" % (interpol_mode,))
    if padding_mode not in ops.WARP_PAD:
        raise ValueError("warp: padding_mode %r: expected 'border', 'zeros' or 'reflection'" % (padding_mode,))
    return ops.to_nchw_view(ops.warp(ops.to_nhwc(x), ops.to_nhwc(flo), interpol_mode, padding_mode, bool(align_corners)))
