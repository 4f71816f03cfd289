/*
 * aivc_hip_color.h -- 8-bit RGB <-> YCbCr for the PNG frame I/O (part of the C ABI of libaivc_hip.so since ABI 19;
 * conventions, types and error codes: aivc_hip.h).
 *
 * Replaces: src/func_util/img_processing.py:179-196 (load_RGB_as_YUV420_dic: Image.convert('YCbCr') and the nearest x 0.5 of
 * the chroma) and :221-287 (save_tensor_as_img: nearest x 2 of the chroma, the crop, to_pil_image(..., 'YCbCr').convert('RGB')).
 *
 * The arithmetic is Pillow's 8-bit JFIF conversion, bit for bit: integer tables with 6 fractional bits
 * (aivc_amd/csrc/color_tables.h, recovered from Pillow by tools/gen_color_tables.py), integer adds, arithmetic shifts and
 * clamps -- no floating point.  With T the tables and x >> 6 an arithmetic shift (a floor):
 *
 *   Y  = (Y_R[r] + Y_G[g] + Y_B[b]) >> 6
 *   Cb = ((CB_R[r] + CB_G[g] + 32 b) >> 6) + 128
 *   Cr = ((32 r + CR_G[g] + CR_B[b]) >> 6) + 128
 *   R  = clamp(y + (R_CR[cr] >> 6), 0, 255)
 *   G  = clamp(y + ((G_CB[cb] + G_CR[cr]) >> 6), 0, 255)
 *   B  = clamp(y + (B_CB[cb] >> 6), 0, 255)
 *
 * These entry points have no `_ref` twin in the CPU oracle; tests/test_color_tables.py pins the tables against Pillow on
 * all 2^24 triples in both directions on the CPU, tests/test_gpu_color.py pins the kernels against Pillow.
 */
#ifndef AIVC_HIP_COLOR_H
#define AIVC_HIP_COLOR_H

#include "aivc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rgb [n][h][w][3] uint8 -> planar uint8 y [n][h][w], u and v [n][h / 2][w / 2] (FLOOR sizes, the reference's
 * interpolate(scale_factor=0.5, mode='nearest'): chroma sample (i, j) is the Cb / Cr of pixel (2i, 2j) alone; an odd last row
 * or column has luma only).  Note that the planar .yuv path (aivc_frame_to_yuv420, aivc_yuv420u8_to_444) stores CEIL-sized
 * chroma planes; the two agree for even h and w.  u and v may be NULL when h / 2 * (w / 2) == 0.
 * One thread owns a 2 x 16 block (w % 16 == 0 and 16-byte aligned rgb / y, 8-byte aligned u / v: 16-byte loads and stores)
 * or a 2 x 2 block (anything else). */
int aivc_rgb8_to_yuv420u8(const uint8_t *rgb, int32_t n, int32_t h, int32_t w, uint8_t *y, uint8_t *u, uint8_t *v,
                          aivc_stream_t stream);

/* planar uint8 y [n][h][w], u and v [n][ch][cw] -> rgb [n][h][w][3] uint8.
 *   chroma_shift == 0: full-resolution chroma (yuv444 / yuv444_nodic); ch == h and cw == w.
 *   chroma_shift == 1: half-resolution chroma, nearest x 2 and cropped to the luma size: pixel (i, j) reads chroma sample
 *                      (min(i / 2, ch - 1), min(j / 2, cw - 1)).  ch >= max(h / 2, 1) and cw >= max(w / 2, 1): planes of the
 *                      floor size (aivc_rgb8_to_yuv420u8) and of the ceil size (the planar .yuv path) both work.  With
 *                      floor-sized planes an odd last row / column repeats the last chroma sample (the reference cannot
 *                      save such a frame at all: its upsampled planes are one short of the luma).
 * AIVC_ERR_ARG for any other chroma_shift or plane size (a chroma plane of size zero included). */
int aivc_yuv8_to_rgb8(const uint8_t *y, const uint8_t *u, const uint8_t *v, int32_t n, int32_t h, int32_t w, int32_t ch,
                      int32_t cw, int32_t chroma_shift, uint8_t *rgb, aivc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AIVC_HIP_COLOR_H */
