/*
 * aivc_hip_color_matrix.h -- 8-bit RGB <-> YCbCr by matrix and range: BT.601 / BT.709 / BT.2020, full or limited range (entry
 * points added to the C ABI of libaivc_hip.so beside aivc_hip_color.h; conventions, types and error codes: aivc_hip.h).
 *
 * aivc_hip_color.h is Pillow's JFIF arithmetic (BT.601, full range, floored), the reference's and the default.  These two entry
 * points are the conversion a caller ASKS for by naming what the planes carry.  The arithmetic is stated once, in
 * aivc_amd/color.py (coefficients, forward_numpy, inverse_numpy); this header repeats it.  Integer only, S = 14 fractional
 * bits, x >> k an arithmetic shift (a floor), every result clamped to 0 ... 255:
 *
 *   forward   out_i = clamp((fwd[i][0] r + fwd[i][1] g + fwd[i][2] b + (fwd_off[i] << S) + (1 << (S - 1))) >> S)   i = Y, Cb, Cr
 *   box       Cb, Cr of a 4:2:0 sample from the exact sums R, G, B of its 2 x 2 block, rounded once:
 *             out_i = clamp((fwd[i][0] R + fwd[i][1] G + fwd[i][2] B + (fwd_off[i] << (S + 2)) + (1 << (S + 1))) >> (S + 2))
 *   inverse   with inv = (cy, rv, gu, gv, bu), y' = cy (Y - inv_yoff) + (1 << (S - 1)), cb = Cb - 128, cr = Cr - 128:
 *             R = clamp((y' + rv cr) >> S)   G = clamp((y' + gu cb + gv cr) >> S)   B = clamp((y' + bu cb) >> S)
 *
 * The integers of a matrix and range (aivc_amd/color.py: coefficients): with Kr, Kb the standard's luma weights, Kg = 1 - Kr -
 * Kb, (ys, cs, yo) = (1, 1, 0) for full and (219 / 255, 224 / 255, 16) for limited range,
 *   fwd = round(2^S x) of the rows ys (Kr, Kg, Kb), cs (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb)), cs (1 - Kr, -Kg, -Kb) / (2 (1 - Kr)),
 *         half to even, the G entry then corrected so that the Y row sums to round(2^S ys) and the chroma rows to 0 (a grey
 *         pixel has Cb = Cr = 128 exactly);  fwd_off = (yo, 128, 128);
 *   inv = round(2^S x) of 1 / ys, 2 (1 - Kr) / cs, -Kb 2 (1 - Kb) / (Kg cs), -Kr 2 (1 - Kr) / (Kg cs), 2 (1 - Kb) / cs;  inv_yoff = yo.
 * Every output before the clamp is within 0.5 + 0.04 of the real-valued formula (tests/test_colour_matrix.py, all 2^24 triples).
 *
 * No `_ref` twin in the CPU oracle: the statement is numpy (aivc_amd/color.py), tests/test_gpu_colour_matrix.py pins the
 * kernels against it byte for byte.
 */
#ifndef AIVC_HIP_COLOR_MATRIX_H
#define AIVC_HIP_COLOR_MATRIX_H

#include "aivc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AIVC_COLOR_MATRIX_SHIFT 14      /* S */
#define AIVC_COLOR_MATRIX_MAX_COEF 65536 /* largest magnitude of an entry of fwd / inv: every int32 sum of the kernels then
                                            stays below 2^31 (the box sum: 3 x 65536 x 1020) */

/* A HOST pointer; read before the call returns.  fwd rows Y, Cb, Cr over columns R, G, B. */
typedef struct aivc_color_matrix {
  int32_t fwd[3][3];
  int32_t fwd_off[3];
  int32_t inv[5]; /* cy, rv, gu, gv, bu */
  int32_t inv_yoff;
} aivc_color_matrix;

/* rgb [n][h][w][3] uint8 -> planar uint8 y [n][h][w], u and v [n][h / 2][w / 2]: the shapes, the FLOOR-sized chroma planes and
 * the NULL u / v of a frame without a chroma sample are those of aivc_rgb8_to_yuv420u8.
 *   chroma_down == 0 (point): chroma sample (i, j) is the Cb / Cr of pixel (2i, 2j) alone.
 *   chroma_down == 1 (box):   ... of the sum of the pixels (2i, 2j) ... (2i + 1, 2j + 1), rounded once.  Floor-sized planes hold
 *                             whole blocks only: there is no edge rule.
 * One thread owns a 2 x 16 block (w % 16 == 0 and 16-byte aligned rgb / y, 8-byte aligned u / v: 16-byte loads and stores) or a
 * 2 x 2 block (anything else); every output byte is written exactly once.
 * AIVC_ERR_ARG as aivc_rgb8_to_yuv420u8, and for m == NULL, any other chroma_down, an entry of fwd / inv whose magnitude is
 * above AIVC_COLOR_MATRIX_MAX_COEF, an entry of fwd_off or inv_yoff outside 0 ... 255. */
int aivc_rgb8_to_yuv420u8_matrix(const uint8_t *rgb, int32_t n, int32_t h, int32_t w, const aivc_color_matrix *m,
                                 int32_t chroma_down, uint8_t *y, uint8_t *u, uint8_t *v, aivc_stream_t stream);

/* planar uint8 y [n][h][w], u and v [n][ch][cw] -> rgb [n][h][w][3] uint8.  chroma_shift, the plane sizes it takes and the
 * chroma geometry (nearest x 2, cropped, indices clamped to the plane) are exactly those of aivc_yuv8_to_rgb8.  Inputs outside
 * the nominal range (Y < 16 under limited range) go through the same formula.
 * AIVC_ERR_ARG as aivc_yuv8_to_rgb8, and for m as above. */
int aivc_yuv8_to_rgb8_matrix(const uint8_t *y, const uint8_t *u, const uint8_t *v, int32_t n, int32_t h, int32_t w, int32_t ch,
                             int32_t cw, int32_t chroma_shift, const aivc_color_matrix *m, uint8_t *rgb, aivc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AIVC_HIP_COLOR_MATRIX_H */
