"""Recovers Pillow's 8-bit JFIF colour tables (Image.convert between 'RGB' and 'YCbCr') from Pillow's behaviour on the CPU
and prints aivc_amd/csrc/color_tables.h.

    python tools/gen_color_tables.py > aivc_amd/csrc/color_tables.h

The model (6 fractional bits, arithmetic shifts; x >> 6 floors):

    Y  = (Y_R[r] + Y_G[g] + Y_B[b]) >> 6
    Cb = ((CB_R[r] + CB_G[g] + HALF[b]) >> 6) + 128
    Cr = ((HALF[r] + CR_G[g] + CR_B[b]) >> 6) + 128          HALF[i] = 32 i
    R  = clamp(y + (R_CR[cr] >> 6))
    G  = clamp(y + ((G_CB[cb] + G_CR[cr]) >> 6))
    B  = clamp(y + (B_CB[cb] >> 6))

Pillow's chroma and inverse tables are not the plainly rounded products, so they are read off its outputs:

  * luma: floor(c * 64 * i + 0.5), which is exact;
  * a channel that reads ONE table (R from Cr, B from Cb) shows only T >> 6: the table is 64 * that, observed at a luma that
    keeps the result off the clamp;
  * a channel that sums TWO unknown tables (Cb, Cr, G) shows, for every pair (i, j), a window [lo, hi] for A[i] + B[j]: 32 wide
    for the forward channels (the third term moves in steps of 32), 64 wide for G.  The 2 x 256 entries are then a solution
    of that system of difference constraints, found by relaxation (Bellman-Ford on the complete bipartite graph) started
    from the truncated products, so that the entries stay next to them.  Any solution reproduces every observation.

Before anything is printed the tables are checked against Pillow on all 2^24 triples in both directions
(tests/test_color_tables.py repeats that check on the committed header)."""
import sys

import numpy as np
from PIL import Image
import PIL

I = np.arange(256, dtype=np.int64)


def pil_forward(rgb):
    return np.asarray(Image.fromarray(np.ascontiguousarray(rgb), 'RGB').convert('YCbCr'))


def pil_inverse(ycc):
    return np.asarray(Image.fromarray(np.ascontiguousarray(ycc), 'YCbCr').convert('RGB'))


def pair_image(pos_a, pos_b, pos_c, c):
    """[256, 256, 3]: channel pos_a = row index, pos_b = column index, pos_c = the constant c"""
    img = np.empty((256, 256, 3), np.uint8)
    img[..., pos_a] = I[:, None]
    img[..., pos_b] = I[None, :]
    img[..., pos_c] = c
    return img


def solve_pairs(lo, hi, a0, b0):
    """int tables a, b with lo[i, j] <= a[i] + b[j] <= hi[i, j]; started from a0, b0 (relaxation only lowers a and raises b)"""
    a, nb = a0.astype(np.int64).copy(), -b0.astype(np.int64)  # variables a[i] and nb[j] = -b[j]: lo <= a - nb <= hi
    for _ in range(4 * 512):
        a2 = np.minimum(a, (nb[None, :] + hi).min(axis=1))
        nb2 = np.minimum(nb, (a2[:, None] - lo).min(axis=0))
        if np.array_equal(a2, a) and np.array_equal(nb2, nb):
            s = a[:, None] - nb[None, :]
            assert ((s >= lo) & (s <= hi)).all()
            return a, -nb
        a, nb = a2, nb2
    raise RuntimeError('the observed windows admit no pair of tables: the model is wrong')


def forward_pair(pos_a, pos_b, pos_half, ch, ca, cb):
    q0 = pil_forward(pair_image(pos_a, pos_b, pos_half, 0))[..., ch].astype(np.int64) - 128  # floor(S / 64)
    q1 = pil_forward(pair_image(pos_a, pos_b, pos_half, 1))[..., ch].astype(np.int64) - 128  # floor((S + 32) / 64)
    lo = 64 * q0 + 32 * (q1 - q0)
    return solve_pairs(lo, lo + 31, np.trunc(ca * 64 * I), np.trunc(cb * 64 * I))


def off_clamp(observe):
    """observe(y) -> channel value [..]; y + table term, taken at a luma where the result is not clamped"""
    out = None
    for y in (0, 64, 128, 192, 255):
        v = observe(y).astype(np.int64)
        ok = (v > 0) & (v < 255)
        out = np.where(ok, v - y, 1 << 20) if out is None else np.where(ok & (out == 1 << 20), v - y, out)
    assert (out != 1 << 20).all()
    return out


def recover():
    t = {}
    for name, c in (('Y_R', 0.299), ('Y_G', 0.587), ('Y_B', 0.114)):
        t[name] = np.floor(c * 64 * I + 0.5).astype(np.int64)
    t['HALF'] = 32 * I
    t['CB_R'], t['CB_G'] = forward_pair(0, 1, 2, 1, -0.168736, -0.331264)
    t['CR_G'], t['CR_B'] = forward_pair(1, 2, 0, 2, -0.418688, -0.081312)

    def line(pos, ch):
        def observe(y):
            img = np.full((1, 256, 3), 128, np.uint8)
            img[..., 0] = y
            img[0, :, pos] = I
            return pil_inverse(img)[0, :, ch]
        return observe
    t['R_CR'] = 64 * off_clamp(line(2, 0))
    t['B_CB'] = 64 * off_clamp(line(1, 2))
    q = off_clamp(lambda y: pil_inverse(pair_image(1, 2, 0, y))[..., 1])
    t['G_CB'], t['G_CR'] = solve_pairs(64 * q, 64 * q + 63, np.trunc(-0.344136 * 64 * (I - 128)), np.trunc(-0.714136 * 64 * (I - 128)))
    return t


FORWARD = ('Y_R', 'Y_G', 'Y_B', 'CB_R', 'CB_G', 'CR_G', 'CR_B')  # (HALF, Cb's B term and Cr's R term, is the shift i << 5: no table)
INVERSE = ('R_CR', 'G_CB', 'G_CR', 'B_CB')


def forward_np(t, r, g, b):
    y = (t['Y_R'][r] + t['Y_G'][g] + t['Y_B'][b]) >> 6
    cb = ((t['CB_R'][r] + t['CB_G'][g] + t['HALF'][b]) >> 6) + 128
    cr = ((t['HALF'][r] + t['CR_G'][g] + t['CR_B'][b]) >> 6) + 128
    return y, cb, cr


def inverse_np(t, y, cb, cr):
    y = y.astype(np.int64)
    return (np.clip(y + (t['R_CR'][cr] >> 6), 0, 255), np.clip(y + ((t['G_CB'][cb] + t['G_CR'][cr]) >> 6), 0, 255),
            np.clip(y + (t['B_CB'][cb] >> 6), 0, 255))


def all_triples():
    """[4096, 4096, 3] uint8 holding every triple once: pixel (i, j) is (i >> 4, ((i & 15) << 4) | (j >> 8), j & 255)"""
    i, j = np.meshgrid(np.arange(4096), np.arange(4096), indexing='ij')
    return np.stack([i >> 4, ((i & 15) << 4) | (j >> 8), j & 255], axis=-1).astype(np.uint8)


def mismatches(t):
    """(forward, inverse) mismatch counts per channel against Pillow over all 2^24 triples"""
    img = all_triples()
    a, b, c = (img[..., k].astype(np.intp) for k in range(3))
    want = pil_forward(img)
    fwd = [int(np.count_nonzero(got != want[..., k])) for k, got in enumerate(forward_np(t, a, b, c))]
    want = pil_inverse(img)
    inv = [int(np.count_nonzero(got != want[..., k])) for k, got in enumerate(inverse_np(t, img[..., 0], b, c))]
    return fwd, inv


def render(t):
    out = ['// color_tables.h -- Pillow\'s 8-bit JFIF colour tables (6 fractional bits), recovered from Pillow %s by' % PIL.__version__,
           '// tools/gen_color_tables.py, which states the arithmetic they enter.  Data: generated, not edited.',
           '#pragma once', '#include <stdint.h>', '',
           '#ifndef AIVC_COLOR_TABLE  /* (color.hip places the tables in device memory) */', '#define AIVC_COLOR_TABLE static const', '#endif', '',
           '#define AIVC_COLOR_FWD_TABLES %d' % len(FORWARD), '#define AIVC_COLOR_INV_TABLES %d' % len(INVERSE), '']
    for group, names in (('FWD', FORWARD), ('INV', INVERSE)):
        out += ['#define AIVC_COLOR_%s %d' % (name, k) for k, name in enumerate(names)]
        out.append('AIVC_COLOR_TABLE int16_t AIVC_COLOR_%s[%d][256] = {' % (group, len(names)))
        for name in names:
            v = t[name]
            assert v.min() >= -32768 and v.max() <= 32767
            out.append('    /* %s */ {' % name)
            out += ['        ' + ', '.join('%d' % x for x in v[k:k + 16]) + ',' for k in range(0, 256, 16)]
            out.append('    },')
        out += ['};', '']
    return '\n'.join(out) + '\n'

def parse_header(text):
    """{name: int64 [256]} from the text of color_tables.h (HALF, which has no table, included)"""
    import re
    t = {name: np.array([int(x) for x in body.replace('\n', ' ').split(',') if x.strip()], np.int64)
         for name, body in re.findall(r'/\* (\w+) \*/ \{([^}]*)\}', text)}
    assert sorted(t) == sorted(FORWARD + INVERSE) and all(v.shape == (256,) for v in t.values())
    t['HALF'] = 32 * I
    return t


if __name__ == '__main__':
    tables = recover()
    fwd, inv = mismatches(tables)
    sys.stderr.write('mismatches against Pillow %s over 2^24 triples: Y/Cb/Cr %s, R/G/B %s\n' % (PIL.__version__, fwd, inv))
    if any(fwd) or any(inv):
        sys.exit('tables are not exact')
    sys.stdout.write(render(tables))
