"""The encoder's per-frame quality record, scored on the device while the frames are coded.

FrameCodec.encode_units(stats=QualityStats(...)) hands every level batch over right after its reconstruction:
  * aivc_frame_sse_u8     the exact squared error of the batch's 8-bit planes (PSNR: the same on every GPU and rank count),
  * aivc_frame_aux_stats  the sums of MOFNet's alpha / beta maps and of (warping - code)^2, fixed summation order,
  * aivc_ssim_means / aivc_pool2x2  MS-SSIM of all luma planes of the batch as [N,h,w] and of its chroma planes as
                          [2N,hc,wc]: 5 + 5 scale launches and 4 + 4 pooling pairs per batch instead of per frame.
Only the few numbers per frame stay (on the device, until rows() fetches them all at once): nothing here synchronises the
host, the auxiliary tensors are dropped with the batch.

A row is ROW_LEN float64: sse y / u / v, sum alpha, sum beta, sum (warping - code)^2, MS-SSIM y / u / v, the four section
sizes in bytes (MOFNet z, y, CodecNet z, y), h, w.  func_util.result_logging.frame_result turns it into the reference's
per-frame dictionary (src/model_mngt/loss_function.py:103-257)."""
import numpy as np
import torch

from . import ops
from .func_util.ms_ssim import _WEIGHTS, gaussian

ROW_LEN = 15


def msssim_planes_u8(a, b, window_size=11):
    """a, b: uint8 CUDA planes [n,h,w] -> float64 CUDA [n]: msssim(val_range=1) of src/func_util/ms_ssim.py:93-150 of every
    plane pair on its own (levels / 255 in fp64; five scales, the window shrinks to the plane)"""
    p1, p2 = a.to(torch.float64) / 255.0, b.to(torch.float64) / 255.0
    mssim = mcs = None
    terms = []
    for s, wgt in enumerate(_WEIGHTS):
        _, h, w = p1.shape
        win = gaussian(min(window_size, h, w), 1.5).numpy().astype(np.float64)
        m = ops.ssim_means(p1, p2, win, 0.01 ** 2, 0.03 ** 2)  # [n, 2]: mean SSIM, mean contrast-structure
        terms.append((m[:, 0] if s == len(_WEIGHTS) - 1 else m[:, 1]) ** wgt)
        if s < len(_WEIGHTS) - 1:
            p1, p2 = ops.pool2x2(p1, 0), ops.pool2x2(p2, 0)
    return torch.prod(torch.stack(terms), dim=0)


class QualityStats:
    """collector of FrameCodec.encode_units(stats=...): rows under (unit, display index in the unit)"""

    def __init__(self):
        self._batches = []   # (keys, h, w, sse [n,3] int64, aux [n,3] fp64, ms-ssim y [n] fp64, ms-ssim u then v [2n] fp64)
        self._sections = {}  # key -> [4 sizes]

    def score_batch(self, keys, aux):
        """aux: what encode_batch(want_aux=True) returned for the frames `keys` (in batch order)"""
        cur, rec = aux['cur_planes'], aux['rec_planes']
        if rec is None:
            raise ValueError('a frame that is not reconstructed cannot be scored')
        n, h, w = cur['y'].shape
        sse = ops.frame_sse_u8(cur, rec)
        sums = ops.frame_aux_stats(aux.get('alpha'), aux.get('beta'), aux.get('warping'), aux['code'], c=3)
        ms_y = msssim_planes_u8(cur['y'], rec['y'])
        ms_c = msssim_planes_u8(torch.cat([cur['u'], cur['v']]), torch.cat([rec['u'], rec['v']]))
        self._batches.append((list(keys), h, w, sse, sums, ms_y, ms_c))

    def add_sections(self, key, sizes):
        self._sections[key] = [int(v) for v in sizes]

    def rows(self):
        """-> {key: float64 [ROW_LEN]} of every frame scored so far (one device -> host copy per batch, waits for them)"""
        out = {}
        for keys, h, w, sse, sums, ms_y, ms_c in self._batches:
            n = len(keys)
            sse, sums, ms_y, ms_c = (t.cpu().numpy() for t in (sse, sums, ms_y, ms_c))
            for i, k in enumerate(keys):
                sec = self._sections.get(k, [0, 0, 0, 0])
                out[k] = np.array([sse[i, 0], sse[i, 1], sse[i, 2], sums[i, 0], sums[i, 1], sums[i, 2],
                                   ms_y[i], ms_c[i], ms_c[n + i]] + sec + [h, w], np.float64)
        return out
