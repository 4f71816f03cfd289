"""The encoder's per-frame result table, <working_dir>/detailed.txt, in the reference's format
(src/func_util/result_logging.py, src/model_mngt/loss_function.py:103-339, src/model_mngt/model_management.py:207-241).

A line is a row of cells between pipes, every cell centred in its column (str.center): the name column is 40 characters
wide, the eleven others 12.  The columns and the way each value is printed:

    Video        the sequence's name                       str
    Frame idx.   'frame_<index in the video>', 'sequence'  str
    PSNR dB      psnr                                      5 decimals
    R bpp        total_rate_bpp                            6 decimals
    R Mode bpp   mode_rate_bpp                             6 decimals
    R Codec bpp  codec_rate_bpp                            6 decimals
    alpha        mean_alpha                                3 decimals
    beta         mean_beta                                 3 decimals
    Loss         loss                                      5 decimals
    MS-SSIM dB   ms_ssim_db                                5 decimals
    h, w         luma size                                 as a float ('48.0': the reference keeps them in float tensors)

The numbers are Python floats (fp64) computed from what the device kernels summed (aivc_amd/quality.py); the reference holds
them in fp32 tensors."""
import math

SIZE_PIC_NAME = 40
SIZE_COL_LOG = 12

# (title, key of the result dictionary, format)
_COLUMNS = (('Video', 'pic_name', str), ('Frame idx.', 'frame_idx', str), ('PSNR dB', 'psnr', '%.5f'),
            ('R bpp', 'total_rate_bpp', '%.6f'), ('R Mode bpp', 'mode_rate_bpp', '%.6f'), ('R Codec bpp', 'codec_rate_bpp', '%.6f'),
            ('alpha', 'mean_alpha', '%.3f'), ('beta', 'mean_beta', '%.3f'), ('Loss', 'loss', '%.5f'),
            ('MS-SSIM dB', 'ms_ssim_db', '%.5f'), ('h', 'h', float), ('w', 'w', float))

# keys of a frame's result dictionary (those of compute_metrics_one_GOP)
RESULT_KEYS = ('loss', 'mse', 'mse_warping', 'psnr', 'psnr_warping', 'codec_rate_bpp', 'mode_rate_bpp', 'total_rate_bpp',
               'mean_alpha', 'mean_beta', 'ms_ssim', 'ms_ssim_db', 'h', 'w')
# distortion figures: a padded frame (a repeat of the last one that completes the last unit) counts for rate, not for these
_NOT_FOR_PADDED = ('mse', 'mse_warping', 'ms_ssim', 'ms_ssim_db', 'psnr')


def _line(cells):
    return ''.join('|' + c.center(SIZE_PIC_NAME if i == 0 else SIZE_COL_LOG) for i, c in enumerate(cells)) + '|\n'


def generate_header_file():
    """the top row of a log file"""
    return _line([title for title, _, _ in _COLUMNS])


def _scalar(v):
    return float(v.item()) if hasattr(v, 'item') else float(v)


def generate_log_metric_one_frame(result):
    """one row from a frame's (or the sequence's) result dictionary"""
    cells = []
    for _, key, fmt in _COLUMNS:
        v = result.get(key)
        if fmt is str:
            cells.append(str(v))
        elif fmt is float:
            cells.append(str(_scalar(v)))
        else:
            cells.append(fmt % _scalar(v))
    return _line(cells)


def _db(x):
    """10 log10(1 / x)"""
    return math.inf if x <= 0 else (-math.inf if math.isinf(x) else -10.0 * math.log10(x))


def frame_result(row, lambda_tradeoff=0.0):
    """a row of aivc_amd.quality (ROW_LEN numbers) -> the frame's result dictionary as compute_metrics_one_GOP fills it for the
    call infer_one_GOP makes (distortion = MSE, both rate weights = lambda, no frame weighting):
      mse = SSE / (255^2 x number of values over Y + U + V), ms_ssim = the numel-weighted mean over the three planes,
      rates in bit per luma pixel, loss = lambda x codec rate + lambda x mode rate + mse"""
    sse, (s_alpha, s_beta, s_warp), ms = row[0:3], row[3:6], row[6:9]
    sec, h, w = row[9:13], int(row[13]), int(row[14])
    n_y, n_c = h * w, ((h + 1) // 2) * ((w + 1) // 2)
    nb_values = n_y + 2 * n_c
    r = {}
    r['mse'] = float(sse[0] + sse[1] + sse[2]) / (255.0 ** 2 * nb_values)
    r['mse_warping'] = float(s_warp) / (3 * n_y)
    r['psnr'], r['psnr_warping'] = _db(r['mse']), _db(r['mse_warping'])
    r['mode_rate_bpp'] = 8.0 * float(sec[0] + sec[1]) / n_y
    r['codec_rate_bpp'] = 8.0 * float(sec[2] + sec[3]) / n_y
    r['total_rate_bpp'] = r['mode_rate_bpp'] + r['codec_rate_bpp']
    r['mean_alpha'], r['mean_beta'] = float(s_alpha) / n_y, float(s_beta) / n_y
    r['ms_ssim'] = float(ms[0] * n_y + ms[1] * n_c + ms[2] * n_c) / nb_values
    r['ms_ssim_db'] = _db(1.0 - r['ms_ssim'])
    r['loss'] = lambda_tradeoff * r['codec_rate_bpp'] + lambda_tradeoff * r['mode_rate_bpp'] + r['mse']
    r['h'], r['w'] = float(h), float(w)
    return r


def average_N_frame(x, nb_pad_frame=0):
    """x: {frame name: result dictionary} in display order, the last nb_pad_frame of them padding -> the average dictionary.
    Every key is the mean over all frames, except the distortion keys, which are the mean over the frames that are not
    padding; then the PSNRs come from the averaged MSEs and the MS-SSIM dB from the averaged MS-SSIM."""
    frames = list(x.values())
    nb_frame = len(frames)
    nb_real = nb_frame - nb_pad_frame
    avg = {}
    for k in frames[0]:
        if k in ('pic_name', 'frame_idx'):
            continue
        if k in _NOT_FOR_PADDED:
            avg[k] = sum(_scalar(f[k]) for f in frames[:nb_real]) / nb_real
        else:
            avg[k] = sum(_scalar(f[k]) for f in frames) / nb_frame
    avg['psnr'], avg['psnr_warping'] = _db(avg['mse']), _db(avg['mse_warping'])
    avg['ms_ssim_db'] = _db(1.0 - avg['ms_ssim'])
    return avg
