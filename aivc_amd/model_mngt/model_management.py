"""load_model / infer_one_sequence / infer_one_GOP with the reference's signatures
(src/model_mngt/model_management.py)."""
import math
import os

import torch

from ..func_util.console_display import print_log_msg
from ..func_util.nn_util import get_value
from ..real_life.bitstream import ArithmeticCoder
from ..real_life.cat_binary_files import cat_one_video


def attach_arithmetic_coders(model, device=None):
    """src/model_mngt/model_management.py:349-359: the coders are not pickled, they are attached
    after loading."""
    for net in (model.codec_net.codec_net, model.mode_net.mode_net):
        net.ac = ArithmeticCoder({'balle_pdf_estim_z': net.pdf_z, 'device': device})
    return model


def load_model(prefix='', on_cpu=False):
    """torch.load of a full-module pickle './<prefix>model.pt' (src/model_mngt/model_management.py:341-361).
    Classes are resolved by the dotted path the pickle names (the reference's module names are aliases of this
    package, aivc_amd.install_aliases()) and, where that path does not exist here -- the `models` package is missing
    from the reference snapshot, its real module layout is unknown -- by CLASS NAME over this package's classes
    (pickle_compat.py).  Every name that resolves neither way is reported before the load starts."""
    import aivc_amd
    from . import pickle_compat
    aivc_amd.install_aliases()
    path = './' + prefix + 'model.pt'
    missing = pickle_compat.unresolved(path)
    if missing:
        raise ImportError('%s names classes this build does not define: %s -- list what the file asks for with '
                          '`python tools/inspect_pickle.py %s`' % (path, ', '.join('%s.%s' % mn for mn in missing), path))
    map_loc = torch.device('cpu') if on_cpu else None
    by_name = []
    model = torch.load(path, map_location=map_loc, weights_only=False, pickle_module=pickle_compat.resolver(by_name))
    for mod, name, target in by_name:
        print_log_msg('INFO', 'load_model', 'class resolved by name', '%s.%s -> %s' % (mod, name, target))
    return attach_arithmetic_coders(model, map_loc)


def infer_one_GOP(param):
    default = {'model': None, 'GOP_struct': None, 'GOP_struct_name': None, 'raw_frames': None, 'l_codec': 0.,
               'l_mof': 0., 'index_GOP_in_video': 0, 'generate_bitstream': False, 'bitstream_dir': '',
               'real_idx_first_frame': 0, 'idx_rate': 0., 'flag_bitstream_debug': False}
    model = get_value('model', param, default).eval()
    keys = ('GOP_struct', 'GOP_struct_name', 'raw_frames', 'idx_rate', 'index_GOP_in_video',
            'generate_bitstream', 'real_idx_first_frame', 'bitstream_dir', 'flag_bitstream_debug')
    with torch.no_grad():
        net_out = model.GOP_forward({k: get_value(k, param, default) for k in keys})
    # x_hat is already cropped to the frame size and cast to 8-bit levels by the reconstruction kernel
    result = {f: {'size_bytes': float(sum(net_out[f][k].item() for k in
                                          ('mode_rate_y', 'mode_rate_z', 'codec_rate_y', 'codec_rate_z')) / 8)}
              for f in net_out}
    return net_out, result


def infer_one_sequence(param):
    """GOP loop over a PNG-triplet directory is replaced by direct planar input: `raw_video` is a
    list of YUV dicts (float levels or uint8) for frames idx_starting_frame..idx_end_frame."""
    default = {'model': None, 'GOP_struct': None, 'GOP_struct_name': None, 'raw_video': None,
               'idx_starting_frame': 0, 'idx_end_frame': 8, 'generate_bitstream': False, 'bitstream_dir': '',
               'idx_rate': 0., 'flag_bitstream_debug': False, 'final_bitstream_path': ''}
    model = get_value('model', param, default)
    gop = get_value('GOP_struct', param, default)
    gop_name = get_value('GOP_struct_name', param, default)
    video = get_value('raw_video', param, default)
    first = get_value('idx_starting_frame', param, default)
    last = get_value('idx_end_frame', param, default)
    gen = get_value('generate_bitstream', param, default)
    bdir = get_value('bitstream_dir', param, default)
    nb_frames = last - first + 1
    unit = len(gop)
    nb_gop = math.ceil(nb_frames / unit)
    print_log_msg('DEBUG', 'infer_one_sequence', 'nb_GOP', nb_gop)
    if gen:
        bdir = bdir if bdir.endswith('/') else bdir + '/'
        os.makedirs(bdir, exist_ok=True)
    seq = {}
    for i in range(nb_gop):
        raw = {'frame_%d' % f: video[min(i * unit + f, nb_frames - 1)] for f in range(unit)}
        _, res = infer_one_GOP({'model': model, 'GOP_struct': gop, 'GOP_struct_name': gop_name, 'raw_frames': raw,
                                'index_GOP_in_video': i, 'generate_bitstream': gen, 'bitstream_dir': bdir,
                                'real_idx_first_frame': i * unit + first,
                                'idx_rate': get_value('idx_rate', param, default)})
        for f in range(unit):
            seq['frame_%d' % (i * unit + f + first)] = res['frame_%d' % f]
    if gen:
        cat_one_video({'bitstream_dir': bdir, 'idx_starting_frame': first, 'idx_end_frame': last,
                       'final_bitstream_path': get_value('final_bitstream_path', param, default)})
    return seq


# ---- the per-frame result table of a sequence (src/model_mngt/model_management.py:96-116,156-241) -----------------------------
def lambda_tradeoff_of(model, idx_rate):
    """the rate weight of the logged loss: model.model_param['lambda_tradeoff'][round(idx_rate)], 0.0 for a model without one"""
    lambdas = (getattr(model, 'model_param', None) or {}).get('lambda_tradeoff')
    return float(lambdas[int(round(idx_rate))]) if lambdas else 0.0


def sequence_result_from_rows(rows, nb_gop, unit, idx_starting_frame, nb_frames, lambda_tradeoff=0.0):
    """rows: {(unit number, display index): row of aivc_amd.quality} of all nb_gop x unit coded frames -> the reference's
    sequence_result: {'frame_<index in the video>': result dictionary, ..., 'sequence': their average}, the frames in display
    order; the frames past nb_frames are the padding of the last unit (rate counts, distortion does not).
    lambda_tradeoff: one number, or one per unit (units coded at different rate indices: the loss column of a frame uses its
    unit's; the sequence row averages the frames' columns, so its loss weighs every frame's rate with that frame's lambda).
    unit: the frames per unit, or the aivc_amd.scene.UnitLayout of a video whose units differ (scene cuts): a frame is named
    by its position in the layout, and the padding count is the layout's."""
    from ..func_util.result_logging import average_N_frame, frame_result
    from ..scene import as_layout
    layout = as_layout(unit, nb_gop, nb_frames)
    if len(layout.names) != nb_gop or layout.n_frames != nb_frames:
        raise ValueError('a layout of %d units and %d frames for %d units and %d frames'
                         % (len(layout.names), layout.n_frames, nb_gop, nb_frames))
    per_unit = isinstance(lambda_tradeoff, (list, tuple))
    seq = {}
    for u, i in layout.keys():
        seq['frame_%d' % (layout.position(u, i) + idx_starting_frame)] = frame_result(rows[(u, i)],
                                                                                     lambda_tradeoff[u] if per_unit else lambda_tradeoff)
    seq['sequence'] = average_N_frame(seq, nb_pad_frame=layout.padding)
    return seq


def write_detailed_log(working_dir, sequence_result, sequence_name):
    """<working_dir>/detailed.txt: the header, one row per coded frame, the sequence's average as the last line"""
    from ..func_util.result_logging import generate_header_file, generate_log_metric_one_frame
    os.makedirs(working_dir, exist_ok=True)
    path = os.path.join(working_dir, 'detailed.txt')
    with open(path, 'w') as f:
        f.write(generate_header_file())
        for name, res in sequence_result.items():
            res['pic_name'], res['frame_idx'] = sequence_name, name
            f.write(generate_log_metric_one_frame(res))
    return path
