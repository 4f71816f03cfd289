"""The options of encode.py, decode.py and aivc.py, and of the library calls behind them, each stated once.

Source and Sink are the two records the options travel in: how a clip becomes the 8-bit 4:2:0 planes that are coded, and how
decoded planes are written.  A field's name is the flag's, the argparse dest and the key of the param dictionaries
(real_life.encode.encode, real_life.decode.decode_one_video, func_util.img_processing.load_frames); Source() and Sink() hold the
defaults, and nothing else writes them down.  check(path) is the one statement of which option goes with which kind of input or
output: a command line turns its ValueError into an argparse error (parse), the library lets it propagate.

FLAGS declares every shared flag of the three commands: its argparse keywords here, what follows the parse in _normalise, how a
value goes back into an argument list in argv_of (aivc.py runs the other two in-process).  To add an option: a field (or an
UNSAID entry), a FLAGS entry, and its use.  Pure Python: importing this needs neither torch nor a GPU."""
import argparse
import collections
import os

from . import color, png, rawvideo, resize


def is_png_folder(out_file):
    """the opt-in of -o: a name that ends in '/' or an existing directory asks for RGB pictures, anything else for a .yuv"""
    return bool(out_file) and (out_file.endswith('/') or os.path.isdir(out_file))


class _Record:
    """what Source and Sink share; SIZE names the field whose size `resample` is the filter of"""
    __slots__ = ()

    @classmethod
    def from_param(cls, param):
        """the record of a param dictionary, by func_util.nn_util.get_value's rule: an absent or None entry is the default"""
        return cls(**{k: param[k] for k in cls._fields if param.get(k) is not None})

    @classmethod
    def from_args(cls, a):
        """the record of a parsed command line; without a size the filter is the default one, whatever the other half was given"""
        rec = cls(**{k: getattr(a, k) for k in cls._fields})
        return rec if getattr(rec, cls.SIZE) is not None else rec._replace(resample=cls().resample)

    def _check_resample(self):
        resize.check_resample(None if self.resample == type(self)().resample else self.resample, {'--' + self.SIZE: getattr(self, self.SIZE)})


class Source(_Record, collections.namedtuple('Source', 'pix_fmt png_reader colour chroma_down size resample',
                                             defaults=(None, 'pillow', None, 'point', None, resize.DEFAULT_FILTER))):
    """how a clip becomes the planes that are coded (real_life.encode.encode says what each entry means)"""
    __slots__ = ()
    SIZE = 'size'

    def check(self, path):
        """a ValueError for an option that does not go with the input `path`: png_reader 'device' needs a directory, a colour a
        folder of RGB pictures, chroma_down 'box' a colour, a resample filter a size"""
        png.check_reader(self.png_reader, path, os.path.isdir(path))
        color.check_convertible(self.colour, self.chroma_down, path, self.colour is not None and color.is_rgb_folder(path))
        self._check_resample()


class Sink(_Record, collections.namedtuple('Sink', 'out_size resample out_pix_fmt fps png_coder colour',
                                           defaults=(None, resize.DEFAULT_FILTER, 'yuv420p', (25, 1), 'pillow', None))):
    """how decoded planes are written (real_life.decode.decode_one_video says what each entry means)"""
    __slots__ = ()
    SIZE = 'out_size'

    def check(self, out_file, odd_pictures=False):
        """a ValueError for an option that does not go with the output `out_file`: a .y4m name needs a layout that has a tag,
        png_coder 'device' and a colour need a picture folder, a resample filter an out_size.  A picture folder refuses an odd
        out_size, for the encoder's sake; odd_pictures: the library's word, it writes what it is asked to"""
        folder = is_png_folder(out_file)
        rawvideo.check_writable(self.out_pix_fmt, '' if folder else out_file)
        png.check_coder(self.png_coder, out_file or None, folder)
        color.check_convertible(self.colour, 'point', out_file, folder, flag='-o')
        self._check_resample()
        if self.out_size is not None and folder and not odd_pictures and (self.out_size[0] % 2 or self.out_size[1] % 2):
            # their chroma would not be the ceil-sized planes the encoder takes back (real_life.encode.read_png_folder)
            raise ValueError('--out_size %dx%d with RGB pictures as output (-o %s): RGB pictures need even sides'
                             % (tuple(self.out_size) + (out_file,)))


SOURCE, SINK = Source(), Sink()
# what an option holds when its flag is not given, after _normalise: the value argv_of leaves out
UNSAID = dict(SOURCE._asdict(), idx_rate=0, target_bpp=0., rate_step=0.0625, scene_cut=None, verify='', frames=None, max_level=None,
              **SINK._asdict())


# ---- the declarations ----------------------------------------------------------------------------------------------------------
def _size_arg(text):
    try:
        return resize.parse_size(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def frames_arg(text):
    from .partial import parse_frames_arg
    try:
        return parse_frames_arg(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


_WRITABLE = [n for n in rawvideo.PIX_FMTS if rawvideo.PixFmt(n).writable]
_SIDES = {'source': '-i, a folder of RGB pictures', 'sink': '-o, a picture folder'}
_SIZES = {'source': '--size', 'sink': '--out_size'}


def _sides(groups, names, sep):
    return sep.join(names[g] for g in ('source', 'sink') if g in groups)


# flag -> its argparse keywords, or a function of the command's groups that gives them
FLAGS = {
    '--idx_rate': dict(default=None, type=float,
                       help='rate index of the whole clip: a multiple of 1/16 in [0, rate indices of the model - 1]; default 0'),
    '--target_bpp': dict(default=UNSAID['target_bpp'], type=float,
                         help='bit per pixel: every intra-period unit is coded at the richest rate index whose GOP record fits '
                              'target_bpp x w x h x frames / 8 bytes (a few bitstream-only encodes per unit); 0: off'),
    '--rate_step': dict(default=UNSAID['rate_step'], type=float, help='grid step of the --target_bpp search (a multiple of 1/16)'),
    '--scene_cut': dict(nargs='?', const=10.0, default=None, type=float, metavar='T',
                        help='detect scene cuts on the device and open a new intra-period unit at each: a frame whose mean absolute '
                             'luma difference to its predecessor stands out over both neighbouring differences by at least T grey '
                             'levels (default 10, a convention that has not been measured on real material); the units in front of a '
                             'cut take a shorter coding structure, any decoder of the format reads the stream; off by default'),
    '--verify': dict(nargs='?', const=True, default=UNSAID['verify'], metavar='MANIFEST',  # '' is off, True the manifest next to the bitstream
                     help='digest the decoded planes on the device and compare them with the manifest the encoder wrote under '
                          '--digests (default: <bitstream>.md5); exit status 4 when planes differ and the stream itself decoded cleanly'),
    '--frames': dict(default=None, type=frames_arg, metavar='A:B',
                     help='partial decode: only the frames A ... B (inclusive, absolute display indices as in the manifest and the '
                          'picture names; also A:, :B or A) are written; only their references are decoded and only their units read'),
    '--max_level': dict(default=None, type=int, metavar='L',
                        help='partial decode: only frames of temporal level <= L (the dependency depth inside an intra-period unit: '
                             '0 the I frame, 1 the P frame; 1_GOP_32 has levels 0 ... 6, each one less halves the frame count)'),
    '--pix_fmt': dict(default=SOURCE.pix_fmt, choices=rawvideo.PIX_FMTS, metavar='NAME',
                      help='layout of a headerless -i file, under ffmpeg\'s names (%s); unset: the _420 / _422 / _444 and _10b / _12b / '
                           '_16b / _<n>bit tokens of its name, default yuv420p.  A .y4m file says what it holds.  Anything but planar '
                           '8-bit 4:2:0 is converted to it on the device before everything else (--size included): what is coded, '
                           'digested and scored by --log_dir are the converted planes' % ', '.join(rawvideo.PIX_FMTS)),
    '--png_reader': dict(default=SOURCE.png_reader, choices=png.READERS,
                         help='who reads the pictures of a folder given as -i: pillow (one Image.open per picture on the host, the default) or '
                              'device (8-bit grey and RGB pictures are inflated and unfiltered on the device, all pictures of the clip at '
                              'once; any other PNG still goes through Pillow); the same planes and the same bitstream either way'),
    '--matrix': lambda groups: dict(
        default=None, choices=list(color.MATRICES),
        help='the colour matrix of the 8-bit planes (%s): RGB pictures are converted by it, in integers on the device, instead of '
             'by Pillow\'s arithmetic (BT.601, full range, the default without this flag).  --matrix alone means --range limited, '
             'video\'s convention.  The stream stores no colour description: encoder and decoder are both told (%s)'
             % (', '.join(color.MATRICES), _sides(groups, _SIDES, ' and '))),
    '--range': dict(default=None, choices=list(color.RANGES),
                    help='range of the planes under --matrix: limited (luma 16 ... 235, chroma 16 ... 240; the default) or full'),
    '--chroma_down': dict(default=SOURCE.chroma_down, choices=list(color.CHROMA_DOWN),
                          help='the chroma of a 4:2:0 sample under --matrix: point (of pixel (2i, 2j) alone, the default) or box (of '
                               'the sum of the 2 x 2 block, rounded once)'),
    '--size': dict(default=SOURCE.size, type=_size_arg, metavar='WxH',
                   help='code the clip at this size: every plane is resized on the device right after it has been read (y to H x W, u '
                        'and v to the ceil half size, each on its own; RGB pictures are converted to 4:2:0 first); header, scene cuts, '
                        'digests, the byte budget of --target_bpp and the --log_dir table (which scores against the RESIZED source) see '
                        'the coded size.  The stream has no display-size field: decode.py --out_size writes another size'),
    '--out_size': dict(default=SINK.out_size, type=_size_arg, metavar='WxH',
                       help='write the decoded frames at this size: resized on the device just before they are written, .yuv or pictures '
                            '(y to H x W, u and v to the ceil half size); --verify keeps digesting the planes at coded size, --frames / '
                            '--max_level resize only what they write.  The name of a .yuv output is the caller\'s business'),
    '--resample': lambda groups: dict(
        default=None, choices=list(resize.FILTERS),
        help="the filter of %s: Pillow's Image.resize on every 8-bit plane, bit for bit, on the device; default %s "
             "(Pillow's own default)" % (_sides(groups, _SIZES, ' / '), SOURCE.resample)),
    '--out_pix_fmt': dict(default=SINK.out_pix_fmt, choices=_WRITABLE, metavar='NAME',
                          help='layout of the file that is written (%s; 4:2:0 and grey layouts only): exported on the device, after '
                               '--out_size.  -o out.y4m writes a .y4m file (planar and grey layouts)' % ', '.join(_WRITABLE)),
    '--fps': dict(default='%d:%d' % SINK.fps, type=str, metavar='N[:D]',
                  help='frame rate in the header of a .y4m output (default 25:1): the stream stores no frame rate'),
    '--png_coder': dict(default=SINK.png_coder, choices=png.CODERS,
                        help='who codes the <idx>.png pictures of a folder given as -o: pillow (one Image.save per frame on the host, the '
                             'default) or device (row filters and a Huffman deflate on the GPU: the same pixels, other bytes)'),
}
RATE, SCENE, VERIFY, PARTIAL = ('idx_rate', 'target_bpp', 'rate_step'), ('scene_cut',), ('verify',), ('frames', 'max_level')


def _flags_of(record):
    """the flags that fill a record: one per field, --matrix and --range for colour"""
    return tuple(d for f in record._fields for d in (('matrix', 'range') if f == 'colour' else (f,)))


GROUPS = {'rate': RATE, 'scene': SCENE, 'verify': VERIFY, 'partial': PARTIAL, 'source': _flags_of(Source), 'sink': _flags_of(Sink)}


def _contract(choices):
    """--contract: unset is the behaviour without the flag, AIVC_CONTRACT or the library default"""
    return dict(default=None, choices=list(choices),
                help='arithmetic contract of the run (aivc_amd.ops.set_precision); an encoder and a decoder must agree.  '
                     'Unset: AIVC_CONTRACT or the library default'
                     + ('.  auto: the contract named by the manifest <bitstream>.md5, else a trial decode of the first unit'
                        if 'auto' in choices else ''))


def _normalise(a, groups):
    """what follows the parse: --idx_rate None becomes 0, --fps (N, D), --resample None the default filter, --matrix / --range
    a.colour; a ValueError for values, and pairs of flags, that no input or output makes lawful"""
    if 'rate' in groups:
        from . import rate_control
        if a.target_bpp < 0:
            raise ValueError('--target_bpp must be positive (0: off)')
        if a.idx_rate is not None and a.target_bpp > 0:
            raise ValueError('--idx_rate and --target_bpp are mutually exclusive: a byte budget chooses the rate index itself')
        if a.idx_rate is not None and (a.idx_rate < 0 or not rate_control.on_sixteenths(a.idx_rate)):
            raise ValueError('--idx_rate %r: expected a non-negative multiple of 1/16 (the GOP header stores sixteenths)' % a.idx_rate)
        if a.rate_step <= 0 or not rate_control.on_sixteenths(a.rate_step):
            raise ValueError('--rate_step %r: expected a positive multiple of 1/16' % a.rate_step)
        a.idx_rate = UNSAID['idx_rate'] if a.idx_rate is None else a.idx_rate
    if 'scene' in groups and a.scene_cut is not None and not a.scene_cut >= 0:
        raise ValueError('--scene_cut %r: the threshold is a non-negative number of grey levels' % a.scene_cut)
    if 'partial' in groups and a.max_level is not None and a.max_level < 0:
        raise ValueError('--max_level %d: temporal levels count from 0' % a.max_level)
    if 'sink' in groups:
        a.fps = rawvideo.parse_fps(a.fps)
    if 'source' in groups or 'sink' in groups:
        if a.matrix is None and a.range is not None:
            raise ValueError('--range %s needs --matrix: without it the conversion is Pillow\'s (BT.601, full range)' % a.range)
        a.colour = None if a.matrix is None else color.ColourSpec(a.matrix, a.range or 'limited')
        resize.check_resample(a.resample, {_SIZES[g]: getattr(a, _SIZES[g][2:]) for g in ('source', 'sink') if g in groups})
        a.resample = SOURCE.resample if a.resample is None else a.resample


def parse(p, argv, *groups, contract=None):
    """the rest of a parse_args: declares the flags of `groups` (and --contract with these choices) on p, parses, normalises,
    builds a.source / a.sink and checks them against a.i / a.o.  A ValueError of any of this is an argparse error: exit status 2"""
    for dest in dict.fromkeys(d for g in groups for d in GROUPS[g]):
        kw = FLAGS['--' + dest]
        p.add_argument('--' + dest, **(kw(groups) if callable(kw) else kw))
    if contract:
        p.add_argument('--contract', **_contract(contract))
    a = p.parse_args(argv)
    try:
        _normalise(a, groups)
        if 'source' in groups:
            a.source = Source.from_args(a)
            a.source.check(a.i)
        if 'sink' in groups:
            a.sink = Sink.from_args(a)
            a.sink.check(a.o)
    except ValueError as e:
        p.error(str(e))
    return a


_TEXT = {'size': '%dx%d', 'out_size': '%dx%d', 'fps': '%d:%d'}


def argv_of(a, dests=None, always=()):
    """a record, or the entries `dests` of a parsed command line, written back as an argument list: every option that does not hold
    what it holds unsaid (UNSAID), and those named in `always`"""
    values = a._asdict() if dests is None else {d: getattr(a, d) for d in dests}
    out = []
    for dest, v in values.items():
        if v == UNSAID[dest] and dest not in always:
            continue
        if dest == 'colour':
            out += ['--matrix', v.matrix, '--range', v.range]
        else:
            out += ['--' + dest] + ([] if v is True else [_TEXT[dest] % tuple(v) if dest in _TEXT else str(v)])
    return out
