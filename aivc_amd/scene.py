"""Scene cuts and the unit layout that follows from them: pure functions of Python integers, no torch.

The encoder's input is one number per pair of consecutive frames, the sum of absolute luma differences
(aivc_amd.ops.pair_sad_u8, include/aivc_hip_scene.h).  scene_cuts() decides on them, plan_units() cuts the clip into
intra-period units so that every cut opens a unit -- each unit with a coding structure of its own, which its 6-byte GOP header
states and every decoder of the format already reads -- and UnitLayout is the ONE statement of where a frame of the clip lies
in that sequence of units: the encoder, the byte budgets, the quality log and the digests all ask it.

Both results are integer arithmetic on integer inputs: every rank of a distributed encode computes the same layout."""
import bisect

from .func_util.GOP_structure import generate_gop_struct

DEFAULT_THRESHOLD = 10.0  # grey levels of mean absolute difference; a convention, not measured on real material


def scene_cuts(sad, npix, threshold=DEFAULT_THRESHOLD):
    """sad[t - 1]: the sum of absolute luma differences between frames t - 1 and t of an n-frame clip (n = len(sad) + 1),
    S_t below; npix: samples per luma plane; threshold: grey levels of mean absolute difference.
    -> the sorted display positions t, 1 <= t <= n - 1, of the frames that open a new scene:
        16 * (S_t - max(S_{t-1}, S_{t+1})) >= round(16 * threshold) * npix
    with a neighbour that does not exist (t = 1, t = n - 1) left out; a frame without any neighbour (n = 2) is no cut.
    A peak rule: a cut stands out over BOTH its neighbours.  A moving scene's ordinary difference cancels, and a one-frame
    flash -- two equal peaks side by side -- is no cut."""
    s = [int(v) for v in sad]
    npix = int(npix)
    if npix <= 0:
        raise ValueError('scene_cuts: npix must be positive, got %d' % npix)
    if threshold < 0:
        raise ValueError('scene_cuts: the threshold cannot be negative, got %r' % (threshold,))
    bound = int(round(16 * threshold)) * npix
    n = len(s) + 1
    cuts = []
    for t in range(1, n):
        around = [s[k - 1] for k in (t - 1, t + 1) if 1 <= k <= n - 1]
        if around and 16 * (s[t - 1] - max(around)) >= bound:
            cuts.append(t)
    return cuts


def cut_scores(sad, npix, cuts):
    """grey levels by which each cut's mean absolute difference stands over its neighbours' (what the [SCENE] lines print)"""
    s = [int(v) for v in sad]
    n = len(s) + 1
    return [(s[t - 1] - max(s[k - 1] for k in (t - 1, t + 1) if 1 <= k <= n - 1)) / float(npix) for t in cuts]


class UnitLayout:
    """The intra-period units of an n-frame clip: unit u is coded under the structure names[u], holds lengths[u] frames
    (= len(generate_gop_struct(names[u]))), starts at display position starts[u], and real[u] of its frames are frames of the
    clip -- the others, behind the clip's last frame, repeat that frame (only the last unit has any)."""

    def __init__(self, n_frames, names, starts, lengths, real):
        self.n_frames = int(n_frames)
        self.names, self.starts, self.lengths, self.real = list(names), list(starts), list(lengths), list(real)

    def __len__(self):
        return len(self.names)

    def __eq__(self, other):
        return isinstance(other, UnitLayout) and (self.n_frames, self.names, self.starts, self.lengths, self.real) == \
            (other.n_frames, other.names, other.starts, other.lengths, other.real)

    def __repr__(self):
        return 'UnitLayout(%d frames: %s)' % (self.n_frames, ', '.join('%s@%d' % p for p in zip(self.names, self.starts)))

    @property
    def coded_frames(self):
        return sum(self.lengths)

    @property
    def padding(self):
        """repeats of the last frame behind the clip's end"""
        return self.coded_frames - self.n_frames

    def position(self, u, i):
        """display position in the clip of frame i of unit u (>= n_frames: a padded repeat)"""
        if not (0 <= u < len(self.names) and 0 <= i < self.lengths[u]):
            raise IndexError('no frame %d in unit %d of %r' % (i, u, self))
        return self.starts[u] + i

    def locate(self, t):
        """(u, i) of display position t (the padded repeats behind the clip's end included)"""
        if not 0 <= t < self.coded_frames:
            raise IndexError('position %d outside the %d coded frames' % (t, self.coded_frames))
        u = bisect.bisect_right(self.starts, t) - 1
        return u, t - self.starts[u]

    def units(self, frames):
        """the frame lists of the units, the tail padded by repeating the last frame"""
        if len(frames) != self.n_frames:
            raise ValueError('%d frames for a layout of %d' % (len(frames), self.n_frames))
        last = self.n_frames - 1
        return [[frames[min(s + i, last)] for i in range(n)] for s, n in zip(self.starts, self.lengths)]

    def keys(self):
        """(u, i) of every coded frame, in display order"""
        return [(u, i) for u, n in enumerate(self.lengths) for i in range(n)]

    def summary(self):
        """'<count> (<count> x <name>, ...)', the names in order of first use"""
        count = {}
        for name in self.names:
            count[name] = count.get(name, 0) + 1
        return '%d (%s)' % (len(self.names), ', '.join('%d x %s' % (c, name) for name, c in count.items()))


def _remainder_units(gop_name, r):
    """the units that code exactly r frames (0 < r < the configured structure's length) in front of a cut"""
    m = r - 1
    toks = gop_name.split('_')
    if m == 0:
        return ['1_GOP_0']
    if 'LDP' in toks:
        return ['LDP_%d' % m]
    if m == 1:
        return ['LDP_1']
    if m % 2:  # odd: the even structure over the first m frames, the last one on its own
        return _remainder_units(gop_name, r - 1) + ['1_GOP_0']
    size = 1 << (max(int(toks[-1]), 2).bit_length() - 1)  # the largest power of two <= the configured GOP size
    while m % size:
        size //= 2
    return ['%d_GOP_%d' % (m // size, size)]  # one I frame, m / size chained GOPs behind it


def plan_units(n_frames, cuts, gop_name):
    """The units of an n_frames clip coded under gop_name with a new unit at every display position of `cuts`.
    The clip falls into segments at the cuts.  Inside a segment: units of gop_name while a whole one fits; what is left of
    the LAST segment is one more gop_name unit, padded by repeating the last frame (no cuts: ceil(n / U) units, the layout
    of a clip coded by counting); what is left in front of a cut has to be coded exactly, since nothing can be padded
    mid-stream, and takes the structure with the fewest intra frames that a GOP header can express (_remainder_units).
    1_GOP_0: every frame is a unit already, cuts change nothing."""
    n = int(n_frames)
    if n <= 0:
        raise ValueError('plan_units: a clip has at least one frame')
    cuts = sorted({int(c) for c in cuts})
    if cuts and not (1 <= cuts[0] and cuts[-1] <= n - 1):
        raise ValueError('plan_units: cuts %s outside 1 ... %d' % (cuts, n - 1))
    unit = len(generate_gop_struct(gop_name))
    names = []
    bounds = [0] + (cuts if unit > 1 else []) + [n]
    for a, b in zip(bounds, bounds[1:]):
        whole, left = divmod(b - a, unit)
        names += [gop_name] * whole
        if left:
            names += [gop_name] if b == n else _remainder_units(gop_name, left)
    lengths = [unit if name == gop_name else len(generate_gop_struct(name)) for name in names]
    starts, pos = [], 0
    for k in lengths:
        starts.append(pos)
        pos += k
    return UnitLayout(n, names, starts, lengths, [min(k, n - s) for s, k in zip(starts, lengths)])


def as_layout(layout_or_unit, nb_gop, nb_frames, gop_name=None):
    """callers that count in whole units of one length pass that length: the uniform layout of nb_gop such units"""
    if isinstance(layout_or_unit, UnitLayout):
        return layout_or_unit
    unit = int(layout_or_unit)
    starts = [u * unit for u in range(nb_gop)]
    return UnitLayout(nb_frames, [gop_name] * nb_gop, starts, [unit] * nb_gop, [max(0, min(unit, nb_frames - s)) for s in starts])
