"""Choosing the rate index: the checks of a per-unit rate list, and byte budgets per intra-period unit.

The codec is variable-rate: a GainMatrix holds one gain vector per rate index, fractional indices are interpolated, and every
GOP header carries round(idx_rate * 16) in one byte.  FrameCodec.encode_units / encode_video take one rate per unit; this
module holds what is host logic about them (no torch, no device):

  check_unit_rates   what a rate given for a unit must satisfy to survive the header's byte
  rate_grid          the rates a search may choose from
  search_rates       the search for the richest grid rate of every unit that fits the unit's byte budget
  unit_budgets       byte budgets from a target in bit per pixel
  encode_video_budgeted   the search driven by real encodes (FrameCodec.encode_units on mixed-rate batches)

Nothing is assumed about which end of the index is the rich one (it depends on the model's gains): the search prices both
ends first.  Sizes are assumed to grow from the lean end to the rich end; where they do not, the search is still the
procedure written down at search_rates, and what it returns always fits unless the lean end itself does not.
"""
import math
from collections import namedtuple

UnitChoice = namedtuple('UnitChoice', 'rate nbytes over_budget probes')  # probes: [(rate, bytes), ...] in the order priced


def is_rate_list(idx_rate):
    """one rate per unit / item (a sequence), as opposed to one scalar for all"""
    return isinstance(idx_rate, (list, tuple))


def on_sixteenths(r):
    return r * 16 == round(r * 16)


def check_unit_rates(rates, nb_rates, unit_numbers=None):
    """Every rate of a per-unit list must be on the 1/16 grid the GOP header stores (one byte, round(r * 16)) and inside the
    model's gain matrix, 0 <= r <= nb_rates - 1; else ValueError naming the unit (unit_numbers[i]: the number of list entry
    i, default i).  -> the rates as floats"""
    out = []
    for i, r in enumerate(rates):
        u = i if unit_numbers is None else unit_numbers[i]
        try:
            r = float(r)
        except (TypeError, ValueError):
            raise ValueError('unit %d: idx_rate %r is not a number' % (u, r))
        if not (0.0 <= r <= nb_rates - 1) or not on_sixteenths(r):
            raise ValueError('unit %d: idx_rate %r: expected a multiple of 1/16 in [0, %d] (the GOP header stores '
                             'sixteenths in one byte; the model has %d rate indices)' % (u, r, nb_rates - 1, nb_rates))
        out.append(r)
    return out


def rate_grid(nb_rates, step=1 / 16):
    """0, step, 2 * step, ..., nb_rates - 1 (ascending); step a multiple of 1/16 that divides the range"""
    if step <= 0 or not on_sixteenths(step):
        raise ValueError('rate step %r: expected a positive multiple of 1/16' % (step,))
    top = nb_rates - 1
    k = int(round(step * 16))
    if (top * 16) % k:
        raise ValueError('rate step %r does not divide the index range [0, %d]' % (step, top))
    return [i * k / 16 for i in range(top * 16 // k + 1)]


def max_probe_calls(n_grid):
    """the bound on probe calls of search_rates for a grid of n_grid rates"""
    return 1 if n_grid == 1 else 2 + int(math.ceil(math.log2(n_grid - 1)))


def search_rates(probe, n_units, grid, budgets):
    """The richest rate of `grid` whose GOP blob fits the unit's budget, for n_units units at once.

    probe([(unit, rate), ...]) -> [bytes of that unit's GOP blob at that rate, ...]; grid: ascending rates; budgets: bytes per
    unit.  -> [UnitChoice per unit].  The procedure:
      1. every unit is priced at grid[0] and at grid[-1] (two probe calls).  The LEAN end of a unit is the one with fewer
         bytes (a tie: grid[0]), the other one its RICH end.
      2. rich <= budget: the rich end is chosen.  lean > budget: the lean end, over_budget=True.
      3. else bisection over grid positions counted from the lean end, lo = lean (fits), hi = rich (does not):
         mid = (lo + hi) // 2; bytes <= budget -> lo = mid, else hi = mid; until hi - lo == 1; lo is chosen.  A round is ONE
         probe call with every still open unit at its own mid.
      4. a one-point grid: one call, that point.
    At most 2 + ceil(log2(len(grid) - 1)) calls.  A unit's result depends on its own sizes only."""
    grid = list(grid)
    if len(budgets) != n_units:
        raise ValueError('%d budgets for %d units' % (len(budgets), n_units))
    units = list(range(n_units))
    probes = [[] for _ in units]

    def price(pairs):
        sizes = [int(s) for s in probe(list(pairs))]
        if len(sizes) != len(pairs):
            raise ValueError('probe returned %d sizes for %d (unit, rate) pairs' % (len(sizes), len(pairs)))
        for (u, r), s in zip(pairs, sizes):
            probes[u].append((r, s))
        return sizes

    if not units:
        return []
    first = price([(u, grid[0]) for u in units])
    if len(grid) == 1:
        return [UnitChoice(grid[0], first[u], first[u] > budgets[u], probes[u]) for u in units]
    last = price([(u, grid[-1]) for u in units])
    top = len(grid) - 1
    chosen = {}   # unit -> (position counted from the lean end, bytes)
    flipped = {}  # unit -> the lean end is grid[-1]: position p from the lean end is grid[top - p]
    state = {}    # open units -> [lo, hi, bytes at lo]
    for u in units:
        flipped[u] = last[u] < first[u]
        lean, rich = (last[u], first[u]) if flipped[u] else (first[u], last[u])
        if rich <= budgets[u]:
            chosen[u] = (top, rich)
        elif lean > budgets[u] or top == 1:
            chosen[u] = (0, lean)
        else:
            state[u] = [0, top, lean]

    def rate_at(u, pos):
        return grid[top - pos] if flipped[u] else grid[pos]

    while state:
        open_units = sorted(state)
        mids = {u: (state[u][0] + state[u][1]) // 2 for u in open_units}
        sizes = price([(u, rate_at(u, mids[u])) for u in open_units])
        for u, s in zip(open_units, sizes):
            if s <= budgets[u]:
                state[u][0], state[u][2] = mids[u], s
            else:
                state[u][1] = mids[u]
            if state[u][1] - state[u][0] == 1:
                chosen[u] = (state[u][0], state[u][2])
                del state[u]
    return [UnitChoice(rate_at(u, chosen[u][0]), chosen[u][1], chosen[u][1] > budgets[u], probes[u]) for u in units]


def unit_budgets(target_bpp, w, h, nb_frames, unit):
    """bytes per intra-period unit of a video of nb_frames frames of w x h in units of `unit` frames:
    floor(target_bpp * w * h * real frames of the unit / 8) -- the repeats that pad the last unit do not count"""
    nb_gop = int(math.ceil(nb_frames / unit))
    return [int(math.floor(target_bpp * w * h * min(unit, nb_frames - u * unit) / 8)) for u in range(nb_gop)]


def layout_budgets(target_bpp, w, h, layout):
    """unit_budgets for the units of an aivc_amd.scene.UnitLayout: floor(target_bpp * w * h * real[u] / 8) bytes for unit u"""
    return [int(math.floor(target_bpp * w * h * r / 8)) for r in layout.real]


def nb_rates_of(frame_codec):
    """rate indices of the codec's model (the gain matrices of both networks have the same number)"""
    return len(frame_codec.cod.gain_I.enc_gain_list)


def encode_video_budgeted(frame_codec, frames, gop_name, budgets_or_bpp, step=1 / 16, idx_starting_frame=0, stats=None,
                          unit_filter=None, layout=None):
    """FrameCodec.encode_video with the rate index of every intra-period unit chosen by search_rates so that the unit's GOP
    blob -- len(gops[u]): GOP header and frame length prefixes included, the 18-byte video header not -- fits its budget.
    budgets_or_bpp: a list of bytes per unit of the video, or a number: a target in bit per pixel (unit_budgets).
    A probe is encode_units on the still open units, each at its own rate, bitstream only (recon='refs'): one mixed-rate
    batch per dependency level.  One last encode_units call with every unit at its chosen rate (recon='all', stats) gives the
    returned video; its blobs are the bytes the probes priced.  unit_filter: as in encode_video (each rank of a unit-sharded
    job searches its own units; a unit's result does not depend on the others).
    -> encode_video's dict + 'rates' ([rate per unit], None for units filtered out), 'choices' ([UnitChoice or None]) and
    'budgets'.
    layout (aivc_amd.scene.UnitLayout, optional): the units of the video where they are not ceil(n / unit) units of gop_name
    (scene cuts); budgets, probes and the final pass all speak of ITS units, a target in bit per pixel weighs unit u with its
    real[u] frames."""
    from . import scene
    n = len(frames)
    uniform = layout is None
    if uniform:
        layout = scene.plan_units(n, (), gop_name)
    nb_gop = len(layout.names)
    h, w = frames[0]['y'].shape[-2:]
    if isinstance(budgets_or_bpp, (list, tuple)):
        budgets = [int(b) for b in budgets_or_bpp]
        if len(budgets) != nb_gop:
            raise ValueError('%d budgets for the %d units of the video' % (len(budgets), nb_gop))
    else:
        budgets = layout_budgets(float(budgets_or_bpp), w, h, layout)
    grid = rate_grid(nb_rates_of(frame_codec), step)
    mine = [u for u in range(nb_gop) if unit_filter is None or unit_filter(u)]
    every = layout.units(frames)
    units = [every[u] for u in mine]
    names = gop_name if uniform else [layout.names[u] for u in mine]
    priced = {}  # (local unit, rate) -> the blob a probe priced

    def probe(pairs):
        # (the codec's running rate log -- estimated bits against bytes written -- speaks of the stream that is kept)
        log = {k: getattr(frame_codec, k) for k in ('estimated_bits', 'coded_payload_bytes') if hasattr(frame_codec, k)}
        blobs, _, _ = frame_codec.encode_units([units[k] for k, _ in pairs], gop_name if uniform else [names[k] for k, _ in pairs],
                                               idx_rate=[r for _, r in pairs], recon='refs')
        for k in ('estimated_bits', 'coded_payload_bytes'):
            if k in log:
                setattr(frame_codec, k, log[k])
            elif hasattr(frame_codec, k):
                delattr(frame_codec, k)
        priced.update(zip(pairs, blobs))
        return [len(b) for b in blobs]

    choices = search_rates(probe, len(mine), grid, [budgets[u] for u in mine])
    rates = [None] * nb_gop
    for u, ch in zip(mine, choices):
        rates[u] = ch.rate
    enc = frame_codec.encode_video(frames, gop_name, idx_starting_frame=idx_starting_frame, idx_rate=rates,
                                   unit_filter=unit_filter, stats=stats, **({} if uniform else {'layout': layout}))
    for k, (u, ch) in enumerate(zip(mine, choices)):
        assert enc['gops'][u] == priced[(k, ch.rate)], 'unit %d: the final pass is not the stream its probe priced' % u
    full = [None] * nb_gop
    for u, ch in zip(mine, choices):
        full[u] = ch
    return dict(enc, rates=rates, choices=full, budgets=budgets)
