"""Frame digests: the sidecar manifest `<bitstream>.md5` and the choice of the arithmetic contract a decoder runs in.  Host only:
the digests themselves come from the device (aivc_amd.ops.md5_planes, include/aivc_hip_digest.h).

The manifest is out of band, like flag_md5sum's sections and the `.debug/` folder of flag_bitstream_debug: the bitstream does not
change by one byte.  It is a text file:

    # aivc-frame-digests 1 contract=<fp32|fp32w|bf16x3> md5=raw
    <absolute frame index> <md5 y> <md5 u> <md5 v>
    ...

one line per real frame from idx_starting_frame to idx_end_frame, ascending (the padded repeats of the last frame are not listed);
the digests are MD5 of the raw 8-bit planes as 32 lower-case hexadecimal digits.  `contract` is the arithmetic contract the
encoder ran in (aivc_amd.ops.set_precision): what a decoder has to run in to reproduce the planes."""
import collections
import re

MAGIC = 'aivc-frame-digests'
VERSION = 1
CONTRACTS = ('fp32', 'fp32w', 'bf16x3')
FP32_CONTRACTS = ('fp32w', 'fp32')  # the two versions of the fp32 contract: what a trial decode can tell apart

Manifest = collections.namedtuple('Manifest', 'contract rows')  # rows: {absolute frame index: (md5 y, md5 u, md5 v)}

_HEX = re.compile(r'^[0-9a-f]{32}$')


class ManifestError(ValueError):
    pass


def manifest_path(bitstream_path):
    return bitstream_path + '.md5'


def hex_rows(first, digests_yuv):
    """three [n, 16] uint8 arrays (y, u, v digests of n consecutive frames) -> {first + i: (hex y, hex u, hex v)}"""
    y, u, v = digests_yuv
    return {first + i: (bytes(bytearray(y[i])).hex(), bytes(bytearray(u[i])).hex(), bytes(bytearray(v[i])).hex())
            for i in range(len(y))}


def write_manifest(path, contract, rows):
    """rows: {absolute frame index: (md5 y, md5 u, md5 v)} as hexadecimal strings"""
    if contract not in CONTRACTS:
        raise ManifestError('contract %r: expected one of %s' % (contract, ', '.join(CONTRACTS)))
    lines = ['# %s %d contract=%s md5=raw' % (MAGIC, VERSION, contract)]
    for idx in sorted(rows):
        y, u, v = rows[idx]
        for d in (y, u, v):
            if not _HEX.match(d):
                raise ManifestError('frame %d: %r is not an md5 digest' % (idx, d))
        lines.append('%d %s %s %s' % (idx, y, u, v))
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def read_manifest(path):
    """-> Manifest; ManifestError naming the file and the line for anything that is not of the format above"""
    with open(path) as f:
        lines = f.read().split('\n')

    def bad(i, why):
        return ManifestError('%s, line %d: %s: %r' % (path, i + 1, why, lines[i]))
    head = lines[0].split()
    if len(head) != 5 or head[0] != '#' or head[1] != MAGIC:
        raise bad(0, "expected '# %s %d contract=<name> md5=raw'" % (MAGIC, VERSION))
    if head[2] != str(VERSION):
        raise bad(0, 'manifest version %s, this reader knows %d' % (head[2], VERSION))
    if not head[3].startswith('contract=') or head[3][9:] not in CONTRACTS:
        raise bad(0, 'contract is none of %s' % ', '.join(CONTRACTS))
    if head[4] != 'md5=raw':
        raise bad(0, 'digest kind is not md5=raw')
    rows, prev = {}, None
    for i in range(1, len(lines)):
        if not lines[i] and i == len(lines) - 1:  # (the newline that ends the file)
            break
        tok = lines[i].split(' ')
        if len(tok) != 4 or not tok[0].isdigit() or not all(_HEX.match(t) for t in tok[1:]):
            raise bad(i, 'expected <frame index> <md5 y> <md5 u> <md5 v>')
        idx = int(tok[0])
        if prev is not None and idx <= prev:
            raise bad(i, 'frame indices do not ascend')
        rows[idx] = tuple(tok[1:])
        prev = idx
    return Manifest(head[3][9:], rows)


def compare(expected, found):
    """expected, found: {frame index: (md5 y, md5 u, md5 v)} -> the names '<idx>_<c>' of the planes that differ, ascending.  A frame
    that only one side lists counts with all three planes."""
    out = []
    for idx in sorted(set(expected) | set(found)):
        e, f = expected.get(idx), found.get(idx)
        for c, name in enumerate('yuv'):
            if e is None or f is None or e[c] != f[c]:
                out.append('%d_%s' % (idx, name))
    return out


def manifest_subset(rows, indices):
    """the manifest's rows of the frames a partial decode returned (compare() then counts exactly those; a returned frame the
    manifest does not list has no row here and differs with all three planes)"""
    return {i: rows[i] for i in indices if i in rows}


def verify_lines(n_frames, differing):
    """what a decoder prints about a comparison"""
    lines = ['[VERIFY] %d frames, %d planes differ' % (n_frames, len(differing))]
    if differing:
        lines.append('\t' + ' '.join(differing[:8]) + (' ...' if len(differing) > 8 else ''))
    return lines


def other_contracts(default):
    return [c for c in FP32_CONTRACTS if c != default]


def choose_contract(manifest_contract, default, probe, world=1):
    """`--contract auto` of the decoders as a pure function -> (contract, reason, message to print or None).
    manifest_contract: the manifest's, or None without a manifest.  default: what the process runs in.
    probe(name) -> number of sections of unit 0 that did not decode to where their payload ends under contract `name` (the
    always-on bit-count identity, real_life/decode.py: report_stream_errors); only called without a manifest in a single process.
    reason is one of 'manifest', 'default-clean', 'detected', 'undetected', 'multi-rank'."""
    if manifest_contract is not None:
        return manifest_contract, 'manifest', '[INFO] arithmetic contract: %s (from the manifest)' % manifest_contract
    if world > 1:
        return default, 'multi-rank', ('[INFO] arithmetic contract: %s (the default: without a manifest, a job of %d ranks makes '
                                       'no trial decode)' % (default, world))
    if probe(default) == 0:
        return default, 'default-clean', ('[INFO] arithmetic contract: %s (the default decodes unit 0 cleanly; a stream without a '
                                          'manifest can be told apart only where its entropy stage depends on the contract)'
                                          % default)
    for name in other_contracts(default):
        if probe(name) == 0:
            return name, 'detected', '[INFO] arithmetic contract: %s (detected on unit 0)' % name
    return default, 'undetected', None  # (both leave errors: the normal report and exit status say so)
