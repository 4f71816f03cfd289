"""The options of the three command lines, pinned: what each parser declares (A), what aivc.py hands to the encoder, the decoder
and the evaluation (B), and the two records that carry them through the library (C).  A and B compare with
tests/golden/cli_options.json, which `python tests/test_cli_options.py` records with the helpers below (the file names the commit
it was recorded at); they ran unchanged in front of and behind the change that introduced aivc_amd/options.py.  No GPU."""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'cli_options.json')
CLIP, PICS = 'clip_8x8_25_420.yuv', 'pics'
FOLDERS = ['-i', PICS, '-o', 'out/']
CASES = {  # name -> what follows `aivc.py -i clip_8x8_25_420.yuv` (a later -i / -o wins)
    'plain': [],
    'idx_rate': ['--idx_rate', '1.25'],
    'target_bpp': ['--target_bpp', '0.4', '--rate_step', '0.25'],
    'scene_cut': ['--scene_cut', '3'],
    'digests': ['--digests'],
    'verify': ['--verify', 'm.md5'],
    'contract_fp32w': ['--contract', 'fp32w'],
    'contract_auto': ['--contract', 'auto'],
    'size': ['--size', '16x12', '--resample', 'box'],
    'out_size': ['--out_size', '16x12'],
    'both_sizes': ['--size', '16x12', '--out_size', '8x8', '--resample', 'lanczos'],
    'raw_formats': ['-o', 'o.y4m', '--pix_fmt', 'yuv420p', '--out_pix_fmt', 'gray', '--fps', '30000:1001'],
    'png_device': FOLDERS + ['--png_reader', 'device', '--png_coder', 'device'],
    'colour': FOLDERS + ['--matrix', 'bt709', '--range', 'full', '--chroma_down', 'box'],
    'own_flags': ['--log_dir', 'logs', '--model', 'm', '--rng_seed', '5', '--start_frame', '1', '--end_frame', '2'],
    'ldp': ['--coding_config', 'LDP', '--intra_period', '8'],
}


def clis():
    from aivc_amd import aivc, decode, encode
    return {'encode': encode, 'decode': decode, 'aivc': aivc}


def plain(x):
    """as JSON holds it: tuples (a ColourSpec, a size, a frame rate) become lists"""
    return json.loads(json.dumps(x))


class _Captured(Exception):
    pass


def parser_table(cli):
    """{flag: [default, choices, nargs, const, metavar, type name, help]} of every action of cli.parse_args' parser"""
    def stop(self, *args, **kw):
        raise _Captured(self)
    with pytest.MonkeyPatch.context() as mp, pytest.raises(_Captured) as e:
        mp.setattr(argparse.ArgumentParser, 'parse_args', stop)
        cli.parse_args([])
    return plain({'/'.join(a.option_strings): [a.default, None if a.choices is None else list(a.choices), a.nargs, a.const, a.metavar,
                                               getattr(a.type, '__name__', None), a.help] for a in e.value.args[0]._actions})


def options_of(a):
    """vars() of a parsed command line; the records a.source / a.sink restate flat entries and are compared in part C"""
    return plain({k: v for k, v in vars(a).items() if k not in ('source', 'sink')})


def forwarded(argv):
    """aivc.main(argv) with the three commands it runs replaced by recorders -> what the encoder and the decoder make of their
    argument lists, and the evaluation's list as it is (None: not run)"""
    from aivc_amd import aivc
    got = {'encode': None, 'decode': None, 'evaluate': None}

    def recorder(name):
        def main(args):
            got[name] = list(args)
            return 0
        return main
    with pytest.MonkeyPatch.context() as mp, contextlib.redirect_stdout(io.StringIO()):
        for name, cli in (('encode', aivc.enc_cli), ('decode', aivc.dec_cli), ('evaluate', aivc.eval_cli)):
            mp.setattr(cli, 'main', recorder(name))
        assert aivc.main(['-i', CLIP] + argv) == 0
    return {'encode': options_of(aivc.enc_cli.parse_args(got['encode'])), 'decode': options_of(aivc.dec_cli.parse_args(got['decode'])),
            'evaluate': got['evaluate']}


def make_clip_dir(tmp):
    """the working directory of the cases: three 8 x 8 frames, and a folder holding one 4 x 4 RGB picture"""
    from PIL import Image
    with open(os.path.join(tmp, CLIP), 'wb') as f:
        f.write(bytes(96 * 3))
    os.makedirs(os.path.join(tmp, PICS))
    Image.fromarray(np.zeros((4, 4, 3), np.uint8), 'RGB').save(os.path.join(tmp, PICS, '0.png'))


@pytest.fixture
def clip_dir(tmp_path, monkeypatch):
    make_clip_dir(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    return tmp_path


@pytest.fixture(scope='module')
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- A: the options are what they were -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['encode', 'decode', 'aivc'])
def test_parser_declares_what_it_declared(name, recorded):
    got, want = parser_table(clis()[name]), recorded['parsers'][name]
    assert sorted(got) == sorted(want)
    for flag in want:
        assert got[flag] == want[flag], flag


# ---- B: forwarding ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(CASES))
def test_aivc_forwards_what_it_forwarded(case, recorded, clip_dir):
    got, want = forwarded(CASES[case]), recorded['forwarded'][case]
    for half in ('encode', 'decode'):
        assert sorted(got[half]) == sorted(want[half]), half
        for key in want[half]:
            assert got[half][key] == want[half][key], (half, key)
    assert got['evaluate'] == want['evaluate']


# ---- C: the records ----------------------------------------------------------------------------------------------------------------
def test_records_hold_the_defaults_and_read_param_dictionaries():
    from aivc_amd.color import ColourSpec
    from aivc_amd.options import Sink, Source
    assert Source()._asdict() == {'pix_fmt': None, 'png_reader': 'pillow', 'colour': None, 'chroma_down': 'point', 'size': None,
                                  'resample': 'bicubic'}
    assert Sink()._asdict() == {'out_size': None, 'resample': 'bicubic', 'out_pix_fmt': 'yuv420p', 'fps': (25, 1), 'png_coder': 'pillow',
                                'colour': None}
    for record in (Source, Sink):
        assert record.from_param({}) == record() == record.from_param(dict.fromkeys(record._fields))  # (a None entry is an absent one)
        with pytest.raises(AttributeError):
            record().resample = 'box'
    full = Source('nv12', 'device', ColourSpec('bt709', 'full'), 'box', (16, 12), 'lanczos')
    assert Source.from_param(dict(full._asdict(), model=None, sequence_path='x')) == full
    full = Sink((16, 12), 'box', 'gray', (30000, 1001), 'device', ColourSpec('bt2020'))
    assert Sink.from_param(dict(full._asdict(), decoder=None, verify=True)) == full


def test_options_import_without_torch():
    import subprocess
    code = 'import sys; import aivc_amd.options; assert "torch" not in sys.modules, "aivc_amd.options imported torch"'
    subprocess.run([sys.executable, '-c', code], cwd=ROOT, check=True)


def refused(check, *args, word):
    with pytest.raises(ValueError) as e:
        check(*args)
    assert word in str(e.value)


def test_source_check_is_the_rules_of_an_input(clip_dir):
    from aivc_amd.color import ColourSpec
    from aivc_amd.options import Source
    spec = ColourSpec('bt709')
    os.makedirs('triplets')
    open(os.path.join('triplets', '0_y.png'), 'wb').close()
    for path in (CLIP, PICS, 'triplets', 'not-there.yuv'):
        Source().check(path)
    Source(png_reader='device').check(PICS)
    for path in (CLIP, 'not-there'):
        refused(Source(png_reader='device').check, path, word='--png_reader device')
    refused(Source(png_reader='zlib').check, PICS, word='png reader')
    Source(colour=spec).check(PICS)
    Source(colour=('bt709', 'full'), chroma_down='box').check(PICS)
    for path in (CLIP, 'triplets', 'not-there.yuv'):
        refused(Source(colour=spec).check, path, word='is not a folder of RGB pictures')
    refused(Source(colour=('bt470', 'full')).check, PICS, word='colour matrix')
    refused(Source(chroma_down='box').check, PICS, word='--chroma_down box needs --matrix')
    Source(size=(16, 12), resample='box').check(CLIP)
    Source(size=(16, 12)).check(CLIP)
    refused(Source(resample='box').check, CLIP, word='--resample box: needs --size')


def test_sink_check_is_the_rules_of_an_output(tmp_path):
    from aivc_amd.color import ColourSpec
    from aivc_amd.options import Sink
    folder, existing, yuv, y4m = str(tmp_path / 'new') + '/', str(tmp_path), str(tmp_path / 'out.yuv'), str(tmp_path / 'out.y4m')
    for out in (folder, existing, yuv, y4m, ''):
        Sink().check(out)
    for out in (folder, existing):
        Sink(png_coder='device', colour=ColourSpec('bt601', 'full'), out_size=(16, 12)).check(out)
        refused(Sink(out_size=(15, 12)).check, out, word='even sides')
        refused(Sink(out_size=(16, 11)).check, out, word='even sides')
        Sink(out_size=(15, 11)).check(out, odd_pictures=True)  # (the library writes what it is asked to)
        Sink(out_pix_fmt='p010le').check(out)  # (no file is written: the layout is not looked at further)
    for out in (yuv, y4m):
        Sink(out_size=(15, 11), resample='hamming').check(out)
        refused(Sink(png_coder='device').check, out, word='--png_coder device')
        refused(Sink(colour=ColourSpec('bt709')).check, out, word='is a raw video file')
    refused(Sink(png_coder='zlib').check, folder, word='png coder')
    Sink(out_pix_fmt='nv12').check(yuv)
    Sink(out_pix_fmt='gray10le').check(y4m)
    for fmt in ('nv12', 'p010le'):
        refused(Sink(out_pix_fmt=fmt).check, y4m, word='.y4m')
    refused(Sink(out_pix_fmt='yuv444p').check, yuv, word='is not written')
    refused(Sink(resample='lanczos').check, yuv, word='--resample lanczos: needs --out_size')


def test_parsed_records_restate_the_flat_entries(clip_dir):
    """a.source / a.sink are the flat entries under the same names; a half that resizes nothing keeps the default filter"""
    from aivc_amd import aivc, decode, encode
    from aivc_amd.options import Sink, Source
    a = encode.parse_args(['-i', PICS, '--matrix', 'bt709', '--chroma_down', 'box', '--size', '16x12', '--resample', 'box', '--png_reader', 'device'])
    assert a.source == Source(None, 'device', ('bt709', 'limited'), 'box', (16, 12), 'box') == Source(**{k: getattr(a, k) for k in Source._fields})
    a = decode.parse_args(['-o', 'o.y4m', '--out_pix_fmt', 'gray', '--fps', '50', '--out_size', '15x11'])
    assert a.sink == Sink((15, 11), 'bicubic', 'gray', (50, 1), 'pillow', None) == Sink(**{k: getattr(a, k) for k in Sink._fields})
    assert not hasattr(a, 'source') and not hasattr(encode.parse_args(['-i', CLIP]), 'sink')
    a = aivc.parse_args(['-i', CLIP, '--out_size', '16x12', '--resample', 'box'])
    assert a.resample == 'box' and a.sink == Sink(out_size=(16, 12), resample='box') and a.source == Source()


def record():
    """writes tests/golden/cli_options.json from the code as it stands"""
    import subprocess
    import tempfile
    out = {'recorded_at': subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=ROOT, text=True).strip(),
           'parsers': {name: parser_table(cli) for name, cli in clis().items()}, 'forwarded': {}}
    with tempfile.TemporaryDirectory() as tmp, pytest.MonkeyPatch.context() as mp:
        make_clip_dir(tmp)
        mp.chdir(tmp)
        for case, argv in CASES.items():
            out['forwarded'][case] = forwarded(argv)
    with open(GOLDEN, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    record()
