"""The host half of the device PNG reader, no GPU: png.parse on every file of png_read_cases.py, the --png_reader flag, the C ABI
without a launch, and the decoder core itself -- aivc_amd/csrc/inflate_core.h, the text the kernel runs -- compiled into the
stand-alone program tools/inflate_host.cpp under the host sanitizers and run over every valid and damaged stream."""
import ctypes
import inspect
import os
import shutil
import struct
import subprocess
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_cases as pcs  # noqa: E402
import png_read_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- parse ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(cases.FILES))
def test_parse_finds_size_and_idats(name):
    from PIL import Image
    import io
    from aivc_amd import png
    data, mode = cases.FILES[name]
    w, h, c, idats = png.parse(data)
    img = Image.open(io.BytesIO(data))
    assert (w, h) == img.size and c == (1 if mode == 'L' else 3) and img.mode == mode
    want = [d for k, d in pcs.chunks(data) if k == b'IDAT']
    assert [bytes(data[o:o + n]) for o, n in idats] == want
    assert len(zlib.decompress(b''.join(want))) == h * (1 + w * c)
    if name == 'rechunked':
        assert sorted({n for _, n in idats}) == [0, 1] and len(idats) > 50


@pytest.mark.parametrize('name', sorted(cases.OTHER_KINDS))
def test_parse_hands_other_kinds_to_pillow(name):
    from aivc_amd import png
    with pytest.raises(png.Unsupported):
        png.parse(cases.OTHER_KINDS[name][0])


@pytest.mark.parametrize('what', ['idat-crc', 'no-iend', 'no-idat', 'truncated-chunk', 'signature'])
def test_parse_names_what_is_wrong(what):
    from aivc_amd import png
    assert issubclass(png.PngError, ValueError) and not issubclass(png.Unsupported, png.PngError)
    with pytest.raises(png.PngError) as e:
        png.parse(cases.broken_files()[what])
    word = {'idat-crc': 'CRC', 'no-iend': 'IEND', 'no-idat': 'IDAT', 'truncated-chunk': 'truncated', 'signature': 'signature'}[what]
    assert word in str(e.value)


# ---- the flag ------------------------------------------------------------------------------------------------------------------------
def test_png_reader_flag(tmp_path, capsys):
    from aivc_amd import aivc as aivc_cli
    from aivc_amd import encode as enc_cli
    from aivc_amd import png
    assert png.READERS == ('pillow', 'device')
    folder, a_file = str(tmp_path), str(tmp_path / 'clip_64x48_30_420.yuv')
    open(a_file, 'wb').close()
    for cli in (enc_cli, aivc_cli):
        assert cli.parse_args(['-i', folder]).png_reader == 'pillow'
        assert cli.parse_args(['-i', a_file]).png_reader == 'pillow'
        assert cli.parse_args(['-i', folder, '--png_reader', 'pillow']).png_reader == 'pillow'
        assert cli.parse_args(['-i', a_file, '--png_reader', 'pillow']).png_reader == 'pillow'
        assert cli.parse_args(['-i', folder, '--png_reader', 'device']).png_reader == 'device'
        for argv in (['-i', folder, '--png_reader', 'zlib'], ['-i', a_file, '--png_reader', 'device'],
                     ['-i', str(tmp_path / 'nothing-here'), '--png_reader', 'device']):
            with pytest.raises(SystemExit) as e:
                cli.parse_args(argv)
            assert e.value.code == 2
            assert '--png_reader' in capsys.readouterr().err
    # --png_coder keeps its meaning: who WRITES
    a = aivc_cli.parse_args(['-i', folder, '-o', folder + '/', '--png_reader', 'device'])
    assert (a.png_reader, a.png_coder) == ('device', 'pillow')
    assert png.check_reader('device') == 'device' and png.check_reader('device', folder, True) == 'device'
    with pytest.raises(ValueError):
        png.check_reader('device', a_file, False)
    with pytest.raises(ValueError):
        png.check_reader('gpu')


def test_default_arguments_keep_the_pillow_path():
    from aivc_amd.func_util import img_processing
    from aivc_amd.real_life import encode
    assert inspect.signature(encode.read_png_folder).parameters['reader'].default == 'pillow'
    from aivc_amd.options import Source
    assert Source().png_reader == 'pillow'
    assert inspect.signature(img_processing.load_RGB_as_YUV420_dic).parameters['reader'].default == 'pillow'
    assert inspect.signature(img_processing.load_YUV_as_dic_tensor).parameters['reader'].default == 'pillow'
    with pytest.raises(ValueError):
        img_processing.load_frames({'sequence_path': '/nonexistent/never-made', 'png_reader': 'zlib'})
    with pytest.raises(ValueError):
        encode.read_png_folder('/nonexistent/never-made', reader='zlib')


# ---- the C entry points, no launch ---------------------------------------------------------------------------------------------------
def test_library_exports_and_abi():
    from aivc_amd import abi
    assert abi.ABI_VERSION == 26 and set(abi.PNG_READ_PROTOTYPES) == {'aivc_inflate', 'aivc_png_unfilter'}
    lib_path = os.path.join(ROOT, 'aivc_amd', 'lib', 'libaivc_hip.so')
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build_hip()
    lib = ctypes.CDLL(lib_path)  # loads without a GPU (no compute call is made)
    for name in abi.PNG_READ_PROTOTYPES:
        assert hasattr(lib, name), 'libaivc_hip.so does not export %s' % name
    lib.aivc_abi_version.restype = ctypes.c_int
    assert lib.aivc_abi_version() == abi.ABI_VERSION
    header = open(os.path.join(ROOT, 'include', 'aivc_hip_png_read.h')).read()
    assert all('int %s(' % name in header for name in abi.PNG_READ_PROTOTYPES)
    for value, words in abi.INFLATE_STATUS.items():  # every status is in the header, under its number
        assert any(line.startswith('#define AIVC_INFLATE_') and line.split()[2] == str(value) for line in header.splitlines()), words
    from aivc_amd import _lib
    fns = _lib.load()  # the loader binds them beside what abi.declare binds, each with its stream argument
    for name, args in abi.PNG_READ_PROTOTYPES.items():
        assert fns[name].argtypes == list(args) + [ctypes.c_void_p] and fns[name].restype is ctypes.c_int
    assert not set(abi.PNG_READ_PROTOTYPES) & (set(abi.declare(lib)) | set(abi.PNG_PROTOTYPES))


def test_argument_errors_without_a_launch():
    from aivc_amd import _lib
    fns = _lib.load()

    def inflate(src=16, table=16, n=1, max_src=100, max_dst=100, dst=16, info=16):
        return fns['aivc_inflate'](src, table, n, max_src, max_dst, dst, info, None)

    def unfilter(filt=16, table=16, n=1, max_bytes=100, pix=16, status=16):
        return fns['aivc_png_unfilter'](filt, table, n, max_bytes, pix, status, None)
    for kw in (dict(src=None), dict(table=None), dict(dst=None), dict(info=None), dict(n=0), dict(n=-1)):
        assert inflate(**kw) == -1, kw
    for kw in (dict(filt=None), dict(table=None), dict(pix=None), dict(status=None), dict(n=0), dict(n=-5)):
        assert unfilter(**kw) == -1, kw
    assert inflate(max_src=1 << 31) == -2 and inflate(max_dst=1 << 31) == -2 and inflate(max_dst=(1 << 40) + 5) == -2
    assert unfilter(max_bytes=1 << 31) == -2


# ---- the decoder core on the host ----------------------------------------------------------------------------------------------------
def _host_compiler():
    for name in (os.environ.get('CXX'), 'c++', 'g++', 'clang++'):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_inflate_core_under_the_host_sanitizers(tmp_path):
    """tools/inflate_host.cpp runs on its own: nothing is loaded into this process.  Valid streams must come out as zlib's bytes
    with status 0 and every source byte consumed; every damaged one with a status that is not 0, its destination untouched
    behind what it reports as produced; the sanitizers must have nothing to say (they end the program with another exit status at their first finding)."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'inflate_host')
    build = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
             os.path.join(ROOT, 'tools', 'inflate_host.cpp'), '-o', exe]
    # the runtimes inside the program where the compiler can (gcc's flags, clang's flag), so that it needs nothing of its environment
    for static in (['-static-libasan', '-static-libubsan'], ['-static-libsan'], []):
        if subprocess.run(build + static, capture_output=True).returncode == 0:
            break
    else:
        subprocess.run(build, check=True)
    todo = [(z, len(d)) for _, z, d in cases.VALID] + [(z, n) for _, z, n in cases.DAMAGED]
    with open(tmp_path / 'cases.bin', 'wb') as f:
        f.write(struct.pack('<I', len(todo)))
        for z, n in todo:
            f.write(struct.pack('<II', len(z), n) + z)
    run = subprocess.run([exe, str(tmp_path / 'cases.bin'), str(tmp_path / 'results.bin')], capture_output=True, text=True)
    assert run.returncode == 0 and 'Sanitizer' not in run.stderr and 'runtime error' not in run.stderr, run.stderr[-4000:]
    res = open(tmp_path / 'results.bin', 'rb').read()
    at = 0
    for k, (z, n) in enumerate(todo):
        status, produced, consumed = struct.unpack('<III', res[at:at + 12])
        got = res[at + 12:at + 12 + n]
        at += 12 + n
        if k < len(cases.VALID):
            name, _, want = cases.VALID[k]
            assert (status, produced, consumed) == (0, len(want), len(z)) and got == want, name
        else:
            name = cases.DAMAGED[k - len(cases.VALID)][0]
            assert status != 0 and produced <= n and got[produced:] == b'\xa5' * (n - produced), name
    assert at == len(res)
