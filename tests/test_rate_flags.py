"""The host side of choosing a rate index: the command-line flags, the check of a per-unit rate list, the ABI of the gain-row
entry points (include/aivc_hip_rates.h).  No device: nothing here launches a kernel."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'aivc_channel_gain_rows', 'aivc_quantize_center_rows', 'aivc_dequantize_rows'}


@pytest.mark.parametrize('cli', ['encode', 'aivc'])
def test_cli_parses_idx_rate_and_refuses_it_with_target_bpp(cli, capsys):
    import importlib
    mod = importlib.import_module('aivc_amd.' + cli)
    a = mod.parse_args(['--idx_rate', '1.25'])
    assert a.idx_rate == 1.25 and a.target_bpp == 0 and a.rate_step == 0.0625
    a = mod.parse_args(['--target_bpp', '0.4', '--rate_step', '0.25'])
    assert a.target_bpp == 0.4 and a.rate_step == 0.25
    assert mod.parse_args([]).target_bpp == 0
    for bad in (['--idx_rate', '1.25', '--target_bpp', '0.4'], ['--idx_rate', '0', '--target_bpp', '0.4'],
                ['--idx_rate', '0.3'], ['--idx_rate', '-0.0625'], ['--rate_step', '0.1'], ['--target_bpp', '-1']):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(bad)
        assert e.value.code == 2  # argparse's error exit
        assert 'error:' in capsys.readouterr().err


def test_encode_cli_default_is_rate_zero_and_passes_the_flags_on():
    from aivc_amd import encode as enc_cli
    assert enc_cli.parse_args([]).idx_rate == 0  # today's behaviour
    seen = {}
    real = (enc_cli.encode, enc_cli.get_model, enc_cli.resolve_device)
    enc_cli.encode, enc_cli.get_model, enc_cli.resolve_device = seen.update, (lambda name, dev: None), (lambda cpu: None)
    try:
        enc_cli.main(['-i', 'x_8x8_1_420.yuv', '--gop', '1_GOP_2'])
        assert seen['idx_rate'] == 0 and seen['target_bpp'] == 0
        enc_cli.main(['-i', 'x_8x8_1_420.yuv', '--gop', '1_GOP_2', '--target_bpp', '0.5', '--rate_step', '0.5'])
        assert seen['idx_rate'] == 0 and seen['target_bpp'] == 0.5 and seen['rate_step'] == 0.5
    finally:
        enc_cli.encode, enc_cli.get_model, enc_cli.resolve_device = real


def test_unit_rate_list_validation():
    from aivc_amd import rate_control as rc
    nb_rates = 3
    assert rc.check_unit_rates([0, 0.5, 1.25, 2, 2.0, 1 / 16], nb_rates) == [0.0, 0.5, 1.25, 2.0, 2.0, 0.0625]
    for bad in (0.3, -1 / 16, nb_rates - 1 + 1 / 16):
        with pytest.raises(ValueError, match='unit 1'):
            rc.check_unit_rates([0.5, bad, 1.0], nb_rates)
        with pytest.raises(ValueError, match='unit 7'):  # named by its number in the video
            rc.check_unit_rates([0.5, bad], nb_rates, [4, 7])
    with pytest.raises(ValueError, match='unit 0'):
        rc.check_unit_rates([None], nb_rates)
    assert rc.is_rate_list([0.5]) and rc.is_rate_list((0.5, 1)) and not rc.is_rate_list(0.5) and not rc.is_rate_list(0)


def rates_header_functions():
    src = open(os.path.join(ROOT, 'include', 'aivc_hip_rates.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return set(re.findall(r'\bint\s+(aivc_\w+)\s*\(', src))


def test_abi_names_exactly_the_three_new_symbols_and_the_library_exports_them():
    from aivc_amd import abi
    assert abi.ABI_VERSION >= 21
    assert set(abi.RATES_PROTOTYPES) == NEW == rates_header_functions()
    assert not NEW & set(abi.PROTOTYPES)  # the main header (and its `_ref` twins in the oracle) is unchanged
    assert 'aivc_hip_rates' not in open(os.path.join(ROOT, 'include', 'aivc_hip.h')).read()
    lib_path = os.path.join(ROOT, 'aivc_amd', 'lib', 'libaivc_hip.so')
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build_hip()
    lib = ctypes.CDLL(lib_path)  # loads without a GPU (no compute call is made)
    for n in NEW:
        assert hasattr(lib, n), 'libaivc_hip.so does not export %s' % n
    lib.aivc_abi_version.restype = ctypes.c_int
    assert lib.aivc_abi_version() == abi.ABI_VERSION


def test_argument_checks_return_codes_without_a_launch():
    """n <= 0, c <= 0 or a NULL required pointer: AIVC_ERR_ARG; n > 65535 (the image is blockIdx.y): AIVC_ERR_UNSUPPORTED.
    The pointers are never dereferenced on these paths (no device is needed)."""
    from aivc_amd import _lib
    fns = _lib.load()
    p = 4096  # any non-NULL address: the argument checks come first
    gain, quant, deq = fns['aivc_channel_gain_rows'], fns['aivc_quantize_center_rows'], fns['aivc_dequantize_rows']
    assert gain(None, p, 2, 4, 8, p, None) == -1 and gain(p, p, 2, 4, 8, None, None) == -1
    assert gain(p, p, 0, 4, 8, p, None) == -1 and gain(p, p, -1, 4, 8, p, None) == -1 and gain(p, p, 2, 4, 0, p, None) == -1
    assert gain(p, p, 65536, 4, 8, p, None) == -2
    assert quant(None, p, p, 2, 4, 8, p, p, None) == -1 and quant(p, p, p, 2, 4, 8, None, None, None) == -1
    assert quant(p, p, p, 0, 4, 8, p, p, None) == -1 and quant(p, p, p, 2, 4, -3, p, p, None) == -1
    assert quant(p, None, None, 70000, 4, 8, p, None, None) == -2
    assert deq(None, p, p, 2, 4, 8, p, None) == -1 and deq(p, p, p, 2, 4, 8, None, None) == -1
    assert deq(p, p, p, 0, 4, 8, p, None) == -1 and deq(p, p, p, 2, 4, 0, p, None) == -1
    assert deq(p, None, None, 65536, 4, 8, p, None) == -2
    assert gain(p, None, 3, 0, 8, p, None) == 0  # no positions: nothing to launch
