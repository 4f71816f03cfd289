"""Frame digests, the host side (aivc_amd/digests.py): the sidecar manifest `<bitstream>.md5`, the flags of the three command
lines, the decision function behind `--contract auto`, and the C ABI entry the digests come from (include/aivc_hip_digest.h:
bound and exported; the kernel itself is tests/test_gpu_digest.py's)."""
import ctypes
import hashlib
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def md5(s):
    return hashlib.md5(s).hexdigest()


ROWS = {7: (md5(b'y7'), md5(b'u7'), md5(b'v7')), 8: (md5(b'y8'), md5(b'u8'), md5(b'v8')), 10: (md5(b''), md5(b'u'), md5(b'v'))}


# ---- manifest ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('contract', ['fp32', 'fp32w', 'bf16x3'])
def test_manifest_round_trip(tmp_path, contract):
    from aivc_amd import digests
    path = str(tmp_path / 'bits.bin.md5')
    digests.write_manifest(path, contract, ROWS)
    text = open(path).read()
    lines = text.split('\n')
    assert lines[0] == '# aivc-frame-digests 1 contract=%s md5=raw' % contract
    assert lines[1] == '7 %s %s %s' % ROWS[7] and text.endswith('\n') and len(lines) == 5  # header, 3 frames, final newline
    assert [int(l.split()[0]) for l in lines[1:4]] == [7, 8, 10]  # ascending, whatever the dictionary's order
    m = digests.read_manifest(path)
    assert m.contract == contract and m.rows == ROWS
    assert digests.compare(m.rows, ROWS) == []
    assert digests.manifest_path('a/b.bin') == 'a/b.bin.md5'


def test_manifest_of_no_frames(tmp_path):
    from aivc_amd import digests
    path = str(tmp_path / 'empty.md5')
    digests.write_manifest(path, 'fp32w', {})
    assert digests.read_manifest(path) == digests.Manifest('fp32w', {})


@pytest.mark.parametrize('line_no,replacement,what', [
    (2, '8 %s %s' % (md5(b'a'), md5(b'b')), 'three digests'),
    (2, '8 %s %s %s' % (md5(b'a'), md5(b'b'), md5(b'c')[:-1]), 'a short digest'),
    (2, '8 %s %s %s' % (md5(b'a'), md5(b'b'), md5(b'c').upper()), 'upper case'),
    (3, 'x %s %s %s' % ROWS[10], 'an index that is no number'),
    (3, '7 %s %s %s' % ROWS[10], 'an index that does not ascend'),
    (2, '', 'an empty line inside'),
    (1, '# aivc-frame-digests 1 contract=fp16 md5=raw', 'an unknown contract'),
    (1, '# aivc-frame-digests 2 contract=fp32 md5=raw', 'an unknown version'),
    (1, '# aivc-frame-digests 1 contract=fp32 md5=png', 'an unknown digest kind'),
    (1, '7 %s %s %s' % ROWS[7], 'no header'),
])
def test_malformed_manifest_names_file_and_line(tmp_path, line_no, replacement, what):
    from aivc_amd import digests
    path = str(tmp_path / 'bad.md5')
    digests.write_manifest(path, 'fp32', ROWS)
    lines = open(path).read().split('\n')
    lines[line_no - 1] = replacement
    with open(path, 'w') as f:
        f.write('\n'.join(lines))
    with pytest.raises(digests.ManifestError) as e:
        digests.read_manifest(path)
    assert path in str(e.value) and 'line %d' % line_no in str(e.value), what


def test_write_manifest_refuses_what_it_could_not_read_back(tmp_path):
    from aivc_amd import digests
    with pytest.raises(digests.ManifestError):
        digests.write_manifest(str(tmp_path / 'a.md5'), 'fp16', ROWS)
    with pytest.raises(digests.ManifestError):
        digests.write_manifest(str(tmp_path / 'a.md5'), 'fp32', {0: ('00', md5(b''), md5(b''))})


def test_compare_names_the_planes():
    from aivc_amd import digests
    found = dict(ROWS)
    found[8] = (ROWS[8][0], md5(b'other'), ROWS[8][2])
    assert digests.compare(ROWS, found) == ['8_u']
    del found[10]
    found[11] = ROWS[10]
    assert digests.compare(ROWS, found) == ['8_u', '10_y', '10_u', '10_v', '11_y', '11_u', '11_v']
    assert digests.verify_lines(3, []) == ['[VERIFY] 3 frames, 0 planes differ']
    many = ['%d_y' % i for i in range(12)]
    out = digests.verify_lines(12, many)
    assert out[0] == '[VERIFY] 12 frames, 12 planes differ' and out[1].split()[:8] == many[:8] and '8_y' not in out[1]


def test_hex_rows_is_hashlib_hex():
    import numpy as np
    from aivc_amd import digests
    d = [np.frombuffer(hashlib.md5(b'%d' % i).digest() + hashlib.md5(b'x%d' % i).digest(), np.uint8).reshape(2, 16) for i in range(3)]
    rows = digests.hex_rows(5, d)
    assert rows == {5: (md5(b'0'), md5(b'1'), md5(b'2')), 6: (md5(b'x0'), md5(b'x1'), md5(b'x2'))}


# ---- the decision behind --contract auto ------------------------------------------------------------------------------------
def _probe(errors, calls):
    def probe(name):
        calls.append(name)
        return errors[name]
    return probe


def test_choice_manifest_wins():
    from aivc_amd import digests
    calls = []
    choice, reason, note = digests.choose_contract('fp32', 'fp32w', _probe({}, calls), world=1)
    assert (choice, reason) == ('fp32', 'manifest') and calls == [] and 'fp32' in note
    assert digests.choose_contract('bf16x3', 'fp32w', _probe({}, calls), world=4)[:2] == ('bf16x3', 'manifest') and calls == []


def test_choice_default_clean():
    from aivc_amd import digests
    calls = []
    choice, reason, note = digests.choose_contract(None, 'fp32w', _probe({'fp32w': 0, 'fp32': 5}, calls))
    assert (choice, reason) == ('fp32w', 'default-clean') and calls == ['fp32w']  # (no second decode)
    assert 'without a manifest' in note and 'entropy stage' in note


@pytest.mark.parametrize('default,other', [('fp32w', 'fp32'), ('fp32', 'fp32w')])
def test_choice_default_dirty_other_clean(default, other):
    from aivc_amd import digests
    calls = []
    choice, reason, note = digests.choose_contract(None, default, _probe({default: 2, other: 0}, calls))
    assert (choice, reason) == (other, 'detected') and calls == [default, other]
    assert note == '[INFO] arithmetic contract: %s (detected on unit 0)' % other


def test_choice_both_dirty_stays_on_the_default():
    from aivc_amd import digests
    calls = []
    choice, reason, note = digests.choose_contract(None, 'fp32w', _probe({'fp32w': 2, 'fp32': 1}, calls))
    assert (choice, reason, note) == ('fp32w', 'undetected', None) and calls == ['fp32w', 'fp32']


def test_choice_multi_rank_makes_no_trial_decode():
    from aivc_amd import digests
    calls = []
    choice, reason, note = digests.choose_contract(None, 'fp32w', _probe({}, calls), world=2)
    assert (choice, reason) == ('fp32w', 'multi-rank') and calls == [] and '2 ranks' in note


# ---- command lines -------------------------------------------------------------------------------------------------------
def test_encode_flags():
    from aivc_amd import encode as enc_cli
    a = enc_cli.parse_args([])
    assert a.digests is False and a.contract is None
    a = enc_cli.parse_args(['--digests', '--contract', 'fp32'])
    assert a.digests is True and a.contract == 'fp32'
    assert enc_cli.parse_args(['--contract', 'fp32w']).contract == 'fp32w'
    with pytest.raises(SystemExit):
        enc_cli.parse_args(['--contract', 'auto'])  # (an encoder has nothing to detect)
    with pytest.raises(SystemExit):
        enc_cli.parse_args(['--contract', 'bf16x3'])


def test_decode_flags():
    from aivc_amd import decode as dec_cli
    a = dec_cli.parse_args([])
    assert a.verify == '' and a.contract is None
    assert dec_cli.parse_args(['--verify']).verify is True
    assert dec_cli.parse_args(['--verify', 'm.md5', '-i', 'b.bin']).verify == 'm.md5'
    assert dec_cli.parse_args(['--verify', '-i', 'b.bin']).verify is True
    for c in ('fp32', 'fp32w', 'auto'):
        assert dec_cli.parse_args(['--contract', c]).contract == c
    with pytest.raises(SystemExit):
        dec_cli.parse_args(['--contract', 'bf16x3'])


def test_aivc_flags_reach_both_halves(monkeypatch):
    from aivc_amd import aivc as cli
    a = cli.parse_args([])
    assert a.digests is False and a.verify == '' and a.contract is None
    seen = {}
    monkeypatch.setattr(cli.enc_cli, 'main', lambda argv: seen.__setitem__('enc', argv))
    monkeypatch.setattr(cli.dec_cli, 'main', lambda argv: seen.__setitem__('dec', argv) or 4)
    monkeypatch.setattr(cli.eval_cli, 'main', lambda argv: None)
    assert cli.main(['-i', 'clip_8x8_1_420.yuv']) == 4
    for half in ('enc', 'dec'):
        assert not {'--digests', '--verify', '--contract'} & set(seen[half])  # unset: the command lines of before
    assert cli.main(['-i', 'clip_8x8_1_420.yuv', '--digests', '--contract', 'fp32']) == 4
    assert '--digests' in seen['enc'] and seen['enc'][seen['enc'].index('--contract') + 1] == 'fp32'
    assert seen['dec'][-3:] == ['--verify', '--contract', 'fp32']  # --digests verifies its own decode
    cli.main(['-i', 'clip_8x8_1_420.yuv', '--verify', 'm.md5', '--contract', 'auto'])
    assert '--contract' not in seen['enc'] and '--digests' not in seen['enc']  # (auto is the decoder's choice)
    assert seen['dec'][-4:] == ['--verify', 'm.md5', '--contract', 'auto']


def test_exit_status_precedence(monkeypatch):
    from aivc_amd import decode as dec_cli
    from aivc_amd.real_life import decode as rdec
    for errors, differing, status in ((0, 0, 0), (0, 2, 4), (1, 0, 3), (1, 2, 3)):
        monkeypatch.setattr(rdec, 'stream_error_count', lambda e=errors: e)
        monkeypatch.setattr(rdec, 'verify_mismatch_count', lambda d=differing: d)
        assert dec_cli.exit_status() == status


def test_contract_flag_scope():
    """a named contract is ops.set_precision for the run and the previous one afterwards; unset (and auto, which the decoder
    library resolves) leaves aivc_amd.ops untouched"""
    from aivc_amd import ops
    from aivc_amd.cli_common import contract_scope
    before = ops.PRECISION
    calls = []
    real = ops.set_precision
    try:
        ops.set_precision = lambda name: calls.append(name) or real(name)
        for unset in (None, 'auto'):
            with contract_scope(unset):
                assert ops.PRECISION == before
        assert calls == []
        other = 'fp32' if ops.precision_name() == 'fp32w' else 'fp32w'
        with contract_scope(other):
            assert ops.precision_name() == other
        assert ops.PRECISION == before and calls[0] == other
        with pytest.raises(RuntimeError):
            with contract_scope(other):
                raise RuntimeError('the run failed')
        assert ops.PRECISION == before
    finally:
        ops.set_precision = real


def test_encode_main_passes_digests_and_restores_precision(monkeypatch):
    from aivc_amd import encode as enc_cli
    from aivc_amd import ops
    seen = {}

    class Model:
        pass
    monkeypatch.setattr(enc_cli, 'resolve_device', lambda cpu: 'cuda:0')
    monkeypatch.setattr(enc_cli, 'get_model', lambda name, dev: Model())
    monkeypatch.setattr(enc_cli, 'encode', lambda param: seen.update(param, precision=ops.precision_name()))
    before = ops.PRECISION
    enc_cli.main(['-i', 'clip_8x8_1_420.yuv'])
    assert seen['digests'] is False and ops._CONTRACT_NAMES[seen['precision']] == before
    enc_cli.main(['-i', 'clip_8x8_1_420.yuv', '--digests', '--contract', 'fp32'])
    assert seen['digests'] is True and seen['precision'] == 'fp32' and ops.PRECISION == before


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_abi_binds_and_library_exports_md5_batch():
    from aivc_amd import abi
    assert abi.ABI_VERSION >= 23 and set(abi.DIGEST_PROTOTYPES) == {'aivc_md5_batch'}
    lib_path = os.path.join(ROOT, 'aivc_amd', 'lib', 'libaivc_hip.so')
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build_hip()
    lib = ctypes.CDLL(lib_path)  # loads without a GPU (no compute call is made)
    assert hasattr(lib, 'aivc_md5_batch')
    lib.aivc_abi_version.restype = ctypes.c_int
    assert lib.aivc_abi_version() == abi.ABI_VERSION
    header = open(os.path.join(ROOT, 'include', 'aivc_hip_digest.h')).read()
    assert 'int aivc_md5_batch(' in header
    assert not set(abi.DIGEST_PROTOTYPES) & set(abi.PROTOTYPES)  # device only: the oracle has no `_ref` twin


def test_md5_batch_argument_errors_without_gpu():
    """error paths return codes before anything is launched (stand-in pointers are never read through)"""
    from aivc_amd import _lib
    md5_batch = _lib.load()['aivc_md5_batch']
    assert md5_batch(None, 0, 0, None, None) == 0  # n == 0 does nothing
    assert md5_batch(None, -5, 0, None, None) == 0
    assert md5_batch(16, 4, -1, 16, None) == -1
    assert md5_batch(None, 4, 1, 16, None) == -1 and md5_batch(16, 4, 1, None, None) == -1
    assert md5_batch(16, -1, 1, 16, None) == -1
    assert md5_batch(16, 1 << 31, 1, 16, None) == -1 and md5_batch(16, 1 << 40, 1, 16, None) == -1


def test_md5_planes_rejects_cpu_tensors():
    import torch
    from aivc_amd import ops
    from aivc_amd._lib import AivcNativeError
    with pytest.raises(AivcNativeError):
        ops.md5_planes(torch.zeros(2, 8, dtype=torch.uint8))
    with pytest.raises(AivcNativeError):
        ops.md5_planes([torch.zeros(8, dtype=torch.uint8)])
