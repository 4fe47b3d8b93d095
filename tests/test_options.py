"""The option table and the scan-mode table of csrc/aae_options.h against tests/golden/option_rules.json, which was recorded from
the commit before the tables existed (tests/golden/make_option_rules.cpp): tests/native/options_host.cpp, a program of that
header alone, replays every recorded call in the product and in the experiments build; what aae_encoder_set_option adds for the
handle, and the upright copies of a codebook, are checked on the emulator library; the documented names are the table's names."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest

import emu_backend as eb
from augmentedautoencoder_amd.weights import EncoderConfig
from oracle import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SECTIONS = {'product': [], 'experiments': ['-DAAE_EXPERIMENTS']}
# aae_encoder_set_option looks at the handle or the runtime for these before the table is asked
HANDLE_OPTIONS = ('detect_chain', 'chain_timeline', 'wavek_timeline', 'winograd', 'precision')
# ... and for a default-config encoder that changes one recorded answer: the product library refuses the per-component Winograd
# launches, a value the table's range accepts (test_gpu_options.py checks the answer on the library itself)
HANDLE_ANSWERS = {('product', 'winograd', 2)}


def _compiler():
    for c in ('g++', '/opt/rocm/lib/llvm/bin/clang++', 'clang++'):
        path = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if path:
            return path
    raise RuntimeError('no host C++ compiler (g++ or clang++) found')


def _build(out_dir, flags, name):
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-O2', '-Wall', '-Wextra', '-Werror'] + flags + [os.path.join(HERE, 'native', 'options_host.cpp'), '-o', exe])
    return exe


@pytest.fixture(scope='module')
def rules():
    with open(os.path.join(HERE, 'golden', 'option_rules.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def host_exes(tmp_path_factory):
    out = tmp_path_factory.mktemp('options_host')
    return {section: _build(out, flags, 'options_host_' + section) for section, flags in SECTIONS.items()}


def _replay(exe, calls):
    """[(name, value)] -> [(rc, stored, default)], None where the program prints '-'"""
    text = ''.join('%s %d\n' % c for c in calls)
    lines = subprocess.run([exe], input=text, stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout.splitlines()
    assert len(lines) == len(calls)
    return [tuple(None if w == '-' else int(w) for w in line.split()) for line in lines]


def _calls(section):
    return [(name, v) for name, rec in section['options'].items() for v, _, _ in rec['probes']]


@pytest.mark.parametrize('build', sorted(SECTIONS))
def test_every_recorded_option_call_replays(rules, host_exes, build):
    section = rules[build]
    assert len(section['options']) == 68
    calls = _calls(section)
    got = dict(zip(calls, _replay(host_exes[build], calls)))
    checked = 0
    for name, rec in section['options'].items():
        for value, rc, stored in rec['probes']:
            if (build, name, value) in HANDLE_ANSWERS:
                assert name in HANDLE_OPTIONS
                continue
            assert got[(name, value)] == (rc, stored, rec['default']), (build, name, value)
            checked += 1
    assert checked == len(calls) - sum(b == build for b, _, _ in HANDLE_ANSWERS)
    unknown = [(name, 1) for name, _ in section['unknown']]
    assert len(unknown) == 3
    assert [r[0] for r in _replay(host_exes[build], unknown)] == [rc for _, rc in section['unknown']] == [-1, -1, -1]


def test_the_fixture_probes_every_bound(rules):
    """what the recording had to contain: the six fixed values everywhere, and both sides of every bound of the rules"""
    want = {'wavek_eff64x32_pct': (29, 30, 31, 99, 100, 101), 'wavek_max_tiles': (8191, 8192, 8193), 'wavek_waves': (3, 4, 5, 7, 8, 9), 'wavek_tiny_waves': (3, 4, 5, 7, 8, 9),
            'wavek_depth': (1, 2, 3, 4), 'x3h_act_shift': (-9, -8, -7, 11, 12, 13), 'winograd_xcd_cols': (-2, -1, 0, 7, 8, 9), 'detect_chain_blocks': (0, 1, 2, 1023, 1024, 1025),
            'wavek_target_blocks': (-1, 0, 1, 511, 512, 513), 'wavek_g_boost': (0, 1, 2, 3, 4, 5), 'winograd_min_fill_pct': (0, 1, 2, 99, 100, 101), 'wavek_spread': (2, 3, 4),
            'winograd': (-1, 0, 1, 2, 3), 'precision': (-1, 0, 1, 2, 3), 'wavek_force_tail_g': (1, 2, 3)}
    for build in SECTIONS:
        for name, rec in rules[build]['options'].items():
            values = [p[0] for p in rec['probes']]
            assert set(values) >= {-2 ** 31, -1, 0, 1, 2, 2 ** 31 - 1} | set(want.get(name, ())), name
            if rec['default'] is not None:
                assert set(values) >= {rec['default'] - 1, rec['default'], rec['default'] + 1}, name


@pytest.mark.parametrize('build', sorted(SECTIONS))
def test_every_scan_mode_replays(rules, host_exes, build):
    rows = [[int(w) for w in line.split()] for line in subprocess.check_output([host_exes[build], '--scan'], universal_newlines=True).splitlines()]
    want = rules[build]['scan_modes']
    assert [m['mode'] for m in want] == list(range(-1, 13))
    assert rows == [[m['mode'], m['rc']] + m['fields'] for m in want]


@pytest.fixture(scope='module')
def emu_encoder():
    cfg = EncoderConfig()
    enc = eb.EmuEncoder(synth.make_weights(seed=3), cfg)
    yield enc
    enc.close()


def test_handle_options_on_the_emulator(rules, emu_encoder):
    """(the emulator library is an experiments build; the return codes do not depend on what earlier calls stored)"""
    L = emu_encoder.L
    assert L.aae_has_experiments() == 1
    for name in HANDLE_OPTIONS:
        for value, rc, _ in rules['experiments']['options'][name]['probes']:
            assert L.aae_encoder_set_option(emu_encoder.h, name.encode(), value) == rc, (name, value)


def test_upright_copies_follow_the_scan_mode(rules):
    L = eb.lib()
    L.aae_emu_codebook_scan_settings.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]

    def settings(cb, stride):
        out = (ctypes.c_int * 8)()
        assert L.aae_emu_codebook_scan_settings(cb.h, stride, out) == 0
        return list(out)

    E = synth.make_codebook(64, 128, seed=5)
    for m in rules['experiments']['scan_modes']:
        cb = eb.EmuCodebook(E)
        cb.prepare_upright(2)                                  # a copy made before the call ...
        assert L.aae_codebook_set_scan_mode(cb.h, m['mode']) == m['rc']
        cb.prepare_upright(3)                                  # ... and one made after it
        assert (settings(cb, 1), settings(cb, 2), settings(cb, 3)) == (m['fields'], m['upright_before'], m['upright_after']), m['mode']
        if m['rc'] == 0:
            assert m['fields'] == m['upright_before'] == m['upright_after']
        cb.close()


def test_every_option_is_documented(host_exes):
    names = subprocess.check_output([host_exes['product'], '--list'], universal_newlines=True).split()
    assert len(names) == len(set(names)) == 68
    assert names == subprocess.check_output([host_exes['experiments'], '--list'], universal_newlines=True).split()
    quoted = {}
    for header in ('aae_hip.h', 'aae_hip_tuning.h'):
        with open(os.path.join(ROOT, 'include', header)) as f:
            quoted[header] = set(re.findall(r'"([a-z][a-z_0-9]*)"', f.read()))
    assert set(names) <= quoted['aae_hip.h'] | quoted['aae_hip_tuning.h']
    assert (quoted['aae_hip.h'] | quoted['aae_hip_tuning.h']) - set(names) == {'f32x3h', 'next'}
    assert quoted['aae_hip_tuning.h'] - set(names) <= {'f32x3h', 'next'}


def test_host_program_under_sanitizers(rules, tmp_path, host_exes):
    """address + undefined-behaviour sanitizers on the stand-alone program (host code only): every recorded call, the scan modes, the list"""
    exe = _build(tmp_path, ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'], 'options_host_san')
    calls = _calls(rules['product']) + [('no_such_option', 1), ('', 0), ('x' * 100, 2 ** 31 - 1)]
    assert _replay(exe, calls) == _replay(host_exes['product'], calls)
    for arg in ('--scan', '--list'):
        assert subprocess.check_output([exe, arg]) == subprocess.check_output([host_exes['product'], arg])
