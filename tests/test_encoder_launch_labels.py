"""The per-class launch code (csrc/aae_encoder_launch.h, the decoder's launch_stage) against tests/golden/encoder_launch_labels.json,
recorded from commit c0553b5 before every kernel family got one form list and the launches one tail
(tests/golden/make_encoder_launch_labels.py): per case of tests/encoder_launch_cases.py the complete sequence of (kernel label,
flops) of one forward, in the experiments build (the emulator library) and in the product build, where an option the build
refuses is the recorded refusal code."""
import ctypes
import fcntl
import json
import os
import subprocess

import pytest

import emu_backend as eb
import encoder_launch_cases as elc
from augmentedautoencoder_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
AAE_ERR_UNSUPPORTED = -2      # include/aae_hip.h

# Arms the emulator does not replay, by name, with the reason (at most three).  Their records ARE in the fixture -- the recorder
# took the minute -- and tests/test_gpu_launch_forms.py runs them on the hardware.
NOT_REPLAYED = {
    'f32x3h wide256 tag 2': 'a 256 x 256 tile over K = 6400 in three fp16 products: 25 s on the emulator',
    'f32x3h wide256 tag 3': 'a 256 x 256 tile over K = 6400 in three fp16 products: 25 s on the emulator',
}


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(HERE, 'golden', 'encoder_launch_labels.json')) as f:
        return json.load(f)


def _lib_of(build):
    if build == 'experiments':
        return eb.lib()
    with open(os.path.join(HERE, 'emu', '.build.lock'), 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(['make', '-s', '-C', os.path.join(HERE, 'emu'), 'libaae_emu_product.so'])
    return _lib.declare(ctypes.CDLL(os.path.join(HERE, 'emu', 'libaae_emu_product.so')))


def test_the_fixture_holds_the_cases_and_names_the_parent(golden):
    assert golden['parent'] == 'c0553b5'
    assert golden['cases'] == elc.cases() and golden['decoder_cases'] == elc.decoder_cases()
    for build in elc.BOTH:
        assert len(golden[build]['encoder']) == len(golden['cases']) and len(golden[build]['decoder']) == len(golden['decoder_cases'])
    assert all(any(name == 'wavek_target_blocks' for name, _ in c['options']) for c in golden['cases'])


@pytest.mark.parametrize('build', elc.BOTH)
def test_every_recorded_case_replays(golden, build):
    L = _lib_of(build)
    assert L.aae_has_experiments() == (build == 'experiments')
    for case, want in zip(golden['cases'], golden[build]['encoder']):
        if not case['slow']:
            assert elc.replay(L, case) == want, case['name']
    for case, want in zip(golden['decoder_cases'], golden[build]['decoder']):
        assert elc.replay_decoder(L, case) == want, case['name']


def test_the_fixture_reaches_every_dispatch_arm(golden):
    """a case list that exercises nothing cannot pass: every arm of the launch code is in the recording of the builds that have it, the
    product build refuses what it does not have, and the cases the emulator leaves out are the arms NOT_REPLAYED names -- no more"""
    names = [c['name'] for c in golden['cases']] + [c['name'] for c in golden['decoder_cases']]
    assert len(set(names)) == len(names)
    record = {build: dict(zip(names, golden[build]['encoder'] + golden[build]['decoder'])) for build in elc.BOTH}
    for arm, (builds, case, pattern) in elc.ARMS.items():
        for build in builds:
            rec = record[build][case]
            assert 'records' in rec and elc.arm_reached(pattern, rec['records']), (arm, build, rec)
        if elc.P not in builds:                                   # an experiments-only form: the product build says so, or runs another kernel
            rec = record[elc.P][case]
            assert rec.get('refused', [None, 0])[1] == AAE_ERR_UNSUPPORTED or not elc.arm_reached(pattern, rec['records']), (arm, rec)
    for build in elc.BOTH:
        assert all(r['records'] and all(flops >= 0.0 for _, flops in r['records']) for r in record[build].values() if 'records' in r)
    assert any('refused' in r for r in record[elc.P].values()) and not any('refused' in r for r in record[elc.E].values())
    slow = {c['name'] for c in golden['cases'] if c['slow']}
    only_slow = {arm for arm, (_, case, _) in elc.ARMS.items() if case in slow}
    assert only_slow == set(NOT_REPLAYED) and len(NOT_REPLAYED) <= 3
