"""The grouped multi-object query's host planner (csrc/aae_multi_impl.h) against tests/golden/multi_plans.json, which was recorded
from commit 9689de6, before the planner's rules and the launch tables' builders were brought down to one copy each
(tests/golden/make_multi_plans.py): per frame, which objects aae_multi_workspace_bytes prepares Winograd-domain weights for, the
size it returns and every field of the MultiPlan, in the experiments build (the emulator library) and in the product build."""
import ctypes
import fcntl
import json
import os
import subprocess

import pytest

import emu_backend as eb
import multi_plan_frames as mpf
from augmentedautoencoder_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(HERE, 'golden', 'multi_plans.json')) as f:
        return json.load(f)


def _product_lib():
    with open(os.path.join(HERE, 'emu', '.build.lock'), 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(['make', '-s', '-C', os.path.join(HERE, 'emu'), 'libaae_emu_product.so'])
    return _lib.declare(ctypes.CDLL(os.path.join(HERE, 'emu', 'libaae_emu_product.so')))


def test_the_fixture_holds_the_frames_and_names_the_parent(golden):
    assert golden['parent'] == '9689de6'
    assert golden['frames'] == mpf.frames()
    assert len(golden['product']) == len(golden['experiments']) == len(golden['frames']) >= 38


@pytest.mark.parametrize('build', ['experiments', 'product'])
def test_every_recorded_frame_replays(golden, build):
    L = eb.lib() if build == 'experiments' else _product_lib()
    assert L.aae_has_experiments() == (build == 'experiments')
    for frame, want in zip(golden['frames'], golden[build]):
        got = mpf.replay(L, frame)
        for key in ('before', 'workspace_bytes', 'after'):
            assert got[key] == want[key], (frame, key)


@pytest.mark.parametrize('build', ['experiments', 'product'])
def test_the_fixture_exercises_every_outcome(golden, build):
    """a frame list that exercises nothing cannot pass: each form the planner can decide on is in the recording"""
    seen = set()
    for frame, rec in zip(golden['frames'], golden[build]):
        after = rec['after']
        assert after['rc'] == 0 and rec['workspace_bytes'] == after['total'] > 0
        assert all(not any(flags) for flags in rec['before']['prepared'])
        items = after['items']
        assert [it['row0'] for it in items] == [sum(i['n'] for i in items[:k]) for k in range(len(items))]
        assert sum(it['n'] for it in items) == sum(frame['counts'])
        if frame['scan_only']:
            seen.add('scan only')
            continue
        for g, wino in zip(after['groups'], after['group_wino']):
            if len(g) >= 2:
                seen.add('per-detection group with a Winograd layer' if any(wino) else 'per-detection group without a Winograd layer')
                # ... and then the size query prepared every member's weights
                assert not any(wino) or all(any(after['prepared'][items[i]['enc']]) for i in g)
        for g, rem in zip(after['mid_groups'], after['mid_rem']):
            assert len(g) >= 2 and all(items[i]['mid'] and any(after['prepared'][items[i]['enc']]) for i in g)
            seen.add('mid-batch group with handed-over images' if any(rem) else 'mid-batch group without handed-over images')
            if any(rem):
                assert any(p is not None for i in g for p in items[i]['rem_plans'])
        if after['split']:
            seen.add('split class')
            assert len(items) > len(frame['counts']) and max(it['n'] for it in items) <= 4
        alone = [it for it in items if not it['grouped'] and not it['mid']]
        if alone:
            assert after['seq'][1] > 0 and after['seq'][3] > 0
        # the default options: every class of five or more boxes is a mid-batch candidate; one left to the per-object path had its group dissolved
        if not frame['options'] and any(it['n'] >= 5 for it in alone):
            seen.add('dissolved mid-batch candidate group of %d' % sum(it['n'] >= 5 for it in alone))
        if any(it['n'] <= 4 for it in alone):
            seen.add('fallback item')
            assert {items.index(it) for it in alone} == {frame['bf16_item'], frame['stride2_item']}
    assert seen == {'scan only', 'per-detection group with a Winograd layer', 'per-detection group without a Winograd layer', 'mid-batch group with handed-over images',
                    'mid-batch group without handed-over images', 'split class', 'dissolved mid-batch candidate group of 1', 'dissolved mid-batch candidate group of 2',
                    'fallback item'}
