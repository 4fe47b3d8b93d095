"""Several meshes into one frame without a GPU: the scene text of csrc/kernels/render_core.h (key packing and decoding, the
per-draw bounds, the overlay blend) compiled for the host and driven serially by tests/native/scene_host.cpp, against the
reference composed in tests/scene_cases.py from the NumPy float64 render of each draw alone; and the same driver under
-fsanitize=address,undefined as a stand-alone program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import render_cases as rc
import scene_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))


def _compiler():
    for c in ('g++', '/opt/rocm/lib/llvm/bin/clang++', 'clang++'):
        path = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if path:
            return path
    raise RuntimeError('no host C++ compiler (g++ or clang++) found')


def _build(out_dir, flags, name):
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-O2', '-ffp-contract=off', '-Wall'] + flags +
                          [os.path.join(HERE, 'native', 'scene_host.cpp'), '-o', exe])
    return exe


@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('scene_host'), [], 'scene_host')


def _run(exe, tmp_path, kind, draws, tag='', **kw):
    scene, out = str(tmp_path / ('scene%s.bin' % tag)), str(tmp_path / ('out%s.bin' % tag))
    sc.write_scene(scene, kind, draws, **kw)
    subprocess.check_call([exe, scene, out])
    return open(out, 'rb').read(), sc.read_host_output(out, len(draws), kw.get('n_scenes', 1))


def _check_scene_a(kind, scenes, bbs, visible, label):
    ref = sc.check_scene_a_is_not_empty(kind)
    s = scenes[0]
    n_diff = sc.check_scene(ref, s['bgr'], s['depth'], s['draw'], s['tri'], label)
    print('%s: measured %d differing pixels (expectation 0)' % (label, n_diff))
    assert bbs.tolist() == ref['bbs'].tolist()
    assert visible == sc.FLAGS_A
    return n_diff


@pytest.mark.parametrize('kind', rc.MODELS)
def test_scene_a_matches_composed_reference_in_any_draw_order(host_exe, tmp_path, kind):
    D = len(sc.SCENE_A)
    orders = {'forward': list(range(D)), 'reversed': list(range(D))[::-1], 'shuffled': np.random.RandomState(7).permutation(D).tolist()}
    assert orders['shuffled'] not in (orders['forward'], orders['reversed'])
    raws = {}
    for tag, order in orders.items():
        raws[tag], (scenes, bbs, visible) = _run(host_exe, tmp_path, kind, sc.SCENE_A, tag=tag, order=order)
        _check_scene_a(kind, scenes, bbs, visible, 'scene A/%s %s' % (kind, tag))
    assert raws['forward'] == raws['reversed'] == raws['shuffled']


def test_scene_a_pixel_counts():
    """The counts the case was designed with (kind reconst): who covers, who wins, who ties."""
    ref = sc.check_scene_a_is_not_empty('reconst')
    assert ref['covered'] == [1798, 634, 1270, 1798, 0]
    assert ref['wins'] == [1429, 117, 792, 0, 0]


def test_batched_scenes_equal_single_scenes(host_exe, tmp_path):
    """1, 4, 0 and 2 draws in four scenes, scene ids interleaved: every scene equals the scene drawn alone."""
    draws = (sc.SCENE_A[0], ('degenerate', 1, rc.T0), sc.SCENE_A[1], sc.SCENE_A[2], ('box', 2, rc.T0), sc.SCENE_A[3], ('torus', 4, rc.T_BORDER))
    scene_ids = [1, 0, 1, 3, 1, 1, 3]
    _, (scenes, bbs, visible) = _run(host_exe, tmp_path, 'reconst', draws, scene_ids=scene_ids, n_scenes=4)
    assert not scenes[2]['bgr'].any() and not scenes[2]['depth'].any() and (scenes[2]['draw'] == -1).all() and (scenes[2]['tri'] == -1).all()
    for s in (0, 1, 3):
        members = [d for d in range(len(draws)) if scene_ids[d] == s]
        ref = sc.compose('reconst', [draws[d] for d in members])
        draw = scenes[s]['draw'].copy()
        for local, d in enumerate(members):                               # the call's draw index -> the index within the scene
            draw[scenes[s]['draw'] == d] = local
        sc.check_scene(ref, scenes[s]['bgr'], scenes[s]['depth'], draw, scenes[s]['tri'], 'batched scene %d' % s)
        assert bbs[members].tolist() == ref['bbs'].tolist()
    assert visible == [1] * 7


def test_host_driver_under_sanitizers(tmp_path):
    """address + undefined-behaviour sanitizers on the stand-alone driver, Scene A and the blend table."""
    exe = _build(tmp_path, ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'], 'scene_host_san')
    for kind in rc.MODELS:
        _, (scenes, bbs, visible) = _run(exe, tmp_path, kind, sc.SCENE_A, tag=kind, order=[2, 4, 0, 3, 1])
        _check_scene_a(kind, scenes, bbs, visible, 'sanitized scene A/%s' % kind)
    image, render = sc.blend_table()
    assert _blend(exe, tmp_path, image, render, 1).tobytes() == sc.blend_reference(image, render, 1).tobytes()


def _blend(exe, tmp_path, image, render, channel):
    src, out = str(tmp_path / 'blend_in.bin'), str(tmp_path / 'blend_out.bin')
    with open(src, 'wb') as f:
        f.write(image.tobytes())
        f.write(render.tobytes())
    subprocess.check_call([exe, '--blend', str(channel), src, out])
    return np.frombuffer(open(out, 'rb').read(), np.uint8).reshape(image.shape)


@pytest.mark.parametrize('channel', [0, 1, 2])
def test_blend_equals_the_reference_expression_for_every_byte_pair(host_exe, tmp_path, channel):
    image, render = sc.blend_table()
    assert image.shape == (256, 256, 3) and len(set(zip(render[:, :, 0].ravel().tolist(), image[:, :, 0].ravel().tolist()))) == 65536
    want = sc.blend_reference(image, render, channel)
    got = _blend(host_exe, tmp_path, image, render, channel)
    assert got.dtype == np.uint8 and got.tobytes() == want.tobytes()
    # where the render is 0 the image stays; elsewhere the other channels keep a third of the image
    assert np.array_equal(got[0], image[0]) and np.array_equal(got[1:, :, (channel + 1) % 3], (image[1:, :, 0].astype(np.float64) * 1. / 3.).astype(np.uint8))
