"""Training pairs without a GPU: the training text of csrc/kernels/render_core.h (rc_light_dir, rc_offset_box, rc_shade_relit)
compiled for the host and driven by tests/native/train_host.cpp against the NumPy float64 reference composed in
tests/train_cases.py; the byte equalities between the pair and the existing embedding crop; the same driver under
-fsanitize=address,undefined; the random draws against a fixture recorded from the reference's own loop
(tests/golden/make_training_draws_golden.py); and the Python surface (file name, load-if-present, extract_square_patch, errors,
command line, exports)."""
import configparser
import hashlib
import os
import subprocess

import numpy as np
import pytest

import render_cases as rc
import render_reference as rr
import train_cases as tc
from test_render_cpu import _compiler
from augmentedautoencoder_amd import _lib, ae_train_data, meshrenderer as mr
from augmentedautoencoder_amd.dataset import Dataset

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, 'golden')


def _build(out_dir, flags, source, name):
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-O2', '-ffp-contract=off', '-Wall'] + flags + [os.path.join(HERE, 'native', source), '-o', exe])
    return exe


@pytest.fixture(scope='module')
def train_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('train_host'), [], 'train_host.cpp', 'train_host')


@pytest.fixture(scope='module')
def render_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('render_host_for_train'), [], 'render_host.cpp', 'render_host')


def _run(exe, tmp_path, name, kind, Rs, t, lights, offsets):
    scene, out = str(tmp_path / 'train_scene.bin'), str(tmp_path / 'train_out.bin')
    n = tc.write_scene(scene, name, kind, Rs, t, lights, offsets)
    subprocess.check_call([exe, scene, out])
    return tc.read_host_output(out, n)


@pytest.mark.parametrize('name,kind,t', tc.CASES)
def test_pairs_match_reference(train_exe, tmp_path, name, kind, t):
    refs = tc.assert_case_is_sharp(name, kind, t)
    views = _run(train_exe, tmp_path, name, kind, rc.rotations(name), t, tc.lights(name, kind), tc.U)
    for i, (v, ref) in enumerate(zip(views, refs)):
        label = '%s/%s t=%s view %d' % (name, kind, t, i)
        tc.check_pair(ref, v['train_x'], v['mask_x'], v['train_y'], v['bb'], v['visible'], label)
        assert v['rect_x'] == ref['rect_x'] and v['rect_y'] == ref['rect_y'], label
        assert v['bb_off'] == np.array(ref['bb_off']).astype(np.int32).tolist(), label


def test_train_y_equals_the_embedding_crop(train_exe, render_exe, tmp_path):
    for name, kind, t in (('torus', 'reconst', rc.T_BORDER), ('box', 'cad', rc.T0)):
        Rs = rc.rotations(name)
        views = _run(train_exe, tmp_path, name, kind, Rs, t, tc.lights(name, kind), tc.U)
        scene, out = str(tmp_path / 'scene.bin'), str(tmp_path / 'out.bin')
        n = rc.write_scene(scene, name, kind, Rs, t=t, crop=tc.CROP)
        subprocess.check_call([render_exe, scene, out])
        for v, w in zip(views, rc.read_host_output(out, n, crop=tc.CROP)):
            assert v['train_y'].tobytes() == w['crop'].tobytes() and v['bb'] == w['bb'] and v['visible'] == w['visible'] == 1


def test_no_shift_and_default_light_give_x_equal_y(train_exe, tmp_path):
    for name, kind, t in (('torus', 'reconst', tc.T_LEFT), ('box', 'cad', rc.T0)):
        views = _run(train_exe, tmp_path, name, kind, rc.rotations(name), t, np.tile(tc.DEFAULT_LIGHT, (rc.N_ROT, 1)), np.zeros((rc.N_ROT, 2)))
        for v in views:
            assert v['train_x'].tobytes() == v['train_y'].tobytes() and v['train_y'].any()
            assert np.array_equal(v['mask_x'] == 1, v['train_y'].max(axis=2) == 0)          # no object colour of these meshes is black
            assert v['rect_x'] == v['rect_y'] and v['bb_off'] == v['bb']


def test_offscreen_view(train_exe, tmp_path):
    v = _run(train_exe, tmp_path, 'torus', 'reconst', rc.rotations('torus')[:1], rc.T_OFF, tc.lights('torus', 'reconst')[:1], tc.U[:1])[0]
    assert v['visible'] == 0 and not v['train_x'].any() and not v['train_y'].any() and (v['mask_x'] == 1).all() and v['bb'] == [0, 0, 0, 0]


def test_host_driver_under_sanitizers(tmp_path):
    """address + undefined-behaviour sanitizers on the stand-alone driver: a border case, the cad kind, the off-screen view."""
    exe = _build(tmp_path, ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'], 'train_host.cpp', 'train_host_san')
    for name, kind, t in (('torus', 'reconst', rc.T_BORDER), ('box', 'cad', rc.T0), ('torus', 'cad', rc.T_OFF)):
        views = _run(exe, tmp_path, name, kind, rc.rotations(name)[:2], t, tc.lights(name, kind)[:2], tc.U[:2])
        if t == rc.T_BORDER:
            ref = tc.reference_pair(name, kind, 0, t)
            tc.check_pair(ref, views[0]['train_x'], views[0]['mask_x'], views[0]['train_y'], views[0]['bb'], views[0]['visible'], 'sanitized')


# ---- the random draws and the rectangles against the reference's own loop -------------------------------------------------
def _host_rects(exe, tmp_path, bbs, us, W, H, pad):
    src, out = str(tmp_path / 'rects_in.bin'), str(tmp_path / 'rects_out.bin')
    with open(src, 'wb') as f:
        f.write(np.array([len(bbs), W, H], dtype=np.int32).tobytes())
        f.write(np.array([pad], dtype=np.float64).tobytes())
        for bb, u in zip(bbs, us):
            f.write(np.asarray(bb, dtype=np.int32).tobytes())
            f.write(np.asarray(u, dtype=np.float64).tobytes())
    subprocess.check_call([exe, '--rects', src, out])
    return np.fromfile(out, dtype=np.int32).reshape(len(bbs), 12)


def test_draws_and_rectangles_equal_the_reference_loop(train_exe, tmp_path):
    gold = np.load(os.path.join(GOLDEN, 'training_draws_ref.npz'))
    W, H = [int(v) for v in gold['render_dims']]
    pad, m = float(gold['pad_factor']), float(gold['max_rel_offset'])
    n = int(gold['noof_training_imgs'])
    runs = sharp = 0
    for kind in ('reconst', 'cad'):
        for seed in gold['seeds']:
            key = '%s_%d_' % (kind, seed)
            np.random.seed(int(seed))
            Rs, lights, offsets = mr.draw_training_params(n, m, kind)
            assert Rs.tobytes() == gold[key + 'R'].tobytes()
            assert lights.tobytes() == gold[key + 'light'].tobytes()        # position, then the constants the kind's renderer perturbs
            bbs = gold[key + 'bb']
            shifted = bbs[:, :2] + gold[key + 'trans']
            sharp += int(((shifted < 0) & (np.floor(shifted) != np.trunc(shifted))).sum())
            want = gold[key + 'rects']                                    # per image: x colour patch, x depth patch, y patch (l, r, t, b)
            got = _host_rects(train_exe, tmp_path, bbs, offsets, W, H, pad)
            assert np.array_equal(got[:, 4:8], want[:, 0]) and np.array_equal(got[:, 4:8], want[:, 1]) and np.array_equal(got[:, 8:12], want[:, 2])
            # the offsets themselves: the reference's products u * w and u * h, bit for bit
            assert (offsets[:, 0] * bbs[:, 2]).tobytes() == gold[key + 'trans'][:, 0].tobytes()
            assert (offsets[:, 1] * bbs[:, 3]).tobytes() == gold[key + 'trans'][:, 1].tobytes()
            # and what np.random holds afterwards: nothing more, nothing less was drawn
            assert np.random.rand() == float(gold[key + 'next_rand'])
            runs += 1
    assert runs == 2 * len(gold['seeds']) >= 4
    assert sharp >= 10                            # shifted corners left of / above the frame, where a floor would cut another rectangle
    assert any((gold['%s_%d_rects' % (k, s)][:, 0] != gold['%s_%d_rects' % (k, s)][:, 2]).any() for k in ('reconst', 'cad') for s in gold['seeds'])


def test_random_rotation_matrix_is_a_rotation():
    R = mr.random_rotation_matrix(np.array([0.3, 0.6, 0.9]))
    assert R.shape == (4, 4) and np.allclose(R.T.dot(R), np.identity(4)) and np.isclose(np.linalg.det(R[:3, :3]), 1.0)
    assert np.array_equal(R[3], [0, 0, 0, 1]) and np.array_equal(R[:, 3], [0, 0, 0, 1])


# ---- Python surface without a GPU -------------------------------------------------------------------------------------------
CFG = """[Paths]
MODEL_PATH: %s
BACKGROUND_IMAGES_GLOB: /nowhere/*.jpg
[Dataset]
MODEL: reconst
H: 32
W: 32
C: 3
RADIUS: 700
RENDER_DIMS: (160, 120)
K: [1075.65*160/720, 0, 160/2, 0, 1073.90*120/540, 120/2, 0, 0, 1]
VERTEX_SCALE: 1
ANTIALIASING: 1
PAD_FACTOR: 1.2
CLIP_NEAR: 10
CLIP_FAR: 10000
NOOF_TRAINING_IMGS: 12
MAX_REL_OFFSET: 0.2
[Embedding]
EMBED_BB: True
MIN_N_VIEWS: 12
NUM_CYCLO: 6
"""


def _args(tmp_path):
    path = str(tmp_path / 'torus.ply')
    rr.write_ply(path, rr.torus_model())
    args = configparser.ConfigParser()
    args.read_string(CFG % path)
    return args


def test_file_name_and_load_if_present(tmp_path, monkeypatch):
    from augmentedautoencoder_amd import ae_factory as factory
    args = _args(tmp_path)
    ds = factory.build_dataset(str(tmp_path), args)
    assert ds.noof_training_imgs == 12
    pairs = [(k, args.get('Dataset', k)) for k in args.options('Dataset')] + [(k, args.get('Paths', k)) for k in args.options('Paths')]
    name = hashlib.md5(repr(pairs).encode('utf-8')).hexdigest() + '.npz'
    rng = np.random.RandomState(3)
    x, y = rng.randint(0, 255, (5, 32, 32, 3)), rng.randint(0, 255, (5, 32, 32, 3))
    mask = rng.rand(5, 32, 32) < 0.5
    np.savez(str(tmp_path / name), train_x=x, mask_x=mask, train_y=y)             # int64 on purpose: the load casts to uint8
    monkeypatch.setattr(mr.Renderer, '_open', lambda self: pytest.fail('the load-if-present branch opened the renderer'))
    monkeypatch.setattr(Dataset, 'render_training_images', lambda self, batch=256: pytest.fail('the load-if-present branch rendered'))
    path = ds.get_training_images(str(tmp_path), args)
    assert os.path.basename(path) == name
    assert ds.train_x.dtype == np.uint8 and ds.train_y.dtype == np.uint8 and ds.mask_x.dtype == bool
    assert np.array_equal(ds.train_x, x) and np.array_equal(ds.train_y, y) and np.array_equal(ds.mask_x, mask)
    assert np.array_equal(ds.noof_obj_pixels, (~mask).sum(axis=(1, 2)))


def test_extract_square_patch_equals_reference():
    ds = Dataset('', h=8, w=8, c=3)                                     # every new keyword is read lazily
    rng = np.random.RandomState(9)
    img = rng.randint(0, 255, (120, 160, 3)).astype(np.uint8)
    depth = rng.rand(120, 160).astype(np.float32)
    for bb in ([40, 30, 50, 40], [120, 0, 39, 60], [-7.9, 90.7, 30, 29], [0, 0, 159, 119], [60.5, 50.5, 1, 1]):
        for size in ((32, 32), (128, 128), (7, 7)):
            assert np.array_equal(ds.extract_square_patch(img, bb, 1.2, resize=size), rr.extract_square_patch(img, bb, 1.2, resize=size))
            assert np.array_equal(ds.extract_square_patch(depth, bb, 1.2, resize=size, interpolation=0), rr.extract_square_patch(depth, bb, 1.2, resize=size))
    got = ds.extract_square_patch(img, [40, 30, 50, 40], 1.2, resize=(60, 60), black_borders=True)
    assert not got[0].any() and not got[:, 0].any() and got[30, 30].any()
    for bad in ('linear', 1, 3):
        with pytest.raises(NotImplementedError, match='nearest'):
            ds.extract_square_patch(img, [40, 30, 50, 40], 1.2, interpolation=bad)


def test_construction_errors(tmp_path):
    from test_render_cpu import _dataset
    with pytest.raises(KeyError):
        Dataset('', h=8, w=8, c=3).noof_training_imgs
    with pytest.raises(NotImplementedError, match='C = 1'):
        _dataset(tmp_path, c=1, noof_training_imgs=2, max_rel_offset=0.2).render_training_images()
    with pytest.raises(NotImplementedError, match='square'):
        _dataset(tmp_path, h=32, w=48, noof_training_imgs=2, max_rel_offset=0.2).render_training_images()
    with pytest.raises(NotImplementedError, match='ANTIALIASING'):
        _dataset(tmp_path, antialiasing=8, noof_training_imgs=2, max_rel_offset=0.2).render_training_images()
    with pytest.raises(KeyError, match='max_rel_offset'):
        _dataset(tmp_path, noof_training_imgs=2).render_training_images()


def test_command_line_argument_errors(tmp_path, monkeypatch, capsys):
    from augmentedautoencoder_amd import utils as u
    monkeypatch.delenv('AE_WORKSPACE_PATH', raising=False)
    with pytest.raises(SystemExit, match='AE_WORKSPACE_PATH'):
        ae_train_data.main(['grp/obj'])
    ws = tmp_path / 'ws'
    monkeypatch.setenv('AE_WORKSPACE_PATH', str(ws))
    with pytest.raises(SystemExit, match='config file'):
        ae_train_data.main(['grp/obj'])
    with pytest.raises(SystemExit):
        ae_train_data.main(['grp/obj', '--batch', '0'])
    with pytest.raises(SystemExit):
        ae_train_data.main([])
    cfg_path = u.get_config_file_path(str(ws), 'obj', 'grp')
    os.makedirs(os.path.dirname(cfg_path))
    with open(cfg_path, 'w') as f:
        f.write(CFG % str(tmp_path / 'missing_model.ply'))
    with pytest.raises(SystemExit, match='missing_model.ply'):
        ae_train_data.main(['grp/obj', '--seed', '3'])
    opts = ae_train_data._parse(['grp/obj', '--seed', '3', '--batch', '64'])
    assert (opts.seed, opts.batch) == (3, 64) and ae_train_data._parse(['obj']).batch == 256


def test_training_symbols_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'aae_hip.h')).read()
    names = ('aae_render_training_workspace_bytes', 'aae_render_training_views', 'aae_render_training_views_timed')
    import __graft_entry__ as g
    g.build()
    out = subprocess.check_output(['/opt/rocm/lib/llvm/bin/llvm-readelf', '--dyn-syms', '--wide', g.LIB]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if ' FUNC ' in l and ' UND ' not in l)
    for name in names:
        assert name + '(' in header and name in _lib.EXPORTED_SYMBOLS and name in exported
    assert '#define AAE_ABI_VERSION 3' in header and _lib.AAE_ABI_VERSION == 3
