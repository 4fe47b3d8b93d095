"""The rasteriser without a GPU: csrc/kernels/render_core.h compiled for the host and driven by tests/native/render_host.cpp
(serial loops in place of the launches) against the NumPy float64 reference of tests/render_reference.py, with the
assertions of the GPU test; the PLY reader and the camera against goldens recorded from the reference's own code; the
construction errors of the Python surface; and the same driver under -fsanitize=address,undefined."""
import configparser
import os
import shutil
import subprocess

import numpy as np
import pytest

import render_cases as rc
import render_reference as rr
from augmentedautoencoder_amd import _lib, ae_embed, meshrenderer as mr
from augmentedautoencoder_amd.dataset import Dataset, MeshViewSource

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, 'golden')


def _compiler():
    for c in ('g++', '/opt/rocm/lib/llvm/bin/clang++', 'clang++'):
        path = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if path:
            return path
    raise RuntimeError('no host C++ compiler (g++ or clang++) found')


def _build(out_dir, flags, name):
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-O2', '-ffp-contract=off', '-Wall'] + flags +
                          [os.path.join(HERE, 'native', 'render_host.cpp'), '-o', exe])
    return exe


@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('render_host'), [], 'render_host')


def _run(exe, tmp_path, name, kind, Rs, crop=0, **kw):
    scene, out = str(tmp_path / 'scene.bin'), str(tmp_path / 'out.bin')
    n = rc.write_scene(scene, name, kind, Rs, crop=crop, **kw)
    subprocess.check_call([exe, scene, out])
    return rc.read_host_output(out, n, kw.get('dims', rc.DIMS), crop)


@pytest.mark.parametrize('kind', rc.MODELS)
@pytest.mark.parametrize('name', rc.MESHES)
def test_frames_and_crops_match_reference(host_exe, tmp_path, name, kind):
    views = _run(host_exe, tmp_path, name, kind, rc.rotations(name), crop=32)
    covered = 0
    for i, v in enumerate(views):
        ref = rc.reference(name, kind, i)
        rc.check_frame(ref, v['bgr'], v['depth'], v['tri'], '%s/%s view %d' % (name, kind, i))
        assert v['visible'] == 1 and v['bb'] == ref['bb']
        rc.check_crop(ref, v['crop'], '%s/%s view %d' % (name, kind, i))
        covered += int((ref['tri'] >= 0).sum())
    assert covered > 6 * 500                      # the object is there (torus: 1500-2000 pixels a view)


def test_degenerate_faces_are_skipped(host_exe, tmp_path):
    faces = rc.arrays('degenerate', 'reconst')[3]
    skipped = [0, 101, len(faces) - 1]
    assert faces[0][0] == faces[0][1] and faces[101][1] == faces[101][2]
    for i, v in enumerate(_run(host_exe, tmp_path, 'degenerate', 'reconst', rc.rotations('degenerate'))):
        assert not np.isin(v['tri'], skipped).any()
        # the other faces are the torus's, shifted by the inserted ones
        assert np.array_equal(v['depth'] > 0, rc.reference('degenerate', 'reconst', i)['tri'] >= 0)


def test_frame_border_and_offscreen(host_exe, tmp_path):
    Rs = rc.rotations('torus')
    for crop in (128, 32):
        views = _run(host_exe, tmp_path, 'torus', 'reconst', Rs[:2], t=rc.T_BORDER, crop=crop)
        for i, v in enumerate(views):
            ref = rc.reference('torus', 'reconst', i, rc.T_BORDER)
            rc.check_frame(ref, v['bgr'], v['depth'], v['tri'], 'border view %d' % i)
            x, y, w, h = ref['bb']
            assert x + w == rc.DIMS[0] - 1 and y == 0                     # clipped as calc_2d_bbox clips it
            assert v['bb'] == ref['bb']
            rc.check_crop(ref, v['crop'], 'border view %d' % i)
    off = _run(host_exe, tmp_path, 'torus', 'reconst', Rs[:1], t=rc.T_OFF, crop=32)[0]
    assert off['visible'] == 0 and not off['depth'].any() and not off['bgr'].any() and not off['crop'].any()


def test_full_resolution_view(host_exe, tmp_path):
    v = _run(host_exe, tmp_path, 'torus', 'reconst', rc.rotations('torus')[:1], dims=rc.FULL_DIMS, crop=128)[0]
    ref = rc.reference('torus', 'reconst', 0, rc.T0, rc.FULL_DIMS)
    rc.check_frame(ref, v['bgr'], v['depth'], v['tri'], 'full resolution')
    assert v['bb'] == ref['bb']
    rc.check_crop(ref, v['crop'], 'full resolution')


def test_per_view_translations(host_exe, tmp_path):
    Rs = rc.rotations('box')[:2]
    ts = np.array([rc.T0, rc.T_BORDER])
    views = _run(host_exe, tmp_path, 'box', 'cad', Rs, ts=ts)
    for i, v in enumerate(views):
        ref = rc.reference('box', 'cad', i, tuple(ts[i]))
        rc.check_frame(ref, v['bgr'], v['depth'], v['tri'], 'box/cad t%d' % i)


def test_host_driver_under_sanitizers(tmp_path):
    """address + undefined-behaviour sanitizers on the stand-alone driver: every mesh, the border, the off-screen view."""
    exe = _build(tmp_path, ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'], 'render_host_san')
    for name, kind, t in (('torus', 'reconst', rc.T0), ('box', 'cad', rc.T0), ('degenerate', 'reconst', rc.T_BORDER), ('torus', 'cad', rc.T_OFF)):
        views = _run(exe, tmp_path, name, kind, rc.rotations(name)[:2], t=t, crop=32)
        if t == rc.T0:
            rc.check_frame(rc.reference(name, kind, 0), views[0]['bgr'], views[0]['depth'], views[0]['tri'], 'sanitized %s/%s' % (name, kind))


# ---- PLY reader and camera against the reference's own code (tests/golden/make_render_golden.py) ------------------------
@pytest.mark.parametrize('fmt', ['ascii', 'binary'])
def test_load_ply_equals_reference_reader(fmt):
    gold = np.load(os.path.join(GOLDEN, 'render_golden.npz'))
    model = mr.load_ply(os.path.join(GOLDEN, 'render_%s.ply' % fmt))
    for key in ('pts', 'normals', 'colors', 'faces'):
        want = gold['%s_%s' % (fmt, key)]
        assert model[key].dtype == want.dtype and np.array_equal(model[key], want), key
    assert set(model) == {'pts', 'normals', 'colors', 'faces'}


def test_pixel_coordinates_equal_reference_camera():
    gold = np.load(os.path.join(GOLDEN, 'render_golden.npz'))
    X = np.concatenate([rr.torus_model()['pts'][::7], rr.box_model()['pts']])
    for k in range(3):
        W, H = [int(v) for v in gold['cam_dims'][k]]
        K, R, t = gold['cam_K'][k], gold['cam_R'][k], gold['cam_t'][k]
        view, proj = gold['cam_T_view_world'][k].astype(np.float64), gold['cam_T_proj_view'][k].astype(np.float64)
        u, v, zc = rr.pixel_coordinates(K, R, t, X)
        # float64 matrices of the same construction (the recorded ones are the reference's float32 copies: compared loosely,
        # they pin the convention; the float64 rebuild pins the numbers to 1e-9)
        view64 = rr.view_matrix(R, t)
        assert np.allclose(view64, view, rtol=1e-5, atol=1e-3)
        proj64 = rr.projection_matrix(K, W, H, gold['cam_near_far'][k][0], gold['cam_near_far'][k][1])
        assert np.allclose(proj64, proj, rtol=1e-5, atol=1e-4)
        for V_, P_, tol in ((view64, proj64, 1e-9), (view, proj, 2e-4)):
            clip = np.concatenate([X, np.ones((len(X), 1))], axis=1).dot(V_.T).dot(P_.T)
            ndc = clip[:, :3] / clip[:, 3:4]
            want_u, want_v = (ndc[:, 0] + 1) / 2 * W, (1 - ndc[:, 1]) / 2 * H
            # glReadPixels rows start at the bottom and the reference flips them (meshrenderer_phong.py:161-162); with
            # originIsInTopLeft the projection flips y once more: row 0 is the top, v grows downwards
            assert np.allclose(u, want_u, rtol=tol, atol=tol * W) and np.allclose(v, want_v, rtol=tol, atol=tol * H)


# ---- Python surface without a GPU ---------------------------------------------------------------------------------------
def _dataset(tmp_path, **over):
    kw = dict(h=32, w=32, c=3, model='reconst', model_path=str(tmp_path / 'torus.ply'), antialiasing=1, vertex_scale=1, radius=700,
              render_dims='(160, 120)', k='[1075.65*160/720, 0, 160/2, 0, 1073.90*120/540, 120/2, 0, 0, 1]', clip_near=10, clip_far=10000,
              pad_factor=1.2, min_n_views=12, num_cyclo=6)
    kw.update(over)
    rr.write_ply(kw['model_path'], rr.torus_model())
    return Dataset(str(tmp_path), **kw)


def test_ply_round_trip_and_mesh_arrays(tmp_path):
    for name in rc.MESHES:
        model = rc.model_dict(name)
        for binary in (False, True):
            path = str(tmp_path / ('%s_%d.ply' % (name, binary)))
            rr.write_ply(path, model, binary=binary)
            back = mr.load_ply(path)
            for key in ('pts', 'normals', 'colors', 'faces'):
                # (an ascii file carries float32 values as 9 significant digits: equal once rounded to float32, which is
                #  what the vertex buffer holds)
                assert np.array_equal(np.float32(back[key]), np.float32(model[key])), (name, binary, key)
    verts, normals, colors, faces = rc.arrays('box', 'cad')
    assert verts.shape == (36, 3) and faces.tolist() == np.arange(36).reshape(12, 3).tolist()
    assert np.allclose(np.abs(normals).max(axis=1), 1) and np.allclose(colors[0] * 255, [223, 214, 205])
    assert np.array_equal(mr.calc_normals(np.zeros((3, 3), np.float32)), np.zeros((3, 3), np.float32))
    no_colour = dict(model)
    del no_colour['colors']
    assert np.all(mr.mesh_arrays(no_colour, 'reconst')[2] == np.float32(160.0 / 255.0))


def test_dataset_renderer_and_view_source_errors(tmp_path):
    with pytest.raises(NotImplementedError):
        Dataset('', h=8, w=8, c=3).render_embedding_image_batch(0, 1)          # unchanged without a view source
    ds = _dataset(tmp_path)
    src = MeshViewSource(ds)
    assert src.render_dims == (160, 120) and src.crop == 32 and src.K[0, 2] == 80.0 and src.renderer is ds.renderer
    assert ds.renderer.model == 'reconst' and len(ds.renderer._arrays[0][3]) == 576
    with pytest.raises(FileNotFoundError, match='nothing.ply'):
        Dataset('', h=32, w=32, c=3, model='reconst', model_path=str(tmp_path / 'nothing.ply')).renderer
    with pytest.raises(NotImplementedError, match='ANTIALIASING'):
        _dataset(tmp_path, antialiasing=8).renderer
    with pytest.raises(NotImplementedError, match='C = 1'):
        MeshViewSource(_dataset(tmp_path, c=1))
    with pytest.raises(NotImplementedError, match='square'):
        MeshViewSource(_dataset(tmp_path, h=32, w=48))
    with pytest.raises(ValueError, match='MODEL'):
        _dataset(tmp_path, model='mesh').renderer
    with pytest.raises(ValueError):
        MeshViewSource(_dataset(tmp_path, k='[__import__("os").getcwd(), 0, 0, 0, 1, 0, 0, 0, 1]'))


def test_random_light_draws_in_the_reference_order():
    np.random.seed(5)
    light, a, d, s = mr.draw_light(True, None, 'reconst')
    np.random.seed(5)
    want_light = 1000. * np.random.random(3)
    want_d = 0.8 + 0.1 * (2 * np.random.rand() - 1)
    want_s = 0.3 + 0.1 * (2 * np.random.rand() - 1)
    assert np.array_equal(light, want_light) and (a, d, s) == (0.4, want_d, want_s)
    np.random.seed(5)
    light, a, d, s = mr.draw_light(True, {'ambient': 0.5, 'diffuse': 0.6, 'specular': 0.1}, 'cad')
    np.random.seed(5)
    np.random.random(3)
    assert a == 0.5 + 0.1 * (2 * np.random.rand() - 1) and d == 0.6 + 0.1 * (2 * np.random.rand() - 1)
    assert mr.draw_light(False, None, 'cad') == ((400., 400., 400.), 0.4, 0.8, 0.3)


CFG = """[Paths]
MODEL_PATH: %s
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
[Embedding]
EMBED_BB: True
MIN_N_VIEWS: 12
NUM_CYCLO: 6
[Network]
BATCH_NORMALIZATION: False
LATENT_SPACE_SIZE: 128
NUM_FILTER: [32, 64]
STRIDES: [2, 2]
KERNEL_SIZE_ENCODER: 5
[Training]
BATCH_SIZE: 16
"""


def test_ae_embed_render_argument_errors(tmp_path, monkeypatch):
    from augmentedautoencoder_amd import session as S, utils as u
    S.reset_default_graph()
    ws = tmp_path / 'ws'
    monkeypatch.setenv('AE_WORKSPACE_PATH', str(ws))
    cfg_path = u.get_config_file_path(str(ws), 'obj', 'grp')
    os.makedirs(os.path.dirname(cfg_path))
    missing = str(tmp_path / 'missing_model.ply')
    with open(cfg_path, 'w') as f:
        f.write(CFG % missing)
    with pytest.raises(SystemExit, match='--render'):
        ae_embed.main(['grp/obj'])                                            # no view source named: the message lists --render
    with pytest.raises(SystemExit, match='missing_model.ply'):
        ae_embed.main(['grp/obj', '--render'])
    assert ae_embed._parse(['grp/obj', '--render']).render is True


def test_render_symbols_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'aae_hip.h')).read()
    names = ('aae_mesh_create', 'aae_mesh_destroy', 'aae_render_workspace_bytes', 'aae_render_embedding_views',
             'aae_render_embedding_views_timed', 'aae_render_frames')
    import __graft_entry__ as g
    g.build()
    out = subprocess.check_output(['/opt/rocm/lib/llvm/bin/llvm-readelf', '--dyn-syms', '--wide', g.LIB]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if ' FUNC ' in l and ' UND ' not in l)
    for name in names:
        assert name + '(' in header and name in _lib.EXPORTED_SYMBOLS and name in exported
    import ctypes
    assert ctypes.sizeof(_lib.RenderParams) == 9 * 8 + 3 * 8 + 8 + 3 * 8 + 6 * 4
