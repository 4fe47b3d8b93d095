"""Training pairs on the MI355X (aae_render_training_views through meshrenderer.Renderer.render_training_views and Dataset)
against the NumPy float64 reference composed in tests/train_cases.py, the byte equalities with the existing entry points,
batching into a workspace full of garbage, the off-screen view, and the training-set file end to end (Dataset and the command
line)."""
import configparser
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import render_cases as rc
import render_reference as rr
import train_cases as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def renderers(tmp_path_factory):
    from augmentedautoencoder_amd.meshrenderer import Renderer
    d = tmp_path_factory.mktemp('train_ply')
    out = {}
    for k, (name, kind) in enumerate((('torus', 'reconst'), ('box', 'cad'))):
        path = str(d / (name + '.ply'))
        rr.write_ply(path, rc.model_dict(name), binary=(k % 2 == 1))
        out[name, kind] = Renderer([path], model=kind)
    yield out
    for r in out.values():
        r.close()


def _pairs(renderer, Rs, t, lights, offsets, **kw):
    W, H = rc.DIMS
    return renderer.render_training_views(0, W, H, rr.scaled_K(W, H), Rs, t, rc.NEAR, rc.FAR, rc.PAD, tc.CROP, lights, offsets, **kw)


def _host(tensors):
    return [t.cpu().numpy() for t in tensors]


@pytest.mark.parametrize('name,kind,t', tc.CASES)
def test_pairs_match_reference(renderers, name, kind, t):
    import torch
    refs = tc.assert_case_is_sharp(name, kind, t)
    out = _pairs(renderers[name, kind], rc.rotations(name), t, tc.lights(name, kind), tc.U)
    assert out[1].dtype == torch.bool and all(o.is_cuda for o in out)
    x, m, y, bbs, vis = _host(out)
    assert x.shape == y.shape == (rc.N_ROT, tc.CROP, tc.CROP, 3) and m.shape == (rc.N_ROT, tc.CROP, tc.CROP)
    for i, ref in enumerate(refs):
        tc.check_pair(ref, x[i], m[i], y[i], bbs[i].tolist(), int(vis[i]), '%s/%s t=%s view %d' % (name, kind, t, i))


@pytest.mark.parametrize('name,kind,t', [('torus', 'reconst', rc.T_BORDER), ('box', 'cad', rc.T0)])
def test_byte_equalities_with_the_existing_entry_points(renderers, name, kind, t):
    r = renderers[name, kind]
    W, H = rc.DIMS
    Rs, lights = rc.rotations(name), tc.lights(name, kind)
    x, m, y, bbs, vis = _host(_pairs(r, Rs, t, lights, tc.U))
    crops, bbs_e, vis_e = _host(r.render_embedding_views(0, W, H, rr.scaled_K(W, H), Rs, t, rc.NEAR, rc.FAR, rc.PAD, tc.CROP))
    assert y.tobytes() == crops.tobytes() and np.array_equal(bbs, bbs_e) and np.array_equal(vis, vis_e) and vis.all()
    for i in range(rc.N_ROT):
        bgr, depth, bb, _ = _host(r.render_batch(0, W, H, rr.scaled_K(W, H), Rs[i:i + 1], np.asarray(t, dtype=np.float64), rc.NEAR, rc.FAR,
                                                 light=tc.light_tuple(lights[i])))
        assert np.array_equal(bb[0], bbs[i])
        w, h = bb[0][2], bb[0][3]
        shifted = bb[0] + np.array([tc.U[i, 0] * w, tc.U[i, 1] * h, 0, 0])
        assert x[i].tobytes() == rr.extract_square_patch(bgr[0], shifted, rc.PAD, resize=(tc.CROP, tc.CROP)).tobytes(), 'train_x %d' % i
        assert np.array_equal(m[i], rr.extract_square_patch(depth[0], shifted, rc.PAD, resize=(tc.CROP, tc.CROP)) == 0), 'mask_x %d' % i
        assert x[i].any() and not m[i].all() and m[i].any()


def test_batches_and_garbage_workspace_give_identical_bytes(renderers):
    """14 views as one batch, as two of 7 and one by one, every call into a workspace pre-filled with 0xA5"""
    import torch
    r = renderers['torus', 'reconst']
    r._open()
    rng = np.random.RandomState(77)
    Rs = rr.random_rotations(14, 5)
    lights = np.concatenate([tc.lights('torus', 'reconst'), tc.lights('torus', 'cad'), tc.lights('torus', 'reconst')[:2]])
    offsets = rng.uniform(-0.2, 0.2, (14, 2))
    nbytes = int(r.lib.aae_render_training_workspace_bytes(r._meshes[0], 14, rc.DIMS[0], rc.DIMS[1]))
    assert nbytes > int(r.lib.aae_render_workspace_bytes(r._meshes[0], 14, rc.DIMS[0], rc.DIMS[1]))
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device='cuda')
    ptr = ws.data_ptr() + (-ws.data_ptr()) % 256

    def run(step):
        parts = []
        for a in range(0, 14, step):
            ws.fill_(0xA5)
            parts.append(_host(_pairs(r, Rs[a:a + step], rc.T_BORDER, lights[a:a + step], offsets[a:a + step], workspace=(ptr, nbytes))))
        return [np.concatenate([p[k] for p in parts]) for k in range(5)]

    whole, sevens, singles = run(14), run(7), run(1)
    assert whole[4].all() and whole[0].any() and whole[2].any() and not whole[1].all()
    for other in (sevens, singles):
        for a, b in zip(whole, other):
            assert a.tobytes() == b.tobytes()
    with pytest.raises(ValueError, match='workspace'):
        _pairs(r, Rs, rc.T_BORDER, lights, offsets, workspace=(ptr, nbytes // 2))
    timed = _pairs(r, Rs, rc.T_BORDER, lights, offsets, timed=True)
    assert len(timed[5]) == 6 and all(ms >= 0 for ms in timed[5]) and timed[0].cpu().numpy().tobytes() == whole[0].tobytes()


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
K: [1075.65*160/720, 0, %s, 0, 1073.90*120/540, 120/2, 0, 0, 1]
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
[Network]
BATCH_NORMALIZATION: False
LATENT_SPACE_SIZE: 128
NUM_FILTER: [32, 64]
STRIDES: [2, 2]
KERNEL_SIZE_ENCODER: 5
[Training]
BATCH_SIZE: 32
"""


def _args(tmp_path, k02='160/2'):
    path = str(tmp_path / 'torus.ply')
    if not os.path.exists(path):
        rr.write_ply(path, rc.model_dict('torus'), binary=True)
    text = CFG % (path, k02)
    args = configparser.ConfigParser()
    args.read_string(text)
    return args, text


def test_offscreen_view(renderers, tmp_path):
    from augmentedautoencoder_amd import ae_factory as factory
    x, m, y, bbs, vis = _host(_pairs(renderers['torus', 'reconst'], rc.rotations('torus')[:2], rc.T_OFF, tc.lights('torus', 'reconst')[:2], tc.U[:2]))
    assert vis.tolist() == [0, 0] and not x.any() and not y.any() and m.all() and not bbs.any()
    args, _ = _args(tmp_path, k02='160/2 + 5000')                             # a principal point that throws every view off the frame
    ds = factory.build_dataset(str(tmp_path), args)
    with pytest.raises(ValueError, match=r'training image 0\). Have you scaled the vertices to mm\?'):
        ds.render_training_images()


def test_training_set_file_end_to_end(tmp_path):
    from augmentedautoencoder_amd import ae_factory as factory, utils as u
    from augmentedautoencoder_amd.meshrenderer import Renderer
    args, text = _args(tmp_path)
    name = hashlib.md5(str(args.items('Dataset') + args.items('Paths')).encode('utf-8')).hexdigest() + '.npz'

    def render(seed, folder):
        os.makedirs(str(folder))
        ds = factory.build_dataset(str(folder), args)
        np.random.seed(seed)
        path = ds.get_training_images(str(folder), args, batch=5)             # 12 images in calls of 5, 5 and 2
        assert path == os.path.join(str(folder), name) and os.path.exists(path)
        return ds, np.load(path)

    ds, data = render(4, tmp_path / 'a')
    assert sorted(data.keys()) == ['mask_x', 'train_x', 'train_y']
    assert data['train_x'].shape == data['train_y'].shape == (12, 32, 32, 3) and data['train_x'].dtype == data['train_y'].dtype == np.uint8
    assert data['mask_x'].shape == (12, 32, 32) and data['mask_x'].dtype == bool
    assert ds.noof_obj_pixels.shape == (12,) and (ds.noof_obj_pixels > 0).all()
    assert np.array_equal(ds.noof_obj_pixels, (~data['mask_x']).sum(axis=(1, 2)))
    assert not np.array_equal(data['train_x'], data['train_y'])

    again = factory.build_dataset(str(tmp_path / 'a'), args)                  # finds the file: nothing is rendered
    opened = []
    orig = Renderer._open
    Renderer._open = lambda self: opened.append(1) or orig(self)
    try:
        again.get_training_images(str(tmp_path / 'a'), args)
    finally:
        Renderer._open = orig
    assert not opened and all(np.array_equal(getattr(again, k), data[k]) for k in data.keys())

    _, same = render(4, tmp_path / 'b')
    _, other = render(5, tmp_path / 'c')
    assert all(same[k].tobytes() == data[k].tobytes() for k in data.keys())
    assert other['train_x'].tobytes() != data['train_x'].tobytes() and other['train_y'].tobytes() != data['train_y'].tobytes()

    # the command line on a workspace of its own: the same file
    ws = tmp_path / 'ws'
    cfg_path = u.get_config_file_path(str(ws), 'obj', 'grp')
    os.makedirs(os.path.dirname(cfg_path))
    with open(cfg_path, 'w') as f:
        f.write(text)
    env = dict(os.environ, AE_WORKSPACE_PATH=str(ws), PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.check_output([sys.executable, '-m', 'augmentedautoencoder_amd.ae_train_data', 'grp/obj', '--seed', '4', '--batch', '5'], env=env,
                                  cwd=ROOT, timeout=300).decode()
    cli_path = os.path.join(u.get_dataset_path(str(ws)), name)
    assert cli_path in out and 'images/s' in out
    cli = np.load(cli_path)
    assert all(cli[k].tobytes() == data[k].tobytes() and cli[k].dtype == data[k].dtype for k in data.keys())
