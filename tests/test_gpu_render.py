"""The mesh rasteriser on the MI355X against the NumPy float64 reference of tests/render_reference.py: full frames
(aae_render_frames through meshrenderer.Renderer), the fused embedding path (aae_render_embedding_views), batching into a
workspace full of garbage, and a codebook built end to end from rendered views (Dataset + MeshViewSource +
Codebook.update_embedding).  The meshes reach the renderer through PLY files, half of them binary."""
import configparser
import os

import numpy as np
import pytest

import render_cases as rc
import render_reference as rr
from oracle import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def renderers(tmp_path_factory):
    from augmentedautoencoder_amd.meshrenderer import Renderer
    d = tmp_path_factory.mktemp('render_ply')
    out = {}
    for k, name in enumerate(rc.MESHES):
        path = str(d / (name + '.ply'))
        rr.write_ply(path, rc.model_dict(name), binary=(k % 2 == 1))
        for kind in rc.MODELS:
            out[name, kind] = Renderer([path], model=kind)
            for got, want in zip(out[name, kind]._arrays[0], rc.arrays(name, kind)):
                assert np.array_equal(got, want)                 # the PLY round trip hands the kernels what the reference gets
    yield out
    for r in out.values():
        r.close()


def _frames(renderer, Rs, t, dims=rc.DIMS):
    W, H = dims
    bgr, depth, bbs, vis, tri = renderer.render_batch(0, W, H, rr.scaled_K(W, H), Rs, np.asarray(t, dtype=np.float64), rc.NEAR, rc.FAR, return_tri=True)
    return bgr.cpu().numpy(), depth.cpu().numpy(), bbs.cpu().numpy(), vis.cpu().numpy(), tri.cpu().numpy()


def _crops(renderer, Rs, t, crop, dims=rc.DIMS, **kw):
    W, H = dims
    return renderer.render_embedding_views(0, W, H, rr.scaled_K(W, H), Rs, t, rc.NEAR, rc.FAR, rc.PAD, crop, **kw)


@pytest.mark.parametrize('kind', rc.MODELS)
@pytest.mark.parametrize('name', rc.MESHES)
def test_frames_match_reference(renderers, name, kind):
    bgr, depth, bbs, vis, tri = _frames(renderers[name, kind], rc.rotations(name), rc.T0)
    total = 0
    for i in range(rc.N_ROT):
        ref = rc.reference(name, kind, i)
        total += rc.check_frame(ref, bgr[i], depth[i], tri[i], '%s/%s view %d' % (name, kind, i))
        assert vis[i] == 1 and bbs[i].tolist() == ref['bb']
    print('%s/%s: %d differing pixels in %d views' % (name, kind, total, rc.N_ROT))


def test_single_render_call_and_full_resolution(renderers):
    r = renderers['torus', 'reconst']
    W, H = rc.FULL_DIMS
    bgr, depth = r.render(0, W, H, rr.scaled_K(W, H), rc.rotations('torus')[0], np.array(rc.T0), rc.NEAR, rc.FAR)
    assert bgr.shape == (H, W, 3) and bgr.dtype == np.uint8 and depth.shape == (H, W) and depth.dtype == np.float32
    ref = rc.reference('torus', 'reconst', 0, rc.T0, rc.FULL_DIMS)
    rc.check_frame(ref, bgr, depth, None, 'full resolution')
    crops, bbs, vis = _crops(r, rc.rotations('torus')[:1], rc.T0, 128, dims=rc.FULL_DIMS)
    assert bbs.cpu().numpy()[0].tolist() == ref['bb']
    rc.check_crop(ref, crops.cpu().numpy()[0], 'full resolution')


def test_frame_border(renderers):
    Rs = rc.rotations('torus')
    bgr, depth, bbs, vis, tri = _frames(renderers['torus', 'reconst'], Rs, rc.T_BORDER)
    for i in range(rc.N_ROT):
        ref = rc.reference('torus', 'reconst', i, rc.T_BORDER)
        rc.check_frame(ref, bgr[i], depth[i], tri[i], 'border view %d' % i)
        x, y, w, h = ref['bb']
        assert x + w == rc.DIMS[0] - 1 and y == 0                  # clipped as calc_2d_bbox clips it
        assert bbs[i].tolist() == ref['bb'] and vis[i] == 1


def test_per_view_translations(renderers):
    Rs = rc.rotations('box')[:2]
    ts = np.array([rc.T0, rc.T_BORDER])
    W, H = rc.DIMS
    bgr, depth, bbs, vis, tri = renderers['box', 'cad'].render_batch(0, W, H, rr.scaled_K(W, H), Rs, ts, rc.NEAR, rc.FAR, return_tri=True)
    for i in range(2):
        ref = rc.reference('box', 'cad', i, tuple(ts[i]))
        rc.check_frame(ref, bgr[i].cpu().numpy(), depth[i].cpu().numpy(), tri[i].cpu().numpy(), 'box/cad t%d' % i)


@pytest.mark.parametrize('crop', [128, 32])
def test_embedding_views(renderers, crop):
    for name, kind in (('torus', 'reconst'), ('box', 'reconst'), ('box', 'cad'), ('degenerate', 'cad')):
        for t in ((rc.T0, rc.T_BORDER) if name == 'torus' else (rc.T0,)):
            crops, bbs, vis = _crops(renderers[name, kind], rc.rotations(name), t, crop)
            crops, bbs, vis = crops.cpu().numpy(), bbs.cpu().numpy(), vis.cpu().numpy()
            assert crops.shape == (rc.N_ROT, crop, crop, 3) and crops.dtype == np.uint8
            for i in range(rc.N_ROT):
                ref = rc.reference(name, kind, i, t)
                assert vis[i] == 1 and bbs[i].tolist() == ref['bb']
                if t == rc.T_BORDER:
                    x, y, w, h = ref['bb']
                    size = int(max(h, w) * rc.PAD)
                    assert x + w / 2 + size / 2 > rc.DIMS[0] and y + h / 2 - size / 2 < 0      # the source patch is clipped: not square
                rc.check_crop(ref, crops[i], '%s/%s view %d' % (name, kind, i))


def test_offscreen_view_sets_the_flag(renderers):
    crops, bbs, vis = _crops(renderers['torus', 'reconst'], rc.rotations('torus')[:2], rc.T_OFF, 32)
    assert vis.cpu().numpy().tolist() == [0, 0] and not crops.cpu().numpy().any() and not bbs.cpu().numpy().any()
    bgr, depth, bbs, vis, tri = _frames(renderers['torus', 'reconst'], rc.rotations('torus')[:1], rc.T_OFF)
    assert vis[0] == 0 and not bgr.any() and not depth.any() and (tri == -1).all()


CFG = """[Paths]
MODEL_PATH: %s
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


def _experiment(tmp_path, k02='160/2'):
    from augmentedautoencoder_amd import ae_factory as factory, session as S
    from augmentedautoencoder_amd.dataset import MeshViewSource
    S.reset_default_graph()
    path = str(tmp_path / 'torus.ply')
    rr.write_ply(path, rc.model_dict('torus'), binary=True)
    args = configparser.ConfigParser()
    args.read_string(CFG % (path, k02))
    with S.variable_scope('render_e2e'):
        ds = factory.build_dataset(str(tmp_path), args)
        enc = factory.build_encoder(S.Placeholder(ds.shape), args)
        cb = factory.build_codebook(enc, ds, args)
    return ds, enc, cb, MeshViewSource(ds)


def test_batches_and_garbage_workspace_give_identical_bytes(renderers, tmp_path):
    """rows [0, 70) of the 72-view viewsphere as one batch, as batches of 7 and one by one, every call into a workspace
    pre-filled with 0xA5"""
    import torch
    ds, _, _, src = _experiment(tmp_path)
    assert ds.embedding_size == 72
    Rs = ds.viewsphere_for_embedding[:70]
    r = src.renderer
    r._open()
    nbytes = int(r.lib.aae_render_workspace_bytes(r._meshes[0], 70, rc.DIMS[0], rc.DIMS[1]))
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device='cuda')
    ptr = ws.data_ptr() + (-ws.data_ptr()) % 256

    def run(step):
        parts = []
        for a in range(0, 70, step):
            ws.fill_(0xA5)
            c, b, v = _crops(r, Rs[a:a + step], src.t, 32, workspace=(ptr, nbytes))
            parts.append((c.cpu().numpy(), b.cpu().numpy(), v.cpu().numpy()))
        return [np.concatenate([p[k] for p in parts]) for k in range(3)]

    whole, sevens, singles = run(70), run(7), run(1)
    assert whole[2].all() and whole[0].any()
    for other in (sevens, singles):
        for a, b in zip(whole, other):
            assert a.tobytes() == b.tobytes()
    with pytest.raises(ValueError, match='workspace'):
        _crops(r, Rs, src.t, 32, workspace=(ptr, nbytes // 2))


def test_codebook_from_rendered_views_end_to_end(tmp_path):
    import torch
    ds, enc, cb, src = _experiment(tmp_path)
    enc.load_weights(synth.make_weights(seed=31, shape=(32, 32, 3), num_filter=[32, 64], strides=[2, 2], latent=128))
    ds.set_view_source(src)
    batch, bbs = ds.render_embedding_image_batch(0, 4)
    assert isinstance(batch, torch.Tensor) and batch.is_cuda and batch.dtype == torch.uint8 and tuple(batch.shape) == (4, 32, 32, 3)
    assert isinstance(bbs, np.ndarray) and bbs.shape == (4, 4)
    cb.update_embedding(None, 32)
    Rs = ds.viewsphere_for_embedding
    views, _ = src(0, 72, Rs)
    views = views.cpu().numpy()
    # Duplicate rotations share rows, so the matrices are compared, not the indices: linspace(0, 2pi, NUM_CYCLO) holds both
    # endpoints, and row 6k+5 = rot_z(-2pi)·R is row 6k up to sin(2pi) = 2.4e-16 in float64 -- the same image, and either row
    # may answer.  1e-12 is 4000 times that; two different rows of this viewsphere are 60 degrees in plane or an icosahedron's
    # edge apart, entries differing by more than 0.1.
    assert np.abs(Rs[5] - Rs[0]).max() < 1e-15 and not np.array_equal(Rs[5], Rs[0])
    for i in range(72):
        R = cb.nearest_rotation(None, views[i])
        assert np.abs(R - Rs[i]).max() < 1e-12, 'view %d came back as another rotation' % i
    mesh = rr.mesh_dict(rc.arrays('torus', 'reconst'))
    want = [rr.render(mesh, 'reconst', rr.scaled_K(*rc.DIMS), Rs[i], np.array(rc.T0), rc.DIMS[0], rc.DIMS[1], rc.NEAR, rc.FAR, shade=False)['bb']
            for i in range(72)]
    assert cb.embed_obj_bbs_value().tolist() == want


def test_view_source_names_the_hidden_row(tmp_path):
    ds, _, _, src = _experiment(tmp_path, k02='160/2 + 5000')                           # a principal point that throws every view off the frame
    ds.set_view_source(src)
    with pytest.raises(ValueError, match='row 8'):
        ds.render_embedding_image_batch(8, 12)
