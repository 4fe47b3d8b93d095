"""Several meshes into one frame on the MI355X (aae_render_scenes through meshrenderer.Renderer, built from PLY files): Scene A
against the reference composed in tests/scene_cases.py, the order rule, one draw per scene against render_batch, batched scenes
into a workspace full of garbage, the refusals, the overlay blend and PoseVisualizer."""
import ctypes

import numpy as np
import pytest

import render_cases as rc
import render_reference as rr
import scene_cases as sc

pytestmark = pytest.mark.gpu

W, H = rc.DIMS
K = rr.scaled_K(W, H)


@pytest.fixture(scope='module')
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp('scene_ply')
    out = {}
    for k, name in enumerate(sc.SET):
        out[name] = str(d / (name + '.ply'))
        rr.write_ply(out[name], rc.model_dict(name), binary=(k % 2 == 1))
    return out


@pytest.fixture(scope='module')
def renderers(paths):
    from augmentedautoencoder_amd.meshrenderer import Renderer
    out = {kind: Renderer([paths[name] for name in sc.SET], model=kind) for kind in rc.MODELS}
    yield out
    for r in out.values():
        r.close()


def _scenes(r, draws, scene_ids=None, n_scenes=1, **kw):
    Rs, ts = sc.poses(draws)
    scene_ids = [0] * len(draws) if scene_ids is None else scene_ids
    out = r.render_scenes(sc.obj_ids(draws), scene_ids, n_scenes, W, H, K, Rs, ts, rc.NEAR, rc.FAR, return_ids=True, **kw)
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize('kind', rc.MODELS)
def test_scene_a_matches_composed_reference(renderers, kind):
    ref = sc.check_scene_a_is_not_empty(kind)
    bgr, depth, bbs, vis, draw, tri = _scenes(renderers[kind], sc.SCENE_A)
    assert bgr.shape == (1, H, W, 3) and bgr.dtype == np.uint8 and depth.dtype == np.float32 and draw.dtype == np.int32 and tri.dtype == np.int32
    n_diff = sc.check_scene(ref, bgr[0], depth[0], draw[0], tri[0], 'scene A/%s' % kind)
    print('scene A/%s: measured %d differing pixels (expectation 0)' % (kind, n_diff))
    assert bbs.tolist() == ref['bbs'].tolist() and vis.tolist() == sc.FLAGS_A


def test_render_many_returns_the_reference_types(renderers):
    r = renderers['cad']
    draws = sc.SCENE_A[:3]
    Rs, ts = sc.poses(draws)
    bgr, depth, bbs = r.render_many(sc.obj_ids(draws), W, H, K, list(Rs), list(ts), rc.NEAR, rc.FAR)
    assert isinstance(bgr, np.ndarray) and bgr.dtype == np.uint8 and bgr.shape == (H, W, 3)
    assert isinstance(depth, np.ndarray) and depth.dtype == np.float32 and depth.shape == (H, W)
    assert isinstance(bbs, list) and all(isinstance(bb, list) and all(type(v) is int for v in bb) for bb in bbs)
    ref = sc.compose('cad', draws)
    assert bbs == ref['bbs'].tolist()
    sc.check_scene(ref, bgr, depth, ref['draw'], ref['tri'], 'render_many')
    draws = sc.SCENE_A
    Rs, ts = sc.poses(draws)
    with pytest.raises(ValueError, match=r'draw 4 \(obj_id 1\)'):
        r.render_many(sc.obj_ids(draws), W, H, K, list(Rs), list(ts), rc.NEAR, rc.FAR)
    # the default light is the reference's for the kind: drawn (np.random, the reference's order) for reconst, fixed for cad
    np.random.seed(5)
    renderers['reconst'].render_many([0], W, H, K, [Rs[0]], [ts[0]], rc.NEAR, rc.FAR)
    after = np.random.rand()
    np.random.seed(5)
    np.random.random(3), np.random.rand(), np.random.rand()
    assert after == np.random.rand()
    np.random.seed(5)
    r.render_many([0], W, H, K, [Rs[0]], [ts[0]], rc.NEAR, rc.FAR)
    after = np.random.rand()
    np.random.seed(5)
    assert after == np.random.rand()


@pytest.mark.parametrize('kind', rc.MODELS)
def test_draw_order_does_not_change_the_frame(renderers, kind):
    fwd = _scenes(renderers[kind], sc.SCENE_A[:4])
    perm = [3, 2, 1, 0]                                                        # reversed call position -> forward draw
    rev = _scenes(renderers[kind], [sc.SCENE_A[d] for d in perm])
    assert fwd[0].tobytes() == rev[0].tobytes() and fwd[1].tobytes() == rev[1].tobytes()
    assert np.array_equal(fwd[5], rev[5])                                     # the same face of the same mesh
    back = np.where(rev[4] >= 0, np.array(perm)[np.maximum(rev[4], 0)], -1)
    tied = fwd[4] == 0                                                        # draws 0 and 3 are one draw: the lower index is reported
    assert tied.sum() > 1000 and np.array_equal(back[~tied], fwd[4][~tied])
    assert (rev[4][tied] == 0).all() and (back[tied] == 3).all()
    assert np.array_equal(np.asarray(rev[2])[perm], fwd[2]) and np.array_equal(np.asarray(rev[3])[perm], fwd[3])


def test_one_draw_per_scene_equals_render_batch(renderers, paths):
    from augmentedautoencoder_amd.meshrenderer import Renderer
    for kind, name in (('reconst', 'torus'), ('cad', 'box'), ('reconst', 'degenerate')):
        single = Renderer([paths[name]], model=kind)
        Rs = rc.rotations(name)
        ts = np.array([rc.T0, rc.T_BORDER, rc.T0, rc.T_OFF, rc.T0, rc.T_BORDER])
        want = [t.cpu().numpy() for t in single.render_batch(0, W, H, K, Rs, ts, rc.NEAR, rc.FAR, return_tri=True)]
        draws = [(name, v, tuple(ts[v])) for v in range(rc.N_ROT)]
        bgr, depth, bbs, vis, draw, tri = _scenes(renderers[kind], draws, scene_ids=list(range(rc.N_ROT)), n_scenes=rc.N_ROT)
        for got, exp in zip((bgr, depth, bbs, vis, tri), want):
            assert got.dtype == exp.dtype and got.tobytes() == exp.tobytes()
        assert vis.tolist() == [1, 1, 1, 0, 1, 1]
        assert np.array_equal(draw, np.where(tri >= 0, np.arange(rc.N_ROT)[:, None, None], -1))
        single.close()


def test_batched_scenes_into_a_garbage_workspace(renderers):
    """1, 4, 0 and 2 draws in four scenes, scene ids interleaved, all three meshes of the set: one call into a workspace filled
    with 0xA5 equals four single-scene calls byte for byte."""
    import torch
    r = renderers['reconst']
    draws = (sc.SCENE_A[0], ('degenerate', 1, rc.T0), sc.SCENE_A[1], sc.SCENE_A[2], ('box', 2, rc.T0), sc.SCENE_A[3], ('torus', 4, rc.T_BORDER))
    scene_ids = [1, 0, 1, 3, 1, 1, 3]
    r._open()
    nbytes = int(r.lib.aae_render_scenes_workspace_bytes(r._set, len(draws), 4, W, H))
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device='cuda')
    ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    ws.fill_(0xA5)
    bgr, depth, bbs, vis, draw, tri = _scenes(r, draws, scene_ids=scene_ids, n_scenes=4, workspace=(ptr, nbytes))
    assert not bgr[2].any() and not depth[2].any() and (draw[2] == -1).all() and (tri[2] == -1).all()
    assert vis.tolist() == [1] * 7
    for s in (0, 1, 3):
        members = [d for d in range(len(draws)) if scene_ids[d] == s]
        ws.fill_(0xA5)
        one = _scenes(r, [draws[d] for d in members], workspace=(ptr, nbytes))
        assert one[0][0].tobytes() == bgr[s].tobytes() and one[1][0].tobytes() == depth[s].tobytes() and one[5][0].tobytes() == tri[s].tobytes()
        assert one[2].tobytes() == bbs[members].tobytes() and one[3].tobytes() == vis[members].tobytes()
        assert np.array_equal(np.where(one[4][0] >= 0, np.array(members)[np.maximum(one[4][0], 0)], -1), draw[s])
        sc.check_scene(sc.compose('reconst', [draws[d] for d in members]), one[0][0], one[1][0], one[4][0], one[5][0], 'batched scene %d' % s)
    with pytest.raises(ValueError, match='workspace'):
        _scenes(r, draws, scene_ids=scene_ids, n_scenes=4, workspace=(ptr, nbytes // 2))


def test_box_of_a_draw_across_the_frame_border(renderers):
    draws = (sc.SCENE_A[1], ('torus', 0, rc.T_BORDER), ('torus', 1, rc.T_BORDER))
    bgr, depth, bbs, vis, draw, tri = _scenes(renderers['reconst'], draws)
    for d, view in ((1, 0), (2, 1)):
        want = rc.reference('torus', 'reconst', view, rc.T_BORDER)['bb']
        assert want[0] + want[2] == W - 1 and want[1] == 0                    # clipped as calc_2d_bbox clips it
        assert bbs[d].tolist() == want
    sc.check_scene(sc.compose('reconst', draws), bgr[0], depth[0], draw[0], tri[0], 'border scene')


def test_refusals_name_the_call(renderers):
    r = renderers['reconst']
    Rs, ts = sc.poses(sc.SCENE_A[:2])
    with pytest.raises(ValueError, match='aae_render_scenes.*257 draws'):
        r.render_scenes([0] * 257, [0] * 257, 1, W, H, K, np.tile(Rs[:1], (257, 1, 1)), np.tile(ts[:1], (257, 1)), rc.NEAR, rc.FAR)
    with pytest.raises(ValueError, match='aae_render_scenes.*draw 1 names mesh 3'):
        r.render_scenes([0, 3], [0, 0], 1, W, H, K, Rs, ts, rc.NEAR, rc.FAR)
    with pytest.raises(ValueError, match='aae_render_scenes.*draw 1 names mesh -1'):
        r.render_scenes([0, -1], [0, 0], 1, W, H, K, Rs, ts, rc.NEAR, rc.FAR)
    with pytest.raises(ValueError, match='aae_render_scenes.*draw 0 names scene 2 of 2'):
        r.render_scenes([0, 1], [2, 0], 2, W, H, K, Rs, ts, rc.NEAR, rc.FAR)
    with pytest.raises(ValueError, match='aae_render_scenes.*near'):
        r.render_scenes([0, 1], [0, 0], 1, W, H, K, Rs, ts, rc.FAR, rc.NEAR)
    # the raw call refuses 257 draws too, and a set of two model kinds cannot be made
    obj = (ctypes.c_int32 * 257)()
    one = ctypes.c_void_p(256)
    rcode = r.lib.aae_render_scenes(r._set, obj, obj, one, one, 257, 1, ctypes.byref(rr_params()), one, one, None, None, one, one, one, 1 << 30, None)
    assert rcode == -2 and b'aae_render_scenes: 257 draws' in r.lib.aae_last_error()
    renderers['cad']._open()
    mixed = (ctypes.c_void_p * 2)(r._meshes[0].value, renderers['cad']._meshes[0].value)
    h = ctypes.c_void_p()
    assert r.lib.aae_mesh_set_create(mixed, 2, ctypes.byref(h)) == -2 and not h.value
    assert b'aae_mesh_set_create' in r.lib.aae_last_error() and b'kind' in r.lib.aae_last_error()


def rr_params():
    from augmentedautoencoder_amd.meshrenderer import render_params
    return render_params(W, H, K, None, rc.NEAR, rc.FAR)


@pytest.mark.parametrize('channel', [0, 1, 2])
def test_overlay_blend_equals_the_reference_expression(renderers, channel):
    import torch
    r = renderers['cad']
    image, render = sc.blend_table()
    want = sc.blend_reference(image, render, channel)
    img_d, ren_d = torch.as_tensor(image, device='cuda'), torch.as_tensor(render, device='cuda')
    out = r.overlay_blend(img_d, ren_d, channel=channel)
    assert out.cpu().numpy().tobytes() == want.tobytes() and img_d.cpu().numpy().tobytes() == image.tobytes()
    same = r.overlay_blend(img_d, ren_d, channel=channel, out=img_d)           # out aliases image
    assert same is img_d and img_d.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError, match='aae_overlay_blend'):
        r.overlay_blend(img_d, ren_d, channel=3)


def test_pose_visualizer(paths):
    from augmentedautoencoder_amd.pose_estimator import PoseEstimate
    from augmentedautoencoder_amd.visualization import PoseVisualizer
    vis = PoseVisualizer(sc.Estimator([('torus', paths['torus']), ('box', paths['box'])]))
    rng = np.random.RandomState(17)
    images = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2)]
    poses = []
    for name, view, t in sc.SCENE_A[:2]:
        trafo = np.eye(4)
        trafo[:3, :3], trafo[:3, 3] = rc.rotations(name)[view], t
        poses.append(PoseEstimate(name=name, trafo=trafo))
    keep = images[0].copy()
    shown = vis.render_poses(images[0], K, poses, [], vis_bbs=False)
    assert np.array_equal(images[0], keep) and shown.dtype == np.uint8 and shown.shape == (H, W, 3)
    bgr, depth, bbs = vis.renderer.render_many([0, 1], W, H, K, [p.trafo[:3, :3] for p in poses], [p.trafo[:3, 3] for p in poses], 10, 10000)
    assert vis.renderer.model == 'cad' and (bgr > 0).any(axis=2).sum() > 1500
    assert shown.tobytes() == sc.blend_reference(images[0], bgr, 1).tobytes()
    assert np.array_equal(shown[bgr == 0], images[0][bgr == 0])               # untouched outside the render
    both = vis.render_poses_batch(images, K, [poses, poses[:1]])
    assert both[0].tobytes() == shown.tobytes()
    assert both[1].tobytes() == vis.render_poses(images[1], K, poses[:1], [], vis_bbs=False).tobytes()
    assert np.array_equal(vis.render_poses_batch(images, K, [[], poses[1:]])[0], images[0])          # an image without poses stays as it is
    vis.close()
