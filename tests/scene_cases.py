"""The cases of the scene tests (several meshes drawn into one frame), shared by the CPU test (the scene text of render_core.h
through tests/native/scene_host.cpp) and the GPU test (the kernels of render_scene.h): the draws of Scene A, the reference of a
scene composed from tests/render_reference.render of each draw alone (per pixel the smallest fp32 depth, the earlier draw on
equality; the draw's box is that render's box), and the frame assertions of render_cases.check_frame carried over to
(draw, triangle) winners."""
import collections
import configparser
import functools

import numpy as np

import render_cases as rc
import render_reference as rr

SET = rc.MESHES                                 # the mesh set: obj_id indexes it (torus 0, box 1, degenerate 2)
W, H = rc.DIMS

# Scene A: (mesh, view of render_cases.rotations(mesh), t).  Draw 3 is draw 0 again (every pixel ties), draw 4 is off-screen.
SCENE_A = (('torus', 0, (0.0, 0.0, 700.0)),
           ('box', 1, (25.0, 10.0, 680.0)),
           ('torus', 2, (-40.0, 20.0, 740.0)),
           ('torus', 0, (0.0, 0.0, 700.0)),
           ('box', 3, (5000.0, 0.0, 700.0)))
FLAGS_A = [1, 1, 1, 1, 0]


def obj_ids(draws):
    return [SET.index(name) for name, _, _ in draws]


def poses(draws):
    Rs = np.stack([rc.rotations(name)[view] for name, view, _ in draws]).astype(np.float64)
    ts = np.array([t for _, _, t in draws], dtype=np.float64)
    return Rs, ts


def draw_reference(kind, draw):
    name, view, t = draw
    return rc.reference(name, kind, view, tuple(t))


def compose(kind, draws):
    """The scene's reference: dict(bgr, depth, draw, tri (-1 background), bbs [D,4] (0 where nothing is covered), visible [D],
    covered [D] and wins [D] pixel counts)."""
    depth = np.zeros((H, W), np.float32)
    draw_i = np.full((H, W), -1, np.int64)
    tri = np.full((H, W), -1, np.int64)
    bgr = np.zeros((H, W, 3), np.uint8)
    bbs, visible, covered = [], [], []
    for d, draw in enumerate(draws):
        ref = draw_reference(kind, draw)
        cov = ref['tri'] >= 0
        take = cov & ((draw_i < 0) | (ref['depth'] < depth))             # strictly nearer: the earlier draw keeps a tie
        depth[take] = ref['depth'][take]
        draw_i[take] = d
        tri[take] = ref['tri'][take]
        bgr[take] = ref['bgr'][take]
        bbs.append(ref['bb'] if ref['bb'] is not None else [0, 0, 0, 0])
        visible.append(0 if ref['bb'] is None else 1)
        covered.append(int(cov.sum()))
    wins = [int((draw_i == d).sum()) for d in range(len(draws))]
    return dict(bgr=bgr, depth=depth, draw=draw_i, tri=tri, bbs=np.array(bbs, np.int32).reshape(-1, 4), visible=visible, covered=covered, wins=wins)


@functools.lru_cache(maxsize=None)
def scene_a(kind):
    return compose(kind, SCENE_A)


def check_scene_a_is_not_empty(kind):
    """The properties the case stands on, asserted on the composed reference itself, so a change of the fixtures cannot
    silently empty it: each of draws 0-2 both wins and loses pixels, and draw 3 ties with draw 0 on all of draw 0's pixels."""
    ref = scene_a(kind)
    for d in range(3):
        assert 0 < ref['wins'][d] < ref['covered'][d], 'draw %d: %d covered, %d won' % (d, ref['covered'][d], ref['wins'][d])
    r0, r3 = draw_reference(kind, SCENE_A[0]), draw_reference(kind, SCENE_A[3])
    ties = (r0['tri'] >= 0) & (r3['tri'] >= 0) & (r0['depth'] == r3['depth'])
    assert int(ties.sum()) == ref['covered'][0] == ref['covered'][3] > 1000
    assert ref['wins'][3] == 0 and ref['covered'][4] == 0 and ref['visible'] == FLAGS_A
    return ref


def check_scene(ref, bgr, depth, draw, tri, label=''):
    """render_cases.check_frame with (draw, triangle) as the winner.  Returns the number of differing pixels."""
    cov_ref = ref['draw'] >= 0
    cov = depth > 0
    assert np.all(bgr[~cov] == 0) and np.all(depth[~cov] == 0), '%s: background must be exactly 0' % label
    assert np.array_equal(draw >= 0, cov) and np.array_equal(tri >= 0, cov)
    n_cov = int(cov_ref.sum())
    both = cov & cov_ref
    differ = (cov != cov_ref) | (both & ((draw != ref['draw']) | (tri != ref['tri'])))
    ulps = rc.ulp_distance(depth, ref['depth'])
    differ |= both & (ulps > 2)
    n_diff = int(differ.sum())
    agree = both & ~differ
    print('%s: %d covered pixels, %d differ' % (label, n_cov, n_diff))
    assert n_diff <= 1e-4 * n_cov, '%s: %d of %d covered pixels differ' % (label, n_diff, n_cov)
    assert ulps[agree].max(initial=0) <= 2
    err = np.abs(bgr.astype(np.int32) - ref['bgr'].astype(np.int32))[agree]
    assert err.max(initial=0) <= 1, '%s: BGR differs by %d levels' % (label, err.max(initial=0))
    return n_diff


# ---- the blend of visualization/render_pose.py:44-46 -------------------------------------------------------------------
def blend_table():
    """Every (render, image) byte pair as a 256 x 256 x 3 image pair: (image, render), render value along the rows."""
    g, i = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    return np.ascontiguousarray(np.repeat(i[:, :, None], 3, axis=2)), np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def blend_reference(image, render, channel):
    """The reference's literal lines with `channel` in place of 1."""
    image_show = image.copy()
    bgr = render
    g_y = np.zeros_like(bgr)
    g_y[:, :, channel] = bgr[:, :, channel]
    image_show[bgr > 0] = g_y[bgr > 0]*2./3. + image_show[bgr > 0]*1./3.
    return image_show


# ---- PoseVisualizer ---------------------------------------------------------------------------------------------------------
TRAIN_CFG = """[Paths]
MODEL_PATH: %s
[Dataset]
VERTEX_SCALE: %d
"""


class Estimator(object):
    """What PoseVisualizer reads of an AePoseEstimator: class_2_encoder (its key order is the class order) and all_train_args."""

    def __init__(self, models, vertex_scale=1):
        self.class_2_encoder = collections.OrderedDict((name, object()) for name, _ in models)
        self.all_train_args = {}
        for name, path in models:
            args = configparser.ConfigParser()
            args.read_string(TRAIN_CFG % (path, vertex_scale))
            self.all_train_args[name] = args


# ---- tests/native/scene_host.cpp: scene file in, frames out ------------------------------------------------------------
def write_scene(path, kind, draws, scene_ids=None, n_scenes=1, order=None):
    D = len(draws)
    Rs, ts = poses(draws)
    scene_ids = [0] * D if scene_ids is None else scene_ids
    order = list(range(D)) if order is None else list(order)
    with open(path, 'wb') as f:
        f.write(np.array([len(SET), 1 if kind == 'cad' else 0, D, n_scenes, W, H], dtype=np.int32).tobytes())
        f.write(np.asarray(rr.scaled_K(W, H), dtype=np.float64).tobytes())
        f.write(np.array([rc.NEAR, rc.FAR], dtype=np.float64).tobytes())
        f.write(np.array([400, 400, 400, 0.4, 0.8, 0.3], dtype=np.float32).tobytes())
        for name in SET:
            verts, normals, colors, faces = rc.arrays(name, kind)
            f.write(np.array([len(verts), len(faces)], dtype=np.int32).tobytes())
            f.write(verts.astype(np.float32).tobytes())
            f.write(normals.astype(np.float32).tobytes())
            f.write(colors.astype(np.float32).tobytes())
            f.write(faces.astype(np.int32).tobytes())
        f.write(np.array(obj_ids(draws), dtype=np.int32).tobytes())
        f.write(np.array(scene_ids, dtype=np.int32).tobytes())
        f.write(np.array(order, dtype=np.int32).tobytes())
        f.write(Rs.tobytes())
        f.write(ts.tobytes())


def read_host_output(path, n_draws, n_scenes=1):
    raw = open(path, 'rb').read()
    scenes, o = [], 0
    for _ in range(n_scenes):
        s = {}
        s['bgr'] = np.frombuffer(raw, np.uint8, W * H * 3, o).reshape(H, W, 3); o += W * H * 3
        s['depth'] = np.frombuffer(raw, np.float32, W * H, o).reshape(H, W); o += W * H * 4
        s['draw'] = np.frombuffer(raw, np.int32, W * H, o).reshape(H, W); o += W * H * 4
        s['tri'] = np.frombuffer(raw, np.int32, W * H, o).reshape(H, W); o += W * H * 4
        scenes.append(s)
    bbs = np.frombuffer(raw, np.int32, n_draws * 4, o).reshape(n_draws, 4); o += n_draws * 16
    visible = np.frombuffer(raw, np.int32, n_draws, o).tolist(); o += n_draws * 4
    assert o == len(raw)
    return scenes, bbs, visible
