"""The cases of the training-pair tests, shared by the CPU test (render_core.h through tests/native/train_host.cpp) and the GPU
test (render_train.h): render_cases' meshes, rotations and camera, one more translation, per-view box offsets and lights, the
reference of a pair composed in NumPy float64 from tests/render_reference.py (computed once per process), and the assertions:
train_x and train_y within 1 grey level with at most 1e-4 of the sampled object pixels outside (expectation 0), mask_x equal
under the same cap, boxes and flags equal."""
import functools

import numpy as np

import render_cases as rc
import render_reference as rr

CROP = 32
T_LEFT = (-200.0, 150.0, 700.0)                 # torus across the left and bottom edges
# per-view (u_x, u_y): the corners of MAX_REL_OFFSET = 0.2, no shift, and one that is no round fraction
U = np.array([(0.2, -0.2), (-0.2, 0.2), (0.0, 0.0), (0.13, -0.07), (-0.2, -0.2), (0.2, 0.2)])
CASES = (('torus', 'reconst', rc.T0), ('torus', 'reconst', rc.T_BORDER), ('torus', 'reconst', T_LEFT), ('box', 'cad', rc.T0))
DEFAULT_LIGHT = np.array([400, 400, 400, 0.4, 0.8, 0.3], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def lights(name, kind):
    """[N_ROT,6] float32 in draw_light's ranges (meshrenderer_phong.py:117-121, meshrenderer.py:97-109) from a seeded RandomState."""
    rng = np.random.RandomState({'torus': 101, 'box': 202}[name])
    out = np.empty((rc.N_ROT, 6))
    for i in range(rc.N_ROT):
        out[i, :3] = 1000. * rng.random_sample(3)
        out[i, 3] = 0.4 + (0.1 * (2 * rng.rand() - 1) if kind == 'cad' else 0.0)
        out[i, 4] = 0.8 + 0.1 * (2 * rng.rand() - 1)
        out[i, 5] = 0.3 + 0.1 * (2 * rng.rand() - 1)
    return out.astype(np.float32)


def light_tuple(row):
    """a lights() row as render_batch's light argument"""
    return (tuple(float(v) for v in row[:3]), float(row[3]), float(row[4]), float(row[5]))


def source_rect(bb, shape):
    """left, right, top, bottom of extract_square_patch (dataset.py:356-362) for an int box"""
    x, y, w, h = np.array(bb).astype(np.int32)
    size = int(np.maximum(h, w) * rc.PAD)
    return (int(np.maximum(x + w / 2 - size / 2, 0)), int(np.minimum(x + w / 2 + size / 2, shape[1])),
            int(np.maximum(y + h / 2 - size / 2, 0)), int(np.minimum(y + h / 2 + size / 2, shape[0])))


@functools.lru_cache(maxsize=None)
def reference_pair(name, kind, view, t):
    """dataset.py:243-303 for one image: dict(train_x, mask_x, train_y, bb, bb_off (float64, before the int32 cast), rect_x, rect_y,
    relit: the number of object pixels of the frame whose colour under the view's light differs from the default light's by
    more than 1 level)."""
    W, H = rc.DIMS
    ref_y = rc.reference(name, kind, view, t)
    lt = lights(name, kind)[view].astype(np.float64)
    ref_x = rr.render(rr.mesh_dict(rc.arrays(name, kind)), kind, rr.scaled_K(W, H), rc.rotations(name)[view], np.array(t), W, H, rc.NEAR, rc.FAR,
                      light=tuple(lt[:3]), ambient=lt[3], diffuse=lt[4], specular=lt[5])
    assert np.array_equal(ref_x['tri'], ref_y['tri']) and ref_x['bb'] == ref_y['bb']
    x, y, w, h = ref_y['bb']
    bb_off = np.array(ref_y['bb']) + np.array([U[view, 0] * w, U[view, 1] * h, 0, 0])
    train_x = rr.extract_square_patch(ref_x['bgr'], bb_off, rc.PAD, resize=(CROP, CROP))
    depth_x = rr.extract_square_patch(ref_x['depth'], bb_off, rc.PAD, resize=(CROP, CROP))
    train_y = rr.extract_square_patch(ref_y['bgr'], ref_y['bb'], rc.PAD, resize=(CROP, CROP))
    covered = ref_y['tri'] >= 0
    relit = int((np.abs(ref_x['bgr'].astype(np.int32) - ref_y['bgr'].astype(np.int32)).max(axis=2)[covered] > 1).sum())
    return dict(train_x=train_x, mask_x=depth_x == 0., train_y=train_y, bb=ref_y['bb'], bb_off=bb_off,
                rect_x=source_rect(bb_off, ref_x['bgr'].shape), rect_y=source_rect(ref_y['bb'], ref_x['bgr'].shape), relit=relit,
                frame_x=ref_x['bgr'], depth=ref_x['depth'])


def floor_rect(ref):
    """the source rectangle a floor in place of the int32 truncation would give"""
    return source_rect(np.floor(ref['bb_off']), (rc.DIMS[1], rc.DIMS[0]))


def assert_case_is_sharp(name, kind, t):
    """What the cases are chosen for, asserted on the reference so that none can vanish silently: every view has object pixels
    that the view's light recolours by more than 1 level; at the frame's borders truncation and floor of the shifted box give
    different source rectangles, and the clipped patches are not square."""
    refs = [reference_pair(name, kind, i, t) for i in range(rc.N_ROT)]
    for i, ref in enumerate(refs):
        assert ref['relit'] > 50, (name, kind, t, i, ref['relit'])
    differ = [i for i, ref in enumerate(refs) if floor_rect(ref) != ref['rect_x']]
    if t == rc.T_BORDER:
        assert differ == [0, 3, 4]
        assert [(refs[i]['rect_x'][3], floor_rect(refs[i])[3]) for i in differ] == [(33, 32), (37, 36), (35, 34)]
    if t == T_LEFT:
        assert differ == [1, 4]
        assert [(refs[i]['rect_x'][1], floor_rect(refs[i])[1]) for i in differ] == [(34, 33), (37, 36)]
    if t in (rc.T_BORDER, T_LEFT):
        for i in differ:
            l, r, tp, b = refs[i]['rect_x']
            assert r - l != b - tp
    return refs


def check_pair(ref, train_x, mask_x, train_y, bb, visible, label=''):
    """The assertions of a pair against its reference."""
    assert visible == 1 and list(bb) == ref['bb'], label
    n_obj = {}
    for key, got in (('train_x', train_x), ('train_y', train_y)):
        want = ref[key]
        assert got.shape == want.shape == (CROP, CROP, 3) and got.dtype == np.uint8
        err = np.abs(got.astype(np.int32) - want.astype(np.int32)).max(axis=2)
        bad = int((err > 1).sum())
        n_obj[key] = int((want.max(axis=2) > 0).sum())
        print('%s: %s, %d sampled object pixels, %d differ by more than 1 level' % (label, key, n_obj[key], bad))
        assert bad <= 1e-4 * n_obj[key], '%s: %d %s pixels differ by more than 1 level' % (label, bad, key)
    mask = np.asarray(mask_x).astype(bool)
    assert mask.shape == (CROP, CROP)
    bad = int((mask != ref['mask_x']).sum())
    assert bad <= 1e-4 * int((~ref['mask_x']).sum()), '%s: %d mask pixels differ' % (label, bad)
    assert n_obj['train_x'] > 100 and n_obj['train_y'] > 100, label


# ---- tests/native/train_host.cpp ---------------------------------------------------------------------------------------
def write_scene(path, name, kind, Rs, t, lights_, offsets, crop=CROP):
    n = rc.write_scene(path, name, kind, Rs, t=t, crop=crop)
    with open(path, 'ab') as f:
        f.write(np.ascontiguousarray(lights_, dtype=np.float32).reshape(n, 6).tobytes())
        f.write(np.ascontiguousarray(offsets, dtype=np.float64).reshape(n, 2).tobytes())
    return n


def read_host_output(path, n, crop=CROP):
    raw = open(path, 'rb').read()
    out, o = [], 0
    for _ in range(n):
        v = {}
        v['train_x'] = np.frombuffer(raw, np.uint8, crop * crop * 3, o).reshape(crop, crop, 3); o += crop * crop * 3
        v['mask_x'] = np.frombuffer(raw, np.uint8, crop * crop, o).reshape(crop, crop); o += crop * crop
        v['train_y'] = np.frombuffer(raw, np.uint8, crop * crop * 3, o).reshape(crop, crop, 3); o += crop * crop * 3
        v['bb'] = np.frombuffer(raw, np.int32, 4, o).tolist(); o += 16
        v['visible'] = int(np.frombuffer(raw, np.int32, 1, o)[0]); o += 4
        r = np.frombuffer(raw, np.int32, 12, o).tolist(); o += 48
        v['bb_off'], v['rect_x'], v['rect_y'] = r[:4], tuple(r[4:8]), tuple(r[8:])
        out.append(v)
    assert o == len(raw)
    return out
