"""Golden fixture for the random draws and the patch rectangles of the training set, produced by running the REFERENCE's own
loop:

    auto_pose/ae/dataset.py                       Dataset.render_training_images (:219-306), extract_square_patch (:354-373)
    auto_pose/ae/pysixd_stuff/transform.py        random_rotation_matrix (:1463-1503)
    auto_pose/ae/pysixd_stuff/view_sampler.py     calc_2d_bbox (:10-15)

The modules are loaded from where they lie (as make_codebook_logic_golden.py loads them); cv2 and progressbar are stand-ins and
np.float is restored for NumPy 2.  What cannot run here is the OpenGL renderer, so the Dataset gets a stand-in of this file's
on `_cache_renderer`: it consumes np.random exactly as a render call with random_light does (three numbers for the position,
one per perturbed constant: diffuse and specular for 'reconst', ambient too for 'cad'), records the rotation and the light it
was called with, and returns a frame whose pixel values encode their own coordinates.  The stand-in cv2.resize then reads, from
the corner of the patch it is handed, the rectangle extract_square_patch cut.  What is recorded is therefore the reference's
behaviour from "np.random" to "rotation, light, shifted box, three source rectangles" -- the boundary the rasteriser replaces.

Run where the reference tree lies (REF below); the tests read only the fixture:
    python tests/golden/make_training_draws_golden.py     ->  tests/golden/training_draws_ref.npz
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = '/root/reference/auto_pose'
W, H = 160, 120
CROP = 32
N_IMGS = 8
SEEDS = (1, 7, 2024)
KW = {'h': str(CROP), 'w': str(CROP), 'c': '3', 'render_dims': '(%d, %d)' % (W, H),
      'k': '[1075.65*160/720, 0, 160/2, 0, 1073.90*120/540, 120/2, 0, 0, 1]', 'clip_near': '10', 'clip_far': '10000', 'pad_factor': '1.2',
      'max_rel_offset': '0.2', 'radius': '700'}

PATCHES = []                                     # (left, right, top, bottom) of every patch cv2.resize was handed, in call order


def _resize(src, dsize, interpolation=None):
    """stand-in for cv2.resize: records the rectangle the patch was cut from and returns a blank image of the asked size"""
    code = abs(float(src[0, 0, 2] if src.ndim == 3 else src[0, 0])) - 1
    top, left = int(code) // W, int(code) % W
    PATCHES.append((left, left + src.shape[1], top, top + src.shape[0]))
    return np.zeros((dsize[1], dsize[0]) + src.shape[2:], dtype=src.dtype)


class _Widget(object):
    def __init__(self, *a, **kw):
        pass

    def start(self):
        pass

    def update(self, i):
        pass

    def finish(self):
        pass


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load_reference_modules():
    if not hasattr(np, 'float'):
        np.float = float                          # the reference predates NumPy 1.24
    _stub('cv2', INTER_NEAREST=0, INTER_LINEAR=1, INTER_CUBIC=2, INTER_AREA=3, resize=_resize)
    _stub('progressbar', Percentage=_Widget, Bar=_Widget, Counter=_Widget, ETA=_Widget, ProgressBar=_Widget)
    for pkg, path in (('auto_pose', REF), ('auto_pose.ae', REF + '/ae'), ('auto_pose.ae.pysixd_stuff', REF + '/ae/pysixd_stuff')):
        p = types.ModuleType(pkg)
        p.__path__ = [path]                       # a package shell: the real __init__ is NOT run
        sys.modules[pkg] = p
    mods = {}
    for name, rel in (('auto_pose.ae.utils', 'ae/utils.py'),
                      ('auto_pose.ae.pysixd_stuff.transform', 'ae/pysixd_stuff/transform.py'),
                      ('auto_pose.ae.pysixd_stuff.view_sampler', 'ae/pysixd_stuff/view_sampler.py'),
                      ('auto_pose.ae.dataset', 'ae/dataset.py')):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        mods[name.rsplit('.', 1)[1]] = m
    return mods


class StandInRenderer(object):
    """render() of the two OpenGL renderers as far as np.random and the caller can tell"""

    def __init__(self, kind):
        self.kind = kind
        self.calls = []                           # (R, random_light, light position or None, ambient, diffuse, specular)

    def render(self, obj_id, W, H, K, R, t, near, far, random_light=False):
        W, H = int(W), int(H)
        if random_light:
            pos = 1000. * np.random.random(3)
            ambient = 0.4 + 0.1 * (2 * np.random.rand() - 1) if self.kind == 'cad' else 0.4
            diffuse = 0.8 + 0.1 * (2 * np.random.rand() - 1)
            specular = 0.3 + 0.1 * (2 * np.random.rand() - 1)
        else:
            pos, ambient, diffuse, specular = np.array([400., 400., 400.]), 0.4, 0.8, 0.3
        self.calls.append((np.array(R), bool(random_light), pos, ambient, diffuse, specular))
        # the "object": a box placed by the rotation, many of them across a border of the frame
        bw, bh = 40 + int(200 * abs(R[0, 1])), 40 + int(200 * abs(R[1, 2]))
        cx, cy = int(W / 2 + 0.5 * W * R[0, 2]), int(H / 2 + 0.5 * H * R[1, 0])
        x0, x1 = max(cx - bw // 2, 0), min(cx + bw // 2, W - 1)
        y0, y1 = max(cy - bh // 2, 0), min(cy + bh // 2, H - 1)
        code = 1.0 + np.arange(H)[:, None] * W + np.arange(W)[None, :]          # pixel (x, y) holds 1 + y W + x ...
        inside = np.zeros((H, W), dtype=bool)
        inside[y0:y1 + 1, x0:x1 + 1] = True
        depth = np.where(inside, code, -code)                                    # ... negated outside the object: depth > 0 is the object
        bgr = np.stack([np.zeros((H, W)), np.zeros((H, W)), code], axis=-1)
        return bgr, depth


def main():
    mods = load_reference_modules()
    Dataset, view_sampler = mods['dataset'].Dataset, mods['view_sampler']
    out = {'render_dims': np.array([W, H]), 'pad_factor': np.float64(KW['pad_factor']), 'max_rel_offset': np.float64(KW['max_rel_offset']),
           'noof_training_imgs': np.int64(N_IMGS), 'seeds': np.array(SEEDS)}
    for kind in ('reconst', 'cad'):
        for seed in SEEDS:
            ds = object.__new__(Dataset)
            ds._kw = dict(KW, model=kind)
            ds.shape = (CROP, CROP, 3)
            ds.noof_training_imgs = N_IMGS
            ds.train_x = np.empty((N_IMGS, CROP, CROP, 3), dtype=np.uint8)
            ds.mask_x = np.empty((N_IMGS, CROP, CROP), dtype=bool)
            ds.train_y = np.empty((N_IMGS, CROP, CROP, 3), dtype=np.uint8)
            ds._cache_renderer = StandInRenderer(kind)
            del PATCHES[:]
            np.random.seed(seed)
            ds.render_training_images()
            next_rand = np.random.rand()
            calls = ds._cache_renderer.calls
            assert len(calls) == 2 * N_IMGS and len(PATCHES) == 3 * N_IMGS
            key = '%s_%d_' % (kind, seed)
            xs, ys = calls[0::2], calls[1::2]
            assert all(c[1] for c in xs) and not any(c[1] for c in ys) and all(np.array_equal(a[0], b[0]) for a, b in zip(xs, ys))
            out[key + 'R'] = np.array([c[0] for c in xs])
            out[key + 'light'] = np.array([list(c[2]) + [c[3], c[4], c[5]] for c in xs])
            rects = np.array(PATCHES, dtype=np.int64).reshape(N_IMGS, 3, 4)
            out[key + 'rects'] = rects
            # the true box of every image, from the same stand-in frame through the reference's calc_2d_bbox, and the shift the
            # loop added to it: x' - x and y' - y are not recorded by the loop, so they are recomputed from the recorded state
            np.random.seed(seed)
            bbs, trans = [], []
            probe = StandInRenderer(kind)
            for i in range(N_IMGS):
                R = mods['transform'].random_rotation_matrix()[:3, :3]
                _, depth = probe.render(0, W, H, None, R, None, 10, 10000, random_light=True)
                yy, xx = np.nonzero(depth > 0)
                bb = view_sampler.calc_2d_bbox(xx, yy, (W, H))
                m = float(KW['max_rel_offset'])
                trans.append([np.random.uniform(-m, m) * bb[2], np.random.uniform(-m, m) * bb[3]])
                bbs.append(bb)
            assert np.random.rand() == next_rand                               # the replay consumed what the loop consumed
            out[key + 'bb'] = np.array(bbs, dtype=np.int64)
            out[key + 'trans'] = np.array(trans)
            out[key + 'next_rand'] = np.float64(next_rand)
            # the replay is the loop: its boxes reproduce the recorded rectangles through the reference's extract_square_patch
            for i in range(N_IMGS):
                del PATCHES[:]
                frame = probe.render(0, W, H, None, out[key + 'R'][i], None, 10, 10000)[0]
                ds.extract_square_patch(frame, np.array(bbs[i]) + np.array([trans[i][0], trans[i][1], 0, 0]), float(KW['pad_factor']), resize=(CROP, CROP))
                ds.extract_square_patch(frame, bbs[i], float(KW['pad_factor']), resize=(CROP, CROP))
                assert PATCHES[0] == tuple(rects[i, 0]) == tuple(rects[i, 1]) and PATCHES[1] == tuple(rects[i, 2])
    here = os.path.dirname(os.path.abspath(__file__))
    np.savez_compressed(os.path.join(here, 'training_draws_ref.npz'), **out)
    for k, v in out.items():
        print(k, getattr(v, 'shape', ()), getattr(v, 'dtype', type(v)))


if __name__ == '__main__':
    main()
