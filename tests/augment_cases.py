"""One table of augmentation cases for the host driver (test_augment_cpu.py) and the GPU (test_gpu_augment.py): ragged images
(H = 37, W = 46, C = 3: rows of 138 bytes, images of 5106 bytes, neither a multiple of 4), random uint8 objects and backgrounds,
masks with all-background, all-object and single-pixel rows, and programs whose parameters make every fp32 intermediate exact
wherever byte equality is claimed: 1 / scale in {1, 27/32, 31/32, 40/32}, factors and alphas in multiples of 1/64 between 0.5
and 2.25, Add in {-25, 0, 25, 255}.  The reference of a case is computed once and shared (reference())."""
import numpy as np

import augment_reference as ar
from augmentedautoencoder_amd import augmentation as aug

H, W, C = 37, 46, 3
N, M = 9, 7
INV_S = (1.0, 27 / 32.0, 31 / 32.0, 40 / 32.0)
ADDS = (-25, 0, 25, 255)
SIGMAS = (0.3, 0.75, 1.2)
WIDE_SIGMAS = (2.0, 4.0, 5.5)                  # k = 7, 11, 15


def make_data(shape=(H, W, C), n=N, m=M, seed=11):
    """(train_x, mask_x, train_y, bg): mask 0 of all background, mask 1 of all object, mask 2 with rows of a single pixel of each kind"""
    h, w, c = shape
    rng = np.random.RandomState(seed)
    train_x = rng.randint(0, 256, (n, h, w, c)).astype(np.uint8)
    train_y = rng.randint(0, 256, (n, h, w, c)).astype(np.uint8)
    bg = rng.randint(0, 256, (m, h, w, c)).astype(np.uint8)
    mask = rng.rand(n, h, w) < 0.5
    mask[0] = True
    mask[1] = False
    mask[2, 0::4] = False
    mask[2, 0::4, w // 3] = True
    mask[2, 2::4] = True
    mask[2, 2::4, w - 1] = False
    # extreme values where rounding and clipping bite
    train_x[min(3, n - 1), :4] = 255
    train_x[min(3, n - 1), 4:8] = 0
    bg[1, :, :3] = 255
    return train_x, mask, train_y, bg


DATA = make_data()


def _sixtyfourths(rng, n):
    return rng.randint(32, 145, n) / 64.0          # 0.5 ... 2.25


def _drop(rng, planes, size_percent, p):
    h_s, w_s = aug.dropout_grid(H, W, size_percent)
    return rng.rand(planes, h_s, w_s) < p


def _empty(pb, rng):
    pass


def _affine(pb, rng):
    for b in range(pb.B):
        pb.affine(b, INV_S[b % 4])


def _dropout(per_channel):
    def build(pb, rng):
        for b, sp in zip(range(pb.B), (0.05, 0.2, 1.0, 0.5, 0.03)):
            pb.dropout(b, _drop(rng, C if per_channel else 1, sp, 0.3))
    return build


def _blur(sigmas):
    def build(pb, rng):
        for b in range(pb.B):
            pb.blur(b, sigmas[b % len(sigmas)])
    return build


def _pointwise(name, per_channel):
    def build(pb, rng):
        for b in range(pb.B):
            n = C if per_channel else 1
            if name == 'add':
                pb.add(b, [ADDS[(b + j) % 4] for j in range(n)])
            elif name == 'invert':
                pb.invert(b, [(b + j) % 2 == 0 for j in range(n)])
            elif name == 'multiply':
                pb.multiply(b, _sixtyfourths(rng, n))
            else:
                pb.contrast(b, _sixtyfourths(rng, n))
    return build


def template_chain(pb, rng, sigma_scale=1.2):
    """the cfg template's chain with its Sometimes probabilities, parameters from the exact sets"""
    for b in range(pb.B):
        pc = lambda p: C if rng.rand() < p else 1
        if rng.rand() < 0.5:
            pb.affine(b, INV_S[rng.randint(0, 3)])                        # scale (1.0, 1.2): 1 / scale <= 1
        if rng.rand() < 0.5:
            pb.dropout(b, rng.rand(1, *aug.dropout_grid(pb.H, pb.W, 0.05)) < 0.2)
        if rng.rand() < 0.5:
            pb.blur(b, sigma_scale * rng.rand())
        if rng.rand() < 0.5:
            pb.add(b, np.array(ADDS)[rng.randint(0, 3, pc(0.3))])
        if rng.rand() < 0.3:
            pb.invert(b, rng.rand(C) < 0.2)
        if rng.rand() < 0.5:
            pb.multiply(b, _sixtyfourths(rng, pc(0.5)))
        if rng.rand() < 0.5:
            pb.multiply(b, _sixtyfourths(rng, 1))
        if rng.rand() < 0.5:
            pb.contrast(b, _sixtyfourths(rng, pc(0.3)))


def _blur_first_affine_last(pb, rng):
    # the affine widens what a left-out blur pixel reaches to at most four pixels; sigma <= 0.75 keeps the share under the cap
    for b in range(pb.B):
        pb.blur(b, (0.3, 0.75, 0.6, 0.5, 0.75)[b % 5])
        pb.multiply(b, _sixtyfourths(rng, C))
        pb.add(b, [ADDS[b % 3]])
        pb.affine(b, INV_S[1 + b % 3])


def _sixteen(pb, rng):
    for b in range(pb.B):
        pb.affine(b, INV_S[2])
        pb.add(b, [25, -25, 0])
        pb.dropout(b, _drop(rng, C, 0.2, 0.2))
        pb.multiply(b, [1.25, 0.75, 1.0])
        pb.invert(b, [True, False, True])
        pb.contrast(b, [1.5])
        pb.affine(b, INV_S[3])
        pb.add(b, [255])
        pb.invert(b, [True])
        pb.multiply(b, [0.5])
        pb.contrast(b, [0.75, 2.0, 1.0])
        pb.dropout(b, _drop(rng, 1, 0.05, 0.5))
        pb.add(b, [-25])
        pb.affine(b, INV_S[1])
        pb.blur(b, 0.75)
        pb.multiply(b, [2.25, 1.0, 0.515625])
        assert pb.n_ops[b] == 16


# name -> (batch size, builder)
CASES = {
    'empty': (5, _empty),
    'affine': (5, _affine),
    'dropout': (5, _dropout(False)),
    'dropout_per_channel': (5, _dropout(True)),
    'blur': (5, _blur(SIGMAS)),
    'blur_wide': (5, _blur(WIDE_SIGMAS)),
    'add': (5, _pointwise('add', False)),
    'add_per_channel': (5, _pointwise('add', True)),
    'invert': (5, _pointwise('invert', False)),
    'invert_per_channel': (5, _pointwise('invert', True)),
    'multiply': (5, _pointwise('multiply', False)),
    'multiply_per_channel': (5, _pointwise('multiply', True)),
    'contrast': (5, _pointwise('contrast', False)),
    'contrast_per_channel': (5, _pointwise('contrast', True)),
    'template_chain': (67, template_chain),
    'blur_first_affine_last': (5, _blur_first_affine_last),
    'sixteen_ops': (1, _sixteen),
}
BLUR_FREE = ('empty', 'affine', 'dropout', 'dropout_per_channel', 'add', 'add_per_channel', 'invert', 'invert_per_channel', 'multiply',
             'multiply_per_channel', 'contrast', 'contrast_per_channel')

_BUILT = {}


def build(name):
    """(ProgramBuilder, train_idx, bg_idx) of a case; the same object every time"""
    if name not in _BUILT:
        B, fn = CASES[name]
        seed = sorted(CASES).index(name)
        rng = np.random.RandomState(100 + seed)
        pb = aug.ProgramBuilder(B, (H, W, C))
        fn(pb, rng)
        train_idx = (np.arange(B) * 4 + seed) % N              # every mask kind appears in every case of 5
        if B >= 3:
            train_idx[:3] = (0, 1, 2)
        bg_idx = (np.arange(B) * 3 + seed) % M
        _BUILT[name] = (pb, train_idx.astype(np.int32), bg_idx.astype(np.int32))
    return _BUILT[name]


_REFS = {}


def reference(name):
    """(batch_x uint8, must-be-equal mask, batch_y uint8) of a case, computed once and read-only"""
    if name not in _REFS:
        pb, ti, bi = build(name)
        out = ar.reference_batch(DATA[0], DATA[1], DATA[2], DATA[3], ti, bi, pb.programs)
        for a in out:
            a.setflags(write=False)
        _REFS[name] = out
    return _REFS[name]


def check(name, got_u8, got_x=None, got_y=None):
    ref, sure, ref_y = reference(name)
    left_out, _ = ar.check_batch(got_u8, ref, sure, name)
    if name in BLUR_FREE:
        assert sure.all() and np.array_equal(got_u8, ref), name
    if got_x is not None:
        assert got_x.dtype == np.float32 and got_x.tobytes() == ar.unit_f32(got_u8).tobytes(), name
    if got_y is not None:
        assert got_y.dtype == np.float32 and got_y.tobytes() == ar.unit_f32(ref_y).tobytes(), name
    return left_out


# ---- the file the host driver reads, and what it writes ---------------------------------------------------------------------
def write_input(path, data, train_idx, bg_idx, pb):
    train_x, mask_x, train_y, bg = data
    aux = pb.aux
    with open(path, 'wb') as f:
        f.write(np.array([len(train_x), len(bg), pb.H, pb.W, pb.C, pb.B, len(aux)], dtype=np.int32).tobytes())
        for a in (train_x, mask_x.astype(np.uint8), train_y, bg, train_idx.astype(np.int32), bg_idx.astype(np.int32), pb.n_ops, pb.ops, aux):
            f.write(np.ascontiguousarray(a).tobytes())


def read_output(path, pb):
    n = pb.B * pb.H * pb.W * pb.C
    raw = np.fromfile(path, dtype=np.uint8)
    assert len(raw) == 9 * n, 'host driver wrote %d bytes, %d expected' % (len(raw), 9 * n)
    shape = (pb.B, pb.H, pb.W, pb.C)
    return raw[:n].reshape(shape), raw[n:5 * n].view(np.float32).reshape(shape), raw[5 * n:].view(np.float32).reshape(shape)
