"""Training batches without a GPU: csrc/kernels/augment_core.h compiled for the host and driven by tests/native/augment_host.cpp
over the table of tests/augment_cases.py against the NumPy float64 restatement (tests/augment_reference.py, itself cross-checked
against scipy.ndimage); the same driver under -fsanitize=address,undefined; the CODE parser, the draws, load_bg_images, the /255
values, the np.random order of Dataset.batch and the refusals."""
import configparser
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import augment_cases as ac
import augment_reference as ar
from test_render_cpu import _compiler
from augmentedautoencoder_amd import _lib, augmentation as aug
from augmentedautoencoder_amd.dataset import Dataset

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

TEMPLATE_CODE = """Sequential([
	#Sometimes(0.5, PerspectiveTransform(0.05)),
	#Sometimes(0.5, CropAndPad(percent=(-0.05, 0.1))),
	Sometimes(0.5, Affine(scale=(1.0, 1.2))),
	Sometimes(0.5, CoarseDropout( p=0.2, size_percent=0.05) ),
	Sometimes(0.5, GaussianBlur(1.2*np.random.rand())),
    Sometimes(0.5, Add((-25, 25), per_channel=0.3)),
    Sometimes(0.3, Invert(0.2, per_channel=True)),
    Sometimes(0.5, Multiply((0.6, 1.4), per_channel=0.5)),
    Sometimes(0.5, Multiply((0.6, 1.4))),
    Sometimes(0.5, ContrastNormalization((0.5, 2.2), per_channel=0.3))
	], random_order=False)"""


def _build(out_dir, flags, name):
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-O2', '-ffp-contract=off', '-Wall'] + flags + [os.path.join(HERE, 'native', 'augment_host.cpp'), '-o', exe])
    return exe


@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('augment_host'), [], 'augment_host')


def _run(exe, tmp_path, data, ti, bi, pb):
    src, out = str(tmp_path / 'aug_in.bin'), str(tmp_path / 'aug_out.bin')
    ac.write_input(src, data, ti, bi, pb)
    subprocess.check_call([exe, src, out])
    return ac.read_output(out, pb)


# ---- the reference against scipy ------------------------------------------------------------------------------------------------
def test_reference_blur_and_affine_equal_scipy():
    import scipy.ndimage as ndi
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, (ac.H, ac.W, ac.C)).astype(np.float64)
    for sigma in ac.SIGMAS + ac.WIDE_SIGMAS:
        k = aug.blur_kernel_size(sigma)
        w = aug.gaussian_weights(k, sigma).astype(np.float64)
        real = ar.blur_real(img, w)
        for c in range(ac.C):
            assert np.abs(real[..., c] - ndi.correlate(img[..., c], np.outer(w, w), mode='mirror')).max() < 1e-9
    for inv_s in ac.INV_S + (1.7, 0.31):                     # 40/32 and 1.7: scale < 1, border pixels blend with the constant 0
        real = ar.affine_real(img, inv_s)
        inv = float(np.float32(inv_s))
        centre = np.array([(ac.H - 1) / 2.0, (ac.W - 1) / 2.0])
        for c in range(ac.C):
            want = ndi.affine_transform(img[..., c], [inv, inv], offset=centre - centre * inv, order=1, mode='grid-constant', cval=0.0)
            assert np.abs(real[..., c] - want).max() < 1e-9
        if inv_s == 40 / 32.0:                                    # column 4 samples x = -0.625: 0.375 of column 0 blended with the constant 0
            assert real[5:-5, 4].any() and real[:, 4].max() <= 0.375 * 255 and not real[:, 3].any()


def test_reference_rounding_and_reflection():
    assert ar.round_u8(np.array([0.5, 1.5, 2.5, 254.5, 255.5, 300.0, -0.5, -7.0, 127.49999])).tolist() == [0, 2, 2, 254, 255, 255, 0, 0, 127]
    assert ar.reflect101(np.array([-3, -1, 0, 4, 5, 7]), 5).tolist() == [3, 1, 0, 4, 3, 1]
    assert aug.blur_kernel_size(0.3) == aug.blur_kernel_size(1.2) == 5
    assert [aug.blur_kernel_size(s) for s in ac.WIDE_SIGMAS] == [7, 11, 15]
    assert aug.nearest_table(8, 3).tolist() == [0, 0, 0, 1, 1, 1, 2, 2] and aug.dropout_grid(128, 128, 0.05) == (6, 6) and aug.dropout_grid(10, 10, 0.01) == (1, 1)


# ---- the core header on the host ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(ac.CASES))
def test_host_driver_matches_reference(host_exe, tmp_path, name):
    pb, ti, bi = ac.build(name)
    u8, x, y = _run(host_exe, tmp_path, ac.DATA, ti, bi, pb)
    left_out = ac.check(name, u8, x, y)
    print('%s: %.3f %% left out' % (name, 100 * left_out))
    if name == 'empty':
        assert np.array_equal(u8, ar.composite(ac.DATA[0][ti], ac.DATA[1][ti], ac.DATA[3][bi]))
        assert np.array_equal(u8[0], ac.DATA[3][bi[0]]) and np.array_equal(u8[1], ac.DATA[0][1])      # all background, all object


def test_cases_cover_what_they_claim():
    assert (ac.H * ac.W * ac.C) % 4 and (ac.W * ac.C) % 4
    m = ac.DATA[1]
    assert m[0].all() and not m[1].any() and (m[2].sum(axis=1) == 1).any() and (m[2].sum(axis=1) == ac.W - 1).any()
    assert {ac.CASES[n][0] for n in ac.CASES} == {1, 5, 67}
    assert ac.build('sixteen_ops')[0].n_ops.tolist() == [16]
    chain = ac.build('template_chain')[0]
    names = {op[0] for prog in chain.programs for op in prog}
    assert names == {'affine', 'dropout', 'blur', 'add', 'invert', 'multiply', 'contrast'} and chain.n_ops.min() <= 1 and chain.n_ops.max() >= 7
    assert [p[0][0] for p in ac.build('blur_first_affine_last')[0].programs] == ['blur'] * 5
    assert [p[-1][0] for p in ac.build('blur_first_affine_last')[0].programs] == ['affine'] * 5
    # a blurred case does leave pixels out, and the reference stays inside the cap on its own
    for name in ('blur', 'blur_wide', 'blur_first_affine_last', 'template_chain'):
        sure = ac.reference(name)[1]
        assert 0.0 < 1.0 - sure.mean() <= ar.LEFT_OUT_CAP, name


def test_host_driver_under_sanitizers(tmp_path):
    """address + undefined-behaviour sanitizers on the stand-alone driver: ragged sizes, every op, and programs whose aux offsets,
    indices and op counts point outside (skipped, as the kernel skips them)"""
    exe = _build(tmp_path, ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'], 'augment_host_san')
    for name in ('sixteen_ops', 'blur_wide', 'dropout_per_channel'):
        pb, ti, bi = ac.build(name)
        ac.check(name, *_run(exe, tmp_path, ac.DATA, ti, bi, pb))
    pb = aug.ProgramBuilder(5, (ac.H, ac.W, ac.C))
    for b in range(4):
        pb.blur(b, 1.2)
        pb.dropout(b, np.ones((1, 3, 3), dtype=bool))
        pb.affine(b, 1.0)
    pb.dropout(4, np.ones((3, 5, 5), dtype=bool))             # valid ranges, but a row table and a plane stride of garbage
    pb.ops['i'][0, 0, 1] = len(pb.aux) - 2                    # weights run past the pool
    pb.ops['i'][0, 1, 0] = 1 << 30                            # mask bits far outside
    pb.multiply(0, [1.0])
    pb.ops['f'][0, 3] = (np.nan, np.inf, -np.inf)             # non-finite factors (the builder refuses them; a device-resident program may hold them)
    pb.ops['i'][1, 0, 0] = 17                                 # k over the limit
    pb.ops['i'][1, 1, 1] = -5                                 # negative table offset
    pb.ops['f'][1, 2, 0] = np.nan
    pb.ops['code'][2, 0] = 99
    pb.n_ops[2] = 40
    aux = pb.aux.copy()
    r0 = pb.ops['i'][4, 0, 1]
    aux[r0:r0 + ac.H] = (0x7FFFFFFF, 0xFFFFFFFF, 0x80000000, 12345678) * 9 + (7 << 20,)
    pb._aux = [aux]
    pb.ops['i'][4, 0, 3] = 0x7FFFFFFF
    ti, bi = np.array([3, 4, 5, 99, 6], dtype=np.int32), np.array([0, 1, -1, 2, 3], dtype=np.int32)
    u8, x, y = _run(exe, tmp_path, ac.DATA, ti, bi, pb)
    assert (u8[2:4] == 0xA5).all() and (x[2:4].view(np.uint32) == 0xA5A5A5A5).all()                    # out-of-range images stay unwritten
    base = ar.composite(ac.DATA[0][3], ac.DATA[1][3], ac.DATA[3][0])                                  # both bad ops skipped, affine at 1 is the identity
    assert not u8[0][..., 0].any() and not u8[0][..., 2].any()                                         # x * NaN and x * -inf clip to 0
    assert np.array_equal(u8[0][..., 1], np.where(base[..., 1] > 0, 255, 0))                           # x * inf: 255, and 0 * inf = NaN -> 0
    assert not u8[1].any()                                                                              # NaN scale: every sample is outside
    kept = ar.composite(ac.DATA[0][6], ac.DATA[1][6], ac.DATA[3][3])                                  # garbage bit indices wrap in uint32: whichever bit
    assert ((u8[4] == kept) | (u8[4] == 0)).all() and (u8[4] == kept).mean() > 0.5                    # they name, a pixel is kept or dropped, nothing else


def test_unit_table_is_float32_of_v_over_255(host_exe, tmp_path):
    out = str(tmp_path / 'unit.bin')
    subprocess.check_call([host_exe, '--unit', out])
    got = np.fromfile(out, dtype=np.float32)
    assert got.tobytes() == np.float32(np.arange(256) / 255.).tobytes()
    assert got.tobytes() == ar.unit_f32(np.arange(256, dtype=np.uint8)).tobytes()


# ---- the parser -------------------------------------------------------------------------------------------------------------------
def test_parse_the_template_verbatim():
    np.random.seed(4)
    plan = aug.parse_code(TEMPLATE_CODE)
    np.random.seed(4)
    sigma = 1.2 * np.random.rand()
    assert [a['name'] for a in plan] == ['Affine', 'CoarseDropout', 'GaussianBlur', 'Add', 'Invert', 'Multiply', 'Multiply', 'ContrastNormalization']
    assert [a['sometimes'] for a in plan] == [0.5, 0.5, 0.5, 0.5, 0.3, 0.5, 0.5, 0.5]
    assert [a['per_channel'] for a in plan] == [0.0, 0.0, 0.0, 0.3, 1.0, 0.5, 0.0, 0.3]
    assert plan[0]['args'] == {'scale': (1.0, 1.2)} and plan[1]['args'] == {'p': 0.2, 'size_percent': 0.05}
    assert plan[2]['args'] == {'sigma': sigma}                           # drawn once, at parse time
    assert plan[3]['args'] == {'value': (-25, 25)} and plan[4]['args'] == {'p': 0.2}
    assert plan[5]['args'] == plan[6]['args'] == {'mul': (0.6, 1.4)} and plan[7]['args'] == {'alpha': (0.5, 2.2)}


def test_parse_forms():
    plan = aug.parse_code('Sequential([GaussianBlur(sigma=(0.0, 3.0/2)), Sometimes(0.25, Add(value=-(2+3)*2, per_channel=False)), iaa.Multiply(1.5)])')
    assert [a['sometimes'] for a in plan] == [None, 0.25, None]
    assert plan[0]['args'] == {'sigma': (0.0, 1.5)} and plan[1]['args'] == {'value': -10} and plan[1]['per_channel'] == 0.0 and plan[2]['args'] == {'mul': 1.5}
    np.random.seed(1)
    a = aug.parse_code('Sequential([Multiply(0.5 + np.random.rand() / 2)])')[0]['args']['mul']
    np.random.seed(1)
    assert a == 0.5 + np.random.rand() / 2


@pytest.mark.parametrize('code,word', [
    ('Sequential([Add(1)], random_order=True)', 'random_order'),
    ('Sequential([Sometimes(0.5, PerspectiveTransform(0.05))])', 'PerspectiveTransform'),
    ('Sequential([CropAndPad(percent=(-0.05, 0.1))])', 'CropAndPad'),
    ('Sequential([Affine(rotate=(-10, 10))])', 'rotate'),
    ('Sequential([Affine(scale=1.1, order=0)])', 'order'),
    ('Sequential([CoarseDropout(p=0.2, size_px=4)])', 'size_px'),
    ('Sequential([CoarseDropout(p=0.2)])', 'size_percent'),
    ('Sequential([Add(1)], deterministic=True)', 'deterministic'),
    ('SomeOf(2, [Add(1)])', 'SomeOf'),
    ('Sequential([Sometimes(0.5, Add(1), Add(2))])', 'Sometimes'),
])
def test_parse_refusals_name_what_is_missing(code, word):
    with pytest.raises(NotImplementedError, match=word):
        aug.parse_code(code)


def test_parse_executes_nothing():
    for code in ('Sequential([Add(__import__("os").getpid())])', 'Sequential([Add(np.random.seed(1))])', 'Sequential([Add(np.random.rand(3))])',
                 'Sequential([Add((1, 2, 3))])', 'Sequential([Sometimes(1.5, Add(1))])', 'Sequential([Add(1, per_channel=2)])'):
        with pytest.raises(ValueError):
            aug.parse_code(code)


# ---- the draws --------------------------------------------------------------------------------------------------------------------
def test_sometimes_coins_and_ranges():
    plan = aug.parse_code('Sequential([Sometimes(0.5, Affine(scale=(1.0, 1.2))), Sometimes(0.5, Add((-25, 25), per_channel=0.3)), '
                          'Sometimes(0.5, Multiply((0.6, 1.4), per_channel=0.5)), Sometimes(0.5, ContrastNormalization((0.5, 2.2))), '
                          'Sometimes(0.3, Invert(0.2, per_channel=True))])')
    np.random.seed(7)
    pb = aug.draw_programs(plan, 4000, (8, 8, 3))
    ops = [op for prog in pb.programs for op in prog]
    by = lambda name: [op for op in ops if op[0] == name]
    for name, p in (('affine', 0.5), ('add', 0.5), ('multiply', 0.5), ('contrast', 0.5)):
        assert abs(len(by(name)) / 4000.0 - p) < 0.04, name
    assert abs(len(by('invert')) / 4000.0 - 0.3) < 0.04
    inv_s = np.array([op[1] for op in by('affine')])
    assert (inv_s >= np.float32(1 / 1.2) - 1e-6).all() and (inv_s <= 1.0).all() and inv_s.std() > 0.01
    adds = np.array([op[1] for op in by('add')])
    assert adds.min() == -25 and adds.max() == 25 and (adds == np.rint(adds)).all() and len(np.unique(adds)) == 51
    shared = (adds[:, 0] == adds[:, 1]) & (adds[:, 1] == adds[:, 2])
    assert abs((~shared).mean() - 0.3) < 0.05                             # the per_channel coin; a false coin shares one value
    mul = np.array([op[1] for op in by('multiply')])
    assert (mul >= np.float32(0.6)).all() and (mul <= np.float32(1.4)).all()
    assert abs((mul[:, 0] != mul[:, 1]).mean() - 0.5) < 0.05
    con = np.array([op[1] for op in by('contrast')])
    assert (con >= 0.5).all() and (con <= np.float32(2.2)).all() and (con[:, 0] == con[:, 2]).all()
    flags = np.array([op[1] for op in by('invert')])
    assert abs(flags.mean() - 0.2) < 0.03 and (flags[:, 0] != flags[:, 1]).any()


def test_dropout_cells_and_tables():
    plan = aug.parse_code('Sequential([CoarseDropout(p=0.2, size_percent=0.05), CoarseDropout(p=(0.4, 0.6), size_percent=(0.1, 0.5), per_channel=True)])')
    np.random.seed(3)
    pb = aug.draw_programs(plan, 300, (128, 128, 3))
    first = np.array([prog[0][1] for prog in pb.programs])
    assert first.shape == (300, 1, 6, 6) and abs(first.mean() - 0.2) < 0.02             # h_s = max(1, int(128 * 0.05)) = 6; Bernoulli(1 - p) keeps
    second = [prog[1][1] for prog in pb.programs]
    assert all(m.shape[0] == 3 and 12 <= m.shape[1] <= 64 and m.shape[1] == m.shape[2] for m in second)
    assert abs(np.mean([m.mean() for m in second]) - 0.5) < 0.03
    rows = pb.programs[0][0][2]
    assert rows.tolist() == aug.nearest_table(128, 6).tolist() and rows.max() == 5 and (np.diff(rows) >= 0).all()
    op = pb.ops[0, 0]
    aux = pb.aux
    assert op['code'] == _lib.AAE_AUGMENT_DROPOUT and op['i'][3] == 0
    assert aux[op['i'][1]:op['i'][1] + 128].tolist() == (rows * 6).tolist() and aux[op['i'][2]:op['i'][2] + 128].tolist() == rows.tolist()
    bits = np.unpackbits(aux[op['i'][0]:op['i'][0] + 2].view(np.uint8), bitorder='little')[:36]
    assert bits.astype(bool).tolist() == first[0].reshape(-1).tolist()
    assert pb.ops[0, 1]['i'][3] == second[0].shape[1] * second[0].shape[2]


def test_draws_are_reproducible_and_documented_order():
    plan = aug.parse_code('Sequential([Sometimes(0.5, Multiply((0.6, 1.4), per_channel=0.5))])')
    np.random.seed(11)
    pb = aug.draw_programs(plan, 6, (8, 8, 3))
    np.random.seed(11)
    want = []
    for b in range(6):
        if not np.random.rand() < 0.5:
            want.append(None)
            continue
        n = 3 if np.random.rand() < 0.5 else 1
        want.append(np.float32(np.random.uniform(0.6, 1.4, size=n)))
    for prog, w in zip(pb.programs, want):
        assert (prog == []) if w is None else np.array_equal(np.float32(prog[0][1]), np.resize(w, 3))
    assert len(pb.aux) == 0


def test_builder_refusals():
    pb = aug.ProgramBuilder(1, (16, 16, 3))
    with pytest.raises(NotImplementedError, match='kernel size'):
        pb.blur(0, 7.0)
    with pytest.raises(ValueError, match='kernel size'):
        aug.ProgramBuilder(1, (2, 16, 3)).blur(0, 1.0)
    pb.blur(0, 0.0)
    assert pb.n_ops[0] == 0                                        # sigma = 0 is the identity: no op
    for _ in range(16):
        pb.add(0, [1])
    with pytest.raises(ValueError, match='more than 16'):
        pb.add(0, [1])
    with pytest.raises(NotImplementedError, match='C = 4'):
        aug.ProgramBuilder(1, (8, 8, 4))
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match='finite'):
            aug.ProgramBuilder(1, (8, 8, 3)).multiply(0, [1.0, bad, 1.0])
        with pytest.raises(ValueError, match='finite'):
            aug.ProgramBuilder(1, (8, 8, 3)).contrast(0, [bad])
    with pytest.raises(ValueError, match='limit of 81920'):
        aug.check_image_bytes((166, 166, 3))
    aug.check_image_bytes((128, 128, 3))
    assert aug.MAX_IMAGE_BYTES == 81920


# ---- Dataset ----------------------------------------------------------------------------------------------------------------------
def _png(path, rgb):
    from PIL import Image
    Image.fromarray(rgb, 'RGB').save(path)


def test_load_bg_images(tmp_path, monkeypatch, capsys):
    rng = np.random.RandomState(2)
    src = tmp_path / 'bg'
    src.mkdir()
    imgs = {}
    for i, (h, w) in enumerate([(20, 30), (16, 12), (8, 40), (12, 16), (40, 40)]):
        imgs['b%d.png' % i] = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        _png(str(src / ('b%d.png' % i)), imgs['b%d.png' % i])
    pattern = str(src / '*.png')
    ds = Dataset(str(tmp_path), h=12, w=16, c=3, background_images_glob=pattern, noof_bg_imgs=4)
    assert ds.noof_bg_imgs == 4 and Dataset('', h=1, w=1, c=1, background_images_glob=pattern, noof_bg_imgs=50).noof_bg_imgs == 5
    random.seed(5)
    np.random.seed(6)
    path = ds.load_bg_images(str(tmp_path))
    assert os.path.basename(path) == hashlib.md5((str((12, 16, 3)) + '4' + pattern).encode('utf-8')).hexdigest() + '.npy'
    # replay: the reference's order of random.shuffle and the two np.random.rand() per file
    files = ds.bg_img_paths[:4]
    random.seed(5)
    random.shuffle(files)
    np.random.seed(6)
    small = 0
    for j, f in enumerate(files):
        rgb = imgs[os.path.basename(f)]
        Hh, Ww = rgb.shape[:2]
        ya, xa = int(np.random.rand() * (Hh - 12)), int(np.random.rand() * (Ww - 16))
        cut = rgb[ya:ya + 12, xa:xa + 16]
        if cut.shape[:2] != (12, 16):
            small += 1
            assert not ds.bg_imgs[j].any()                       # too small: left zero
        else:
            assert np.array_equal(ds.bg_imgs[j], cut[:, :, ::-1])        # BGR
    assert ds.bg_imgs.shape == (4, 12, 16, 3) and ds.bg_imgs.dtype == np.uint8
    assert np.random.rand() == np.random.RandomState(6).rand(9)[8]
    # load-if-present: no decoder is touched
    again = Dataset(str(tmp_path), h=12, w=16, c=3, background_images_glob=pattern, noof_bg_imgs=4)
    import PIL.Image
    monkeypatch.setattr(PIL.Image, 'open', lambda *a, **k: pytest.fail('the load-if-present branch decoded a file'))
    again.load_bg_images(str(tmp_path))
    assert np.array_equal(again.bg_imgs, ds.bg_imgs)
    assert small >= 1                                             # b2.png (8 rows) or b1.png (12 columns) is among any four of the five


def test_load_bg_images_leaves_small_files_zero(tmp_path):
    _png(str(tmp_path / 'tiny.png'), np.full((5, 5, 3), 200, dtype=np.uint8))
    _png(str(tmp_path / 'exact.png'), np.dstack([np.full((12, 16), v, dtype=np.uint8) for v in (10, 20, 30)]))
    ds = Dataset(str(tmp_path), h=12, w=16, c=3, background_images_glob=str(tmp_path / '*.png'), noof_bg_imgs=2)
    ds.load_bg_images(str(tmp_path))
    sums = sorted(int(b.sum()) for b in ds.bg_imgs)
    assert sums[0] == 0 and sums[1] == 12 * 16 * 60
    kept = ds.bg_imgs[np.argmax([b.sum() for b in ds.bg_imgs])]
    assert kept[0, 0].tolist() == [30, 20, 10]                       # R = 10, G = 20, B = 30 on disk
    with pytest.raises(NotImplementedError, match='C = 1'):
        Dataset(str(tmp_path), h=12, w=16, c=1, background_images_glob=str(tmp_path / '*.png'), noof_bg_imgs=2).load_bg_images(str(tmp_path))


def _memory_dataset(**over):
    kw = dict(h=ac.H, w=ac.W, c=ac.C, code=TEMPLATE_CODE, realistic_occlusion='False', square_occlusion='False', noof_training_imgs=ac.N)
    kw.update(over)
    ds = Dataset('', **kw)
    ds.train_x, ds.mask_x, ds.train_y, ds.bg_imgs = ac.DATA
    return ds


def test_batch_consumes_np_random_in_the_reference_order():
    np.random.seed(21)
    ds = _memory_dataset()
    ti, bi, pb = ds._draw_batch(5)
    after = np.random.rand()
    np.random.seed(21)
    want_ti = np.random.choice(ac.N, 5, replace=False)            # dataset.py:461
    want_bi = np.random.choice(ac.M, 5, replace=False)            # dataset.py:465
    plan = aug.parse_code(TEMPLATE_CODE)                           # dataset.py:488 touches the lazy _aug: the blur's np.random.rand() is drawn here, on the first batch
    want = aug.draw_programs(plan, 5, (ac.H, ac.W, ac.C))
    assert np.array_equal(ti, want_ti) and np.array_equal(bi, want_bi)
    assert pb.ops.tobytes() == want.ops.tobytes() and pb.n_ops.tolist() == want.n_ops.tolist() and pb.aux.tobytes() == want.aux.tobytes()
    assert after == np.random.rand()
    # the second batch parses nothing: choice, choice, draws
    np.random.seed(22)
    ti2, bi2, pb2 = ds._draw_batch(5)
    np.random.seed(22)
    assert np.array_equal(ti2, np.random.choice(ac.N, 5, replace=False)) and np.array_equal(bi2, np.random.choice(ac.M, 5, replace=False))
    assert pb2.ops.tobytes() == aug.draw_programs(plan, 5, (ac.H, ac.W, ac.C)).ops.tobytes()
    with pytest.raises(ValueError):
        ds._draw_batch(ac.N + 1)                                     # choice(..., replace=False) of more than there are, as in the reference


def test_occlusion_switches_and_unknown_augmenters_are_refused():
    for key, value in (('realistic_occlusion', '0.25'), ('square_occlusion', 'True'), ('square_occlusion', '0.25')):
        with pytest.raises(NotImplementedError, match=key.upper()):
            _memory_dataset(**{key: value})._draw_batch(2)
    with pytest.raises(NotImplementedError, match='PerspectiveTransform'):
        _memory_dataset(code='Sequential([Sometimes(0.5, PerspectiveTransform(0.05))])')._draw_batch(2)
    ds = _memory_dataset(realistic_occlusion='0', square_occlusion='0.0')
    assert len(ds._draw_batch(2)[0]) == 2


def test_build_dataset_hands_the_augmentation_keys_through(tmp_path):
    from augmentedautoencoder_amd import ae_factory as factory
    args = configparser.ConfigParser()
    args.read_string('[Paths]\nBACKGROUND_IMAGES_GLOB: %s\n[Dataset]\nH: 12\nW: 16\nC: 3\nNOOF_BG_IMGS: 15000\n[Augmentation]\n'
                     'REALISTIC_OCCLUSION: False\nSQUARE_OCCLUSION: False\nCODE: %s\n' % (str(tmp_path / '*.jpg'), TEMPLATE_CODE.replace('\n', '\n\t')))
    ds = factory.build_dataset(str(tmp_path), args)
    assert ds.noof_bg_imgs == 0 and ds.bg_img_paths == []
    assert [a['name'] for a in ds._aug_plan][:3] == ['Affine', 'CoarseDropout', 'GaussianBlur'] and len(ds._aug_plan) == 8
    ds._refuse_occlusion()


def test_augment_symbols_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'aae_hip.h')).read()
    import __graft_entry__ as g
    g.build()
    out = subprocess.check_output(['/opt/rocm/lib/llvm/bin/llvm-readelf', '--dyn-syms', '--wide', g.LIB]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if ' FUNC ' in l and ' UND ' not in l)
    for name in ('aae_augment_max_image_bytes', 'aae_augment_batch'):
        assert name + '(' in header and name in _lib.EXPORTED_SYMBOLS and name in exported
    for name, value in (('AAE_AUGMENT_MAX_OPS', 16), ('AAE_AUGMENT_MAX_BLUR_K', 15), ('AAE_AUGMENT_AFFINE', 1), ('AAE_AUGMENT_DROPOUT', 2), ('AAE_AUGMENT_BLUR', 3),
                        ('AAE_AUGMENT_ADD', 4), ('AAE_AUGMENT_INVERT', 5), ('AAE_AUGMENT_MULTIPLY', 6), ('AAE_AUGMENT_CONTRAST', 7)):
        assert '#define %s %d' % (name, value) in header and getattr(_lib, name) == value
