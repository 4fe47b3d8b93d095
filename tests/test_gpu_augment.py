"""Training batches on the MI355X: the table of tests/augment_cases.py through aae_augment_batch against the NumPy float64
restatement (outputs handed in full of 0xA5), the 128x128x3 shape the product runs at (the LDS ceiling it needs: 96 KB), the
refusal just over the limit, null output pointers, a second call, and Dataset.batch_device / Dataset.batch on a tiny in-memory
dataset.

Acceptance rule (tests/augment_reference.py): where no blur ran before a pixel's value was fixed the uint8 output equals the
reference byte for byte; a pixel whose float64 blur value lies within 1e-3 (scaled with k^2 above k = 7) of a half-integer, and
what later spatial ops compute from it, is left out; at most 1 % of a case may be left out."""
import ctypes

import numpy as np
import pytest

import augment_cases as ac
import augment_reference as ar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def device_data():
    import torch
    tx, m, ty, bg = ac.DATA
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (tx, m, ty, bg))


def _garbage(shape, dtype):
    """a device tensor whose every byte is 0xA5"""
    import torch
    size = torch.empty((), dtype=dtype).element_size()
    return torch.full(tuple(shape) + (size,), 0xA5, dtype=torch.uint8, device='cuda').view(dtype).reshape(tuple(shape))


def _run(device_data, name, out=None):
    from augmentedautoencoder_amd import augmentation as aug
    pb, ti, bi = ac.build(name)
    shape = (pb.B, pb.H, pb.W, pb.C)
    import torch
    out = out or (_garbage(shape, torch.uint8), _garbage(shape, torch.float32), _garbage(shape, torch.float32))
    assert all(t is None or tuple(t.shape) == shape for t in out)
    return aug.run_batch(*device_data, ti, bi, pb, out=out)


@pytest.mark.parametrize('name', sorted(ac.CASES))
def test_table_matches_reference(device_data, name):
    u8, x, y = [t.cpu().numpy() for t in _run(device_data, name)]
    left_out = ac.check(name, u8, x, y)
    print('%s: %.3f %% left out, largest difference %d' % (name, 100 * left_out, np.abs(u8.astype(int) - ac.reference(name)[0].astype(int)).max()))


def test_null_outputs_and_second_call(device_data):
    import torch
    name = 'template_chain'
    first = [t.cpu().numpy() for t in _run(device_data, name)]
    again = [t.cpu().numpy() for t in _run(device_data, name)]
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    shape = first[0].shape
    for keep in range(3):
        out = [None, None, None]
        out[keep] = _garbage(shape, torch.uint8 if keep == 0 else torch.float32)
        got = _run(device_data, name, out=tuple(out))
        assert [g is None for g in got] == [k != keep for k in range(3)]
        assert got[keep].cpu().numpy().tobytes() == first[keep].tobytes()
    # all three null: accepted, nothing launched, nothing written
    from augmentedautoencoder_amd import augmentation as aug
    pb, ti, bi = ac.build(name)
    assert aug.run_batch(*device_data, ti, bi, pb, out=(None, None, None)) == (None, None, None)


def test_product_shape_with_the_template_chain():
    """128 x 128 x 3: two 48 KB image buffers, the dword path (H*W*C % 4 == 0), more workgroups than one wave of them"""
    import torch
    from augmentedautoencoder_amd import augmentation as aug
    shape = (128, 128, 3)
    data = ac.make_data(shape, n=4, m=3, seed=23)
    B = 6
    pb = aug.ProgramBuilder(B, shape)
    ac.template_chain(pb, np.random.RandomState(8))
    pb.blur(0, 1.2)                                            # whatever the coins said, image 0 is blurred and image 1 scaled
    pb.affine(1, ac.INV_S[1])
    ti, bi = np.arange(B, dtype=np.int32) % 4, np.arange(B, dtype=np.int32) % 3
    dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in data)
    out = tuple(_garbage((B,) + shape, dt) for dt in (torch.uint8, torch.float32, torch.float32))
    u8, x, y = [t.cpu().numpy() for t in aug.run_batch(*dev, ti, bi, pb, out=out)]
    ref, sure, ref_y = ar.reference_batch(*data, ti, bi, pb.programs)
    left_out, _ = ar.check_batch(u8, ref, sure, '128x128x3')
    print('128x128x3 template chain: %.3f %% left out' % (100 * left_out))
    assert x.tobytes() == ar.unit_f32(u8).tobytes() and y.tobytes() == ar.unit_f32(ref_y).tobytes()


def test_shape_over_the_lds_limit_is_refused_without_a_launch():
    import torch
    from augmentedautoencoder_amd import _lib, augmentation as aug
    lib = _lib.load()
    limit = lib.aae_augment_max_image_bytes()
    assert limit == aug.MAX_IMAGE_BYTES == 81920
    shape = (166, 165, 3)                                      # 82170 bytes; 165 x 165 x 3 = 81675 fits
    assert 165 * 165 * 3 <= limit < shape[0] * shape[1] * shape[2]
    data = [torch.zeros((1,) + shape, dtype=torch.uint8, device='cuda'), torch.zeros((1,) + shape[:2], dtype=torch.bool, device='cuda'),
            torch.zeros((1,) + shape, dtype=torch.uint8, device='cuda'), torch.zeros((1,) + shape, dtype=torch.uint8, device='cuda')]
    pb = aug.ProgramBuilder(1, shape)
    out = (_garbage((1,) + shape, torch.uint8), None, None)
    with pytest.raises(ValueError, match='over the limit of 81920 bytes'):
        aug.run_batch(*data, np.zeros(1, np.int32), np.zeros(1, np.int32), pb, out=out)
    torch.cuda.synchronize()
    assert (out[0] == 0xA5).all()                              # nothing ran
    s = _lib.AugmentShape(1, 1, 4096, 8, 3, 1, 0)
    assert lib.aae_augment_batch(ctypes.byref(s), *[ctypes.c_void_p(t.data_ptr()) for t in data], *([ctypes.c_void_p(data[0].data_ptr())] * 4), None,
                                 ctypes.c_void_p(out[0].data_ptr()), None, None, None) == -2
    assert b'outside' in lib.aae_last_error()
    assert lib.aae_augment_batch(ctypes.byref(s), None, *([None] * 12)) == -1 and b'null' in lib.aae_last_error()


def test_fitting_shape_just_under_the_limit():
    """165 x 165 x 3 = 81675 bytes: the largest square that fits, an odd byte count, the identity program and one blur"""
    import torch
    from augmentedautoencoder_amd import augmentation as aug
    shape = (165, 165, 3)
    data = ac.make_data(shape, n=3, m=2, seed=31)
    pb = aug.ProgramBuilder(2, shape)
    pb.blur(1, 0.75)
    ti, bi = np.array([2, 0], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in data)
    u8 = aug.run_batch(*dev, ti, bi, pb, want_x=False, want_y=False)[0].cpu().numpy()
    ref, sure, _ = ar.reference_batch(*data, ti, bi, pb.programs)
    ar.check_batch(u8, ref, sure, '165x165x3')
    assert np.array_equal(u8[0], ref[0])


# every parameter exact in fp32 (1 / 1.28 = 25/32), so the acceptance rule of the table applies to what Dataset draws
EXACT_CODE = """Sequential([
    Sometimes(0.5, Affine(scale=1.28)),
    Sometimes(0.5, CoarseDropout(p=0.2, size_percent=0.1)),
    Sometimes(0.5, GaussianBlur(0.75)),
    Sometimes(0.5, Add((-25, 25), per_channel=0.3)),
    Sometimes(0.3, Invert(0.2, per_channel=True)),
    Sometimes(0.5, Multiply(1.25, per_channel=0.5)),
    Sometimes(0.5, ContrastNormalization(0.75))], random_order=False)"""


def test_dataset_batch_device_and_batch():
    """N = 9, M = 7, batch 5"""
    import torch
    from augmentedautoencoder_amd import augmentation as aug
    from augmentedautoencoder_amd.dataset import Dataset
    ds = Dataset('', h=ac.H, w=ac.W, c=ac.C, code=EXACT_CODE, realistic_occlusion='False', square_occlusion='False', noof_training_imgs=ac.N)
    ds.train_x, ds.mask_x, ds.train_y, ds.bg_imgs = ac.DATA
    assert ds.to_device() is ds
    assert len(ds._aug_plan) == 7                               # parsed here: the first batch of a Dataset parses CODE after its two choices (dataset.py:488)
    np.random.seed(77)
    x, y = ds.batch_device(5)
    after = np.random.rand()
    assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (5, ac.H, ac.W, ac.C) and tuple(y.shape) == tuple(x.shape)
    np.random.seed(77)
    bx, by = ds.batch(5)
    assert after == np.random.rand()                           # both consume np.random alike
    assert bx.dtype == np.float64 and by.dtype == np.float64 and bx.shape == (5, ac.H, ac.W, ac.C)
    np.random.seed(77)
    ti = np.random.choice(ac.N, 5, replace=False)
    bi = np.random.choice(ac.M, 5, replace=False)
    pb = aug.draw_programs(ds._aug_plan, 5, (ac.H, ac.W, ac.C))
    assert float(np.float32(pb.ops['f'][pb.ops['code'] == 1][:, 0]).max(initial=0.78125)) == 0.78125
    u8 = np.rint(bx * 255.).astype(np.uint8)
    assert np.array_equal(u8 / 255., bx) and np.array_equal(by, ac.DATA[2][ti] / 255.)
    assert x.cpu().numpy().tobytes() == ar.unit_f32(u8).tobytes() and y.cpu().numpy().tobytes() == ar.unit_f32(ac.DATA[2][ti]).tobytes()
    ref, sure, _ = ar.reference_batch(*ac.DATA, ti, bi, pb.programs)
    ar.check_batch(u8, ref, sure, 'Dataset.batch')
    assert pb.n_ops.sum() >= 5                                  # the seed draws a batch that does something
