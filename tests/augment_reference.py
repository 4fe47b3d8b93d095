"""NumPy float64 restatement of Dataset.batch's pixel arithmetic: the background composite and the seven ops of
csrc/kernels/augment_core.h, each as the real-valued image before rounding (``*_real``) and as the uint8 image after it, plus the
acceptance rule of the augmentation tests (``apply_program`` returns the image and the mask of pixels that must be equal).

Programs are the (name, values) tuples of augmentation.ProgramBuilder.programs.  Parameters arrive as the fp32 values the kernel
receives, widened to float64.  test_augment_cpu.py cross-checks blur_real and affine_real against scipy.ndimage to 1e-9."""
import numpy as np

BLUR_MARGIN = 1e-3            # for k <= 7; scaled with k^2 above (the fp32 sum's bound is about (k^2 + 1) 2^-24 255)
LEFT_OUT_CAP = 0.01


def round_u8(real):
    """clip to [0,255], round half to even"""
    return np.rint(np.clip(real, 0.0, 255.0)).astype(np.uint8)


def composite(train_x, mask_x, bg):
    return np.where(np.asarray(mask_x).astype(bool)[..., None], bg, train_x).astype(np.uint8)


def reflect101(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def _affine_gather(img, inv_s):
    """the four neighbours (0 outside the image) and the two fractions of every destination pixel"""
    H, W = img.shape[:2]
    inv_s = float(np.float32(inv_s))
    sx = (W - 1) / 2.0 + (np.arange(W) - (W - 1) / 2.0) * inv_s
    sy = (H - 1) / 2.0 + (np.arange(H) - (H - 1) / 2.0) * inv_s
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = (sx - x0)[None, :, None], (sy - y0)[:, None, None]

    def take(yy, xx):
        ok = ((yy >= 0) & (yy < H))[:, None] & ((xx >= 0) & (xx < W))[None, :]
        return img[np.clip(yy, 0, H - 1)][:, np.clip(xx, 0, W - 1)] * ok[..., None]
    return take(y0, x0), take(y0, x0 + 1), take(y0 + 1, x0), take(y0 + 1, x0 + 1), fx, fy


def affine_real(img, inv_s):
    p00, p01, p10, p11, fx, fy = _affine_gather(np.asarray(img, dtype=np.float64), inv_s)
    return (1 - fy) * ((1 - fx) * p00 + fx * p01) + fy * ((1 - fx) * p10 + fx * p11)


def blur_real(img, weights):
    img = np.asarray(img, dtype=np.float64)
    H, W = img.shape[:2]
    w = np.asarray(weights, dtype=np.float64)
    k = len(w)
    iy = reflect101(np.arange(H)[:, None] + np.arange(k)[None, :] - k // 2, H)
    ix = reflect101(np.arange(W)[:, None] + np.arange(k)[None, :] - k // 2, W)
    rows = sum(w[d] * img[:, ix[:, d]] for d in range(k))
    return sum(w[d] * rows[iy[:, d]] for d in range(k))


def dropout_mask(dropped, rows, cols, C):
    """bool [H,W,C]: the pixel is dropped"""
    planes = dropped[np.arange(C) % dropped.shape[0]]
    return np.moveaxis(planes[:, rows][:, :, cols], 0, -1)


def pointwise_real(name, img, values):
    x = np.asarray(img, dtype=np.float64)
    v = np.asarray(values)[:x.shape[-1]]
    if name == 'add':
        return x + v
    if name == 'invert':
        return np.where(v.astype(bool), 255.0 - x, x)
    if name == 'multiply':
        return x * v
    if name == 'contrast':
        return 128.0 + v * (x - 128.0)
    raise KeyError(name)


def _spread_affine(bad, inv_s):
    p00, p01, p10, p11, _, _ = _affine_gather(bad.astype(np.float64), inv_s)
    return (p00 + p01 + p10 + p11) > 0


def _spread_blur(bad, k):
    return blur_real(bad.astype(np.float64), np.ones(k)) > 0


def apply_program(img, program, track=True):
    """(uint8 image after the program, bool mask of the pixels that must equal it).  A pixel whose float64 blur value lies
    within the margin of a half-integer may round either way in fp32: it leaves the mask there, and so does every pixel a later
    spatial op computes from it.  A dropped pixel is 0 whatever it was and joins the mask again.  track=False computes the image
    alone (the mask is None): what a user of the restatement would run."""
    img = np.asarray(img, dtype=np.uint8)
    sure = np.ones(img.shape, dtype=bool) if track else None
    for op in program:
        name = op[0]
        if name == 'affine':
            if track:
                sure = ~_spread_affine(~sure, op[1])
            img = round_u8(affine_real(img, op[1]))
        elif name == 'blur':
            k, w = op[1], op[2]
            real = blur_real(img, w)
            if track:
                margin = BLUR_MARGIN * max(1.0, k * k / 49.0)
                sure = ~_spread_blur(~sure, k) & ~(np.abs(real - np.floor(real) - 0.5) < margin)
            img = round_u8(real)
        elif name == 'dropout':
            drop = dropout_mask(op[1], op[2], op[3], img.shape[-1])
            img = np.where(drop, 0, img).astype(np.uint8)
            if track:
                sure = sure | drop
        else:
            img = round_u8(pointwise_real(name, img, op[1]))
    return img, sure


def unit_f32(u8):
    """np.float32(v / 255.)"""
    return (np.asarray(u8) / 255.).astype(np.float32)


def reference_batch(train_x, mask_x, train_y, bg, train_idx, bg_idx, programs, track=True):
    """(batch_x uint8 [B,H,W,C], must-be-equal mask or None, batch_y uint8) of one batch"""
    xs, sures = [], []
    for b, (ti, bi) in enumerate(zip(train_idx, bg_idx)):
        x, sure = apply_program(composite(train_x[ti], mask_x[ti], bg[bi]), programs[b], track)
        xs.append(x)
        sures.append(sure)
    return np.stack(xs), np.stack(sures) if track else None, np.asarray(train_y)[np.asarray(train_idx)]


def check_batch(got_u8, ref_u8, sure, label):
    """the acceptance rule: every pixel of the mask equal, at most 1 % of a case outside the mask"""
    left_out = 1.0 - sure.mean()
    assert left_out <= LEFT_OUT_CAP, '%s: %.3f %% of the pixels left out' % (label, 100 * left_out)
    wrong = (np.asarray(got_u8) != ref_u8) & sure
    assert not wrong.any(), '%s: %d pixels differ, first at %s: got %d, reference %d' % (
        label, wrong.sum(), tuple(np.argwhere(wrong)[0]), np.asarray(got_u8)[tuple(np.argwhere(wrong)[0])], ref_u8[tuple(np.argwhere(wrong)[0])])
    off = np.abs(np.asarray(got_u8).astype(np.int64) - ref_u8.astype(np.int64))
    return left_out, int(off.max())
