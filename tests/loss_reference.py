"""The training loss restated in NumPy (the reference's auto_pose/ae/decoder.py:86-132 and encoder.py:97-100 as DESIGN.md section 4i
reads them), the case table of the loss tests and the checks every implementation (the host driver over loss_core.h, the kernels)
has to pass.

With n = H*W*C and x, t the flattened reconstruction and target of an image, both float32:
    d = x - t and e = d*d (L2) or |d| (L1), each operation in float32;
    k = n // bootstrap_ratio; the selected set of an image is the first k entries of a stable descending sort of e (tf.nn.top_k:
    among equal values the lower index first); a NaN ranks above every number; ratio 1 selects everything;
    per_image = the float64 mean of the selected float32 errors, loss = the mean of per_image;
    dx = 2 d / (B k) (L2) or sign(d) / (B k) (L1) on a selected element, in float64 from the float32 d, 0 elsewhere."""
import numpy as np

U = 2.0 ** -24                       # unit roundoff of float32
SUM_RTOL = 1e-5                      # (64 + log2(B n)) u < 6e-6: non-negative terms, chains of at most 64, then trees
GRAD_RTOL = 4 * U                    # two roundings and the rounded scale
NEG_NAN = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]       # a NaN with the sign bit set


def errors(x, t, kind):
    d = (x.astype(np.float32) - t.astype(np.float32)).astype(np.float32)
    e = np.abs(d) if kind == 'L1' else (d * d).astype(np.float32)
    return d, e.astype(np.float32)


def order(e):
    """indices of one image by descending error, lower index first among equals, NaN above everything: for NaN-free errors this is
    np.argsort(-e, kind='stable')"""
    key = (e.view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int64)
    return np.argsort(-key, kind='stable')


def reference(x, t, kind, ratio):
    """-> dict(d, e, k, sel bool [B,n], per_image float64 [B], loss float64, dx float64 [B,n])"""
    B, n = x.shape
    d, e = errors(x, t, kind)
    k = n // ratio
    assert k >= 1
    sel = np.zeros((B, n), dtype=bool)
    for b in range(B):
        sel[b, order(e[b])[:k]] = True
    with np.errstate(invalid='ignore'):
        per_image = np.array([e[b][sel[b]].astype(np.float64).sum() / k for b in range(B)])
        d64 = d.astype(np.float64)
        g = 2.0 * d64 if kind == 'L2' else np.sign(d64)
        dx = np.where(sel, g / (float(B) * k), 0.0)
    return dict(d=d, e=e, k=k, sel=sel, per_image=per_image, loss=per_image.mean(), dx=dx)


def reg_reference(z):
    """-> (loss float64, dz float64 [B,J]) from the float32 z; a zero row has gradient 0"""
    z64 = z.astype(np.float64)
    norm = np.sqrt((z64 * z64).sum(axis=1))
    loss = np.abs(norm - 1.0).mean()
    with np.errstate(invalid='ignore', divide='ignore'):
        dz = np.sign(norm - 1.0)[:, None] * z64 / norm[:, None] / z.shape[0]
    dz[norm == 0.0] = 0.0
    return loss, dz


# ---- the case table -----------------------------------------------------------------------------------------------------------------
N_TINY, N_SMALL, N_RAGGED, N_PRODUCT, N_OVER = 1, 7 * 5 * 3, 37 * 46 * 3, 128 * 128 * 3, 129 * 128 * 3
CASES = {}          # name -> (builder() -> (x, t, kind, ratio), what: 'distinct' | 'cut' | 'exact' | None)


def _case(name, what=None):
    def add(fn):
        CASES[name] = (fn, what)
        return fn
    return add


def _random(B, n, seed):
    rng = np.random.RandomState(seed)
    return rng.rand(B, n).astype(np.float32), rng.rand(B, n).astype(np.float32)


def _grid():
    seed = 100
    for n in (N_TINY, N_SMALL, N_RAGGED):
        for B in (1, 5, 67):
            for kind in ('L2', 'L1'):
                for ratio in sorted({1, 2, 3, 4, n}):
                    if n // ratio < 1:
                        continue
                    seed += 1
                    name = 'rand_n%d_B%d_%s_r%d' % (n, B, kind, ratio)
                    CASES[name] = ((lambda B=B, n=n, kind=kind, ratio=ratio, seed=seed: _random(B, n, seed) + (kind, ratio)), 'distinct' if ratio > 1 else None)


_grid()


@_case('product_L2_r4', 'distinct')
def _product():
    return _random(3, N_PRODUCT, 7) + ('L2', 4)


@_case('over_resident_L2_r4', 'distinct')
def _over():
    return _random(2, N_OVER, 8) + ('L2', 4)


@_case('over_resident_L1_r1')
def _over_all():
    return _random(2, N_OVER, 9) + ('L1', 1)


def _planted(B, n, ratio, kind, group, extra, seed):
    """small random errors, k - extra large ones, and a tie group (d = 0.25) at the indices `group`: k cuts the group after `extra`"""
    rng = np.random.RandomState(seed)
    k = n // ratio
    t = (rng.rand(B, n) * 0.5).astype(np.float32)
    x = t.copy()
    group = np.asarray(sorted(set(int(g) % n for g in group)))
    free = np.setdiff1d(np.arange(n), group)
    for b in range(B):
        x[b, free] = t[b, free] + (rng.rand(len(free)) * 0.1).astype(np.float32)
        big = rng.choice(free, k - extra, replace=False)
        x[b, big] = t[b, big] + np.float32(0.3) + (rng.rand(len(big)) * 0.1).astype(np.float32)
    t[:, group] = np.float32(0.25)
    x[:, group] = np.float32(0.5)
    return x, t, kind, ratio


# lane 63|64 (a wave's end), 1023|1024 (a row's end), 2047|2048, the last elements of the image, and a run inside one wave
_BOUNDARY = [3, 62, 63, 64, 65, 700, 701, 702, 1022, 1023, 1024, 1025, 2047, 2048, 4095, 4096, 4097, 5000, -2, -1]


@_case('ties_cut_L2', 'cut')
def _ties_cut():
    return _planted(5, N_RAGGED, 4, 'L2', _BOUNDARY, 9, 11)


@_case('ties_cut_L1_B67', 'cut')
def _ties_cut_l1():
    return _planted(67, N_RAGGED, 3, 'L1', _BOUNDARY, 13, 12)


@_case('ties_cut_small', 'cut')
def _ties_cut_small():
    return _planted(5, N_SMALL, 2, 'L2', [0, 1, 50, 63, 64, 65, 104], 3, 13)


@_case('ties_cut_product', 'cut')
def _ties_cut_product():
    return _planted(2, N_PRODUCT, 4, 'L2', _BOUNDARY + [20000, 30000, 49000, 48 * 1024 - 1025], 11, 14)


@_case('ties_cut_over_resident', 'cut')
def _ties_cut_over():
    # the second chunk of 64 rows does not exist at this size, the 49th row does: ties in it, beyond what the resident form holds
    return _planted(2, N_OVER, 4, 'L1', _BOUNDARY + [48 * 1024, 48 * 1024 + 63, 48 * 1024 + 64, 49000], 12, 15)


@_case('ties_end_at_k', 'exact')
def _ties_exact():
    group = sorted(set(g % N_RAGGED for g in _BOUNDARY))
    return _planted(5, N_RAGGED, 4, 'L2', group, len(group), 16)


@_case('all_equal_L2', 'cut')
def _all_equal():
    return np.full((5, N_RAGGED), 0.75, np.float32), np.full((5, N_RAGGED), 0.25, np.float32), 'L2', 4


@_case('all_equal_L1_small', 'cut')
def _all_equal_l1():
    return np.full((67, N_SMALL), 0.25, np.float32), np.full((67, N_SMALL), 0.75, np.float32), 'L1', 3


@_case('x_equals_t', 'cut')
def _same():
    x = _random(5, N_RAGGED, 17)[0]
    return x, x.copy(), 'L2', 4


@_case('low_mantissa_bit', 'cut')
def _low_bit():
    rng = np.random.RandomState(18)
    x = (np.float32(0.5) + rng.randint(0, 2, (5, N_RAGGED)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    return x, np.zeros_like(x), 'L1', 4


@_case('exponent_only', 'cut')
def _exponent():
    rng = np.random.RandomState(19)
    x = np.ldexp(np.float32(1.0), -rng.randint(1, 21, (5, N_RAGGED))).astype(np.float32)
    return x, np.zeros_like(x), 'L1', 4


@_case('subnormal_errors', 'cut')
def _subnormal():
    # the threshold is a subnormal square (the tie group of 2^-140 is cut); a tenth of the errors are 0.25, so that the means are
    # normal numbers and float32 can hold them to the bound
    rng = np.random.RandomState(20)
    pick = np.array([0.0, 2.0 ** -70, 2.0 ** -71, 3 * 2.0 ** -72, 2.0 ** -74], dtype=np.float32)       # squares: 0 and subnormals down to 2^-148
    x = pick[rng.randint(0, len(pick), (5, N_RAGGED))]
    x[rng.rand(5, N_RAGGED) < 0.1] = np.float32(0.5)
    return x * np.where(rng.rand(5, N_RAGGED) < 0.5, np.float32(-1), np.float32(1)), np.zeros((5, N_RAGGED), np.float32), 'L2', 4


@_case('one_ulp_apart', 'distinct')
def _one_ulp():
    rng = np.random.RandomState(21)
    x = np.stack([np.float32(0.5) + rng.permutation(N_RAGGED).astype(np.float32) * np.float32(2.0 ** -24) for _ in range(5)]).astype(np.float32)
    return x, np.zeros_like(x), 'L1', 4


def _with_nan(kind):
    x, t = _random(5, N_RAGGED, 22)
    x[2, 1234] = NEG_NAN
    return x, t, kind, 4


CASES['nan_image_L2'] = (lambda: _with_nan('L2'), None)
CASES['nan_image_L1'] = (lambda: _with_nan('L1'), None)

_BUILT = {}


def build(name):
    """-> (x, t, kind, ratio, reference dict), built once and shared; asserts what the case is for"""
    if name not in _BUILT:
        fn, what = CASES[name]
        x, t, kind, ratio = fn()
        x, t = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(t, dtype=np.float32)
        ref = reference(x, t, kind, ratio)
        k, n = ref['k'], x.shape[1]
        for b in range(x.shape[0]):
            srt = ref['e'][b][order(ref['e'][b])]
            if what == 'distinct':
                assert k < n and srt[k - 1] > srt[k], (name, b)
            elif what == 'cut':                      # the tie group of the k-th value starts before rank k or at it, and goes on past it
                assert k < n and srt[k - 1] == srt[k], (name, b)
            elif what == 'exact':
                assert k < n and srt[k - 1] > srt[k] and srt[k - 1] == srt[k - 2], (name, b)
        for a in (x, t):
            a.setflags(write=False)
        _BUILT[name] = (x, t, kind, ratio, ref)
    return _BUILT[name]


def check(name, loss, per_image, dx):
    """The checks of a case on float32 outputs; returns the measured maxima (sum rel err, L2 grad rel err in units of u)."""
    x, t, kind, ratio, ref = build(name)
    B, n = x.shape
    k = ref['k']
    loss, per_image, dx = np.float32(loss), np.asarray(per_image, np.float32).reshape(B), np.asarray(dx, np.float32).reshape(B, n)
    ok_img = ~np.isnan(ref['per_image'])
    assert np.isnan(per_image[~ok_img]).all(), name
    rel = np.abs(per_image[ok_img] - ref['per_image'][ok_img]) / np.maximum(np.abs(ref['per_image'][ok_img]), 1e-300)
    rel = np.where(ref['per_image'][ok_img] == 0, np.abs(per_image[ok_img]), rel)
    sum_err = float(rel.max()) if rel.size else 0.0
    if np.isnan(ref['loss']):
        assert np.isnan(loss), name
    else:
        lerr = abs(float(loss) - ref['loss']) / ref['loss'] if ref['loss'] != 0 else abs(float(loss))
        sum_err = max(sum_err, lerr)
    assert sum_err <= SUM_RTOL, (name, sum_err)
    grad_err = 0.0
    scale = np.float32(1.0 / (B * k))
    for b in np.nonzero(ok_img)[0]:
        want = ref['dx'][b]
        # {dx != 0} together with the selected elements whose gradient is 0 is the reference's selected set
        assert np.array_equal(dx[b] != 0, ref['sel'][b] & (want != 0)), (name, b, int(((dx[b] != 0) != (ref['sel'][b] & (want != 0))).sum()))
        if kind == 'L1':
            assert dx[b].tobytes() == (np.sign(want).astype(np.float32) * scale).astype(np.float32).tobytes(), (name, b)
        else:
            nz = want != 0
            err = np.abs(dx[b][nz].astype(np.float64) - want[nz]) / np.abs(want[nz])
            if err.size:
                grad_err = max(grad_err, float(err.max()))
    assert grad_err <= GRAD_RTOL, (name, grad_err / U)
    return sum_err, grad_err / U


# ---- the host driver's files --------------------------------------------------------------------------------------------------------
def write_input(path, x, t, kind, ratio):
    B, n = x.shape
    with open(path, 'wb') as f:
        np.array([B, n, 1 if kind == 'L1' else 0, ratio], dtype=np.int32).tofile(f)
        x.tofile(f)
        t.tofile(f)


def read_output(path, B, n):
    raw = np.fromfile(path, dtype=np.float32)
    assert raw.size == 1 + B + B * n
    return raw[0], raw[1:1 + B], raw[1 + B:].reshape(B, n)


REG_CASES = [(J, B) for J in (4, 128, 129) for B in (1, 67)]


def reg_input(J, B):
    """rows with norm below, above and exactly 1 and a zero row (B = 1: the row of norm exactly 1 only when J = 4)"""
    rng = np.random.RandomState(1000 + 7 * J + B)
    z = rng.randn(B, J).astype(np.float32)
    if B == 1:
        if J == 4:
            z[0] = (0.0, 1.0, 0.0, 0.0)
        elif J == 128:
            z[0] *= np.float32(0.01)
        return z
    z[0::4] *= np.float32(0.3 / np.sqrt(J))          # norms below 1
    z[1::4] *= np.float32(3.0 / np.sqrt(J))          # above
    z[5] = 0.0
    z[6] = 0.0
    z[6, J - 1] = -1.0                               # exactly 1
    z[7] = 0.0
    z[7, :4] = 0.5                                   # exactly 1: 4 * 0.25
    return z


def check_reg(z, loss, dz):
    want_loss, want_dz = reg_reference(z)
    lerr = abs(float(loss) - want_loss) / want_loss if want_loss != 0 else abs(float(loss))
    assert lerr <= SUM_RTOL, lerr
    dz = np.asarray(dz, np.float32).reshape(z.shape)
    assert np.array_equal(dz != 0, want_dz != 0)
    nz = want_dz != 0
    gerr = float((np.abs(dz[nz].astype(np.float64) - want_dz[nz]) / np.abs(want_dz[nz])).max()) if nz.any() else 0.0
    assert gerr <= GRAD_RTOL, gerr / U
    return lerr, gerr / U
