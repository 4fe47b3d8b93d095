"""The decoder's backward pass restated in float64 NumPy, in its DIRECT form: the upsampled image is materialised, every tap of
the KS x KS kernel is its own product, nothing is folded into phases -- so the phase-folded kernels (csrc/kernels/decoder_bwd_core.h,
decoder_bwd_f32.h) are checked against something that shares no index map with them.  TEST INFRASTRUCTURE ONLY.

For a stage  a_out = act(conv_same(resize_nearest(a_in, UH x UW), w) + b)  and g_out = dL/da_out:
    delta = g_out where a_out > 0 else 0 (ReLU);  (g_out a_out)(1 - a_out) (sigmoid)
    db[co]          = sum_{b,y,x} delta
    dw[kh,kw,ci,co] = sum_{b,y,x} up(a_in)[b, y+kh-p, x+kw-p, ci] delta[b,y,x,co]          (taps outside the upsampled image: nothing)
    g_in[b,h,w,ci]  = sum over the upsampled pixels that read (h,w), and kh,kw,co, of delta[b,y-kh+p,x-kw+p,co] w[kh,kw,ci,co]
For the dense layer a_out = relu(z w + b):  dw = z^T delta, db = sum_b delta, dz = delta w^T.

Every gradient comes with S = sum |products| and the term count n of each element.  The bound of a fp32 evaluation in ANY
summation order is |got - ref64| <= gamma_n S <~ n u S, u = 2^-24; the checks here allow (n + 8) u S: the 8 covers the single
rounding of a folded weight (1), the sums of the four-phase unfold and of the K splits being separate roundings already counted in
n but grouped differently, and the final reduce.  For the sigmoid stage the device's delta is itself a fp32 value of three roundings
(two products and a difference), which every downstream sum inherits: those elements get n + 3.  The reference is evaluated on
exactly the float32 inputs the call was given, so the ReLU masks agree by construction and no element is left out.

The case table (CASES, DENSE_CASES) holds the smallest shapes at which each thing can go wrong; plan() restates the launch
planner so that a test can pin the form, the tile counts and the K splits a case ran with."""
import collections
import functools
import re

import numpy as np

U32 = 2.0 ** -24
SLACK = 8
RELU, SIGMOID = 0, 1

Stage = collections.namedtuple('Stage', 'name B H W Cin UH UW Cout KS act g_in')
Dense = collections.namedtuple('Dense', 'name B J U dz')

CASES = collections.OrderedDict((c.name, c) for c in [
    # every tile partial; 45 contraction pixels: one slab and 13 of the next, split in two
    Stage('ragged_3x5', 3, 3, 5, 32, 6, 10, 32, 5, RELU, True),
    # neither channel count a multiple of 32 or 4: scalar delta gathers, a 40-row tap inside a 128-row tile
    Stage('cin40_cout5', 2, 4, 3, 40, 8, 6, 5, 5, RELU, True),
    Stage('ks1', 2, 3, 4, 32, 6, 8, 32, 1, RELU, True),                    # U = 1
    Stage('ks3', 2, 3, 4, 32, 6, 8, 8, 3, RELU, True),                     # U = 2
    Stage('ks7', 2, 3, 3, 32, 6, 6, 16, 7, RELU, True),                    # U = 4: taps reach past a 3-pixel source on both sides
    Stage('one_pixel', 2, 1, 1, 32, 2, 2, 32, 5, RELU, True),              # every tap but the centre crosses a border
    Stage('plain_7x9', 2, 7, 9, 32, 7, 9, 24, 5, RELU, True),              # a 1x stage: the one-phase case, U = KS
    Stage('sigmoid_last', 2, 8, 8, 32, 16, 16, 3, 5, SIGMOID, True),       # the output stage
    # 576 rows per phase = 4.5 row tiles (five per phase, twenty in all), a second column tile with 8 columns; 18 pixels: no K split
    Stage('two_col_tiles', 2, 3, 3, 64, 6, 6, 136, 5, RELU, True),
    Stage('split_k', 4, 8, 8, 32, 16, 16, 32, 5, RELU, True),              # 256 pixels = 8 slabs over 12 tiles: one slab per split
    Stage('no_g_in', 2, 4, 4, 32, 8, 8, 32, 5, RELU, False),
])

DENSE_CASES = collections.OrderedDict((c.name, c) for c in [
    Dense('dense_J128_U96_B1', 1, 128, 96, True),
    Dense('dense_J128_U240_B5', 5, 128, 240, True),
    Dense('dense_J33_U96_B67', 67, 33, 96, True),
    Dense('dense_J33_U240_B67', 67, 33, 240, True),
    Dense('dense_J128_U96_B5_no_dz', 5, 128, 96, False),
])


def _seed(name):
    return 7000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


def _readonly(d):
    for v in d.values():
        v.setflags(write=False)
    return d


def _activation_values(rng, shape, act):
    """about half exactly 0; the rest positive (ReLU) or inside (0, 1) (sigmoid)"""
    a = rng.uniform(0.05, 0.95, shape) if act == SIGMOID else np.abs(rng.standard_normal(shape)) + 0.01
    a[rng.random(shape) < 0.5] = 0.0
    return a.astype(np.float32)


@functools.lru_cache(maxsize=None)
def stage_inputs(name):
    c = CASES[name]
    rng = np.random.default_rng(_seed(name))
    return _readonly(dict(
        a_in=(rng.standard_normal((c.B, c.H, c.W, c.Cin)) * (rng.random((c.B, c.H, c.W, c.Cin)) < 0.7)).astype(np.float32),
        a_out=_activation_values(rng, (c.B, c.UH, c.UW, c.Cout), c.act),
        g_out=rng.standard_normal((c.B, c.UH, c.UW, c.Cout)).astype(np.float32),
        w=(rng.standard_normal((c.KS, c.KS, c.Cin, c.Cout)) * 0.1).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def dense_inputs(name):
    c = DENSE_CASES[name]
    rng = np.random.default_rng(_seed(name))
    return _readonly(dict(
        z=rng.standard_normal((c.B, c.J)).astype(np.float32),
        a_out=_activation_values(rng, (c.B, c.U), RELU),
        g_out=rng.standard_normal((c.B, c.U)).astype(np.float32),
        w=(rng.standard_normal((c.J, c.U)) * 0.1).astype(np.float32)))


# ---- the direct formulas ------------------------------------------------------------------------------------------------------------
def resize_index(n_out, n_in):
    return np.minimum((np.arange(n_out) * n_in) // n_out, n_in - 1)


def delta_of(g_out, a_out, act):
    """(delta, S, n) in float64"""
    g, a = np.asarray(g_out, np.float64), np.asarray(a_out, np.float64)
    if act == SIGMOID:
        d = (g * a) * (1.0 - a)
        return d, np.abs(d), np.full(d.shape, 3.0)
    d = np.where(a > 0, g, 0.0)
    return d, np.abs(d), np.ones(d.shape)


def _stage_products(a, d, w, UH, UW, want_g_in=True):
    """db, dw, g_in of the direct formulas for float64 a [B,H,W,Cin], d [B,UH,UW,Cout], w [KS,KS,Cin,Cout]; a_mask: see callers"""
    B, H, W, Cin = a.shape
    KS, Cout = w.shape[0], w.shape[3]
    p = (KS - 1) // 2
    iy, ix = resize_index(UH, H), resize_index(UW, W)
    up = np.zeros((B, UH + 2 * p, UW + 2 * p, Cin))
    up[:, p:p + UH, p:p + UW] = a[:, iy][:, :, ix]
    db = d.sum(axis=(0, 1, 2))
    dw = np.empty((KS, KS, Cin, Cout))
    for kh in range(KS):
        for kw in range(KS):
            dw[kh, kw] = np.einsum('byxi,byxo->io', up[:, kh:kh + UH, kw:kw + UW], d)
    if not want_g_in:
        return db, dw, None
    # forward: out[y,x] += up[y+kh-p, x+kw-p] w[kh,kw]  =>  g_up[y+kh-p, x+kw-p] += delta[y,x] w[kh,kw]^T
    g_up = np.zeros((B, UH + 2 * p, UW + 2 * p, Cin))
    for kh in range(KS):
        for kw in range(KS):
            g_up[:, kh:kh + UH, kw:kw + UW] += d @ w[kh, kw].T
    g_up = g_up[:, p:p + UH, p:p + UW]
    g_in = np.zeros((B, H, W, Cin))
    for y in range(UH):
        for x in range(UW):
            g_in[:, iy[y], ix[x]] += g_up[:, y, x]
    return db, dw, g_in


Ref = collections.namedtuple('Ref', 'val S n')


def stage_reference_arrays(a_in, a_out, g_out, w, UH, UW, act, want_g_in=True):
    """{'delta' | 'db' | 'dw' | 'g_in': Ref(val, S, n)} in float64, from the float32 arrays a call is given"""
    a, w64 = np.asarray(a_in, np.float64), np.asarray(w, np.float64)
    d, dS, dn = delta_of(g_out, a_out, act)
    extra = 3.0 if act == SIGMOID else 0.0
    val = _stage_products(a, d, w64, UH, UW, want_g_in)
    S = _stage_products(np.abs(a), dS, np.abs(w64), UH, UW, want_g_in)
    n = _stage_products(np.ones_like(a), np.ones_like(d), np.ones_like(w64), UH, UW, want_g_in)
    out = {'delta': Ref(d, dS, dn)}
    for key, v, s, k in zip(('db', 'dw', 'g_in'), val, S, n):
        if v is not None:
            out[key] = Ref(v, s, k + extra)
    return out


def dense_reference_arrays(z, a_out, g_out, w, want_dz=True):
    z64, w64 = np.asarray(z, np.float64), np.asarray(w, np.float64)
    d, dS, dn = delta_of(g_out, a_out, RELU)
    B, J = z64.shape
    U = w64.shape[1]
    out = {'delta': Ref(d, dS, dn),
           'db': Ref(d.sum(axis=0), dS.sum(axis=0), np.full((U,), float(B))),
           'dw': Ref(z64.T @ d, np.abs(z64).T @ dS, np.full((J, U), float(B)))}
    if want_dz:
        out['dz'] = Ref(d @ w64.T, dS @ np.abs(w64).T, np.full((B, J), float(U)))
    return out


@functools.lru_cache(maxsize=None)
def stage_reference(name):
    c, i = CASES[name], stage_inputs(name)
    return stage_reference_arrays(i['a_in'], i['a_out'], i['g_out'], i['w'], c.UH, c.UW, c.act, c.g_in)


@functools.lru_cache(maxsize=None)
def dense_reference(name):
    c, i = DENSE_CASES[name], dense_inputs(name)
    return dense_reference_arrays(i['z'], i['a_out'], i['g_out'], i['w'], c.dz)


def check(name, ref, got):
    """got: {'delta' | 'db' | 'dw' | 'g_in' | 'dz': float32 array}.  Asserts the per-element bound on EVERY element of every
    tensor of ref and returns {tensor: largest |got - ref| / (u S)} (the measured multiple of u S; 0 where S = 0)."""
    worst = {}
    for key, r in ref.items():
        g = np.asarray(got[key])
        assert g.dtype == np.float32 and g.shape == r.val.shape, (name, key, g.dtype, g.shape, r.val.shape)
        assert not np.isnan(g).any(), '%s: %s has %d unwritten (NaN) elements, first at %s' % (name, key, np.isnan(g).sum(), np.argwhere(np.isnan(g))[0].tolist())
        err = np.abs(g.astype(np.float64) - r.val)
        bound = (r.n + SLACK) * U32 * r.S
        with np.errstate(divide='ignore', invalid='ignore'):
            mult = np.where(r.S > 0, err / (U32 * r.S), 0.0)
        worst[key] = float(mult.max())
        bad = err > bound
        assert not bad.any(), '%s: %s misses (n + %d) u S at %d of %d elements; first %s: got %r, ref %r, S %r, n %r' % (
            name, key, SLACK, bad.sum(), bad.size, np.argwhere(bad)[0].tolist(), g[tuple(np.argwhere(bad)[0])], r.val[tuple(np.argwhere(bad)[0])],
            r.S[tuple(np.argwhere(bad)[0])], r.n[tuple(np.argwhere(bad)[0])])
    return worst


# ---- the launch planner, restated (aae_decoder_bwd_impl.h: plan_stage, plan_dense, choose_bwd_splits) ---------------------------------
TARGET_BLOCKS, MAX_SPLITS, BM, BK = 512, 64, 128, 32


def _ceil(a, b):
    return -(-a // b)


def tile_nt(n):
    return 1 if n <= 32 else (2 if n <= 64 else 4)


def splits_of(tiles, slabs):
    s = max(1, min(_ceil(TARGET_BLOCKS, tiles), MAX_SPLITS, slabs))
    return _ceil(slabs, _ceil(slabs, s))


def plan(c):
    """the launches a case must report: [(label prefix, {key: number in the label})]"""
    if isinstance(c, Dense):
        out = [('dense:delta_bias ', dict(rows=c.B, C=c.U)), ('dense:column_sum_finish ', dict(C=c.U)), ('dense:dw_plain ', dict(M=c.J, N=c.U, K=c.B))]
        if c.dz:
            nt = tile_nt(c.J)
            rt, ct = _ceil(c.B, BM), _ceil(c.J, 32 * nt)
            s = splits_of(rt * ct, _ceil(c.U, BK))
            out += [('dense:dz_mfma_f32 ', dict(M=c.B, N=c.J, K=c.U, tiles='%dx%d' % (rt, ct), nt=nt, splits=s)), ('dense:dz_reduce ', dict(splits=s))]
        return out
    x2 = (c.UH, c.UW) == (2 * c.H, 2 * c.W)
    P, U = (4, (c.KS + 1) // 2) if x2 else (1, c.KS)
    rows, kpix = U * U * c.Cin, c.B * c.H * c.W
    nt = tile_nt(c.Cout)
    rt, ct = _ceil(rows, BM), _ceil(c.Cout, 32 * nt)
    s = splits_of(P * rt * ct, _ceil(kpix, BK))
    out = [('up:delta_bias ', dict(rows=c.B * c.UH * c.UW, C=c.Cout)), ('up:column_sum_finish ', dict(C=c.Cout)),
           ('up:wgrad_mfma_f32 %d phases x ' % P, dict(M=rows, N=c.Cout, K=kpix, tiles='%dx%d' % (rt, ct), nt=nt, splits=s)),
           ('up:wgrad_reduce_unfold ', dict(phases=P, splits=s))]
    if c.g_in:
        dnt = tile_nt(c.Cin)
        out += [('up:fold_weights ', dict(phases=P, taps='%dx%d' % (U, U))),
                ('up:dgrad_mfma_f32 ', dict(M=kpix, N=c.Cin, K=4 * P * U * U * _ceil(c.Cout, 4), tiles='%dx%d' % (_ceil(kpix, BM), _ceil(c.Cin, 32 * dnt)), nt=dnt, splits=1))]
    return out


_NUMBER = re.compile(r'(\w+)=(\d+x\d+|\d+)')


def check_labels(c, labels):
    want = plan(c)
    assert len(labels) == len(want), (labels, want)
    for label, (prefix, numbers) in zip(labels, want):
        assert label.startswith(prefix), (label, prefix)
        got = dict(_NUMBER.findall(label))
        for key, value in numbers.items():
            assert got.get(key) == str(value), (label, key, value)


def check_table():
    """what the table exists for; a table that lost one of these fails at import"""
    cs = list(CASES.values())
    assert {c.KS for c in cs} >= {1, 3, 5, 7} and any(c.act == SIGMOID and c.Cout == 3 for c in cs)
    assert any((c.H, c.W) == (1, 1) for c in cs) and any((c.UH, c.UW) == (c.H, c.W) for c in cs) and any(not c.g_in for c in cs)
    assert any(c.Cin % 32 and c.Cout % 4 for c in cs) and any(c.Cout > 128 for c in cs)
    split = {dict(plan(c)[2][1])['splits'] for c in cs}
    assert 1 in split and max(split) > 1, split
    assert any((c.B * c.H * c.W) % BK for c in cs)
    ds = list(DENSE_CASES.values())
    assert {c.J for c in ds} == {128, 33} and {c.U for c in ds} == {96, 240} and {c.B for c in ds} == {1, 5, 67} and any(not c.dz for c in ds)


check_table()


# ---- the whole chain ------------------------------------------------------------------------------------------------------------------
def chain_reference(weights, names, z, acts, x, dx, dims, dtype=np.float64):
    """Back-propagation through a decoder without batch norm, from SAVED activations.  names = (dense, [conv...], final): the
    variables' names in `weights`; acts[0] the dense output [B, h0, w0, C0], acts[i] the output of hidden stage i; x the sigmoid
    output; dims[i] the resolution of acts[i].  dtype float64: the reference; float32: the same arithmetic in the precision of the
    device, in NumPy's order (what the chain tolerance is measured from).  Returns ({variable name: gradient}, dz, {name: S})."""
    dense, convs, final = names
    f = lambda a: np.asarray(a, dtype)
    grads, S = collections.OrderedDict(), {}
    stages = [(convs[i], acts[i], acts[i + 1], RELU) for i in range(len(convs))] + [(final, acts[-1], x, SIGMOID)]
    g = f(dx)
    for name, a_in, a_out, act in reversed(stages):
        UH, UW = a_out.shape[1:3]
        if dtype == np.float64:
            r = stage_reference_arrays(a_in, a_out, g, weights[name + '/kernel'], UH, UW, act)
            grads[name + '/kernel'], grads[name + '/bias'], g = r['dw'].val, r['db'].val, r['g_in'].val
            S[name + '/kernel'], S[name + '/bias'], S['g_in:' + name] = r['dw'].S, r['db'].S, r['g_in'].S
        else:
            d = ((g * f(a_out)) * (dtype(1) - f(a_out))) if act == SIGMOID else np.where(f(a_out) > 0, g, dtype(0))
            db, dw, g = _stage_products_typed(f(a_in), d.astype(dtype), f(weights[name + '/kernel']), UH, UW, dtype)
            grads[name + '/kernel'], grads[name + '/bias'] = dw, db
    a0 = f(acts[0]).reshape(len(z), -1)
    g = g.reshape(len(z), -1)
    if dtype == np.float64:
        r = dense_reference_arrays(z, a0, g, weights[dense + '/kernel'])
        grads[dense + '/kernel'], grads[dense + '/bias'], dz = r['dw'].val, r['db'].val, r['dz'].val
        S[dense + '/kernel'], S[dense + '/bias'], S['dz'] = r['dw'].S, r['db'].S, r['dz'].S
    else:
        d = np.where(a0 > 0, g, dtype(0)).astype(dtype)
        grads[dense + '/kernel'], grads[dense + '/bias'], dz = f(z).T @ d, d.sum(axis=0, dtype=dtype), d @ f(weights[dense + '/kernel']).T
    return grads, dz, S


def _stage_products_typed(a, d, w, UH, UW, dtype):
    """_stage_products with every array and every sum in `dtype`"""
    B, H, W, Cin = a.shape
    KS, Cout = w.shape[0], w.shape[3]
    p = (KS - 1) // 2
    iy, ix = resize_index(UH, H), resize_index(UW, W)
    up = np.zeros((B, UH + 2 * p, UW + 2 * p, Cin), dtype)
    up[:, p:p + UH, p:p + UW] = a[:, iy][:, :, ix]
    db = d.reshape(-1, Cout).sum(axis=0, dtype=dtype)
    dw = np.empty((KS, KS, Cin, Cout), dtype)
    g_up = np.zeros((B, UH + 2 * p, UW + 2 * p, Cin), dtype)
    for kh in range(KS):
        for kw in range(KS):
            dw[kh, kw] = up[:, kh:kh + UH, kw:kw + UW].reshape(-1, Cin).T @ d.reshape(-1, Cout)
            g_up[:, kh:kh + UH, kw:kw + UW] += d @ w[kh, kw].T
    g_up = g_up[:, p:p + UH, p:p + UW]
    g_in = np.zeros((B, H, W, Cin), dtype)
    for y in range(UH):
        for x in range(UW):
            g_in[:, iy[y], ix[x]] += g_up[:, y, x]
    return db, dw, g_in
