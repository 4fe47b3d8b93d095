"""The encoder's backward pass restated in float64 NumPy, in its DIRECT form: the input is padded as oracle.reference_cpu.same_pad says,
every tap of the KS x KS kernel is its own strided slice, nothing is split by parity -- so the parity kernels
(csrc/kernels/encoder_bwd_core.h, encoder_bwd_f32.h) are checked against something that shares no index map with them.
TEST INFRASTRUCTURE ONLY.

For a layer  a_out = relu(conv(a_in, w, stride S, 'same') + b)  and g_out = dL/da_out, (pt, pb), (pl, pr) from same_pad:
    delta = g_out where a_out > 0 else 0;   db[co] = sum_{b,oy,ox} delta
    dw[kh,kw,ci,co] = sum_{b,oy,ox} a_in[b, S oy + kh - pt, S ox + kw - pl, ci] delta[b,oy,ox,co]      (taps in the padding: nothing)
    g_in[b,iy,ix,ci] = sum delta[b,oy,ox,co] w[kh,kw,ci,co] over the (kh, kw) with S oy + kh - pt = iy, S ox + kw - pl = ix
For the linear dense layer z = a w + b:  dw = a^T dz, db = sum_b dz, g_a = dz w^T.

Every gradient comes with S = sum |products| and the term count n of each element.  The bound of a fp32 evaluation in ANY summation
order is |got - ref64| <= gamma_n S <~ n u S, u = 2^-24; the checks allow (n + 8) u S, the 8 as in decoder_grad_reference.py (the
K-split partials and the final reduce are roundings already counted in n but grouped differently).  An input pixel that no tap
reaches (KS 1, S 2: the odd parities) has n = 0 and S = 0: the bound is 0, the device must write an exact zero.  The reference is
evaluated on exactly the arrays the call was given (a uint8 a_in through the table float32(v / 255.)), so the ReLU masks agree
by construction and no element is left out.

Measured on the MI355X (tests/test_gpu_encoder_bwd.py), largest |got - ref64| / (u S) over the table: see that file's header.

The case table (CASES, DENSE_CASES) holds the smallest shapes at which each thing can go wrong; plan() restates the launch planner
(aae_encoder_bwd_impl.h) so that a test can pin the form, the tile counts and the K splits a case ran with."""
import collections
import functools
import re

import numpy as np

from oracle import reference_cpu as ref_cpu

U32 = 2.0 ** -24
SLACK = 8

Layer = collections.namedtuple('Layer', 'name B H W Cin Cout KS S u8 g_in')
Dense = collections.namedtuple('Dense', 'name B J U g_a')

CASES = collections.OrderedDict((c.name, c) for c in [
    Layer('conv1_f32', 2, 16, 16, 3, 32, 5, 2, False, False),          # first layer, no g_in; pads (1, 2)
    Layer('conv1_u8', 2, 16, 16, 3, 32, 5, 2, True, False),            # ... from uint8
    Layer('conv1_dx', 1, 16, 16, 3, 32, 5, 2, False, True),            # g_in with Cin 3
    Layer('even_8x12', 3, 8, 12, 32, 64, 5, 2, False, True),           # non-square
    Layer('mixed_7x10', 2, 7, 10, 20, 36, 5, 2, False, True),          # pads (2, 2) in y and (1, 2) in x: a swapped axis shows
    Layer('odd_9x9', 2, 9, 9, 8, 8, 5, 2, False, True),                # pads (2, 2), Ho = 5
    Layer('k3_6x6', 2, 6, 6, 8, 8, 3, 2, False, True),                 # pads (0, 1)
    Layer('k4_8x8', 1, 8, 8, 4, 12, 4, 2, False, True),                # even KS, pads (1, 1)
    Layer('k1_8x8', 2, 8, 8, 8, 8, 1, 2, False, True),                 # odd-parity pixels receive exact zeros
    Layer('s1_5x6', 2, 5, 6, 12, 20, 5, 1, False, True),               # stride 1
    Layer('tiny_2x2', 3, 2, 2, 16, 16, 5, 2, False, True),             # image smaller than the kernel, Ho = 1, pads (1, 2)
    Layer('row_1x7', 2, 1, 7, 8, 8, 5, 2, False, True),                # H = 1
    Layer('ragged_ch', 1, 4, 4, 33, 130, 5, 2, False, True),           # every tile edge, NT = 4 plus a ragged column tile
    Layer('split_k', 5, 32, 32, 8, 16, 5, 2, False, True),             # K = 1280: K split and a fixed-order reduce
    Layer('wide', 2, 8, 8, 160, 64, 5, 2, False, True),                # more than one row tile per tap
    # the two weight-gradient instances the shapes above do not reach
    Layer('nt2_scalar', 1, 4, 4, 6, 40, 5, 2, False, True),            # 64 columns with single-word loads
    Layer('nt4_quads', 1, 4, 4, 8, 132, 3, 2, False, True),            # 128 columns with 16-byte loads
])

DENSE_CASES = collections.OrderedDict((c.name, c) for c in [
    Dense('linear_B5_J160_U128', 5, 160, 128, True),
    Dense('linear_B67_J33_U20', 67, 33, 20, True),
    Dense('linear_B1_J4096_U128', 1, 4096, 128, True),
    Dense('linear_B5_J160_U128_no_g_a', 5, 160, 128, False),
    Dense('linear_B2_J32_U8', 2, 32, 8, True),                         # the 32-column instance of the g_a kernel
])


def _seed(name):
    return 9000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


def _readonly(d):
    for v in d.values():
        v.setflags(write=False)
    return d


def out_shape(c):
    return ref_cpu.same_pad(c.H, c.KS, c.S)[0], ref_cpu.same_pad(c.W, c.KS, c.S)[0]


@functools.lru_cache(maxsize=None)
def layer_inputs(name):
    c = CASES[name]
    rng = np.random.default_rng(_seed(name))
    Ho, Wo = out_shape(c)
    if c.u8:
        a_in = rng.integers(0, 256, (c.B, c.H, c.W, c.Cin), dtype=np.uint8)
    else:
        a_in = (rng.standard_normal((c.B, c.H, c.W, c.Cin)) * (rng.random((c.B, c.H, c.W, c.Cin)) < 0.7)).astype(np.float32)
    a_out = np.abs(rng.standard_normal((c.B, Ho, Wo, c.Cout))) + 0.01
    a_out[rng.random(a_out.shape) < 0.5] = 0.0
    return _readonly(dict(a_in=a_in, a_out=a_out.astype(np.float32), g_out=rng.standard_normal((c.B, Ho, Wo, c.Cout)).astype(np.float32),
                          w=(rng.standard_normal((c.KS, c.KS, c.Cin, c.Cout)) * 0.1).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def dense_inputs(name):
    c = DENSE_CASES[name]
    rng = np.random.default_rng(_seed(name))
    return _readonly(dict(a=(rng.standard_normal((c.B, c.J)) * (rng.random((c.B, c.J)) < 0.6)).astype(np.float32), dz=rng.standard_normal((c.B, c.U)).astype(np.float32),
                          w=(rng.standard_normal((c.J, c.U)) * 0.1).astype(np.float32)))


# ---- the direct formulas ------------------------------------------------------------------------------------------------------------
def input_values(a_in):
    """the float32 values a layer input stands for: a uint8 array through the forward's table"""
    a_in = np.asarray(a_in)
    return ref_cpu.u8_lut_f32()[a_in] if a_in.dtype == np.uint8 else a_in


def _layer_products(a, d, w, S, want_g_in=True, dtype=np.float64):
    """db, dw, g_in of the direct formulas for a [B,H,W,Cin], d [B,Ho,Wo,Cout], w [KS,KS,Cin,Cout], all sums in dtype"""
    B, H, W, Cin = a.shape
    KS, Cout = w.shape[0], w.shape[3]
    Ho, pt, pb = ref_cpu.same_pad(H, KS, S)
    Wo, pl, pr = ref_cpu.same_pad(W, KS, S)
    assert d.shape == (B, Ho, Wo, Cout), (d.shape, (B, Ho, Wo, Cout))
    xp = np.zeros((B, H + pt + pb, W + pl + pr, Cin), dtype)
    xp[:, pt:pt + H, pl:pl + W] = a
    db = d.reshape(-1, Cout).sum(axis=0, dtype=dtype)
    dw = np.empty((KS, KS, Cin, Cout), dtype)
    g_pad = np.zeros_like(xp)
    for kh in range(KS):
        for kw in range(KS):
            dw[kh, kw] = xp[:, kh:kh + S * Ho:S, kw:kw + S * Wo:S].reshape(-1, Cin).T @ d.reshape(-1, Cout)
            if want_g_in:
                g_pad[:, kh:kh + S * Ho:S, kw:kw + S * Wo:S] += d @ w[kh, kw].T
    return db, dw, (g_pad[:, pt:pt + H, pl:pl + W] if want_g_in else None)


Ref = collections.namedtuple('Ref', 'val S n')


def layer_reference_arrays(a_in, a_out, g_out, w, S, want_g_in=True):
    """{'delta' | 'db' | 'dw' | 'g_in': Ref(val, S, n)} in float64, from the arrays a call is given"""
    a, w64 = np.asarray(input_values(a_in), np.float64), np.asarray(w, np.float64)
    d = np.where(np.asarray(a_out) > 0, np.asarray(g_out, np.float64), 0.0)
    val = _layer_products(a, d, w64, S, want_g_in)
    Sv = _layer_products(np.abs(a), np.abs(d), np.abs(w64), S, want_g_in)
    n = _layer_products(np.ones_like(a), np.ones_like(d), np.ones_like(w64), S, want_g_in)
    out = {'delta': Ref(d, np.abs(d), np.ones(d.shape))}
    for key, v, s, k in zip(('db', 'dw', 'g_in'), val, Sv, n):
        if v is not None:
            out[key] = Ref(v, s, k)
    return out


def dense_reference_arrays(a, dz, w, want_g_a=True):
    a64, d, w64 = np.asarray(a, np.float64), np.asarray(dz, np.float64), np.asarray(w, np.float64)
    B, J = a64.shape
    U = w64.shape[1]
    out = {'db': Ref(d.sum(axis=0), np.abs(d).sum(axis=0), np.full((U,), float(B))),
           'dw': Ref(a64.T @ d, np.abs(a64).T @ np.abs(d), np.full((J, U), float(B)))}
    if want_g_a:
        out['g_a'] = Ref(d @ w64.T, np.abs(d) @ np.abs(w64).T, np.full((B, J), float(U)))
    return out


@functools.lru_cache(maxsize=None)
def layer_reference(name):
    c, i = CASES[name], layer_inputs(name)
    return layer_reference_arrays(i['a_in'], i['a_out'], i['g_out'], i['w'], c.S, c.g_in)


@functools.lru_cache(maxsize=None)
def dense_reference(name):
    c, i = DENSE_CASES[name], dense_inputs(name)
    return dense_reference_arrays(i['a'], i['dz'], i['w'], c.g_a)


def check(name, ref, got):
    """got: {'delta' | 'db' | 'dw' | 'g_in' | 'g_a': float32 array}.  Asserts the per-element bound on EVERY element of every
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
        if bad.any():
            i = tuple(np.argwhere(bad)[0])
            raise AssertionError('%s: %s misses (n + %d) u S at %d of %d elements; first %s: got %r, ref %r, S %r, n %r' % (
                name, key, SLACK, bad.sum(), bad.size, list(i), g[i], r.val[i], r.S[i], r.n[i]))
    return worst


# ---- the launch planner, restated (aae_encoder_bwd_impl.h: plan_conv, plan_linear, choose_splits) --------------------------------------
TARGET_BLOCKS, MAX_SPLITS, BM, BK = 512, 256, 128, 32


def _ceil(a, b):
    return -(-a // b)


def tile_nt(n):
    return 1 if n <= 32 else (2 if n <= 64 else 4)


def splits_of(tiles, slabs):
    s = max(1, min(_ceil(TARGET_BLOCKS, tiles), MAX_SPLITS, slabs))
    return _ceil(slabs, _ceil(slabs, s))


def plan(c, prefix=None):
    """the launches a case must report: [(label prefix, {key: number or word in the label})]"""
    if isinstance(c, Dense):
        out = [('dense:column_partial ', dict(rows=c.B, C=c.U)), ('dense:column_sum_finish ', dict(C=c.U)), ('dense:dw_plain ', dict(M=c.J, N=c.U, K=c.B))]
        if c.g_a:
            nt = tile_nt(c.J)
            rt, ct = _ceil(c.B, BM), _ceil(c.J, 32 * nt)
            s = splits_of(rt * ct, _ceil(c.U, BK))
            out.append(('dense:ga_mfma_f32 ', dict(M=c.B, N=c.J, K=c.U, tiles='%dx%d' % (rt, ct), nt=nt, splits=s)))
            if s > 1:
                out.append(('dense:ga_reduce ', dict(splits=s)))
        return out
    p = prefix or 'conv'
    Ho, Wo = out_shape(c)
    M, K = c.KS * c.KS * c.Cin, c.B * Ho * Wo
    nt = tile_nt(c.Cout)
    rt, ct = _ceil(M, BM), _ceil(c.Cout, 32 * nt)
    s = splits_of(rt * ct, _ceil(K, BK))
    load = 'u8' if c.u8 else ('x4' if c.Cin % 4 == 0 else 'x1')
    out = [(p + ':delta_bias ', dict(rows=K, C=c.Cout)), (p + ':column_sum_finish ', dict(C=c.Cout)),
           (p + ':wgrad_mfma_f32 ', dict(M=M, N=c.Cout, K=K, tiles='%dx%d' % (rt, ct), nt=nt, load=load, splits=s))]
    if s > 1:
        out.append((p + ':wgrad_reduce ', dict(splits=s)))
    if c.g_in:
        dnt = tile_nt(c.Cin)
        rows0 = c.B * _ceil(c.H, c.S) * _ceil(c.W, c.S)
        out.append((p + ':dgrad_parity_mfma_f32 ', dict(parities=c.S * c.S, M=c.B * c.H * c.W, N=c.Cin, K=c.KS * c.KS * 4 * _ceil(c.Cout, 4),
                                                         tiles='%dx%d' % (_ceil(rows0, BM), _ceil(c.Cin, 32 * dnt)), nt=dnt, splits=1)))
    return out


_NUMBER = re.compile(r'(\w+)=(\d+x\d+|\w+)')


def check_labels(c, labels, prefix=None):
    want = plan(c, prefix)
    assert len(labels) == len(want), (labels, want)
    for label, (prefix_, numbers) in zip(labels, want):
        assert label.startswith(prefix_), (label, prefix_)
        got = dict(_NUMBER.findall(label))
        for key, value in numbers.items():
            assert got.get(key) == str(value), (label, key, value)


def check_table():
    """what the table exists for: every launch form is reached by some case; a table that lost one fails at import"""
    cs = list(CASES.values())
    wgrad = {(tile_nt(c.Cout), 'u8' if c.u8 else c.Cin % 4 == 0) for c in cs}
    assert wgrad >= {(nt, v) for nt in (1, 2, 4) for v in (True, False)} | {(1, 'u8')}, wgrad
    assert {tile_nt(c.Cin) for c in cs if c.g_in} == {1, 2, 4} and any(not c.g_in for c in cs)
    assert {c.S for c in cs} == {1, 2} and {c.KS for c in cs} >= {1, 3, 4, 5} and any(c.H != c.W for c in cs)
    assert any(c.Cout % 4 for c in cs if c.g_in) and any(c.Cout % 4 == 0 for c in cs if c.g_in)        # both delta / w load widths of the data gradient
    splits = {dict(plan(c)[2][1])['splits'] for c in cs}
    assert 1 in splits and max(splits) > 1, splits
    assert any(_ceil(c.KS * c.KS * c.Cin, BM) > c.KS * c.KS for c in cs)                                # more than one row tile per tap
    assert any(ref_cpu.same_pad(c.H, c.KS, c.S)[1:] != ref_cpu.same_pad(c.W, c.KS, c.S)[1:] for c in cs)
    assert any(c.KS < c.S for c in cs)                                                                  # a parity class without a tap
    ds = list(DENSE_CASES.values())
    assert {tile_nt(c.J) for c in ds if c.g_a} == {1, 2, 4} and any(not c.g_a for c in ds)
    dsplit = {dict(plan(c)[3][1])['splits'] for c in ds if c.g_a}
    assert 1 in dsplit and max(dsplit) > 1, dsplit


check_table()


# ---- the whole chain ------------------------------------------------------------------------------------------------------------------
def chain_reference(weights, strides, x, acts, dz, dtype=np.float64):
    """Back-propagation through an encoder without batch norm, from SAVED activations: x the input batch (float32 or uint8), acts[i]
    the output of conv layer i, dz = dL/dz.  dtype float64: the reference; float32: the same arithmetic in the precision of the
    device, in NumPy's order (what the chain tolerance is measured from).  Returns ({variable name: gradient}, dx, {name: S})."""
    convs, _ = ref_cpu.layer_names(len(strides), False)
    f = lambda a: np.asarray(a, dtype)
    grads, S = collections.OrderedDict(), {}
    B = len(dz)
    flat = f(acts[-1]).reshape(B, -1)
    wd = f(weights['dense/kernel'])
    if dtype == np.float64:
        r = dense_reference_arrays(flat, dz, wd)
        dense = (r['dw'].val, r['db'].val)
        S['dense/kernel'], S['dense/bias'] = r['dw'].S, r['db'].S
        g = r['g_a'].val
    else:
        dense = (flat.T @ f(dz), f(dz).sum(axis=0, dtype=dtype))
        g = f(dz) @ wd.T
    g = g.reshape(acts[-1].shape)
    per_layer = {}
    for i in reversed(range(len(strides))):
        a_in = input_values(x) if i == 0 else acts[i - 1]
        name = convs[i]
        if dtype == np.float64:
            r = layer_reference_arrays(a_in, acts[i], g, weights[name + '/kernel'], strides[i])
            per_layer[name] = (r['dw'].val, r['db'].val)
            S[name + '/kernel'], S[name + '/bias'], S['g_in:' + name] = r['dw'].S, r['db'].S, r['g_in'].S
            g = r['g_in'].val
        else:
            d = np.where(f(acts[i]) > 0, g, dtype(0)).astype(dtype)
            db, dw, g = _layer_products(f(a_in), d, f(weights[name + '/kernel']), strides[i], True, dtype)
            per_layer[name] = (dw, db)
    for name in convs:
        grads[name + '/kernel'], grads[name + '/bias'] = per_layer[name]
    grads['dense/kernel'], grads['dense/bias'] = dense
    return grads, g, S
