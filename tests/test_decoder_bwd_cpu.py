"""The decoder's backward pass without a GPU: the float64 restatement (tests/decoder_grad_reference.py) against central finite
differences of oracle.decoder_cpu.decoder_forward_np; csrc/kernels/decoder_bwd_core.h compiled for the host and run serially in
phase form by tests/native/decoder_bwd_host.cpp over the case table, the same driver under -fsanitize=address,undefined, and with
each of four seeded index mistakes (every one must be noticed by at least one case); and what the API checks before it touches the
device: arguments, the refusals (NotImplementedError by name), the symbols."""
import configparser
import os
import subprocess

import numpy as np
import pytest

import decoder_grad_reference as dg
from test_render_cpu import _compiler
from augmentedautoencoder_amd import _lib, ae_factory as factory, decoder_grad as G, session as S
from augmentedautoencoder_amd.weights import DecoderConfig
from oracle import decoder_cpu as dref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MISTAKES = {1: 'a phase offset off by one', 2: 'taps not flipped in the data gradient', 3: 'the border folded in', 4: 'parity x and y swapped'}


def _build(out_dir, flags, name):
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-O2', '-ffp-contract=off', '-Wall', '-Wno-unused-variable'] + flags +
                          [os.path.join(HERE, 'native', 'decoder_bwd_host.cpp'), '-o', exe])
    return exe


@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('decoder_bwd_host'), [], 'decoder_bwd_host')


def _run(exe, tmp_path, name, mutate=0):
    src, out = str(tmp_path / 'bwd_in.bin'), str(tmp_path / 'bwd_out.bin')
    if name in dg.CASES:
        c, inp = dg.CASES[name], dg.stage_inputs(name)
        head = [0, c.B, c.H, c.W, c.Cin, c.UH, c.UW, c.Cout, c.KS, c.act, int(c.g_in), 0]
        arrays = [inp[k] for k in ('a_in', 'a_out', 'g_out', 'w')]
        shapes = [('delta', (c.B, c.UH, c.UW, c.Cout)), ('db', (c.Cout,)), ('dw', (c.KS, c.KS, c.Cin, c.Cout))] + ([('g_in', (c.B, c.H, c.W, c.Cin))] if c.g_in else [])
    else:
        c, inp = dg.DENSE_CASES[name], dg.dense_inputs(name)
        head = [1, c.B, c.J, c.U, int(c.dz)] + [0] * 7
        arrays = [inp[k] for k in ('z', 'a_out', 'g_out', 'w')]
        shapes = [('delta', (c.B, c.U)), ('db', (c.U,)), ('dw', (c.J, c.U))] + ([('dz', (c.B, c.J))] if c.dz else [])
    with open(src, 'wb') as f:
        np.array(head, dtype=np.int32).tofile(f)
        for a in arrays:
            a.tofile(f)
    subprocess.check_call([exe] + (['--mutate', str(mutate)] if mutate else []) + [src, out])
    raw = np.fromfile(out, dtype=np.float32)
    got, at = {}, 0
    for key, shape in shapes:
        n = int(np.prod(shape))
        got[key] = raw[at:at + n].reshape(shape)
        at += n
    assert at == raw.size
    return got


def _ref(name):
    return dg.stage_reference(name) if name in dg.CASES else dg.dense_reference(name)


# ---- the restatement against finite differences -----------------------------------------------------------------------------------
def test_reference_matches_finite_differences_of_the_forward():
    """L2 loss with ratio 1 (every element selected: the selected set is the whole image and does not move) on a 2-stage
    network in float64: loss = mean_b mean_i (x - t)^2, dx = 2 (x - t) / (B n)."""
    out_shape, nf_enc, st_enc, k, latent, B = (8, 8, 3), (16, 32), (2, 2), 5, 8, 3
    cfg = DecoderConfig(out_shape, nf_enc, st_enc, k, latent)
    w = dref.make_decoder_weights(seed=99, out_shape=out_shape, num_filter=nf_enc, strides=st_enc, kernel_size=k, latent=latent)
    w = {n: np.asarray(a, np.float64) for n, a in w.items()}
    rng = np.random.default_rng(5)
    z = (np.round(rng.standard_normal((B, latent)) * 4096) / 4096).astype(np.float32)
    t = rng.random((B,) + out_shape)
    dense, convs, final, _ = cfg.variable_names(w)

    def loss_of(weights, zz):
        x = dref.decoder_forward_np(zz, weights, cfg.shape, cfg.num_filters, cfg.strides)
        return np.mean((x - t) ** 2)

    x, acts = dref.decoder_forward_np(z, w, cfg.shape, cfg.num_filters, cfg.strides, return_activations=True)
    assert x.size // B // 1 == x[0].size                                   # ratio 1: k = n, the selected set is every element
    dx = 2.0 * (x - t) / x.size
    grads, dz, _ = dg.chain_reference(w, (dense, convs, final), z, acts, x, dx, cfg.layer_dimensions())
    assert list(grads) == [final + '/kernel', final + '/bias', convs[0] + '/kernel', convs[0] + '/bias', dense + '/kernel', dense + '/bias']
    h = 1e-6
    worst = 0.0
    for name, g in grads.items():
        scale = np.abs(g).max()
        assert scale > 0, name
        flat = rng.choice(g.size, size=min(8, g.size), replace=False)
        for i in flat:
            idx = np.unravel_index(i, g.shape)
            up, dn = dict(w), dict(w)
            up[name], dn[name] = w[name].copy(), w[name].copy()
            up[name][idx] += h
            dn[name][idx] -= h
            fd = (loss_of(up, z) - loss_of(dn, z)) / (2 * h)
            worst = max(worst, abs(fd - g[idx]) / scale)
    print('reference against central differences: largest deviation %.2e of the tensor maximum' % worst)
    assert worst < 1e-6
    # dz: decoder_forward_np takes z as float32, so the step is a power of two on codes that are multiples of 2^-12 (exact)
    hz, worst_z = 2.0 ** -18, 0.0
    for b in range(B):
        for j in range(latent):
            up, dn = z.copy(), z.copy()
            up[b, j] += np.float32(hz)
            dn[b, j] -= np.float32(hz)
            fd = (loss_of(w, up) - loss_of(w, dn)) / (2 * hz)
            worst_z = max(worst_z, abs(fd - dz[b, j]) / np.abs(dz).max())
    print('dz against central differences (h = 2^-18): largest deviation %.2e of the maximum' % worst_z)
    assert np.abs(z).max() < 8 and worst_z < 1e-5          # (a ReLU whose input changes sign inside the step would show here: none does; an index mistake is O(1))


def test_cases_cover_what_they_claim():
    dg.check_table()
    for name in dg.CASES:
        a = dg.stage_inputs(name)['a_out']
        assert 0.35 < np.mean(a == 0) < 0.65, name
    c = dg.CASES['two_col_tiles']
    assert dict(dg.plan(c)[2][1])['tiles'] == '5x2' and dict(dg.plan(c)[2][1])['splits'] == 1
    assert dict(dg.plan(dg.CASES['split_k'])[2][1])['splits'] == 8


# ---- the core header on the host ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(dg.CASES) + list(dg.DENSE_CASES))
def test_host_driver_matches_reference(host_exe, tmp_path, name):
    worst = dg.check(name, _ref(name), _run(host_exe, tmp_path, name))
    print('%s: largest error in units of u S: %s' % (name, ' '.join('%s %.2f' % kv for kv in sorted(worst.items()))))


def test_seeded_mistakes_are_noticed(host_exe, tmp_path):
    counts = {}
    for m, what in MISTAKES.items():
        tripped = []
        for name in dg.CASES:
            try:
                dg.check(name, _ref(name), _run(host_exe, tmp_path, name, mutate=m))
            except AssertionError:
                tripped.append(name)
        counts[m] = len(tripped)
        print('mistake %d (%s): noticed by %d of %d cases: %s' % (m, what, len(tripped), len(dg.CASES), ' '.join(tripped)))
    assert all(n >= 1 for n in counts.values()), counts


def test_host_driver_under_sanitizers(tmp_path):
    """address + undefined-behaviour sanitizers on the stand-alone driver: the border gathers of every tap count, the 1x1 source, the 1x stage"""
    exe = _build(tmp_path, ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'], 'decoder_bwd_host_san')
    for name in ('ragged_3x5', 'cin40_cout5', 'ks1', 'ks7', 'one_pixel', 'plain_7x9', 'sigmoid_last', 'no_g_in', 'dense_J33_U96_B67'):
        dg.check(name, _ref(name), _run(exe, tmp_path, name))


# ---- the API, before the device ----------------------------------------------------------------------------------------------------
def test_argument_checks_need_no_gpu():
    import torch
    a_in, a_out, w = torch.zeros((2, 3, 4, 8)), torch.zeros((2, 6, 8, 5)), torch.zeros((5, 5, 8, 5))
    with pytest.raises(ValueError, match='GPU'):
        G.upconv_backward(a_in, a_out, a_out, w)
    with pytest.raises(ValueError, match='torch tensor'):
        G.upconv_backward(np.zeros((2, 3, 4, 8), np.float32), a_out, a_out, w)
    with pytest.raises(ValueError, match='float32'):
        G.upconv_backward(a_in.double(), a_out, a_out, w)
    with pytest.raises(ValueError, match='unknown activation'):
        G.upconv_backward(a_in, a_out, a_out, w, activation='tanh')
    with pytest.raises(ValueError, match='GPU'):
        G.dense_backward(torch.zeros((2, 8)), torch.zeros((2, 16)), torch.zeros((2, 16)), torch.zeros((8, 16)))
    with pytest.raises(ValueError, match='float32'):
        G.dense_backward(torch.zeros((2, 8), dtype=torch.float16), torch.zeros((2, 16)), torch.zeros((2, 16)), torch.zeros((8, 16)))
    G.check_resize(3, 5, 6, 10)
    G.check_resize(7, 9, 7, 9)
    for bad in ((3, 5, 7, 10), (3, 5, 9, 15), (3, 5, 6, 5), (7, 7, 15, 15)):
        with pytest.raises(NotImplementedError, match='only exact 2x and 1x'):
            G.check_resize(*bad)


NET_CFG = """
[Dataset]
H: %d
W: 16
C: 3
[Network]
BATCH_NORMALIZATION: %s
AUXILIARY_MASK: %s
VARIATIONAL: 0
LOSS: L2
BOOTSTRAP_RATIO: 4
NORM_REGULARIZE: 0.1
LATENT_SPACE_SIZE: 128
NUM_FILTER: [32, 64]
STRIDES: %s
KERNEL_SIZE_ENCODER: 5
KERNEL_SIZE_DECODER: 5
"""


def _pair(h=16, bn='False', mask='False', strides='[2, 2]'):
    args = configparser.ConfigParser()
    args.read_string(NET_CFG % (h, bn, mask, strides))
    enc = factory.build_encoder(S.Placeholder((h, 16, 3)), args)
    return enc, factory.build_decoder(S.Placeholder((h, 16, 3), 'reconst_target'), enc, args), args


def test_refusals_by_name():
    enc, dec, args = _pair()
    G.check_trainable(dec.config)
    feed = {dec._latent_code: np.zeros((1, 128), np.float32), dec.reconstruction_target: np.zeros((1, 16, 16, 3), np.float32)}
    enc_b, dec_b, _ = _pair(bn='True')
    with pytest.raises(NotImplementedError, match='batch_norm'):
        dec_b.gradients_device(feed)
    enc_m, dec_m, _ = _pair(mask='True')
    with pytest.raises(NotImplementedError, match='auxiliary_mask'):
        dec_m.gradients_device(feed)
    enc_r, dec_r, _ = _pair(h=30, strides='[2, 2]')                    # int(30 / 4) = 7 -> 15: neither 2x nor 1x
    with pytest.raises(NotImplementedError, match='only exact 2x and 1x'):
        dec_r.gradients_device(feed)
    enc_3, dec_3, _ = _pair(h=18, strides='[3, 3]')
    with pytest.raises(NotImplementedError, match='only exact 2x and 1x'):
        G.check_trainable(dec_3.config)
    G.check_trainable(_pair(strides='[1, 2]')[1].config)                # a 1x stage trains
    for name in ('build_queue', 'build_train_op'):
        with pytest.raises(NotImplementedError, match=name):
            getattr(factory, name)(None, None)
    with pytest.raises(NotImplementedError, match='is_training'):
        factory.build_decoder(S.Placeholder((16, 16, 3)), enc, args, is_training=True)
    ae = factory.build_ae(enc, dec, args)
    assert callable(ae.gradients_device) and callable(dec.gradients_device)


def test_backward_symbols_declared_bound_and_exported():
    import ctypes
    header = open(os.path.join(ROOT, 'include', 'aae_hip.h')).read()
    import __graft_entry__ as g
    g.build()
    out = subprocess.check_output(['/opt/rocm/lib/llvm/bin/llvm-readelf', '--dyn-syms', '--wide', g.LIB]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if ' FUNC ' in l and ' UND ' not in l)
    for name in ('aae_upconv_backward_workspace_bytes', 'aae_upconv_backward', 'aae_dense_backward_workspace_bytes', 'aae_dense_backward', 'aae_decoder_get_desc',
                 'aae_decoder_backward_workspace_bytes', 'aae_decoder_backward', 'aae_decoder_backward_timed', 'aae_decoder_bwd_label_count', 'aae_decoder_bwd_label'):
        assert name + '(' in header and name in _lib.EXPORTED_SYMBOLS and name in exported, name
    assert _lib.AAE_ABI_VERSION == 3 and '#define AAE_ABI_VERSION 3' in header
    assert ctypes.sizeof(_lib.UpconvBackwardDesc) == 36 and ctypes.sizeof(_lib.DenseBackwardDesc) == 12
