"""The encoder's backward pass without a GPU: the float64 restatement (tests/encoder_grad_reference.py) against central finite
differences of oracle.reference_cpu.conv2d_same_relu_np and encoder_forward_np; csrc/kernels/encoder_bwd_core.h compiled for the host
and run serially in parity form by tests/native/encoder_bwd_host.cpp over the case table, the same driver under
-fsanitize=address,undefined, and with each of five seeded index mistakes (every one must be noticed by at least one case); and what
the API checks before it touches the device: arguments, the refusals (NotImplementedError by name), the symbols.

Finite differences: float64 throughout, h = 1e-6.  On these cases the restatement deviates from the central difference by at most
2e-9 of the tensor's maximum (the truncation error of a piecewise-linear function is zero away from a ReLU kink, what is left is
the rounding of the difference quotient, about 1e-16 |loss| / h); the allowance is 4e-9, section 4j's.  An index mistake is O(1)."""
import os
import subprocess

import numpy as np
import pytest

import encoder_grad_reference as eg
from test_render_cpu import _compiler
from augmentedautoencoder_amd import _lib, encoder_grad as G
from augmentedautoencoder_amd.weights import EncoderConfig
from oracle import reference_cpu as ref
from oracle import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MISTAKES = {1: 'pads (before, after) swapped', 2: 'parity tap residue off by one', 3: 'taps not matched to w in the data gradient', 4: 'x and y pads exchanged',
            5: 'zero-parity pixels left unwritten'}
FD_ALLOWANCE = 4e-9


def _build(out_dir, flags, name):
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-O2', '-ffp-contract=off', '-Wall', '-Wno-unused-variable'] + flags +
                          [os.path.join(HERE, 'native', 'encoder_bwd_host.cpp'), '-o', exe])
    return exe


@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('encoder_bwd_host'), [], 'encoder_bwd_host')


def _run(exe, tmp_path, name, mutate=0):
    src, out = str(tmp_path / 'bwd_in.bin'), str(tmp_path / 'bwd_out.bin')
    if name in eg.CASES:
        c, inp = eg.CASES[name], eg.layer_inputs(name)
        head = [0, c.B, c.H, c.W, c.Cin, c.Cout, c.KS, c.S, int(c.u8), int(c.g_in), 0, 0]
        a_in = inp['a_in']
        if c.u8:
            a_in = np.concatenate([a_in.reshape(-1), np.zeros((-a_in.size) % 4, np.uint8)])
        arrays = [a_in] + [inp[k] for k in ('a_out', 'g_out', 'w')]
        shapes = [('delta', inp['a_out'].shape), ('db', (c.Cout,)), ('dw', (c.KS, c.KS, c.Cin, c.Cout))] + ([('g_in', (c.B, c.H, c.W, c.Cin))] if c.g_in else [])
    else:
        c, inp = eg.DENSE_CASES[name], eg.dense_inputs(name)
        head = [1, c.B, c.J, c.U, int(c.g_a)] + [0] * 7
        arrays = [inp[k] for k in ('a', 'dz', 'w')]
        shapes = [('db', (c.U,)), ('dw', (c.J, c.U))] + ([('g_a', (c.B, c.J))] if c.g_a else [])
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
    return eg.layer_reference(name) if name in eg.CASES else eg.dense_reference(name)


# ---- the restatement against finite differences -----------------------------------------------------------------------------------
def _fd_check(loss_of, tensors, grads, rng, h=1e-6, picks=10):
    worst = 0.0
    for name, g in grads.items():
        scale = np.abs(g).max()
        assert scale > 0, name
        for i in rng.choice(g.size, size=min(picks, g.size), replace=False):
            idx = np.unravel_index(i, g.shape)
            up, dn = dict(tensors), dict(tensors)
            up[name], dn[name] = tensors[name].copy(), tensors[name].copy()
            up[name][idx] += h
            dn[name][idx] -= h
            worst = max(worst, abs((loss_of(up) - loss_of(dn)) / (2 * h) - g[idx]) / scale)
    return worst


@pytest.mark.parametrize('name', ['mixed_7x10', 'odd_9x9', 'k4_8x8', 'k1_8x8', 's1_5x6', 'tiny_2x2', 'row_1x7'])
def test_layer_reference_matches_finite_differences(name):
    """loss = sum(relu(conv(a, w) + b) * g_out): its gradients are dw, db and g_in for delta = g_out where the output is positive"""
    c = eg.CASES[name]
    rng = np.random.default_rng(31)
    Ho, Wo = eg.out_shape(c)
    t = dict(a=rng.standard_normal((c.B, c.H, c.W, c.Cin)), w=rng.standard_normal((c.KS, c.KS, c.Cin, c.Cout)) * 0.3, b=rng.standard_normal((c.Cout,)) * 0.1)
    g_out = rng.standard_normal((c.B, Ho, Wo, c.Cout))
    loss_of = lambda tt: float(np.sum(ref.conv2d_same_relu_np(tt['a'], tt['w'], tt['b'], c.S) * g_out))
    a_out = ref.conv2d_same_relu_np(t['a'], t['w'], t['b'], c.S)
    d = np.where(a_out > 0, g_out, 0.0)
    db, dw, g_in = eg._layer_products(t['a'], d, t['w'], c.S)
    worst = _fd_check(loss_of, t, dict(a=g_in, w=dw, b=db), rng)
    print('%s: restatement against central differences: largest deviation %.2e of the tensor maximum' % (name, worst))
    assert worst < FD_ALLOWANCE


def test_chain_reference_matches_finite_differences_of_the_forward():
    shape, filters, strides, latent, B = (9, 10, 3), (6, 8), (2, 1), 7, 3
    w = {k: np.asarray(v, np.float64) for k, v in synth.make_weights(seed=41, shape=shape, num_filter=list(filters), strides=list(strides), latent=latent).items()}
    rng = np.random.default_rng(6)
    x = rng.random((B,) + shape).astype(np.float32)
    gz = rng.standard_normal((B, latent))
    loss_of = lambda ww: float(np.sum(ref.encoder_forward_np(x, ww, list(strides)) * gz))
    _, acts = ref.encoder_forward_np(x, w, list(strides), return_activations=True)
    grads, dx, _ = eg.chain_reference(w, list(strides), x, acts, gz)
    assert list(grads) == ['conv2d/kernel', 'conv2d/bias', 'conv2d_1/kernel', 'conv2d_1/bias', 'dense/kernel', 'dense/bias']
    worst = _fd_check(loss_of, w, grads, rng)
    print('chain restatement against central differences: largest deviation %.2e of the tensor maximum' % worst)
    assert worst < FD_ALLOWANCE and dx.shape == x.shape and np.abs(dx).max() > 0


def test_cases_cover_what_they_claim():
    eg.check_table()
    pads = lambda c: (ref.same_pad(c.H, c.KS, c.S)[1:], ref.same_pad(c.W, c.KS, c.S)[1:])
    assert pads(eg.CASES['conv1_f32']) == ((1, 2), (1, 2)) and pads(eg.CASES['mixed_7x10']) == ((2, 2), (1, 2)) and pads(eg.CASES['odd_9x9']) == ((2, 2), (2, 2))
    assert pads(eg.CASES['k3_6x6']) == ((0, 1), (0, 1)) and pads(eg.CASES['k4_8x8']) == ((1, 1), (1, 1)) and pads(eg.CASES['tiny_2x2']) == ((1, 2), (1, 2))
    assert eg.out_shape(eg.CASES['odd_9x9']) == (5, 5) and eg.out_shape(eg.CASES['tiny_2x2']) == (1, 1)
    for name in eg.CASES:
        assert 0.35 < np.mean(eg.layer_inputs(name)['a_out'] == 0) < 0.65, name
    assert dict(eg.plan(eg.CASES['split_k'])[2][1])['splits'] == 40 and dict(eg.plan(eg.CASES['ragged_ch'])[2][1])['tiles'] == '7x2'
    assert dict(eg.plan(eg.CASES['wide'])[2][1])['tiles'] == '32x1'
    # the forward's table of a uint8 input is one correctly rounded float32 division: what the kernel computes
    assert np.array_equal(np.arange(256, dtype=np.float32) / np.float32(255.0), ref.u8_lut_f32())


# ---- the core header on the host ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(eg.CASES) + list(eg.DENSE_CASES))
def test_host_driver_matches_reference(host_exe, tmp_path, name):
    worst = eg.check(name, _ref(name), _run(host_exe, tmp_path, name))
    print('%s: largest error in units of u S: %s' % (name, ' '.join('%s %.2f' % kv for kv in sorted(worst.items()))))


def test_seeded_mistakes_are_noticed(host_exe, tmp_path):
    counts = {}
    for m, what in MISTAKES.items():
        tripped = []
        for name in eg.CASES:
            try:
                eg.check(name, _ref(name), _run(host_exe, tmp_path, name, mutate=m))
            except AssertionError:
                tripped.append(name)
        counts[m] = len(tripped)
        print('mistake %d (%s): noticed by %d of %d cases: %s' % (m, what, len(tripped), len(eg.CASES), ' '.join(tripped)))
    assert all(n >= 1 for n in counts.values()), counts


def test_host_driver_under_sanitizers(tmp_path):
    """address + undefined-behaviour sanitizers on the stand-alone driver, over the whole table"""
    exe = _build(tmp_path, ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'], 'encoder_bwd_host_san')
    for name in list(eg.CASES) + list(eg.DENSE_CASES):
        eg.check(name, _ref(name), _run(exe, tmp_path, name))


# ---- the API, before the device ----------------------------------------------------------------------------------------------------
def test_argument_checks_need_no_gpu():
    import torch
    a_in, a_out, w = torch.zeros((2, 6, 8, 8)), torch.zeros((2, 3, 4, 5)), torch.zeros((5, 5, 8, 5))
    with pytest.raises(ValueError, match='GPU'):
        G.conv_backward(a_in, a_out, a_out, w, 2)
    with pytest.raises(ValueError, match='GPU'):
        G.conv_backward(a_in.to(torch.uint8), a_out, a_out, w, 2)
    with pytest.raises(ValueError, match='torch tensor'):
        G.conv_backward(np.zeros((2, 6, 8, 8), np.float32), a_out, a_out, w, 2)
    with pytest.raises(ValueError, match='float32'):
        G.conv_backward(a_in.double(), a_out, a_out, w, 2)
    with pytest.raises(ValueError, match='GPU'):
        G.linear_backward(torch.zeros((2, 8)), torch.zeros((2, 16)), torch.zeros((8, 16)))
    with pytest.raises(ValueError, match='float32'):
        G.linear_backward(torch.zeros((2, 8), dtype=torch.float16), torch.zeros((2, 16)), torch.zeros((8, 16)))
    G.check_stride(1, 7)
    G.check_stride(2, 1)
    with pytest.raises(NotImplementedError, match='stride 3'):
        G.check_stride(3)
    with pytest.raises(NotImplementedError, match='kernel size 9'):
        G.check_stride(2, 9)


def test_refusals_by_name():
    G.check_trainable(EncoderConfig((16, 16, 3), (8, 8), (2, 1), 5, 16))
    with pytest.raises(NotImplementedError, match='batch_norm'):
        G.check_trainable(EncoderConfig((16, 16, 3), (8, 8), (2, 2), 5, 16, batch_norm=True))
    with pytest.raises(NotImplementedError, match='stride 3'):
        G.check_trainable(EncoderConfig((18, 18, 3), (8, 8), (3, 2), 5, 16))
    from augmentedautoencoder_amd import ae_factory as factory
    for name in ('build_queue', 'build_train_op'):
        with pytest.raises(NotImplementedError, match=name):
            getattr(factory, name)(None, None)


def test_backward_symbols_declared_bound_and_exported():
    import ctypes
    header = open(os.path.join(ROOT, 'include', 'aae_hip.h')).read()
    import __graft_entry__ as g
    g.build()
    out = subprocess.check_output(['/opt/rocm/lib/llvm/bin/llvm-readelf', '--dyn-syms', '--wide', g.LIB]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if ' FUNC ' in l and ' UND ' not in l)
    for name in ('aae_conv_backward_workspace_bytes', 'aae_conv_backward', 'aae_linear_backward_workspace_bytes', 'aae_linear_backward', 'aae_encoder_get_desc',
                 'aae_encoder_backward_workspace_bytes', 'aae_encoder_backward', 'aae_encoder_backward_timed', 'aae_encoder_bwd_label_count', 'aae_encoder_bwd_label'):
        assert name + '(' in header and name in _lib.EXPORTED_SYMBOLS and name in exported, name
    assert _lib.AAE_ABI_VERSION == 3 and '#define AAE_ABI_VERSION 3' in header
    assert ctypes.sizeof(_lib.ConvBackwardDesc) == 32
