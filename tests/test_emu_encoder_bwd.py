"""The encoder's backward kernels (csrc/kernels/encoder_bwd_f32.h) and their host code (csrc/aae_encoder_bwd_impl.h) on the CPU fiber
emulator: tests/emu/encoder_bwd_emu.cpp, built here with the compiler and flags of tests/emu/Makefile, exports the library's own
entry points on host pointers.  The case table of tests/encoder_grad_reference.py runs through aae_conv_backward /
aae_linear_backward with the outputs handed in full of NaN and the workspace full of 0xA5; every element of delta, db, dw, g_in / g_a
is held to (n + 8) u S against the direct float64 formulas, the labels to the planner's restatement, a second call to the same bits.
What the emulator proves: the MFMA fragment maps, the k-major and row-major slab layouts, the strided gathers and the parity maps,
the masks of ragged tiles, the K splits.  What it cannot: timing, bank conflicts, the order of the hardware's fp32 sums (the GPU test)."""
import ctypes
import fcntl
import os
import subprocess

import numpy as np
import pytest

import encoder_grad_reference as eg

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, 'emu')
CSRC = os.path.join(HERE, '..', 'augmentedautoencoder_amd', 'csrc')
_LIB = None
_P = ctypes.c_void_p


class ConvDesc(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ('B', 'H', 'W', 'Cin', 'Cout', 'KS', 'S', 'x_dtype')]


class DenseDesc(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ('B', 'J', 'U')]


def _lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(EMU, 'libencoder_bwd_emu.so')
        deps = [os.path.join(EMU, f) for f in ('encoder_bwd_emu.cpp', 'hip_emu.cpp', 'hip_emu.h')]
        deps += [os.path.join(CSRC, 'aae_encoder_bwd_impl.h')]
        deps += [os.path.join(CSRC, 'kernels', f) for f in ('encoder_bwd_core.h', 'encoder_bwd_f32.h', 'decoder_bwd_core.h', 'decoder_bwd_f32.h', 'tile_f32.h')]
        with open(os.path.join(EMU, '.build.lock'), 'w') as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
                subprocess.check_call(['/opt/rocm/lib/llvm/bin/clang++', '-DAAE_EXPERIMENTS', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wall',
                                       '-Wno-unused-function', '-Wno-unknown-pragmas', '-Wno-pass-failed', '-Wno-psabi',
                                       '-o', so + '.tmp', 'encoder_bwd_emu.cpp', 'hip_emu.cpp'], cwd=EMU)
                os.replace(so + '.tmp', so)
        lib = ctypes.CDLL(so)
        lib.aae_conv_backward_workspace_bytes.restype = ctypes.c_size_t
        lib.aae_conv_backward_workspace_bytes.argtypes = [ctypes.POINTER(ConvDesc)]
        lib.aae_conv_backward.restype = ctypes.c_int
        lib.aae_conv_backward.argtypes = [ctypes.POINTER(ConvDesc)] + [_P] * 8 + [ctypes.c_size_t, _P]
        lib.aae_linear_backward_workspace_bytes.restype = ctypes.c_size_t
        lib.aae_linear_backward_workspace_bytes.argtypes = [ctypes.POINTER(DenseDesc), ctypes.c_int]
        lib.aae_linear_backward.restype = ctypes.c_int
        lib.aae_linear_backward.argtypes = [ctypes.POINTER(DenseDesc)] + [_P] * 7 + [ctypes.c_size_t, _P]
        lib.aae_encoder_bwd_label_count.restype = ctypes.c_int
        lib.aae_encoder_bwd_label.restype = ctypes.c_char_p
        lib.aae_encoder_bwd_label.argtypes = [ctypes.c_int]
        lib.aae_last_error.restype = ctypes.c_char_p
        _LIB = lib
    return _LIB


def _aligned(nbytes, fill):
    """a 256-byte aligned uint8 buffer filled with `fill`"""
    raw = np.full(nbytes + 256, fill, np.uint8)
    off = (-raw.ctypes.data) % 256
    return raw[off:off + nbytes]


def _copy(src):
    """a 256-byte aligned copy of src, in its dtype"""
    a = _aligned(src.nbytes, 0).view(src.dtype).reshape(src.shape)
    a[...] = src
    return a


def _nan(shape):
    a = _aligned(4 * int(np.prod(shape)), 0).view(np.float32).reshape(shape)
    a[...] = np.nan
    return a


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _labels(lib):
    return [lib.aae_encoder_bwd_label(i).decode() for i in range(lib.aae_encoder_bwd_label_count())]


def _desc(c, **over):
    f = dict(B=c.B, H=c.H, W=c.W, Cin=c.Cin, Cout=c.Cout, KS=c.KS, S=c.S, x_dtype=0 if c.u8 else 1)
    f.update(over)
    return ConvDesc(*[f[k] for k in ('B', 'H', 'W', 'Cin', 'Cout', 'KS', 'S', 'x_dtype')])


def run_layer(c, inp):
    lib = _lib()
    desc = _desc(c)
    need = lib.aae_conv_backward_workspace_bytes(ctypes.byref(desc))
    assert need > 0, lib.aae_last_error()
    ws = _aligned(need, 0xA5)
    ins = [_copy(inp[k]) for k in ('a_in', 'a_out', 'g_out', 'w')]
    dw, db = _nan((c.KS, c.KS, c.Cin, c.Cout)), _nan((c.Cout,))
    g_in = _nan((c.B, c.H, c.W, c.Cin)) if c.g_in else None
    rc = lib.aae_conv_backward(ctypes.byref(desc), *[_ptr(a) for a in ins], _ptr(dw), _ptr(db), _ptr(g_in), _ptr(ws), need, None)
    assert rc == 0, lib.aae_last_error()
    got = {'delta': ws[:4 * inp['a_out'].size].view(np.float32).reshape(inp['a_out'].shape).copy(), 'db': db, 'dw': dw}
    if c.g_in:
        got['g_in'] = g_in
    return got, _labels(lib)


def run_dense(c, inp):
    lib = _lib()
    desc = DenseDesc(c.B, c.J, c.U)
    need = lib.aae_linear_backward_workspace_bytes(ctypes.byref(desc), int(c.g_a))
    assert need > 0, lib.aae_last_error()
    ws = _aligned(need, 0xA5)
    ins = [_copy(inp[k]) for k in ('a', 'dz', 'w')]
    dw, db = _nan((c.J, c.U)), _nan((c.U,))
    g_a = _nan((c.B, c.J)) if c.g_a else None
    rc = lib.aae_linear_backward(ctypes.byref(desc), *[_ptr(a) for a in ins], _ptr(dw), _ptr(db), _ptr(g_a), _ptr(ws), need, None)
    assert rc == 0, lib.aae_last_error()
    got = {'db': db, 'dw': dw}
    if c.g_a:
        got['g_a'] = g_a
    return got, _labels(lib)


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


@pytest.mark.parametrize('name', list(eg.CASES))
def test_layer_case_on_the_emulator(name):
    c = eg.CASES[name]
    got, labels = run_layer(c, eg.layer_inputs(name))
    worst = eg.check(name, eg.layer_reference(name), got)
    print('%s: largest error in units of u S: %s; %s' % (name, ' '.join('%s %.2f' % kv for kv in sorted(worst.items())), labels))
    eg.check_labels(c, labels)
    again, _ = run_layer(c, eg.layer_inputs(name))
    assert _same_bits(got, again), 'a second call gives other bits'


@pytest.mark.parametrize('name', list(eg.DENSE_CASES))
def test_dense_case_on_the_emulator(name):
    c = eg.DENSE_CASES[name]
    got, labels = run_dense(c, eg.dense_inputs(name))
    worst = eg.check(name, eg.dense_reference(name), got)
    print('%s: largest error in units of u S: %s; %s' % (name, ' '.join('%s %.2f' % kv for kv in sorted(worst.items())), labels))
    eg.check_labels(c, labels)
    again, _ = run_dense(c, eg.dense_inputs(name))
    assert _same_bits(got, again), 'a second call gives other bits'


def test_zero_parity_pixels_are_exact_zeros():
    got, _ = run_layer(eg.CASES['k1_8x8'], eg.layer_inputs('k1_8x8'))
    g = got['g_in']
    assert (g[:, 1::2].view(np.uint32) == 0).all() and (g[:, :, 1::2].view(np.uint32) == 0).all() and np.abs(g[:, ::2, ::2]).max() > 0


def test_refusals_launch_nothing():
    lib = _lib()
    c = eg.CASES['odd_9x9']
    inp = eg.layer_inputs('odd_9x9')
    ins = [_copy(inp[k]) for k in ('a_in', 'a_out', 'g_out', 'w')]
    dw, db = _nan((c.KS, c.KS, c.Cin, c.Cout)), _nan((c.Cout,))
    ws = _aligned(1 << 20, 0xA5)
    for over, code, text in ((dict(S=3), -2, 'stride 3'), (dict(S=4), -2, 'stride 4'), (dict(KS=9), -2, 'kernel size 9'), (dict(KS=0), -1, ''), (dict(S=0), -1, ''),
                             (dict(B=0), -1, ''), (dict(Cout=0), -1, ''), (dict(x_dtype=2), -1, 'x_dtype')):
        desc = _desc(c, **over)
        assert lib.aae_conv_backward_workspace_bytes(ctypes.byref(desc)) == 0
        rc = lib.aae_conv_backward(ctypes.byref(desc), *[_ptr(a) for a in ins], _ptr(dw), _ptr(db), None, _ptr(ws), ws.size, None)
        assert rc == code and text in lib.aae_last_error().decode() and lib.aae_encoder_bwd_label_count() == 0, (over, rc, lib.aae_last_error())
    big = _desc(c, B=1 << 16, H=256, W=256)
    assert lib.aae_conv_backward_workspace_bytes(ctypes.byref(big)) == 0 and '2^31' in lib.aae_last_error().decode()
    desc = _desc(c)
    need = lib.aae_conv_backward_workspace_bytes(ctypes.byref(desc))
    for args, code in (((_ptr(ws), need - 1), -4), ((ctypes.c_void_p(ws.ctypes.data + 16), need), -4), ((None, need), -1)):
        rc = lib.aae_conv_backward(ctypes.byref(desc), *[_ptr(a) for a in ins], _ptr(dw), _ptr(db), None, args[0], args[1], None)
        assert rc == code and lib.aae_encoder_bwd_label_count() == 0, (rc, code)
    rc = lib.aae_conv_backward(ctypes.byref(desc), ctypes.c_void_p(ins[0].ctypes.data + 4), *[_ptr(a) for a in ins[1:]], _ptr(dw), _ptr(db), None, _ptr(ws), need, None)
    assert rc == -1 and '16-byte aligned' in lib.aae_last_error().decode() and lib.aae_encoder_bwd_label_count() == 0
    assert np.isnan(dw).all() and np.isnan(db).all() and (ws == 0xA5).all()
    dd = DenseDesc(0, 8, 8)
    assert lib.aae_linear_backward_workspace_bytes(ctypes.byref(dd), 1) == 0
