"""The decoder's backward kernels (csrc/kernels/decoder_bwd_f32.h) and their host code (csrc/aae_decoder_bwd_impl.h) on the CPU fiber
emulator: tests/emu/decoder_bwd_emu.cpp, built here with the compiler and flags of tests/emu/Makefile, exports the library's own
entry points on host pointers.  The case table of tests/decoder_grad_reference.py runs through aae_upconv_backward /
aae_dense_backward with the outputs handed in full of NaN and the workspace full of 0xA5; every element of delta, db, dw, g_in / dz is
held to (n + 8) u S against the direct float64 formulas, the labels to the planner's restatement, a second call to the same bits.
What the emulator proves: the MFMA fragment maps, the k-major and row-major slab layouts, the phase gathers, the masks of ragged
tiles, the K splits and the unfold.  What it cannot: timing, bank conflicts, the order of the hardware's fp32 sums (the GPU test)."""
import ctypes
import fcntl
import os
import subprocess

import numpy as np
import pytest

import decoder_grad_reference as dg

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, 'emu')
CSRC = os.path.join(HERE, '..', 'augmentedautoencoder_amd', 'csrc')
_LIB = None
_P = ctypes.c_void_p


class UpconvDesc(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ('B', 'H', 'W', 'Cin', 'UH', 'UW', 'Cout', 'KS', 'act')]


class DenseDesc(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ('B', 'J', 'U')]


def _lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(EMU, 'libdecoder_bwd_emu.so')
        deps = [os.path.join(EMU, f) for f in ('decoder_bwd_emu.cpp', 'hip_emu.cpp', 'hip_emu.h')]
        deps += [os.path.join(CSRC, 'aae_decoder_bwd_impl.h')] + [os.path.join(CSRC, 'kernels', f) for f in ('decoder_bwd_core.h', 'decoder_bwd_f32.h', 'tile_f32.h')]
        with open(os.path.join(EMU, '.build.lock'), 'w') as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
                subprocess.check_call(['/opt/rocm/lib/llvm/bin/clang++', '-DAAE_EXPERIMENTS', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wall',
                                       '-Wno-unused-function', '-Wno-unknown-pragmas', '-Wno-pass-failed', '-Wno-psabi',
                                       '-o', so + '.tmp', 'decoder_bwd_emu.cpp', 'hip_emu.cpp'], cwd=EMU)
                os.replace(so + '.tmp', so)
        lib = ctypes.CDLL(so)
        lib.aae_upconv_backward_workspace_bytes.restype = ctypes.c_size_t
        lib.aae_upconv_backward_workspace_bytes.argtypes = [ctypes.POINTER(UpconvDesc), ctypes.c_int]
        lib.aae_upconv_backward.restype = ctypes.c_int
        lib.aae_upconv_backward.argtypes = [ctypes.POINTER(UpconvDesc)] + [_P] * 8 + [ctypes.c_size_t, _P]
        lib.aae_dense_backward_workspace_bytes.restype = ctypes.c_size_t
        lib.aae_dense_backward_workspace_bytes.argtypes = [ctypes.POINTER(DenseDesc), ctypes.c_int]
        lib.aae_dense_backward.restype = ctypes.c_int
        lib.aae_dense_backward.argtypes = [ctypes.POINTER(DenseDesc)] + [_P] * 8 + [ctypes.c_size_t, _P]
        lib.aae_decoder_bwd_label_count.restype = ctypes.c_int
        lib.aae_decoder_bwd_label.restype = ctypes.c_char_p
        lib.aae_decoder_bwd_label.argtypes = [ctypes.c_int]
        lib.aae_last_error.restype = ctypes.c_char_p
        _LIB = lib
    return _LIB


def _aligned(nbytes, fill):
    """a 256-byte aligned uint8 buffer filled with `fill`"""
    raw = np.full(nbytes + 256, fill, np.uint8)
    off = (-raw.ctypes.data) % 256
    return raw[off:off + nbytes]


def _f32(shape, src=None):
    """a 256-byte aligned float32 array: a copy of src, or full of NaN"""
    n = int(np.prod(shape))
    a = _aligned(4 * n, 0).view(np.float32).reshape(shape)
    a[...] = np.nan if src is None else src
    return a


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _labels(lib):
    return [lib.aae_decoder_bwd_label(i).decode() for i in range(lib.aae_decoder_bwd_label_count())]


def run_stage(c, inp):
    lib = _lib()
    desc = UpconvDesc(c.B, c.H, c.W, c.Cin, c.UH, c.UW, c.Cout, c.KS, c.act)
    need = lib.aae_upconv_backward_workspace_bytes(ctypes.byref(desc), int(c.g_in))
    assert need > 0, lib.aae_last_error()
    ws = _aligned(need, 0xA5)
    ins = [_f32(inp[k].shape, inp[k]) for k in ('a_in', 'a_out', 'g_out', 'w')]
    dw, db = _f32((c.KS, c.KS, c.Cin, c.Cout)), _f32((c.Cout,))
    g_in = _f32((c.B, c.H, c.W, c.Cin)) if c.g_in else None
    rc = lib.aae_upconv_backward(ctypes.byref(desc), *[_ptr(a) for a in ins], _ptr(dw), _ptr(db), _ptr(g_in), _ptr(ws), need, None)
    assert rc == 0, lib.aae_last_error()
    got = {'delta': ws[:4 * c.B * c.UH * c.UW * c.Cout].view(np.float32).reshape(c.B, c.UH, c.UW, c.Cout).copy(), 'db': db, 'dw': dw}
    if c.g_in:
        got['g_in'] = g_in
    return got, _labels(lib)


def run_dense(c, inp):
    lib = _lib()
    desc = DenseDesc(c.B, c.J, c.U)
    need = lib.aae_dense_backward_workspace_bytes(ctypes.byref(desc), int(c.dz))
    assert need > 0, lib.aae_last_error()
    ws = _aligned(need, 0xA5)
    ins = [_f32(inp[k].shape, inp[k]) for k in ('z', 'a_out', 'g_out', 'w')]
    dw, db = _f32((c.J, c.U)), _f32((c.U,))
    dz = _f32((c.B, c.J)) if c.dz else None
    rc = lib.aae_dense_backward(ctypes.byref(desc), *[_ptr(a) for a in ins], _ptr(dw), _ptr(db), _ptr(dz), _ptr(ws), need, None)
    assert rc == 0, lib.aae_last_error()
    got = {'delta': ws[:4 * c.B * c.U].view(np.float32).reshape(c.B, c.U).copy(), 'db': db, 'dw': dw}
    if c.dz:
        got['dz'] = dz
    return got, _labels(lib)


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


@pytest.mark.parametrize('name', list(dg.CASES))
def test_stage_case_on_the_emulator(name):
    c = dg.CASES[name]
    got, labels = run_stage(c, dg.stage_inputs(name))
    worst = dg.check(name, dg.stage_reference(name), got)
    print('%s: largest error in units of u S: %s; %s' % (name, ' '.join('%s %.2f' % kv for kv in sorted(worst.items())), labels))
    dg.check_labels(c, labels)
    again, _ = run_stage(c, dg.stage_inputs(name))
    assert _same_bits(got, again), 'a second call gives other bits'


@pytest.mark.parametrize('name', list(dg.DENSE_CASES))
def test_dense_case_on_the_emulator(name):
    c = dg.DENSE_CASES[name]
    got, labels = run_dense(c, dg.dense_inputs(name))
    worst = dg.check(name, dg.dense_reference(name), got)
    print('%s: largest error in units of u S: %s; %s' % (name, ' '.join('%s %.2f' % kv for kv in sorted(worst.items())), labels))
    dg.check_labels(c, labels)
    again, _ = run_dense(c, dg.dense_inputs(name))
    assert _same_bits(got, again), 'a second call gives other bits'


def test_refusals_launch_nothing():
    lib = _lib()
    c = dg.CASES['ragged_3x5']
    inp = dg.stage_inputs('ragged_3x5')
    ins = [_f32(inp[k].shape, inp[k]) for k in ('a_in', 'a_out', 'g_out', 'w')]
    dw, db = _f32((c.KS, c.KS, c.Cin, c.Cout)), _f32((c.Cout,))
    ws = _aligned(1 << 20, 0xA5)
    for UH, UW, code, text in ((7, 10, -2, 'only exact 2x and 1x'), (9, 15, -2, 'only exact 2x and 1x'), (6, 5, -2, 'only exact 2x and 1x')):
        desc = UpconvDesc(c.B, c.H, c.W, c.Cin, UH, UW, c.Cout, c.KS, c.act)
        assert lib.aae_upconv_backward_workspace_bytes(ctypes.byref(desc), 1) == 0
        rc = lib.aae_upconv_backward(ctypes.byref(desc), *[_ptr(a) for a in ins], _ptr(dw), _ptr(db), None, _ptr(ws), ws.size, None)
        assert rc == code and text in lib.aae_last_error().decode() and lib.aae_decoder_bwd_label_count() == 0
    desc = UpconvDesc(c.B, c.H, c.W, c.Cin, c.UH, c.UW, c.Cout, c.KS, c.act)
    need = lib.aae_upconv_backward_workspace_bytes(ctypes.byref(desc), 0)
    for args, code in (((_ptr(ws), need - 1), -4), ((ctypes.c_void_p(ws.ctypes.data + 16), need), -4), ((None, need), -1)):
        rc = lib.aae_upconv_backward(ctypes.byref(desc), *[_ptr(a) for a in ins], _ptr(dw), _ptr(db), None, args[0], args[1], None)
        assert rc == code and lib.aae_decoder_bwd_label_count() == 0, (rc, code)
    for bad in (dict(KS=4), dict(act=2), dict(B=0), dict(Cout=0)):
        f = dict(B=c.B, H=c.H, W=c.W, Cin=c.Cin, UH=c.UH, UW=c.UW, Cout=c.Cout, KS=c.KS, act=c.act)
        f.update(bad)
        desc = UpconvDesc(*[f[k] for k in ('B', 'H', 'W', 'Cin', 'UH', 'UW', 'Cout', 'KS', 'act')])
        rc = lib.aae_upconv_backward(ctypes.byref(desc), *[_ptr(a) for a in ins], _ptr(dw), _ptr(db), None, _ptr(ws), ws.size, None)
        assert rc == -1 and lib.aae_decoder_bwd_label_count() == 0, bad
    assert np.isnan(dw).all() and np.isnan(db).all() and (ws == 0xA5).all()
    dd = DenseDesc(0, 8, 8)
    assert lib.aae_dense_backward_workspace_bytes(ctypes.byref(dd), 1) == 0
