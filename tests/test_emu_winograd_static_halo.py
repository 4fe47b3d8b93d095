"""The Winograd layer kernel's static zero halo and the four-image mosaic (csrc/kernels/conv_winograd_f32.h: WinoFillPlan<.., STATIC = true>,
WinoGeom<1>) on the CPU fiber emulator, driven directly (tests/emu/wino_layer_halo.cpp: the launch wrappers on synthetic activations, both
block geometries, options "winograd_static_halo" and "winograd_stage32" per call).  The emulator hands LDS over poisoned (0xFF = NaN) between
blocks, and the stage fill of the static form never writes a halo unit: a unit that a patch read touches and wino_zero_halo misses shows as NaN.
  conv3 geometry (32 x 32 inputs, one 16 x 16-pixel region per image): B = 1, 2; 1, 2, 3 stages of 32 channels and the 16-channel fallback (Cin = 48).
  conv4 geometry (16 x 16 inputs, four 8 x 8-output images per block): B = 1, 4, 5, 7 (ragged groups, two blocks of groups), the same widths,
  one and two 64-column blocks.
Every case in block orders 0 and 2: BIT-EQUAL to "winograd_static_halo" = 0 (the fill that loads the halo in every stage; for conv4 the four
windows of their own in 16-channel stages = the kernel before the mosaic) and, for conv4, to "winograd_stage32" = 0 (the mosaic in 16-channel
stages); right against a float64 convolution at the bound of tests/test_emu_winograd_drain.py (5e-6 of the output scale).  The grouped launch
bit-equal to the per-object launches; a layer with 2 x 2 regions per image keeps the loading fill whatever the option says.
What the emulator cannot show: bank conflicts (compile-time checks beside WinoGeom / wino_fill_pixel) and timing (profiles/)."""
import ctypes
import fcntl
import os
import subprocess

import numpy as np
import pytest

from oracle import reference_cpu as ref
from test_emu_winograd_stages32 import _layer_inputs, _pack

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, 'emu')
CSRC = os.path.join(HERE, '..', 'augmentedautoencoder_amd', 'csrc')
_LIB = None
_F = ctypes.POINTER(ctypes.c_float)


def _lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(EMU, 'libwino_layer_halo.so')
        deps = [os.path.join(EMU, f) for f in ('wino_layer_halo.cpp', 'hip_emu.cpp', 'hip_emu.h')]
        deps += [os.path.join(CSRC, 'aae_wino_launch.h'), os.path.join(CSRC, 'kernels', 'conv_winograd_f32.h'), os.path.join(CSRC, 'kernels', 'multi_launch.h')]
        with open(os.path.join(EMU, '.build.lock'), 'w') as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
                # (the compiler and flags of tests/emu/Makefile: the kernel sources use clang's vector types)
                subprocess.check_call(['/opt/rocm/lib/llvm/bin/clang++', '-DAAE_EXPERIMENTS', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wall',
                                       '-Wno-unused-function', '-Wno-unknown-pragmas', '-Wno-pass-failed', '-Wno-psabi',
                                       '-o', so + '.tmp', 'wino_layer_halo.cpp', 'hip_emu.cpp'], cwd=EMU)
                os.replace(so + '.tmp', so)
        _LIB = ctypes.CDLL(so)
    return _LIB


def _run_layer(geom, x, U4, bias, Cout, stage32=1, static_halo=1, xcd_cols=0):
    B, H, _, Cin = x.shape
    out = np.full((B, H // 2, H // 2, Cout), np.nan, np.float32)
    ptrs = (_F * 4)(*[u.ctypes.data_as(_F) for u in U4])
    form = _lib().wino_halo_layer(geom, x.ctypes.data_as(_F), ptrs, bias.ctypes.data_as(_F), out.ctypes.data_as(_F), B, H, Cin, Cout, 1, stage32, static_halo, xcd_cols)
    return out, form


def _run_multi(geom, objs, packed, Cout, stage32=1, static_halo=1):
    n = len(objs)
    counts = [x.shape[0] for x, _, _ in objs]
    H, Cin = objs[0][0].shape[1], objs[0][0].shape[3]
    outs = [np.full((c, H // 2, H // 2, Cout), np.nan, np.float32) for c in counts]
    xs = (_F * n)(*[x.ctypes.data_as(_F) for x, _, _ in objs])
    us = (_F * (4 * n))(*[u.ctypes.data_as(_F) for U4 in packed for u in U4])
    bs = (_F * n)(*[b.ctypes.data_as(_F) for _, _, b in objs])
    os_ = (_F * n)(*[o.ctypes.data_as(_F) for o in outs])
    form = _lib().wino_halo_layer_multi(geom, n, xs, us, bs, os_, (ctypes.c_int * n)(*counts), H, Cin, Cout, 1, stage32, static_halo, 0)
    return outs, form


def _set_order(order):
    _lib().aae_emu_set_block_order(int(order))


def _form(tag, static, channels):
    return 1000 * tag + 100 * static + channels


def _check(geom, B, H, Cin, Cout, runs, seed):
    """runs: {name: (stage32, static_halo, form the launch must report)}; the first one is the default form"""
    x, w, bias = _layer_inputs(B, H, Cin, Cout, seed)
    U4 = _pack(w)
    want = ref.conv2d_same_relu_np(x.astype(np.float64), w.astype(np.float64), bias.astype(np.float64), 2)
    outs = {}
    try:
        for order in (0, 2):
            _set_order(order)
            for name, (stage32, static_halo, form) in list(runs.items())[:1 if order else None]:      # (order 2: the default form)
                out, took = _run_layer(geom, x, U4, bias, Cout, stage32, static_halo)
                assert took == form, '%s: ran as %d, expected %d' % (name, took, form)
                outs[order, name] = out
    finally:
        _set_order(0)
    first = next(iter(runs))
    assert np.isfinite(outs[0, first]).all(), 'a halo unit was read that nobody zeroed'
    err = np.abs(outs[0, first] - want).max() / np.abs(want).max()
    print('geom %d B %d Cin %d Cout %d: rel err %.2e' % (geom, B, Cin, Cout, err))
    assert err < 5e-6, 'rel err %.2e' % err
    for key, out in outs.items():
        assert np.array_equal(out, outs[0, 'halo0']), '(block order, form) = %s differs from winograd_static_halo = 0 in order 0' % (key,)


@pytest.mark.parametrize('B', [1, 2])
@pytest.mark.parametrize('Cin,sc', [(32, 32), (64, 32), (96, 32), (48, 16)])
def test_conv3_geometry_static_halo_same_bits(B, Cin, sc):
    _check(0, B, 32, Cin, 64, {'static': (1, 1, _form(0, 1, sc)), 'halo0': (1, 0, _form(0, 0, sc))}, 400 + 10 * Cin + B)


@pytest.mark.parametrize('Cout', [64, 128])
@pytest.mark.parametrize('B', [1, 4, 5, 7])
@pytest.mark.parametrize('Cin,sc', [(32, 32), (64, 32), (96, 32), (48, 16)])
def test_conv4_geometry_mosaic_same_bits(B, Cin, sc, Cout):
    runs = {'mosaic': (1, 1, _form(1, 1, sc)), 'halo0': (1, 0, _form(2, 0, 16)), 'mosaic16': (0, 1, _form(1, 1, 16))}
    _check(1, B, 16, Cin, Cout, runs, 500 + 10 * Cin + B + Cout)


@pytest.mark.parametrize('geom,H,counts', [(0, 32, [2, 1]), (1, 16, [5, 2])])
@pytest.mark.parametrize('order', [0, 2])
def test_grouped_launch_equals_the_per_object_launches(geom, H, counts, order):
    Cin, Cout = 64, 64
    objs = [_layer_inputs(n, H, Cin, Cout, 600 + 7 * geom + o) for o, n in enumerate(counts)]
    packed = [_pack(w) for _, w, _ in objs]
    _set_order(order)
    try:
        single = [_run_layer(geom, x, U4, bias, Cout)[0] for (x, _, bias), U4 in zip(objs, packed)]
        for stage32, static_halo in ((1, 1), (1, 0), (0, 1)):
            outs, form = _run_multi(geom, objs, packed, Cout, stage32, static_halo)
            assert form == _run_layer(geom, objs[0][0], packed[0], objs[0][2], Cout, stage32, static_halo)[1]
            for a, b in zip(outs, single):
                assert np.array_equal(a, b)
    finally:
        _set_order(0)


def test_layer_with_several_regions_per_image_keeps_the_loading_fill():
    # 64 x 64 inputs: 2 x 2 regions per image (conv2's shape) -- the halo is real data on two sides of every region
    B, H, Cin, Cout = 1, 64, 64, 64
    x, w, bias = _layer_inputs(B, H, Cin, Cout, 701)
    U4 = _pack(w)
    want = ref.conv2d_same_relu_np(x.astype(np.float64), w.astype(np.float64), bias.astype(np.float64), 2)
    on, form_on = _run_layer(0, x, U4, bias, Cout, 1, 1)
    off, form_off = _run_layer(0, x, U4, bias, Cout, 1, 0)
    assert form_on == form_off == _form(0, 0, 32)
    assert np.abs(on - want).max() / np.abs(want).max() < 5e-6
    assert np.array_equal(on, off)
