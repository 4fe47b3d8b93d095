"""The Winograd layer kernel's 32-channel stages (csrc/kernels/conv_winograd_f32.h: conv_wino_layer_kernel<0, false, 32>, the form of every
layer with 16 x 16-pixel output regions and 32 | Cin) on the CPU fiber emulator, driven directly (tests/emu/wino_layer_direct.cpp: the launch
wrappers on synthetic activations -- the planner gives no layer with Cin % 32 == 16 the Winograd form, and the stage size is chosen per call):
layers of 1, 2 and 3 stages of 32 channels and one of 48 channels, which must run in 16-channel stages; block orders 0 and 2; right against
a float64 convolution at the bound of tests/test_emu_winograd_drain.py (5e-6 of the output scale); BIT-EQUAL to the same layer in 16-channel
stages (option "winograd_stage32" = 0: the stage size changes the schedule, never a sum); the grouped launch bit-equal to the per-object
launches.  Through the encoder as well: option "winograd_stage32" = 0 | 1 gives the same bits for every activation.
What the emulator cannot show: bank conflicts of the stage-buffer layout and the timing of the stage barriers (profiles/)."""
import ctypes
import fcntl
import os
import subprocess

import numpy as np
import pytest

import emu_backend as eb
from augmentedautoencoder_amd.weights import EncoderConfig
from oracle import reference_cpu as ref
from oracle import synth

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, 'emu')
CSRC = os.path.join(HERE, '..', 'augmentedautoencoder_amd', 'csrc')
_DIRECT = None
_F = ctypes.POINTER(ctypes.c_float)


def _direct():
    global _DIRECT
    if _DIRECT is None:
        so = os.path.join(EMU, 'libwino_layer_direct.so')
        deps = [os.path.join(EMU, f) for f in ('wino_layer_direct.cpp', 'hip_emu.cpp', 'hip_emu.h')]
        deps += [os.path.join(CSRC, 'aae_wino_launch.h'), os.path.join(CSRC, 'kernels', 'conv_winograd_f32.h'), os.path.join(CSRC, 'kernels', 'multi_launch.h')]
        with open(os.path.join(EMU, '.build.lock'), 'w') as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
                # (the compiler and flags of tests/emu/Makefile: the kernel sources use clang's vector types)
                subprocess.check_call(['/opt/rocm/lib/llvm/bin/clang++', '-DAAE_EXPERIMENTS', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wall',
                                       '-Wno-unused-function', '-Wno-unknown-pragmas', '-Wno-pass-failed', '-Wno-psabi',
                                       '-o', so + '.tmp', 'wino_layer_direct.cpp', 'hip_emu.cpp'], cwd=EMU)
                os.replace(so + '.tmp', so)
        _DIRECT = ctypes.CDLL(so)
    return _DIRECT


def _pack_component(w, eh, ew, swap):
    """Winograd-domain weights of one polyphase component in the kernel's fragment order (the layout of conv_winograd_f32.h's header comment:
    [32-column block][8-channel group][point a PB + b][K half][32 columns][4 channels]; U = G g G^T in float64, rounded once)."""
    G = {3: np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64), 2: np.array([[1, 0], [1, 1], [0, 1]], np.float64)}
    g = w[(0 if eh else 1)::2, (0 if ew else 1)::2].astype(np.float64)           # taps [rows][columns][Cin][Cout]
    if swap:
        g = g.transpose(1, 0, 2, 3)                                              # [along A][along B]
    tA, tB = g.shape[:2]
    U = np.einsum('ak,klcn,bl->abcn', G[tA], g, G[tB])                           # [PA][PB][Cin][Cout]
    PA, PB, Cin, Cout = U.shape
    U = U.reshape(PA * PB, Cin // 8, 2, 4, Cout // 32, 32)                       # [point][group][K half][channel][column block][column]
    return np.ascontiguousarray(U.transpose(4, 1, 0, 2, 5, 3).astype(np.float32)).ravel()


def _pack(w):
    return [_pack_component(w, eh, ew, swap=(eh == 0 and ew == 1)) for eh in (0, 1) for ew in (0, 1)]      # index 2 eh + ew


def _layer_inputs(B, H, Cin, Cout, seed):
    rng = np.random.RandomState(seed)
    x = rng.rand(B, H, H, Cin).astype(np.float32)
    x[rng.rand(*x.shape) < 0.45] = 0.0                                           # (post-ReLU activations)
    w = (rng.randn(5, 5, Cin, Cout) * (2.0 / (25 * Cin)) ** 0.5).astype(np.float32)
    bias = (rng.randn(Cout) * 0.1).astype(np.float32)
    return x, w, bias


def _run_layer(x, U4, bias, Cout, stage32, xcd_cols=0):
    B, H, _, Cin = x.shape
    out = np.full((B, H // 2, H // 2, Cout), np.nan, np.float32)
    ptrs = (_F * 4)(*[u.ctypes.data_as(_F) for u in U4])
    form = _direct().wino_direct_layer(x.ctypes.data_as(_F), ptrs, bias.ctypes.data_as(_F), out.ctypes.data_as(_F), B, H, Cin, Cout, 1, stage32, xcd_cols)
    return out, form


def _set_order(order):
    _direct().aae_emu_set_block_order(int(order))


# (Cin, stages of the form the layer takes): 1, 2 and 3 stages of 32 channels; 48 channels = three 16-channel stages
@pytest.mark.parametrize('Cin,form', [(32, 32), (64, 32), (96, 32), (48, 16)])
def test_stage_forms_same_bits_in_every_block_order_and_right_against_float64(Cin, form):
    B, H, Cout = 2, 32, 64
    x, w, bias = _layer_inputs(B, H, Cin, Cout, 100 + Cin)
    U4 = _pack(w)
    want = ref.conv2d_same_relu_np(x.astype(np.float64), w.astype(np.float64), bias.astype(np.float64), 2)
    outs = {}
    try:
        for order in (0, 2):
            _set_order(order)
            for stage32 in (1, 0):
                out, took = _run_layer(x, U4, bias, Cout, stage32)
                assert took == (form if stage32 else 16)
                outs[order, stage32] = out
    finally:
        _set_order(0)
    err = np.abs(outs[0, 1] - want).max() / np.abs(want).max()
    print('Cin %d: %d-channel stages, rel err %.2e' % (Cin, form, err))
    assert err < 5e-6, 'Cin %d rel err %.2e' % (Cin, err)
    for key, out in outs.items():
        assert np.array_equal(out, outs[0, 0]), 'Cin %d: (block order, stage32) = %s differs from 16-channel stages in order 0' % (Cin, key)


def test_several_regions_and_column_blocks_xcd_map():
    # 64 x 64 inputs: 2 x 2 regions per image; 128 output channels: two 64-column blocks, dealt out over the XCDs
    B, H, Cin, Cout = 1, 64, 64, 128
    x, w, bias = _layer_inputs(B, H, Cin, Cout, 211)
    U4 = _pack(w)
    want = ref.conv2d_same_relu_np(x.astype(np.float64), w.astype(np.float64), bias.astype(np.float64), 2)
    out32, took = _run_layer(x, U4, bias, Cout, 1, xcd_cols=2)
    out16, _ = _run_layer(x, U4, bias, Cout, 0, xcd_cols=0)
    assert took == 32
    assert np.abs(out32 - want).max() / np.abs(want).max() < 5e-6
    assert np.array_equal(out32, out16)


@pytest.mark.parametrize('order', [0, 2])
def test_grouped_launch_equals_the_per_object_launches(order):
    H, Cin, Cout, counts = 32, 64, 64, [2, 1, 3]
    objs = [_layer_inputs(n, H, Cin, Cout, 300 + o) for o, n in enumerate(counts)]
    packed = [_pack(w) for _, w, _ in objs]
    _set_order(order)
    try:
        single = [_run_layer(x, U4, bias, Cout, 1)[0] for (x, _, bias), U4 in zip(objs, packed)]
        for stage32 in (1, 0):
            outs = [np.full((n, H // 2, H // 2, Cout), np.nan, np.float32) for n in counts]
            n = len(objs)
            xs = (_F * n)(*[x.ctypes.data_as(_F) for x, _, _ in objs])
            us = (_F * (4 * n))(*[u.ctypes.data_as(_F) for U4 in packed for u in U4])
            bs = (_F * n)(*[b.ctypes.data_as(_F) for _, _, b in objs])
            os_ = (_F * n)(*[o.ctypes.data_as(_F) for o in outs])
            took = _direct().wino_direct_layer_multi(n, xs, us, bs, os_, (ctypes.c_int * n)(*counts), H, Cin, Cout, 1, stage32, 0)
            assert took == (32 if stage32 else 16)
            for a, b in zip(outs, single):
                assert np.array_equal(a, b)
    finally:
        _set_order(0)


def test_encoder_option_stage32_changes_no_bit():
    # conv2: 32 -> 64 channels at 16 x 16 outputs (one 32-channel stage | two 16-channel ones), conv3: 8 x 8 outputs (four images per block: 16-channel stages either way)
    cfg = EncoderConfig((64, 64, 3), [32, 64, 64], [2, 2, 2], 5, 128, True)
    w = synth.make_weights(seed=71, shape=cfg.shape, num_filter=cfg.num_filter, strides=cfg.strides, latent=cfg.latent_space_size, batch_norm=cfg.batch_norm,
                           kernel_size=cfg.kernel_size)
    x = synth.make_crops(5, seed=72, shape=cfg.shape)
    runs = []
    for stage32 in (1, 0):
        enc = eb.EmuEncoder(w, cfg)
        for k, v in {'winograd_min_batch': 1, 'winograd_min_blocks': 1, 'winograd': 1, 'winograd_stage32': stage32}.items():
            enc.set_option(k, v)
        z = enc.forward(x)
        assert sum('conv_wino_f32' in l for l in enc.labels()) == 2
        runs.append([z] + [enc.activation(i).copy() for i in range(3)])
        enc.close()
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    _, acts64 = ref.encoder_forward_np(ref.input_to_float(x), w, cfg.strides, cfg.batch_norm, return_activations=True)
    for i in (1, 2):
        assert np.abs(runs[0][1 + i] - acts64[i]).max() / np.abs(acts64[i]).max() < 5e-6
