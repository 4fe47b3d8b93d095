"""The Winograd layer kernel's phase boundary (csrc/kernels/conv_winograd_f32.h: wino_phase_body's output transform, compiled once per point-row
half and chosen by a wave-uniform branch; the exchange's second barrier left to the next phase's stage barrier when that phase has one) on the
CPU fiber emulator: both block geometries with several stages per phase, the same bits in every block order, right against the fp64 oracle,
the grouped multi-object launch (conv_wino_layer_multi_kernel) bit for bit the per-object launches -- and all of it bit for bit what the
kernel before this form computed (tests/golden/wino_drain_parent.npz: that kernel's emulator run of the same inputs).
What the emulator cannot show: it compiles the plain C++ of the drain's asm adds, not the asm, and no MFMA timing (the wait states in front of
the drain are checked in the ISA), and a fiber runs to its next barrier, so a missing barrier need not show here."""
import os

import numpy as np
import pytest

import emu_backend as eb
from augmentedautoencoder_amd.weights import EncoderConfig
from oracle import reference_cpu as ref
from oracle import synth

_WINO = {'winograd_min_batch': 1, 'winograd_min_blocks': 1, 'winograd': 1}
# conv2 (32 -> 64 channels, 16 x 16 outputs: GEOM 0, two 16-channel stages) and conv3 (64 -> 64, 8 x 8 outputs: GEOM 1, four stages) with BN
_CFG = EncoderConfig((64, 64, 3), [32, 64, 64], [2, 2, 2], 5, 128, True)


_GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wino_drain_parent.npz'))


def _weights(seed):
    return synth.make_weights(seed=seed, shape=_CFG.shape, num_filter=_CFG.num_filter, strides=_CFG.strides, latent=_CFG.latent_space_size,
                              batch_norm=_CFG.batch_norm, kernel_size=_CFG.kernel_size)


def _activations(w, x, opts=None):
    enc = eb.EmuEncoder(w, _CFG)
    for k, v in dict(_WINO, **(opts or {})).items():
        enc.set_option(k, v)
    z = enc.forward(x)
    labels = enc.labels()
    acts = [enc.activation(i).copy() for i in range(3)]
    enc.close()
    assert [l.startswith('conv%d' % (i + 2)) for i, l in enumerate(l for l in labels if 'conv_wino_f32' in l)] == [True, True]
    return z, acts


def test_both_geometries_same_bits_in_every_block_order_and_right_against_the_oracle():
    w = _weights(71)
    x = synth.make_crops(5, seed=72, shape=_CFG.shape)        # (GEOM 1: two blocks of four images, the second ragged)
    _, acts64 = ref.encoder_forward_np(ref.input_to_float(x), w, _CFG.strides, _CFG.batch_norm, return_activations=True)
    runs = []
    try:
        for order in (0, 2):
            eb.set_block_order(order)
            runs.append(_activations(w, x))
    finally:
        eb.set_block_order(0)
    (z0, a0), (z1, a1) = runs
    assert np.array_equal(z0, z1) and all(np.array_equal(p, q) for p, q in zip(a0, a1))
    for i in (1, 2):
        err = np.abs(a0[i] - acts64[i]).max() / np.abs(acts64[i]).max()
        assert err < 5e-6, 'layer %d rel err %.2e' % (i, err)
    assert np.array_equal(a0[1], _GOLDEN['act1']) and np.array_equal(a0[2], _GOLDEN['act2']) and np.array_equal(z0, _GOLDEN['z'])


@pytest.mark.parametrize('order', [0, 2])
def test_grouped_launch_equals_the_per_object_launches(order):
    counts = [5, 6]
    eb.set_block_order(order)
    objs = []
    try:
        for o in range(2):
            w = _weights(80 + o)
            enc = eb.EmuEncoder(w, _CFG)
            for k, v in dict(_WINO, first_group_split_max_tiles=0).items():
                enc.set_option(k, v)
            cb = eb.EmuCodebook(synth.make_codebook(36 * 9 + o, _CFG.latent_space_size, seed=90 + o, planted_duplicates=5))
            objs.append((enc, cb, w))
        items = [(e, c, n, 1) for (e, c, _), n in zip(objs, counts)]
        x = synth.make_crops(sum(counts), seed=85, shape=_CFG.shape)
        zs, at = [], 0
        for (e, c, _), n in zip(objs, counts):
            zs.append(eb.encode_nn(e, c, x[at:at + n], 1)[0])
            at += n
        z1, _, _, launches = eb.encode_nn_multi(items, x)
        assert launches == 5          # (grouped: conv1, the Winograd conv2 and conv3 across the objects, the scans + one reduce)
        assert np.array_equal(z1, np.concatenate(zs)) and np.array_equal(z1, _GOLDEN['z_group'])
        at = 0
        for (_, _, w), n in zip(objs, counts):
            z64 = ref.encoder_forward_np(ref.input_to_float(x[at:at + n]), w, _CFG.strides, _CFG.batch_norm)
            assert np.abs(z1[at:at + n] - z64).max() / np.abs(z64).max() < 5e-6
            at += n
    finally:
        eb.set_block_order(0)
        for enc, cb, _ in objs:
            enc.close()
            cb.close()
