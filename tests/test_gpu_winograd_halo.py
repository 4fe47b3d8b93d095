"""The Winograd layer kernel's static zero halo and the four-image mosaic with 32-channel stages (csrc/kernels/conv_winograd_f32.h, encoder options
"winograd_static_halo" and "winograd_stage32") on the MI355X: a layer of each block geometry and the full default encoder at the first batch
whose conv4 takes the Winograd form, BIT-EQUAL with the two options turned off (the halo loaded in every stage, four-image blocks on windows of
their own in 16-channel stages) and within the bounds of tests/test_gpu_winograd.py of the fp64 oracle."""
import numpy as np
import pytest

from oracle import reference_cpu as ref
from oracle import synth

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def _run(cfg, B, seed, wino_layers, force):
    from augmentedautoencoder_amd.engine import EncoderEngine
    weights = synth.make_weights(seed=seed, shape=cfg.shape, num_filter=cfg.num_filter, strides=cfg.strides, latent=cfg.latent_space_size, batch_norm=cfg.batch_norm)
    crops = synth.make_crops(B, seed=seed + 1, shape=cfg.shape)
    enc = EncoderEngine(cfg, weights, max_batch=B)
    if force:                                                                 # (a small net's launches stay below the product rule's block counts)
        enc.set_option('winograd_min_batch', 1)
        enc.set_option('winograd_min_blocks', 1)
    nl = len(cfg.num_filter)
    runs = {}
    for halo, stage32 in ((1, 1), (0, 1), (1, 0), (0, 0)):
        enc.set_option('winograd_static_halo', halo)
        enc.set_option('winograd_stage32', stage32)
        z, recs = enc.encode_timed(crops)
        assert [l.split(':')[0] for l, _, _ in recs if 'conv_wino_f32 layer' in l] == wino_layers, [l for l, _, _ in recs]
        runs[halo, stage32] = [z.cpu().numpy()] + [enc.activation(i).cpu().numpy() for i in range(nl)]
    enc.close()
    for key, got in runs.items():
        for a, b in zip(got, runs[0, 0]):
            assert np.array_equal(a, b), '(static_halo, stage32) = %s differs from both options off' % (key,)
    n = min(B, 24)                                                            # (the fp64 oracle of 24 crops takes seconds; the last ones: the ragged group)
    z64, acts = ref.encoder_forward_torch(ref.input_to_float(crops[-n:]), weights, cfg.strides, cfg.batch_norm, 'float64', return_activations=True)
    for i, a in enumerate(acts):
        assert _rel(runs[1, 1][1 + i][-n:], a) < 2e-5, 'layer %d: %.2e' % (i, _rel(runs[1, 1][1 + i][-n:], a))
    assert _rel(runs[1, 1][0][-n:], z64) < 5e-6, 'latent vs fp64: %.2e' % _rel(runs[1, 1][0][-n:], z64)


def test_four_image_blocks_on_the_mosaic_ragged_group():
    from augmentedautoencoder_amd.weights import EncoderConfig
    # conv2: 64 -> 64 channels at 8 x 8 outputs; B = 5: one whole group of four images and one with a single image
    _run(EncoderConfig((32, 32, 3), [64, 64], [2, 2], 5, 64), 5, 811, ['conv2'], True)


def test_one_region_per_image_static_halo():
    from augmentedautoencoder_amd.weights import EncoderConfig
    # conv2: 64 -> 64 channels at 16 x 16 outputs: one region per image
    _run(EncoderConfig((64, 64, 3), [64, 64], [2, 2], 5, 64), 2, 821, ['conv2'], True)


def test_default_encoder_at_the_first_batch_whose_conv4_takes_the_winograd_form():
    from augmentedautoencoder_amd.weights import EncoderConfig
    _run(EncoderConfig(), 69, 831, ['conv2', 'conv3', 'conv4'], False)
