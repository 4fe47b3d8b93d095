"""tests/wino_shape_cases.py on the MI355X: the Winograd layer kernel at non-square images, three regions per image, region lists that
leave XCD region groups empty, 3 / 5 / 6 / 12 column blocks in every block order, an odd number of 32-channel stages, ragged
four-image blocks and the BN epilogue -- every AAE_WINO_FORMS row, each layer element by element against the fp64 convolution of its
own input, bit-equal under the (static halo, stage32) settings, the block orders, a permuted batch and a workspace full of NaN.  The
emulator twin (tests/test_emu_winograd_shapes.py) pins the same labels and the host maps on the CPU; what only the hardware shows is
the buffer-view reads outside the image, the LDS-DMA fills, the packed-math asm, the XCD block order and the raised LDS ceilings at
these shapes.  Then one grouped frame: conv_wino_layer_multi_kernel at blocks_x = 2."""
import numpy as np
import pytest

import parity_report
import wino_shape_cases as wsc
from oracle import reference_cpu as ref
from oracle import synth
from test_gpu_parity import _check_indices

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', wsc.cases(), ids=wsc.case_id)
def test_winograd_shape(case):
    ratios = wsc.run_case(case, wsc.GpuBackend())
    parity_report.record('winograd_shapes', case.name, allowance=wsc.ALLOWANCE, **{'%s_%s' % (n, k): r for n, (k, r) in ratios.items()})


def test_grouped_frame_at_two_regions_per_image():
    """three objects of the (64, 128, 3) [32, 64] net with 5, 7 and 6 detections through MultiObjectQuery: conv2 of all three as ONE launch
    of conv_wino_layer_multi_kernel over 36 regions of a 1 x 2 grid; the launch count is the emulator's
    (tests/test_emu_winograd_shapes.py: test_grouped_frame_launch_count)"""
    import torch
    from augmentedautoencoder_amd.engine import CodebookEngine, EncoderEngine, MultiObjectQuery
    from augmentedautoencoder_amd.weights import EncoderConfig
    g = wsc.GROUPED
    cfg = EncoderConfig(*g['config'])
    counts = g['counts']
    host = synth.make_crops(sum(counts), seed=g['crop_seed'], shape=cfg.shape)
    objs, weights, books = [], [], []
    try:
        for seed, rows in zip(g['weight_seeds'], g['codebook_rows']):
            weights.append(synth.make_weights(seed=seed, shape=cfg.shape, num_filter=cfg.num_filter, strides=cfg.strides, latent=cfg.latent_space_size))
            books.append(synth.make_codebook(rows, cfg.latent_space_size, seed=seed + 100, planted_duplicates=5))
            enc = EncoderEngine(cfg, weights[-1], max_batch=64)
            objs.append((enc, CodebookEngine(books[-1])))
            for name, value in wsc.grouped_options().items():
                enc.set_option(name, value)
        mq = MultiObjectQuery([(e, c, n) for (e, c), n in zip(objs, counts)])
        z, idx, _ = [t.cpu().numpy() for t in mq(torch.from_numpy(host).to(torch.device('cuda', 0)))]
        assert mq.launches == g['launches'], mq.launches
    finally:
        for e, c in objs:
            e.close()
            c.close()
    at = 0
    for o, n in enumerate(counts):
        sl = slice(at, at + n)
        z64 = ref.encoder_forward_torch(ref.input_to_float(host[sl]), weights[o], cfg.strides, cfg.batch_norm, 'float64')
        err = float(np.abs(z[sl] - z64).max() / np.abs(z64).max())
        print('grouped frame %s: object %d latent vs fp64 %.3e' % (counts, o, err))
        assert err < wsc.GROUPED_LATENT_TOL, (o, err)
        _check_indices(idx[sl], ref.cos_similarity(z64, books[o]), where='grouped frame at blocks_x = 2, object %d' % o)
        at += n
