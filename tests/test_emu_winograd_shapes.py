"""tests/wino_shape_cases.py on the CPU fiber emulator: proves without a GPU that every case reaches the Winograd layers its row states
(the labels of launch_winograd), that the host maps -- wino_block_index / wino_block_geometry over non-square region grids, the XCD
block orders of 3, 5, 6 and 12 column blocks, the fill plans, the K loop over an odd number of stages -- agree with fp64 element by
element, and that the bit equalities of the table hold.  Also runs the experiments-only forms the GPU suite skips (one launch per
phase, the 4-wave blocks) on the non-square and the three-stage shapes, and pins the launch count of the grouped frame that
tests/test_gpu_winograd_shapes.py runs on the hardware."""
import numpy as np
import pytest

import emu_backend as eb
import wino_shape_cases as wsc
from augmentedautoencoder_amd.weights import EncoderConfig
from oracle import reference_cpu as ref
from oracle import synth

BY_NAME = {c.name: c for c in wsc.cases()}

# the grouped part of the frame of wsc.GROUPED: conv1 (whole tiles) and conv2 (ONE Winograd launch at blocks_x = 2) across the three
# objects, the three scans as one launch, one reduce launch; the dense layer per object
GROUPED_LAUNCHES = 4


@pytest.mark.parametrize('case', [c for c in wsc.cases() if not c.gpu_only], ids=wsc.case_id)
def test_winograd_shape(case):
    wsc.run_case(case, wsc.EmuBackend())


@pytest.mark.parametrize('case', [c for c in wsc.cases() if c.gpu_only], ids=wsc.case_id)
def test_inputs_of_a_gpu_only_case(case):
    """the cases the emulator does not run: their weights, crops and fp64 expectation are built here all the same -- a dead layer is
    found on the CPU -- and the handle is created with the case's options: its workspace plan is the host's"""
    inp = wsc.build_inputs(case.name)
    enc = wsc.EmuBackend().create(inp.cfg, inp.w, case.B)
    try:
        for k, v in case.options.items():
            enc.set_option(k, v)
        assert enc.L.aae_encoder_workspace_bytes(enc.h, case.B) > 0
    finally:
        enc.close()


# the experiments-only forms (tests/test_emu_winograd.py: option "winograd" = 2, one launch per phase on 32-channel stages, the phases add
# up in the output buffer; "winograd_wide" = 1, blocks of four waves over both 32-channel halves): checks a-c of one run
@pytest.mark.parametrize('name', ['wide_16x32_b1', 'tall_32x16_b1', 'cin96_16x16'])
@pytest.mark.parametrize('form', ['per_phase', 'wide'])
def test_experiments_only_forms(name, form):
    case = BY_NAME[name]
    if form == 'wide':
        wsc.run_case(case, wsc.EmuBackend(), options={'winograd_wide': 1}, bit_checks=False)
        return
    seen = []

    class Recording(wsc.EmuBackend):
        def forward(self, enc, x):
            run = wsc.EmuBackend.forward(self, enc, x)
            seen.append(run.labels)
            return run
    wsc.run_case(case, Recording(), options={'winograd': 2}, bit_checks=False)
    wino = [l for l in seen[0] if 'conv_wino_f32' in l]
    assert [l.split(':')[0] for l in wino] == [n for n in case.wino for _ in range(4)]
    assert [l.split('phase ')[1][:2] for l in wino] == ['11', '10', '01', '00'] * len(case.wino)


def test_grouped_frame_launch_count():
    """three objects of the (64, 128, 3) [32, 64] net with 5, 7 and 6 detections through aae_encode_nn_multi: the launch count the GPU
    twin must see, and the latents of every object against fp64"""
    g = wsc.GROUPED
    cfg = EncoderConfig(*g['config'])
    objs = []
    try:
        for seed, rows in zip(g['weight_seeds'], g['codebook_rows']):
            w = synth.make_weights(seed=seed, shape=cfg.shape, num_filter=cfg.num_filter, strides=cfg.strides, latent=cfg.latent_space_size)
            enc = eb.EmuEncoder(w, cfg)
            for k, v in wsc.grouped_options().items():
                enc.set_option(k, v)
            objs.append((enc, eb.EmuCodebook(synth.make_codebook(rows, cfg.latent_space_size, seed=seed + 100, planted_duplicates=5)), w))
        x = synth.make_crops(sum(g['counts']), seed=g['crop_seed'], shape=cfg.shape)
        z, idx, _, launches = eb.encode_nn_multi([(e, c, n, 1) for (e, c, _), n in zip(objs, g['counts'])], x)
        assert launches == GROUPED_LAUNCHES == g['launches'], launches
        at = 0
        for (e, c, w), n in zip(objs, g['counts']):
            z64 = ref.encoder_forward_np(ref.input_to_float(x[at:at + n]), w, cfg.strides, cfg.batch_norm)
            err = float(np.abs(z[at:at + n] - z64).max() / np.abs(z64).max())
            assert err < wsc.GROUPED_LATENT_TOL, err
            assert np.array_equal(idx[at:at + n], np.argmax(c.similarity(z[at:at + n]), axis=1))
            at += n
    finally:
        for e, c, _ in objs:
            e.close()
            c.close()


def test_the_table_covers_what_it_exists_for():
    wsc.check_coverage(wsc.cases())
    gpu_only = [c.name for c in wsc.cases() if c.gpu_only]
    assert len(gpu_only) <= 5, gpu_only
