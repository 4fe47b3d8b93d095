"""The product half of tests/golden/encoder_launch_labels.json on the MI355X: the hardware twin of tests/test_encoder_launch_labels.py.
The emulator cannot see whether a form's dynamic-LDS ceiling was raised -- a form that is launched but missing from the attribute
list of its family passes every CPU test and fails here with an invalid-value launch error.  Per product-build case of
tests/encoder_launch_cases.py: a fresh handle, one timed forward, the label sequence of the fixture (same host code, same options,
the planner's round size pinned) and the result within 2e-5 of the fp64 oracle, of the oracle's maximum (test_gpu_parity.py's bound
for a latent).  Then two grouped frames, so that every kernel the grouped query launches on its own runs after a fresh handle's
creation: [1, 1] (conv1, the wave-split-K layers, the GEMV and the stream scan across the objects) and [6] * 4 (whole-tile conv1,
Winograd layers, the handed-over images, the resident scans and their reduce across the objects)."""
import json
import os

import numpy as np
import pytest

import encoder_launch_cases as elc
import multi_form_cases as mfc
from oracle import decoder_cpu as dref
from oracle import reference_cpu as ref
from oracle import synth
from test_gpu_parity import _check_indices

pytestmark = pytest.mark.gpu

ORACLE_TOL = 2e-5
HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, 'golden', 'encoder_launch_labels.json')) as _f:
    GOLDEN = json.load(_f)
ENCODER = [(c, want) for c, want in zip(GOLDEN['cases'], GOLDEN['product']['encoder']) if 'records' in want]
DECODER = list(zip(GOLDEN['decoder_cases'], GOLDEN['product']['decoder']))


@pytest.mark.parametrize('case,want', ENCODER, ids=[c['name'] for c, _ in ENCODER])
def test_encoder_case_runs_the_recorded_launches_and_matches_fp64(case, want):
    from augmentedautoencoder_amd.engine import EncoderEngine
    cfg, w = elc.encoder_config(case), elc.encoder_weights(case)
    xin, x = elc.encoder_input(case)
    enc = EncoderEngine(cfg, w, max_batch=64)
    try:
        for name, value in case['options']:
            enc.set_option(name, value)
        z, recs = enc.encode_timed(xin)
        z = z.cpu().numpy()
    finally:
        enc.close()
    assert [[label, flops] for label, _, flops in recs] == want['records']
    z64 = ref.encoder_forward_np(ref.input_to_float(x), w, cfg.strides, cfg.batch_norm)
    err = float(np.abs(z - z64).max() / np.abs(z64).max())
    print('%s: latent vs fp64 %.3e' % (case['name'], err))
    assert err < ORACLE_TOL, (case['name'], err)


@pytest.mark.parametrize('case,want', DECODER, ids=[c['name'] for c, _ in DECODER])
def test_decoder_case_runs_the_recorded_launches_and_matches_fp64(case, want):
    from augmentedautoencoder_amd.engine import DecoderEngine
    cfg, w, z = elc.decoder_config(case), elc.decoder_weights(case), elc.decoder_input(case)
    dec = DecoderEngine(cfg, w)
    try:
        out, recs = dec.decode_timed(z)
        out = out.cpu().numpy()
    finally:
        dec.close()
    assert [[label, flops] for label, _, flops in recs] == want['records']
    x64 = dref.decoder_forward_np(z, w, cfg.shape, cfg.num_filters, cfg.strides, cfg.batch_norm)
    err = float(np.abs(out - x64).max() / np.abs(x64).max())
    print('%s: reconstruction vs fp64 %.3e' % (case['name'], err))
    assert err < ORACLE_TOL, (case['name'], err)


# (the net and the options of a case of tests/multi_form_cases.py, detections per object, launches of the grouped part: the count the emulator gives for the same frame)
@pytest.mark.parametrize('case,counts,launches', [('split_items', [1, 1], 6),                     # conv1, conv2 ... conv4, GEMV, scan: one launch each across the objects
                                                  ('mid_batch_group_ragged', [6] * 4, 6)],        # conv1, conv2, conv3's complete blocks, conv3's last two images, scans, reduce
                         ids=['1x2', '6x4'])
def test_grouped_frame_on_fresh_handles(case, counts, launches):
    import torch
    from augmentedautoencoder_amd.engine import CodebookEngine, EncoderEngine, MultiObjectQuery
    cfg = mfc.config(case)
    dev = torch.device('cuda', 0)
    host = synth.make_crops(sum(counts), seed=77, shape=cfg.shape)
    objs, weights, books = [], [], []
    try:
        for k in range(len(counts)):
            weights.append(mfc.weights(cfg, 300 + k))
            books.append(mfc.codebook(cfg, 300 + k, 36 * 8 + k))
            enc = EncoderEngine(cfg, weights[k], max_batch=64)
            objs.append((enc, CodebookEngine(books[k])))
            for name, value in mfc.CASES[case]['options'].items():
                enc.set_option(name, value)
        mq = MultiObjectQuery([(e, c, n) for (e, c), n in zip(objs, counts)])
        z, idx, _ = [t.cpu().numpy() for t in mq(torch.from_numpy(host).to(dev))]
        assert mq.launches == launches
    finally:
        for e, c in objs:
            e.close()
            c.close()
    for o, sl in enumerate(mfc.slices(counts)):
        z64 = ref.encoder_forward_torch(ref.input_to_float(host[sl]), weights[o], cfg.strides, cfg.batch_norm, 'float64')
        err = float(np.abs(z[sl] - z64).max() / np.abs(z64).max())
        print('%s %s: object %d latent vs fp64 %.3e' % (case, counts, o, err))
        assert err < ORACLE_TOL, (case, o, err)
        _check_indices(idx[sl], ref.cos_similarity(z64, books[o]), where='%s, object %d' % (case, o))
