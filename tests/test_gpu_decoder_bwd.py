"""The decoder's backward pass on the MI355X: the case table of tests/decoder_grad_reference.py through aae_upconv_backward /
aae_dense_backward (decoder_grad.py), outputs handed in full of NaN and the workspace full of 0xA5; then the whole chain
decode -> reconstruction_loss(grad=True) -> backward on two decoders of tests/decoder_form_cases.py, and AE.gradients_device.

Per element, every tensor, no element left out:  |got - ref64| <= (n + 8) u S,  u = 2^-24  (derived in decoder_grad_reference.py,
not measured).  A second call gives the same bits; the labels are the planner's restatement; the refusals launch nothing.
Measured maxima as multiples of u S (the bound n + 8 is between 9 and about 1200 at these shapes): MEASURED_STAGE_MAXIMA below.

Whole chain: the reference back-propagates in float64 through the DEVICE's saved activations, x and dx.  Per-stage errors compound,
so the tolerance is measured: the same NumPy restatement in float32 against float64 on these cases, and the GPU is allowed 4x that
error per tensor, relative to the tensor's largest S (the same precision, another order).  MEASURED_CHAIN below."""
import ctypes

import numpy as np
import pytest

import decoder_grad_reference as dg

pytestmark = pytest.mark.gpu

# largest |got - ref64| / (u S) over the table, per tensor (MI355X); the bound is (n + 8)
MEASURED_STAGE_MAXIMA = 'delta 2.15 (sigmoid_last), db 1.54, dw 4.43 (dense_J33_U240_B67; stages 2.72), g_in 3.87 (plain_7x9), dz 1.48'
# whole chain, per case: largest float32-NumPy error and largest GPU error over the tensors, both relative to the tensor's largest S
MEASURED_CHAIN = 'dense_generic: float32 NumPy 1.05e-7, GPU 3.20e-7; last_wide: 2.58e-7 and 4.94e-7 (per tensor the GPU used at most 3.85 of its allowance of 4: dense_1/bias of last_wide)'


def _nan(shape):
    import torch
    return torch.full(tuple(shape), float('nan'), dtype=torch.float32, device='cuda')


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _dirty(nbytes):
    import torch
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device='cuda')


def _run_stage(c, inp):
    from augmentedautoencoder_amd import _lib, decoder_grad as G
    lib = _lib.load()
    desc = _lib.UpconvBackwardDesc(c.B, c.H, c.W, c.Cin, c.UH, c.UW, c.Cout, c.KS, c.act)
    ws = _dirty(int(lib.aae_upconv_backward_workspace_bytes(ctypes.byref(desc), int(c.g_in))))
    out = (_nan((c.KS, c.KS, c.Cin, c.Cout)), _nan((c.Cout,)), _nan((c.B, c.H, c.W, c.Cin)) if c.g_in else None)
    dw, db, g_in = G.upconv_backward(_dev(inp['a_in']), _dev(inp['a_out']), _dev(inp['g_out']), _dev(inp['w']), activation='sigmoid' if c.act == dg.SIGMOID else 'relu',
                                     out=out, workspace=ws)
    assert dw is out[0] and db is out[1] and g_in is out[2]
    n = c.B * c.UH * c.UW * c.Cout
    got = {'delta': ws[:4 * n].view(__import__('torch').float32).reshape(c.B, c.UH, c.UW, c.Cout).cpu().numpy(), 'db': db.cpu().numpy(), 'dw': dw.cpu().numpy()}
    if c.g_in:
        got['g_in'] = g_in.cpu().numpy()
    return got, G.labels()


def _run_dense(c, inp):
    from augmentedautoencoder_amd import _lib, decoder_grad as G
    lib = _lib.load()
    desc = _lib.DenseBackwardDesc(c.B, c.J, c.U)
    ws = _dirty(int(lib.aae_dense_backward_workspace_bytes(ctypes.byref(desc), int(c.dz))))
    out = (_nan((c.J, c.U)), _nan((c.U,)), _nan((c.B, c.J)) if c.dz else None)
    dw, db, dz = G.dense_backward(_dev(inp['z']), _dev(inp['a_out']), _dev(inp['g_out']), _dev(inp['w']), out=out, workspace=ws)
    got = {'delta': ws[:4 * c.B * c.U].view(__import__('torch').float32).reshape(c.B, c.U).cpu().numpy(), 'db': db.cpu().numpy(), 'dw': dw.cpu().numpy()}
    if c.dz:
        got['dz'] = dz.cpu().numpy()
    return got, G.labels()


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


@pytest.mark.parametrize('name', list(dg.CASES))
def test_stage_case(name):
    c = dg.CASES[name]
    got, labels = _run_stage(c, dg.stage_inputs(name))
    ref = dg.stage_reference(name)
    print('%s: labels %s' % (name, labels))
    worst = None
    try:
        worst = dg.check(name, ref, got)
    finally:
        print('%s: largest error in units of u S: %s' % (name, worst and ' '.join('%s %.2f' % kv for kv in sorted(worst.items()))))
    dg.check_labels(c, labels)
    again, _ = _run_stage(c, dg.stage_inputs(name))
    assert _same_bits(got, again), 'a second call gives other bits'


@pytest.mark.parametrize('name', list(dg.DENSE_CASES))
def test_dense_case(name):
    c = dg.DENSE_CASES[name]
    got, labels = _run_dense(c, dg.dense_inputs(name))
    print('%s: labels %s' % (name, labels))
    worst = None
    try:
        worst = dg.check(name, dg.dense_reference(name), got)
    finally:
        print('%s: largest error in units of u S: %s' % (name, worst and ' '.join('%s %.2f' % kv for kv in sorted(worst.items()))))
    dg.check_labels(c, labels)
    again, _ = _run_dense(c, dg.dense_inputs(name))
    assert _same_bits(got, again), 'a second call gives other bits'


def test_refusals_launch_nothing():
    import torch
    from augmentedautoencoder_amd import _lib, decoder_grad as G
    lib = _lib.load()
    c, inp = dg.CASES['ragged_3x5'], dg.stage_inputs('ragged_3x5')
    a_in, g_out, w = _dev(inp['a_in']), _dev(inp['g_out']), _dev(inp['w'])
    dw, db, ws = _nan(w.shape), _nan((c.Cout,)), _dirty(1 << 20)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    G.upconv_backward(a_in, _dev(inp['a_out']), g_out, w)                       # (so that the label list is not empty to begin with)
    assert G.labels()
    for UH, UW in ((7, 10), (9, 15), (6, 5)):
        desc = _lib.UpconvBackwardDesc(c.B, c.H, c.W, c.Cin, UH, UW, c.Cout, c.KS, c.act)
        a_out = torch.zeros((c.B, UH, UW, c.Cout), device='cuda')
        assert lib.aae_upconv_backward_workspace_bytes(ctypes.byref(desc), 1) == 0
        rc = lib.aae_upconv_backward(ctypes.byref(desc), p(a_in), p(a_out), p(a_out), p(w), p(dw), p(db), None, p(ws), ws.numel(), stream)
        assert rc == -2 and b'only exact 2x and 1x' in lib.aae_last_error() and G.labels() == []
        with pytest.raises(NotImplementedError, match='only exact 2x and 1x'):
            G.upconv_backward(a_in, a_out, a_out, w, out=(dw, db, None), workspace=ws)
    desc = _lib.UpconvBackwardDesc(c.B, c.H, c.W, c.Cin, c.UH, c.UW, c.Cout, c.KS, c.act)
    need = lib.aae_upconv_backward_workspace_bytes(ctypes.byref(desc), 0)
    a_out = _dev(inp['a_out'])
    rc = lib.aae_upconv_backward(ctypes.byref(desc), p(a_in), p(a_out), p(g_out), p(w), p(dw), p(db), None, p(ws), need - 1, stream)
    assert rc == -4 and G.labels() == []
    rc = lib.aae_upconv_backward(ctypes.byref(desc), p(a_in), p(a_out), p(g_out), p(w), p(dw), p(db), None, ctypes.c_void_p(ws.data_ptr() + 16), need, stream)
    assert rc == -4 and G.labels() == []
    with pytest.raises(ValueError, match='shape'):
        G.upconv_backward(a_in, a_out, g_out, w, out=(dw, _nan((c.Cout + 1,)), None))
    with pytest.raises(ValueError, match='contiguous'):
        G.upconv_backward(a_in.transpose(1, 2), a_out, g_out, w)
    torch.cuda.synchronize()
    assert torch.isnan(dw).all() and torch.isnan(db).all() and (ws == 0xA5).all()


# ---- the whole chain ----------------------------------------------------------------------------------------------------------------
CHAIN_NETS = ('dense_generic', 'last_wide')          # the smallest decoder of the table without batch norm (two stages, 3 channels out), and one with 5


def _chain(name, ratio=4):
    import torch
    import decoder_form_cases as dc
    from augmentedautoencoder_amd.engine import DecoderEngine
    from augmentedautoencoder_amd.loss import reconstruction_loss
    case = {c.name: c for c in dc.cases()}[name]
    inp = dc.build_inputs(name)
    eng = DecoderEngine(inp.cfg, inp.w)
    try:
        z = _dev(inp.z)
        x = eng.decode(z)
        target = torch.from_numpy(np.random.RandomState(11).rand(*x.shape).astype(np.float32)).cuda()
        _, _, dx = reconstruction_loss(x, target, loss='L2', bootstrap_ratio=ratio, grad=True)
        grads, dz = eng.backward(z, x, dx)
        grads2, dz2 = eng.backward(z, x, dx)
        assert all(torch.equal(grads[k].view(torch.int32), grads2[k].view(torch.int32)) for k in grads) and torch.equal(dz.view(torch.int32), dz2.view(torch.int32))
        acts = [eng.activation(i).cpu().numpy() for i in range(len(case.F))]
        names = inp.cfg.variable_names(inp.w)[:3]
        return case, inp, names, acts, x.cpu().numpy(), dx.cpu().numpy(), {k: v.cpu().numpy() for k, v in grads.items()}, dz.cpu().numpy()
    finally:
        eng.close()


@pytest.mark.parametrize('name', CHAIN_NETS)
def test_whole_chain(name):
    case, inp, names, acts, x, dx, grads, dz = _chain(name)
    assert np.count_nonzero(dx) and np.count_nonzero(dx) < dx.size                  # bootstrapped: some elements carry no gradient
    g64, dz64, S = dg.chain_reference(inp.w, names, inp.z, acts, x, dx, inp.cfg.layer_dimensions())
    g32, dz32, _ = dg.chain_reference(inp.w, names, inp.z, acts, x, dx, inp.cfg.layer_dimensions(), dtype=np.float32)
    assert set(grads) == set(g64) and all(grads[k].shape == g64[k].shape for k in g64)
    rows = [(k, grads[k], g32[k], g64[k], S[k].max()) for k in g64] + [('dz', dz, dz32, dz64, S['dz'].max())]
    worst32 = worst_gpu = 0.0
    failed = []
    for k, got, f32, f64, s in rows:
        assert s > 0 and not np.isnan(got).any(), k
        e32, egpu = float(np.abs(f32.astype(np.float64) - f64).max() / s), float(np.abs(got.astype(np.float64) - f64).max() / s)
        worst32, worst_gpu = max(worst32, e32), max(worst_gpu, egpu)
        print('%s %-18s float32 NumPy %.3e   GPU %.3e   (of the largest S)' % (name, k, e32, egpu))
        if not egpu <= 4.0 * e32:
            failed.append((k, e32, egpu))
    print('%s: largest float32-NumPy error %.3e, largest GPU error %.3e' % (name, worst32, worst_gpu))
    assert not failed, failed


def test_ae_gradients_device():
    import decoder_form_cases as dc
    from oracle import synth
    from augmentedautoencoder_amd import session as S
    from augmentedautoencoder_amd.ae import AE
    from augmentedautoencoder_amd.decoder import Decoder
    from augmentedautoencoder_amd.encoder import Encoder
    from augmentedautoencoder_amd.loss import latent_reg_loss
    case = {c.name: c for c in dc.cases()}['dense_generic']
    inputs = dc.build_inputs('dense_generic')
    F, strides = list(reversed(case.F)), list(reversed(case.S))
    with S.variable_scope('grad_api'):
        enc = Encoder(S.Placeholder(case.out), case.latent, F, case.k, strides, False)
        dec = Decoder(S.Placeholder(case.out, 'reconst_target'), enc.z, list(case.F), case.k, list(case.S), loss='L2', bootstrap_ratio=4, encoder=enc)
    try:
        enc.load_weights(synth.make_weights(seed=77, shape=case.out, num_filter=F, strides=strides, latent=case.latent))
        dec.load_weights(inputs.w)
        rng = np.random.RandomState(5)
        crops = rng.randint(0, 256, (5,) + tuple(case.out)).astype(np.uint8)
        target = rng.rand(5, *case.out).astype(np.float32)
        feed = {enc.x: crops, dec.reconstruction_target: target}
        loss0, grads0, dz0 = AE(enc, dec, 0.0, 0).gradients_device(feed)
        ae = AE(enc, dec, 0.25, 0)
        loss, grads, dz = ae.gradients_device(feed)
        assert abs(float(loss.cpu()[0]) - float(S.Session().run(ae.loss, feed))) <= 1e-6 * abs(float(loss.cpu()[0]))
        assert list(grads) == dec.engine.gradient_names() and all(np.array_equal(grads[k].cpu().numpy(), grads0[k].cpu().numpy()) for k in grads)
        z = enc.engine.encode_checked(enc._feed(feed))
        _, dz_reg = latent_reg_loss(dec.engine._z(z), grad=True)
        want = dz0.cpu().numpy() + dz_reg.cpu().numpy() * np.float32(0.25)
        assert np.abs(dz_reg.cpu().numpy()).max() > 0 and np.array_equal(dz.cpu().numpy(), want)
        for k, g in grads.items():
            assert tuple(g.shape) == np.shape(inputs.w[k]) and np.isfinite(g.cpu().numpy()).all() and np.abs(g.cpu().numpy()).max() > 0, k
        with pytest.raises(ValueError, match='single chunk'):
            dec.engine.backward(np.zeros((7, case.latent), np.float32), dec.engine.decode(np.zeros((5, case.latent), np.float32)), dec.engine.decode(np.zeros((5, case.latent), np.float32)))
    finally:
        dec.close()
        enc.close()
