"""The encoder's backward pass on the MI355X: the case table of tests/encoder_grad_reference.py through aae_conv_backward /
aae_linear_backward (encoder_grad.py), outputs handed in full of NaN and the workspace full of 0xA5; the refusals; then the whole
chain encode -> a seeded random dz -> backward on two encoders, and AE.variable_gradients_device.

Per element, every tensor, no element left out:  |got - ref64| <= (n + 8) u S,  u = 2^-24  (derived in encoder_grad_reference.py,
not measured).  A second call gives the same bits; the labels are the planner's restatement; the refusals launch nothing.
Measured maxima as multiples of u S: MEASURED_LAYER_MAXIMA below.

Whole chain: the reference back-propagates in float64 through the DEVICE's saved activations.  Per-layer errors compound, so the
tolerance is measured, as in test_gpu_decoder_bwd.py: the same NumPy restatement in float32 against float64 on these cases, and the
GPU is allowed 4x that error per tensor, relative to the tensor's largest S (the same precision, another order).  MEASURED_CHAIN below."""
import collections
import ctypes

import numpy as np
import pytest

import encoder_grad_reference as eg

pytestmark = pytest.mark.gpu

# largest |got - ref64| / (u S) over the table, per tensor (MI355X); the bound is (n + 8)
MEASURED_LAYER_MAXIMA = 'delta 0.00, db 1.54 (ragged_ch), dw 3.67 (wide; dense 2.49), g_in 4.01 (split_k), g_a 3.38 (linear_B67_J33_U20)'
# whole chain, per case: largest float32-NumPy error and largest GPU error over the tensors, both relative to the tensor's largest S
MEASURED_CHAIN = ('wino_64: float32 NumPy 9.06e-8, GPU 1.72e-7 (dx: 1.9 of its allowance of 4, the most any tensor used); '
                  'ragged_s1: 1.32e-7 and 1.13e-7 (dx 4.62e-8 and 8.85e-8)')


def _nan(shape):
    import torch
    return torch.full(tuple(shape), float('nan'), dtype=torch.float32, device='cuda')


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _dirty(nbytes):
    import torch
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device='cuda')


def _conv_desc(c, **over):
    from augmentedautoencoder_amd import _lib
    f = dict(B=c.B, H=c.H, W=c.W, Cin=c.Cin, Cout=c.Cout, KS=c.KS, S=c.S, x_dtype=_lib.AAE_DTYPE_U8 if c.u8 else _lib.AAE_DTYPE_F32)
    f.update(over)
    return _lib.ConvBackwardDesc(*[f[k] for k in ('B', 'H', 'W', 'Cin', 'Cout', 'KS', 'S', 'x_dtype')])


def _run_layer(c, inp):
    import torch
    from augmentedautoencoder_amd import _lib, encoder_grad as G
    lib = _lib.load()
    desc = _conv_desc(c)
    ws = _dirty(int(lib.aae_conv_backward_workspace_bytes(ctypes.byref(desc))))
    out = (_nan((c.KS, c.KS, c.Cin, c.Cout)), _nan((c.Cout,)), _nan((c.B, c.H, c.W, c.Cin)) if c.g_in else None)
    dw, db, g_in = G.conv_backward(_dev(inp['a_in']), _dev(inp['a_out']), _dev(inp['g_out']), _dev(inp['w']), c.S, out=out, workspace=ws)
    assert dw is out[0] and db is out[1] and g_in is out[2]
    got = {'delta': ws[:4 * inp['a_out'].size].view(torch.float32).reshape(inp['a_out'].shape).cpu().numpy(), 'db': db.cpu().numpy(), 'dw': dw.cpu().numpy()}
    if c.g_in:
        got['g_in'] = g_in.cpu().numpy()
    return got, G.labels()


def _run_dense(c, inp):
    from augmentedautoencoder_amd import _lib, encoder_grad as G
    lib = _lib.load()
    desc = _lib.DenseBackwardDesc(c.B, c.J, c.U)
    ws = _dirty(int(lib.aae_linear_backward_workspace_bytes(ctypes.byref(desc), int(c.g_a))))
    out = (_nan((c.J, c.U)), _nan((c.U,)), _nan((c.B, c.J)) if c.g_a else None)
    dw, db, g_a = G.linear_backward(_dev(inp['a']), _dev(inp['dz']), _dev(inp['w']), out=out, workspace=ws)
    got = {'db': db.cpu().numpy(), 'dw': dw.cpu().numpy()}
    if c.g_a:
        got['g_a'] = g_a.cpu().numpy()
    return got, G.labels()


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


@pytest.mark.parametrize('name', list(eg.CASES))
def test_layer_case(name):
    c = eg.CASES[name]
    got, labels = _run_layer(c, eg.layer_inputs(name))
    print('%s: labels %s' % (name, labels))
    worst = None
    try:
        worst = eg.check(name, eg.layer_reference(name), got)
    finally:
        print('%s: largest error in units of u S: %s' % (name, worst and ' '.join('%s %.2f' % kv for kv in sorted(worst.items()))))
    eg.check_labels(c, labels)
    if name == 'k1_8x8':                                                    # a parity class without a tap: exact zeros
        g = got['g_in']
        assert (g[:, 1::2].view(np.uint32) == 0).all() and (g[:, :, 1::2].view(np.uint32) == 0).all() and np.abs(g[:, ::2, ::2]).max() > 0
    again, _ = _run_layer(c, eg.layer_inputs(name))
    assert _same_bits(got, again), 'a second call gives other bits'


@pytest.mark.parametrize('name', list(eg.DENSE_CASES))
def test_dense_case(name):
    c = eg.DENSE_CASES[name]
    got, labels = _run_dense(c, eg.dense_inputs(name))
    print('%s: labels %s' % (name, labels))
    worst = None
    try:
        worst = eg.check(name, eg.dense_reference(name), got)
    finally:
        print('%s: largest error in units of u S: %s' % (name, worst and ' '.join('%s %.2f' % kv for kv in sorted(worst.items()))))
    eg.check_labels(c, labels)
    again, _ = _run_dense(c, eg.dense_inputs(name))
    assert _same_bits(got, again), 'a second call gives other bits'


def test_layer_refusals_launch_nothing():
    import torch
    from augmentedautoencoder_amd import _lib, encoder_grad as G
    lib = _lib.load()
    c, inp = eg.CASES['odd_9x9'], eg.layer_inputs('odd_9x9')
    a_in, a_out, g_out, w = (_dev(inp[k]) for k in ('a_in', 'a_out', 'g_out', 'w'))
    dw, db, ws = _nan(w.shape), _nan((c.Cout,)), _dirty(1 << 20)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    G.conv_backward(a_in, a_out, g_out, w, c.S)                             # (so that the label list is not empty to begin with)
    assert G.labels()
    desc = _conv_desc(c, S=3)
    a_out3 = torch.zeros((c.B, 3, 3, c.Cout), device='cuda')
    assert lib.aae_conv_backward_workspace_bytes(ctypes.byref(desc)) == 0
    rc = lib.aae_conv_backward(ctypes.byref(desc), p(a_in), p(a_out3), p(a_out3), p(w), p(dw), p(db), None, p(ws), ws.numel(), stream)
    assert rc == -2 and b'stride 3' in lib.aae_last_error() and G.labels() == []
    with pytest.raises(NotImplementedError, match='stride 3'):
        G.conv_backward(a_in, a_out3, a_out3, w, 3, out=(dw, db, None), workspace=ws)
    desc = _conv_desc(c)
    need = lib.aae_conv_backward_workspace_bytes(ctypes.byref(desc))
    rc = lib.aae_conv_backward(ctypes.byref(desc), p(a_in), p(a_out), p(g_out), p(w), p(dw), p(db), None, p(ws), need - 1, stream)
    assert rc == -4 and G.labels() == []
    rc = lib.aae_conv_backward(ctypes.byref(desc), p(a_in), p(a_out), p(g_out), p(w), p(dw), p(db), None, ctypes.c_void_p(ws.data_ptr() + 16), need, stream)
    assert rc == -4 and G.labels() == []
    with pytest.raises(ValueError, match='shape'):
        G.conv_backward(a_in, a_out, g_out, w, c.S, out=(dw, _nan((c.Cout + 1,)), None))
    with pytest.raises(ValueError, match='contiguous'):
        G.conv_backward(a_in.transpose(1, 2), a_out, g_out, w, c.S)
    with pytest.raises(ValueError, match='same'):
        G.conv_backward(a_in, a_out, g_out, w, 1)
    torch.cuda.synchronize()
    assert torch.isnan(dw).all() and torch.isnan(db).all() and (ws == 0xA5).all()


# ---- the whole chain ----------------------------------------------------------------------------------------------------------------
Net = collections.namedtuple('Net', 'shape filters strides latent B u8 options wino_layers')
CHAIN_NETS = collections.OrderedDict([
    # conv2 and conv3 of the forward run on the polyphase Winograd kernels (asked for at this small batch by a plain block count)
    ('wino_64', Net((64, 64, 3), (32, 64, 64), (2, 2, 2), 128, 8, True, (('winograd_min_blocks', 1),), 2)),
    # ragged channels, a non-square image, a stride-1 layer; the direct kernels
    ('ragged_s1', Net((12, 10, 3), (20, 33), (2, 1), 24, 3, False, (('winograd', 0),), 0)),
])


def _engine(net, **cfg):
    from oracle import synth
    from augmentedautoencoder_amd.engine import EncoderEngine
    from augmentedautoencoder_amd.weights import EncoderConfig
    w = synth.make_weights(seed=303, shape=net.shape, num_filter=list(net.filters), strides=list(net.strides), latent=net.latent, **cfg)
    eng = EncoderEngine(EncoderConfig(shape=net.shape, num_filter=net.filters, strides=net.strides, latent_space_size=net.latent, **cfg), w)
    for k, v in net.options:
        eng.set_option(k, v)
    return eng, w


def _crops(net, seed=17):
    rng = np.random.RandomState(seed)
    x = rng.randint(0, 256, (net.B,) + tuple(net.shape)).astype(np.uint8)
    return x if net.u8 else (x / 255.).astype(np.float32)


def _bwd_ws_fill(eng, value):
    """the engine's backward workspace (allocated by a first call) filled with `value`"""
    eng._bwd_ws.fill_(value)
    return eng._bwd_ws


@pytest.mark.parametrize('name', list(CHAIN_NETS))
def test_whole_chain(name):
    import torch
    from augmentedautoencoder_amd import encoder_grad as G
    net = CHAIN_NETS[name]
    eng, w = _engine(net)
    try:
        x = _crops(net)
        z, recs = eng.encode_timed(x)
        assert sum('conv_wino_f32' in r[0] for r in recs) == net.wino_layers, [r[0] for r in recs]
        dz = torch.from_numpy(np.random.RandomState(23).standard_normal(tuple(z.shape)).astype(np.float32)).cuda()
        eng.backward(x, dz)                                                 # (allocates the workspace)
        _bwd_ws_fill(eng, 0xA5)
        out = collections.OrderedDict((n, _nan(t.shape)) for n, t in zip(eng.gradient_names(), eng.device_weights()))
        grads, dx = eng.backward(x, dz, out=out, need_dx=True)
        labels = G.labels()
        grads2, dx2 = eng.backward(x, dz, need_dx=True)
        assert all(torch.equal(grads[k].view(torch.int32), grads2[k].view(torch.int32)) for k in grads) and torch.equal(dx.view(torch.int32), dx2.view(torch.int32))
        acts = [eng.activation(i).cpu().numpy() for i in range(len(net.filters))]
        grads = {k: v.cpu().numpy() for k, v in grads.items()}
        dx, dz = dx.cpu().numpy(), dz.cpu().numpy()
    finally:
        eng.close()
    # the labels: the dense layer, then every conv layer from the last to the first, each the planner's restatement
    H, W, C = net.shape
    layers = []
    for i, (f, s) in enumerate(zip(net.filters, net.strides)):
        layers.append(eg.Layer('conv%d' % (i + 1), net.B, H, W, C, f, 5, s, net.u8 and i == 0, True))
        H, W, C = -(-H // s), -(-W // s), f
    want = eg.plan(eg.Dense('dense', net.B, H * W * C, net.latent, True))
    for L in reversed(layers):
        want += eg.plan(L, L.name)
    assert len(labels) == len(want) and all(l.startswith(p) for l, (p, _) in zip(labels, want)), (labels, want)
    g64, dx64, S = eg.chain_reference(w, list(net.strides), x, acts, dz)
    g32, dx32, _ = eg.chain_reference(w, list(net.strides), x, acts, dz, dtype=np.float32)
    assert list(grads) == list(g64) and all(grads[k].shape == g64[k].shape for k in g64)
    rows = [(k, grads[k], g32[k], g64[k], S[k].max()) for k in g64] + [('dx', dx, dx32, dx64, S['g_in:conv2d'].max())]
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


def test_chain_refusals_launch_nothing():
    import torch
    from augmentedautoencoder_amd import encoder_grad as G
    net = CHAIN_NETS['ragged_s1']
    eng, _ = _engine(net)
    try:
        x = _crops(net)
        z = eng.encode(x)
        dz = torch.ones_like(z)
        eng.backward(x, dz)
        assert G.labels()
        out = collections.OrderedDict((n, _nan(t.shape)) for n, t in zip(eng.gradient_names(), eng.device_weights()))
        ws = _bwd_ws_fill(eng, 0xA5)

        def untouched():
            torch.cuda.synchronize()
            return all(torch.isnan(t).all() for t in out.values()) and bool((ws == 0xA5).all()) and eng._bwd_ws is ws

        # a workspace that is too small, a misaligned one: the C call itself
        wp = (ctypes.c_void_p * len(out))(*[t.data_ptr() for t in eng.device_weights()])
        gp = (ctypes.c_void_p * len(out))(*[t.data_ptr() for t in out.values()])
        xt = eng.to_device_batch(x)
        _, fwd = eng.ws.get(0)
        need = int(eng.lib.aae_encoder_backward_workspace_bytes(eng.handle, net.B))
        assert 0 < need <= ws.numel()
        args = lambda ptr, n: (eng.handle, net.B, ctypes.c_void_p(xt.data_ptr()), 1, ctypes.c_void_p(dz.data_ptr()), ctypes.c_void_p(fwd), wp, gp, None,
                               ctypes.c_void_p(ptr), n, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert eng.lib.aae_encoder_backward(*args(ws.data_ptr(), need - 1)) == -4 and G.labels() == [] and untouched()
        eng.backward(x, dz)
        _bwd_ws_fill(eng, 0xA5)
        assert eng.lib.aae_encoder_backward(*args(ws.data_ptr() + 16, need)) == -4 and G.labels() == [] and untouched()
        # a wrong batch: refused by the engine before the library is entered (the label list stays empty)
        with pytest.raises(ValueError, match='single chunk'):
            eng.backward(x[:2], dz[:2].contiguous(), out=out)
        assert G.labels() == [] and untouched()
    finally:
        eng.close()
    # compact_workspace (three layers: the first one's output would be overwritten by the third), then split precision
    net3 = Net((16, 16, 3), (32, 32, 32), (2, 2, 2), 16, 2, False, (), 0)
    eng, _ = _engine(net3)
    try:
        x = _crops(net3)
        dz = torch.ones_like(eng.encode(x))
        eng.backward(x, dz)
        for option, text in (('compact_workspace', 'compact_workspace'), ('precision', 'split precision')):
            eng.set_option(option, 1)
            _c_refusal(eng, net3.B, x, dz, text)
            out = collections.OrderedDict((n, _nan(t.shape)) for n, t in zip(eng.gradient_names(), eng.device_weights()))
            ws = _bwd_ws_fill(eng, 0xA5)
            with pytest.raises(NotImplementedError, match=text):
                eng.backward(x, dz, out=out)
            torch.cuda.synchronize()
            assert G.labels() == [] and all(torch.isnan(t).all() for t in out.values()) and bool((ws == 0xA5).all())
            eng.set_option(option, 0)
    finally:
        eng.close()
    # batch norm and a stride of 3: the engine refuses from the configuration; the library's own refusal is called directly
    for net, cfg, text in ((Net((16, 16, 3), (8, 8), (2, 2), 16, 2, False, (), 0), dict(batch_norm=True), 'batch_norm'),
                           (Net((18, 18, 3), (8, 8), (3, 2), 16, 2, False, (), 0), {}, 'stride 3')):
        eng, _ = _engine(net, **cfg)
        try:
            x = _crops(net)
            dz = torch.ones((net.B, net.latent), device='cuda')
            _c_refusal(eng, net.B, x, dz, text)
            with pytest.raises(NotImplementedError, match=text):
                eng.backward(x, dz)
            assert G.labels() == []
            assert eng.lib.aae_encoder_backward_workspace_bytes(eng.handle, net.B) == 0 and text.encode() in eng.lib.aae_last_error()
        finally:
            eng.close()


def _c_refusal(eng, B, x, dz, text):
    """aae_encoder_backward itself refuses with AAE_ERR_UNSUPPORTED and a message that names the cause: the label list, not empty
    before, is empty after; outputs handed in full of NaN and a workspace full of 0xA5 are untouched"""
    import torch
    from augmentedautoencoder_amd import encoder_grad as G
    G.linear_backward(torch.ones((2, 8), device='cuda'), torch.ones((2, 4), device='cuda'), torch.ones((8, 4), device='cuda'))
    assert G.labels()
    n = len(eng.gradient_names())
    outs = [_nan((64,)) for _ in range(n)]
    ws = _dirty(1 << 22)
    xt = eng.to_device_batch(x)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in outs])
    rc = eng.lib.aae_encoder_backward(eng.handle, B, ctypes.c_void_p(xt.data_ptr()), 1, ctypes.c_void_p(dz.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ptrs, ptrs, None,
                                      ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == -2 and text.encode() in eng.lib.aae_last_error(), (rc, eng.lib.aae_last_error())
    assert G.labels() == [] and all(torch.isnan(t).all() for t in outs) and bool((ws == 0xA5).all())


def test_ae_variable_gradients_device():
    import torch
    import decoder_form_cases as dc
    from oracle import synth
    from augmentedautoencoder_amd import session as S
    from augmentedautoencoder_amd.ae import AE
    from augmentedautoencoder_amd.decoder import Decoder
    from augmentedautoencoder_amd.encoder import Encoder
    case = {c.name: c for c in dc.cases()}['dense_generic']
    inputs = dc.build_inputs('dense_generic')
    F, strides = list(reversed(case.F)), list(reversed(case.S))
    with S.variable_scope('variable_grad_api'):
        enc = Encoder(S.Placeholder(case.out), case.latent, F, case.k, strides, False)
        dec = Decoder(S.Placeholder(case.out, 'reconst_target'), enc.z, list(case.F), case.k, list(case.S), loss='L2', bootstrap_ratio=4, encoder=enc)
    try:
        enc_w = synth.make_weights(seed=77, shape=case.out, num_filter=F, strides=strides, latent=case.latent)
        enc.load_weights(enc_w)
        dec.load_weights(inputs.w)
        rng = np.random.RandomState(5)
        crops = rng.randint(0, 256, (5,) + tuple(case.out)).astype(np.uint8)
        target = rng.rand(5, *case.out).astype(np.float32)
        feed = {enc.x: crops, dec.reconstruction_target: target}
        ae = AE(enc, dec, 0.25, 0)
        loss0, dgrads, dz = ae.gradients_device(feed)
        loss, grads = ae.variable_gradients_device(feed)
        assert list(grads) == enc.engine.gradient_names() + dec.engine.gradient_names()
        assert torch.equal(loss.view(torch.int32), loss0.view(torch.int32))
        for k in dec.engine.gradient_names():
            assert tuple(grads[k].shape) == np.shape(inputs.w[k]) and torch.equal(grads[k].view(torch.int32), dgrads[k].view(torch.int32)), k
        enc.engine.encode_checked(crops)
        egrads, _ = enc.engine.backward(crops, dz.contiguous())
        for k in enc.engine.gradient_names():
            g = grads[k].cpu().numpy()
            assert tuple(g.shape) == np.shape(enc_w[k]) and torch.equal(grads[k].view(torch.int32), egrads[k].view(torch.int32)), k
            assert np.isfinite(g).all() and np.abs(g).max() > 0, k
        with pytest.raises(ValueError, match='_latent_code'):
            ae.variable_gradients_device({dec._latent_code: np.zeros((5, case.latent), np.float32), dec.reconstruction_target: target})
    finally:
        dec.close()
        enc.close()
