"""The training loss on the MI355X: the case table of tests/loss_reference.py through aae_recon_loss (outputs handed in full of NaN,
the workspace full of 0xA5) against the NumPy restatement, the regulariser, a second call, a null dx, the refusals, and
Decoder.reconstr_loss / Encoder.reg_loss / AE.loss on the smallest decoder of tests/decoder_form_cases.py without batch norm.

Bounds (tests/loss_reference.py): per_image and loss within 1e-5 relative of the float64 sums ((64 + log2(B n)) u < 6e-6); L2
gradients within 4 u relative of float64; L1 gradients bit-equal to +-float32(1 / (B k)) or 0; the set of non-zero gradients equal
to the reference's selected set.  Measured maxima over the table: sums 1.6e-7 relative, L2 gradients 1.63 u; the regulariser: loss
3.6e-8 relative, gradient 0.99 u."""
import ctypes

import numpy as np
import pytest

import loss_reference as lr

pytestmark = pytest.mark.gpu


def _nan(shape):
    import torch
    return torch.full(tuple(shape), float('nan'), dtype=torch.float32, device='cuda')


def _workspace(B, n, extra=0):
    import torch
    from augmentedautoencoder_amd import _lib
    need = int(_lib.load().aae_recon_loss_workspace_bytes(B, n))
    assert need >= 4 * B and need % 16 == 0
    return torch.full((need + extra,), 0xA5, dtype=torch.uint8, device='cuda')


@pytest.fixture(scope='module')
def device_cases():
    import torch
    cache = {}

    def get(name):
        if name not in cache:
            x, t, kind, ratio, _ = lr.build(name)
            cache[name] = (torch.from_numpy(x.copy()).cuda(), torch.from_numpy(t.copy()).cuda(), kind, ratio)       # (the shared arrays are read-only)
        return cache[name]
    return get


def _call(device_cases, name, grad=True):
    from augmentedautoencoder_amd import loss as L
    x, t, kind, ratio = device_cases(name)
    B, n = x.shape
    out = (_nan((1,)), _nan((B,)), _nan((B, n)) if grad else None)
    loss, per_image, dx = L.reconstruction_loss(x, t, loss=kind, bootstrap_ratio=ratio, out=out, workspace=_workspace(B, n))
    assert loss is out[0] and per_image is out[1] and dx is out[2]
    return loss.cpu().numpy(), per_image.cpu().numpy(), None if dx is None else dx.cpu().numpy()


@pytest.mark.parametrize('name', sorted(lr.CASES))
def test_table_matches_reference(device_cases, name):
    loss, per_image, dx = _call(device_cases, name)
    ok = ~np.isnan(lr.build(name)[4]['per_image'])
    assert not np.isnan(dx[ok]).any()                                                 # every element was written
    sum_err, grad_err = lr.check(name, loss[0], per_image, dx)
    print('%s: sums %.2e relative, L2 gradient %.2f u' % (name, sum_err, grad_err))


@pytest.mark.parametrize('name', ['rand_n5106_B67_L2_r4', 'ties_cut_L1_B67', 'ties_cut_over_resident', 'product_L2_r4', 'rand_n105_B5_L1_r1', 'nan_image_L2'])
def test_second_call_and_null_dx_give_the_same_bits(device_cases, name):
    first = _call(device_cases, name)
    again = _call(device_cases, name)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    loss, per_image, dx = _call(device_cases, name, grad=False)
    assert dx is None and loss.tobytes() == first[0].tobytes() and per_image.tobytes() == first[1].tobytes()


def test_null_per_image_through_the_c_abi(device_cases):
    import torch
    from augmentedautoencoder_amd import _lib
    lib = _lib.load()
    name = 'ties_cut_L2'
    x, t, kind, ratio = device_cases(name)
    B, n = x.shape
    want = _call(device_cases, name)
    loss, ws = _nan((1,)), _workspace(B, n)
    desc = _lib.ReconLossDesc(B, n, _lib.AAE_LOSS_L2, ratio)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.aae_recon_loss(ctypes.byref(desc), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(loss.data_ptr()), None, None,
                            ctypes.c_void_p(ws.data_ptr()), ws.numel(), stream)
    assert rc == 0 and loss.cpu().numpy().tobytes() == want[0].tobytes()


def test_refusals_launch_nothing(device_cases):
    import torch
    from augmentedautoencoder_amd import _lib, loss as L
    lib = _lib.load()
    x, t, kind, ratio = device_cases('rand_n105_B5_L2_r4')
    B, n = x.shape
    loss, per_image, dx, ws = _nan((1,)), _nan((B,)), _nan((B, n)), _workspace(B, n, extra=16)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda tensor, off=0: ctypes.c_void_p(tensor.data_ptr() + off)
    full = int(lib.aae_recon_loss_workspace_bytes(B, n))

    def call(desc, x_=x, t_=t, loss_=loss, ws_=p(ws), ws_bytes=full):
        return lib.aae_recon_loss(ctypes.byref(desc) if desc is not None else None, None if x_ is None else p(x_), None if t_ is None else p(t_),
                                  None if loss_ is None else p(loss_), p(per_image), p(dx), ws_, ws_bytes, stream)

    good = _lib.ReconLossDesc(B, n, 0, 4)
    assert call(None) == -1 and call(good, x_=None) == -1 and call(good, t_=None) == -1 and call(good, loss_=None) == -1 and call(good, ws_=None) == -1
    for bad in ((0, n, 0, 4), (B, 0, 0, 4), (B, n, 0, 0), (B, n, 0, -3), (B, n, 2, 4), (B, n, -1, 4), (B, n, 0, n + 1)):
        assert call(_lib.ReconLossDesc(*bad)) == -1, bad
    assert b'n / ratio = 0' in lib.aae_last_error()
    assert call(_lib.ReconLossDesc(_lib.AAE_LOSS_MAX_BATCH + 1, n, 0, 4)) == -2 and call(_lib.ReconLossDesc(B, _lib.AAE_LOSS_MAX_N + 1, 0, 4)) == -2
    assert call(good, ws_bytes=full - 1) == -4 and call(good, ws_=p(ws, 4)) == -4
    assert lib.aae_recon_loss_workspace_bytes(0, n) == 0 and lib.aae_recon_loss_workspace_bytes(B, _lib.AAE_LOSS_MAX_N + 1) == 0
    z, dz = torch.ones((3, 8), device='cuda'), _nan((3, 8))
    reg = lambda z_, B_, J_: lib.aae_latent_reg_loss(None if z_ is None else p(z_), B_, J_, p(loss), p(dz), stream)
    assert reg(None, 3, 8) == -1 and reg(z, 0, 8) == -1 and reg(z, 3, 0) == -1 and reg(z, _lib.AAE_LOSS_MAX_BATCH + 1, 8) == -2
    assert lib.aae_latent_reg_loss(p(z), 3, 8, None, p(dz), stream) == -1
    with pytest.raises(ValueError, match='n // ratio = 0'):
        L.reconstruction_loss(x, t, bootstrap_ratio=n + 1, out=(loss, per_image, dx))
    with pytest.raises(ValueError, match='shape'):
        L.reconstruction_loss(x, t[:, :-1].contiguous(), out=(loss, per_image, dx))
    with pytest.raises(ValueError, match='contiguous'):
        L.reconstruction_loss(x.t(), t.t(), out=(loss, per_image, dx))
    with pytest.raises(ValueError, match='shape'):
        L.reconstruction_loss(x, t, out=(loss, per_image[:-1], dx))
    torch.cuda.synchronize()
    for out in (loss, per_image, dx, dz):
        assert torch.isnan(out).all()                                                 # nothing ran
    assert (ws == 0xA5).all()
    assert call(good) == 0                                                            # and the same arguments, unspoilt, are accepted
    torch.cuda.synchronize()
    assert not torch.isnan(dx).any() and not torch.isnan(loss).any()


@pytest.mark.parametrize('J,B', lr.REG_CASES)
def test_latent_reg_loss(J, B):
    import torch
    from augmentedautoencoder_amd import loss as L
    z = lr.reg_input(J, B)
    zd = torch.from_numpy(z).cuda()
    out = (_nan((1,)), _nan((B, J)))
    loss, dz = L.latent_reg_loss(zd, out=out)
    assert loss is out[0] and dz is out[1]
    lerr, gerr = lr.check_reg(z, loss.cpu().numpy()[0], dz.cpu().numpy())
    print('J=%d B=%d: loss %.2e relative, gradient %.2f u' % (J, B, lerr, gerr))
    again, dz2 = L.latent_reg_loss(zd, grad=True)
    none, no_dz = L.latent_reg_loss(zd)
    assert no_dz is None and again.cpu().numpy().tobytes() == loss.cpu().numpy().tobytes() == none.cpu().numpy().tobytes()
    assert dz2.cpu().numpy().tobytes() == dz.cpu().numpy().tobytes()
    if B == 67:
        assert not dz[5].any() and not dz[6].any() and not dz[7].any()               # the zero row and the two rows of norm exactly 1


# ---- through the API --------------------------------------------------------------------------------------------------------------
NET = 'dense_generic'          # 8 x 8 x 3, two layers, latent 33: the smallest network of the decoder table, no batch norm


@pytest.fixture(scope='module')
def autoencoder():
    import decoder_form_cases as dc
    from oracle import synth
    from augmentedautoencoder_amd import session as S
    from augmentedautoencoder_amd.decoder import Decoder
    from augmentedautoencoder_amd.encoder import Encoder
    case = {c.name: c for c in dc.cases()}[NET]
    assert not case.bn and case.out == min((c.out for c in dc.cases() if not c.bn), key=lambda o: o[0] * o[1] * o[2])
    inputs = dc.build_inputs(NET)
    F, strides = list(reversed(case.F)), list(reversed(case.S))                         # encoder order
    with S.variable_scope('loss_api'):
        enc = Encoder(S.Placeholder(case.out), case.latent, F, case.k, strides, False)
        dec = {(kind, ratio): Decoder(S.Placeholder(case.out, 'reconst_target'), enc.z, list(case.F), case.k, list(case.S), loss=kind, bootstrap_ratio=ratio,
                                      encoder=enc) for kind, ratio in (('L2', 4), ('L1', 1))}
    enc.load_weights(synth.make_weights(seed=77, shape=case.out, num_filter=F, strides=strides, latent=case.latent))
    for d in dec.values():
        d.load_weights(inputs.w)
    rng = np.random.RandomState(5)
    crops = rng.randint(0, 256, (5,) + tuple(case.out)).astype(np.uint8)
    target = rng.rand(5, *case.out).astype(np.float32)
    yield enc, dec, crops, target, np.asarray(inputs.z)
    for d in dec.values():
        d.close()
    enc.close()


def _loss64(recon, target, kind, ratio):
    B = recon.shape[0]
    return lr.reference(recon.reshape(B, -1), target.reshape(B, -1), kind, ratio)['loss']


@pytest.mark.parametrize('kind,ratio', [('L2', 4), ('L1', 1)])
def test_decoder_reconstr_loss(autoencoder, kind, ratio):
    from augmentedautoencoder_amd import session as S
    enc, decs, crops, target, z = autoencoder
    dec = decs[(kind, ratio)]
    sess = S.Session()
    got = sess.run(dec.reconstr_loss, {enc.x: crops, dec.reconstruction_target: target})
    recon = sess.run(dec.x, {enc.x: crops})
    assert isinstance(got, np.float32) and recon.dtype == np.float32
    want = _loss64(recon, target, kind, ratio)
    assert abs(float(got) - want) <= lr.SUM_RTOL * want, (got, want)
    # latent codes in place of the encoder's input, and a device-resident target
    import torch
    got_z = sess.run(dec.reconstr_loss, {dec._latent_code: z[:2].copy(), dec.reconstruction_target: torch.from_numpy(target[:2]).cuda()})
    want_z = _loss64(sess.run(dec.x, {dec._latent_code: z[:2].copy()}), target[:2], kind, ratio)
    assert abs(float(got_z) - want_z) <= lr.SUM_RTOL * want_z, (got_z, want_z)
    loss, per_image, dx, x = dec.reconstr_loss_device({enc.x: crops, dec.reconstruction_target: target}, grad=True)
    assert x.is_cuda and dx.shape == x.shape and per_image.shape == (5,) and loss.cpu().numpy()[0].tobytes() == got.tobytes()
    with pytest.raises(ValueError, match='shape'):
        sess.run(dec.reconstr_loss, {enc.x: crops, dec.reconstruction_target: target[:3]})


@pytest.mark.parametrize('norm_regularize', [0.0, 0.1])
def test_ae_loss(autoencoder, norm_regularize):
    from augmentedautoencoder_amd import session as S
    from augmentedautoencoder_amd.ae import AE
    enc, decs, crops, target, _ = autoencoder
    dec = decs[('L2', 4)]
    ae = AE(enc, dec, norm_regularize, 0)
    sess = S.Session()
    feed = {ae.x: crops, ae.reconstruction_target: target}
    got = sess.run(ae.loss, feed)
    recon, z = sess.run([ae.reconstruction, ae.z], feed)
    want = _loss64(recon, target, 'L2', 4)
    reg = sess.run(enc.reg_loss, feed)
    reg64 = lr.reg_reference(z)[0]
    assert abs(float(reg) - reg64) <= lr.SUM_RTOL * reg64
    if norm_regularize > 0:
        want = want + reg64 * float(np.float32(norm_regularize))
    assert isinstance(got, np.float32) and abs(float(got) - want) <= lr.SUM_RTOL * want, (got, want)
    assert sess.run(ae.global_step) == 0
