"""The training loss without a GPU: csrc/kernels/loss_core.h compiled for the host and driven serially by tests/native/loss_host.cpp
over the case table of tests/loss_reference.py, the same driver under -fsanitize=address,undefined, and what the API checks before
it touches the device: arguments, Decoder.reconstr_loss / Encoder.reg_loss / AE / build_ae construction and the refusals."""
import configparser
import os
import subprocess

import numpy as np
import pytest

import loss_reference as lr
from test_render_cpu import _compiler
from augmentedautoencoder_amd import _lib, ae_factory as factory, loss as L, session as S
from augmentedautoencoder_amd.ae import AE
from augmentedautoencoder_amd.decoder import Decoder
from augmentedautoencoder_amd.encoder import Encoder

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build(out_dir, flags, name):
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-O2', '-ffp-contract=off', '-Wall'] + flags + [os.path.join(HERE, 'native', 'loss_host.cpp'), '-o', exe])
    return exe


@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('loss_host'), [], 'loss_host')


def _run(exe, tmp_path, name):
    x, t, kind, ratio, _ = lr.build(name)
    src, out = str(tmp_path / 'loss_in.bin'), str(tmp_path / 'loss_out.bin')
    lr.write_input(src, x, t, kind, ratio)
    subprocess.check_call([exe, src, out])
    return lr.read_output(out, *x.shape)


def _run_reg(exe, tmp_path, z):
    src, out = str(tmp_path / 'reg_in.bin'), str(tmp_path / 'reg_out.bin')
    with open(src, 'wb') as f:
        np.array(z.shape, dtype=np.int32).tofile(f)
        z.tofile(f)
    subprocess.check_call([exe, '--reg', src, out])
    raw = np.fromfile(out, dtype=np.float32)
    return raw[0], raw[1:].reshape(z.shape)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_reference_order_is_the_stable_descending_sort():
    rng = np.random.RandomState(3)
    e = rng.randint(0, 6, 500).astype(np.float32) * np.float32(0.125)                 # many ties
    assert np.array_equal(lr.order(e), np.argsort(-e, kind='stable'))
    e[17] = lr.NEG_NAN
    e[400] = np.nan
    assert lr.order(e)[:2].tolist() == [17, 400]                                      # NaNs first, whatever their sign, lower index first
    ref = lr.reference(np.array([[3, 1, 3, 0, 3, 2]], np.float32), np.zeros((1, 6), np.float32), 'L1', 2)
    assert ref['sel'].tolist() == [[True, False, True, False, True, False]] and ref['per_image'].tolist() == [3.0]
    ref = lr.reference(np.array([[3, 1, 3, 0, 3, 2]], np.float32), np.zeros((1, 6), np.float32), 'L2', 3)
    assert ref['sel'].tolist() == [[True, False, True, False, False, False]] and ref['dx'][0, :3].tolist() == [3.0, 0.0, 3.0]


def test_cases_cover_what_they_claim():
    names = set(lr.CASES)
    for n in (lr.N_TINY, lr.N_SMALL, lr.N_RAGGED):
        for B in (1, 5, 67):
            for kind in ('L2', 'L1'):
                assert 'rand_n%d_B%d_%s_r1' % (n, B, kind) in names
    for kind in ('L2', 'L1'):
        for ratio in (2, 3, 4, lr.N_RAGGED):
            assert 'rand_n%d_B67_%s_r%d' % (lr.N_RAGGED, kind, ratio) in names
    assert lr.N_SMALL < 1024 and lr.N_SMALL % 4 and 1024 < lr.N_RAGGED <= 8192 and lr.N_PRODUCT == 48 * 1024 < lr.N_OVER
    assert lr.N_RAGGED % 4 and lr.N_SMALL % 2 and lr.N_SMALL % 4                        # k = n // ratio is a floor at ratios 2 and 4 (both sizes are multiples of 3)
    x, t, kind, ratio, ref = lr.build('subnormal_errors')
    tiny = np.finfo(np.float32).tiny
    kth = np.sort(ref['e'], axis=1)[:, ::-1][:, ref['k'] - 1]
    assert ((kth > 0) & (kth < tiny)).all() and (ref['e'] == 0.25).any() and (ref['per_image'] > tiny).all()
    x, t, kind, ratio, ref = lr.build('low_mantissa_bit')
    assert len(np.unique(ref['e'].view(np.uint32) >> 1)) == 1 and len(np.unique(ref['e'])) == 2
    x, t, kind, ratio, ref = lr.build('exponent_only')
    assert not (ref['e'].view(np.uint32) & 0x7FFFFF).any() and len(np.unique(ref['e'])) == 20
    x, t, kind, ratio, ref = lr.build('one_ulp_apart')
    srt = np.sort(ref['e'][0])[::-1]
    assert int(srt[ref['k'] - 1].view(np.uint32)) - int(srt[ref['k']].view(np.uint32)) == 1
    x, t, kind, ratio, ref = lr.build('nan_image_L2')
    assert np.isnan(ref['per_image']).tolist() == [False, False, True, False, False] and np.isnan(ref['loss'])
    assert (ref['e'][2].view(np.uint32) >> 31).any()                                    # the squared NaN keeps its sign bit: the key has to clear it
    x, t, kind, ratio, ref = lr.build('ties_cut_over_resident')
    assert (ref['sel'][:, 48 * 1024:].any(axis=1)).all() and not ref['sel'][:, 49000].any()      # ties past row 48: the first taken, the last not


# ---- the core header on the host ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(lr.CASES))
def test_host_driver_matches_reference(host_exe, tmp_path, name):
    sum_err, grad_err = lr.check(name, *_run(host_exe, tmp_path, name))
    print('%s: sums %.2e relative, L2 gradient %.2f u' % (name, sum_err, grad_err))


@pytest.mark.parametrize('J,B', lr.REG_CASES)
def test_host_driver_reg_loss(host_exe, tmp_path, J, B):
    z = lr.reg_input(J, B)
    lerr, gerr = lr.check_reg(z, *_run_reg(host_exe, tmp_path, z))
    print('J=%d B=%d: loss %.2e relative, gradient %.2f u' % (J, B, lerr, gerr))
    if B == 67:
        norm = np.sqrt((z.astype(np.float64) ** 2).sum(axis=1))
        assert (norm == 0).any() and (norm == 1).sum() >= 2 and (norm < 1).any() and (norm > 1).any()


def test_host_driver_under_sanitizers(tmp_path):
    """address + undefined-behaviour sanitizers on the stand-alone driver: every pass of the selection, the tie paths, NaN keys, n = 1"""
    exe = _build(tmp_path, ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'], 'loss_host_san')
    for name in ('rand_n1_B5_L2_r1', 'rand_n105_B5_L1_r105', 'ties_cut_L2', 'ties_end_at_k', 'subnormal_errors', 'low_mantissa_bit', 'nan_image_L2', 'all_equal_L1_small'):
        lr.check(name, *_run(exe, tmp_path, name))
    z = lr.reg_input(129, 67)
    lr.check_reg(z, *_run_reg(exe, tmp_path, z))


# ---- the API, before the device ----------------------------------------------------------------------------------------------------
def test_argument_checks_need_no_gpu():
    import torch
    x = torch.zeros((2, 4, 4, 3))
    with pytest.raises(ValueError, match='unknown loss'):
        L.reconstruction_loss(x, x, loss='L3')
    with pytest.raises(ValueError, match='torch tensor'):
        L.reconstruction_loss(np.zeros((2, 3), np.float32), x)
    with pytest.raises(ValueError, match='GPU'):
        L.reconstruction_loss(x, x)
    with pytest.raises(ValueError, match='float32'):
        L.reconstruction_loss(x.double(), x)
    with pytest.raises(ValueError, match='GPU'):
        L.latent_reg_loss(torch.zeros((2, 8)))
    with pytest.raises(ValueError, match='float32'):
        L.latent_reg_loss(torch.zeros((2, 8), dtype=torch.float16))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='bootstrap_ratio'):
            L.check_bootstrap_ratio(bad)
    with pytest.raises(ValueError, match='selects n // ratio = 0'):
        L.check_bootstrap_ratio(49, 48)
    assert L.check_bootstrap_ratio(48, 48) == 48 and L.check_bootstrap_ratio(4.0) == 4
    assert L.loss_kind('L2') == _lib.AAE_LOSS_L2 == 0 and L.loss_kind('L1') == _lib.AAE_LOSS_L1 == 1


NET_CFG = """
[Dataset]
H: 16
W: 16
C: 3
[Network]
BATCH_NORMALIZATION: False
AUXILIARY_MASK: %s
VARIATIONAL: %s
LOSS: %s
BOOTSTRAP_RATIO: 4
NORM_REGULARIZE: %s
LATENT_SPACE_SIZE: 128
NUM_FILTER: [32, 64]
STRIDES: [2, 2]
KERNEL_SIZE_ENCODER: 5
KERNEL_SIZE_DECODER: 5
"""


def _args(mask='False', variational='0', loss='L2', reg='0'):
    args = configparser.ConfigParser()
    args.read_string(NET_CFG % (mask, variational, loss, reg))
    return args


def _pair(args):
    enc = factory.build_encoder(S.Placeholder((16, 16, 3)), args)
    return enc, factory.build_decoder(S.Placeholder((16, 16, 3), 'reconst_target'), enc, args)


def test_build_ae_reads_its_two_settings():
    enc, dec = _pair(_args(reg='0.1'))
    ae = factory.build_ae(enc, dec, _args(reg='0.1'))
    assert isinstance(ae, AE) and ae._norm_regularize == 0.1 and not ae._variational
    assert ae.x is enc.x and ae.z is enc.z and ae.reconstruction is dec.x and ae.reconstruction_target is dec.reconstruction_target
    assert isinstance(ae.loss, S.Op) and isinstance(dec.reconstr_loss, S.Op) and isinstance(enc.reg_loss, S.Op)
    step = S.Session().run(ae.global_step)
    assert step == 0 and step.dtype == np.int64
    assert dec._loss == 'L2' and dec._bootstrap_ratio == 4
    with pytest.raises(configparser.NoOptionError):
        args = _args()
        args.remove_option('Network', 'NORM_REGULARIZE')
        factory.build_ae(enc, dec, args)


def test_refusals():
    enc, dec = _pair(_args())
    with pytest.raises(NotImplementedError, match='q_sigma'):
        factory.build_ae(enc, dec, _args(variational='0.5'))
    with pytest.raises(NotImplementedError, match='q_sigma'):
        AE(enc, dec, 0.0, 1)
    with pytest.raises(ValueError, match='unknown loss'):
        _pair(_args(loss='Huber'))
    with pytest.raises(ValueError, match='unknown loss'):
        Decoder(S.Placeholder((16, 16, 3)), enc.z, [64, 32], 5, [2, 2], loss='l2', encoder=enc)
    enc_m, dec_m = _pair(_args(mask='True'))
    with pytest.raises(NotImplementedError, match='mask head'):
        dec_m.reconstr_loss
    with pytest.raises(NotImplementedError, match='mask head'):
        factory.build_ae(enc_m, dec_m, _args(mask='True'))
    for name in ('build_queue', 'build_train_op'):
        with pytest.raises(NotImplementedError, match=name):
            getattr(factory, name)(None, None)
    with pytest.raises(NotImplementedError, match='is_training'):
        factory.build_encoder(S.Placeholder((16, 16, 3)), _args(), is_training=True)
    with pytest.raises(NotImplementedError, match='is_training'):
        factory.build_decoder(S.Placeholder((16, 16, 3)), enc, _args(), is_training=True)
    with pytest.raises(ValueError, match='reconstruction_target'):
        dec.reconstr_loss_device({dec._latent_code: np.zeros((1, 128), np.float32)})


def test_loss_symbols_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'aae_hip.h')).read()
    import __graft_entry__ as g
    g.build()
    out = subprocess.check_output(['/opt/rocm/lib/llvm/bin/llvm-readelf', '--dyn-syms', '--wide', g.LIB]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if ' FUNC ' in l and ' UND ' not in l)
    for name in ('aae_recon_loss_workspace_bytes', 'aae_recon_loss', 'aae_latent_reg_loss'):
        assert name + '(' in header and name in _lib.EXPORTED_SYMBOLS and name in exported
    for name, value in (('AAE_LOSS_L2', 0), ('AAE_LOSS_L1', 1), ('AAE_LOSS_MAX_BATCH', 65536), ('AAE_LOSS_MAX_N', 4194304), ('AAE_LOSS_MAX_LATENT', 1048576)):
        assert '#define %s %d' % (name, value) in header and getattr(_lib, name) == value
    assert '#define AAE_ABI_VERSION 3' in header or _lib.AAE_ABI_VERSION == 3
    assert ctypes_sizeof_desc() == 16


def ctypes_sizeof_desc():
    import ctypes
    return ctypes.sizeof(_lib.ReconLossDesc)
