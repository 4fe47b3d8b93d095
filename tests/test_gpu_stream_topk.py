"""Top-k (2 ... 8) of per-detection batches (B <= 4) on the GPU: sorted lists per block inside the stream scan, merged by the
last block to arrive -- one launch -- and the fused call aae_encode_nn_topk behind EncoderEngine.encode_nn(topk=...),
Codebook.nearest_rotation(top_n > 1) and auto_pose6d(top_n > 1).  The equalities are those of tests/test_emu_stream_topk.py:
against the library's own similarity at the same batch size (rows: canonical order, scores: bit for bit), against the top-1
answer, against the similarity-row form (AAE_SCAN_AUTO_TOPK_ROWS) and the merge-launch form (AAE_SCAN_STREAM_2L), and the
launch counts."""
import configparser

import numpy as np
import pytest

from oracle import reference_cpu as ref
from oracle import synth

pytestmark = pytest.mark.gpu

GAP_TOL = 2e-6           # the project's gap rule (tests/test_gpu_parity.py)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(cb, z, k):
    """cb: CodebookEngine, z: host latents [B,J] (B <= 4).  Returns the rows [B,k]."""
    from augmentedautoencoder_amd import _lib
    L = _lib.load()
    cb.set_scan_mode(_lib.AAE_SCAN_AUTO)
    cs = cb.similarity(z).cpu().numpy()
    i1, s1 = (t.cpu().numpy() for t in cb.nn(z, 1))
    want = ref.topk_canonical(cs, k)
    first = None
    for mode, launches in ((_lib.AAE_SCAN_AUTO, 1), (_lib.AAE_SCAN_STREAM_2L, 2), (_lib.AAE_SCAN_AUTO_TOPK_ROWS, 3), (_lib.AAE_SCAN_AUTO, 1)):
        cb.set_scan_mode(mode)
        ik, sk = cb.nn(z, k)
        assert L.aae_codebook_last_launches() == launches, mode
        ik, sk = ik.cpu().numpy(), sk.cpu().numpy()
        assert np.array_equal(ik, want), (mode, ik, want)
        assert np.array_equal(_bits(sk), _bits(np.take_along_axis(cs, ik, axis=1))), mode
        assert np.array_equal(ik[:, :1], i1) and np.array_equal(_bits(sk[:, :1]), _bits(s1)), mode
        if first is None:
            first = (ik, sk)
        assert np.array_equal(ik, first[0]) and np.array_equal(_bits(sk), _bits(first[1])), mode
    cb.set_scan_mode(_lib.AAE_SCAN_AUTO)
    return first[0]


def _oracle_swaps(ik, cs64, k):
    want = ref.topk_canonical(cs64, k)
    swaps = 0
    for b in range(len(ik)):
        for j in range(k):
            if ik[b, j] != want[b, j]:
                d = abs(float(cs64[b, ik[b, j]]) - float(cs64[b, want[b, j]]))
                assert d < GAP_TOL, (b, j, ik[b, j], want[b, j], d)
                swaps += 1
    return swaps


@pytest.fixture(scope='module')
def tie_book():
    """401 rows (three full 128-row blocks and a partial one) with identical rows in one block and in others"""
    from augmentedautoencoder_amd.engine import CodebookEngine
    E = synth.make_codebook(401, 128, seed=7, planted_duplicates=0)
    twins = [7, 130, 140, 300]
    for r in twins[1:]:
        E[r] = E[twins[0]]
    z = np.concatenate([3.0 * E[7:8], np.random.default_rng(1234).standard_normal((3, 128)).astype(np.float32)])
    cb = CodebookEngine(E)
    yield cb, z, twins
    cb.close()


@pytest.mark.parametrize('k', [2, 8])
@pytest.mark.parametrize('B', [1, 4])
def test_full_and_partial_blocks_with_identical_rows(tie_book, B, k):
    cb, z, twins = tie_book
    ik = _check(cb, z[:B], k)
    assert ik[0, :min(k, 4)].tolist() == twins[:min(k, 4)]


def test_second_block_of_two_rows():
    from augmentedautoencoder_amd.engine import CodebookEngine
    E = synth.make_codebook(130, 128, seed=7, planted_duplicates=0)
    z = synth.make_queries_near_rows(E, [129, 128, 3, 50], noise=0.3, seed=4)
    cb = CodebookEngine(E)
    ik = _check(cb, z, 8)
    assert ik[0, 0] == 129 and ik[1, 0] == 128 and ik.max() < 130
    cb.close()


def test_more_blocks_than_finisher_threads():
    from augmentedautoencoder_amd.engine import CodebookEngine
    N = 128 * 300 + 5
    E = synth.make_codebook(N, 128, seed=7, planted_duplicates=0)
    rows = [N - 1, 128 * 299, 17, 128 * 150 + 3]
    z = synth.make_queries_near_rows(E, rows, noise=0.3, seed=8)
    cb = CodebookEngine(E)
    ik = _check(cb, z, 8)
    assert ik[:, 0].tolist() == rows
    cb.close()


def test_bf16_codebook():
    from augmentedautoencoder_amd.engine import CodebookEngine
    E = synth.make_codebook(256 * 2 + 7, 128, seed=7, planted_duplicates=0)
    z = np.random.default_rng(1234).standard_normal((3, 128)).astype(np.float32)
    cb = CodebookEngine(E, dtype='bf16')
    _check(cb, z, 5)
    cb.close()


def test_consecutive_calls_with_different_k_reuse_the_workspace(tie_book):
    cb, z, _ = tie_book
    cs4, cs1 = cb.similarity(z).cpu().numpy(), cb.similarity(z[:1]).cpu().numpy()
    i8, s8 = cb.nn(z, 8)
    i2, s2 = cb.nn(z[:1], 2)
    i1, _ = cb.nn(z, 1)
    i5, s5 = cb.nn(z, 5)
    assert np.array_equal(i8.cpu().numpy(), ref.topk_canonical(cs4, 8)) and np.array_equal(i2.cpu().numpy(), ref.topk_canonical(cs1, 2))
    assert np.array_equal(i5.cpu().numpy(), ref.topk_canonical(cs4, 5)) and np.array_equal(i1.cpu().numpy()[:, 0], np.argmax(cs4, axis=1))
    assert np.array_equal(_bits(s8.cpu().numpy()), _bits(np.take_along_axis(cs4, i8.cpu().numpy(), axis=1)))
    assert np.array_equal(_bits(s2.cpu().numpy()), _bits(np.take_along_axis(cs1, i2.cpu().numpy(), axis=1)))
    assert np.array_equal(_bits(s5.cpu().numpy()), _bits(np.take_along_axis(cs4, i5.cpu().numpy(), axis=1)))


# ---- the default network --------------------------------------------------------------------------------------------------
class _Views(object):
    """what Codebook asks of a dataset: 1000 embedding views (rotations are looked up by row, never computed with)"""
    embedding_size = 1000
    _kw = {'num_cyclo': 36}

    def __init__(self):
        self.viewsphere_for_embedding = np.random.default_rng(3).standard_normal((1000, 3, 3))


@pytest.fixture(scope='module')
def default_net():
    from augmentedautoencoder_amd import session as S
    from augmentedautoencoder_amd.codebook import Codebook
    from augmentedautoencoder_amd.encoder import Encoder
    weights = synth.make_weights(seed=2024)
    ds = _Views()
    with S.variable_scope('stream_topk'):
        enc = Encoder(S.Placeholder((128, 128, 3)), 128, synth.DEFAULT_NUM_FILTER, 5, [2, 2, 2, 2], False)
        cb = Codebook(enc, ds, True)
    enc.load_weights(weights)
    E = synth.make_codebook(1000, 128, seed=7, planted_duplicates=0)
    cb.assign_embedding(E)
    crops = synth.make_crops(3, seed=5)
    z64 = ref.encoder_forward_np(ref.input_to_float(crops), weights, [2, 2, 2, 2])
    cs64 = ref.cos_similarity(z64, E)
    yield enc, cb, ds, E, crops, cs64
    cb.close(close_encoder=True)


@pytest.mark.parametrize('B', [1, 3])
def test_fused_call_equals_the_two_calls_and_the_fp64_oracle(default_net, B):
    from augmentedautoencoder_amd import _lib
    enc, cb, ds, E, crops, cs64 = default_net
    eng, cbe = enc.engine, cb.engine
    z0 = eng.encode(crops[:B])
    i0, s0 = cbe.nn(z0, 8)
    z1, i1, s1 = eng.encode_nn(cbe, crops[:B], topk=8)
    assert _lib.load().aae_codebook_last_launches() == 1
    assert i1.shape == (B, 8) and s1.shape == (B, 8)
    assert np.array_equal(_bits(z1.cpu().numpy()), _bits(z0.cpu().numpy()))
    assert np.array_equal(i1.cpu().numpy(), i0.cpu().numpy()) and np.array_equal(_bits(s1.cpu().numpy()), _bits(s0.cpu().numpy()))
    best = np.sort(cs64[:B], axis=1)[:, ::-1][:, :9]
    assert np.min(best[:, :-1] - best[:, 1:]) >= 4e-5        # the reference alone leaves the gap rule nothing to excuse
    assert _oracle_swaps(i1.cpu().numpy(), cs64[:B], 8) == 0


def test_nearest_rotation_and_auto_pose6d_top_n(default_net):
    enc, cb, ds, E, crops, cs64 = default_net
    want = ref.topk_canonical(cs64[:1], 8)[0]
    idcs = cb.nearest_rotation(None, crops[0], top_n=8, return_idcs=True)
    assert idcs.dtype == np.int64 and np.array_equal(idcs, want)
    assert np.array_equal(cb.nearest_rotation(None, crops[:1], top_n=8), ds.viewsphere_for_embedding[want])
    ii, ss = cb.nearest_rotation_with_scores(crops[:1], top_n=8)
    assert ii.shape == (1, 8) and np.array_equal(ii[0], want) and np.all(np.diff(ss[0]) <= 0)
    assert np.abs(ss[0] - cs64[0, want]).max() < 1e-5
    rng = np.random.default_rng(4)
    cb.assign_obj_bbs(np.stack([rng.integers(200, 300, 1000), rng.integers(150, 250, 1000), rng.integers(60, 200, 1000), rng.integers(60, 200, 1000)], 1))
    args = configparser.ConfigParser()
    args.read_string('[Dataset]\nRADIUS: 700\nK: [1075.65, 0, 720/2, 0, 1073.90, 540/2, 0, 0, 1]\n')
    K_test = np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]])
    box = [310, 180, 90, 120]
    Rs, ts = cb.auto_pose6d(None, crops[0], box, K_test, 8, args)
    Rw, tw = cb.pose_from_indices(want, box, K_test, args)
    assert Rs.shape == (8, 3, 3) and ts.shape == (8, 3)
    assert np.array_equal(Rs, Rw) and np.array_equal(ts, tw)
    with pytest.raises(ValueError):
        cb.nearest_rotation(None, crops[:2], top_n=2)
