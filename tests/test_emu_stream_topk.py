"""Top-k (2 ... 8) inside the B <= 4 stream scans, on the CPU fiber emulator: every block leaves a sorted list per query
(scan_block_topk_store), the last block to arrive merges them (scan_topk_merge_lists) -- one launch, no similarity row --
and the fused call aae_encode_nn_topk.  The reference defines top_n > 1 for one crop per call (codebook.py:69-71); the
canonical order is score descending, lower row first among equal scores (oracle.reference_cpu.topk_canonical).

Checked wherever a query runs (``_check``): the rows are the canonical top-k of the library's OWN similarity at the same
batch size, the scores are those similarity values bit for bit, entry 0 is the top-1 answer, and the in-launch form, the
form with a merge launch (AAE_SCAN_STREAM_2L) and the earlier similarity-row form (AAE_SCAN_AUTO_TOPK_ROWS) agree bit for
bit in every block order of the emulator (ascending, descending, scrambled)."""
import os

import numpy as np
import pytest

import emu_backend as eb
from augmentedautoencoder_amd import _lib
from augmentedautoencoder_amd.weights import EncoderConfig, to_bf16_bits
from oracle import reference_cpu as ref
from oracle import synth

GAP_TOL = 2e-6           # the project's gap rule (tests/test_gpu_parity.py): a differing row is excused only where the fp64 scores differ by less
BF16_GAP_TOL = 1e-5      # ... for bf16 codebooks
ROWS = {'f32': 128, 'bf16': 256}         # codebook rows per block of the stream kernels
MODES = (_lib.AAE_SCAN_AUTO, _lib.AAE_SCAN_STREAM_2L, _lib.AAE_SCAN_AUTO_TOPK_ROWS)
LAUNCHES = {_lib.AAE_SCAN_AUTO: 1, _lib.AAE_SCAN_STREAM_2L: 2, _lib.AAE_SCAN_AUTO_TOPK_ROWS: 3}


@pytest.fixture(autouse=True)
def _ascending_blocks_afterwards():
    yield
    eb.set_block_order(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _main_n(dtype):
    return 401 if dtype == 'f32' else 256 * 2 + 7      # three full blocks and a partial one / two and a partial one


def _check(cb, z, k, orders=(0, 1, 2), modes=MODES):
    """The equalities of the module docstring; returns (rows [B,k], scores [B,k], the library's own similarity)."""
    L = eb.lib()
    z = np.ascontiguousarray(z, dtype=np.float32)
    N = cb.E.shape[0]
    cb.set_mode(_lib.AAE_SCAN_AUTO)
    eb.set_block_order(0)
    cs = cb.similarity(z)
    i1, s1 = cb.nn(z, 1)
    want = ref.topk_canonical(cs, k)
    first = None
    for order in orders:
        eb.set_block_order(order)
        for mode in modes:
            cb.set_mode(mode)
            ik, sk = cb.nn(z, k)
            where = (order, mode)
            assert L.aae_codebook_last_launches() == LAUNCHES[mode], where
            assert np.array_equal(ik, want), (where, ik, want)
            assert np.array_equal(_bits(sk), _bits(np.take_along_axis(cs, ik, axis=1))), where
            assert np.array_equal(ik[:, :1], i1) and np.array_equal(_bits(sk[:, :1]), _bits(s1)), where
            assert ik.min() >= 0 and ik.max() < N, where
            for b in range(len(ik)):
                assert len(set(ik[b].tolist())) == k, (where, ik[b])
            if first is None:
                first = (ik, sk)
            assert np.array_equal(ik, first[0]) and np.array_equal(_bits(sk), _bits(first[1])), where
    cb.set_mode(_lib.AAE_SCAN_AUTO)
    eb.set_block_order(0)
    return first[0], first[1], cs


def _oracle_swaps(ik, z, E64, k, gap_tol):
    """Rows against the fp64 oracle's canonical list, position by position, under the gap rule: a different row passes only
    where its fp64 score is within gap_tol of the wanted one.  Returns how many positions the rule had to excuse."""
    cs64 = ref.cos_similarity(z, E64)
    want = ref.topk_canonical(cs64, k)
    best = np.sort(cs64, axis=1)[:, ::-1][:, :k + 1]
    assert np.min(best[:, :-1] - best[:, 1:]) >= 4e-5       # the reference alone leaves the rule nothing to excuse (fp32 scores: ~1e-7)
    swaps = 0
    for b in range(len(ik)):
        for j in range(k):
            if ik[b, j] != want[b, j]:
                d = abs(float(cs64[b, ik[b, j]]) - float(cs64[b, want[b, j]]))
                assert d < gap_tol, (b, j, ik[b, j], want[b, j], d)
                swaps += 1
    return swaps


def _bf16_rounded(E):
    return (to_bf16_bits(np.ascontiguousarray(E, dtype=np.float32)).astype(np.uint32) << 16).view(np.float32)


def _cluster(E, rows, seed, spread=0.3):
    """Makes `rows` of E near-copies of one direction u (cosine ~0.95 with u, the other rows ~0.1): the best rows of the query u
    are then exactly `rows`, in an order the noise decides.  Returns (E', u)."""
    rng = np.random.default_rng(seed)
    E = E.copy()
    J = E.shape[1]
    u = rng.standard_normal(J)
    u /= np.linalg.norm(u)
    for r in rows:
        v = u + spread * rng.standard_normal(J) / np.sqrt(J)
        E[r] = (v / np.linalg.norm(v)).astype(np.float32)
    return E, (7.5 * u).astype(np.float32)[None]


# ---- what fails on the commit before this kernel ------------------------------------------------------------------------------
def test_new_exports_in_header_binding_and_library():
    root = os.path.dirname(eb.HERE)
    header = open(os.path.join(root, 'include', 'aae_hip.h')).read()
    L = eb.lib()
    for name in ('aae_encode_nn_topk', 'aae_codebook_last_launches'):
        assert name + '(' in header
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(L, name)
    assert L.aae_abi_version() == _lib.AAE_ABI_VERSION == 3


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_one_launch_and_two_under_the_two_launch_mode(dtype):
    L = eb.lib()
    E = synth.make_codebook(_main_n(dtype), 128, seed=7, planted_duplicates=0)
    z = np.random.default_rng(1234).standard_normal((4, 128)).astype(np.float32)
    cb = eb.EmuCodebook(E, dtype)
    for B in (1, 4):
        for k in (2, 5, 8):
            cb.set_mode(_lib.AAE_SCAN_AUTO)
            cb.nn(z[:B], k)
            assert L.aae_codebook_last_launches() == 1, (B, k)
            cb.set_mode(_lib.AAE_SCAN_STREAM_2L)
            cb.nn(z[:B], k)
            assert L.aae_codebook_last_launches() == 2, (B, k)
    cb.set_mode(_lib.AAE_SCAN_AUTO)
    cb.nn(z[:1], 1)
    assert L.aae_codebook_last_launches() == 1
    cb.close()


def test_workspace_holds_no_similarity_rows():
    N = 128 * 300 + 5
    E = synth.make_codebook(N, 128, seed=7, planted_duplicates=0)
    cb = eb.EmuCodebook(E)
    L = eb.lib()
    extra = L.aae_codebook_workspace_bytes(cb.h, 4, 8) - L.aae_codebook_workspace_bytes(cb.h, 4, 1)
    assert 0 < extra < 4 * N * 4, extra
    cb.set_mode(_lib.AAE_SCAN_AUTO_TOPK_ROWS)           # the earlier form keeps its [B,N] rows
    assert L.aae_codebook_workspace_bytes(cb.h, 4, 8) - L.aae_codebook_workspace_bytes(cb.h, 4, 1) >= 4 * N * 4
    cb.close()


# ---- shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('B', [1, 2, 3, 4])
def test_shapes_and_the_fp64_oracle(B, dtype):
    """B x k on a codebook of full blocks and a partial one; no duplicate rows, so the fp64 oracle's list is the answer with
    nothing for the gap rule to excuse (the nine best fp64 scores of these inputs lie >= 4e-5 apart)."""
    E = synth.make_codebook(_main_n(dtype), 128, seed=7, planted_duplicates=0)
    z = np.random.default_rng(1234).standard_normal((4, 128)).astype(np.float32)[:B]
    cb = eb.EmuCodebook(E, dtype)
    E64 = _bf16_rounded(E) if dtype == 'bf16' else E
    for k in (2, 3, 5, 8):
        ik, _, _ = _check(cb, z, k)
        assert _oracle_swaps(ik, z, E64, k, BF16_GAP_TOL if dtype == 'bf16' else GAP_TOL) == 0
    cb.close()


@pytest.mark.parametrize('N', [100, 259, 387, 1000])
def test_fp64_oracle_on_more_codebooks(N):
    E = synth.make_codebook(N, 128, seed=7, planted_duplicates=0)
    z = np.random.default_rng(1234).standard_normal((4, 128)).astype(np.float32)
    cs64 = np.sort(ref.cos_similarity(z, E), axis=1)[:, ::-1]
    assert np.min(cs64[:, :8] - cs64[:, 1:9]) >= 4e-5          # the reference alone stays inside a cap of zero excused positions
    cb = eb.EmuCodebook(E)
    ik, _, _ = _check(cb, z, 8, orders=(0, 2), modes=(_lib.AAE_SCAN_AUTO,))
    assert _oracle_swaps(ik, z, E, 8, GAP_TOL) == 0
    cb.close()


def test_short_latent_code():
    E = synth.make_codebook(401, 8, seed=7, planted_duplicates=0)
    z = np.random.default_rng(1234).standard_normal((3, 8)).astype(np.float32)
    cb = eb.EmuCodebook(E)
    _check(cb, z, 5)
    cb.close()


# ---- tail blocks and sentinels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_second_block_of_two_rows(dtype):
    N = ROWS[dtype] + 2
    E = synth.make_codebook(N, 128, seed=7, planted_duplicates=0)
    z = synth.make_queries_near_rows(E, [N - 1, N - 2, 3, 50], noise=0.3, seed=4)       # two of them nearest to the short block
    cb = eb.EmuCodebook(E, dtype)
    ik, _, _ = _check(cb, z, 8)
    assert ik[0, 0] == N - 1 and ik[1, 0] == N - 2
    cb.close()


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('N', [8, 5])
def test_every_row_of_a_tiny_codebook(N, dtype):
    E = synth.make_codebook(N, 128, seed=7, planted_duplicates=0)
    z = np.random.default_rng(1234).standard_normal((2, 128)).astype(np.float32)
    cb = eb.EmuCodebook(E, dtype)
    ik, _, _ = _check(cb, z, N)
    assert sorted(ik[0].tolist()) == list(range(N)) and sorted(ik[1].tolist()) == list(range(N))
    cb.close()


# ---- where the best rows lie ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('k', [2, 5, 8])
def test_whole_list_from_one_block(k, dtype):
    """All k best rows in one block: the finisher has to follow ONE list to its end."""
    rpb = ROWS[dtype]
    N = 3 * rpb + 17
    E = synth.make_codebook(N, 128, seed=7, planted_duplicates=0)
    rows = [2 * rpb + r for r in (5, 64, 6, 127, 0, 33, 90, 91)[:k]]
    E, z = _cluster(E, rows, seed=k)
    cb = eb.EmuCodebook(E, dtype)
    ik, _, _ = _check(cb, np.concatenate([z, z[::-1] * 0.5 + E[3]]), k)
    assert sorted(ik[0].tolist()) == sorted(rows)
    cb.close()


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_one_row_per_block(dtype):
    rpb = ROWS[dtype]
    N = 8 * rpb + 5
    E = synth.make_codebook(N, 128, seed=7, planted_duplicates=0)
    rows = [b * rpb + off for b, off in enumerate((0, 127, 31, 64, 1, 99, 126, 2))]
    E, z = _cluster(E, rows, seed=11)
    cb = eb.EmuCodebook(E, dtype)
    ik, _, _ = _check(cb, z, 8)
    assert sorted(ik[0].tolist()) == rows
    cb.close()


def test_lists_that_share_a_finisher_lane_and_lists_read_to_different_depths():
    """Blocks 0 ... 11 are the twelve lists of the finisher's lane 0, block 12 is lane 1's: three best rows in block 3, two in
    block 7 (same lane), two in block 12, one in block 20."""
    N = 128 * 21 + 9
    E = synth.make_codebook(N, 128, seed=7, planted_duplicates=0)
    rows = [3 * 128 + 5, 3 * 128 + 6, 3 * 128 + 100, 7 * 128 + 1, 7 * 128 + 127, 12 * 128, 12 * 128 + 64, 20 * 128 + 8]
    E, z = _cluster(E, rows, seed=5)
    cb = eb.EmuCodebook(E)
    for k in (5, 8):
        ik, _, _ = _check(cb, z, k, orders=(0, 2))
        assert set(ik[0].tolist()) <= set(rows)
    cb.close()


# ---- ties -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_identical_rows_in_one_block_and_in_others(dtype):
    rpb = ROWS[dtype]
    N = 3 * rpb + 17
    E = synth.make_codebook(N, 128, seed=7, planted_duplicates=0)
    twins = [7, rpb + 2, rpb + 12, 2 * rpb + 44]
    for r in twins[1:]:
        E[r] = E[twins[0]]
    z = np.stack([3.0 * E[7], E[50]]).astype(np.float32)
    cb = eb.EmuCodebook(E, dtype)
    for k in (2, 5, 8):
        ik, sk, _ = _check(cb, z, k)
        assert ik[0, :min(k, 4)].tolist() == twins[:min(k, 4)]
        assert len(set(_bits(sk[0, :min(k, 4)]).tolist())) == 1
    cb.close()


def test_ten_identical_rows_over_three_blocks():
    N = 401
    E = synth.make_codebook(N, 128, seed=7, planted_duplicates=0)
    same = [3, 4, 90, 127, 128, 129, 200, 255, 256, 300]
    for r in same[1:]:
        E[r] = E[same[0]]
    z = np.stack([0.25 * E[3], E[3] + 0.01 * E[9], E[77], E[400]]).astype(np.float32)
    cb = eb.EmuCodebook(E)
    ik, _, _ = _check(cb, z, 8)
    assert ik[0].tolist() == same[:8] and ik[1].tolist() == same[:8]
    cb.close()


# ---- many blocks, buffers ---------------------------------------------------------------------------------------------------
def test_more_blocks_than_finisher_threads():
    N = 128 * 300 + 5
    E = synth.make_codebook(N, 128, seed=7, planted_duplicates=0)
    rows = [N - 1, 128 * 299, 17, 128 * 150 + 3]
    z = synth.make_queries_near_rows(E, rows, noise=0.3, seed=8)
    cb = eb.EmuCodebook(E)
    ik, _, _ = _check(cb, z, 8)
    assert ik[:, 0].tolist() == rows
    assert _oracle_swaps(ik, z, E, 8, GAP_TOL) == 0
    cb.close()


def test_more_lists_than_one_finisher_chunk():
    """> 768 blocks: the finisher carries its winners from one chunk of lists into the next -- best rows in both chunks, ties
    across the chunk boundary."""
    N = 128 * 800 + 3
    E = synth.make_codebook(N, 128, seed=7, planted_duplicates=0)
    rows = [128 * 2 + 1, 128 * 700, 128 * 767 + 127, 128 * 768, 128 * 768 + 1, 128 * 799 + 5, N - 1, 128 * 400]
    E, z = _cluster(E, rows, seed=3)
    E[128 * 790 + 9] = E[128 * 2 + 1]                   # a twin of a first-chunk row in the second chunk
    cb = eb.EmuCodebook(E)
    ik, _, _ = _check(cb, z, 8, orders=(2,), modes=(_lib.AAE_SCAN_AUTO, _lib.AAE_SCAN_AUTO_TOPK_ROWS))
    assert set(ik[0].tolist()) <= set(rows + [128 * 790 + 9])
    pos = ik[0].tolist()
    if 128 * 790 + 9 in pos:
        assert pos.index(128 * 2 + 1) + 1 == pos.index(128 * 790 + 9)
    cb.close()


def _nn_into(cb, z, k, ws, idx, score):
    L = eb.lib()
    z = np.ascontiguousarray(z, dtype=np.float32)
    n = L.aae_codebook_workspace_bytes(cb.h, z.shape[0], k)
    assert n <= len(ws)
    rc = L.aae_codebook_nn(cb.h, z.ctypes.data, z.shape[0], k, 1, idx.ctypes.data, score.ctypes.data, ws.ctypes.data, len(ws), None)
    _lib.check(L, rc, 'aae_codebook_nn')


@pytest.mark.parametrize('k', [3, 5, 8])
def test_nothing_written_beyond_row_B_or_column_k(k):
    E = synth.make_codebook(401, 128, seed=7, planted_duplicates=0)
    z = np.random.default_rng(1234).standard_normal((3, 128)).astype(np.float32)
    cb = eb.EmuCodebook(E)
    want_i, want_s = cb.nn(z, k)
    for mode in (_lib.AAE_SCAN_AUTO, _lib.AAE_SCAN_STREAM_2L):
        cb.set_mode(mode)
        idx = np.full((4, k), -7, dtype=np.int64)
        score = np.full((4, k), 123.5, dtype=np.float32)
        _nn_into(cb, z, k, eb._aligned(eb.lib().aae_codebook_workspace_bytes(cb.h, 3, k)), idx, score)
        assert np.array_equal(idx[:3], want_i) and np.array_equal(_bits(score[:3]), _bits(want_s))
        assert np.all(idx[3] == -7) and np.all(score[3] == 123.5)
    cb.close()


def test_one_workspace_reused_across_k_batch_and_codebook():
    L = eb.lib()
    E = synth.make_codebook(401, 128, seed=7, planted_duplicates=0)
    E2 = synth.make_codebook(259, 128, seed=8, planted_duplicates=0)
    z = np.random.default_rng(1234).standard_normal((4, 128)).astype(np.float32)
    cb, cb2 = eb.EmuCodebook(E), eb.EmuCodebook(E2)
    ws = eb._aligned(max(L.aae_codebook_workspace_bytes(c.h, B, k) for c in (cb, cb2) for B in (1, 4) for k in (1, 2, 5, 8)))   # arrives filled with junk
    for order in (0, 2):
        eb.set_block_order(order)
        for c, B, k in ((cb, 4, 8), (cb, 1, 2), (cb, 4, 1), (cb2, 3, 5)):
            idx = np.full((B, k), -7, dtype=np.int64)
            score = np.zeros((B, k), dtype=np.float32)
            _nn_into(c, z[:B], k, ws, idx, score)
            cs = c.similarity(z[:B])
            assert np.array_equal(idx, ref.topk_canonical(cs, k)), (order, B, k)
            assert np.array_equal(_bits(score), _bits(np.take_along_axis(cs, idx, axis=1))), (order, B, k)
    cb.close()
    cb2.close()


# ---- the fused call ---------------------------------------------------------------------------------------------------------
def _encode_nn_topk(enc, cb, x, k):
    L = eb.lib()
    x = np.ascontiguousarray(x)
    B = x.shape[0]
    dt = _lib.AAE_DTYPE_U8 if x.dtype == np.uint8 else _lib.AAE_DTYPE_F32
    n_e = L.aae_encoder_workspace_bytes(enc.h, B)
    n_c = L.aae_codebook_workspace_bytes(cb.h, B, k)
    enc.ws, ws_c = eb._aligned(n_e), eb._aligned(n_c)
    enc.B = B
    z = np.zeros((B, enc.cfg.latent_space_size), dtype=np.float32)
    idx = np.full((B, k), -7, dtype=np.int64)
    score = np.zeros((B, k), dtype=np.float32)
    rc = L.aae_encode_nn_topk(enc.h, cb.h, x.ctypes.data, dt, B, k, z.ctypes.data, idx.ctypes.data, score.ctypes.data,
                              enc.ws.ctypes.data, n_e, ws_c.ctypes.data, n_c, None)
    _lib.check(L, rc, 'aae_encode_nn_topk')
    return z, idx, score


@pytest.mark.parametrize('order', [0, 2])
@pytest.mark.parametrize('B', [1, 3, 6])
def test_fused_encode_nn_topk_equals_the_two_calls(B, order):
    """aae_encode_nn_topk: conv1's block 0 installs the nonce of the scan's ticket words too (ticket_prep 1), or the scan installs its
    own (0); forward + nn(topk) bit for bit either way.  B = 6: the two calls in one (query-resident scan)."""
    L = eb.lib()
    eb.set_block_order(order)
    cfg = EncoderConfig((16, 16, 3), [32, 64], [2, 2], 5, 128)
    w = synth.make_weights(seed=21, shape=cfg.shape, num_filter=cfg.num_filter, strides=cfg.strides, latent=128)
    x = synth.make_crops(B, seed=22, shape=cfg.shape)
    E = synth.make_codebook(36 * 11 + 5, 128, seed=7, planted_duplicates=11)
    enc, cb = eb.EmuEncoder(w, cfg), eb.EmuCodebook(E)
    z0 = enc.forward(x)
    for k in (8, 3):
        i0, s0 = cb.nn(z0, k)
        assert np.array_equal(i0, ref.topk_canonical(cb.similarity(z0), k))
        for chain in (0, 1):                              # (the persistent per-detection launch answers top-1 only: same six launches)
            enc.set_option('detect_chain', chain)
            for prep in (1, 0):
                enc.set_option('ticket_prep', prep)
                z1, i1, s1 = _encode_nn_topk(enc, cb, x, k)
                assert np.array_equal(z1, z0) and np.array_equal(i1, i0) and np.array_equal(_bits(s1), _bits(s0)), (k, chain, prep)
                if B <= 4:
                    assert L.aae_codebook_last_launches() == 1
        enc.set_option('detect_chain', 0)
        enc.set_option('ticket_prep', 1)
    z1, i1, s1 = _encode_nn_topk(enc, cb, x, 1)           # topk 1 is aae_encode_nn
    z2, i2, s2 = eb.encode_nn(enc, cb, x)
    assert np.array_equal(z1, z2) and np.array_equal(i1, i2) and np.array_equal(_bits(s1), _bits(s2))
    enc.close()
    cb.close()
