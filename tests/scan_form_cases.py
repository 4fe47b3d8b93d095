"""The launch forms of the codebook scan at ragged and tiny sizes: one table, run on the CPU fiber emulator
(tests/test_emu_scan_forms.py: the host branches, the inputs' gap condition, the launch counts) and on the MI355X
(tests/test_gpu_scan_forms.py: what the emulator cannot see -- the out-of-range part of an LDS-DMA tile, the raised dynamic-LDS
ceilings, the real MFMA paths, a 256-CU row-block split).

A case is (dtype, N, J, B, call, k, col_stride, upright_copy, mode, z_offset_floats) plus the number of kernel launches the
call must queue (aae_codebook_last_launches: the only evidence that the intended form ran) and a gpu_only tag.  run_case()
does all the checking through the small common surface of engine.CodebookEngine and emu_backend.EmuCodebook.

Row counts: the edges of every tile size the scan uses -- 64 rows (fp32 query-resident), 128 (fp32 with four waves per tile,
bf16, MFMA, fp32 stream), 256 (bf16 stream) -- and of the 2048-row top-k chunk.  The one sizeable book has 36 900 = 36 x 1025
rows.  On a 256-CU device plan_scan gives it, for fp32 and B <= 128, 193 row blocks of three 64-row tiles (577 tiles: the last
block has ONE tile, of 36 rows); with four waves per tile, and for bf16, 145 blocks of two 128-row tiles (289 tiles: the last
block has one tile of 36 rows); for B = 257, two query chunks x 116 blocks of five 64-row tiles (the last block has two).
(Not asserted: it depends on the CU count.)

Inputs per case: queries near chosen rows (synth.make_queries_near_rows, noise 0.3; chosen_rows() orders them: row N-1 in
EVERY case -- the builder asserts it is an answer -- then both sides of the last tile edge, the other edges, row 0, as far as
the batch reaches), one zero latent (every score 0: row 0, top-k 0 ... k-1) and queries that tie two planted
identical rows exactly (the lower row must win); on books of at most J / 2 + 1 rows also a latent that every row scores below
zero (a row past N, let through with the 0 of its tile's out-of-range part, would win; on larger books the positive scores
of the other queries hide such a row, so the row < N masks of later tiles rest on the N <= 65 cases alone).  Row indices and top-k lists are
compared EXACTLY with np.argmax / ref.topk_canonical of the fp64 similarity (identical rows given identical fp64 scores); that
is legitimate because build_inputs() asserts, for every query, that the fp64
scores of the oracle's top (k + 1) lie at least MIN_GAP = 1e-4 apart (for bf16 on the fp32 book and on the rounded one) -- far
above the fp32 rounding of a 128-term dot product (~1e-6) and the 3.8e-6 bound of the two-term bf16 queries
(codebook_scan_bf16.h).  The only gaps below that are exact zeros between bit-identical rows and the zero latent's, both
decided by the lowest-row rule.  The noise seed of each query is the first one (counting up from the case's) whose scores
satisfy the condition; the tie query is an exact power-of-two multiple of the planted row where that query's other scores
satisfy it, else the planted row plus noise (the two rows are identical: the tie is exact for any query)."""
import collections
import ctypes
import functools

import numpy as np

from augmentedautoencoder_amd import _lib
from augmentedautoencoder_amd.weights import to_bf16_bits
from oracle import reference_cpu as ref
from oracle import synth

COS_TOL = 1e-5           # tests/test_gpu_parity.py's own bound on |cosine - fp64 oracle|
MIN_GAP = 1e-4           # least fp64 distance between consecutive scores of the oracle's top (k + 1)
BIG = 36900              # 36 x 1025
LADDER_N = 10243         # six 2048-row top-k chunks; carries the graded rows of the k = 400 case

A = _lib.AAE_SCAN_AUTO
MFMA = _lib.AAE_SCAN_MFMA
STREAM = _lib.AAE_SCAN_STREAM
STREAM_2L = _lib.AAE_SCAN_STREAM_2L
NO_PRUNE = _lib.AAE_SCAN_AUTO_NO_PRUNE
PACKED = _lib.AAE_SCAN_AUTO_PACKED
RH2 = _lib.AAE_SCAN_AUTO_RH2
FIN = _lib.AAE_SCAN_AUTO_FIN
TOPK_ROWS = _lib.AAE_SCAN_AUTO_TOPK_ROWS
MODE_NAMES = {A: 'auto', MFMA: 'mfma', STREAM: 'stream', STREAM_2L: 'stream2l', NO_PRUNE: 'noprune', PACKED: 'packed', RH2: 'rh2',
              FIN: 'fin', TOPK_ROWS: 'topkrows'}

Case = collections.namedtuple('Case', 'dtype N J B call k col_stride upright_copy mode z_offset_floats launches gpu_only')


def case_id(c):
    call = 'sim' if c.call == 'similarity' else 'k%d' % c.k
    up = '' if c.col_stride == 1 else ('-upcopy%d' % c.col_stride if c.upright_copy else '-upmask%d' % c.col_stride)
    return '%s-N%d-J%d-B%d-%s%s-%s%s' % (c.dtype, c.N, c.J, c.B, call, up, MODE_NAMES[c.mode], '-zoff%d' % c.z_offset_floats if c.z_offset_floats else '')


def _nn(dtype, N, B, launches, k=1, mode=A, J=128, stride=1, copy=False, zoff=0, gpu_only=False):
    return Case(dtype, N, J, B, 'nn', k, stride, copy, mode, zoff, launches, gpu_only)


def _sim(dtype, N, B, launches, mode=A, J=128, gpu_only=False):
    return Case(dtype, N, J, B, 'similarity', 1, 1, False, mode, 0, launches, gpu_only)


def cases():
    """Launch counts as read from plan_scan / run_scan / nn_impl (aae_codebook_scan.h, aae_abi_impl.h); similarity() does not
    reset the counter, its number is the increase over the call.  gpu_only: more than about ten seconds on the emulator
    (other cases of the same form confirm the count there), or a read the emulator's host cannot do."""
    out = []
    f, h = 'f32', 'bf16'
    # ---- fp32, J = 128, B <= 4: the stream kernel (128 rows per block), answers inside the launch
    for N in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2049):
        out += [_nn(f, N, 1, 1), _nn(f, N, 4, 1)]
    out += [_nn(f, N, B, 1) for N in (129, 257) for B in (2, 3)]
    out += [_nn(f, 129, 4, 1, mode=STREAM), _nn(f, 129, 3, 2, mode=STREAM_2L), _nn(f, 1, 1, 2, mode=STREAM_2L)]     # 2L: scan + argmax_reduce
    # top-k 2 ... 8 in the stream scan: sorted lists per block, merged by the last block to arrive
    out += [_nn(f, 8, 2, 1, k=8), _nn(f, 65, 1, 1, k=2), _nn(f, 129, 3, 1, k=3), _nn(f, 129, 4, 1, k=5), _nn(f, 257, 4, 1, k=8), _nn(f, 2049, 1, 1, k=5)]
    out += [_nn(f, 129, 2, 2, k=5, mode=STREAM_2L), _nn(f, 257, 4, 2, k=2, mode=STREAM_2L)]                            # scan + merge launch
    out += [_nn(f, 129, 3, 3, k=8, mode=TOPK_ROWS), _nn(f, 2049, 4, 3, k=3, mode=TOPK_ROWS)]                          # scan with similarity rows + chunks + merge
    # k > 8 at B <= 4: stream scan with similarity rows + two-level selection, on books smaller than one chunk and of two
    out += [_nn(f, 129, 3, 3, k=9), _nn(f, 257, 1, 3, k=60), _nn(f, 2049, 4, 3, k=9)]
    out += [_nn(f, 129, 3, 3, mode=MFMA), _nn(f, 129, 3, 4, k=5, mode=MFMA)]                                           # l2norm + MFMA + reduce / + chunks + merge
    # ---- fp32, J = 128, B > 4 arg-max: the query-resident kernel normalises its queries, argmax_reduce behind it
    for i, N in enumerate((1, 8, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2049, BIG)):
        out.append(_nn(f, N, (5, 32)[i % 2], 2))                     # four waves per 128-row tile
    out += [_nn(f, N, B, 2) for N, B in ((127, 5), (128, 32), (129, 5), (64, 5), (BIG, 32))]
    for i, N in enumerate((1, 63, 64, 65, 127, 128, 129, 257, BIG)):
        out.append(_nn(f, N, (33, 70, 128)[i % 3], 2))               # two waves per 64-row tile (70: padded to 128, last query group partly filled)
    out += [_nn(f, 65, 128, 2), _nn(f, 129, 70, 2), _nn(f, BIG, 70, 2)]
    for i, N in enumerate((1, 63, 64, 65, 129, 257, BIG)):
        out.append(_nn(f, N, (129, 256)[i % 2], 2))                  # one wave per tile, 256 queries per block
    out += [_nn(f, N, 257, 2) for N in (1, 65, 129, BIG)]            # a second grid column of query chunks
    out += [_nn(f, 129, 5, 3, mode=PACKED), _nn(f, 65, 32, 3, mode=PACKED), _nn(f, 257, 129, 3, mode=PACKED)]        # l2norm_pack in front
    out += [_nn(f, 129, 5, 2, mode=RH2), _nn(f, 65, 32, 2, mode=RH2), _nn(f, 1, 5, 2, mode=RH2)]
    out += [_nn(f, 129, 5, 1, mode=FIN), _nn(f, 257, 32, 1, mode=FIN), _nn(f, BIG, 32, 1, mode=FIN)]                  # the last row block answers
    out += [_nn(f, 129, 257, 2, mode=FIN)]                           # (two grid columns: argmax_reduce stays)
    out += [_nn(f, 129, 5, 3, mode=MFMA), _nn(f, 65, 70, 3, mode=MFMA)]
    # top-k 2 ... 8 inside the query-resident scan: l2norm_pack + scan + topk_merge
    out += [_nn(f, 8, 5, 3, k=8), _nn(f, 65, 32, 3, k=2), _nn(f, 129, 33, 3, k=3), _nn(f, 129, 129, 3, k=5), _nn(f, 257, 70, 3, k=8),
            _nn(f, 64, 256, 3, k=5, gpu_only=True), _nn(f, 128, 257, 3, k=2), _nn(f, 2049, 5, 3, k=5), _nn(f, BIG, 128, 3, k=8), _nn(f, BIG, 257, 3, k=3)]
    out += [_nn(f, 129, 33, 3, k=5, mode=NO_PRUNE), _nn(f, BIG, 5, 3, k=8, mode=NO_PRUNE), _nn(f, 129, 33, 4, k=5, mode=MFMA)]
    # k > 8 at B > 4: l2norm_pack + MFMA with the similarity matrix + topk_chunks + topk_merge
    out += [_nn(f, 129, 5, 4, k=9), _nn(f, 257, 33, 4, k=60, gpu_only=True), _nn(f, 65, 33, 4, k=60, gpu_only=True), _nn(f, 65, 5, 4, k=60), _nn(f, 65, 129, 4, k=60, gpu_only=True), _nn(f, 2049, 257, 4, k=9, gpu_only=True)]
    # 6 chunks x 400 > 2048 candidates: topk_merge_kernel<false>
    out += [_nn(f, LADDER_N, 5, 4, k=400), _nn(f, LADDER_N, 2, 3, k=400), _nn(f, LADDER_N, 33, 3, k=8), _nn(f, LADDER_N, 4, 1, k=8)]
    # ---- similarity(): the stream kernel (B <= 4) or l2norm_pack + the tile-resident MFMA kernel, N % 4 != 0
    out += [_sim(f, 401, B, 1) for B in (1, 3, 4)] + [_sim(f, 401, B, 2) for B in (5, 33, 70, 129, 257)]
    out += [_sim(f, 1, 5, 2), _sim(f, BIG, 70, 2), _sim(f, 401, 3, 2, mode=MFMA)]
    # ---- upright, col_stride 36, before prepare_upright: masked, the tile-resident kernels at every B
    out += [_nn(f, N, B, 3, stride=36) for N, B in ((36, 1), (36, 5), (125, 4), (125, 33), (269, 2), (269, 5), (269, 129), (BIG, 5))]
    # ... and after: an ordinary scan of the ceil(N / 36) rows of the compacted copy (N = 36 m + 17: the last one exists only if the division rounds up)
    out += [_nn(f, 36, 1, 1, stride=36, copy=True), _nn(f, 36, 5, 2, stride=36, copy=True), _nn(f, 125, 4, 1, stride=36, copy=True),
            _nn(f, 125, 33, 2, stride=36, copy=True), _nn(f, 269, 5, 2, stride=36, copy=True), _nn(f, BIG, 1, 1, stride=36, copy=True),
            _nn(f, BIG, 70, 2, stride=36, copy=True), _nn(f, BIG, 257, 2, stride=36, copy=True)]
    # ---- bf16 (J = 128): 256 rows per stream block (no NQ = 3: three queries run as four), 128-row tiles elsewhere
    out += [_nn(h, N, B, 1) for N, B in ((1, 1), (129, 2), (255, 4), (256, 1), (257, 3), (257, 4))]
    out += [_nn(h, 257, 4, 1, k=5), _nn(h, 8, 2, 1, k=8), _nn(h, 257, 2, 2, mode=STREAM_2L), _nn(h, 257, 1, 3, k=3, mode=TOPK_ROWS), _nn(h, 257, 2, 3, k=9)]
    for i, N in enumerate((1, 127, 128, 129, 257, BIG)):
        out.append(_nn(h, N, (5, 32)[i % 2], 2))
    out += [_nn(h, 129, 33, 2), _nn(h, BIG, 70, 2), _nn(h, 128, 128, 2), _nn(h, 128, 129, 2), _nn(h, 257, 256, 2), _nn(h, 129, 257, 2), _nn(h, BIG, 257, 2)]
    out += [_nn(h, 129, 5, 3, k=5), _nn(h, 257, 70, 3, k=8), _nn(h, BIG, 129, 3, k=2), _nn(h, 129, 5, 4, k=9)]
    out += [_nn(h, 129, 5, 3, mode=PACKED), _nn(h, 129, 32, 1, mode=FIN), _nn(h, 129, 5, 3, mode=MFMA), _nn(h, 129, 5, 2, mode=RH2)]
    out += [_sim(h, 401, 2, 1), _sim(h, 401, 5, 2), _sim(h, 401, 70, 2)]
    out += [_nn(h, 269, 5, 3, stride=36), _nn(h, 269, 5, 2, stride=36, copy=True), _nn(h, 269, 2, 1, stride=36, copy=True)]
    # ---- narrow latents (fp32): the padded-J branches of the stream kernels, the MFMA kernel and l2norm_pack; J < 128 at B > 4 has
    # no query-resident form: l2norm_pack + MFMA + argmax_reduce
    for J in (4, 64, 124):
        out += [_nn(f, N, B, 1 if B <= 4 else 3, J=J) for N, B in ((1, 1), (1, 5), (65, 3), (65, 33), (129, 4), (129, 70), (401, 1), (401, 5))]
        out += [_nn(f, 65, 4, 1, k=5, J=J), _nn(f, 401, 3, 1, k=5, J=J), _nn(f, 129, 5, 4, k=5, J=J), _nn(f, 401, 33, 4, k=5, J=J)]
        out += [_nn(f, 65, 1, 3, k=9, J=J), _nn(f, 129, 33, 4, k=9, J=J), _nn(f, 401, 70, 4, k=9, J=J)]
        out += [_sim(f, 129, 3, 1, J=J), _sim(f, 401, 5, 2, J=J), _sim(f, 65, 70, 2, J=J)]
        out += [_nn(f, 65, 1, 3, J=J, stride=36), _nn(f, 129, 5, 3, J=J, stride=36), _nn(f, 401, 33, 3, J=J, stride=36)]
        out += [_nn(f, 129, 4, 1, J=J, stride=36, copy=True), _nn(f, 401, 70, 3, J=J, stride=36, copy=True)]
    # ---- z one float into a larger buffer (4-byte aligned): the stream kernels read it as it is; the query-resident arg-max
    # falls back from its fused-norm prologue to l2norm_pack in front -- AUTO_PACKED's three launches, the aligned call's bits
    # (the stream cases on the GPU only: the emulator's host compiler turns the kernels' f32x4 reads of z into aligned x86 loads)
    out += [_nn(f, 129, 1, 1, zoff=1, gpu_only=True), _nn(f, 129, 4, 1, zoff=1, gpu_only=True), _nn(f, 129, 9, 3, zoff=1), _nn(f, 129, 130, 3, zoff=1), _nn(f, BIG, 9, 3, zoff=1),
            _nn(h, 129, 9, 3, zoff=1)]
    # the two large books take the emulator 15 s to 4 min per batched case (each passed there once, with these launch counts)
    out = [c._replace(gpu_only=c.gpu_only or (c.N in (BIG, LADDER_N) and c.B > 4) or (c.N == LADDER_N and c.k > 8)) for c in out]
    ids = [case_id(c) for c in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out


# ---- books ---------------------------------------------------------------------------------------------------------------------
def bf16_rounded(E):
    return (to_bf16_bits(np.ascontiguousarray(E, dtype=np.float32)).astype(np.uint32) << 16).view(np.float32)


def twin_pairs(N):
    """(lower, higher) rows planted identical: in one tile, in different tiles, in different row blocks (36 900), on multiples of
    36 (what an upright query can see; never the last multiple of 36 below N -- the row a compacted copy has only if
    ceil(N / 36) rounds up must answer for itself)"""
    pairs = [p for p in ((3, 40), (10, 70), (20, 200), (36, 72), (108, 216), (100, 30000), (144, 36000)) if p[1] < N]
    return pairs


def chosen_rows(N, step=1):
    """The rows the near-row queries of a case aim at, most wanted first: the last row (upright: the last visible one), both sides
    of the book's last edge of a 64-, 128- and 256-row tile, the named rows of the large books, both sides of every earlier tile
    and chunk edge, row 0.  A case takes as many of them as it has queries left (build_inputs)."""
    edges = sorted({e - d for T in (64, 128, 256) for e in [(N - 1) // T * T] if e > 0 for d in (0, 1)}, reverse=True)
    rows = [N - 1] + edges
    if N == BIG:
        rows += [BIG - 20, 18600]            # in the final 36 rows; in the last full tile of a middle row block (tile 290 of 577)
    if N == LADDER_N:
        rows += [8192, 8191]                 # both sides of a top-k chunk edge
    rows += [r for r in (2048, 2047, 256, 255, 128, 127, 64, 63) if r < N - 1] + [0]
    taken = set(r for p in twin_pairs(N) for r in p)
    rows = [r for r in dict.fromkeys(rows) if r not in taken and 0 <= r < N]
    if step > 1:                              # what an upright query can see
        rows = [r for r in dict.fromkeys([step * ((N - 1) // step)] + [r - r % step for r in rows]) if r not in taken]
    return rows


LADDER_ROWS = 460
LADDER_TWIN = (159, 4000)                    # ladder row 7 again in the second 2048-row chunk


def _ladder(E, seed=77):
    """460 rows (every 22nd, all six chunks) with cosines 0.97, 0.97 - 2.5e-4, ... (in scrambled row order) to one direction u,
    their other component orthogonal to u and to a second direction w: a query in the (u, w) plane at an angle phi to u scores
    cos(phi) x the ladder -- 400 best scores >= 2.3e-4 apart.  The LAST row (in the book's 3-row final tile) is the rung above them
    all, 0.985: it heads every such query's list.  Returns (E', u, w)."""
    rng = np.random.default_rng(seed)
    J = E.shape[1]
    u = rng.standard_normal(J)
    u /= np.linalg.norm(u)
    w = rng.standard_normal(J)
    w -= (w @ u) * u
    w /= np.linalg.norm(w)
    steps = rng.permutation(LADDER_ROWS)
    E = E.astype(np.float64)
    for i in range(LADDER_ROWS):
        v = rng.standard_normal(J)
        v -= (v @ u) * u + (v @ w) * w
        v /= np.linalg.norm(v)
        c = 0.97 - 2.5e-4 * steps[i]
        E[5 + 22 * i] = c * u + np.sqrt(1.0 - c * c) * v
    v = rng.standard_normal(J)
    v -= (v @ u) * u + (v @ w) * w
    E[-1] = 0.985 * u + np.sqrt(1.0 - 0.985 ** 2) * v / np.linalg.norm(v)
    E[LADDER_TWIN[1]] = E[LADDER_TWIN[0]]
    return E.astype(np.float32), u, w


@functools.lru_cache(maxsize=None)
def book(N, J, ladder=False):
    """fp32 rows of the (N, J) book (a bf16 engine rounds them itself); ladder: the 10 243-row book of the k > 8 cases"""
    E = synth.make_codebook(N, J, seed=1000 + N + J, planted_duplicates=0)
    for lo, hi in twin_pairs(N):
        E[hi] = E[lo]
    if ladder:
        E = _ladder(E)[0]
    E.setflags(write=False)
    return E


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _gaps_ok(s, k, E, zero=False):
    """s: fp64 scores of one query against the rows the call can answer with.  The top (k + 1) at least MIN_GAP apart, except
    exact ties of bit-identical rows (and the zero latent, whose scores are all 0)."""
    if zero:
        return bool(np.all(s == 0.0))
    n = min(k + 1, len(s))
    order = np.lexsort((np.arange(len(s)), -s))[:n]
    d = s[order[:-1]] - s[order[1:]]
    for j in np.nonzero(d < MIN_GAP)[0]:
        if not (d[j] == 0.0 and np.array_equal(E[order[j]], E[order[j + 1]])):
            return False
    return True


Inputs = collections.namedtuple('Inputs', 'E z cs64 want kinds ladder')


@functools.lru_cache(maxsize=4)         # (the [257, 36 900] fp64 oracle is 76 MB)
def build_inputs(dtype, N, J, B, k, col_stride):
    """Queries of a case and their fp64 answers.  cs64 [B, N] is the oracle's similarity (bf16: against the rounded book), want
    [B, k] the rows the call must return."""
    ladder = N == LADDER_N and J == 128 and k > 8
    E = book(N, J, ladder)
    books = [E.astype(np.float64)] + ([bf16_rounded(E).astype(np.float64)] if dtype == 'bf16' else [])
    oracle_book = books[-1]
    step = col_stride
    Evis = E[::step]
    twins = twin_pairs(N) + ([LADDER_TWIN] if ladder else [])

    def scores(zq, book64):
        """ref.cos_similarity; identical rows get identical scores (a BLAS product does not promise that: its last bits depend
        on where a row sits)"""
        s = ref.cos_similarity(zq, book64)
        for lo, hi in twins:
            s[:, hi] = s[:, lo]
        return s
    pairs = [p for p in twin_pairs(N) if p[0] % step == 0 and p[1] % step == 0]
    rows = chosen_rows(N, step)
    base_seed = 7919 * N + 131 * J + 17 * B + 3 * k + col_stride

    def ok(zq, zero=False):
        return all(_gaps_ok(scores(zq[None], b64)[0, ::step], k, Evis, zero) for b64 in books)

    def near(row, slot):
        for attempt in range(4000):
            zq = synth.make_queries_near_rows(E, [row], noise=0.3, seed=base_seed + 10007 * slot + attempt)[0]
            if ok(zq) and int(np.argmax(scores(zq[None], oracle_book)[0, ::step])) * step == row:     # (J = 4: the noise can carry it to a neighbour)
                return zq
        raise AssertionError('no query near row %d of the [%d, %d] book keeps its top %d scores %.0e apart' % (row, N, J, k + 1, MIN_GAP))

    def anti(slot):
        """a latent that EVERY row scores below zero (graded, -0.3 ... -0.6 before normalising): the best real score is
        negative, so a row past N that a kernel let through with the 0 of its out-of-range tile part would win"""
        for attempt in range(200):
            rng = np.random.default_rng(base_seed + 10007 * slot + attempt)
            t = -(0.3 + 0.3 * rng.permutation(N) / N)
            for lo, hi in twins:
                t[hi] = t[lo]
            zq = (np.linalg.lstsq(books[0], t, rcond=None)[0] * rng.uniform(0.5, 20.0)).astype(np.float32)
            if ok(zq) and all(scores(zq[None], b64).max() < -1e-3 for b64 in books):
                return zq
        raise AssertionError('no latent below every row of the [%d, %d] book' % (N, J))

    # who gets a query, most wanted first: the last row ALWAYS, then the below-zero latent (books of few enough rows to be nearly
    # orthogonal: the least-squares latent exists), one planted tie, the zero latent, both sides of the last tile edge, the other
    # ties, the remaining chosen rows (round and round)
    small = N <= J // 2 + 1
    plan = [('near', rows[0])] if N > 1 or B > 1 or not small else []
    plan += [('anti', None)] if small else []
    first_tie = pairs[(B + k) % len(pairs)] if pairs else None
    plan += [('tie', first_tie)] if pairs else []
    plan += [('zero', None)]
    plan += [('near', r) for r in rows[1:3]]
    plan += [('tie', p) for p in pairs if p != first_tie][:3]
    rest = rows[3:] + rows[:3]
    plan += [('near', rest[i % len(rest)]) for i in range(max(0, B - len(plan)))]
    plan = plan[:B]
    if ladder:                                  # in the (u, w) plane of the book's graded rows: LADDER_TWIN's exact tie among them, the last row on top
        _, u, w = _ladder(synth.make_codebook(N, J, seed=1000 + N + J, planted_duplicates=0))
        plan = [('zero', None) if (b == 1 and B >= 3) else ('ladder', None) for b in range(B)]
    z = np.zeros((B, J), dtype=np.float32)
    kinds, ties = [], {}
    for b, (kind, what) in enumerate(plan):
        kinds.append(kind)
        if kind == 'anti':
            z[b] = anti(b)
        elif kind == 'ladder':
            phi = 0.05 + 0.04 * (b % 6)
            z[b] = (2.0 ** (b % 5 - 1) * (np.cos(phi) * u + np.sin(phi) * w)).astype(np.float32)
        elif kind == 'tie':
            ties[b] = what
            z[b] = E[what[0]] * np.float32(2.0 ** (1 + b % 3))   # exact multiple: both rows score the same bits
            if not ok(z[b]):
                z[b] = near(what[0], b)
        elif kind == 'near':
            z[b] = near(what, b)
    for b in range(B):
        assert ok(z[b], kinds[b] == 'zero'), (dtype, N, J, B, k, col_stride, b, kinds[b])
    cs64 = scores(z, oracle_book)
    if step > 1:
        want = (np.argmax(cs64[:, ::step], axis=1) * step)[:, None]
    else:
        want = ref.topk_canonical(cs64, k)
    for b, (lo, hi) in ties.items():
        assert want[b, 0] == lo and (k == 1 or want[b, 1] == hi), (b, want[b])
    if N > 1 or B > 1:                          # the last row the call can answer with IS an answer, of every case
        assert rows[0] == step * ((N - 1) // step) and rows[0] in want[:, 0], (dtype, N, J, B, k, col_stride, want[:, 0])
    for b, (kind, what) in enumerate(plan):
        assert kind != 'near' or want[b, 0] == what, (b, what, want[b])
    if ladder:                                  # the twins next to each other, the lower row first, in every non-zero query's list
        for b in range(B):
            if kinds[b] == 'ladder':
                at = want[b].tolist()
                assert at.index(LADDER_TWIN[0]) + 1 == at.index(LADDER_TWIN[1]), b
    return Inputs(E, z, cs64, want, tuple(kinds), ladder)


# ---- the adapter over CodebookEngine / EmuCodebook -----------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Engine(object):
    """nn / similarity on host arrays in and out, scan mode, upright preparation and the launch counter of either engine"""

    def __init__(self, raw):
        self.raw = raw
        self.gpu = hasattr(raw, 'set_scan_mode')
        self.lib = raw.lib if self.gpu else raw.L

    def set_mode(self, mode):
        (self.raw.set_scan_mode if self.gpu else self.raw.set_mode)(mode)

    def prepare_upright(self, col_stride):
        (self.raw.ensure_upright if self.gpu else self.raw.prepare_upright)(col_stride)

    def launches(self):
        return self.lib.aae_codebook_last_launches()

    def _place(self, z, offset_floats):
        """z as the engine takes it; offset_floats > 0: a contiguous [B, J] view that starts that many floats into a larger buffer"""
        z = np.ascontiguousarray(z, dtype=np.float32)
        if self.gpu:
            import torch
            if not offset_floats:
                return torch.from_numpy(z).to(self.raw.device)
            buf = torch.zeros(z.size + offset_floats + 8, dtype=torch.float32, device=self.raw.device)
            view = buf[offset_floats:offset_floats + z.size].view(z.shape)
            view.copy_(torch.from_numpy(z))
            assert view.data_ptr() % 16 == (4 * offset_floats) % 16 and view.is_contiguous()
            return view
        if not offset_floats:
            return z
        buf = np.zeros(z.size + offset_floats + 8, dtype=np.float32)
        at = (-buf.ctypes.data % 16) // 4 + offset_floats
        view = buf[at:at + z.size].reshape(z.shape)
        view[...] = z
        assert view.ctypes.data % 16 == (4 * offset_floats) % 16
        return view

    def _masked_nn(self, z, col_stride):
        """CodebookEngine.nn prepares the compacted copy on the first upright call: the masked form is the C call on its own"""
        import torch
        from augmentedautoencoder_amd import engine as eng
        raw = self.raw
        B = z.shape[0]
        idx = torch.empty((B, 1), dtype=torch.int64, device=raw.device)
        score = torch.empty((B, 1), dtype=torch.float32, device=raw.device)
        nbytes = raw.workspace_bytes(B, 1)
        _, ws_ptr = raw.ws.get(nbytes)
        with eng._on_device(raw.device):
            rc = raw.lib.aae_codebook_nn(raw.handle, ctypes.c_void_p(z.data_ptr()), B, 1, int(col_stride), ctypes.c_void_p(idx.data_ptr()),
                                         ctypes.c_void_p(score.data_ptr()), ctypes.c_void_p(ws_ptr), nbytes, eng._stream_ptr(torch))
        _lib.check(raw.lib, rc, 'aae_codebook_nn')
        return idx, score

    def nn(self, z, k=1, col_stride=1, masked=False, offset_floats=0):
        """(rows int64 [B, k], scores float32 [B, k], launches of the call)"""
        zz = self._place(z, offset_floats)
        if self.gpu and masked:
            idx, score = self._masked_nn(zz, col_stride)
        else:
            idx, score = self.raw.nn(zz, k, col_stride)
        n = self.launches()
        if self.gpu:
            idx, score = idx.cpu().numpy(), score.cpu().numpy()
        return idx, score, n

    def similarity(self, z):
        """(float32 [B, N], launches of the call: the counter is not reset by similarity())"""
        before = self.launches()
        cs = self.raw.similarity(self._place(z, 0))
        n = self.launches() - before
        return (cs.cpu().numpy() if self.gpu else cs), n


def _selection(cs, k, col_stride):
    if col_stride > 1:
        return (np.argmax(cs[:, ::col_stride], axis=1) * col_stride)[:, None]
    return ref.topk_canonical(cs, k)


def run_case(case, make_codebook_engine):
    """make_codebook_engine(E, dtype, key) -> a CodebookEngine / EmuCodebook on the rows E (the caller may hand out one engine
    per key and closes them).  Returns the largest |cosine - fp64 oracle| the case saw."""
    c = case
    inp = build_inputs(c.dtype, c.N, c.J, c.B, c.k, c.col_stride)
    eng = Engine(make_codebook_engine(inp.E, c.dtype, (c.dtype, c.N, c.J, c.upright_copy, inp.ladder)))
    masked = c.col_stride > 1 and not c.upright_copy
    if c.upright_copy:
        eng.prepare_upright(c.col_stride)
    # B <= 4 on a stream kernel: the products are added in another order than on the matrix cores -- the rows must equal the
    # ones under AAE_SCAN_MFMA, the scores are held to the oracle on both sides; everywhere else the scores agree bit for bit
    stream = c.B <= 4 and not masked and c.mode != MFMA
    try:
        eng.set_mode(MFMA if (masked and c.B <= 4) else c.mode)
        cs, n_sim = eng.similarity(inp.z)                               # the library's own similarity at this B, by the kernel family of the call
        assert cs.shape == (c.B, c.N) and np.all(np.isfinite(cs))
        err = float(np.abs(cs - inp.cs64).max())
        assert err <= COS_TOL, ('similarity', err)
        if c.call == 'similarity':
            assert n_sim == c.launches, ('launches', n_sim, c.launches)
            assert np.array_equal(np.argmax(cs, axis=1), np.argmax(inp.cs64, axis=1))
            for b in range(c.B):
                if inp.kinds[b] == 'zero':
                    assert np.all(cs[b] == 0.0), b
            eng.set_mode(MFMA)
            cs_t, _ = eng.similarity(inp.z)
            assert float(np.abs(cs_t - inp.cs64).max()) <= COS_TOL
            assert np.array_equal(np.argmax(cs, axis=1), np.argmax(cs_t, axis=1))
            assert stream or np.array_equal(_bits(cs), _bits(cs_t)), 'similarity differs from the one under AAE_SCAN_MFMA'
            return err
        eng.set_mode(c.mode)
        idx, score, n = eng.nn(inp.z, c.k, c.col_stride, masked, c.z_offset_floats)
        assert n == c.launches, ('launches', n, c.launches)
        assert idx.shape == (c.B, c.k) and score.shape == (c.B, c.k)
        assert idx.min() >= 0 and idx.max() < c.N, (idx.min(), idx.max())
        assert np.array_equal(idx, inp.want), ('rows', np.argwhere(idx != inp.want)[:4].tolist(), idx[idx != inp.want][:4], inp.want[idx != inp.want][:4])
        serr = float(np.abs(score - np.take_along_axis(inp.cs64, idx, axis=1)).max())
        err = max(err, serr)
        assert serr <= COS_TOL, ('scores', serr)
        assert np.all(score[:, :-1] >= score[:, 1:])
        for b in range(c.B):
            assert len(set(idx[b].tolist())) == c.k, (b, idx[b])
            if inp.kinds[b] == 'zero':
                assert idx[b].tolist() == list(range(c.k)) and np.all(score[b] == 0.0), (b, idx[b], score[b])
        # the selection over the library's own similarity at this B, bit for bit
        sel = _selection(cs, c.k, c.col_stride)
        assert np.array_equal(idx, sel), 'rows differ from the selection over similarity()'
        assert np.array_equal(_bits(score), _bits(np.take_along_axis(cs, idx, axis=1))), 'scores differ from similarity()'
        if c.z_offset_floats:                                            # the aligned call: the same bits
            i_a, s_a, _ = eng.nn(inp.z, c.k, c.col_stride, masked, 0)
            assert np.array_equal(idx, i_a) and np.array_equal(_bits(score), _bits(s_a)), 'differs from the aligned call'
        eng.set_mode(MFMA)
        i_t, s_t, _ = eng.nn(inp.z, c.k, c.col_stride, masked, 0)
        assert np.array_equal(idx, i_t), 'rows differ from AAE_SCAN_MFMA'
        assert float(np.abs(s_t - np.take_along_axis(inp.cs64, i_t, axis=1)).max()) <= COS_TOL
        assert stream or np.array_equal(_bits(score), _bits(s_t)), 'scores differ from AAE_SCAN_MFMA'
        return err
    finally:
        eng.set_mode(A)


def check_narrow_bf16_refused(make_codebook_engine):
    """bf16 rows are built for J == 128 only: the create call keeps refusing every other latent size"""
    for J in (4, 64, 124):
        try:
            raw = make_codebook_engine(book(65, J), 'bf16', None)
        except (RuntimeError, ValueError) as e:
            assert 'the bf16 scan kernel is built for J == 128' in str(e), str(e)
        else:
            raw.close()
            raise AssertionError('a bf16 codebook with J = %d was accepted' % J)
