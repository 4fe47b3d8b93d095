"""Every launch form of the grouped multi-object query on the MI355X, on nets small enough to reach each branch in milliseconds: the hardware twins of the
emulator cases of tests/test_emu_multi.py (shared constants: tests/multi_form_cases.py).  The emulator compiles the host branches of the Winograd layer kernel; here
the device branches run -- MFMA fragment layouts, LDS-DMA fills, the XCD block map, the dynamically indexed per-object table in the argument segment, ticket hand-offs
between blocks that really run side by side.  Per case: the launch count the CPU run pins (same host code, same options), the twin's bit-equalities and "not bit-equal"
claims, every latent within 5e-6 of the fp64 oracle of ITS object (a table builder that hands object o the pointers of object o' fails there), tie-aware indices."""
import numpy as np
import pytest

import multi_form_cases as mfc
import parity_report as report
from oracle import reference_cpu as ref
from test_gpu_parity import _check_indices

pytestmark = pytest.mark.gpu

ORACLE_TOL = 5e-6          # latent against the fp64 oracle, of the oracle's maximum (test_gpu_winograd.py: the three-layer net with batch norm)


class _Case(object):
    """the engines of a case, the crops on the device and every object's fp64 oracle (computed once)"""

    def __init__(self, case):
        import torch
        c = mfc.CASES[case]
        self.name, self.cfg, self.counts, self.launches = case, mfc.config(case), c['counts'], c['launches']
        self.dev = torch.device('cuda', 0)
        self.weights, self.books, self.objs = [], [], []
        for seed, rows in zip(c['weight_seeds'], c['codebook_rows']):
            self.add(seed, rows, c['options'])
        self.host = mfc.crops(case)
        self.x = torch.from_numpy(self.host).to(self.dev)
        self.oracle = self.oracle_of(list(range(len(self.counts))), self.counts, self.host)

    def add(self, seed, rows, options):
        from augmentedautoencoder_amd.engine import CodebookEngine, EncoderEngine
        w = mfc.weights(self.cfg, seed)
        E = mfc.codebook(self.cfg, seed, rows)
        enc = EncoderEngine(self.cfg, w, max_batch=64)
        for k, v in options.items():
            enc.set_option(k, v)
        self.weights.append(w), self.books.append(E), self.objs.append((enc, CodebookEngine(E)))
        return len(self.objs) - 1

    def oracle_of(self, who, counts, host):
        out = []
        for o, sl in zip(who, mfc.slices(counts)):
            z64 = ref.encoder_forward_torch(ref.input_to_float(host[sl]), self.weights[o], self.cfg.strides, self.cfg.batch_norm, 'float64')
            out.append((z64, ref.cos_similarity(z64, self.books[o])))
        return out

    def items(self):
        return [(e, c, n) for (e, c), n in zip(self.objs, self.counts)]

    def set_option(self, name, value):
        for e, _ in self.objs:
            e.set_option(name, value)

    def close(self):
        for e, c in self.objs:
            e.close()
            c.close()


def _per_object(items, x):
    import torch
    zs, idxs, scores, at = [], [], [], 0
    for e, c, n in items:
        z, i, s = e.encode_nn(c, x[at:at + n], 1)
        zs.append(z.clone()), idxs.append(i[:, 0].clone()), scores.append(s[:, 0].clone())
        at += n
    return torch.cat(zs), torch.cat(idxs), torch.cat(scores)


def _multi(items, x):
    import torch
    from augmentedautoencoder_amd.engine import MultiObjectQuery
    mq = MultiObjectQuery(items)
    z, i, s = [t.clone() for t in mq(x)]
    torch.cuda.synchronize()
    return z, i, s, mq.launches


def _same(a, b):
    import torch
    return all(torch.equal(u, v) for u, v in zip(a[:3], b[:3]))


def _rel(z, want):
    """largest difference of two latent arrays, of the second one's maximum"""
    return float((z - want).abs().max() / want.abs().max())


def _against_oracle(case, oracle, counts, z, idx, tag):
    """every object's rows against ITS fp64 oracle; returns the largest latent error"""
    worst = 0.0
    zh, ih = z.cpu().numpy(), idx.cpu().numpy()
    for o, (sl, (z64, cs64)) in enumerate(zip(mfc.slices(counts), oracle)):
        err = float(np.abs(zh[sl] - z64).max() / np.abs(z64).max())
        print('%s (%s): object %d (%d crops) latent vs fp64 %.3e' % (case, tag, o, counts[o], err))
        assert err < ORACLE_TOL, (case, tag, o, err)
        _check_indices(ih[sl], cs64, where='%s (%s), object %d (%d crops)' % (case, tag, o, counts[o]))
        worst = max(worst, err)
    return worst


def _indices_equal_outside_near_ties(case, oracle, counts, idx, idx_other):
    """two forms that differ by fp32 summation order give the same index wherever the oracle's own top-2 gap is >= 2e-6"""
    a, b = idx.cpu().numpy(), idx_other.cpu().numpy()
    for o, (sl, (_, cs64)) in enumerate(zip(mfc.slices(counts), oracle)):
        part = np.partition(cs64, cs64.shape[1] - 2, axis=1)
        gap = part[:, -1] - part[:, -2]
        assert not np.any((a[sl] != b[sl]) & (gap >= 2e-6)), (case, o)


def _record(c, tag, launches, vs_oracle, vs_per_object):
    report.record('multi', '%s (%s)' % (c.name, tag), counts=list(c.counts), launches=int(launches), max_latent_err_vs_fp64=vs_oracle,
                  max_latent_err_vs_per_object_calls=vs_per_object)


def test_per_detection_group_runs_conv2_and_conv3_as_one_winograd_launch_each():
    """1 / 2 / 4 detections, batch norm on: conv2 (16 x 16-pixel regions) and conv3 (four-image blocks, every object one ragged block) as group Winograd launches"""
    c = _Case('per_detection_group_winograd')
    try:
        per = _per_object(c.items(), c.x)                                # (every object's own call: Winograd conv layers too under these options)
        got = _multi(c.items(), c.x)
        assert got[3] == c.launches['default']
        worst = _against_oracle(c.name, c.oracle, c.counts, got[0], got[1], 'group Winograd launches')
        assert _rel(got[0], per[0]) < 2e-6
        _indices_equal_outside_near_ties(c.name, c.oracle, c.counts, got[1], per[1])
        assert _same(_multi(c.items(), c.x), got)                        # deterministic
        c.set_option('multi_group_winograd', 0)                          # the wave-split-K kernel for every conv layer again
        off = _multi(c.items(), c.x)
        assert off[3] == c.launches['multi_group_winograd=0']
        assert _rel(off[0], per[0]) < 5e-6
        _indices_equal_outside_near_ties(c.name, c.oracle, c.counts, off[1], per[1])
        assert not _same(off[:1], got[:1])                               # (another kernel computed the conv layers)
        _against_oracle(c.name, c.oracle, c.counts, off[0], off[1], 'multi_group_winograd = 0')
        _record(c, 'default', got[3], worst, _rel(got[0], per[0]))
    finally:
        c.close()


def test_mid_batch_group_one_winograd_launch_per_conv_layer_across_objects():
    """{5, 7, 6}: both block geometries in one launch each across three objects of different sizes -- bit for bit the per-object calls; then the frame that mixes a
    per-detection group, the mid-batch group and a loner"""
    c = _Case('mid_batch_group')
    try:
        per = _per_object(c.items(), c.x)
        got = _multi(c.items(), c.x)
        assert got[3] == c.launches['default']
        worst = _against_oracle(c.name, c.oracle, c.counts, got[0], got[1], 'mid-batch group')
        assert _same(got, per)
        assert _same(_multi(c.items(), c.x), got)
        _record(c, 'default', got[3], worst, _rel(got[0], per[0]))
        mx = mfc.CASES[c.name]['mixed']
        lone = c.add(mx['lone_seed'], mx['lone_rows'], mx['lone_options'])
        small = [c.add(seed, rows, mx['small_options']) for seed, rows in zip(mx['small_seeds'], mx['small_rows'])]
        who = [small[0], 0, 1, lone, small[1]]
        counts = [mx['small_counts'][0], c.counts[0], c.counts[1], mx['lone_count'], mx['small_counts'][1]]
        items = [(c.objs[o][0], c.objs[o][1], n) for o, n in zip(who, counts)]
        host = mfc.crops(c.name, seed=mx['crop_seed'], rows=sum(counts))
        import torch
        xm = torch.from_numpy(host).to(c.dev)
        zp, ip, sp = _per_object(items, xm)
        zm, im, sm, _ = _multi(items, xm)
        oracle = c.oracle_of(who, counts, host)
        _indices_equal_outside_near_ties(c.name, oracle, counts, im, ip)
        for k, sl in enumerate(mfc.slices(counts)):
            same = torch.equal(zm[sl], zp[sl]) and torch.equal(sm[sl], sp[sl])
            assert same or k in (0, 4), k                                # (the two per-detection items share a group plan: summation order)
            assert float((zm[sl] - zp[sl]).abs().max() / zp.abs().max()) < 2e-6 and float((sm[sl] - sp[sl]).abs().max()) < 1e-6
        _against_oracle(c.name, oracle, counts, zm, im, 'mixed frame')
    finally:
        c.close()


def test_mid_batch_group_hands_incomplete_four_image_blocks_to_one_wave_split_k_launch():
    """{5, 7, 6} on 4 "compute units": the objects' last 1 / 3 / 2 images of conv3 go to one grouped wave-split-K launch; then multi_mid_ragged = 0, then multi_mid_scan = 0"""
    import torch
    c = _Case('mid_batch_group_ragged')
    try:
        per = _per_object(c.items(), c.x)
        got = _multi(c.items(), c.x)
        assert got[3] == c.launches['default']
        worst = _against_oracle(c.name, c.oracle, c.counts, got[0], got[1], 'handed-over images')
        for sl, n in zip(mfc.slices(c.counts), c.counts):
            full = sl.start + n // 4 * 4
            assert torch.equal(got[0][sl.start:full], per[0][sl.start:full])
            assert not torch.equal(got[0][full:sl.stop], per[0][full:sl.stop])             # (another kernel computed them ...)
            assert float((got[0][sl] - per[0][sl]).abs().max() / per[0].abs().max()) < 2e-6    # (... to the same numbers)
        assert _same(_multi(c.items(), c.x), got)
        _record(c, 'default', got[3], worst, _rel(got[0], per[0]))
        c.set_option('multi_mid_ragged', 0)
        whole = _multi(c.items(), c.x)
        assert whole[3] == c.launches['multi_mid_ragged=0'] and _same(whole, per)
        c.set_option('multi_mid_scan', 0)
        alone = _multi(c.items(), c.x)                                   # (the scans per object again: the same answers from two launches fewer in the count)
        assert alone[3] == c.launches['multi_mid_ragged=0,multi_mid_scan=0'] and _same(alone, per)
    finally:
        c.close()


def test_mid_batch_fill_rule_counts_the_complete_blocks_when_the_incomplete_ones_leave():
    """25 + 24 crops on 12 "compute units", conv2 with four 8 x 8 images per block: the group forms once the one incomplete block's image leaves the launch"""
    c = _Case('mid_batch_fill_rule')
    try:
        per = _per_object(c.items(), c.x)
        got = _multi(c.items(), c.x)
        assert got[3] == c.launches['default']
        worst = _against_oracle(c.name, c.oracle, c.counts, got[0], got[1], 'complete blocks + one handed-over image')
        assert _rel(got[0], per[0]) < 5e-6
        assert _same(_multi(c.items(), c.x), got)
        _record(c, 'default', got[3], worst, _rel(got[0], per[0]))
        c.set_option('multi_mid_ragged', 0)
        off = _multi(c.items(), c.x)
        assert off[3] == c.launches['multi_mid_ragged=0'] and _same(off[:2], per[:2])      # (13 blocks in two rounds: below the rule, one object after the other)
    finally:
        c.close()


def test_mid_batch_group_takes_the_layers_it_fills_and_leaves_the_others_to_the_objects():
    """2 x 6 on 8 "compute units": conv2 as one Winograd launch across the objects, conv3 per object -- bit for bit the per-object calls"""
    c = _Case('mid_batch_group_some_layers')
    try:
        per = _per_object(c.items(), c.x)
        got = _multi(c.items(), c.x)
        assert got[3] == c.launches['default']
        worst = _against_oracle(c.name, c.oracle, c.counts, got[0], got[1], 'conv2 grouped, conv3 per object')
        assert _same(got, per)
        assert _same(_multi(c.items(), c.x), got)
        _record(c, 'default', got[3], worst, _rel(got[0], per[0]))
    finally:
        c.close()


def test_a_class_with_six_boxes_joins_the_per_detection_group_as_items_of_four():
    """[6, 2]: the first class as two items (4 + 2 boxes, the same handles) inside the frame's per-detection group; multi_split_items = 0: its own call"""
    import torch
    c = _Case('split_items')
    try:
        per = _per_object(c.items(), c.x)
        got = _multi(c.items(), c.x)
        assert got[3] == c.launches['default']
        worst = _against_oracle(c.name, c.oracle, c.counts, got[0], got[1], 'items of four')
        assert _rel(got[0], per[0]) < 5e-6 and float((got[2] - per[2]).abs().max()) < 1e-6
        _indices_equal_outside_near_ties(c.name, c.oracle, c.counts, got[1], per[1])
        assert _same(_multi(c.items(), c.x), got)
        _record(c, 'default', got[3], worst, _rel(got[0], per[0]))
        c.set_option('multi_split_items', 0)
        off = _multi(c.items(), c.x)
        assert torch.equal(off[0][:6], per[0][:6]) and torch.equal(off[1][:6], per[1][:6])  # the 6-box class: its own call, bit for bit
        assert torch.equal(off[1], per[1])                               # (the 2-box class alone in its group keeps its own plan)
    finally:
        c.close()


def test_two_classes_of_five_boxes_that_fill_no_layer_form_no_group():
    c = _Case('no_group')
    try:
        per = _per_object(c.items(), c.x)
        got = _multi(c.items(), c.x)
        assert got[3] == c.launches['default'] == 0 and _same(got, per)
        worst = _against_oracle(c.name, c.oracle, c.counts, got[0], got[1], 'per-object path')
        _record(c, 'default', got[3], worst, _rel(got[0], per[0]))
    finally:
        c.close()
