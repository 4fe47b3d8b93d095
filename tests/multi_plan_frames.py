"""The frames of tests/golden/multi_plans.json and how one is replayed on an emulator library (tests/emu): shared by the recorder
(tests/golden/make_multi_plans.py, run in a checkout of the parent commit) and by tests/test_multi_plans.py (the working tree).

Every frame is on the default network (128 x 128 x 3, filters 128 256 512 512, 5 x 5 stride 2, latent 128) with
wavek_target_blocks = 256 (the MI355X's round size, whatever the emulated device reports), one FRESH encoder and one fresh
8020-row codebook per class; the weights' values do not matter.  Per frame: the prepared flags (all unset), then
aae_multi_workspace_bytes, then its answer, the flags and the plan (aae_emu_multi_plan_dump in tests/emu/aae_emu_lib.cpp)."""
import ctypes
import json
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from augmentedautoencoder_amd import _lib

CONFIG4 = [34, 26, 27, 32, 31, 32, 33, 41]            # one class per bucket of a B = 256 frame
GROUP_OPTIONS = ('multi_group_plan', 'multi_group_winograd', 'multi_mid_group', 'multi_mid_ragged', 'multi_split_items')


def _frame(counts, options=None, scan_only=0, bf16_item=-1, stride2_item=-1):
    return {'counts': list(counts), 'options': dict(options or {}), 'scan_only': scan_only, 'bf16_item': bf16_item, 'stride2_item': stride2_item}


def frames():
    # boxes per class: the frames DESIGN.md section 4c measures and the edges between the forms ({8, 9}: two classes that stay whole and fill no layer together)
    out = [_frame(c) for c in ([1] * 2, [1] * 8, [1] * 16, [1] * 17, [4] * 8, [4] * 16, [1, 1, 2, 4, 1, 3, 1, 2], [5] * 4, [6] * 4, [8] * 4, [10] * 4, [8] * 2,
                               [6] * 8, [16] * 8, [5, 9, 14], [9, 1, 1, 1, 1, 1, 1, 1], CONFIG4, [8, 9])]
    out += [_frame([n]) for n in (4, 5, 9, 17, 18, 69)]                                      # one class alone
    out.append(_frame([4] * 8, bf16_item=2, stride2_item=5))                                 # two items for the per-object path
    for opts in [{name: 0} for name in GROUP_OPTIONS] + [{'winograd_min_blocks': 1}]:
        out += [_frame([4] * 8, opts), _frame(CONFIG4, opts)]
    out += [_frame([1] * 8, scan_only=1), _frame(CONFIG4, scan_only=1)]
    return out


def replay(L, frame):
    """frame -> {'before': ..., 'workspace_bytes': n, 'after': ...} on the library L (an _lib.declare'd emulator build)"""
    L.aae_emu_multi_plan_dump.restype = ctypes.c_size_t
    L.aae_emu_multi_plan_dump.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    from augmentedautoencoder_amd.weights import EncoderConfig
    desc = EncoderConfig().to_desc()
    desc.batch_norm = 0
    w = np.full(25 * 512 * 512, 1e-3, dtype=np.float32)       # (the largest array: every weight pointer reads from it)
    hw = (ctypes.c_void_p * 10)(*([w.ctypes.data] * 10))
    n = len(frame['counts'])
    arr = (_lib.MultiItem * n)()

    def encoder(_):
        h = ctypes.c_void_p()
        _lib.check(L, L.aae_encoder_create(ctypes.byref(desc), hw, 10, ctypes.byref(h)), 'aae_encoder_create')
        for name, value in [('wavek_target_blocks', 256)] + sorted(frame['options'].items()):
            _lib.check(L, L.aae_encoder_set_option(h, name.encode(), value), name)
        return h

    try:
        if not frame['scan_only']:
            with ThreadPoolExecutor(8) as pool:               # (a handle's creation packs 58 MB of weights: most of a replay's time)
                for k, h in enumerate(pool.map(encoder, range(n))):
                    arr[k].enc = h
        for k in range(n):
            h = ctypes.c_void_p()
            dtype = _lib.AAE_DTYPE_BF16 if k == frame['bf16_item'] else _lib.AAE_DTYPE_F32
            _lib.check(L, L.aae_codebook_create(w.ctypes.data, 8020, 128, dtype, 0, ctypes.byref(h)), 'aae_codebook_create')
            arr[k].cb = h
            arr[k].n = frame['counts'][k]
            arr[k].col_stride = 2 if k == frame['stride2_item'] else 1

        def dump(with_plan):
            size = L.aae_emu_multi_plan_dump(arr, n, frame['scan_only'], with_plan, None, 0) + 1
            text = ctypes.create_string_buffer(size)
            L.aae_emu_multi_plan_dump(arr, n, frame['scan_only'], with_plan, text, size)
            return json.loads(text.value.decode())

        before = dump(0)
        nbytes = L.aae_multi_workspace_bytes(arr, n, frame['scan_only'])
        return {'before': before, 'workspace_bytes': nbytes, 'after': dump(1)}
    finally:
        for k in range(n):
            if arr[k].enc:
                L.aae_encoder_destroy(arr[k].enc)
            if arr[k].cb:
                L.aae_codebook_destroy(arr[k].cb)
