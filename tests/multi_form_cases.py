"""The small-net cases of the grouped multi-object query's launch forms, shared by the CPU fiber emulator tests
(tests/test_emu_multi.py: the host branches of the kernels) and their hardware twins (tests/test_gpu_multi_forms.py: the device
branches -- MFMA fragment layouts, LDS-DMA fills, the XCD block map, the indexed per-object argument table, concurrent ticket
hand-offs).  Per case: the network, the detections per object, the encoder options that force the form on a net this small, the
seeds, the codebook sizes and the launch count of the grouped part per option setting.

Every case names its wavek_target_blocks (the planner's round size, "compute units"): the host code and the options are then
the same on the emulator and on the MI355X, so the launch counts asserted on the GPU are the ones the CPU run pins."""
import numpy as np

from augmentedautoencoder_amd.weights import EncoderConfig
from oracle import synth

# (shape, filters, strides, kernel, latent, batch norm)
NET64_BN = ((64, 64, 3), [32, 64, 64], [2, 2, 2], 5, 128, True)           # conv2: 16 x 16 outputs (regions of one image), conv3: 8 x 8 (four images per block)
NET32 = ((32, 32, 3), [32, 64], [2, 2], 5, 128, False)                    # conv2: 8 x 8 outputs (four images per block)
NET16_BN = ((16, 16, 3), [32, 64, 64, 32], [2, 2, 2, 1], 5, 128, True)    # no layer in the Winograd form: the per-detection chain

# every eligible layer as Winograd, alone and in a group (the launches of these nets are tiny against the 256 compute units the fill rule counts with); conv1 in its
# whole-tile form, as at the batch sizes that group on the GPU
WINO = {'winograd_min_batch': 1, 'winograd_min_blocks': 1, 'first_group_split_max_tiles': 0}

CASES = {
    # 1 / 2 / 4 detections: conv2 and conv3 (every object one ragged four-image block) as ONE Winograd launch each inside the per-detection group
    'per_detection_group_winograd': dict(
        config=NET64_BN, counts=[1, 2, 4], options={'winograd_min_batch': 1, 'winograd_min_blocks': 1, 'wavek_target_blocks': 256},
        weight_seeds=[950, 957, 964], codebook_rows=[36 * 8, 36 * 9 + 1, 36 * 10 + 2], crop_seed=63,
        launches={'default': 5,                                       # conv1, conv2 (Winograd), conv3 (Winograd), GEMV, scan
                  'multi_group_winograd=0': 5}),                      # the wave-split-K kernel for every conv layer again
    # {5, 7, 6}: a mid-batch group, both block geometries
    'mid_batch_group': dict(
        config=NET64_BN, counts=[5, 7, 6], options=dict(WINO, wavek_target_blocks=256),
        weight_seeds=[500, 507, 514], codebook_rows=[36 * 9, 36 * 11 + 3, 36 * 13 + 6], crop_seed=58,
        launches={'default': 5},                                      # conv1 (whole tiles), conv2, conv3, the three scans as one launch, one reduce launch; the dense GEMV per object
        # ... and a frame that mixes a per-detection group (n <= 4), the group's first two objects and a loner that joins neither (its own options)
        mixed=dict(lone_seed=600, lone_rows=36 * 8, lone_options=dict(WINO, multi_mid_group=0, wavek_target_blocks=256), lone_count=5,
                   small_seeds=[610, 611], small_rows=[36 * 7, 36 * 7 + 1], small_options={'wavek_target_blocks': 256}, small_counts=[2, 1], crop_seed=59)),
    # the same on 4 "compute units": conv3's incomplete four-image blocks open a second round -> the last 1 / 3 / 2 images go to ONE grouped wave-split-K launch
    'mid_batch_group_ragged': dict(
        config=NET64_BN, counts=[5, 7, 6], options=dict(WINO, wavek_target_blocks=4, winograd_xcd_cols=0),
        weight_seeds=[800, 807, 814], codebook_rows=[36 * 9, 36 * 11 + 3, 36 * 13 + 6], crop_seed=61,
        launches={'default': 6,                                       # conv1, conv2, conv3's complete blocks, conv3's last images, scans, reduce
                  'multi_mid_ragged=0': 5,                            # every image in the Winograd launch
                  'multi_mid_ragged=0,multi_mid_scan=0': 3}),         # ... and the scans per object again
    # 25 + 24 crops on 12 "compute units": 13 four-image blocks fill 54 % of two rounds (no group); without the incomplete one, 12 = one full round
    'mid_batch_fill_rule': dict(
        config=NET32, counts=[25, 24], options={'winograd_min_batch': 1, 'first_group_split_max_tiles': 0, 'wavek_target_blocks': 12, 'winograd_xcd_cols': 0},
        weight_seeds=[900, 901], codebook_rows=[36 * 8, 36 * 8 + 1], crop_seed=62,
        launches={'default': 6,                                       # conv1, conv2's twelve complete blocks, the 25th crop of object 0, the dense layer, scans, reduce
                  'multi_mid_ragged=0': 0}),                          # 13 blocks in two rounds: below the rule, one object after the other
    # 2 x 6 on 8 "compute units": conv2 (12 blocks, two rounds at 75 %) across the objects, conv3 (4 blocks, half a round) per object
    'mid_batch_group_some_layers': dict(
        config=NET64_BN, counts=[6, 6], options={'winograd_min_batch': 1, 'first_group_split_max_tiles': 0, 'wavek_target_blocks': 8, 'winograd_xcd_cols': 0},
        weight_seeds=[970, 971], codebook_rows=[36 * 8, 36 * 8 + 1], crop_seed=64,
        launches={'default': 4}),                                     # conv1, conv2, the scans, the reduce (conv3 and the dense GEMV per object)
    # 6 + 2 boxes: the first class as two items (4 + 2) inside the frame's per-detection group
    'split_items': dict(
        config=NET16_BN, counts=[6, 2], options={'wavek_target_blocks': 256},
        weight_seeds=[980, 981], codebook_rows=[36 * 9, 36 * 9 + 1], crop_seed=65,
        launches={'default': 6}),                                     # conv1, three conv layers, GEMV, scan: one group of three items
    # 2 x 5 under the default fill rule: two tiny launches do not fill 256 compute units -> no group
    'no_group': dict(
        config=NET64_BN, counts=[5, 5], options={'winograd_min_batch': 1, 'multi_split_items': 0, 'wavek_target_blocks': 256},
        weight_seeds=[700, 701], codebook_rows=[36 * 8, 36 * 8], crop_seed=60,
        launches={'default': 0}),
}


def config(case):
    return EncoderConfig(*CASES[case]['config'])


def weights(cfg, seed):
    return synth.make_weights(seed=seed, shape=cfg.shape, num_filter=cfg.num_filter, strides=cfg.strides, latent=cfg.latent_space_size,
                              batch_norm=cfg.batch_norm, kernel_size=cfg.kernel_size)


def codebook(cfg, seed, rows):
    """the codebook that goes with the encoder of `seed`"""
    return synth.make_codebook(rows, cfg.latent_space_size, seed=seed + 100, planted_duplicates=5)


def crops(case, seed=None, rows=None):
    c = CASES[case]
    return synth.make_crops(sum(c['counts']) if rows is None else rows, seed=c['crop_seed'] if seed is None else seed, shape=tuple(c['config'][0]))


def slices(counts):
    at = np.cumsum([0] + list(counts))
    return [slice(int(a), int(b)) for a, b in zip(at[:-1], at[1:])]
