"""Host only: the shuffle trees of the small kernels live in csrc/wave_reduce.h and nowhere else."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ss25_hierarchical_multiscale_image_classification_amd", "csrc")
HEADER = "wave_reduce.h"
# the exceptions the header's comment names: their cross-lane steps are not a 64-lane reduction or scan of one value, or (the
# score loop of mil_heads.hip) a call costs a register
EXCEPTIONS = {"stem.h", "halo16.h", "halo16x2.h", "layer1_c64.h", "block16_c64.h", "tile_place.h", "train_kernels.h",
              "level_planes.hip", "mil_heads.hip"}
SHUFFLES = ("__shfl_down(", "__shfl_xor(", "__shfl_up(")
DELETED = ("ci_block_scan_excl", "ci_block_sum", "ci_block_min", "ev_wave_sum", "ev_block_sum", "block_exclusive_scan256",
           "block_sum_u32", "vd_wave_sum", "block_reduce", "mil_block_reduce", "mil_wave_sum")


def sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")):
            yield name, open(os.path.join(CSRC, name)).read()


def test_the_shuffle_trees_are_shared_not_restated():
    header = open(os.path.join(CSRC, HEADER)).read()
    assert all(s in header for s in SHUFFLES)
    for name in EXCEPTIONS:
        assert name in header, f"{HEADER} does not name the exception {name}"
    for name, text in sources():
        if name != HEADER and name not in EXCEPTIONS:
            assert not any(s in text for s in SHUFFLES), f"{name} has a shuffle tree of its own"
    heads = open(os.path.join(CSRC, "mil_heads.hip")).read()
    assert sum(heads.count(s) for s in SHUFFLES) == 1  # mh_score_kernel's loop, and only that


def test_the_per_file_reduction_helpers_are_gone():
    for name, text in sources():
        for helper in DELETED:
            assert not re.search(r"\b" + helper + r"\b", text), f"{name} still names {helper}"
