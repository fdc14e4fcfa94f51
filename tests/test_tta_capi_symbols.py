"""include/hipac_tta.h <-> libhipac_hip.so <-> tta.TTA_SYMBOLS: every declared entry point is exported and bound, the three
version numbers agree, the older headers are as they were, and the argument checks answer without a GPU."""
import os
import re

import pytest

from ss25_hierarchical_multiscale_image_classification_amd import build, capi, detect, tta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hipac_tta.h")
PATCH_BYTES = 224 * 224 * 3


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return tta.load_tta_library()


def declared_symbols(header):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hipac_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_tta_symbol_is_exported_and_bound(lib):
    names = declared_symbols(HEADER)
    assert names == ["hipac_tta_abi_version", "hipac_tta_reduce", "hipac_tta_view"]
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(tta.TTA_SYMBOLS) == names
    text = open(HEADER).read()
    hdr = int(re.search(r"#define HIPAC_TTA_ABI_VERSION (\d+)", text).group(1))
    assert lib.hipac_tta_abi_version() == hdr == tta.TTA_ABI_VERSION == 1
    assert int(re.search(r"#define HIPAC_TTA_SIDE (\d+)", text).group(1)) == tta.SIDE == capi.PATCH == 224
    assert int(re.search(r"#define HIPAC_TTA_VIEWS (\d+)", text).group(1)) == tta.VIEWS == 8
    assert tta.MODES == {"none": (0,), "rot4": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}


def test_the_source_and_the_header_are_built():
    assert "tta.hip" in build.SOURCES
    assert os.path.join(ROOT, "include", "hipac_tta.h") in [str(h) for h in build.PUBLIC_HEADERS]
    assert os.path.exists(os.path.join(str(build.CSRC), "tta.hip"))


def test_the_older_headers_are_untouched(lib):
    ours = set(declared_symbols(HEADER))
    base = declared_symbols(os.path.join(ROOT, "include", "hipac.h"))
    assert sorted(capi.SYMBOLS) == base and not ours & set(base)
    assert lib.hipac_abi_version() == capi.ABI_VERSION == 8
    det = declared_symbols(os.path.join(ROOT, "include", "hipac_detect.h"))
    assert sorted(detect.DETECT_SYMBOLS) == det and len(det) == 7 and not ours & set(det)
    assert detect.load_detect_library().hipac_detect_abi_version() == detect.DETECT_ABI_VERSION == 1


def test_one_probability_function_for_both_kernels():
    """hipac_detect_probs and hipac_tta_reduce evaluate one device function: the expression is written once, in detect_prob.h."""
    csrc = str(build.CSRC)
    for name in ("detect.hip", "tta.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "detect_prob.h"' in text and "tumor_prob(" in text and "expf" not in text, name
    assert open(os.path.join(csrc, "detect_prob.h")).read().count("expf(") == 1


def test_view_refusals_answer_before_any_launch(lib):
    fake = 1 << 20  # never dereferenced: every check below fails before the first launch
    far = fake + 64 * PATCH_BYTES
    assert lib.hipac_tta_view(None, 4, 1, far, None) == -1
    assert b"null" in lib.hipac_last_error()
    assert lib.hipac_tta_view(fake, 4, 1, None, None) == -1
    assert lib.hipac_tta_view(fake, -1, 1, far, None) == -1
    assert b"n -1" in lib.hipac_last_error()
    assert lib.hipac_tta_view(fake, 1 << 28, 1, far, None) == -1
    for bad in (-1, 8, 100):
        assert lib.hipac_tta_view(fake, 4, bad, far, None) == -1
        assert b"view" in lib.hipac_last_error()
    # byte ranges that intersect: in place, out inside in, in inside out, the last byte of one on the first of the other
    for out in (fake, fake + PATCH_BYTES, fake - PATCH_BYTES, fake + 4 * PATCH_BYTES - 4, fake - 4 * PATCH_BYTES + 4):
        assert lib.hipac_tta_view(fake, 4, 0, out, None) == -1, out
        assert b"intersect" in lib.hipac_last_error()
    assert lib.hipac_tta_view(fake + 1, 4, 1, far, None) == -1
    assert b"aligned" in lib.hipac_last_error()
    assert lib.hipac_tta_view(fake, 4, 1, far + 2, None) == -1
    # n = 0 succeeds without a launch (there is no device here to launch on), also for ranges that touch
    assert lib.hipac_tta_view(fake, 0, 5, far, None) == 0
    assert lib.hipac_tta_view(fake, 0, 0, fake, None) == 0


def test_reduce_refusals_answer_before_any_launch(lib):
    fake = 1 << 20
    assert lib.hipac_tta_reduce(None, 8, 4, 1, fake, fake, None) == -1
    assert b"null" in lib.hipac_last_error()
    assert lib.hipac_tta_reduce(fake, 8, 4, 1, None, fake, None) == -1
    for views in (0, 9, -1):
        assert lib.hipac_tta_reduce(fake, views, 4, 1, fake, None, None) == -1
        assert b"views" in lib.hipac_last_error()
    assert lib.hipac_tta_reduce(fake, 8, -1, 1, fake, None, None) == -1
    assert lib.hipac_tta_reduce(fake, 8, 4, 2, fake, None, None) == -1
    assert b"tumor_class" in lib.hipac_last_error()
    assert lib.hipac_tta_reduce(None, 8, 0, 1, None, None, None) == 0  # nothing to do
