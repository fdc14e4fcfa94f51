"""include/hipac_augment_hed.h <-> libhipac_hip.so <-> augment_hed.AUGMENT_HED_SYMBOLS: every declared entry point is exported and
bound, the version numbers agree, hipac.h's ABI is untouched, and the argument checks answer without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ss25_hierarchical_multiscale_image_classification_amd import augment, augment_hed, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hipac_augment_hed.h")


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return augment_hed.load_augment_hed_library()


def declared_symbols(header):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hipac_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    names = declared_symbols(HEADER)
    assert names == ["hipac_augment_hed_abi_version", "hipac_augment_hed_apply", "hipac_augment_views_hed"]
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(augment_hed.AUGMENT_HED_SYMBOLS) == names
    text = open(HEADER).read()
    define = lambda name: int(re.search(rf"#define HIPAC_AUGMENT_HED_{name} (\d+)", text).group(1))
    assert lib.hipac_augment_hed_abi_version() == define("ABI_VERSION") == augment_hed.AUGMENT_HED_ABI_VERSION == 1
    assert define("PAYLOAD") == augment_hed.PAYLOAD == 12
    assert HEADER in [str(p) for p in build.PUBLIC_HEADERS]
    # the views entry point takes hipac_augment_views' arguments plus the two payload pointers
    assert augment_hed.AUGMENT_HED_SYMBOLS["hipac_augment_views_hed"][1][:15] == capi.SYMBOLS["hipac_augment_views"][1][:15]
    assert len(augment_hed.AUGMENT_HED_SYMBOLS["hipac_augment_views_hed"][1]) == len(capi.SYMBOLS["hipac_augment_views"][1]) + 2


def test_hipac_h_is_untouched(lib):
    names = declared_symbols(os.path.join(ROOT, "include", "hipac.h"))
    assert sorted(capi.SYMBOLS) == names
    assert not set(declared_symbols(HEADER)) & set(capi.SYMBOLS)
    assert lib.hipac_abi_version() == capi.ABI_VERSION == 8
    assert augment.PARAMS == 24


def test_the_od_table_has_one_literal():
    csrc = build.CSRC
    holders = [p.name for p in sorted(csrc.glob("*")) if p.is_file() and p.suffix in (".h", ".hip") and "22713, 19874" in p.read_text()]
    assert holders == ["stain_od.h"]
    assert '#include "stain_od.h"' in (csrc / "stain.hip").read_text() and '#include "stain_od.h"' in (csrc / "augment_hed.h").read_text()


def test_bad_arguments_return_errors_before_any_launch(lib):
    fake = 4096  # never dereferenced: every check below fails before the first launch
    good = (C.c_double * 24)(*augment_hed.identity_maps(2).reshape(-1))
    # hipac_augment_hed_apply(images, n_views, hed_host, hed_dev, stream)
    for k in (0, 2, 3):
        a = [fake, 2, good, fake, None]
        a[k] = None
        assert lib.hipac_augment_hed_apply(*a) == -1 and b"null" in lib.hipac_last_error()
    for n in (0, -1, 65536):
        assert lib.hipac_augment_hed_apply(fake, n, good, fake, None) == -1 and b"n_views" in lib.hipac_last_error()
    assert lib.hipac_augment_hed_apply(fake + 2, 2, good, fake, None) == -1 and b"aligned" in lib.hipac_last_error()
    for entry, value in ((0, float("nan")), (13, float("inf")), (23, float("-inf"))):
        bad = (C.c_double * 24)(*good)
        bad[entry] = value
        assert lib.hipac_augment_hed_apply(fake, 2, bad, fake, None) == -1 and b"finite" in lib.hipac_last_error()
        assert f"view {entry // 12}".encode() in lib.hipac_last_error()
    # hipac_augment_views_hed: hipac_augment_views' checks, then the payload's
    rows = np.array([augment.identity_view(0), augment.identity_view(1)], np.int32)
    pr = rows.ctypes.data

    def views(pool=fake, n_pool=4, P=224, geometry=1, params=pr, pdev=fake, n=2, lut=fake, crops=fake, out=fake, hed=good, hdev=fake):
        return lib.hipac_augment_views_hed(pool, n_pool, P, geometry, params, pdev, n, None, None, 0, lut, None, crops, out, None, hed, hdev, None)

    for kw in ({"pool": None}, {"params": None}, {"pdev": None}, {"lut": None}, {"crops": None}, {"out": None}, {"hdev": None}):
        assert views(**kw) == -1 and b"null" in lib.hipac_last_error(), kw
    for n in (0, 65536):
        assert views(n=n) == -1 and b"bad size" in lib.hipac_last_error()
    assert views(geometry=2) == -1 and views(P=448) == -1 and views(n_pool=1) == -1  # view 1 reads patch 1
    assert views(geometry=0) == -1 and b"tables" in lib.hipac_last_error()
    for entry, value in ((5, float("nan")), (12, float("inf"))):
        bad = (C.c_double * 24)(*good)
        bad[entry] = value
        assert views(hed=bad) == -1 and b"finite" in lib.hipac_last_error() and b"augment_views_hed" in lib.hipac_last_error()
    # without a payload it answers as hipac_augment_views does, word for word
    assert views(hed=None, hdev=None, n=0) == -1
    msg = lib.hipac_last_error()
    assert capi.load_library().hipac_augment_views(fake, 4, 224, 1, pr, fake, 0, None, None, 0, fake, None, fake, fake, None, None) == -1
    assert lib.hipac_last_error() == msg and msg.startswith(b"augment_views:")
