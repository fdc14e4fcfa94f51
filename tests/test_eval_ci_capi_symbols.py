"""include/hipac_eval_ci.h <-> libhipac_hip.so <-> froc_ci.EVAL_CI_SYMBOLS: every declared entry point is exported and
bound, the three version numbers agree, the list shares no name with any other header's, and the refusals answer without
a GPU."""
import ctypes as C
import os
import re

import pytest

from ss25_hierarchical_multiscale_image_classification_amd import (build, capi, detect, froc, froc_ci, mil_dropout, mil_gated, mil_heads,
                                                                   mil_levels, mil_train, stain, tiff_pyramid, tissue, validate)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hipac_eval_ci.h")


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return froc_ci.load_eval_ci_library()


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hipac_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_eval_ci_symbol_is_exported_and_bound(lib):
    names = declared_symbols()
    assert names == ["hipac_eval_ci_abi_version", "hipac_eval_ci_bootstrap", "hipac_eval_ci_counts", "hipac_eval_ci_workspace_bytes"]
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(froc_ci.EVAL_CI_SYMBOLS) == names
    others = (capi.SYMBOLS, froc.EVAL_SYMBOLS, mil_train.MIL_TRAIN_SYMBOLS, mil_dropout.MIL_DROPOUT_SYMBOLS, mil_heads.MIL_HEADS_SYMBOLS,
              mil_gated.MIL_GATED_SYMBOLS, mil_levels.MIL_LEVELS_SYMBOLS, detect.DETECT_SYMBOLS, tissue.TISSUE_SYMBOLS, stain.STAIN_SYMBOLS,
              tiff_pyramid.LZW_SYMBOLS, tiff_pyramid.DEFLATE_SYMBOLS, validate.VALIDATE_SYMBOLS)
    for other in others:
        assert not set(names) & set(other)  # the other headers' lists and ABIs stay as they were
    assert len(froc.EVAL_SYMBOLS) == 5
    text = open(HEADER).read()
    hdr = int(re.search(r"#define HIPAC_EVAL_CI_ABI_VERSION (\d+)", text).group(1))
    assert lib.hipac_eval_ci_abi_version() == hdr == froc_ci.EVAL_CI_ABI_VERSION == 1
    assert lib.hipac_eval_abi_version() == froc.EVAL_ABI_VERSION and lib.hipac_abi_version() == capi.ABI_VERSION
    def macro(name):
        m = re.search(rf"#define HIPAC_EVAL_CI_{name}\s+(?:(\d+)|\(1 << (\d+)\))", text)
        return int(m.group(1)) if m.group(1) else 1 << int(m.group(2))

    assert {k: macro(k) for k in ("MAX_CASES", "MAX_EVENTS", "MAX_REPLICATES", "MAX_RATES", "CHUNK")} == {"MAX_CASES": froc_ci.MAX_CASES, "MAX_EVENTS": froc_ci.MAX_EVENTS, "MAX_REPLICATES": froc_ci.MAX_REPLICATES,
                      "MAX_RATES": froc_ci.MAX_RATES, "CHUNK": froc_ci.CHUNK}
    assert "eval_ci.hip" in build.SOURCES and HEADER in [str(p) for p in build.PUBLIC_HEADERS]


def test_workspace_query_refuses_bad_sizes(lib):
    q = lib.hipac_eval_ci_workspace_bytes
    for S, n, B in ((0, 10, 1), (4097, 10, 1), (-1, 10, 1), (10, -1, 1), (10, (1 << 24) + 1, 1), (10, 10, 0), (10, 10, 65537)):
        assert q(S, n, B) == 0, (S, n, B)
    for S, n, B in ((1, 0, 1), (129, 260000, 2000), (4096, 1 << 24, 65536)):
        assert q(S, n, B) >= 2 * 4 * S, (S, n, B)
    assert q(4096, 0, 1) <= 40 * 1024  # four workgroups of a replicate each fit one CU's 160 KiB


def test_bad_arguments_return_errors_before_any_launch(lib):
    fake = 256  # never dereferenced: every check below fails before the first launch
    rates = (C.c_int32 * 6)(1, 2, 4, 8, 16, 32)
    rp = C.cast(rates, C.c_void_p)
    ok = [fake, fake, fake, 100, fake, fake, fake, fake, 7, 3, 0, 64, rp, 6, fake, fake, fake, fake, fake, None]

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return a

    fn = lib.hipac_eval_ci_bootstrap
    for i in (0, 1, 2, 4, 5, 6, 7, 12, 14, 15, 16, 17, 18):
        assert fn(*with_(i, None)) == -1, i
        assert b"null" in lib.hipac_last_error()
    for i, v in ((11, 0), (11, 65537), (8, 0), (8, 4097), (3, -1), (3, (1 << 24) + 1)):
        assert fn(*with_(i, v)) == -1, (i, v)
        assert b"need" in lib.hipac_last_error()
    assert fn(*with_(0, 260)) == -1 and b"aligned" in lib.hipac_last_error()
    assert fn(*with_(10, -1)) == -1 and b"replicates" in lib.hipac_last_error()
    assert fn(*with_(10, (1 << 32) - 63)) == -1
    for n_rates in (0, 9):
        assert fn(*with_(13, n_rates)) == -1 and b"n_rates" in lib.hipac_last_error()
    bad = (C.c_int32 * 6)(1, 2, 0, 8, 16, 32)
    assert fn(*with_(12, C.cast(bad, C.c_void_p))) == -1 and b"rates4[2]" in lib.hipac_last_error()
    cnt = lib.hipac_eval_ci_counts
    assert cnt(3, 0, 1, 5, None, None) == -1 and b"null" in lib.hipac_last_error()
    for B, S in ((0, 5), (65537, 5), (1, 0), (1, 4097)):
        assert cnt(3, 0, B, S, fake, None) == -1, (B, S)
    assert cnt(3, -1, 1, 5, fake, None) == -1
