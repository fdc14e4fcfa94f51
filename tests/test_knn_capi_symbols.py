"""include/hipac_knn.h <-> libhipac_hip.so <-> knn.KNN_SYMBOLS: every declared entry point is exported and bound, and the
three version numbers agree.  The workspace and split queries and the argument checks answer without a GPU."""
import os
import re

import pytest

from ss25_hierarchical_multiscale_image_classification_amd import build, capi, knn, mil_heads, mil_train, validate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hipac_knn.h")
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return knn.load_knn_library()


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hipac_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_knn_symbol_is_exported_and_bound(lib):
    names = declared_symbols()
    assert names == ["hipac_knn_abi_version", "hipac_knn_bank_splits", "hipac_knn_inv_norms", "hipac_knn_topk",
                     "hipac_knn_topk_workspace_bytes", "hipac_knn_vote"]
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(knn.KNN_SYMBOLS) == names
    for other in (capi.SYMBOLS, capi.PAIR_TAP_SYMBOLS, mil_train.MIL_TRAIN_SYMBOLS, mil_heads.MIL_HEADS_SYMBOLS, validate.VALIDATE_SYMBOLS):
        assert not set(names) & set(other)  # the other headers' lists and ABIs stay as they were
    text = open(HEADER).read()
    hdr = int(re.search(r"#define HIPAC_KNN_ABI_VERSION (\d+)", text).group(1))
    assert lib.hipac_knn_abi_version() == hdr == knn.KNN_ABI_VERSION == 1
    assert int(re.search(r"#define HIPAC_KNN_MAX_K (\d+)", text).group(1)) == knn.MAX_K == 256
    assert lib.hipac_abi_version() == capi.ABI_VERSION and lib.hipac_validate_abi_version() == validate.VALIDATE_ABI_VERSION
    assert "knn.hip" in build.SOURCES and HEADER in [str(p) for p in build.PUBLIC_HEADERS]
    for rule in ("lower position", "NaN", "descending"):  # the three ordering rules are stated where a caller reads them
        assert rule in text, rule


def test_queries_refuse_bad_sizes_and_accept_the_limits(lib):
    big = 1 << 24
    for q in (lib.hipac_knn_topk_workspace_bytes, lib.hipac_knn_bank_splits):
        # (n_q, n_b, F, K)
        for a in ((100, 1000, 6, 20), (100, 1000, 2, 20), (100, 1000, 2052, 20), (100, 1000, 0, 20), (100, 1000, -4, 20),
                  (100, 1000, 512, 0), (100, 1000, 512, 257), (100, 1000, 512, -1),
                  (100, 19, 512, 20), (100, 255, 512, 256), (100, 0, 512, 1),
                  (0, 1000, 512, 20), (-1, 1000, 512, 20), (big + 1, 1000, 512, 20), (100, big + 1, 512, 20)):
            assert q(*a) == 0, a
        for a in ((1, 1, 4, 1), (big, big, 2048, 256), (100, 20, 512, 20), (100, 256, 512, 256), (1, big, 4, 1), (big, 1, 2048, 1),
                  (200_000, 800_000, 512, 20), (1000, 800_000, 512, 20)):
            assert q(*a) > 0, a
    # a bank is cut only when the queries alone leave the device idle; a group keeps at least K rows
    assert lib.hipac_knn_bank_splits(200_000, 800_000, 512, 20) == 1
    assert lib.hipac_knn_bank_splits(1000, 800_000, 512, 20) >= 32
    assert lib.hipac_knn_bank_splits(5, 20_000, 64, 20) >= 2
    assert lib.hipac_knn_bank_splits(3, 2560, 64, 250) == 10
    assert lib.hipac_knn_bank_splits(5, 300, 128, 256) == 1
    for a in ((5, 20_000, 64, 20), (3, 2560, 64, 250), (1, big, 4, 1)):
        s = lib.hipac_knn_bank_splits(*a)
        assert 2 <= s <= 256 and a[0] * s * a[3] * 8 <= lib.hipac_knn_topk_workspace_bytes(*a) < a[0] * s * a[3] * 8 + 256


def test_bad_arguments_return_einval_before_any_launch(lib):
    fake = 256  # never dereferenced: every check below fails before the first launch
    huge = 1 << 40
    # X, n_feat_rows, F, q_rows, n_q, q_scale, b_rows, n_b, b_scale, K, sim_out, idx_out, workspace, bytes, stream
    ok = [fake, 30_000, 64, None, 5, None, None, 20_000, None, 20, fake, fake, fake, huge, None]

    def with_(i, v, base=ok):
        a = list(base)
        a[i] = v
        return a

    for i in (0, 10, 11, 12):
        assert lib.hipac_knn_topk(*with_(i, None)) == EINVAL, i
        assert b"null" in lib.hipac_last_error()
    assert lib.hipac_knn_bank_splits(5, 20_000, 64, 20) >= 2  # so the workspace is more than the 16 bytes below
    assert lib.hipac_knn_topk(*with_(13, 16)) == EINVAL
    assert b"workspace" in lib.hipac_last_error()
    assert lib.hipac_knn_topk(*with_(7, 19)) == EINVAL  # n_b < K: refused, not padded
    assert b"n_b" in lib.hipac_last_error()
    for i, v in ((2, 6), (2, 2052), (9, 0), (9, 257), (4, 0), (4, (1 << 24) + 1), (7, (1 << 24) + 1)):
        assert lib.hipac_knn_topk(*with_(i, v)) == EINVAL, (i, v)
    assert lib.hipac_knn_topk(*with_(0, 260)) == EINVAL
    assert b"aligned" in lib.hipac_last_error()
    assert lib.hipac_knn_topk(*with_(1, 10_000)) == EINVAL  # identity bank list, but more rows than the matrix has
    assert b"n_feat_rows" in lib.hipac_last_error()

    # X, n_feat_rows, rows, n, F, out, stream
    norms = [fake, 1000, None, 100, 512, fake, None]
    for i in (0, 5):
        assert lib.hipac_knn_inv_norms(*with_(i, None, norms)) == EINVAL
        assert b"null" in lib.hipac_last_error()
    for i, v in ((3, 0), (3, (1 << 24) + 1), (4, 510), (4, 4096), (1, 50), (0, 260)):
        assert lib.hipac_knn_inv_norms(*with_(i, v, norms)) == EINVAL, (i, v)

    # sim, idx, bank_labels, n_q, K, inv_T, class_w, scores, pred, stream
    vote = [fake, fake, fake, 100, 20, 1.0 / 0.07, fake, fake, fake, None]
    for i in (0, 1, 2, 6, 7, 8):
        assert lib.hipac_knn_vote(*with_(i, None, vote)) == EINVAL
        assert b"null" in lib.hipac_last_error()
    for i, v in ((3, 0), (4, 0), (4, 257)):
        assert lib.hipac_knn_vote(*with_(i, v, vote)) == EINVAL, (i, v)
