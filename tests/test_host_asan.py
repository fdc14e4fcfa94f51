"""CPU: the host side of the C-ABI library under AddressSanitizer (build.py --asan): argument checks, workspace plans,
the Pillow coefficient restatement and the training parameter table run in a child python with the ASan runtime
preloaded; any heap / stack / global overflow in that host code aborts the child."""
import os
import subprocess
import sys
import textwrap

import pytest

from ss25_hierarchical_multiscale_image_classification_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = textwrap.dedent("""
    import ctypes as C, sys
    import numpy as np
    sys.path.insert(0, %r)
    from ss25_hierarchical_multiscale_image_classification_amd import capi
    lib = capi.load_library(%r)
    for P in (224, 448, 896, 1792):
        ks = lib.hipac_resample_coeffs(P, 224, None, None, 0)
        assert ks > 0
        b = np.zeros((224, 2), np.int32); k = np.zeros((224, ks), np.int32)
        assert lib.hipac_resample_coeffs(P, 224, b.ctypes.data, k.ctypes.data, ks) == ks
        assert lib.hipac_resample_coeffs(P, 224, b.ctypes.data, k.ctypes.data, ks - 1) < 0  # table too narrow: refused
    n = lib.hipac_train_num_convs()
    for i in range(n):
        co, ci, ks_, st = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        po, so = C.c_int64(), C.c_int64()
        assert lib.hipac_train_conv_desc(i, C.byref(co), C.byref(ci), C.byref(ks_), C.byref(st), C.byref(po), C.byref(so)) == 0
    assert lib.hipac_train_conv_desc(n, None, None, None, None, None, None) != 0
    assert lib.hipac_train_param_floats() == 11176512
    for batch in (1, 7, 512, 4096):
        assert lib.hipac_train_workspace_bytes(batch) > 0
        for prec in (0, 1, 2):
            assert lib.hipac_resnet18_workspace_bytes(batch, prec) > 0
    assert lib.hipac_train_debug_offset(4, 1, 19) > 0 and lib.hipac_train_debug_offset(4, 9, 0) == -1
    for batch in (1, 7, 512, 2048):
        assert lib.hipac_train_amp_workspace_bytes(batch) > 0
    assert lib.hipac_train_amp_debug_offset(4, 1, 19) > 0 and lib.hipac_train_amp_debug_offset(4, 9, 0) == -1
    assert lib.hipac_train_amp_debug_offset(4, 0, 20) == -1 and lib.hipac_train_amp_debug_offset(0, 0, 0) == -1
    hb, db, cb = C.c_size_t(), C.c_size_t(), C.c_size_t()
    for W, H in ((5000, 4000), (225, 224), (100000, 100000)):
        for P in (448, 896, 1792):
            assert lib.hipac_level_planes_sizes(W, H, P, C.byref(hb), C.byref(db), C.byref(cb)) == 0 and db.value > 0
    assert lib.hipac_level_planes_sizes(5000, 4000, 100, C.byref(hb), C.byref(db), C.byref(cb)) != 0
    assert b"P 100" in lib.hipac_last_error()
    assert lib.hipac_ntxent_scratch_bytes(1024, 128) > 0
    # null / out-of-range arguments are answered with error codes before anything touches a device
    assert lib.hipac_resnet18_forward(None, None, 4, 0, None, None, None, None, 0, None) != 0
    assert lib.hipac_train_encoder_forward(None, None, None, 4, 0.1, 1e-5, None, None, 0, None) != 0
    assert lib.hipac_train_amp_encoder_forward(None, None, None, 4, 0.1, 1e-5, None, None, 0, None) != 0
    assert b"train_amp_forward: null argument" in lib.hipac_last_error()
    assert lib.hipac_adam_step(None, None, None, None, 10, 1e-3, 0.9, 0.999, 1e-8, 1, None) != 0
    assert lib.hipac_resnet18_pack(None, 0, None) != 0
    assert b"pack: null argument" in lib.hipac_last_error()
    params, handle = capi.ResNet18Params(), C.c_void_p()
    params.num_classes = 2  # fc_w stays NULL
    assert lib.hipac_resnet18_pack(C.byref(params), 0, C.byref(handle)) != 0 and not handle.value
    assert b"pack: fc_w / num_classes mismatch" in lib.hipac_last_error()
    print("asan drive ok")
""")


def test_host_code_under_address_sanitizer():
    try:
        rt = build.asan_runtime()
    except RuntimeError as e:
        pytest.skip(str(e))
    lib = build.build_asan()
    env = dict(os.environ, LD_PRELOAD=str(rt), ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    r = subprocess.run([sys.executable, "-c", DRIVER % (ROOT, str(lib))], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "asan drive ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr
