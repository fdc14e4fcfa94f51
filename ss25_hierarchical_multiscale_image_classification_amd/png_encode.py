"""ctypes binding of include/hipac_png.h: windows of a resident level image encoded to PNG files on the device
(csrc/png_encode.hip).  ``encode_windows`` is one or more ``hipac_png_encode_windows`` calls, batched so that the output
buffer stays under a fixed budget; ``iter_encoded`` hands the files of every batch to the host as bytes."""
from __future__ import annotations

import ctypes as C

import numpy as np

PNG_ABI_VERSION = 1  # include/hipac_png.h HIPAC_PNG_ABI_VERSION this binding was written against
PNG_BAND_BYTES, PNG_MAX_P, PNG_MAX_WINDOWS = 24576, 1792, 4096  # HIPAC_PNG_BAND_BYTES, HIPAC_PNG_MAX_P, HIPAC_PNG_MAX_WINDOWS
PNG_OUT_BUDGET = 1 << 30  # bytes of output buffer per batch: 111 windows at P = 1792
# name -> (restype, argtypes); must list every symbol include/hipac_png.h declares (tests/test_png_capi_symbols.py)
PNG_SYMBOLS = {
    "hipac_png_abi_version": (C.c_int, []),
    "hipac_png_file_bound": (C.c_size_t, [C.c_int]),
    "hipac_png_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "hipac_png_encode_windows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                           C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}

_png_bound = None


def load_png_library():
    """The library of ``capi.load_library()`` with the PNG entry points bound; HipacError on a version mismatch."""
    global _png_bound
    from . import capi

    lib = capi.load_library()
    if _png_bound is not lib:
        _png_bound = capi.bind_symbols(lib, PNG_SYMBOLS, "hipac_png_abi_version", PNG_ABI_VERSION, "PNG ABI")
    return lib


def out_stride(P: int) -> int:
    """Bytes between two files of an output buffer: the file bound rounded up to 256."""
    from . import capi

    bound = int(load_png_library().hipac_png_file_bound(int(P)))
    if bound == 0:
        raise capi.HipacError(f"PNG windows of side {P} are not encoded on the device (1 .. {PNG_MAX_P})")
    return (bound + 255) // 256 * 256


def batch_windows(P: int, budget: int = PNG_OUT_BUDGET) -> int:
    """Windows per call: as many as keep the output buffer within ``budget``, at least one, at most PNG_MAX_WINDOWS."""
    return max(1, min(PNG_MAX_WINDOWS, int(budget) // out_stride(P)))


def _encode_batch(lib, level_tensor, W, H, xy_dev, P, stride):
    import torch

    from . import capi

    n = int(xy_dev.shape[0])
    dev = level_tensor.device
    need = int(lib.hipac_png_workspace_bytes(P, n))
    out = torch.empty(n * stride, dtype=torch.uint8, device=dev)
    sizes = torch.empty(n, dtype=torch.int64, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    capi._check(lib.hipac_png_encode_windows(level_tensor.data_ptr(), int(W), int(H), int(level_tensor.stride(0)), xy_dev.data_ptr(), n,
                                             int(P), out.data_ptr(), stride, sizes.data_ptr(), ws.data_ptr(), need, capi._stream()),
                "hipac_png_encode_windows")
    return out, sizes


def _prepare(level_tensor, xy):
    import torch

    from . import capi

    capi._require_gpu(level_tensor)
    if level_tensor.dtype != torch.uint8 or level_tensor.dim() != 3 or level_tensor.shape[2] != 3 or level_tensor.stride(2) != 1 \
            or level_tensor.stride(1) != 3:
        raise capi.HipacError("png_encode: the level must be uint8[H, Wpad, 3] with packed pixels")
    xy = torch.as_tensor(np.ascontiguousarray(np.asarray(xy.cpu() if hasattr(xy, "cpu") else xy, np.int32).reshape(-1, 2)))
    return xy


def iter_encoded(level_tensor, W: int, H: int, xy, P: int, budget: int = PNG_OUT_BUDGET):
    """Yield ``(first window index, [bytes of every file])`` batch by batch.  One copy per batch brings the used bytes of the
    output buffer to the host (everything up to the end of the last file), not the bound."""
    import torch

    xy = _prepare(level_tensor, xy)
    n = int(xy.shape[0])
    if n == 0:
        return
    lib = load_png_library()
    stride, per = out_stride(P), batch_windows(P, budget)
    with torch.cuda.device(level_tensor.device):
        for lo in range(0, n, per):
            out, sizes = _encode_batch(lib, level_tensor, W, H, xy[lo:lo + per].to(level_tensor.device), int(P), stride)
            sz = sizes.cpu().numpy()  # waits for the stream
            # compact on the device: file i's used bytes go behind file i - 1's, so the copy carries no slack
            offs = np.concatenate([[0], np.cumsum(sz)]).astype(np.int64)
            packed = torch.cat([out[i * stride:i * stride + int(s)] for i, s in enumerate(sz)]).cpu().numpy().tobytes()
            yield lo, [packed[offs[i]:offs[i + 1]] for i in range(len(sz))]


def encode_windows(level_tensor, W: int, H: int, xy, P: int):
    """PNG files of the P x P windows at ``xy`` (int32 [n, 2], any position: outside the level is white) of the resident level
    ``level_tensor`` (uint8[H, Wpad, 3] on the device, W x H pixels).  Returns ``(uint8 device buffer, int64 sizes)``: file i is
    ``buffer[i * stride : i * stride + sizes[i]]`` with ``stride = buffer.numel() // n``.  Calls are sized so that no
    call's own output exceeds PNG_OUT_BUDGET; the buffers of the calls are joined."""
    import torch

    xy = _prepare(level_tensor, xy)
    n = int(xy.shape[0])
    stride, per = out_stride(P), batch_windows(P)
    dev = level_tensor.device
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
    lib = load_png_library()
    outs, sizes = [], []
    with torch.cuda.device(dev):
        for lo in range(0, n, per):
            o, s = _encode_batch(lib, level_tensor, W, H, xy[lo:lo + per].to(dev), int(P), stride)
            outs.append(o)
            sizes.append(s)
        return (outs[0], sizes[0]) if len(outs) == 1 else (torch.cat(outs), torch.cat(sizes))
