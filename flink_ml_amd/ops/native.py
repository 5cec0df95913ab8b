"""Loader for the in-tree native libraries (ctypes, flat C ABI).

The HIP kernels are plain ``extern "C"`` launchers that take device pointers and a
``hipStream_t``; we launch them onto torch's *current* HIP stream, so they order correctly
with torch ops and RCCL collectives and can be captured into a hipGraph
(``torch.cuda.CUDAGraph``) together with them. Every entry point's ctypes signature comes
from its C definition (``build.api_signatures``, carried in the build manifest): nothing
describes the ABI a second time in Python.

Debugging: ``FMLX_SYNC_CHECK=1`` synchronises the device after every native launch and reports an
asynchronous fault under the name of the kernel that caused it (the HIP analogue of a blocking
launch mode; slow, off by default).

Policy: on a GPU host the native library is REQUIRED — ``kernels()`` raises if it is
missing (no silent eager fallback). On CPU-only hosts the ops layer runs its torch reference
implementation (same semantics, fp64), which is what the CPU test-suite exercises.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch  # noqa: F401  (must be imported first: our .so binds to torch's libamdhip64.so.7)

from . import build as _build

_LOCK = threading.Lock()
_KLIB = None
_HLIB = None
# one-time cost of loading every code object of the kernel library at library load (host ms;
# None: not done — no GPU, or FMLX_PRELOAD=0), and the number of code objects
PRELOAD_MS = None
PRELOAD_OBJECTS = 0
BKT_LIMITS = None  # the bucket round's compile-time limits (ops/glm.py _bkt_limits), read at load
PRELOAD_STAGES = {}  # ms per stage of the library load (code objects, pinned blocks, dry launches, pool)

DT_F32, DT_F64, DT_BF16, DT_F16, DT_I32, DT_I64 = 0, 1, 2, 3, 4, 5

_TORCH2DT = {
    torch.float32: DT_F32,
    torch.float64: DT_F64,
    torch.bfloat16: DT_BF16,
    torch.float16: DT_F16,
    torch.int32: DT_I32,
    torch.int64: DT_I64,
}


def _bind(lib, api) -> None:
    """Sets argtypes / restype of every entry point of ``lib`` from ``api`` (build.api_signatures:
    derived from the C definitions; an entry point the library lacks is an error)."""
    for name, (restype, argtypes) in api.items():
        fn = getattr(lib, name)
        fn.argtypes = [getattr(ctypes, a) for a in argtypes]
        fn.restype = restype and getattr(ctypes, restype)


def gpu_available() -> bool:
    from ..parallel.context import get_context

    return get_context().device.type == "cuda"


def kernel_lib_path() -> str:
    return _build.KERNEL_LIB


def kernels():
    """The HIP kernel library (raises if missing: never a silent fallback on GPU)."""
    global _KLIB
    if _KLIB is not None:
        return _KLIB
    with _LOCK:
        if _KLIB is None:
            path = _build.KERNEL_LIB
            if not os.path.exists(path):
                if os.environ.get("FMLX_AUTOBUILD", "1") == "1":
                    _build.build_kernels()
                else:
                    raise RuntimeError("native kernel library missing: %s (run python -m flink_ml_amd.ops.build)" % path)
            api = _build.check_fresh("kernels")  # never load a binary built from other sources
            lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
            _bind(lib, api or _build.api_signatures("kernels"))  # (no manifest record: built by hand)
            _preload(lib)
            _KLIB = lib
    return _KLIB


def _preload(lib) -> None:
    """Loads every code object of the library now (one empty anchor-kernel launch per
    translation unit, csrc/common.h FMLX_DEFINE_PRELOAD) instead of lazily inside the first fit
    that launches one of its kernels; the one-time cost goes to PRELOAD_MS."""
    global PRELOAD_MS, PRELOAD_OBJECTS
    if os.environ.get("FMLX_PRELOAD", "1") == "0" or not torch.cuda.is_available():
        return
    import time

    t0 = time.perf_counter()
    k = lib.fmlx_preload_all(torch.cuda.current_stream().cuda_stream)
    PRELOAD_MS = (time.perf_counter() - t0) * 1e3
    PRELOAD_STAGES["code_objects"] = round(PRELOAD_MS, 2)
    if k < 0:
        raise RuntimeError("preloading the kernel library's code objects failed (%d)" % k)
    from ..utils import hostsync

    t1 = time.perf_counter()
    hostsync.warm(torch.cuda.current_device())  # pinned read-back block + first-use imports
    PRELOAD_STAGES["pinned_readback"] = round((time.perf_counter() - t1) * 1e3, 2)
    t1 = time.perf_counter()
    # every sparse-round kernel launched once, dry
    if lib.fmlx_glm_sparse_warm(torch.cuda.current_stream().cuda_stream) != 0:
        raise RuntimeError("warming the sparse round kernels failed")
    torch.cuda.current_stream().synchronize()
    PRELOAD_STAGES["sparse_warm_launches"] = round((time.perf_counter() - t1) * 1e3, 2)
    torch.cuda.get_device_properties(torch.cuda.current_device())  # (first call: runtime queries)
    # the bucket round's compile-time limits, read here (a first fit paid ~50 µs for the first call
    # of the entry point); through ``lib``: kernels() holds its lock until this returns
    global BKT_LIMITS
    import numpy as np

    lim = np.zeros(8, dtype=np.int32)
    lib.fmlx_glm_bkt_limits(lim.ctypes.data)
    BKT_LIMITS = lim
    # one device segment for torch's caching allocator, freed at once: the trainers' buffers of a
    # first fit are then carved out of it instead of each new size paying a hipMalloc inside the fit
    # (a fresh hipMalloc is tens to hundreds of µs of GPU-idle host time)
    pool = int(os.environ.get("FMLX_DEVICE_POOL_MB", "2048")) << 20
    t1 = time.perf_counter()
    if pool > 0:
        seg = torch.empty(pool, dtype=torch.uint8, device=torch.cuda.current_device())
        del seg
    PRELOAD_STAGES["device_pool"] = round((time.perf_counter() - t1) * 1e3, 2)
    PRELOAD_MS = (time.perf_counter() - t0) * 1e3
    PRELOAD_OBJECTS = k


def host():
    """The host-side C++ runtime library (hashing, caches, sketches)."""
    global _HLIB
    if _HLIB is not None:
        return _HLIB
    with _LOCK:
        if _HLIB is None:
            # FMLX_HOST_LIB: an alternative build of the host runtime (the ASan/UBSan one in tests)
            path = os.environ.get("FMLX_HOST_LIB") or _build.HOST_LIB
            if not os.path.exists(path):
                _build.build_host()
            api = _build.check_fresh("host") if path == _build.HOST_LIB else None
            lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
            _bind(lib, api or _build.api_signatures("host"))  # (no manifest record, or FMLX_HOST_LIB)
            _HLIB = lib
    return _HLIB


def zeros(shape, dtype, device) -> torch.Tensor:
    """``torch.zeros`` on the GPU through the library's own (preloaded) fill kernel: torch's fill
    kernels load their code object lazily on first use (tens of ms inside a fit)."""
    t = torch.empty(shape, dtype=dtype, device=device)
    nbytes = t.numel() * t.element_size()
    if t.device.type != "cuda":
        return t.zero_()
    if nbytes % 4:
        return t.zero_()
    call("fmlx_fill32", t.data_ptr(), nbytes // 4, 0, stream_ptr(t.device))
    return t


def zeros_many(specs, device):
    """Several zero-filled device tensors carved out of ONE allocation with ONE fill launch (each
    launch from Python costs ~15 µs of host time that a short fit's GPU idles through): ``specs`` =
    [(shape, dtype), ...] → list of tensors (256-byte aligned views)."""
    offs, total = [], 0
    for shape, dtype in specs:
        n = 1
        for x in (shape if isinstance(shape, (tuple, list)) else (shape,)):
            n *= int(x)
        es = torch.empty(0, dtype=dtype).element_size()
        offs.append((total, n, dtype, shape))
        total += -(-max(1, n * es) // 256) * 256
    blob = zeros((total // 4,), torch.int32, device)
    raw = blob.view(torch.uint8)
    out = []
    for off, n, dtype, shape in offs:
        es = torch.empty(0, dtype=dtype).element_size()
        out.append(raw[off:off + n * es].view(dtype).reshape(shape))
    return out


def fill_i32(t: torch.Tensor, value: int) -> torch.Tensor:
    """In-place fill of a contiguous int32 CUDA tensor (library kernel)."""
    call("fmlx_fill32", t.data_ptr(), t.numel(), int(value) & 0xFFFFFFFF, stream_ptr(t.device))
    return t


def ptr(t) -> int:
    if t is None:
        return None
    return t.data_ptr()


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def dtype_code(dtype: torch.dtype) -> int:
    return _TORCH2DT[dtype]


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError("HIP launch %s failed with error %d" % (what, rc))


SYNC_CHECK = os.environ.get("FMLX_SYNC_CHECK", "0") == "1"


def call(name: str, *args) -> None:
    rc = getattr(kernels(), name)(*args)
    check(rc, name)
    if SYNC_CHECK and torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            raise RuntimeError("native kernel %s failed asynchronously: %s" % (name, e)) from e
