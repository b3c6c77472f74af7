"""minizip-ng_amd -- MI355X-native codec backend for minizip-ng (host-side Python binding).

The product is ``_build/libmzhip.so`` (hand-written HIP for gfx950 behind a C ABI, see
include/mzhip.h).  This module is only the thin ctypes binding used by the tests and by
bench.py; PyTorch appears solely as the owner of device memory and streams.

There is NO CPU fallback: importing works anywhere (so the C-ABI symbol checks can run
without a GPU), but every compute entry point raises if the library or a HIP device is missing.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MZHIP_LIB") or os.path.join(_HERE, "_build", "libmzhip.so")  # env: tuning builds only


_u64p, _u32p, _i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
HEADER = os.path.join(os.path.dirname(_HERE), "include", "mzhip.h")


class InflateState(C.Structure):
    """include/mzhip.h mzhip_inflate_state"""
    _fields_ = [("hdr_bit", C.c_uint32), ("bit", C.c_uint32), ("out_pos", C.c_uint32), ("flags", C.c_uint32)]


class InflateHostArgs(C.Structure):
    """include/mzhip.h mzhip_inflate_host_args (tests/test_abi.py checks the layout against the header's text)"""
    _fields_ = [("size", C.c_uint32), ("in_len", C.c_uint32), ("buf_cap", C.c_uint32), ("seg_first", C.c_uint32),
                ("seg_stride", C.c_uint32), ("seg_cap", C.c_uint32), ("in_", C.c_void_p), ("buf", C.c_void_p),
                ("state_in", C.c_void_p), ("state_out", C.c_void_p), ("out_len", C.c_void_p), ("in_used", C.c_void_p),
                ("crc", C.c_void_p), ("adler", C.c_void_p), ("seg_crc", C.c_void_p), ("nseg", C.c_void_p)]


class DeflateHostArgs(C.Structure):
    """include/mzhip.h mzhip_deflate_host_args"""
    _fields_ = [("size", C.c_uint32), ("in_len", C.c_uint32), ("final", C.c_uint32), ("out_cap", C.c_uint32),
                ("level", C.c_int32), ("window_log2", C.c_int32), ("in_", C.c_void_p), ("out", C.c_void_p),
                ("out_len", C.c_void_p), ("crc", C.c_void_p), ("adler", C.c_void_p)]


_SCALARS = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
            "int": C.c_int, "uint16_t": C.c_uint16, "uint8_t": C.c_uint8}


def header_prototypes(path=None):
    """{name: (restype, [argtypes])} of every MZHIP_API function include/mzhip.h declares -- the ONE source of the ctypes
    signatures (round 4 lost a GPU suite to a hand-written argtypes list that lagged the header by two arguments).  Every
    pointer becomes c_void_p (bytes, integers, byref() and ctypes arrays all pass), every scalar its fixed-width type."""
    import re

    text = open(path or HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"MZHIP_API\s+([^;{}()]+?)\b(mzhip_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())

        def ctype(decl, is_ret=False):
            decl = decl.strip()
            if "*" in decl:
                return C.c_char_p if is_ret and "char" in decl else C.c_void_p
            words = [w for w in decl.replace("const", " ").split() if w]
            base = words[0] if is_ret or len(words) == 1 else words[-2] if len(words) >= 2 else words[0]
            if base == "void":
                return None
            return _SCALARS[base]

        argt = [] if args in ("", "void") else [ctype(a) for a in args.split(",")]
        out[name] = (ctype(ret, True), argt)
    return out


# every function include/mzhip.h declares (tests/test_abi.py checks that the library exports them all)
BATCH_SYMBOLS = sorted(header_prototypes())


def bind(L, path=None):
    """restype / argtypes of every function the header declares, on a loaded library (libmzhip.so, the drop-in, the mock)"""
    for name, (ret, argt) in header_prototypes(path).items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype = ret
            fn.argtypes = argt
    return L


class MzHipError(RuntimeError):
    pass


def build(verbose=False):
    """Compile every HIP/C source for gfx950 into _build/libmzhip.so."""
    r = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc")], capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout[-4000:], r.stderr[-4000:])
    if r.returncode:
        raise MzHipError("libmzhip.so build failed")
    return LIB_PATH


_lib = None


def lib():
    """The loaded C-ABI library.  Raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MzHipError("%s missing: run __graft_entry__.build() / make -C minizip-ng_amd/csrc" % LIB_PATH)
        _lib = bind(C.CDLL(LIB_PATH))  # every signature from include/mzhip.h
    return _lib


def _check(rc, what):
    if rc != 0:
        raise MzHipError("%s failed (%d): %s" % (what, rc, lib().mzhip_last_error().decode()))


def require_gpu():
    import torch

    if not torch.cuda.is_available():
        raise MzHipError("no HIP device visible: the MI355X backend has no CPU fallback")
    n = lib().mzhip_device_count()
    if n <= 0:
        raise MzHipError("mzhip_device_count() = %d: %s" % (n, lib().mzhip_last_error().decode()))
    return n


def _stream_handle():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def inflate_batch(d_in, in_off, in_len, d_out, out_off, out_cap):
    """Launch K1+K2 over device-resident tensors on torch's current stream (asynchronous).

    d_in/d_out: uint8 CUDA tensors; in_off/out_off: int64; in_len/out_cap: int32 (values < 2^31).
    Returns CUDA tensors (out_len, in_used, crc [as int64-safe uint32 in int32 storage], status)."""
    import torch

    require_gpu()
    n = in_off.numel()
    dev = d_in.device
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    in_used = torch.empty(n, dtype=torch.int32, device=dev)
    crc = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    for t, dt in ((in_off, torch.int64), (out_off, torch.int64), (in_len, torch.int32), (out_cap, torch.int32)):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous()
    assert d_in.dtype == torch.uint8 and d_out.dtype == torch.uint8
    with torch.cuda.device(dev):
        _check(lib().mzhip_inflate_batch(d_in.data_ptr(), in_off.data_ptr(), in_len.data_ptr(), d_out.data_ptr(),
                                         out_off.data_ptr(), out_cap.data_ptr(), n, out_len.data_ptr(),
                                         in_used.data_ptr(), crc.data_ptr(), status.data_ptr(), _stream_handle()),
               "mzhip_inflate_batch")
    return out_len, in_used, crc, status


def crc32_batch(d_buf, off, length, init=None):
    import torch

    require_gpu()
    n = off.numel()
    crc = torch.empty(n, dtype=torch.int32, device=d_buf.device)
    with torch.cuda.device(d_buf.device):
        _check(lib().mzhip_crc32_batch(d_buf.data_ptr(), off.data_ptr(), length.data_ptr(), n,
                                       init.data_ptr() if init is not None else None, crc.data_ptr(),
                                       _stream_handle()), "mzhip_crc32_batch")
    return crc


def inflate_host(data, out_cap):
    """One entry through the host-buffer convenience entry point -> (status, in_used, out bytes, crc)."""
    require_gpu()
    out = C.create_string_buffer(max(out_cap, 1))
    src = C.create_string_buffer(bytes(data), max(len(data), 1))
    ol, iu, crc = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    a = InflateHostArgs(size=C.sizeof(InflateHostArgs), in_len=len(data), buf_cap=out_cap, in_=C.addressof(src), buf=C.addressof(out),
                        out_len=C.addressof(ol), in_used=C.addressof(iu), crc=C.addressof(crc))
    st = lib().mzhip_inflate_host_a(C.byref(a))
    return int(st), int(iu.value), out.raw[: ol.value], int(crc.value)


def bzip2_batch(d_in, in_off, in_len, d_out, out_off, out_cap):
    """ZIP method 12: one bzip2 stream per entry through mzhip_bzip2_batch on torch's current stream (asynchronous).
    Tensors as for inflate_batch; returns CUDA tensors (out_len, in_used, crc, status)."""
    import torch

    require_gpu()
    n = in_off.numel()
    dev = d_in.device
    out_len, in_used, crc, status = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    for t, dt in ((in_off, torch.int64), (out_off, torch.int64), (in_len, torch.int32), (out_cap, torch.int32)):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous()
    assert d_in.dtype == torch.uint8 and d_out.dtype == torch.uint8
    with torch.cuda.device(dev):
        _check(lib().mzhip_bzip2_batch(d_in.data_ptr(), in_off.data_ptr(), in_len.data_ptr(), d_out.data_ptr(),
                                       out_off.data_ptr(), out_cap.data_ptr(), n, out_len.data_ptr(),
                                       in_used.data_ptr(), crc.data_ptr(), status.data_ptr(), _stream_handle()),
               "mzhip_bzip2_batch")
    return out_len, in_used, crc, status


def bzip2_host(data, out_cap):
    """One bzip2 stream through the host-buffer convenience entry point -> (status, in_used, out bytes, crc)."""
    require_gpu()
    out = C.create_string_buffer(max(out_cap, 1))
    ol, iu, crc = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    st = lib().mzhip_bzip2_host(bytes(data), len(data), out, out_cap, C.byref(ol), C.byref(iu), C.byref(crc))
    return int(st), int(iu.value), out.raw[: ol.value], int(crc.value)


def zstd_batch(d_in, in_off, in_len, d_out, out_off, out_cap):
    """ZIP method 93: the Zstandard frames of each entry through mzhip_zstd_batch on torch's current stream (asynchronous).
    Tensors as for inflate_batch; returns CUDA tensors (out_len, in_used, crc, status)."""
    import torch

    require_gpu()
    n = in_off.numel()
    dev = d_in.device
    out_len, in_used, crc, status = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    for t, dt in ((in_off, torch.int64), (out_off, torch.int64), (in_len, torch.int32), (out_cap, torch.int32)):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous()
    assert d_in.dtype == torch.uint8 and d_out.dtype == torch.uint8
    with torch.cuda.device(dev):
        _check(lib().mzhip_zstd_batch(d_in.data_ptr(), in_off.data_ptr(), in_len.data_ptr(), d_out.data_ptr(),
                                      out_off.data_ptr(), out_cap.data_ptr(), n, out_len.data_ptr(),
                                      in_used.data_ptr(), crc.data_ptr(), status.data_ptr(), _stream_handle()),
               "mzhip_zstd_batch")
    return out_len, in_used, crc, status


class ZstdLargeStats(C.Structure):
    """include/mzhip.h mzhip_zstd_large_stats"""
    _fields_ = [("size", C.c_uint32), ("windows", C.c_uint32), ("blocks", C.c_uint32), ("borrowed", C.c_uint32),
                ("rounds", C.c_uint32), ("fallback", C.c_uint32)]


def zstd_large(d_in, d_out, window_bytes=0):
    """ZIP method 93, ONE large entry: the Zstandard frames in the uint8 CUDA tensor d_in decoded into d_out (its size is the
    capacity) by a wave per block through mzhip_zstd_large on torch's current stream (synchronous).  window_bytes = 0 is the
    default window.  Returns (status, out_len, in_used, crc, stats): the first four exactly what zstd_batch gives for the
    entry, stats a dict of windows, blocks, borrowed, rounds and fallback (0: decoded by waves of their own)."""
    import torch

    require_gpu()
    assert d_in.dtype == torch.uint8 and d_out.dtype == torch.uint8 and d_in.is_cuda and d_out.is_cuda
    assert d_in.is_contiguous() and d_out.is_contiguous() and d_in.numel() < 2**32 and d_out.numel() < 2**32
    ol, iu, crc, st = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_int32(0)
    stats = ZstdLargeStats(size=C.sizeof(ZstdLargeStats))
    with torch.cuda.device(d_in.device):
        _check(lib().mzhip_zstd_large(d_in.data_ptr(), d_in.numel(), d_out.data_ptr(), d_out.numel(), window_bytes, C.byref(ol),
                                      C.byref(iu), C.byref(crc), C.byref(st), C.byref(stats), _stream_handle()), "mzhip_zstd_large")
    return (int(st.value), int(ol.value), int(iu.value), int(crc.value),
            dict((k, int(getattr(stats, k))) for k in ("windows", "blocks", "borrowed", "rounds", "fallback")))


def zstd_host(data, out_cap):
    """One entry's Zstandard frames through the host-buffer convenience entry point -> (status, in_used, out bytes, crc)."""
    require_gpu()
    out = C.create_string_buffer(max(out_cap, 1))
    ol, iu, crc = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    st = lib().mzhip_zstd_host(bytes(data), len(data), out, out_cap, C.byref(ol), C.byref(iu), C.byref(crc))
    return int(st), int(iu.value), out.raw[: ol.value], int(crc.value)


def bzip2_encode_batch(d_in, in_off, in_len, d_out, out_off, out_cap, level=6):
    """ZIP method 12, the write side: one bzip2 stream per entry through mzhip_bzip2_encode_batch on torch's current stream
    (asynchronous).  Tensors as for inflate_batch; level 1..9 is the block-size digit, -1 the default 6.  The scratch is
    sized from the largest in_len (one copy of the lengths to the host).  Returns CUDA tensors (out_len, crc, status);
    crc is the CRC-32 of the input."""
    import torch

    require_gpu()
    n = in_off.numel()
    dev = d_in.device
    out_len, crc, status = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    for t, dt in ((in_off, torch.int64), (out_off, torch.int64), (in_len, torch.int32), (out_cap, torch.int32)):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous()
    assert d_in.dtype == torch.uint8 and d_out.dtype == torch.uint8
    max_in_len = int(in_len.max().item()) if n else 0
    with torch.cuda.device(dev):
        _check(lib().mzhip_bzip2_encode_batch(d_in.data_ptr(), in_off.data_ptr(), in_len.data_ptr(), max_in_len, d_out.data_ptr(),
                                              out_off.data_ptr(), out_cap.data_ptr(), n, level, out_len.data_ptr(),
                                              crc.data_ptr(), status.data_ptr(), _stream_handle()),
               "mzhip_bzip2_encode_batch")
    return out_len, crc, status


def bzip2_encode_bound(in_len, level=6):
    """mzhip_bzip2_encode_bound: an output capacity that always suffices (host arithmetic, no device needed)"""
    return int(lib().mzhip_bzip2_encode_bound(in_len, level))


def bzip2_encode_host(data, level=6):
    """One entry through the host-buffer convenience entry point -> (status, bzip2 stream, crc of the data)."""
    require_gpu()
    data = bytes(data)
    cap = max(bzip2_encode_bound(len(data), level), 1)
    out = C.create_string_buffer(cap)
    ol, crc = C.c_uint32(0), C.c_uint32(0)
    st = lib().mzhip_bzip2_encode_host(data, len(data), level, out, cap, C.byref(ol), C.byref(crc))
    return int(st), out.raw[: ol.value], int(crc.value)


def zstd_encode_batch(d_in, in_off, in_len, d_out, out_off, out_cap, level=3, checksum=False):
    """ZIP method 93, the write side: one Zstandard frame per entry through mzhip_zstd_encode_batch on torch's current stream
    (asynchronous).  Tensors as for inflate_batch; level 1..22, -1 and 0 mean 3; checksum adds the XXH64 content checksum.
    The token scratch is sized from the largest in_len (one copy of the lengths to the host).  Returns CUDA tensors
    (out_len, crc, status); crc is the CRC-32 of the input."""
    import torch

    require_gpu()
    n = in_off.numel()
    dev = d_in.device
    out_len, crc, status = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    for t, dt in ((in_off, torch.int64), (out_off, torch.int64), (in_len, torch.int32), (out_cap, torch.int32)):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous()
    assert d_in.dtype == torch.uint8 and d_out.dtype == torch.uint8
    max_in_len = int(in_len.max().item()) if n else 0
    with torch.cuda.device(dev):
        _check(lib().mzhip_zstd_encode_batch(d_in.data_ptr(), in_off.data_ptr(), in_len.data_ptr(), max_in_len, d_out.data_ptr(),
                                             out_off.data_ptr(), out_cap.data_ptr(), n, level, 1 if checksum else 0,
                                             out_len.data_ptr(), crc.data_ptr(), status.data_ptr(), _stream_handle()),
               "mzhip_zstd_encode_batch")
    return out_len, crc, status


def zstd_encode_bound(in_len):
    """mzhip_zstd_encode_bound: an output capacity that always suffices (host arithmetic, no device needed)"""
    return int(lib().mzhip_zstd_encode_bound(in_len))


def zstd_encode_host(data, level=3, checksum=False):
    """One entry through the host-buffer convenience entry point -> (status, Zstandard frame, crc of the data)."""
    require_gpu()
    data = bytes(data)
    cap = zstd_encode_bound(len(data))
    out = C.create_string_buffer(cap)
    ol, crc = C.c_uint32(0), C.c_uint32(0)
    st = lib().mzhip_zstd_encode_host(data, len(data), level, 1 if checksum else 0, out, cap, C.byref(ol), C.byref(crc))
    return int(st), out.raw[: ol.value], int(crc.value)


def crc32_host(data, value=0):
    require_gpu()
    return int(lib().mzhip_crc32_host(value, bytes(data), len(data)))


def u32(t):
    """int32-stored uint32 tensor -> numpy uint32"""
    import numpy as np

    return t.detach().cpu().numpy().view(np.uint32)
