"""A token walker for raw DEFLATE: what a stream is made of, not only what it decodes to.

The encoder tests need to MEASURE what include/mzhip.h promises of the encoder's output -- how far back a match reaches,
which kind every block has and how many bits it takes, where BFINAL sits, how a piece ends.  An inflater cannot tell: it
accepts any distance its window holds.  walk() reads a stream token by token and returns its blocks and matches; it raises
DeflateError on everything RFC 1951 forbids.  The reader itself is tests/deflate_tokens.cpp, written from RFC 1951 alone
(it shares no code and no tables with the decoders of this project or the oracle restatement); this module compiles it
with g++ on first use, the way tests/test_kernel_emul.py builds the emulation, and needs neither a GPU nor a network.

Throughput, measured on one CPU core on zlib level-6 output of the bench corpus (3.5 MB of text, 357 000 matches): 70 - 75 MB
of output per second with the bytes reconstructed, 95 - 130 MB/s without.  The device grid of
tests/test_gpu_deflate_tokens.py is about 25 MB of output: well under a second of walking."""
import collections
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "deflate_tokens.cpp")

Block = collections.namedtuple("Block", "btype bfinal first_bit end_bit out_start out_end")
Walk = collections.namedtuple("Walk", "blocks matches bits out_len data")
Walk.__doc__ = """blocks: [Block]; matches: int64 array [n, 3] of (out_pos, length, distance), out_pos counted from the stream's
own first byte; bits: bits of input used, the final block's last bit included; out_len: bytes the stream stands for;
data: those bytes, or None when walk() was not asked for them."""


class DeflateError(ValueError):
    """the stream is not valid raw DEFLATE (RFC 1951); the message names the rule, the bit and the output position"""


_lib = None


def _load():
    global _lib
    if _lib is not None:
        return _lib
    with open(_SRC, "rb") as f:
        tag = hashlib.sha1(f.read()).hexdigest()[:12]
    name = "libdeflate_tokens_%s.so" % tag
    out = os.path.join(ROOT, "tests", "emul", "_build")
    try:
        os.makedirs(out, exist_ok=True)
        if not os.access(out, os.W_OK):
            raise OSError
    except OSError:
        out = os.path.join(tempfile.gettempdir(), "deflate_tokens_%d" % os.getuid())
        os.makedirs(out, exist_ok=True)
    so = os.path.join(out, name)
    if not os.path.exists(so):
        tmp = "%s.%d.tmp" % (so, os.getpid())
        subprocess.run(["g++", "-O2", "-std=c++14", "-shared", "-fPIC", _SRC, "-o", tmp], check=True)
        os.replace(tmp, so)          # (two processes that build at once both end with a whole file)
    L = C.CDLL(so)
    L.dt_walk.restype = C.c_void_p
    L.dt_walk.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_int, C.c_int]
    L.dt_error.restype = C.c_int
    L.dt_error.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
    L.dt_counts.restype = None
    L.dt_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.dt_fetch.restype = None
    L.dt_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dt_free.restype = None
    L.dt_free.argtypes = [C.c_void_p]
    _lib = L
    return L


def walk(z, history=0, data=False, prefix=None, open_end=False):
    """Read the raw-DEFLATE stream z up to the end of its final block -> Walk.

    history: bytes that lie in front of the stream's first byte in the same stream (a piece that is handed the bytes in front
    of it): a distance may reach that far in front of position 0 and no further.  data: also reconstruct the bytes; a stream
    with history then needs prefix = those `history` bytes.  open_end: z is a piece that is not its stream's last -- it may
    end, on a byte boundary and between two blocks, without a final block.  Bytes of z behind the final block are not looked
    at: compare Walk.bits with len(z) where that matters."""
    z = bytes(z)
    if prefix is not None:
        prefix = bytes(prefix)
        if len(prefix) != history:
            raise ValueError("prefix holds %d bytes, history is %d" % (len(prefix), history))
    if data and history and prefix is None:
        raise ValueError("the bytes of a stream with history can only be reconstructed from the history's bytes (prefix=)")
    L = _load()
    h = L.dt_walk(z, len(z), history, prefix, 1 if data else 0, 1 if open_end else 0)
    try:
        msg = C.create_string_buffer(256)
        if L.dt_error(h, msg, 256):
            raise DeflateError(msg.value.decode())
        c = (C.c_uint64 * 5)()
        L.dt_counts(h, c)
        blocks = np.zeros((c[0], 6), dtype=np.uint64)
        matches = np.zeros((c[1], 3), dtype=np.int64)
        out = np.zeros(c[2], dtype=np.uint8)
        L.dt_fetch(h, blocks.ctypes.data, matches.ctypes.data, out.ctypes.data)
    finally:
        L.dt_free(h)
    return Walk([Block(*(int(v) for v in row)) for row in blocks], matches, int(c[3]), int(c[4]), out.tobytes() if data else None)


def stored_cost_bits(nbytes):
    """what nbytes cost as stored blocks, the figure the encoder compares its Huffman blocks with (deflate_core.h, "the three
    block costs"): the bytes, 40 bits of header and LEN / NLEN per 65535 of them, and up to 7 bits of padding"""
    return 8 * nbytes + 40 * ((nbytes + 65534) // 65535) + 7


def check_encoded(z, data, window_log2, final, prefix=b"", period=None, where=(), pieces=False):
    """What include/mzhip.h and deflate_core.h promise of ONE encoded stream or piece, asserted token by token -> Walk.

    z: the encoder's bytes for `data` (prefix: the bytes in front of it in the same stream that it was allowed to match into);
    final: whether it was asked for a complete stream.  where: what to name in a failure (level, window, case ...).  pieces: z
    is several pieces behind each other (a segment of the WRITE path): every piece but the last closes with an empty stored
    block of its own.
      - z is valid raw DEFLATE, uses every one of its bytes and stands for exactly `data`;
      - every match is 3 .. 258 long and reaches at most 2^window_log2 - 262 bytes back, into the prefix or not;
      - period (an echo of synth.echo_cases: the only source lies exactly `period` back) within that bound: it is USED --
        the bound is reached, not merely avoided;
      - no block is larger than the same bytes stored; a block that stands for no byte is the closing empty stored block of
        a piece, or the one empty fixed block of an empty input;
      - final: BFINAL on the last block and on no other.  Not final: BFINAL nowhere, and the piece ends on a byte boundary in
        an empty stored block (00 00 FF FF), so that the next piece can follow."""
    max_dist = (1 << window_log2) - 262
    wk = walk(z, history=len(prefix), data=True, prefix=prefix if prefix else None, open_end=not final)
    assert wk.data == data, (where, "the stream stands for other bytes", len(wk.data), len(data))
    assert (wk.bits + 7) // 8 == len(z), (where, "bytes behind the stream's end", wk.bits, len(z))
    m = wk.matches
    if len(m):
        assert m[:, 1].min() >= 3 and m[:, 1].max() <= 258, (where, int(m[:, 1].min()), int(m[:, 1].max()))
        far = m[m[:, 2] > max_dist]
        assert len(far) == 0, (where, "%d of %d matches reach beyond %d; the first: output position %d, length %d, distance %d"
                               % (len(far), len(m), max_dist, far[0, 0], far[0, 1], far[0, 2]))
    if period is not None and period <= max_dist:
        assert len(m) and (m[:, 2] == period).any(), (where, "no match at distance %d (largest: %d of %d allowed)"
                                                      % (period, int(m[:, 2].max()) if len(m) else 0, max_dist))
    for i, b in enumerate(wk.blocks):
        n, bits = b.out_end - b.out_start, b.end_bit - b.first_bit
        if n:
            assert bits <= stored_cost_bits(n), (where, "block %d (type %d, %d bytes) takes %d bits, stored: %d" % (i, b.btype, n, bits, stored_cost_bits(n)))
        elif b.btype == 0:
            assert pieces or (not final and i == len(wk.blocks) - 1), (where, "empty stored block %d of %d" % (i, len(wk.blocks)))
        else:
            assert b.btype == 1 and bits == 10 and len(data) == 0, (where, "empty Huffman block %d of %d bits" % (i, bits))
    assert wk.blocks, where
    if final:
        assert [b.bfinal for b in wk.blocks] == [0] * (len(wk.blocks) - 1) + [1], (where, "BFINAL")
    else:
        last = wk.blocks[-1]
        assert not any(b.bfinal for b in wk.blocks), (where, "BFINAL in a piece that is not final")
        assert last.btype == 0 and last.out_start == last.out_end and wk.bits == 8 * len(z) and z[-4:] == b"\x00\x00\xff\xff", (where, z[-5:].hex())
    return wk


def check_stored_layout(wk, n, final, where=()):
    """wk: the walk of an encoder's output for n RANDOM bytes.  The encoder chooses per 64 KiB slice of its input
    (deflate_core.h): a slice of 65535 bytes or more must come out stored, as blocks of 65535 bytes (the most LEN can say) and
    the rest; a slice of one byte must not (a fixed block is cheaper); every LEN is at most 65535 by construction of the
    format -- the assert is that the split is the one the header promises."""
    want = []                      # (stored?, bytes) of every block that stands for bytes, in order
    for s0 in range(0, n, 65536):
        k = min(65536, n - s0)
        if k >= 65535:
            want += [(True, 65535)] + ([(True, k - 65535)] if k > 65535 else [])
        else:
            assert k == 1, "cases are 65535 bytes or more to a slice, or one byte"
            want.append((False, 1))
    got = [(b.btype == 0, b.out_end - b.out_start) for b in wk.blocks if b.out_end > b.out_start]
    assert got == want, (where, got, want)
