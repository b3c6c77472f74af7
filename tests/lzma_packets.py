"""Packet programs: LZMA1 and LZMA2 streams written packet by packet, for the decoders' tests.

Every LZMA stream the decoders saw before this file came out of an encoder (liblzma, the compiled reference, our own K6),
and an optimising encoder visits a small part of the format: it never codes a rep before a distance was set, a distance
beyond the dictionary, an end marker behind length 273, LZMA2 control 0xA0, a raw chunk between two chunks that keep
their state, or a packet trained to cost 14 bytes.  Here the packets are written by hand, by a range encoder with the
adaptive model that is a plain reading of the LZMA specification, and judged by liblzma (Python's lzma).

A PROGRAM is a list of packets plus the parameters lc, lp, pb, dict_size:
    ("lit", byte)            a literal (coded against the match byte where the state asks for it)
    ("match", dist, len)     dist >= 1 (the byte distance; dist - 1 is what is coded), len 2 .. 273
    ("rep", k, len)          k = 0 .. 3
    ("shortrep",)
    ("eos", len)             the end marker: distance 0xFFFFFFFF behind any length
The writer codes illegal packets too (a rep at position 0, a distance beyond the output or the dictionary, an end marker
inside LZMA2).  expand() states the LZ semantics on its own: the bytes, and the index of the packet a decoder must refuse.

A CHUNK PROGRAM (LZMA2) is a list of chunks, ("raw", ctl, bytes) or ("lzma", ctl, packets[, (lc, lp, pb)][, opts]), ctl
any byte (an LZMA chunk's low five bits are filled in from its size).  opts: usize / csize = what the header says instead
of the truth (as a difference), tail = bytes appended inside csize, first = the coder's first byte, last_xor = damage to its
last byte, props_byte = the properties byte as written.

The families at the end return named, seeded programs; tests/test_lzma_packets.py holds the writer against liblzma and
runs them through the host emulation, tests/test_gpu_lzma_packets.py through the batch and host entry points."""
import hashlib
import random
import zlib

TOP = 1 << 24


def round_dict(d):
    """the dictionary liblzma 5.2.5 allocates: at least 4096, a multiple of 16"""
    return (max(d, 4096) + 15) & ~15


def _lz_copy(out, d, n):
    """n bytes from d + 1 back, byte by byte in effect (a copy may read what it wrote)"""
    start = len(out) - d - 1
    if d + 1 >= n:
        out += out[start:start + n]
    else:
        piece = bytes(out[start:])
        out += (piece * (n // (d + 1) + 1))[:n]


class _Rc:
    """the range encoder of the LZMA specification; norms counts the normalisations, which are the bytes a lazily
    normalising decoder has read behind its first five when it has decoded as far"""

    def __init__(self):
        self.low, self.range, self.cache, self.pending, self.out, self.norms = 0, 0xFFFFFFFF, 0, 1, bytearray(), 0
        self.lazy = 0        # normalisations in front of the last decision: the decoder has read 5 + lazy bytes behind it

    def _shift(self):
        if self.low < 0xFF000000 or self.low >= (1 << 32):
            carry = self.low >> 32
            c = self.cache
            while self.pending:
                self.out.append((c + carry) & 0xFF)
                c = 0xFF
                self.pending -= 1
            self.cache = (self.low >> 24) & 0xFF
        self.pending += 1
        self.low = (self.low & 0x00FFFFFF) << 8

    def _norm(self):
        self.lazy = self.norms
        if self.range < TOP:
            self.range = (self.range << 8) & 0xFFFFFFFF
            self._shift()
            self.norms += 1

    def bit(self, probs, i, b):
        p = probs[i]
        bound = (self.range >> 11) * p
        if b:
            self.low += bound
            self.range -= bound
            probs[i] = p - (p >> 5)
        else:
            self.range = bound
            probs[i] = p + ((2048 - p) >> 5)
        self._norm()

    def direct(self, value, n):
        for i in range(n - 1, -1, -1):
            self.range >>= 1
            if (value >> i) & 1:
                self.low += self.range
            self._norm()

    def finish(self):
        for _ in range(5):
            self._shift()
        return bytes(self.out)


class Coder:
    """model, state and reps of one LZMA coder; `out` is everything produced so far (the dictionary), dict_start where the
    dictionary begins in it (LZMA2), base the position the position bits count from"""

    def __init__(self, lc, lp, pb, out=None):
        self.out = bytearray() if out is None else out
        self.dict_start = 0
        self.base = 0
        self.set_props(lc, lp, pb)
        self.stats = dict(leave=[0] * 9, plain=0, kinds={}, lens=set(), slots=set())   # the writer's own bookkeeping of what it coded
        self.rc = None

    def set_props(self, lc, lp, pb):
        if lc + lp > 4:
            lc = lp = 0          # a header every decoder refuses: what is coded behind it does not matter
        self.lc, self.lp, self.pb = lc, lp, pb
        self.reset_state()

    def reset_state(self):
        n = lambda k: [1024] * k
        self.is_match, self.is_rep, self.g0, self.g1, self.g2, self.rep0long = n(192), n(12), n(12), n(12), n(12), n(192)
        self.slot, self.spec, self.align = n(256), n(128), n(16)
        self.len_m, self.len_r = n(2 + 128 + 128 + 256), n(2 + 128 + 128 + 256)
        self.litp = n(0x300 << (self.lc + self.lp))
        self.state, self.reps = 0, [0, 0, 0, 0]

    # ---- pieces -----------------------------------------------------------------------------------------------------
    def _pos(self):
        return len(self.out) - self.base

    def _tree(self, probs, base, nbits, sym):
        m = 1
        for i in range(nbits - 1, -1, -1):
            b = (sym >> i) & 1
            self.rc.bit(probs, base + m, b)
            m = (m << 1) | b

    def _rtree(self, probs, base, nbits, sym):
        m = 1
        for i in range(nbits):
            b = (sym >> i) & 1
            self.rc.bit(probs, base + m, b)
            m = (m << 1) | b

    def _len(self, probs, n, ps):
        self.stats["lens"].add(("match" if probs is self.len_m else "rep", n, ps))
        n -= 2
        if n < 8:
            self.rc.bit(probs, 0, 0)
            self._tree(probs, 2 + ps * 8, 3, n)
        elif n < 16:
            self.rc.bit(probs, 0, 1)
            self.rc.bit(probs, 1, 0)
            self._tree(probs, 2 + 128 + ps * 8, 3, n - 8)
        else:
            self.rc.bit(probs, 0, 1)
            self.rc.bit(probs, 1, 1)
            self._tree(probs, 2 + 256, 8, n - 16)

    def _byte_back(self, d):
        """the byte d + 1 back, 0 where the dictionary does not reach"""
        p = len(self.out) - d - 1
        return self.out[p] if p >= self.dict_start and d < len(self.out) else 0

    def _copy(self, d, n):
        o = self.out
        if d < len(o) - self.dict_start:
            _lz_copy(o, d, n)
        else:
            o.extend(bytes(n))      # an illegal copy: the decoder has stopped, the writer only has to go on

    def _kind(self, k):
        key = (self.state, k, self._pos() & ((1 << self.pb) - 1))          # (state, kind of packet, pos_state)
        self.stats["kinds"][key] = self.stats["kinds"].get(key, 0) + 1

    # ---- packets ----------------------------------------------------------------------------------------------------
    def lit(self, byte):
        rc, pos = self.rc, self._pos()
        self._kind("lit")
        rc.bit(self.is_match, self.state * 16 + (pos & ((1 << self.pb) - 1)), 0)
        prev = self.out[-1] if len(self.out) > self.dict_start else 0
        base = 0x300 * (((pos & ((1 << self.lp) - 1)) << self.lc) + (prev >> (8 - self.lc)))
        sym, i = 1, 7
        if self.state >= 7:
            mb = self._byte_back(self.reps[0])
            leave = 8
            while i >= 0:
                mbit, b = (mb >> i) & 1, (byte >> i) & 1
                rc.bit(self.litp, base + ((1 + mbit) << 8) + sym, b)
                sym = (sym << 1) | b
                i -= 1
                if mbit != b:
                    leave = 6 - i
                    break
            self.stats["leave"][leave] += 1
        else:
            self.stats["plain"] += 1
        while i >= 0:
            b = (byte >> i) & 1
            rc.bit(self.litp, base + sym, b)
            sym = (sym << 1) | b
            i -= 1
        self.out.append(byte)
        s = self.state
        self.state = 0 if s < 4 else (s - 3 if s < 10 else s - 6)

    def _dist(self, d, n):
        """d = distance - 1"""
        if d < 4:
            slot = d
        else:
            nb = d.bit_length() - 1
            slot = 2 * nb + ((d >> (nb - 1)) & 1)
        self.stats["slots"].add((min(n - 2, 3), slot))                     # (len-to-slot-tree class, slot)
        self._tree(self.slot, min(n - 2, 3) * 64, 6, slot)
        if slot >= 4:
            nb = (slot >> 1) - 1
            base = (2 | (slot & 1)) << nb
            if slot < 14:
                self._rtree(self.spec, base - slot, nb, d - base)
            else:
                self.rc.direct((d - base) >> 4, nb - 4)
                self._rtree(self.align, 0, 4, (d - base) & 15)

    def match(self, dist, n):
        rc, ps = self.rc, self._pos() & ((1 << self.pb) - 1)
        self._kind("match")
        rc.bit(self.is_match, self.state * 16 + ps, 1)
        rc.bit(self.is_rep, self.state, 0)
        self._len(self.len_m, n, ps)
        self._dist(dist - 1, n)
        self.reps = [dist - 1] + self.reps[:3]
        self.state = 7 if self.state < 7 else 10
        if dist - 1 != 0xFFFFFFFF:
            self._copy(dist - 1, n)

    def eos(self, n=2):
        self.match(1 << 32, n)

    def rep(self, k, n):
        rc, ps, s = self.rc, self._pos() & ((1 << self.pb) - 1), self.state
        self._kind("rep%d" % k)
        rc.bit(self.is_match, s * 16 + ps, 1)
        rc.bit(self.is_rep, s, 1)
        if k == 0:
            rc.bit(self.g0, s, 0)
            rc.bit(self.rep0long, s * 16 + ps, 1)
        else:
            rc.bit(self.g0, s, 1)
            if k == 1:
                rc.bit(self.g1, s, 0)
            else:
                rc.bit(self.g1, s, 1)
                rc.bit(self.g2, s, k - 2)
            r = self.reps
            r.insert(0, r.pop(k))
        self._len(self.len_r, n, ps)
        self.state = 8 if s < 7 else 11
        self._copy(self.reps[0], n)

    def shortrep(self):
        rc, ps, s = self.rc, self._pos() & ((1 << self.pb) - 1), self.state
        self._kind("shortrep")
        rc.bit(self.is_match, s * 16 + ps, 1)
        rc.bit(self.is_rep, s, 1)
        rc.bit(self.g0, s, 0)
        rc.bit(self.rep0long, s * 16 + ps, 0)
        self.state = 9 if s < 7 else 11
        self._copy(self.reps[0], 1)

    def put(self, p):
        getattr(self, p[0])(*p[1:])

    def run(self, packets):
        """code the packets -> the decoder's input position (from the first coder byte) in front of each and behind the last"""
        at = []
        for p in packets:
            at.append(5 + self.rc.norms)     # in front of a packet the decoder is exactly one normalisation behind at most
            self.put(p)
        at.append(5 + self.rc.norms)
        return at


# ---- LZMA1: method 14 and .lzma -----------------------------------------------------------------------------------------
class Program:
    def __init__(self, name, packets, lc=3, lp=0, pb=2, dict_size=1 << 16, tail=b"", first=None, cut=None, last_xor=0, note=None):
        self.name, self.packets, self.lc, self.lp, self.pb, self.dict_size = name, list(packets), lc, lp, pb, dict_size
        self.tail, self.first, self.cut, self.last_xor, self.note = tail, first, cut, last_xor, note or {}
        self._enc = None

    def props(self):
        return (self.pb * 5 + self.lp) * 9 + self.lc

    def encode(self):
        """-> (the coder's bytes, the coder with its stats, decoder positions in front of each packet)"""
        if self._enc is None:
            c = Coder(self.lc, self.lp, self.pb)
            c.rc = _Rc()
            at = c.run(self.packets)
            body = bytearray(c.rc.finish() + self.tail)
            if self.first is not None:
                body[0] = self.first
            if self.last_xor:                # damage to the coder's last byte: code != 0 behind the end marker
                body[-1] ^= self.last_xor
            if self.cut is not None:
                body = body[:self.cut]
            self._enc = (bytes(body), c, at)
        return self._enc

    def zip14(self):
        """the ZIP method-14 payload: version, props size, props, dictionary, the coder's bytes"""
        return bytes([5, 2, 5, 0, self.props()]) + self.dict_size.to_bytes(4, "little") + self.encode()[0]

    def alone(self):
        """the same as a .lzma file of unknown size, for lzma.FORMAT_ALONE"""
        return bytes([self.props()]) + self.dict_size.to_bytes(4, "little") + b"\xff" * 8 + self.encode()[0]

    def expand(self):
        return expand(self.packets, self.dict_size)

    def packet_bytes(self):
        """compressed bytes per packet, as the decoder reads them"""
        at = self.encode()[2]
        return [b - a for a, b in zip(at, at[1:])]


def expand(packets, dict_size, out=None, dict_start=0, reps=None, lzma2=False, room=None):
    """The LZ semantics, stated apart from the coder -> (bytes, verdict): verdict None = runs to its last packet, "end" =
    ended by the end marker, ("refused", i) = packet i must be refused.  Rules (liblzma 5.2.5): a rep or short rep with an
    empty dictionary is refused; a distance is valid iff distance - 1 < min(bytes in the dictionary, round_dict(dict_size));
    LZMA2: the end marker and a match past the chunk's uncompressed size (room) are refused."""
    out = bytearray() if out is None else out
    reps = [0, 0, 0, 0] if reps is None else reps
    lim = round_dict(dict_size)
    end = None if room is None else len(out) + room
    for i, p in enumerate(packets):
        if end is not None and len(out) == end:
            return out, ("surplus", i)             # the chunk's size is reached: the decoder never reads this packet
        k = p[0]
        if k == "lit":
            out.append(p[1])
            continue
        have = len(out) - dict_start
        if k == "eos":
            return out, (("refused", i) if lzma2 else "end")
        if k == "match":
            reps[:] = [p[1] - 1] + reps[:3]
            n = p[2]
        else:
            if have == 0:
                return out, ("refused", i)
            if k == "rep":
                reps.insert(0, reps.pop(p[1]))
                n = p[2]
            else:
                n = 1
        d = reps[0]
        if d >= have or d >= lim:
            return out, ("refused", i)
        if end is not None and n > end - len(out):
            return out, ("refused", i)
        _lz_copy(out, d, n)
    return out, None


# ---- LZMA2 ----------------------------------------------------------------------------------------------------------------
def _chunk_fields(ch):
    props, opts = None, {}
    for x in ch[3:]:
        if isinstance(x, dict):
            opts = x
        elif x is not None:
            props = x
    return props, opts


class ChunkProgram:
    def __init__(self, name, chunks, dict_size=1 << 16, props=(3, 0, 2), end=True, note=None):
        self.name, self.chunks, self.dict_size, self.props0, self.end, self.note = name, list(chunks), dict_size, props, end, note or {}
        self._enc = self._exp = None

    def encode(self):
        """-> (the raw LZMA2 bytes, the coder, the control class of every chunk, per chunk (offset of its coder bytes,
        decoder positions in front of its packets))"""
        if self._enc is None:
            out = bytearray()
            c = Coder(*self.props0, out=out)
            z = bytearray()
            classes, where = [], []
            for ch in self.chunks:
                ctl = ch[1]
                if ch[0] == "raw":
                    data = bytes(ch[2])
                    opts = ch[3] if len(ch) > 3 else {}
                    n = len(data) + opts.get("usize", 0)
                    z += bytes([ctl]) + ((n - 1) & 0xFFFF).to_bytes(2, "big") + data
                    if ctl == 1:
                        c.dict_start = c.base = len(out)
                    out += data
                    classes.append("raw%d" % ctl if ctl in (1, 2) else "bad")
                    where.append((len(z) - len(data), []))
                    continue
                props, opts = _chunk_fields(ch)
                if ctl >= 0xE0:
                    c.dict_start = c.base = len(out)
                if ctl >= 0xC0:
                    c.set_props(*(props or (c.lc, c.lp, c.pb)))
                elif ctl >= 0xA0:
                    c.reset_state()
                c.rc = _Rc()
                before = len(out)
                at = c.run(ch[2])
                body = c.rc.finish() + opts.get("tail", b"")
                usize = len(out) - before + opts.get("usize", 0)
                csize = len(body) + opts.get("csize", 0)
                ctl = (ctl & 0xE0) | (((usize - 1) >> 16) & 0x1F) if ctl >= 0x80 else ctl
                z += bytes([ctl]) + ((usize - 1) & 0xFFFF).to_bytes(2, "big") + ((csize - 1) & 0xFFFF).to_bytes(2, "big")
                if ctl >= 0xC0:
                    lc, lp, pb = props or (c.lc, c.lp, c.pb)
                    z.append(opts.get("props_byte", (pb * 5 + lp) * 9 + lc))
                where.append((len(z), at))
                if "first" in opts:
                    body = bytes([opts["first"]]) + body[1:]
                if "last_xor" in opts:
                    body = body[:-1] + bytes([body[-1] ^ opts["last_xor"]])
                z += body
                classes.append("%02x" % (ctl & 0xE0) if ctl >= 0x80 else "bad")
            if self.end:
                z.append(0)
            self._enc = (bytes(z), c, classes, where)
        return self._enc

    def raw(self):
        return self.encode()[0]

    def xz(self, check=1):
        return xz_frame(self.raw(), bytes(self.expand()[0]), self.dict_size, check)

    def expand(self):
        """-> (bytes, None or ("refused", chunk index, why))"""
        if self._exp is None:
            self._exp = self._expand()
        return self._exp

    def _expand(self):
        out = bytearray()
        need_props = need_dict = True
        dict_start, reps = 0, [0, 0, 0, 0]
        for i, ch in enumerate(self.chunks):
            ctl = ch[1]
            if ctl == 0:
                return out, ("end", i)
            if ctl >= 0xE0 or ctl == 1:
                need_props, need_dict = True, False
                dict_start = len(out)
            elif need_dict:
                return out, ("refused", i, "no dictionary reset")
            if ch[0] == "raw" or ctl < 0x80:
                if ctl > 2:
                    return out, ("refused", i, "control byte")
                opts = ch[3] if len(ch) > 3 else {}
                if opts.get("usize", 0):
                    return out, ("refused", i, "raw size")
                out += bytes(ch[2])
                continue
            props, opts = _chunk_fields(ch)
            if ctl >= 0xC0:
                pbyte = opts.get("props_byte")
                lc, lp, pb = props or (0, 0, 0)
                if (pbyte is not None and pbyte > 224) or (props and lc + lp > 4) or (pbyte is not None and pbyte % 9 + pbyte // 9 % 5 > 4):
                    return out, ("refused", i, "props")
                need_props = False
            elif need_props:
                return out, ("refused", i, "no props")
            if ctl >= 0xA0:
                reps = [0, 0, 0, 0]
            if opts.get("first"):
                return out, ("refused", i, "first coder byte")
            room = None
            if opts.get("usize", 0):
                room = len(expand(ch[2], self.dict_size, bytearray(out), dict_start, list(reps), True)[0]) - len(out) + opts["usize"]
            out, v = expand(ch[2], self.dict_size, out, dict_start, reps, True, room)
            if v and v[0] == "refused":
                return out, ("refused", i, "packet %d" % v[1])
            if v and v[0] == "surplus":
                return out, ("refused", i, "csize longer than the chunk needs")
            if opts.get("usize", 0) > 0:
                return out, ("refused", i, "usize beyond the packets")
            if opts.get("csize", 0) or opts.get("tail"):
                return out, ("refused", i, "csize is not what the coder reads")
            if opts.get("last_xor"):
                return out, ("refused", i, "code != 0 at the chunk's end")
        return out, (None if self.end else ("cut", len(self.chunks)))


def _vli(v):
    o = bytearray()
    while v >= 0x80:
        o.append((v & 0x7F) | 0x80)
        v >>= 7
    o.append(v)
    return bytes(o)


def _crc64(b):
    import oracle

    return oracle.crc64(b)


def lzma2_dict_byte(dict_size):
    for b in range(41):
        if (2 | (b & 1)) << (b // 2 + 11) >= dict_size:
            return b
    raise ValueError(dict_size)


def xz_frame(lzma2, data, dict_size, check=1):
    """one-block .xz around raw LZMA2 bytes (no sizes in the block header); check 0 none, 1 CRC-32, 4 CRC-64, 10 SHA-256"""
    flags = bytes([0, check])
    head = b"\xfd7zXZ\x00" + flags + zlib.crc32(flags).to_bytes(4, "little")
    bh = bytes([2, 0, 0x21, 1, lzma2_dict_byte(dict_size)]) + bytes(3)
    bh += zlib.crc32(bh).to_bytes(4, "little")
    chk = {0: b"", 1: zlib.crc32(data).to_bytes(4, "little"), 4: _crc64(data).to_bytes(8, "little") if check == 4 else b"",
           10: hashlib.sha256(data).digest()}[check]
    unpadded = len(bh) + len(lzma2) + len(chk)
    blk = bh + lzma2 + bytes(-len(lzma2) % 4) + chk
    idx = b"\x00" + _vli(1) + _vli(unpadded) + _vli(len(data))
    idx += bytes(-len(idx) % 4)
    idx += zlib.crc32(idx).to_bytes(4, "little")
    tail = (len(idx) // 4 - 1).to_bytes(4, "little") + flags
    return head + blk + idx + zlib.crc32(tail).to_bytes(4, "little") + tail + b"YZ"


# ---- helpers for length- and cost-targeted programs --------------------------------------------------------------------
def pad_to_length(make, target, lo=0, hi=4000, **kw):
    """make(n) -> packets in front of the end marker with n padding literals; the first n in lo .. hi whose compressed
    length (coder bytes) is exactly target -> Program"""
    at = Program("pad", make(hi), **kw).encode()[2]
    lo = max(lo, next((n for n in range(hi) if at[n] >= target - 40), hi) - 1, 0)
    for n in range(lo, hi):
        p = Program("pad", make(n), **kw)
        k = len(p.encode()[0])
        if k == target:
            return p
        if k > target + 8:
            break
    return None


def _flip_syms(sym, nbits, msb_first=True):
    """for each depth of a bit tree, deepest first: the symbol that follows sym's path to that depth and takes the other
    branch there (the rest zero) -- coding it trains the node on sym's path against sym"""
    outs = []
    for k in range(nbits - 1, -1, -1):
        if msb_first:
            sh = nbits - 1 - k
            outs.append(((sym >> sh) ^ 1) << sh)
        else:
            outs.append((sym & ((1 << k) - 1)) | ((((sym >> k) & 1) ^ 1) << k))
    return outs


def expensive_match(dist, n, times=100):
    """packets that train every model decision of ("match", dist, n), coded in state 10 with pb = 0, towards the other
    side -- the deepest node of every tree first, so that later training leaves it alone -- and then the match itself:
    every adaptive decision of that one packet then sits near the floor of its probability (31 / 2048: six bits each).
    n >= 18 and dist - 1 in a slot >= 14.  -> (packets, index of the expensive one)"""
    d = dist - 1
    nb = d.bit_length() - 1
    slot = 2 * nb + ((d >> (nb - 1)) & 1)
    assert n >= 18 and 14 <= slot < 32
    base = (2 | (slot & 1)) << ((slot >> 1) - 1)
    pk = [("lit", 0x55)]
    pk += [("match", 1, 273)] * ((max(dist, 70000) + 272) // 273 + 1)        # room for every distance used below
    pk += [("match", 1, 18)] * 3                                       # state 10 from here on
    for h in _flip_syms(n - 18, 8):
        pk += [("match", 1, h + 18)] * times
    pk += [("match", 1, 10)] * times                                   # choice2
    for s in _flip_syms(slot, 6):                                      # (every length >= 5 uses one slot tree; length 5 also
        pk += [("match", (s if s < 4 else (2 | (s & 1)) << ((s >> 1) - 1)) + 1, 5)] * times      # trains `choice` the other way)
    for a in _flip_syms(d & 15, 4, msb_first=False):                   # the align tree through slot 32, which leaves the slot
        pk += [("match", 65536 + a + 1, 5)] * times                    # tree at its root -- against the strike's slot < 32
    pk += [("rep", 0, 2), ("match", 1, 2)] * times                     # is_rep[10]: a rep in state 10, and back to it through 11
    for _ in range(times):                                             # is_match[10]: a literal, and back to state 10
        pk += [("lit", 0x55), ("match", 1, 2), ("match", 1, 2)]
    pk.append(("match", dist, n))
    return pk, len(pk) - 1


# ---- families -------------------------------------------------------------------------------------------------------------
FAMILIES = ("states", "lengths", "distances", "reps", "dictionary", "overlap", "literals", "slots", "window", "expensive")
_cache = {}


def _seed_bytes(rnd, n):
    return [("lit", rnd.randrange(256)) for _ in range(n)]


def _to_state(s):
    """packets that lead from state 0 (with some output) to state s"""
    L, M, R, S = ("lit", 0x41), ("match", 1, 2), ("rep", 0, 2), ("shortrep",)
    return {0: [], 1: [M, L, L], 2: [R, L, L], 3: [S, L, L], 4: [M, L], 5: [R, L], 6: [S, L], 7: [M], 8: [R], 9: [S],
            10: [M, M], 11: [M, R]}[s]


def fam_states(seed=1):
    """every edge of the state graph (12 states x 7 kinds of packet), for pb 0 .. 4 at every pos_state; behind every kind
    of match-like packet a matched literal that leaves the match tree at each of the 8 bit positions and one that never
    leaves it"""
    rnd = random.Random(seed)
    progs = []
    nexts = [("lit", 0x6B), ("match", 3, 5), ("rep", 0, 3), ("rep", 1, 4), ("rep", 2, 2), ("rep", 3, 6), ("shortrep",)]
    size = {"lit": 1, "match": 2, "rep": 2, "shortrep": 1}            # bytes the packets of _to_state produce
    for pb in range(5):
        pk = _seed_bytes(rnd, 40) + [("match", 7, 3), ("match", 11, 4), ("match", 5, 2), ("match", 9, 3), ("lit", 1), ("lit", 2), ("lit", 3)]
        pos = 40 + 12 + 3
        for ps in range(1 << pb):
            for s in range(12):
                for nx in nexts:
                    # literals (the state is 0 and stays 0) until the packets that lead to state s end at pos_state ps
                    lead = _to_state(s)
                    pad = (ps - pos - sum(size[q[0]] for q in lead)) % (1 << pb)
                    pk += _seed_bytes(rnd, pad) + lead + [nx] + _seed_bytes(rnd, 3)      # three literals: any state back to 0
                    pos += pad + sum(size[q[0]] for q in lead) + (nx[2] if len(nx) == 3 else 1) + 3
        progs.append(Program("states/edges/pb%d" % pb, pk + [("eos", 2)], lc=3, lp=0, pb=pb, note=dict(edges=True)))
    for pb in range(5):
        pk = [("lit", b) for b in (0x00, 0xFF, 0x5A, 0xA5, 0x80, 0x01, 0x7F, 0xFE)] + _seed_bytes(rnd, 24)
        for kind in ("match", "rep0", "rep1", "rep2", "rep3", "shortrep", "match+match", "match+rep"):
            for leave in range(9):
                d = rnd.randrange(1, 30)
                pre = {"match": [("match", d, 3)], "rep0": [("match", d, 2), ("lit", 7), ("rep", 0, 3)],
                       "rep1": [("match", d, 2), ("match", d + 1, 2), ("lit", 7), ("rep", 1, 2)],
                       "rep2": [("match", d, 2), ("match", d + 1, 2), ("match", d + 2, 2), ("lit", 7), ("rep", 2, 4)],
                       "rep3": [("match", d, 2), ("match", d + 1, 2), ("match", d + 2, 2), ("match", d + 3, 2), ("lit", 7), ("rep", 3, 2)],
                       "shortrep": [("match", d, 2), ("lit", 7), ("shortrep",)], "match+match": [("match", d + 4, 2), ("match", d, 2)],
                       "match+rep": [("match", d, 2), ("rep", 0, 2)]}[kind]
                pk += pre + [("mlit", leave)]
        progs.append(Program("states/leave/pb%d" % pb, _resolve_mlit(pk) + [("eos", 3)], lc=min(3 - pb % 2, 4 - pb % 3), lp=pb % 3, pb=pb, note=dict(leave=True)))
    return progs


def _resolve_mlit(packets):
    """("mlit", k): a literal whose first k bits equal the match byte's and whose next bit differs (k = 8: the byte itself)"""
    out, reps, res = bytearray(), [0, 0, 0, 0], []
    for p in packets:
        if p[0] == "mlit":
            mb = out[len(out) - reps[0] - 1]
            p = ("lit", mb if p[1] == 8 else (mb ^ (0x80 >> p[1])) & ~((0x80 >> p[1]) - 1) & 0xFF | (0x2A & ((0x80 >> p[1]) - 1)))
        res.append(p)
        out, v = expand([p], 1 << 30, out, 0, reps)
        assert v is None, p
    return res


def fam_lengths(seed=2):
    """every length 2 .. 273 through both length coders at every pos_state (pb = 4: 16 of them; pb = 0, 2): literals in
    front of every match and every rep bring the output position to the wanted residue.  Programs of at most 250 KB."""
    progs = []
    for pb in (0, 2, 4):
        head = [("lit", 0x61), ("lit", 0x62), ("lit", 0x63), ("match", 3, 30)]
        pk, pos, lo = list(head), 33, 2
        for n in range(2, 274):
            for ps in range(1 << pb):
                for what in (("match", 3, n), ("rep", 0, n)):
                    pad = (ps - pos) % (1 << pb)
                    pk += [("lit", 0x61 + (pos + j) % 3) for j in range(pad)] + [what]      # (period 3: the match of distance 3 goes on)
                    pos += pad + n
            if pos > 200000 or n == 273:
                progs.append(Program("lengths/pb%d/%d-%d" % (pb, lo, n), pk + [("eos", 273 - n % 7)], pb=pb, dict_size=1 << 20, note=dict(lengths=(pb, lo, n))))
                pk, pos, lo = list(head), 33, n + 1
    return progs


def _slot_dists(slot, rnd):
    if slot < 4:
        return [slot]
    nb = (slot >> 1) - 1
    base = (2 | (slot & 1)) << nb
    return sorted({base, base + (1 << nb) - 1, base + rnd.randrange(1 << nb), base + rnd.randrange(1 << nb)})


SLOT_CAP = 200000          # bytes of output the slot sweep builds: slots up to 34 and the low end of 35 are valid, beyond refused


def fam_distances(seed=3):
    """every slot 0 .. 63 with low, high and random footer bits, in all four len-to-slot-tree classes: accepted as far as
    SLOT_CAP bytes of output reach (into slot 35), refused twins beyond"""
    rnd = random.Random(seed)
    progs = []
    fill = [("lit", 0x30), ("lit", 0x31), ("lit", 0x32)] + [("match", 3, 273)] * (SLOT_CAP // 273)
    have = 3 + 273 * (SLOT_CAP // 273)
    ok, bad = [], []
    for slot in range(64):
        for d in _slot_dists(slot, rnd):
            if d == 0xFFFFFFFF:
                continue
            (ok if d < have else bad).append((slot, d))
    pk = list(fill)
    for i, (slot, d) in enumerate(ok):
        pk += [("match", d + 1, n) for n in (2, 3, 4, 5, (9, 40, 273)[i % 3])] + [("lit", i & 255)]      # all four slot-tree classes
    progs.append(Program("distances/slots0-35", pk + [("eos", 2)], dict_size=1 << 22, note=dict(slots=sorted({s for s, _ in ok}), bad_slots=sorted({s for s, _ in bad}))))
    for i, (slot, d) in enumerate(bad):
        if i % 2 == 0 or slot >= 62:
            progs.append(Program("distances/refused/slot%d/%d" % (slot, d), [("lit", 1), ("match", 1, 20), ("match", d + 1, 2 + i % 4)] + [("lit", 2), ("eos", 2)],
                                 dict_size=0xFFFFFFFF, note=dict(refused=2)))
    return progs


def big_programs():
    """the few named entries above 256 KiB: distance-1 runs of 1, 2 and 4 MiB with distances up to slot 43 behind them"""
    progs = []
    for mib, top in ((1, 39), (2, 41), (4, 43)):
        n = (mib << 20) // 273
        pk = [("lit", 0x77)] + [("match", 1, 273)] * n
        have = 1 + 273 * n
        for slot in range(30, top + 1):
            nb = (slot >> 1) - 1
            base = (2 | (slot & 1)) << nb
            for d in (base, min(base + (1 << nb) - 1, have - 1)):
                if d < have:
                    pk += [("match", d + 1, 4), ("lit", slot)]
        progs.append(Program("distances/run%dMiB" % mib, pk + [("eos", 2)], dict_size=1 << 23, note=dict(top=top)))
    return progs


def fam_reps(seed=4):
    import itertools

    rnd = random.Random(seed)
    progs = []
    pk = _seed_bytes(rnd, 64)
    for perm in itertools.product((0, 1, 2, 3), repeat=3):
        pk += [("match", 5, 2), ("match", 17, 3), ("match", 29, 2), ("match", 43, 4)]
        for k in perm:
            pk += [("rep", k, 2 + k), ("lit", rnd.randrange(256))]
        pk += [("shortrep",), ("lit", rnd.randrange(256))]
    progs.append(Program("reps/queue", pk + [("eos", 2)]))
    for k in range(4):          # reps before anything was set: all four are distance 1
        progs.append(Program("reps/unset/rep%d" % k, [("lit", 0x21), ("rep", k, 5), ("lit", 0x22), ("rep", 3, 2), ("shortrep",), ("eos", 2)]))
        progs.append(Program("reps/refused/pos0/rep%d" % k, [("rep", k, 2), ("lit", 1), ("eos", 2)], note=dict(refused=0)))
    progs.append(Program("reps/refused/pos0/shortrep", [("shortrep",), ("lit", 1), ("eos", 2)], note=dict(refused=0)))
    # (rep0 valid but rep3 stale and beyond the output cannot be coded: a distance is checked when a match sets it, the output
    # only grows, and whatever resets the dictionary resets the reps.)  An old, far rep3 that is still valid, used and unused:
    pre = _seed_bytes(rnd, 8) + [("match", 8, 273)] * 20 + [("match", 5000, 2), ("match", 3, 2), ("match", 4, 2), ("match", 5, 2)]
    progs.append(Program("reps/far-rep3/unused", pre + [("rep", 0, 2), ("rep", 1, 2), ("rep", 2, 2), ("lit", 9), ("eos", 2)], dict_size=8192))
    progs.append(Program("reps/far-rep3/used-small-dict", [p if p[0] != "match" or p[1] != 5000 else ("match", 4096, 2) for p in pre]
                         + [("rep", 3, 2), ("eos", 2)], dict_size=4096))
    return progs


DICT_SIZES = (0, 1, 100, 4095, 4096, 4097, 4100, 65536, 65537)


def fam_dictionary(seed=5):
    """header dictionary sizes x distances at the rounded size, one below, one above x match, rep0 .. 3, short rep.  A
    distance is coded first by a match (refused there when it is too far), so the rep forms of a too-far distance are the
    match's; the rep forms of the valid ones follow the match."""
    rnd = random.Random(seed)
    progs = []
    for ds in DICT_SIZES:
        lim = round_dict(ds)
        fill = _seed_bytes(rnd, 7) + [("match", 7, 273)] * ((lim + 40) // 273 + 1)
        for what, dist in (("at", lim), ("below", lim - 1), ("above", lim + 1)):
            for use in ("match", "rep0", "rep1", "rep2", "rep3", "shortrep"):
                pk = list(fill) + [("match", dist, 3)]
                if use == "rep0":
                    pk += [("lit", 5), ("rep", 0, 4)]
                elif use == "shortrep":
                    pk += [("lit", 5), ("shortrep",), ("mlit", 3)]
                elif use != "match":
                    k = int(use[3])
                    pk += [("match", 2, 2)] * k + [("lit", 5), ("rep", k, 3), ("mlit", 8)]
                bad = dist > lim
                pk = _resolve_mlit(pk) if not bad else [q if q[0] != "mlit" else ("lit", 0) for q in pk]
                progs.append(Program("dictionary/%d/%s/%s" % (ds, what, use), pk + [("lit", 6), ("eos", 2)], dict_size=ds,
                                     note=dict(refused=len(fill)) if bad else {}))
    return progs


def fam_overlap(seed=6):
    """dist 1 .. 70 x lengths 2, 63 .. 65, 127 .. 129, 272, 273, every copy started at every output offset mod 64 (a literal
    or one match of distance 67 in front brings the position there); two copies in three are matches, the third a rep0
    behind a two-byte match that sets the distance.  Two distances to a program: about 180 KB each."""
    rnd = random.Random(seed)
    progs = []
    lens = (2, 63, 64, 65, 127, 128, 129, 272, 273)
    for first in range(1, 71, 2):
        pk = _seed_bytes(rnd, 70)
        j, have = 0, 70
        for dist in (first, first + 1):
            for n in lens:
                for off in range(64):
                    as_rep = j % 3 == 0
                    want = (off - have - (2 if as_rep else 0)) % 64
                    pk += [("match", 67, want)] if want >= 2 else _seed_bytes(rnd, want)
                    pk += [("match", dist, 2), ("rep", 0, n)] if as_rep else [("match", dist, n)]
                    have += want + n + (2 if as_rep else 0)
                    j += 1
        progs.append(Program("overlap/dist%d-%d" % (first, first + 1), pk + [("eos", 2)], dict_size=1 << 20, note=dict(dists=(first, first + 1))))
    return progs


def out_cap_cases(seed=7):
    """(program, out_cap, status, out_len): copies that end exactly at out_cap, are cut one byte short (-200), a literal
    and a short rep at out_cap (-200)"""
    rnd = random.Random(seed)
    cases = []
    for dist, n in ((1, 273), (3, 64), (64, 65), (70, 128), (5, 2), (200, 129)):
        pre = [("lit", rnd.randrange(128)) for _ in range(200 + dist % 7)]       # four literal contexts: the slot build keeps the entry
        for tail, short, name in (([("match", dist, n)], 0, "exact"), ([("match", dist, n)], 1, "cut1"), ([("match", dist, n)], n - 1, "cut-all-but-1"),
                                  ([("match", dist, n), ("lit", 3)], 1, "lit-at-cap"), ([("match", dist, n), ("shortrep",)], 1, "shortrep-at-cap"),
                                  ([("match", dist, 2), ("rep", 0, n)], 1, "rep-cut1")):
            p = Program("overlap/cap/%s/d%dn%d" % (name, dist, n), pre + tail + [("eos", 2)])
            full = len(p.expand()[0])
            cases.append((p, full - short, -200 if short else 0, full - short))
    return cases


def fam_literals(seed=8):
    """every legal (lc, lp); with lc + lp = 4 plain and matched literals in both halves of the model; positions that flip
    the lp bits"""
    rnd = random.Random(seed)
    progs = []
    for lc in range(9):
        for lp in range(5):
            if lc + lp > 4:
                continue
            pk = []
            for i in range(160):
                b = rnd.randrange(256) if i % 4 else (i * 37) & 255
                pk.append(("lit", b))                    # previous bytes with every top nibble, at every position mod 16
                if i % 5 == 4:
                    pk += [("match", 1 + i % 4, 2), ("mlit", i % 9)]
                if i % 11 == 10:
                    pk += [("shortrep",), ("mlit", (i + 3) % 9), ("lit", 0xF0 | i & 15), ("match", 2, 2), ("mlit", 8), ("lit", 0x0F & i)]
            progs.append(Program("literals/lc%dlp%d" % (lc, lp), _resolve_mlit(pk) + [("eos", 2)], lc=lc, lp=lp, pb=(lc + lp) % 5, note=dict(lclp=lc + lp)))
    for props in ((8, 0, 0), (4, 1, 2), (0, 5, 0), (3, 2, 4)):      # refused by the header
        progs.append(Program("literals/refused/lc%dlp%d" % props[:2], [("lit", 1), ("eos", 2)], lc=props[0], lp=props[1], pb=props[2], note=dict(refused="header")))
    return progs


def _ctx_byte(c, i=0):
    """a byte whose top three bits are c (lc = 3: the literal context of the next byte)"""
    return (c << 5) | (i & 31)


def swap_program(name, contexts, n, matches_first=0, every=1, dist=1 << 16):
    """n literals whose contexts (lc = 3, lp = 0) rotate through `contexts`; every > 1: a distance-1 match of every - 1
    bytes behind each, so that one context is new per `every` bytes of output -- and each such literal is a matched one
    right behind the swap; matches_first bytes of distance-1 run in front"""
    pk = [("lit", _ctx_byte(contexts[0]))]
    if matches_first:
        pk += [("match", 1, 273)] * (matches_first // 273)
    for i in range(n):
        pk.append(("lit", _ctx_byte(contexts[(i + 1) % len(contexts)], i)))
        if every > 1:
            left = every - 1
            while left:
                k = min(left, 273) if left - min(left, 273) != 1 else 272
                pk.append(("match", 1, k))
                left -= k
    return Program(name, pk + [("eos", 2)], lc=3, lp=0, pb=2, dict_size=dist)


def fam_slots(seed=9):
    """K3's slot build: 4 contexts in rotation (4 swaps in all), 5 in rotation (a swap on every literal: given back at the
    65th), swap rates just under and over one per 128 bytes behind 0, 10 000 and 100 000 bytes of matches, matched
    literals right behind a swap.  note: swaps = what the slot build must count, back = whether it gives the entry back,
    back_at = the output position of the literal it stops in front of."""
    progs = []
    p = swap_program("slots/rot4", (0, 1, 2, 3), 400)
    p.note = dict(swaps=4, back=False)
    progs.append(p)
    p = swap_program("slots/rot5", (0, 1, 2, 3, 4), 400)
    p.note = dict(back=True, swaps=65, back_at=65)     # the first two literals share context 0; from then on literal i, at output
                                                       # position i, swaps: the 65th swap at position 65 > 64 + (65 >> 7)
    progs.append(p)
    for first, every_over in ((0, 120), (10000, 112), (100000, 64)):
        m = first // 273 * 273
        for over, every in ((0, 129), (1, every_over)):
            # the allowance is 64 + one per 128 bytes: at one new context per `every` bytes it is crossed -- if ever -- behind
            # t bytes of them, t / every > 64 + (m + t) / 128
            t = int((64 + m / 128.0) / (1.0 / every - 1.0 / 128)) if over else 130000
            q = swap_program("slots/rate-%s/after%d" % ("over" if over else "under", first), (0, 1, 2, 3, 4), t // every + 40, matches_first=first, every=every)
            q.note = dict(back=bool(over), late=m + t if over else None)
            progs.append(q)
    return progs


def predict_slots(program):
    """what LZ_LITERAL_SITE_SLOT does with a program, restated: four slots, least recently used out, a give-back when the
    swap count exceeds 64 + (opos >> 7) -> (gave back, swaps, output position at the give-back or None)"""
    out, reps = bytearray(), [0, 0, 0, 0]
    tags, age, swaps = [None] * 4, [0] * 4, 0
    lc, lp = program.lc, program.lp
    for p in program.packets:
        if p[0] == "lit":
            opos = len(out)
            cx = ((opos & ((1 << lp) - 1)) << lc) + ((out[-1] if out else 0) >> (8 - lc))
            if cx in tags:
                k = tags.index(cx)
            else:
                k = min(range(4), key=lambda j: (age[j], j))
                tags[k] = cx
                swaps += 1
                if swaps > 64 + (opos >> 7):
                    return True, swaps, opos
            age[k] = opos + 1
        out, v = expand([p], program.dict_size, out, 0, reps)
        if v:
            break
    return False, swaps, None


def fam_window(seed=10):
    """compressed lengths 9 + 256 k + r (whole payload), k 0 .. 3, r in 0, 1, 2, 3, 4, 255: the refill of the 256-byte input
    window and its zero-padded tail on every residue; code != 0 behind the marker and a non-zero first coder byte (refused)"""
    rnd = random.Random(seed)
    progs = []
    seedlits = [rnd.randrange(256) for _ in range(5000)]
    for k in range(4):
        for r in (0, 1, 2, 3, 4, 255):
            target = 256 * k + r               # coder bytes: the payload's first nine are the header
            if target < 6:
                continue                       # the shortest coder run (five bytes and the end marker's) is longer
            for el in (2, 273):
                p = pad_to_length(lambda n: [("lit", b) for b in seedlits[:n]] + [("match", 1, 2)] * (n > 0) + [("eos", el)], target)
                if p is not None:
                    p.name = "window/len%d+%d/eos%d" % (256 * k, r, el)
                    progs.append(p)
                    break
    base = [("lit", b) for b in seedlits[:300]] + [("match", 9, 40), ("eos", 5)]
    progs.append(Program("window/refused/code-nonzero", base, last_xor=0x40, note=dict(refused="code")))
    progs.append(Program("window/refused/first-byte", base, first=1, note=dict(refused="first")))
    return progs


def prefix_programs(seed=11):
    """three short programs (at most 300 compressed bytes each); the tests cut them at every length"""
    rnd = random.Random(seed)
    a = _seed_bytes(rnd, 60) + [("match", 7, 30), ("rep", 0, 5), ("shortrep",), ("lit", 3), ("match", 50, 273), ("eos", 2)]
    b = [("lit", 0x41)] + [("match", 1, 273)] * 5 + _seed_bytes(rnd, 100) + [("match", 1400, 9), ("rep", 1, 10), ("eos", 273)]
    c = _seed_bytes(rnd, 230) + [("eos", 17)]
    return [Program("window/prefix/a", a, lc=0, lp=2, pb=0), Program("window/prefix/b", b), Program("window/prefix/c", c, lc=4, lp=0, pb=4)]


def fam_expensive(seed=12):
    """packets trained to cost as many compressed bytes as the model allows (expensive_match); an untrained end marker of
    length 273 closes each program, behind 90 literals (more than 64 bytes of input behind the trained packet)"""
    rnd = random.Random(seed)
    progs = []
    for dist, n in ((65535, 273), (49153 + 0x2AAA, 18 + 0x55), (32768 + 0x1555, 100), (40000, 273)):
        pk, at = expensive_match(dist, n)
        progs.append(Program("expensive/d%dn%d" % (dist, n), pk + _seed_bytes(rnd, 90) + [("eos", 273)], lc=3, lp=0, pb=0, dict_size=1 << 20, note=dict(strike=at)))
    return progs


def family(name):
    if name not in _cache:
        _cache[name] = {"states": fam_states, "lengths": fam_lengths, "distances": fam_distances, "reps": fam_reps,
                        "dictionary": fam_dictionary, "overlap": fam_overlap, "literals": fam_literals, "slots": fam_slots,
                        "window": fam_window, "expensive": fam_expensive}[name]()
    return _cache[name]


def all_programs():
    return [p for f in FAMILIES for p in family(f)]


def accepted():
    """[(program, bytes)] of the programs liblzma accepts"""
    key = "accepted"
    if key not in _cache:
        _cache[key] = [(p, bytes(p.expand()[0])) for p in all_programs() if "refused" not in p.note]
    return _cache[key]


def refused():
    return [p for p in all_programs() if "refused" in p.note]


# ---- LZMA2 chunk families -----------------------------------------------------------------------------------------------
def _run_chunk(n):
    """packets of a distance-1 run of n bytes (n >= 2)"""
    n -= 1
    pk = [("lit", 0x52)]
    while n > 0:
        k = min(n, 273)
        if n - k == 1:
            k -= 1
        pk.append(("match", 1, k) if k >= 2 else ("lit", 0x52))
        n -= k
    return pk


def chunk_programs(seed=20):
    """-> [ChunkProgram]; the verdicts are expand()'s, held against liblzma by the tests"""
    if "chunks" in _cache:
        return _cache["chunks"]
    rnd = random.Random(seed)
    P = []
    text = _seed_bytes(rnd, 40) + [("match", 5, 9), ("lit", 0x33), ("rep", 0, 3)]
    first = ("lzma", 0xE0, text, (3, 0, 2))
    # every control byte as first chunk and as second chunk (LZMA chunks with five low bits k hold k * 64 KiB + 1 bytes)
    for ctl in range(256):
        k = ctl & 0x1F
        for place in ("first", "second"):
            if ctl == 0:
                ch = []
            elif ctl < 0x80:
                ch = [("raw", ctl, bytes(rnd.randrange(256) for _ in range(1 + ctl % 50)))]
            else:
                legal = ctl >= 0xE0 if place == "first" else True
                if k and not legal:
                    body = text                   # refused by its control byte: the size bits need no bytes behind them
                else:
                    body = _run_chunk((k << 16) + 1) if k else text
                ch = [("lzma", ctl, body, (2, 1, 1) if ctl >= 0xC0 else None, {"usize": (k << 16)} if k and not legal else {})]
            chunks = ([first] if place == "second" else []) + ch
            P.append(ChunkProgram("chunks/ctl/%s/%02x" % (place, ctl), chunks, dict_size=1 << 16))
    # legal and illegal sequences of dictionary reset / props / state reset
    lz = lambda ctl, props=None: ("lzma", ctl, _seed_bytes(rnd, 12) + [("match", 3, 4), ("shortrep",)], props)
    raw = lambda ctl, n=20: ("raw", ctl, bytes(rnd.randrange(256) for _ in range(n)))
    seqs = [[lz(0xE0, (3, 0, 2)), lz(0x80), lz(0xA0), lz(0xC0, (0, 2, 1)), lz(0x80), lz(0xE0, (1, 1, 1)), lz(0xA0)],
            [raw(1), lz(0xC0, (3, 0, 2)), lz(0x80), raw(2), lz(0x80), raw(2), lz(0xA0), raw(1), lz(0xE0, (2, 2, 0))],
            [raw(1), raw(2), raw(1), raw(2)], [raw(1), lz(0x80)], [raw(1), lz(0xA0)], [raw(2)], [lz(0xC0, (3, 0, 2))], [lz(0x80)],
            [lz(0xE0, (3, 0, 2)), raw(1), lz(0x80)], [lz(0xE0, (3, 0, 2)), raw(1), lz(0xA0)], [lz(0xE0, (3, 0, 2)), raw(1), lz(0xC0, (3, 0, 2))],
            [lz(0xE0, (3, 0, 2)), raw(2), lz(0xA0), raw(2), lz(0x80)]]
    for i, s in enumerate(seqs):
        P.append(ChunkProgram("chunks/sequence/%d" % i, s))
    # a props change in mid-block to every legal (lc, lp, pb), and to lc + lp > 4
    lits = _seed_bytes(rnd, 30)
    for lc in range(9):
        for lp in range(5):
            for pb in range(5):
                if lc + lp > 4 and pb:
                    continue
                body = lits + [("match", 4, 6)] + _seed_bytes(rnd, 10) + [("shortrep",), ("lit", 0xEE)]
                P.append(ChunkProgram("chunks/props/lc%dlp%dpb%d" % (lc, lp, pb), [first, ("lzma", 0xC0, body, (lc, lp, pb))]))
    P.append(ChunkProgram("chunks/props/byte225", [first, ("lzma", 0xC0, lits, (0, 0, 0), {"props_byte": 225})]))
    # a dictionary reset in mid-block, then a distance that reaches its first byte, and one that reaches one byte further
    for ctl2, mk in ((0xE0, lambda pk: ("lzma", 0xE0, pk, (3, 0, 2))), (1, None)):
        for odd in (37, 48):            # bytes in front of the reset: the position bits restart with the dictionary
            pre = ("lzma", 0xE0, _seed_bytes(rnd, odd - 9) + [("match", 2, 9)], (3, 0, 2))
            for reach in (0, 1):
                if mk:
                    body = _seed_bytes(rnd, 21) + [("match", 21 + reach, 5), ("lit", 1)]
                    ch = [pre, mk(body)]
                else:
                    ch = [pre, ("raw", 1, bytes(rnd.randrange(256) for _ in range(21))), ("lzma", 0xC0, [("match", 21 + reach, 5), ("lit", 1)], (3, 0, 2))]
                P.append(ChunkProgram("chunks/dict-reset/%02x/after%d/%s" % (ctl2, odd, "beyond" if reach else "first-byte"), ch))
    # a stale rep3 behind a dictionary reset is impossible (a reset of the dictionary resets the reps with the state);
    # a raw chunk between two chunks that keep their state: the next packet a matched literal, a short rep, a rep0
    for nxt in ("mlit", "shortrep", "rep0", "rep3"):
        for n in (1, 2, 50):
            a = ("lzma", 0xE0, _seed_bytes(rnd, 30) + [("match", 7, 3), ("match", 9, 2), ("match", 11, 2), ("match", 2, 3)], (3, 0, 2))
            rawb = bytes(rnd.randrange(256) for _ in range(n))
            tail = {"mlit": [("lit", rawb[-2] ^ 0x08 if n > 1 else 0x99)], "shortrep": [("shortrep",)], "rep0": [("rep", 0, 7)], "rep3": [("rep", 3, 4)]}[nxt]
            P.append(ChunkProgram("chunks/raw-between/%s/raw%d" % (nxt, n), [a, ("raw", 2, rawb), ("lzma", 0x80, tail + [("lit", 4), ("shortrep",)])]))
    # chunks of usize 1, the largest usize, the largest csize
    P.append(ChunkProgram("chunks/usize1", [("lzma", 0xE0, [("lit", 0x40)], (3, 0, 2))] + [("lzma", 0x80, [("shortrep",)])] * 5 + [("raw", 2, b"x"), ("lzma", 0x80, [("lit", 0x41)]), ("lzma", 0xA0, [("lit", 0x42)])]))
    P.append(ChunkProgram("chunks/usize-max", [("lzma", 0xE0, _run_chunk(1 << 21), (3, 0, 2)), ("lzma", 0x80, [("rep", 0, 273)])], dict_size=1 << 22))
    big = []
    c = Coder(0, 0, 0)
    c.rc = _Rc()
    lrnd = random.Random(seed + 1)
    while len(c.rc.out) < 65536 - 12:           # literals that always take the improbable side of every decision they can
        b, sym = 0, 1
        for i in range(8):
            bit = 1 if c.litp[sym] >= 1024 else 0
            if c.litp[sym] == 1024:
                bit = lrnd.randrange(2)
            b = (b << 1) | bit
            sym = (sym << 1) | bit
        c.lit(b)
        big.append(("lit", b))
    while True:
        q = ChunkProgram("chunks/csize-max", [("lzma", 0xE0, big, (0, 0, 0))], dict_size=1 << 16)
        n = len(q.raw()) - 7             # the chunk's csize: everything but the six header bytes and the end byte
        if n >= 65536:
            if n == 65536:
                break
            big.pop()
        else:
            big.append(("lit", lrnd.randrange(256)))
    P.append(q)
    # a match crossing chunk_end, an end marker inside a chunk, csize one more / one less, code != 0 at the chunk's end
    body = _seed_bytes(rnd, 20) + [("match", 6, 10)]
    P.append(ChunkProgram("chunks/refused/match-crosses-end", [("lzma", 0xE0, body, (3, 0, 2), {"usize": -1})]))
    P.append(ChunkProgram("chunks/refused/usize+1", [("lzma", 0xE0, body, (3, 0, 2), {"usize": 1})]))
    P.append(ChunkProgram("chunks/refused/eos-inside", [("lzma", 0xE0, body + [("eos", 2)], (3, 0, 2))]))
    P.append(ChunkProgram("chunks/refused/eos-last", [first, ("lzma", 0x80, [("lit", 1), ("eos", 9)])]))
    P.append(ChunkProgram("chunks/refused/csize+1", [("lzma", 0xE0, body, (3, 0, 2), {"csize": 1, "tail": b"\0"}), lz(0x80)]))
    P.append(ChunkProgram("chunks/refused/csize-1", [("lzma", 0xE0, body, (3, 0, 2), {"csize": -1}), lz(0x80)]))
    P.append(ChunkProgram("chunks/refused/first-byte", [("lzma", 0xE0, body, (3, 0, 2), {"first": 1})]))
    P.append(ChunkProgram("chunks/refused/code-nonzero", [("lzma", 0xE0, body, (3, 0, 2), {"last_xor": 0x40}), lz(0x80)]))
    P.append(ChunkProgram("chunks/refused/raw-ctl3", [first, ("raw", 3, b"abc")]))
    _cache["chunks"] = P
    return P
