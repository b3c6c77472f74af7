"""A bzip2 stream writer (and reader) made from the format, in the line of token_programs.py and lzma_packets.py: given
block contents it does the first run-length stage, the BWT (a plain sort: the blocks are small), move-to-front and
RUNA/RUNB, and codes the symbols with caller-chosen tables and selectors.  Every field no compressor varies has a switch
(block(...) / write_stream(...)), so that the decoders (minizip-ng_amd/csrc/bzip2_core.h on the host and on the device) can
be held against libbz2 -- Python's bz2 -- on streams bz2.compress never writes.  PROGRAMS is the shared list of program
families; judge() is libbz2's verdict on a stream, read_stream() this module's own reader half.

Format, bits MSB-first: "BZh" level; per block 48-bit magic 0x314159265359, block CRC (32), randomised (1), origPtr (24),
symbol map (16 + 16 per used group), nGroups (3), nSelectors (15), selectors (unary, move-to-front), code lengths per
table (5-bit start, then per symbol 1x = change: 10 +1 / 11 -1, 0 = done), the symbols; at the end 0x177245385090 and
the combined CRC (32)."""
import bz2
import heapq

BLOCK_MAGIC = 0x314159265359
END_MAGIC = 0x177245385090
RUNA, RUNB = 0, 1
OK, DATA_ERROR, BUF_ERROR, OUT_FULL, UNSUPPORTED = 0, -3, -5, -200, -109

_CRC = []
for _i in range(256):
    _c = _i << 24
    for _ in range(8):
        _c = ((_c << 1) ^ 0x04C11DB7 if _c & 0x80000000 else _c << 1) & 0xFFFFFFFF
    _CRC.append(_c)


def block_crc(data):
    c = 0xFFFFFFFF
    for b in data:
        c = ((c << 8) & 0xFFFFFFFF) ^ _CRC[(c >> 24) ^ b]
    return c ^ 0xFFFFFFFF


def rotl1(v):
    return ((v << 1) | (v >> 31)) & 0xFFFFFFFF


class Bits:
    def __init__(self):
        self.chunks, self.v, self.k, self.n, self.marks = [], 0, 0, 0, []

    def put(self, nbits, value):
        assert 0 <= value < (1 << nbits), (nbits, value)
        self.v = (self.v << nbits) | value
        self.k += nbits
        self.n += nbits
        while self.k >= 8:
            self.k -= 8
            self.chunks.append((self.v >> self.k) & 255)
        self.v &= (1 << self.k) - 1

    def mark(self, name):
        self.marks.append((name, self.n))

    def bytes(self):
        tail = [(self.v << (8 - self.k)) & 255] if self.k else []
        return bytes(self.chunks + tail)


def rle1(data):
    """the first run-length stage: four equal bytes, then a count byte of 0..251 further ones (a run of 255 at most)"""
    out, i, n = bytearray(), 0, len(data)
    while i < n:
        j = i
        while j < n and data[j] == data[i] and j - i < 255:
            j += 1
        out += bytes([data[i]]) * min(j - i, 4)
        if j - i >= 4:
            out.append(j - i - 4)
        i = j
    return bytes(out)


def unrle1(pre):
    """what a block of these bytes decodes to; None when it ends in four equal bytes without a count"""
    out, i, n = bytearray(), 0, len(pre)
    while i < n:
        c, run = pre[i], 1
        i += 1
        while run < 4 and i < n and pre[i] == c:
            run += 1
            i += 1
        if run == 4:
            if i == n:
                return None
            run += pre[i]
            i += 1
        out += bytes([c]) * run
    return bytes(out)


def bwt(pre):
    n = len(pre)
    idx = sorted(range(n), key=lambda i: pre[i:] + pre[:i])
    return bytes(pre[i - 1] for i in idx), idx.index(0) if n else 0


def mtf_symbols(last, used):
    """move-to-front positions over the used byte values, zero runs in bijective base 2 (RUNA = 1, RUNB = 2), then end of block"""
    lst, out, run = list(used), [], 0

    def flush():
        nonlocal run
        while run > 0:
            if run & 1:
                out.append(RUNA)
                run = (run - 1) // 2
            else:
                out.append(RUNB)
                run = (run - 2) // 2

    for b in last:
        p = lst.index(b)
        if p == 0:
            run += 1
        else:
            flush()
            out.append(p + 1)
            lst.insert(0, lst.pop(p))
    flush()
    out.append(len(used) + 1)
    return out


def ibwt(last, orig):
    """the bytes in front of the BWT, from its last column: a stable counting sort gives the links, the walk starts at orig"""
    n = len(last)
    starts, tot = [0] * 256, 0
    for b in range(256):
        starts[b], tot = tot, tot + last.count(b)
    tt = [0] * n
    for i, b in enumerate(last):
        tt[starts[b]] = (i << 8) | b
        starts[b] += 1
    pre, p = bytearray(), orig
    for _ in range(n):
        pre.append(tt[p] & 255)
        p = tt[p] >> 8
    return bytes(pre)


def symbols_to_final(syms, used, orig, cap=900000):
    """what a block of these symbols decodes to (None: it does not), so that a hand-made symbol sequence gets its CRC"""
    lst, last, i, eob = list(used), bytearray(), 0, len(used) + 1
    while i < len(syms) and syms[i] != eob:
        if syms[i] <= 1:
            es, weight = 0, 1
            while i < len(syms) and syms[i] <= 1:
                es += weight << syms[i]
                weight <<= 1
                i += 1
            if len(last) + es > cap:
                return None
            last += bytes([lst[0]]) * es
        else:
            lst.insert(0, lst.pop(syms[i] - 1))
            last.append(lst[0])
            i += 1
    if len(last) > cap or orig >= len(last):
        return None
    return unrle1(ibwt(last, orig))


def huffman_lengths(freq, max_len=20):
    """a complete length set for freq (all counted as >= 1), no code longer than max_len"""
    f = [max(int(x), 1) for x in freq]
    while True:
        heap = [(w, i, (i,)) for i, w in enumerate(f)]
        heapq.heapify(heap)
        lens, tick = [0] * len(f), len(f)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                lens[s] += 1
            heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
            tick += 1
        if max(lens) <= max_len:
            return [max(x, 1) for x in lens]
        f = [x // 2 + 1 for x in f]


def decode_tables(lens):
    """limit / base / perm as libbz2 computes them from a length set, complete or not"""
    lo, hi = min(lens), max(lens)
    perm = [j for l in range(lo, hi + 1) for j, x in enumerate(lens) if x == l]
    base = [0] * 24
    for x in lens:
        base[x + 1] += 1
    for i in range(1, 23):
        base[i] += base[i - 1]
    limit, vec = [0] * 24, 0
    for i in range(lo, hi + 1):
        vec += base[i + 1] - base[i]
        limit[i] = vec - 1
        vec <<= 1
    for i in range(lo + 1, hi + 1):
        base[i] = ((limit[i - 1] + 1) << 1) - base[i]
    return lo, limit, base, perm


def code_of(lens, sym):
    """(bits, value) that libbz2's decoder turns into sym under this length set"""
    _, _, base, perm = decode_tables(lens)
    return lens[sym], perm.index(sym) + base[lens[sym]]


def block(data=None, **kw):
    """One block.  data: the bytes it decodes to.  Switches: pre (the bytes behind the first run-length stage, instead of
    data), magic, crc, randomised, orig_ptr, used (byte values flagged in the symbol map; a superset of those that occur),
    n_groups (the 3-bit field), tables (length sets, one per group written), selectors (group per 50 symbols),
    n_selectors (the 15-bit field), sel_unary (the unary counts as written, instead of move-to-front coding selectors),
    symbols (the symbol sequence, instead of MTF + RUNA/RUNB of the BWT; no end of block unless it holds one)."""
    d = dict(kw)
    d["data"] = data
    return d


def _write_block(w, blk):
    pre = blk["pre"] if blk.get("pre") is not None else rle1(blk["data"] or b"")
    final = unrle1(pre) or b""
    last, orig = bwt(pre)
    used = sorted(blk["used"]) if blk.get("used") is not None else sorted(set(pre))
    if blk.get("symbols") is not None and used:
        final = symbols_to_final(blk["symbols"], used, blk.get("orig_ptr", orig)) or b""
    crc = blk.get("crc", block_crc(final))
    w.mark("block_magic")
    w.put(48, blk.get("magic", BLOCK_MAGIC))
    w.mark("block_crc")
    w.put(32, crc)
    w.mark("randomised")
    w.put(1, blk.get("randomised", 0))
    w.mark("orig_ptr")
    w.put(24, blk.get("orig_ptr", orig))
    w.mark("map16")
    groups = sorted({b >> 4 for b in used})
    w.put(16, sum(1 << (15 - g) for g in groups))
    for g in groups:
        w.mark("map")
        w.put(16, sum(1 << (15 - (b & 15)) for b in used if b >> 4 == g))
    if not used:
        return crc, False
    alpha = len(used) + 2
    syms = blk["symbols"] if blk.get("symbols") is not None else mtf_symbols(last, used)
    tables = blk.get("tables")
    if tables is None:
        freq = [0] * alpha
        for s in syms:
            freq[s] += 1
        tables = [huffman_lengths(freq)] * 2
    n_groups = blk.get("n_groups", len(tables))
    selectors = blk["selectors"] if blk.get("selectors") is not None else [0] * ((len(syms) + 49) // 50)
    w.mark("n_groups")
    w.put(3, n_groups)
    w.mark("n_selectors")
    w.put(15, blk.get("n_selectors", len(selectors)))
    w.mark("selectors")
    if blk.get("sel_unary") is not None:
        unary = blk["sel_unary"]
    else:
        lst, unary = list(range(8)), []
        for s in selectors:
            p = lst.index(s)
            unary.append(p)
            lst.insert(0, lst.pop(p))
    for j in unary:
        w.put(j + 1, ((1 << j) - 1) << 1)
    for lens in tables:
        w.mark("table")
        curr = lens[0]
        w.put(5, curr)
        for x in lens:
            while curr != x:
                w.put(2, 2 if x > curr else 3)
                curr += 1 if x > curr else -1
            w.put(1, 0)
        if not all(1 <= x <= 20 for x in lens):
            return crc, False   # the decoder stops at the length that is out of range
    w.mark("symbols")
    for i, s in enumerate(syms):
        bits, value = code_of(tables[selectors[min(i // 50, len(selectors) - 1)]], s)
        w.put(bits, value)
    return crc, True


def write_stream(blocks, level=9, head=b"BZh", end_magic=END_MAGIC, combined=None, trailing=b"", marks=False):
    """blocks: block(...) specs.  level: the digit (or any byte value as an int below 10, or a raw byte as bytes).
    -> the stream (and, with marks, the (field, bit offset) list)"""
    w = Bits()
    for ch in head:
        w.put(8, ch)
    w.mark("level")
    w.put(8, level[0] if isinstance(level, bytes) else 0x30 + level)
    comb, whole = 0, True
    for blk in blocks:
        crc, whole = _write_block(w, blk)
        comb = rotl1(comb) ^ crc
        if not whole:
            break
    if whole:
        w.mark("end_magic")
        w.put(48, end_magic)
        w.mark("combined_crc")
        w.put(32, comb if combined is None else combined)
    else:
        w.put(64, 0)
    w.mark("end")
    out = w.bytes() + trailing
    return (out, w.marks) if marks else out


# ---- the reader half: the same format read back, libbz2's order of checks ---------------------------------------------------

class _Stop(Exception):
    def __init__(self, status):
        self.status = status


class _Reader:
    def __init__(self, data):
        self.d, self.pos, self.acc, self.cnt = data, 0, 0, 0

    def get(self, n):
        while self.cnt < n:
            if self.pos >= len(self.d):
                raise _Stop(BUF_ERROR)
            self.acc = ((self.acc << 8) | self.d[self.pos]) & 0xFFFFFFFFFF
            self.pos += 1
            self.cnt += 8
        self.cnt -= n
        return (self.acc >> self.cnt) & ((1 << n) - 1)


def read_stream(data):
    """-> (status, bytes of the blocks that checked out, in_used)"""
    r, out = _Reader(bytes(data)), bytearray()
    try:
        for ch in b"BZh":
            if r.get(8) != ch:
                raise _Stop(DATA_ERROR)
        level = r.get(8) - 0x30
        if not 1 <= level <= 9:
            raise _Stop(DATA_ERROR)
        cap, comb = 100000 * level, 0
        while True:
            first = r.get(8)
            if first == 0x17:
                for ch in b"\x72\x45\x38\x50\x90":
                    if r.get(8) != ch:
                        raise _Stop(DATA_ERROR)
                stored = 0
                for _ in range(4):
                    stored = (stored << 8) | r.get(8)
                return (OK if stored == comb else DATA_ERROR), bytes(out), r.pos
            for ch, want in zip([first] + [None] * 5, b"\x31\x41\x59\x26\x53\x59"):
                if (r.get(8) if ch is None else ch) != want:
                    raise _Stop(DATA_ERROR)
            stored = 0
            for _ in range(4):
                stored = (stored << 8) | r.get(8)
            if r.get(1):
                raise _Stop(UNSUPPORTED)
            orig = 0
            for _ in range(3):
                orig = (orig << 8) | r.get(8)
            if orig > 10 + cap:
                raise _Stop(DATA_ERROR)
            m16 = r.get(16)
            used = []
            for g in range(16):
                if (m16 >> (15 - g)) & 1:
                    m = r.get(16)
                    used += [16 * g + j for j in range(16) if (m >> (15 - j)) & 1]
            if not used:
                raise _Stop(DATA_ERROR)
            alpha = len(used) + 2
            n_groups = r.get(3)
            if not 2 <= n_groups <= 6:
                raise _Stop(DATA_ERROR)
            n_sel = r.get(15)
            if n_sel < 1:
                raise _Stop(DATA_ERROR)
            lst, sels = list(range(6)), []
            for i in range(n_sel):
                j = 0
                while r.get(1):
                    j += 1
                    if j >= n_groups:
                        raise _Stop(DATA_ERROR)
                if i < 18002:
                    lst.insert(0, lst.pop(j))
                    sels.append(lst[0])
            tabs = []
            for _ in range(n_groups):
                curr, lens = r.get(5), []
                for _ in range(alpha):
                    while True:
                        if not 1 <= curr <= 20:
                            raise _Stop(DATA_ERROR)
                        if not r.get(1):
                            break
                        curr += -1 if r.get(1) else 1
                    lens.append(curr)
                tabs.append(decode_tables(lens))
            state = dict(g=-1, left=0)

            def sym():
                if state["left"] == 0:
                    state["g"] += 1
                    if state["g"] >= len(sels):
                        raise _Stop(DATA_ERROR)
                    state["left"] = 50
                state["left"] -= 1
                zn, limit, base, perm = tabs[sels[state["g"]]]
                z = r.get(zn)
                while True:
                    if zn > 20:
                        raise _Stop(DATA_ERROR)
                    if z <= limit[zn]:
                        break
                    zn += 1
                    z = (z << 1) | r.get(1)
                if not 0 <= z - base[zn] < 258:
                    raise _Stop(DATA_ERROR)
                return perm[z - base[zn]]

            mtf, last, eob = list(used), bytearray(), len(used) + 1
            s = sym()
            while s != eob:
                if s <= 1:
                    es, weight = 0, 1
                    while s <= 1:
                        if weight >= 2 * 1024 * 1024:
                            raise _Stop(DATA_ERROR)
                        es += weight << s
                        weight <<= 1
                        s = sym()
                    if len(last) + es > cap:
                        raise _Stop(DATA_ERROR)
                    last += bytes([mtf[0]]) * es
                else:
                    if len(last) >= cap:
                        raise _Stop(DATA_ERROR)
                    mtf.insert(0, mtf.pop(s - 1))
                    last.append(mtf[0])
                    s = sym()
            n = len(last)
            if orig >= n:
                raise _Stop(DATA_ERROR)
            final = unrle1(ibwt(last, orig))
            if final is None or block_crc(final) != stored:
                raise _Stop(DATA_ERROR)
            out += final
            comb = rotl1(comb) ^ stored
    except _Stop as e:
        return e.status, bytes(out), r.pos


def judge(stream):
    """libbz2's verdict: (status, bytes, in_used); bytes and in_used are None unless the status is 0"""
    d = bz2.BZ2Decompressor()
    try:
        out = d.decompress(bytes(stream))
    except OSError:
        return DATA_ERROR, None, None
    if not d.eof:
        return BUF_ERROR, None, None
    return OK, out, len(stream) - len(d.unused_data)


# ---- the program families ------------------------------------------------------------------------------------------------------

def _text(n, seed=1):
    import random
    rnd = random.Random(seed)
    words = [bytes(rnd.randrange(97, 123) for _ in range(rnd.randrange(2, 9))) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + b" "
    return bytes(out[:n])


def _flat(alpha, n):
    return [n] * alpha


def programs():
    """[(name, stream, expected status or None)]: None = libbz2 alone decides (it always does; a given status is what the
    writer claims, and test_bzip2_blocks.py holds the claim against libbz2).  Randomised blocks claim UNSUPPORTED: the
    one documented deviation."""
    T = _text(700)
    P = []

    def add(name, stream, want=None):
        P.append((name, stream, want))

    add("plain", write_stream([block(T)]), OK)
    add("empty_stream", write_stream([]), OK)
    add("two_blocks", write_stream([block(T[:300]), block(T[300:])]), OK)
    add("trailing", write_stream([block(T)], trailing=b"trailing bytes \x31\x41"), OK)
    for lv in (1, 5):
        add("level_%d" % lv, write_stream([block(T)], level=lv), OK)
    add("level_0", write_stream([block(T)], level=0), DATA_ERROR)
    add("level_colon", write_stream([block(T)], level=b":"), DATA_ERROR)
    add("head_BZx", write_stream([block(T)], head=b"BZx"), DATA_ERROR)
    add("head_bZh", write_stream([block(T)], head=b"bZh"), DATA_ERROR)
    add("block_magic", write_stream([block(T, magic=BLOCK_MAGIC ^ 0x100)]), DATA_ERROR)
    add("block_magic_first", write_stream([block(T, magic=BLOCK_MAGIC ^ (1 << 44))]), DATA_ERROR)
    add("end_magic", write_stream([block(T)], end_magic=END_MAGIC ^ 1), DATA_ERROR)
    add("block_crc", write_stream([block(T, crc=block_crc(T) ^ 1)]), DATA_ERROR)
    add("block_crc_second", write_stream([block(T[:300]), block(T[300:], crc=5)]), DATA_ERROR)
    add("combined_crc", write_stream([block(T)], combined=block_crc(T) ^ 0x80000000), DATA_ERROR)
    add("randomised", write_stream([block(T, randomised=1)]), UNSUPPORTED)
    n_pre = len(rle1(T))
    add("orig_ptr_other", write_stream([block(T, orig_ptr=3)]), DATA_ERROR)          # a valid walk of other bytes: block CRC
    add("orig_ptr_last", write_stream([block(T, orig_ptr=n_pre - 1)]))
    add("orig_ptr_nblock", write_stream([block(T, orig_ptr=n_pre)]), DATA_ERROR)
    add("orig_ptr_cap", write_stream([block(T, orig_ptr=900011)]), DATA_ERROR)
    add("orig_ptr_cap_level1", write_stream([block(T, orig_ptr=100011)], level=1), DATA_ERROR)
    add("map_empty", write_stream([block(T, used=[])]), DATA_ERROR)
    add("map_superset", write_stream([block(T, used=sorted(set(T) | {0, 1, 128, 255}))]), OK)
    add("map_all", write_stream([block(T, used=range(256))]), OK)
    add("all_bytes", write_stream([block(bytes(range(256)) * 3)]), OK)
    # groups and selectors
    alpha = len(set(rle1(T))) + 2
    flat = _flat(alpha, 8 if alpha <= 256 else 9)
    six = [flat, [7] * 2 + [9] * (alpha - 2)] + [flat] * 4
    syms_t = mtf_symbols(bwt(rle1(T))[0], sorted(set(rle1(T))))
    n50 = (len(syms_t) + 49) // 50
    add("six_groups", write_stream([block(T, tables=six, selectors=[i % 6 for i in range(n50)])]), OK)
    add("n_groups_1", write_stream([block(T, n_groups=1)]), DATA_ERROR)
    add("n_groups_7", write_stream([block(T, n_groups=7)]), DATA_ERROR)
    add("n_groups_0", write_stream([block(T, n_groups=0)]), DATA_ERROR)
    add("n_selectors_0", write_stream([block(T, n_selectors=0)]), DATA_ERROR)
    add("selectors_short", write_stream([block(T, selectors=[0] * (n50 - 1))]))       # running out of selectors
    add("selectors_spare", write_stream([block(T, selectors=[0, 1] * n50)]), OK)
    add("selector_value_nGroups", write_stream([block(T, sel_unary=[2] + [0] * (n50 - 1), n_selectors=n50)]), DATA_ERROR)
    add("selector_value_6", write_stream([block(T, tables=six, sel_unary=[6] + [0] * (n50 - 1), n_selectors=n50)]), DATA_ERROR)
    add("selectors_18002", write_stream([block(T, selectors=[0] * 18002)]), OK)
    # length sets
    add("lengths_flat_incomplete", write_stream([block(T, tables=[_flat(alpha, 10)] * 2)]), OK)
    add("lengths_20", write_stream([block(T, tables=[[20] * alpha] * 2)]), OK)
    add("lengths_oversubscribed", write_stream([block(pre=b"aaa", used=[97, 98, 99], tables=[[2, 2, 2, 2, 1]] * 2)]))
    add("length_0", write_stream([block(T, tables=[[0] * alpha] * 2)]), DATA_ERROR)
    add("length_0_later", write_stream([block(T, tables=[[2, 1, 0] + [5] * (alpha - 3)] * 2)]), DATA_ERROR)
    add("length_21", write_stream([block(T, tables=[[20, 21] + [9] * (alpha - 2)] * 2)]), DATA_ERROR)
    add("length_21_second_table", write_stream([block(T, tables=[flat, [9] * (alpha - 1) + [21]])]), DATA_ERROR)
    # a code no symbol owns: the decoder reads on to 21 bits (or to the end of the input)
    s0, mk = write_stream([block(b"aab", symbols=[], tables=[[2, 2, 2, 3]] * 2, selectors=[0])], marks=True)
    at = (dict(mk)["symbols"] + 7) // 8
    add("unassigned_code", s0[:at] + b"\xff" * 8)
    add("unassigned_code_short", s0[:at] + b"\xff" * 2)
    # runs: weights, capacity, the end of the block
    A = ord("a")
    for reps in (1, 2, 3, 4, 7, 8, 1000):
        add("run_%d" % reps, write_stream([block(pre=b"b" + b"a" * reps + b"c")]), OK)
    add("run_70000", write_stream([block(pre=b"ab", used=[A, A + 1], symbols=_run(70000) + [2, 3], orig_ptr=0)]))
    add("run_weights_21", write_stream([block(pre=b"ab", used=[A, A + 1], symbols=[RUNB] * 21 + [3])], level=9))
    add("run_weights_22", write_stream([block(pre=b"ab", used=[A, A + 1], symbols=[RUNA] * 22 + [3])]), DATA_ERROR)
    add("run_over_capacity", write_stream([block(pre=b"ab", used=[A, A + 1], symbols=_run(100001) + [3])], level=1), DATA_ERROR)
    add("run_at_capacity", write_stream([block(pre=b"ab", used=[A, A + 1], symbols=_run(100000) + [3], orig_ptr=0)], level=1))
    add("symbols_over_capacity", write_stream([block(pre=b"ab", used=[A, A + 1], symbols=_run(100000) + [2, 3])], level=1), DATA_ERROR)
    add("no_end_of_block", write_stream([block(T, symbols=syms_t[:-1])]))
    add("only_end_of_block", write_stream([block(pre=b"ab", used=[A, A + 1], symbols=[3])]), DATA_ERROR)
    # the final run-length stage
    for count in (0, 1, 251, 252, 253, 254, 255):
        add("count_%d" % count, write_stream([block(pre=b"x" + b"q" * 4 + bytes([count]) + b"yz")]), OK)
    add("four_at_end_no_count", write_stream([block(pre=b"xy" + b"q" * 4)]), DATA_ERROR)
    add("four_at_end_count", write_stream([block(pre=b"xy" + b"q" * 4 + b"\x07")]), OK)
    add("four_split_across_blocks", write_stream([block(pre=b"xyqq"), block(pre=b"qq\x05z")]), OK)
    add("three_then_block_of_count", write_stream([block(pre=b"qqq"), block(pre=b"q\x03\x03\x03\x03\x02")]), OK)
    add("count_is_the_byte", write_stream([block(pre=b"\x04\x04\x04\x04\x04\x04\x04\x04\x04\x04")]), OK)
    add("periodic", write_stream([block(b"abcd" * 64)]), OK)
    add("periodic_pre", write_stream([block(pre=b"xyxyxyxyxyxy")]), OK)
    add("one_byte", write_stream([block(b"z")]), OK)
    # a cut at every header field (and through the symbols and the trailer)
    a2 = len(set(rle1(T[:200]))) + 2
    three = [_flat(a2, 8), [7] * 2 + [9] * (a2 - 2), _flat(a2, 6)]
    stream, marks = write_stream([block(T[:200], tables=three, selectors=[0, 1, 2, 1, 0, 2, 1, 0])], marks=True)
    add("cut_whole", stream, OK)
    cuts = sorted({0, 1, 2, 3, len(stream) - 1} | {bit // 8 for _, bit in marks} | {(bit + 7) // 8 for _, bit in marks})
    for c in cuts:
        if c < len(stream):
            add("cut_%d" % c, stream[:c], BUF_ERROR)
    return P


def _run(n):
    """RUNA / RUNB digits of a run of n"""
    out = []
    while n > 0:
        if n & 1:
            out.append(RUNA)
            n = (n - 1) // 2
        else:
            out.append(RUNB)
            n = (n - 2) // 2
    return out


_PROGRAMS = None


def PROGRAMS():
    global _PROGRAMS
    if _PROGRAMS is None:
        _PROGRAMS = programs()
    return _PROGRAMS


def verdicts():
    """[(name, stream, status, bytes or None, in_used or None)]: libbz2's verdict on every program, UNSUPPORTED where the
    writer set the randomised bit; computed once"""
    global _VERDICTS
    if _VERDICTS is None:
        _VERDICTS = []
        for name, stream, want in PROGRAMS():
            st, out, used = judge(stream)
            if want == UNSUPPORTED:
                st, out, used = UNSUPPORTED, None, None
            _VERDICTS.append((name, stream, st, out, used))
    return _VERDICTS


_VERDICTS = None


def _noise(n, seed):
    import numpy as np
    return np.random.RandomState(seed).bytes(n)


def _prose(n, seed):
    """compressible bytes without long runs"""
    import numpy as np
    rs = np.random.RandomState(seed)
    return ((rs.randint(0, 256, n) & rs.randint(0, 256, n) & 0x3F) + 32).astype(np.uint8).tobytes()


_PAYLOADS = None


def payloads():
    """[(name, stream, data)]: bz2.compress output the emulation and the device both decode -- the sizes at which the
    format takes another path (run lengths, the selector step every 50 symbols, the block cut, several blocks, a full
    900 000-symbol block, incompressible bytes, a periodic input whose link permutation has several cycles)"""
    global _PAYLOADS
    if _PAYLOADS is None:
        cases = [("empty", b"")] + [("equal_%d" % k, b"r" * k) for k in (1, 4, 5, 259)]
        cases += [("distinct_%d" % k, bytes(range(k))) for k in (48, 49, 50, 51)]
        cases += [("noise_4k", _noise(4096, 3)), ("periodic", b"abracadabra-" * 300), ("prose_20k", _prose(20000, 4))]
        _PAYLOADS = [("%s_l%d" % (name, lv), bz2.compress(d, lv), d) for name, d in cases for lv in (1, 9)]
        _PAYLOADS += [("cut_%d_l1" % k, bz2.compress(_prose(k, 5), 1), _prose(k, 5)) for k in (99999, 100000, 100001)]
        _PAYLOADS.append(("three_blocks_l1", bz2.compress(_prose(250000, 6), 1), _prose(250000, 6)))
    return _PAYLOADS


_FULL = None


def full_block():
    """(stream, data): 900 000 bytes at level 9 -- one block as full as the compressor makes them (899 981 symbols' worth)
    and a small one behind it"""
    global _FULL
    if _FULL is None:
        d = _prose(900000, 7)
        _FULL = (bz2.compress(d, 9), d)
    return _FULL
