"""Header programs: dynamic block headers of raw DEFLATE spelled field by field, for the tests of the header readers.

Every dynamic header the decoders saw before this file was written by a compressor (zlib's, or the `rle` option of
tests/token_programs.py), or was such a header with bytes damaged.  A compressor Huffman-codes its code-length code, sends the
literal / length and the distance lengths apart and never comes near the longest header the format allows.  Three pieces of
device code read a dynamic header -- mz_block_code (inflate_header.inc + inflate_tables.inc, in three instantiations),
k_check_headers and k_find_blocks (mzhip_kernels.hip) -- and what they decide depends on exactly the shapes no compressor
writes: a symbol that straddles the 64-bit window of the front end, a 16 whose value comes from the window before, a run that
crosses from the literal into the distance lengths, a header longer than the 2048-bit register window, a literal / length code
that fills the second-level table to its last entry.  Here those headers are written by hand and judged by zlib's inflate.

A HEADER PROGRAM is a dict, sent verbatim by tests/token_programs.py (the `hdr` opt of a dynamic block); nothing is validated:
    hlit, hdist, hclen   the raw field values (5, 5 and 4 bits)
    cl                   the 19 lengths of the code-length code, by symbol
    ops                  [(code-length symbol, extra value)]: 0 .. 15 a length, 16 / 17 / 18 a repeat with its extra bits
    raw                  [(value, bits)] sent behind the operations (what stands for a body that no token can say)
    refuse               zlib's message where the body (not the header) is what zlib refuses
The tokens of the block are coded with the two codes the operations spell, so a header program is a block of any token program.

read_header() is the plain statement of what zlib 1.2.11 does with a header, bit by bit and without tables: the judge of
k_check_headers.  sub_entries() / worst_sub_code() state the capacity of the second-level table (inflate_core.h).  The families
at the end return [(name, program, stream, expected bytes or None)] from a seed."""
import random

from tests import token_programs as T

CL_ORDER = T._CL_ORDER
REP = T._CL_EXTRA                        # repeat code: (extra bits, shortest run)
ENDED = "input ended"
NOT_DYNAMIC = "not a dynamic block"
REASONS = ("too many length or distance symbols", "invalid code lengths set", "invalid bit length repeat",
           "invalid code -- missing end-of-block", "invalid literal/lengths set", "invalid distances set")


# ---- the judge -------------------------------------------------------------------------------------------------------------

class _Ended(Exception):
    pass


def _kraft_left(lens, maxbits):
    """(what a code leaves of the code space in units of 2^-maxbits -- negative: over-subscribed --, its longest length)"""
    return (1 << maxbits) - sum((1 << maxbits) >> l for l in lens if l), max([0] + list(lens))


def judge_lengths(lit, dist):
    """zlib's verdict on the two sets of code lengths of a dynamic block: None, or the reason it refuses them"""
    if len(lit) <= 256 or lit[256] == 0:
        return REASONS[3]
    left, longest = _kraft_left(lit, 15)
    if left < 0 or (left > 0 and longest != 1):          # (incomplete is allowed to a single one-bit code alone)
        return REASONS[4]
    left, longest = _kraft_left(dist, 15)
    if left < 0 or (left > 0 and longest > 1):           # (... and to no distance code at all)
        return REASONS[5]
    return None


def read_header(buf, bit):
    """The dynamic block header whose first bit (BFINAL) is bit `bit` of buf, read as zlib 1.2.11's inflate() reads it.
    -> (literal / length lengths, distance lengths, the bit behind the header) when zlib gets past it, one of REASONS in zlib's
    words when it refuses it, ENDED when it asks for input behind buf first, NOT_DYNAMIC when BTYPE is not 2."""
    nbits = 8 * len(buf)
    pos = bit

    def need(k):                          # the next k bits, the first one lowest -- all of them or none (inflate.c NEEDBITS)
        nonlocal pos
        if pos + k > nbits:
            raise _Ended
        v = 0
        for i in range(k):
            v |= ((buf[(pos + i) >> 3] >> ((pos + i) & 7)) & 1) << i
        pos += k
        return v

    try:
        if (need(3) >> 1) != 2:
            return NOT_DYNAMIC
        h = need(14)
        nlen, ndist, ncode = (h & 31) + 257, ((h >> 5) & 31) + 1, (h >> 10) + 4
        if nlen > 286 or ndist > 30:
            return REASONS[0]
        cl = [0] * 19
        for s in CL_ORDER[:ncode]:
            cl[s] = need(3)
        left, longest = _kraft_left(cl, 7)
        seq = []
        if longest == 0:
            # no code at all: inflate_table() answers with invalid entries of one bit, inflate() reads nlen + ndist lengths
            # through them without looking at their kind -- a 0 each -- and then misses the end-of-block code
            for _ in range(nlen + ndist):
                need(1)
            return REASONS[3]
        if left:                          # over-subscribed, or incomplete (a single one-bit code included)
            return REASONS[1]
        count = [sum(1 for l in cl if l == n) for n in range(8)]
        order = [s for n in range(1, 8) for s in range(19) if cl[s] == n]
        while len(seq) < nlen + ndist:
            code = first = index = 0
            for n in range(1, 8):         # one bit at a time, as puff.c does
                code |= need(1)
                if code - first < count[n]:
                    sym = order[index + code - first]
                    break
                index += count[n]
                first = (first + count[n]) << 1
                code <<= 1
            else:
                raise AssertionError("a complete code decodes every pattern")
            if sym < 16:
                seq.append(sym)
                continue
            x = need(REP[sym][0])         # (the extra bits are pulled before the repeat is judged: inflate.c CODELENS)
            if sym == 16 and not seq:
                return REASONS[2]
            rep = REP[sym][1] + x
            if len(seq) + rep > nlen + ndist:
                return REASONS[2]
            seq += [seq[-1] if sym == 16 else 0] * rep
        why = judge_lengths(seq[:nlen], seq[nlen:])
        return why if why else (seq[:nlen], seq[nlen:], pos)
    except _Ended:
        return ENDED


# ---- the capacity of the second-level table ----------------------------------------------------------------------------------

def sub_entries(lens, root):
    """Second-level entries the canonical code of `lens` needs behind a first-level table of `root` bits: every root-bit
    prefix under which codes longer than root bits stand gets 2^(its longest code - root) entries (inflate_core.h)."""
    longest = {}
    for s, (code, n) in T._canonical(lens).items():
        if n > root:
            p = code >> (n - root)
            longest[p] = max(longest.get(p, 0), n)
    return sum(1 << (n - root) for n in longest.values())


_WORST = {}


def worst_sub_code(root, nsym=286, maxbits=15):
    """The lengths (ascending: the canonical code of symbols 0, 1, 2 ...) of a complete code of at most nsym symbols and
    maxbits bits that needs the most second-level entries behind a root of `root` bits, by dynamic programming over the
    prefixes in code order.  In a canonical code lengths never fall, so a prefix whose codes are all `a` bits deeper than the
    root or more, the longest d bits deeper, costs 2^d entries and takes 2^a + d - a symbols at the least (2^a - 1 codes at
    depth a, one at each depth between, two at depth d; 2^a when d = a) -- and the prefix behind it starts at depth d.  The
    P prefixes with long codes leave 2^root - P prefixes to short codes: one symbol per set bit of that number at the least.
    State: (depth the last prefix ended at, symbols spent) -> most entries; one step per prefix."""
    key = (root, nsym, maxbits)
    if key in _WORST:
        return list(_WORST[key])
    deep = maxbits - root
    best = (0, 0, None, None)                                      # entries, prefixes, state, the table it is in
    cur = {(1, 0): (0, None)}                                      # state -> (entries, the state before)
    tables = []
    for p in range(1, (1 << root) + 1):
        nxt = {}
        for (a, n), (cost, _) in cur.items():
            for d in range(a, deep + 1):
                n2 = n + (1 << a) + d - a
                if n2 > nsym:
                    break
                c2 = cost + (1 << d)
                if nxt.get((d, n2), (-1,))[0] < c2:
                    nxt[(d, n2)] = (c2, (a, n))
        if not nxt:
            break
        tables.append(nxt)
        short = bin((1 << root) - p).count("1")
        for (d, n), (cost, _) in nxt.items():
            if n + short <= nsym and cost > best[0]:
                best = (cost, p, (d, n), len(tables) - 1)
        cur = nxt
    cost, p, state, t = best
    depths = []
    while t >= 0:
        depths.append(state[0])
        state = tables[t][state][1]
        t -= 1
    depths.reverse()
    lens = [root - k for k in range(root, -1, -1) if ((1 << root) - p) >> k & 1]
    a = 1
    for d in depths:
        if d == a:
            lens += [root + a] * (1 << a)
        else:
            lens += [root + a] * ((1 << a) - 1) + list(range(root + a + 1, root + d)) + [root + d] * 2
        a = d
    while len(lens) < nsym and any(l < root for l in lens):       # symbols left over: split a short code (the long ones stay)
        k = max(i for i, l in enumerate(lens) if l < root)
        lens[k:k + 1] = [lens[k] + 1] * 2
    lens.sort()
    assert sub_entries(lens, root) == cost
    _WORST[key] = list(lens)
    return lens


# ---- building blocks of the families -------------------------------------------------------------------------------------------

class Unspellable(Exception):
    pass


def header(nlen, ndist, cl, ops, hclen=None, raw=None, refuse=None):
    """a header program from symbol COUNTS nlen / ndist (the fields are 257 and 1 less) and the number of code-length-code
    lengths sent (default: up to the last one that is not zero, 4 at the least)"""
    if hclen is None:
        hclen = max([4] + [k + 1 for k, s in enumerate(CL_ORDER) if cl[s]])
    h = dict(hlit=nlen - 257, hdist=ndist - 1, hclen=hclen - 4, cl=list(cl), ops=list(ops))
    if raw:
        h["raw"] = list(raw)
    if refuse:
        h["refuse"] = refuse
    return h


def op_bits(hdr, op):
    return hdr["cl"][op[0]] + (REP[op[0]][0] if op[0] >= 16 else 0)


def ops_start(hdr):
    """bits from the block's first bit to the first operation"""
    return 17 + 3 * (hdr["hclen"] + 4)


def header_bits(hdr):
    """bits from the block's first bit to the end of the last operation"""
    return ops_start(hdr) + sum(op_bits(hdr, op) for op in hdr["ops"])


def front_end_windows(hdr):
    """[(window number, offset of the operation's first bit in that window, bits)] per operation, as the 64-bit front end of
    inflate_header.inc walks a header that is far from the end of its input: a window takes the symbols that end inside its 64
    bits, and the next one starts at the first symbol that does not."""
    out, w, off = [], 0, 0
    for op in hdr["ops"]:
        n = op_bits(hdr, op)
        if off + n > 64:
            w, off = w + 1, 0
        out.append((w, off, n))
        off += n
    return out


def front_end_model(hdr, start, total_bits):
    """(symbols the 64-bit front end takes, its steps, symbols left to the serial loop) for an ACCEPTED header whose block starts
    at bit `start` of a dword-aligned input of total_bits bits -- inflate_header.inc restated: a step starts while lengths are
    due, its window lies in the first 61 dwords of the register window and 78 bits or more of input lie behind its first bit; it
    takes every operation that ends inside its 64 bits, the one that ends exactly at bit 64 and the last one of the header
    included."""
    ops, k, fe, steps = hdr["ops"], 0, 0, 0
    bitpos = start + ops_start(hdr)
    while k < len(ops):
        if (bitpos >> 5) - (start >> 5) + 3 >= 64 or bitpos + 78 > total_bits:
            break
        cur = 0
        while k < len(ops) and cur + op_bits(hdr, ops[k]) <= 64:
            cur += op_bits(hdr, ops[k])
            k += 1
            fe += 1
        steps += 1
        bitpos += cur
    return fe, steps, len(ops) - fe


def complete_cl(assigned, spare=None):
    """the 19 lengths of a COMPLETE code-length code that gives the symbols of `assigned` = {symbol: bits} those lengths: what
    they leave of the code space goes to symbols of `spare` (default: every other symbol, from 15 down), one per set bit"""
    cl = [0] * 19
    for s, n in assigned.items():
        cl[s] = n
    left, _ = _kraft_left(cl, 7)
    assert left >= 0, assigned
    spare = [s for s in (spare if spare is not None else range(15, -1, -1)) if s not in assigned]
    for b in range(6, -1, -1):
        if left >> b & 1:
            cl[spare.pop(0)] = 7 - b
    return cl


def every_symbol_cl(short):
    """a complete code-length code in which all 19 symbols have a code: `short` = three symbols that get 1, 2 and 3 bits,
    the other sixteen get 7"""
    cl = [7] * 19
    for s, n in zip(short, (1, 2, 3)):
        cl[s] = n
    assert _kraft_left(cl, 7)[0] == 0
    return cl


FLAT_CL = [4] * 13 + [5] * 6             # 13 x 4 + 6 x 5 bits: every symbol has a code, the repeat codes the long ones


def _chain(lengths):
    """counts {length: codes} of the complete code that uses the ascending `lengths` as a chain: all but one code of a
    length, the one left over split into the next length, the last length fills up"""
    out, at = {}, 0
    for k, l in enumerate(lengths):
        n = 1 << (l - at)
        out[l] = n if k == len(lengths) - 1 else n - 1
        at = l
    return out


def _pick_counts(lengths, cap, rnd, want=None):
    """a complete code {length: count} of at most cap symbols from the allowed lengths (with `want` among them)"""
    lengths = sorted(lengths)
    for _ in range(400):
        k = rnd.randrange(1, min(5, len(lengths)) + 1)
        sub = set(rnd.sample(lengths, k))
        if want:
            sub.add(want)
        c = _chain(sorted(sub))
        if 2 <= sum(c.values()) <= cap and all(c.values()):
            return c
    if want and all(l in lengths for l in range(1, want + 1)):
        return _chain(list(range(1, want + 1)))
    raise Unspellable(lengths)


def _zero_sizes(avail):
    return ({1} if 0 in avail else set()) | (set(range(3, 11)) if 17 in avail else set()) | (set(range(11, 139)) if 18 in avail else set())


def _sums(sizes, m):
    can = [True] + [False] * m
    for k in range(1, m + 1):
        can[k] = any(s <= k and can[k - s] for s in sizes)
    return can


def spell(seq, avail, rnd, style="mixed", force=None):
    """Operations that spell the lengths seq with the code-length symbols of `avail` alone.  style: "plain" the shortest
    operation every time, "rle" the longest, "mixed" any.  force = {index: operation}: the operation sent where seq[index]
    is due -- as it is, right or wrong; no other operation reaches across such an index."""
    force = force or {}
    ops, i, n = [], 0, len(seq)
    while i < n:
        if i in force:
            s, x = force[i]
            ops.append((s, x))
            i += 1 if s < 16 else REP[s][1] + x
            continue
        v, j = seq[i], i + 1
        while j < n and seq[j] == v and j not in force:
            j += 1
        m = j - i
        later = ({1} if v in avail else set()) | (_zero_sizes(avail) if v == 0 else set()) | (set(range(3, 7)) if 16 in avail else set())
        can = _sums(later, m)
        same = i > 0 and seq[i - 1] == v
        while m:
            cands = []
            if v in avail and can[m - 1]:
                cands.append((v, 0, 1))
            if same and 16 in avail:
                cands += [(16, r - 3, r) for r in range(3, 7) if r <= m and can[m - r]]
            if v == 0:
                cands += [(s, r - REP[s][1], r) for s in (17, 18) if s in avail for r in range(REP[s][1], REP[s][1] + (1 << REP[s][0]))
                          if r <= m and can[m - r]]
            if not cands:
                raise Unspellable((v, m, sorted(avail)))
            if style == "plain":
                s, x, r = min(cands, key=lambda c: c[2])
            elif style == "rle":
                s, x, r = max(cands, key=lambda c: c[2])
            else:
                kind = rnd.choice(sorted({c[0] for c in cands}))
                s, x, r = rnd.choice([c for c in cands if c[0] == kind])
            ops.append((s, x))
            m -= r
            i += r
            same = True
    return ops


def make_lengths(avail, rnd, want=None):
    """(literal / length lengths, distance lengths) that zlib accepts and that the code-length symbols of `avail` can spell:
    complete codes from the lengths there are (with `want` among the literal / length ones), an end-of-block code, zeros only
    where a zero can be sent -- in runs where only 17 and 18 can send them."""
    nz = [l for l in range(1, 16) if l in avail]
    zsizes = _zero_sizes(avail)
    if not nz:
        raise Unspellable(avail)
    for _ in range(16):
        c = _pick_counts(nz, 286, rnd, want)
        ncoded = sum(c.values())
        pool = [l for l, k in c.items() for _ in range(k)]
        rnd.shuffle(pool)
        if 0 in avail:
            syms = sorted(rnd.sample([s for s in range(286) if s != 256], ncoded - 1) + [256])
            nlen = max(257, syms[-1] + 1 + rnd.randrange(0, 286 - syms[-1]))
        else:
            if ncoded > 257 and not zsizes:
                start = 0
            else:
                start = 256 - (ncoded - 1) + rnd.randrange(0, min(29, ncoded - 1) + 1)
            if start < 0 or (start and not zsizes) or (start and not _sums(zsizes, start)[start]) or (not zsizes and ncoded < 257):
                continue
            syms = list(range(start, start + ncoded))
            nlen = max(257, syms[-1] + 1)
            if syms[-1] < 256 or syms[-1] > 285:
                continue
        lit = [0] * nlen
        for s, l in zip(syms, pool):
            lit[s] = l
        if any(lit[s] == 0 for s in range(nlen)) and not zsizes:
            continue
        how = rnd.choice(("none", "one", "code", "code")) if zsizes else rnd.choice(("one", "code"))
        if how == "none":
            k = 1 if 0 in avail else min(s for s in range(1, 31) if _sums(zsizes, s)[s]) if any(_sums(zsizes, 30)[1:]) else 0
            if not k:
                continue
            dist = [0] * k
        elif how == "one":
            if 1 not in nz:
                continue
            lead = rnd.randrange(0, 30) if 0 in avail else 0
            dist = [0] * lead + [1]
        else:
            try:
                c = _pick_counts(nz, 30, rnd)
            except Unspellable:
                continue
            pool = [l for l, k in c.items() for _ in range(k)]
            rnd.shuffle(pool)
            if 0 in avail:
                syms = sorted(rnd.sample(range(30), len(pool)))
                dist = [0] * (syms[-1] + 1)
                for s, l in zip(syms, pool):
                    dist[s] = l
            else:
                dist = pool
        assert judge_lengths(lit, dist) is None
        return lit, dist
    raise Unspellable(avail)


def spelled_header(cl, rnd, want=None, style="mixed", hclen=None, use=None):
    """an accepted header program through the code-length code cl: lengths made for the symbols that have a code, spelled in
    `style`; use = a code-length symbol that must be among the operations"""
    avail = {s for s in range(19) if cl[s]}
    for _ in range(24):
        try:
            lit, dist = make_lengths(avail, rnd, want)
            ops = spell(lit + dist, avail, rnd, style)
        except Unspellable:
            continue
        if use is None or any(op[0] == use for op in ops):
            return header(len(lit), len(dist), cl, ops, hclen)
    raise Unspellable((cl, want, use))


def code_bits(lens, sym):
    """(value, bits) that put() sends for symbol sym of the canonical code of lens"""
    return T._reversed_codes(lens)[sym]


def body(rnd, lit, dist, nlits=4, match=True, bits=0):
    """a few tokens the two codes can say: literals that have a code (nlits of them, or as many as make `bits` bits), then
    one match -- the shortest length and distance symbols that have a code and reach no further back than the literals"""
    coded = [s for s in range(min(256, len(lit))) if lit[s]]
    toks = [rnd.choice(coded) for _ in range(nlits)] if coded else []
    while coded and bits and sum(lit[t] for t in toks) < bits and len(toks) < 2000:
        toks.append(rnd.choice(coded))
    if match and toks:
        ls = [s for s in range(257, min(286, len(lit))) if lit[s]]
        ds = [s for s in range(min(30, len(dist))) if dist[s] and T._DBASE[s] <= len(toks)]
        if ls and ds:
            toks.append((T._LBASE[rnd.choice(ls) - 257], T._DBASE[rnd.choice(ds)]))
            toks.append(rnd.choice(coded))
    return toks


def block_of(hdr, rnd, final=True, **kw):
    """the dynamic block of a header program: with a few tokens where the header is one zlib gets past, bare where not"""
    sp = T.spelled_lengths(hdr)
    ok = sp is not None and hdr["hlit"] <= 29 and hdr["hdist"] <= 29 and _kraft_left(hdr["cl"], 7)[0] == 0 and judge_lengths(*sp) is None
    toks = body(rnd, sp[0], sp[1], **kw) if ok and not hdr.get("raw") else []
    return ("dynamic", toks, final, {"hdr": hdr})


def header_of(program):
    """(index of the block, header program) of the last block of a program that carries one"""
    k = max(i for i, b in enumerate(program) if len(b) > 3 and b[3] and "hdr" in b[3])
    return k, program[k][3]["hdr"]


def header_bit(program):
    """the bit of the stream at which the block of header_of(program) starts"""
    marks = []
    T.encode(program, marks)
    return marks[header_of(program)[0]]


def finish(named):
    """[(name, program)] -> [(name, program, stream, expected bytes or None)]: expected is what the program stands for where
    the judge gets past its header and nothing says that zlib refuses the body"""
    out = []
    for name, prog in named:
        marks = []
        z = T.encode(prog, marks)
        k, hdr = header_of(prog)
        ok = not isinstance(read_header(z, marks[k]), str) and not hdr.get("refuse")
        data = T.expand(prog) if ok else None
        assert len(z) < 2048 and (data is None or len(data) < 4096), (name, len(z))
        out.append((name, prog, z, data))
    assert len({e[0] for e in out}) == len(out)
    return out


# ---- the families --------------------------------------------------------------------------------------------------------------

CLC_SHAPES = ((1, 1), (2, 2, 2, 2), (1, 2, 3, 4, 5, 6, 7, 7), (3,) * 8, (4,) * 16, (4,) * 13 + (5,) * 6)
HEADER_FIELDS = ((0, 0), (29, 29), (7, 3))


def clc(seed=1):
    """The code-length code: every HCLEN from 4 to 19 (the last length sent is not zero; and once more as HCLEN 19 with zeros
    behind it), each of the 19 symbols with a 1-bit and with a 7-bit code and among the operations, the complete shapes of
    CLC_SHAPES on seeded symbols -- and the refused ones: over-subscribed, incomplete, a single one-bit code, no code at all,
    with the fields of HEADER_FIELDS.  HCLEN 4 can send no length but zero: refused for its missing end-of-block code."""
    out = []
    for h in range(4, 20):
        for k in range(4):
            rnd = random.Random(seed * 100000 + h * 10 + k)
            last = CL_ORDER[h - 1]
            if h == 4:
                cl = complete_cl({16: 2, 17: 2, 18: 2, 0: 2})
                hdr = header(257, 1, cl, spell([0] * 258, {0, 17, 18}, rnd, "mixed"))
            else:
                for _ in range(200):
                    others = rnd.sample(CL_ORDER[:h - 1], rnd.randrange(1, min(h - 1, 7) + 1))
                    shape = list(rnd.choice([s for s in CLC_SHAPES + ((1, 2, 2), (2, 2, 3, 3, 3, 3), (1, 2, 3, 3)) if len(s) <= len(others) + 1]))
                    rnd.shuffle(shape)
                    cl = [0] * 19
                    for s, n in zip([last] + others, shape):
                        cl[s] = n
                    if _kraft_left(cl, 7)[0]:
                        continue
                    try:
                        hdr = spelled_header(cl, rnd, want=last if 1 <= last <= 15 else None, use=last)
                        break
                    except Unspellable:
                        continue
                else:
                    raise Unspellable(h)
            assert hdr["hclen"] + 4 == h
            out.append(("clc/hclen%d/%d" % (h, k), [block_of(hdr, rnd)]))
            if h < 19:
                out.append(("clc/hclen%d/%d/sent_as_19" % (h, k), [block_of(dict(hdr, hclen=15), rnd)]))
    for s in range(19):
        for nbits in (1, 7):
            for k in range(3):
                rnd = random.Random(seed * 100000 + 5000 + s * 20 + nbits * 2 + k)
                rest = [x for x in (0, 8, 18, 7, 9) if x != s]
                short = [s, rest[0], rest[1]] if nbits == 1 else rest[:3]
                cl = every_symbol_cl(short)
                hdr = spelled_header(cl, rnd, want=s if 1 <= s <= 15 else None, use=s, style=("mixed", "rle", "rle" if s >= 16 else "plain")[k])
                out.append(("clc/sym%d_has_%d_bits/%d" % (s, nbits, k), [block_of(hdr, rnd)]))
    for i, shape in enumerate(CLC_SHAPES):
        for k in range(4):
            rnd = random.Random(seed * 100000 + 9000 + i * 10 + k)
            for _ in range(500):
                syms = rnd.sample(range(19), len(shape))
                cl = [0] * 19
                for s, n in zip(syms, shape):
                    cl[s] = n
                try:
                    hdr = spelled_header(cl, rnd)
                    break
                except Unspellable:
                    continue
            else:
                raise Unspellable(shape)
            out.append(("clc/shape%d/%d" % (i, k), [block_of(hdr, rnd)]))
    k = 0
    for hl, hd in HEADER_FIELDS:
        for what in ("over", "incomplete", "single", "none"):
            for var in range(4):
                rnd = random.Random(seed * 100000 + 9500 + k)
                k += 1
                if what == "none":
                    cl = [0] * 19
                    hclen = (4, 19, 6, 12)[var]
                    n = hl + 257 + hd + 1
                    raw = [(rnd.getrandbits(n + 16) if var & 1 else 0, n + 16)]      # (one bit per length, whatever it is)
                    hdr = header(hl + 257, hd + 1, cl, [], hclen, raw)
                else:
                    base = list(rnd.choice(CLC_SHAPES[1:]))
                    if what == "single":
                        base = [1]
                    elif what == "over":
                        if var & 1 or len(base) == 19:                # one code a bit shorter, or one code more
                            j = rnd.choice([j for j, l in enumerate(base) if l > 1])
                            base[j] -= 1
                        else:
                            base.append(rnd.choice((1, 7, 3)))
                    else:
                        j = rnd.randrange(len(base))
                        if var & 1 and base[j] < 7:
                            base[j] += 1
                        else:
                            del base[j]
                    syms = rnd.sample(range(19), len(base))
                    cl = [0] * 19
                    for s, n in zip(syms, base):
                        cl[s] = n
                    assert _kraft_left(cl, 7)[0] != 0 and any(cl)
                    ops = [(s, rnd.randrange(4) if s >= 16 else 0) for s in (rnd.choice(syms) for _ in range(12))]
                    hdr = header(hl + 257, hd + 1, cl, ops, 19 if var == 3 else None)
                out.append(("clc/refused/%s/hlit%d_hdist%d/%d" % (what, hl, hd, var), [block_of(hdr, rnd)]))
    return out


def _tail_code(n, length):
    """lengths of a literal / length code of n symbols whose last 2^length symbols, the end-of-block code among them, share
    `length` bits: zeros in front"""
    k = 1 << length
    assert n - k <= 256 < n
    return [0] * (n - k) + [length] * k


def ops(seed=2):
    """The operations: every extra value of 16, 17 and 18; a 16 behind a plain length, behind a 16, behind a 17 and an 18 (it
    repeats zero); runs that end exactly at HLIT + 257, that cross it by 1 .. their length - 1 (a crossing 16 hands a length from
    the last literal / length symbols to the first distance symbols), that end exactly at the last length -- and the refused
    ones: a 16 as the first operation, and a 16, 17 or 18 that overruns the last length by 1 and by the most it can."""
    out = []
    cls = (FLAT_CL, every_symbol_cl((0, 8, 16)), every_symbol_cl((18, 4, 17)))
    every = set(range(19))
    n = 0

    def add(name, lit, dist, force, cl=None, style="mixed"):
        nonlocal n
        rnd = random.Random(seed * 100000 + n)
        n += 1
        cl = cl or cls[n % 3]
        hdr = header(len(lit), len(dist), cl, spell(lit + dist, every, rnd, style, force))
        out.append((name, [block_of(hdr, rnd)]))

    d16 = [4] * 16
    # 16: 2^3 symbols of 3 bits at 249 .. 256: a plain 3, then repeats
    for x in range(4):
        add("ops/16/extra%d/after_plain" % x, _tail_code(257, 3), [0], {249: (3, 0), 250: (16, x)})
        add("ops/16/extra%d/after_16" % x, _tail_code(260, 4), d16, {244: (4, 0), 245: (16, 3 - x), 248 + 3 - x: (16, x)})
        for z in (17, 18):
            zr = REP[z][1] + x
            add("ops/16/extra%d/after_%d" % (x, z), _tail_code(257, 3), [0], {100: (z, x), 100 + zr: (16, x)})
            add("ops/16/extra%d/first_lengths_by_%d" % (x, z), _tail_code(257, 3), [0], {0: (z, 1), REP[z][1] + 1: (16, x)})
    for x in range(8):
        for at in (0, 57, 249 - 3 - x):
            add("ops/17/extra%d/at%d" % (x, at), _tail_code(257, 3), [1, 1], {at: (17, x)})
    for x in range(128):
        at = (0, 249 - 11 - x, x % 50)[x % 3]
        add("ops/18/extra%d/at%d" % (x, at), _tail_code(257, 3), [1, 1], {at: (18, x)})
    # runs that end at, and cross, HLIT + 257: sixteen symbols of 4 bits at the end of the literal / length lengths and sixteen
    # distance symbols of 4 bits are one run of 32; zeros behind symbol 256 and in front of the first distance code another
    for r in range(3, 7):
        for c in range(0, r):                                       # c = lengths of the run that are distance lengths
            nlen = 260
            start = nlen - (r - c)
            lit = _tail_code(nlen, 4)
            if c == 0:
                add("ops/16/ends_at_hlit/run%d" % r, lit, [1, 1], {start - 1: (4, 0), start: (16, r - 3)})
            else:
                add("ops/16/crosses_hlit/run%d/by%d" % (r, c), lit, d16, {start - 1: (4, 0), start: (16, r - 3)})
        add("ops/16/ends_at_the_last_length/run%d" % r, _tail_code(257, 3), d16, {257 + 16 - r - 1: (4, 0), 257 + 16 - r: (16, r - 3)})
    for z in (17, 18):
        lo = REP[z][1]
        for r in (range(3, 11) if z == 17 else (11, 12, 13, 20, 30, 41, 57)):
            for c in range(0, r):
                if c > 28 or r - c > 29:
                    continue
                if z == 18 and r > 13 and c not in (0, 1, 2, r // 2, r - 2, r - 1, 28, r - 29):
                    continue
                nlen = 257 + (r - c)
                lit = _tail_code(257, 3) + [0] * (r - c)
                dist = [0] * c + [1, 1]
                add("ops/%d/%s/run%d/by%d" % (z, "crosses_hlit" if c else "ends_at_hlit", r, c), lit, dist, {nlen - (r - c): (z, r - lo)})
            if r <= 28:
                add("ops/%d/ends_at_the_last_length/run%d" % (z, r), _tail_code(257, 3), [1, 1] + [0] * r, {257 + 2: (z, r - lo)})
    # refused
    for x in range(4):
        for k, cl in enumerate(cls):
            add("ops/refused/16_first/extra%d/%d" % (x, k), _tail_code(257, 3), [0], {0: (16, x)}, cl)
    for s in (16, 17, 18):
        lo, hi = REP[s][1], REP[s][1] + (1 << REP[s][0]) - 1
        for r, over in [(r, 1) for r in sorted({lo, lo + 1, (lo + hi) // 2, hi})] + [(hi, hi - 1), (hi, hi // 2)]:
            left = r - over                                          # lengths still due where the run starts
            if s == 16:
                lit, dist = _tail_code(257, 3), [4] * 16
                force = {257 + 16 - left: (16, r - lo)}
            else:
                lit, dist = _tail_code(257, 3), [1, 1] + [0] * min(left, 28)
                lit = lit + [0] * (left - min(left, 28))
                force = {len(lit) + len(dist) - left: (s, r - lo)}
            add("ops/refused/%d_overruns/run%d/by%d" % (s, r, over), lit, dist, force)
    return out


WINDOW_CL = every_symbol_cl((8, 0, 1))        # the common length 8 in one bit; 16, 17, 18 and the rare lengths in seven
WINDOW_PROBES = ("plain", "16", "17", "18")


def _complete_after(pre, rnd):
    """literal / length lengths that start with `pre` and are complete: what pre leaves of the code space goes, one symbol per
    set bit, to the symbols up to 256; zeros between"""
    left, _ = _kraft_left(pre, 15)
    assert left > 0
    fill = [15 - b for b in range(14, -1, -1) if left >> b & 1]
    rnd.shuffle(fill)
    assert len(pre) + len(fill) <= 257
    return list(pre) + [0] * (257 - len(pre) - len(fill)) + fill


def window(seed=3):
    """The 64-bit front end.  The common length has a 1-bit code; pad = 0 .. 70 such operations stand in front of one probe: a
    plain length with a 7-bit code, a 16, a 17 or an 18 with 7-bit codes (9, 10 and 14 bits).  The operations start a window,
    so the probe starts at bit pad of the first window or at bit pad - 64 of the second; over the family it ends exactly at
    bit 64 and straddles it by 1 .. 13 bits, and the 16 of pad 64 takes its value from the last symbol of the window before
    (pad 0: a 16 with nothing before it, refused).  Every second program has 100 bits of tokens or more behind the header, so
    that the front end reads it to its last length; the others hand over to the serial loop within 78 bits of the end.  Then the same with an overrun as the probe, behind zeros that bring the
    lengths to where pad + 1 .. are left: refused in the middle of a window."""
    out = []
    every = set(range(19))
    for pad in range(71):
        for probe in WINDOW_PROBES:
            rnd = random.Random(seed * 100000 + pad * 10 + WINDOW_PROBES.index(probe))
            x = rnd.randrange(4 if probe == "16" else 8 if probe == "17" else 100)
            if probe == "plain":
                pre, op = [8] * pad + [9 + pad % 3], (9 + pad % 3, 0)
            elif probe == "16":
                pre, op = [8] * (pad + 3 + x), (16, x)
            else:
                pre, op = [8] * pad + [0] * (REP[int(probe)][1] + x), (int(probe), x)
            lit = _complete_after(pre, rnd) if pad or probe != "16" else _tail_code(257, 3)
            dist = [[0], [1], [1, 1], [0, 0, 2, 2, 2, 2]][pad % 4]
            style = "plain" if pad % 2 else "mixed"
            force = {i: (8, 0) for i in range(pad)}
            force[pad] = op
            hdr = header(len(lit), len(dist), WINDOW_CL, spell(lit + dist, every, rnd, style, force))
            out.append(("window/%s/pad%d" % (probe, pad), [block_of(hdr, rnd, bits=(100 + pad) * ((pad + len(probe)) % 2))]))   # (every second header ends far from the end of the input)
    for pad in range(71):
        for s in (16, 17, 18):
            for most in (False, True):
                rnd = random.Random(seed * 100000 + 5000 + pad * 10 + s - 16 + 3 * most)
                lo, hi = REP[s][1], REP[s][1] + (1 << REP[s][0]) - 1
                r = hi if most else rnd.randrange(lo, hi + 1)
                left = 1 if most else r - 1                       # lengths still due at the probe: the run is `r - left` too long
                if s == 16 and pad == 0:
                    continue                                       # (the 16 needs a length before it: the first family has that case)
                zeros = 258 - left - pad
                seq = [0] * zeros + [8] * pad + [0 if s != 16 else 8] * left
                force = {zeros + i: (8, 0) for i in range(pad)}
                force[zeros + pad] = (s, r - lo)
                hdr = header(257, 1, WINDOW_CL, spell(seq, every, rnd, "rle", force))
                out.append(("window/refused/%d_overruns/%s/pad%d" % (s, "most" if most else "by1", pad), [block_of(hdr, rnd)]))
    return out


LONG_CLS = (("2254", {8: 7, 9: 7, 5: 6, 4: 5}), ("2286", {8: 7, 9: 7, 5: 7, 4: 7}), ("2028", {8: 6, 9: 7, 5: 6, 4: 5}),
            ("2060", {8: 6, 9: 7, 5: 7, 4: 7}), ("1968", {8: 6, 9: 6, 5: 6, 4: 5}))
LONG_SPARE = (1, 2, 3, 6, 7, 10, 11)          # lengths nobody sends take the short codes


def _front_blocks(bits, rnd):
    """small blocks in front of a header that make it start `bits` modulo 32 bits into the stream: empty fixed blocks (10 bits),
    fixed blocks of one literal above 143 (19 bits), and where the count allows an empty stored block first (32 bits then)"""
    a, b = next((a, b) for n in range(40) for a in range(n + 1) for b in (n - a,) if (10 * a + 19 * b) % 32 == bits)
    blocks = [("fixed", [], False)] * a + [("fixed", [rnd.randrange(144, 256)], False)] * b
    rnd.shuffle(blocks)
    return blocks


def long(seed=4):
    """Headers around the 2048-bit register window of mz_block_code.  "2254": the code-length code gives 8 and 9 seven bits, 5 six,
    4 five, and its 1- to 4-bit codes to lengths nobody sends; 226 x 8 + 60 x 9 literal / length lengths and 2 x 4 + 28 x 5
    distance lengths, each a plain operation.  "2286": seven bits for all four, the longest header there is.  "2028" .. "1968":
    shorter codes for the common lengths, so that the edge falls into the distance lengths or the header ends in front of it.
    "with16" / "with18": the 2254 code with a 16 (repeating 9) or an 18 (zeros across HLIT + 257) where bit 2048 falls.  Every
    variant starts at every bit 0 .. 31 modulo 32 behind small blocks, and is followed by literals, a match and end-of-block."""
    out = []
    variants = []
    for name, a in LONG_CLS:
        variants.append((name, complete_cl(a, LONG_SPARE), [8] * 226 + [9] * 60, [4] * 2 + [5] * 28, {}))
    cl = complete_cl({8: 7, 9: 7, 5: 6, 4: 5, 16: 7, 18: 7, 0: 7}, LONG_SPARE)
    variants.append(("with16", cl, [8] * 226 + [9] * 60, [4] * 2 + [5] * 28, "16"))
    variants.append(("with18", cl, None, None, "18"))
    for vname, cl, lit, dist, how in variants:
        for start in range(32):
            rnd = random.Random(seed * 100000 + start)
            if how == "16":
                at = 277 + start % 4
                if (2048 - start - 74 - 8) % 7 == 0:              # (bit 2048 of the window between the two extra bits of the 16)
                    at = (2048 - start - 74 - 8) // 7
                force = {at: (16, start % 4)}                     # (symbols at .. at + 2 + start % 4 repeat the 9 before them)
            elif how == "18":
                z0 = 276 + start % 7                              # zeros from literal / length symbol z0 across into the distance lengths
                nz = 286 - z0 + 7
                a8 = 512 - z0
                lit = [8] * a8 + [9] * (z0 - a8) + [0] * (286 - z0)
                dist = [0] * 7 + [4] * 9 + [5] * 14
                force = {z0: (18, nz - 11)}
            else:
                force = {}
            avail = {s for s in range(19) if cl[s]}
            hdr = header(len(lit), len(dist), cl, spell(lit + dist, avail, rnd, "plain", force), 19 if start % 2 else None)
            front = _front_blocks(start, rnd)
            if start % 8 == 5:
                front = [("stored", [], False)] + front           # (a stored block ends on a byte boundary: 32 bits from bit 0)
            near = T._DBASE[min(s for s in range(30) if dist[s]) + start % 3]      # (one of the three nearest distances that have a code)
            toks = [rnd.randrange(226) for _ in range(near + start % 5)] + [(3 + start % 8, near), rnd.randrange(226)]
            out.append(("long/%s/start%d" % (vname, start), front + [("dynamic", toks, True, {"hdr": hdr})]))
    return out


def _ladder(longest):
    """the complete code of lengths 1, 2 .. longest - 1 and two of `longest` (two one-bit codes for 1)"""
    return list(range(1, longest)) + [longest] * 2


def _place(lengths, n, must, rnd):
    """n code lengths: `lengths` on seeded symbols, the first of them on symbol `must`; zeros elsewhere"""
    syms = [must] + rnd.sample([s for s in range(n) if s != must], len(lengths) - 1)
    out = [0] * n
    for s, l in zip(syms, lengths):
        out[s] = l
    return out


def sets(seed=5):
    """The two codes: a complete literal / length code whose longest code has 1 .. 15 bits, the same for the distance code; every
    value of HLIT and of HDIST; end-of-block as the only code, and its unused pattern; literals without a distance code, and a
    match met there; a single one-bit distance code, used, and its unused pattern; the literal / length code that needs all 404
    second-level entries (worst_sub_code(8)) on seeded symbols, its body made of every symbol whose code is longer than 8 bits.
    Refused: no end-of-block code; either set over-subscribed or incomplete by one code of 1, 2, 8, 9 and 15 bits; HLIT and
    HDIST fields 30 and 31."""
    out = []
    every = set(range(19))
    n = 0

    def add(name, lit, dist, toks=None, raw=None, refuse=None, fields=None, style=None):
        nonlocal n
        rnd = random.Random(seed * 100000 + n)
        n += 1
        hdr = header(len(lit), len(dist), (FLAT_CL, every_symbol_cl((0, 8, 18)))[n % 2], spell(lit + dist, every, rnd, style or ("mixed", "rle", "plain")[n % 3]),
                     raw=raw, refuse=refuse)
        if fields:
            hdr.update(fields)
        blk = block_of(hdr, rnd) if toks is None else ("dynamic", toks, True, {"hdr": hdr})
        out.append((name, [blk]))

    for longest in range(1, 16):
        for k in range(3):
            rnd = random.Random(seed * 1000 + longest * 10 + k)
            nl = rnd.randrange(257, 287)
            add("sets/lit_longest%d/%d" % (longest, k), _place(_ladder(longest), nl, 256, rnd), [[0], [1], [2, 2, 1]][k])
            nd = rnd.randrange(max(2, longest + 1), 31)
            add("sets/dist_longest%d/%d" % (longest, k), _place(_ladder(3), 257 + 5 * k, 256, rnd) if k else _tail_code(260, 4),
                _place(_ladder(longest), nd, rnd.randrange(4), rnd))
    for v in range(30):
        rnd = random.Random(seed * 1000 + 500 + v)
        add("sets/hlit%d" % v, _place(_ladder(2 + v % 7), 257 + v, 256, rnd), [1, 1])
        if v:
            lit = [0] * (257 + v)                                                 # (the last symbol there is room for has a code)
            for sym, l in zip([256 + v, 256] + rnd.sample(range(256), 3), _ladder(4)):
                lit[sym] = l
            add("sets/hlit%d/last_symbol_coded" % v, lit, [1, 1])
        add("sets/hdist%d" % v, _tail_code(257 + v % 4, 2 + v % 3), _place(_ladder(1 + v % 5), v + 1, v, rnd) if v >= 1 + v % 5 else [0] * v + [1])
    eob = [0] * 256 + [1]
    add("sets/eob_only", eob, [0])
    add("sets/eob_only/hdist29", eob, [0] * 30)
    add("sets/eob_only/unused_pattern", eob, [0], raw=[(1, 1), (0, 32)], refuse="invalid literal/length code")
    lits = _place(_ladder(3), 257, 256, random.Random(seed))
    add("sets/literals_without_a_distance_code", lits, [0])
    lm = [0] * 260                                                            # a literal, end-of-block and length 3
    lm[65], lm[256], lm[257] = 1, 2, 2
    add("sets/no_distance_code/a_match_met", lm, [0], raw=[code_bits(lm, 65), code_bits(lm, 257), (0, 32)], refuse="invalid distance code")
    add("sets/no_distance_code/a_match_met/hdist29", lm, [0] * 30, raw=[code_bits(lm, 65), code_bits(lm, 257), (0, 32)], refuse="invalid distance code")
    for ds in (0, 1, 29):
        add("sets/one_distance_code/symbol%d/used" % ds, lm, [0] * ds + [1], toks=[65] * (T._DBASE[ds] if ds < 29 else 1) + ([(3, T._DBASE[ds])] if ds < 29 else []))
        add("sets/one_distance_code/symbol%d/unused_pattern" % ds, lm, [0] * ds + [1], raw=[code_bits(lm, 65), code_bits(lm, 257), (1, 1), (0, 32)],
            refuse="invalid distance code")
    worst = worst_sub_code(8)
    for k in range(12):
        rnd = random.Random(seed * 1000 + 900 + k)
        if len(worst) == 286:
            lit = list(worst)
            rnd.shuffle(lit)
        else:
            lit = _place(worst, 286, 256, rnd)
        for must in (0, 255, 256, 285):                              # these four get long codes (a swap keeps the multiset)
            if lit[must] <= 8:
                j = rnd.choice([s for s in range(286) if lit[s] > 8 and s not in (0, 255, 256, 285)])
                lit[must], lit[j] = lit[j], lit[must]
        assert sub_entries(lit, 8) == 404 and sorted(lit) == sorted(worst + [0] * (286 - len(worst)))
        long_syms = [s for s in range(286) if lit[s] > 8]
        rnd.shuffle(long_syms)
        toks = [s for s in long_syms if s < 256] + [(T._LBASE[s - 257], 1) for s in long_syms if s > 256]
        add("sets/worst_second_level/%d" % k, lit, [1], toks=toks, style=("rle", "mixed", "plain")[k % 3])
    # refused
    nomark = _place(_ladder(3), 257, 7, random.Random(seed + 2))
    nomark[256] = 0
    add("sets/refused/no_end_of_block", nomark, [0])
    add("sets/refused/no_end_of_block/hlit29", _place(_ladder(3), 286, 270, random.Random(seed + 3)), [1, 1])
    for length in (1, 2, 8, 9, 15):
        base = _ladder(length) if length > 1 else [1, 2, 2]
        for which in ("lit", "dist"):
            rnd = random.Random(seed * 1000 + 950 + length)
            good_l, good_d = _place(_ladder(3), 270, 256, rnd), [1, 1]
            over, under = base + [length], list(base)
            under.remove(length)
            if which == "lit":
                add("sets/refused/lit_over_by_one_of_%d" % length, _place(over, 280, 256, rnd), good_d)
                add("sets/refused/lit_incomplete_by_one_of_%d" % length, _place(under, 280, 256, rnd), good_d)
            else:
                add("sets/refused/dist_over_by_one_of_%d" % length, good_l, _place(over, 30, 3, rnd))
                add("sets/refused/dist_incomplete_by_one_of_%d" % length, good_l, _place(under, 30, 3, rnd))
    for f in (30, 31):
        add("sets/refused/hlit_field%d" % f, _tail_code(257, 3), [1, 1], fields=dict(hlit=f), toks=[])
        add("sets/refused/hdist_field%d" % f, _tail_code(257, 3), [1, 1], fields=dict(hdist=f), toks=[])
    return out


FAMILIES = {"clc": clc, "ops": ops, "window": window, "long": long, "sets": sets}
CUT_SAMPLE = {"clc": 5, "ops": 5, "window": 5, "long": 1, "sets": 4}
_BUILT = {}


def family(name):
    """[(name, program, stream, expected bytes or None)] of a family, built once per process; nobody changes it"""
    if name not in _BUILT:
        _BUILT[name] = cut() if name == "cut" else finish(FAMILIES[name]())
    return _BUILT[name]


def cut(seed=6):
    """A seeded sample of the accepted programs of every family, cut at every byte inside the header and at the two bytes
    behind it (the stream, not the program, is cut: the program is the whole one's)."""
    out = []
    rnd = random.Random(seed)
    for fam, k in CUT_SAMPLE.items():
        good = [e for e in family(fam) if e[3] is not None]
        for name, prog, z, data in rnd.sample(good, k):
            bit = header_bit(prog)
            end = read_header(z, bit)[2]
            for n in range(bit // 8, min(len(z) - 1, (end + 7) // 8 + 2) + 1):
                out.append(("cut/%s/at%d" % (name, n), prog, z[:n], None))
    return out


ALL_FAMILIES = tuple(FAMILIES) + ("cut",)


def everything():
    return [e for f in ALL_FAMILIES for e in family(f)]


# ---- programs for the many-wave window: every block another accepted header ---------------------------------------------------

def window_programs(seed=7, count=12):
    """[(name, program, history)] for T.run_window_program: programs of 4 to 40 dynamic blocks, every block with another accepted
    header program of clc, ops, window and sets and 300 bits of tokens or more (literals its code can say, then a match)."""
    rnd = random.Random(seed)
    pool = []
    for fam in ("clc", "ops", "window", "sets"):
        for name, prog, z, data in family(fam):
            hdr = prog[-1][3]["hdr"]
            if data is not None and len(prog) == 1 and "raw" not in hdr and "worst" not in name:
                lit = T.spelled_lengths(hdr)[0]
                if any(lit[:256]):
                    pool.append((name, hdr))
    rnd.shuffle(pool)
    out, at = [], 0
    for k in range(count):
        nblk = (4, 7, 12, 20, 33, 40)[k % 6]
        prog = []
        for i in range(nblk):
            name, hdr = pool[at % len(pool)]
            at += 1
            lit, dist = T.spelled_lengths(hdr)
            prog.append(("dynamic", body(rnd, lit, dist, nlits=8, bits=300), i == nblk - 1, {"hdr": hdr}))
        out.append(("hdr_window/%d/%d_blocks" % (k, nblk), prog, b""))
    return out
