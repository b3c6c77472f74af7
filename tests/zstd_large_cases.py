"""Multi-block Zstandard programs for the wave-per-block reader (mzhip_zstd_large; csrc/zstd_par_core.h, csrc/zstd_parallel.inc),
written with zstd_frames.Frame: what crosses block seams -- treeless literals, Repeat_Mode tables, repeat offsets, copies --
and what does not cross frame seams.  Blocks are tens to hundreds of bytes.  cases() is the list of
(name, stream, status, data, in_used, blocks, borrowed): the verdict of zstd_frames.expand() and the census of census()."""
from tests import zstd_frames as zf
from tests.zstd_frames import Frame, skippable, text

BLOCK_CAP = 32768      # MZ_ZSP_BLOCK_CAP of csrc/zstd_par_core.h


def census(z):
    """a plain walk over the headers of a VALID stream -> (blocks, blocks whose literals are treeless or one of whose tables is
    in Repeat_Mode)"""
    z = bytes(z)
    p, blocks, borrowed = 0, 0, 0
    while p < len(z):
        magic = int.from_bytes(z[p:p + 4], "little")
        if (magic & 0xFFFFFFF0) == 0x184D2A50:
            p += 8 + int.from_bytes(z[p + 4:p + 8], "little")
            continue
        assert magic == zf.MAGIC
        fhd = z[p + 4]
        single = (fhd >> 5) & 1
        p += 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 << (fhd >> 6)) if fhd >> 6 else single)
        while True:
            bh = int.from_bytes(z[p:p + 3], "little")
            last, kind, size = bh & 1, (bh >> 1) & 3, bh >> 3
            p += 3
            blocks += 1
            if kind == 2:
                b = z[p:p + size]
                lt, sf = b[0] & 3, (b[0] >> 2) & 3
                if lt < 2:
                    hdr = 1 if not sf & 1 else 2 if sf == 1 else 3
                    regen = (b[0] >> 3) if not sf & 1 else int.from_bytes(b[:hdr], "little") >> 4
                    q = hdr + (regen if lt == 0 else 1)
                else:
                    hdr = 3 if sf < 2 else sf + 2
                    bits = 10 if sf < 2 else 14 if sf == 2 else 18
                    q = hdr + ((int.from_bytes(b[:hdr], "little") >> 4) >> bits)
                nseq, q = (b[q], q + 1) if b[q] < 128 else (((b[q] - 128) << 8) + b[q + 1], q + 2) if b[q] < 255 else (0x7F00, q + 3)
                rep = nseq and any(((b[q] >> s) & 3) == 3 for s in (6, 4, 2))
                borrowed += 1 if lt == 3 or rep else 0
            p += 1 if kind == 1 else size
            if last:
                break
        p += 4 if fhd & 4 else 0
    return blocks, borrowed


def _finish(f, checksum=False, fcs_bytes=None, **kw):
    """the frame's bytes with its content (from expand()) behind the checksum / content-size switches"""
    single, f.single, f.fcs_bytes, f.checksum = f.single, False, None, False
    st, data, _ = zf.expand(f.bytes())
    assert st == 0, st
    f.single = single
    f.content = data
    f.checksum = checksum
    f.fcs_bytes = fcs_bytes
    for k, v in kw.items():
        setattr(f, k, v)
    return f.bytes()


def _digits(n, seed):
    import random
    r = random.Random(seed)
    return bytes(r.choice(b"0011223456789") for _ in range(n))


def programs():
    P = []
    T = text(6000, 77)
    A = T[:300]                         # the alphabet of the first tree
    only = lambda d: zf._only(d, A)
    add = lambda name, z: P.append((name, bytes(z)))

    # ---- treeless chains
    for streams, fse in ((1, False), (4, False), (1, True), (4, True)):
        f = Frame()
        f.comp(A, lit_mode="huf", lit_streams=streams, lit_fse_weights=fse)
        for k in range(39):
            d = only(T[300 + 120 * k:420 + 120 * k])
            f.comp(d, [(5, 4 + k % 7, 20 + k + 3), (2, 3, 1)], lit_mode="treeless", lit_streams=4 if streams == 4 and k % 2 else 1)
        add("treeless_chain_39_s%d_fse%d" % (streams, int(fse)), _finish(f, checksum=fse))
    f = Frame()
    f.comp(A, lit_mode="huf")
    for k in range(12):
        f.comp(only(T[400 + 90 * k:490 + 90 * k]), [(3, 5, 9)], lit_mode="treeless")
        if k % 4 == 0:
            f.raw(T[k:k + 33])
        elif k % 4 == 1:
            f.rle(65 + k, 70)
        elif k % 4 == 2:
            f.comp(T[2000 + k:2040 + k], [(4, 4, 6)], lit_mode="raw")
        else:
            f.comp(b"q" * 50, [(4, 4, 6)], lit_mode="rle")
    add("treeless_between_other_blocks", _finish(f, checksum=True, fcs_bytes=4))
    f = Frame()
    D = _digits(900, 5)
    f.comp(A, lit_mode="huf")
    for k in range(5):
        f.comp(only(T[400 + 90 * k:490 + 90 * k]), lit_mode="treeless")
    f.comp(D[:200], lit_mode="huf")                    # another alphabet: the nearest definer counts, not the first
    for k in range(5):
        f.comp(D[200 + 100 * k:300 + 100 * k], [(7, 3, 12)], lit_mode="treeless")
    add("treeless_tree_redefined", _finish(f))

    # ---- Repeat_Mode tables
    S4, S3 = [(3, 7, 9)] * 4, [(3, 7, 9)] * 3
    f = Frame()
    f.raw(T[:800])
    f.comp(T[:40], S4, modes=("fse", "pre", "pre"))
    f.comp(T[40:80], S4, modes=("rep", "fse", "pre"))
    f.comp(T[80:120], S4, modes=("rep", "rep", "fse"))
    f.comp(T[120:160], S3, modes=("rep", "rep", "rep"))     # LL from block 1, OF from block 2, ML from block 3
    f.comp(T[160:200], S3, modes=("pre", "rep", "rep"))
    add("repeat_each_table_another_definer", _finish(f, checksum=True))
    for first in ("rle", "pre", "fse"):
        f = Frame()
        f.raw(T[:800])
        f.comp(T[:40], S4, modes=(first,) * 3)
        f.comp(T[40:60])                                     # no sequences: changes nothing
        f.raw(T[60:70])
        f.comp(T[70:110], S3, modes=("rep",) * 3)
        f.comp(T[110:150], S3, modes=("rep", "pre", "rep"))
        f.comp(T[150:190], S3, modes=("rep",) * 3)           # OF: the Predefined of the block before
        add("repeat_of_%s" % first, _finish(f))

    # ---- what does not cross frames, and malformed definers
    two = Frame()
    two.comp(A, lit_mode="huf")
    fr2 = Frame()
    fr2.weights = two.weights
    add("treeless_first_block_of_second_frame", _finish(two) + fr2.comp(only(T[600:700]), lit_mode="treeless").bytes())
    f1, f2 = Frame(), Frame()
    f1.raw(T[:800]).comp(T[:40], S4, modes=("fse",) * 3)
    f2.tables = list(f1.tables)
    f2.raw(T[:800]).comp(T[:40], S4, modes=("pre", "rep", "pre"))
    add("repeat_first_block_of_second_frame", f1.bytes() + f2.bytes())
    f = Frame()
    f.raw(T[:50])
    f.comp(b"\x00\x01\x02" * 2, lit_mode="huf", lit_weights=[2, 1, 1], lit_tree=bytes([0x81, 0x31]))
    f.weights = [2, 1, 1]
    f.comp(b"\x00\x01\x02", lit_mode="treeless")
    add("treeless_definer_malformed", f.bytes())
    f = Frame()
    f.raw(T[:800])
    bad = [1] * 36
    f.comp(T[:40], [(1, 3, 4)] * 2, modes=("fse", "pre", "pre"), norms=(bad, None, None), al=(6, None, None))
    f.comp(T[40:80], [(1, 3, 4)] * 2, modes=("rep", "pre", "pre"))
    add("repeat_definer_malformed", f.bytes())

    # ---- repeat offsets across seams
    start = [(9, 3, 9 + 3), (1, 3, 7 + 3), (1, 3, 5 + 3)]    # repeat offsets 5, 7, 9
    f = Frame()
    f.raw(T[:100])
    f.comp(T[100:130], start)
    f.comp(T[130:140], [(2, 4, 1)])                          # pushes none
    f.comp(T[140:150])                                       # no sequences
    f.comp(T[150:160], [(2, 4, 6 + 3)])                      # pushes one: 6, 5, 7
    f.comp(T[160:170], [(1, 4, 3)])                          # the slot three blocks back: 7, 6, 5
    f.comp(T[170:180], [(2, 3, 11 + 3), (1, 3, 4 + 3)])      # pushes two: 4, 11, 7
    f.comp(T[180:190], [(1, 4, 3), (1, 4, 2), (1, 4, 3)])
    f.comp(T[190:200], [(0, 4, 1), (0, 4, 2), (1, 5, 1)])
    add("rep_pushes_0_1_2", _finish(f, checksum=True))
    f = Frame()
    f.raw(T[:100])
    f.comp(T[100:130], start)
    for k in range(10):
        f.comp(T[130 + 8 * k:138 + 8 * k], [(1 + k % 2, 4, 1 + k % 3), (0, 3 + k % 4, 1 + (k + 1) % 2), (1, 3, 2)])
    add("rep_ten_blocks_of_repeat_codes", _finish(f))
    f = Frame()
    f.raw(T[:100])
    f.comp(T[100:130], start)
    f.comp(T[130:135], [(0, 3, 3)])                          # rep0 - 1 = 4
    f.comp(T[135:140], [(0, 3, 3), (0, 3, 3)])               # incoming - 1, then incoming - 2
    f.comp(T[140:145], [(2, 3, 1), (1, 3, 2), (1, 3, 3)])
    add("rep_minus_one_first_in_block", _finish(f))
    f = Frame()
    f.raw(T[:100])
    f.comp(T[100:110], [(4, 3, 1 + 3)])                      # rep0 = 1
    f.comp(T[110:115], [(0, 3, 3)])                          # incoming - 1 = 0
    add("rep_symbolic_resolves_to_0", f.bytes())
    f = Frame()
    f.raw(T[:100])
    f.comp(T[100:110], [(4, 3, 2 + 3)])                      # rep0 = 2
    f.comp(T[110:115], [(0, 3, 3), (0, 3, 3)])               # 1, then 0
    add("rep_symbolic_nested_to_0", f.bytes())
    add("rep_first_block_offset_4_of_3_bytes", Frame().comp(T[:10], [(3, 3, 2)]).raw(T[10:20]).bytes())
    add("rep_first_block_offset_8_of_5_bytes", Frame().comp(T[:10], [(5, 3, 3)]).raw(T[10:20]).bytes())
    add("rep_first_block_offset_8_of_8_bytes", _finish(Frame().comp(T[:10], [(8, 3, 3)]).raw(T[10:20])))

    # ---- copies across blocks
    good = _finish(Frame().raw(T[:120]), checksum=True)
    f = Frame()
    f.raw(T[:100]).comp(T[100:110], [(2, 30, 102 + 3), (0, 5, 105 + 3)])
    add("copy_to_first_byte_of_second_frame", good + _finish(f))
    f = Frame()
    f.raw(T[:100]).comp(T[100:110], [(2, 30, 103 + 3)])
    add("copy_before_first_byte_of_second_frame", good + f.bytes())
    f = Frame()
    f.raw(T[:40])
    for k in range(64):
        f.comp(b"", [(0, 20, 20 + 3)])                       # every block copies the match of the block before
    add("copy_chain_64_blocks", _finish(f, checksum=True))
    f = Frame()
    f.raw(b"xyz")
    f.comp(b"", [(0, 10, 1 + 3)])
    f.comp(b"", [(0, 11, 2 + 3)])
    f.comp(b"", [(0, 12, 3 + 3)])
    f.comp(b"ab", [(1, 9, 1 + 3), (1, 9, 1 + 3)])
    add("copy_overlap_from_previous_block", _finish(f))
    f = Frame()
    f.raw(T[:30])
    f.comp(T[30:50], [(10, 6, 4 + 3), (3, 20, 2 + 3)])
    add("copy_from_own_literal_run", _finish(f))

    # ---- frames
    fa = Frame()
    fa.comp(T[:60], start).comp(T[60:80], [(1, 4, 2), (1, 4, 3)])
    fb = Frame()
    fb.comp(T[100:130], [(8, 3, 3), (1, 3, 2), (1, 3, 3)]).comp(T[130:140], [(2, 3, 1)])      # (1, 4, 8) again, not frame 1's offsets
    fc = Frame(single=True)
    fc.rle(66, 300).raw(T[:30]).raw(b"")
    za, zb, zc = _finish(fa, checksum=True), _finish(fb, checksum=True, fcs_bytes=8), _finish(fc, fcs_bytes=2)
    add("frames_with_skippables", skippable(0, b"") + za + skippable(7, b"between") + zb + zc + skippable(15, bytes(40)))
    add("frames_checksum_wrong_in_second", za + _finish(fb, checksum=True, checksum_xor=0x100) + zc)
    add("frames_content_size_wrong_in_second", za + _finish(fb, fcs_bytes=4, fcs=len(fb.content) + 1) + zc)
    add("frames_empty_last_blocks", _finish(Frame().raw(T[:20]).raw(b"")) + _finish(Frame().comp(T[:20], [(3, 3, 6)]).rle(1, 0), checksum=True))
    big = zf.noise(zf.BLOCK_MAX, 3)
    add("blocks_raw_and_rle_128k", _finish(Frame().raw(T[:10]).raw(big).rle(114, zf.BLOCK_MAX).comp(T[10:20], [(2, 40, 131072 + 3)]), checksum=True))
    f = Frame(window=0)                                       # blocks of 1 KiB at most
    f.raw(T[:500]).comp(T[:6], [(3, 1024 - 6, 2 + 3)])
    add("block_exactly_blk_max", _finish(f, window=0))
    f = Frame(window=0)
    f.raw(T[:500]).comp(T[:6], [(3, 1025 - 6, 2 + 3)])
    add("block_one_byte_over_blk_max", f.bytes())

    # ---- more blocks than the block cap
    f = Frame()
    for k in range(BLOCK_CAP + 1):
        f.raw(T[k % 5000:k % 5000 + 1])
    add("more_blocks_than_the_cap", f.bytes())
    return P


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = []
        for name, z in programs():
            st, data, used = zf.expand(z)
            _cases.append((name, z, st, data, used) + (census(z) if st == 0 else (0, 0)))
    return _cases


def over_cap(name):
    return name == "more_blocks_than_the_cap"
