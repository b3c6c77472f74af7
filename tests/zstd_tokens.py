"""A structural reader of Zstandard frames (RFC 8878), built on the pieces of tests/zstd_frames.py: read(z) returns what a frame
SAYS -- header fields, and per block its type and sizes, how the literals are coded (mode, streams, size format, direct or
FSE-compressed tree description, longest code), the sequence count and its form, the three table modes and accuracy logs, and
every sequence as written (literal length, match length, offset value) with the distance it resolves to and the repeat
offsets in front of it -- where zstd_frames.expand() only returns the bytes.  replay(frames) executes the sequences.  The
encoder tests (tests/test_zstd_enc_emul.py, tests/test_gpu_zstd_enc.py) hold minizip-ng_amd/csrc/zstd_enc_core.h to its
contract with it; tests/test_zstd_tokens.py holds the reader itself against libzstd's committed streams and the frame programs.
No libzstd is needed."""
from tests import zstd_frames as zf

highbit = zf.highbit


class Malformed(Exception):
    pass


def _need(cond, what):
    if not cond:
        raise Malformed(what)


def _literals(b, st):
    """the literals section at the head of b -> (info, literal bytes, section size)"""
    _need(len(b) >= 1, "literals header")
    kind, sf = b[0] & 3, (b[0] >> 2) & 3
    info = dict(mode=("raw", "rle", "huf", "treeless")[kind], size_format=sf, streams=0, tree=None, max_code_len=0, weights=None)
    if kind < 2:
        hdr = 1 if not sf & 1 else 2 if sf == 1 else 3
        _need(hdr <= len(b), "literals header")
        regen = (b[0] >> 3) if not sf & 1 else int.from_bytes(b[:hdr], "little") >> 4
        if kind == 0:
            _need(regen <= len(b) - hdr, "raw literals")
            lits, used = bytes(b[hdr:hdr + regen]), hdr + regen
        else:
            _need(hdr + 1 <= len(b), "rle literals")
            lits, used = bytes(b[hdr:hdr + 1]) * regen, hdr + 1
        info.update(regen=regen, comp=used - hdr, header=hdr)
        return info, lits, used
    hdr = 3 if sf < 2 else sf + 2
    _need(hdr <= len(b), "literals header")
    bits = 10 if sf < 2 else 14 if sf == 2 else 18
    v = int.from_bytes(b[:hdr], "little") >> 4
    regen, comp = v & ((1 << bits) - 1), v >> bits
    streams = 1 if sf == 0 else 4
    _need(regen > 0 and comp <= len(b) - hdr, "literals sizes")
    body = b[hdr:hdr + comp]
    if kind == 2:
        try:
            w, used = zf._read_tree(body)
        except zf._Bad:
            raise Malformed("tree description")
        mb = highbit(sum(1 << (x - 1) for x in w if x))
        cells = []
        for wt in range(1, mb + 1):
            for s, ws in enumerate(w):
                if ws == wt:
                    cells += [(s, mb + 1 - wt)] * (1 << (wt - 1))
        st["tree"] = (mb, cells)
        info.update(tree="direct" if body[0] >= 128 else "fse", tree_bytes=used, weights=w, max_code_len=mb)
        body = body[used:]
    else:
        _need(st["tree"] is not None, "treeless literals without a tree")
        info.update(max_code_len=st["tree"][0])
    mb, cells = st["tree"]
    try:
        if streams == 1:
            lits = zf._huf_decode(body, regen, mb, cells)
            info["stream_bytes"] = [len(body)]
        else:
            _need(len(body) >= 10, "jump table")
            s1, s2, s3 = (int.from_bytes(body[k:k + 2], "little") for k in (0, 2, 4))
            body = body[6:]
            seg = (regen + 3) // 4
            _need(s1 + s2 + s3 <= len(body) and 3 * seg <= regen, "jump table")
            cuts = [0, s1, s1 + s2, s1 + s2 + s3, len(body)]
            lits = b"".join(zf._huf_decode(body[cuts[k]:cuts[k + 1]], seg if k < 3 else regen - 3 * seg, mb, cells) for k in range(4))
            info["stream_bytes"] = [cuts[k + 1] - cuts[k] for k in range(4)]
    except zf._Bad:
        raise Malformed("huffman stream")
    info.update(regen=regen, comp=comp, header=hdr, streams=streams)
    return info, bytes(lits), hdr + comp


def _sequences(b, st, info):
    """the sequences section b -> list of (ll, ml, offset value, distance, (rep0, rep1, rep2) in front of it)"""
    _need(len(b) >= 1, "sequence count")
    if b[0] < 128:
        nseq, p, form = b[0], 1, 1
    elif b[0] < 255:
        _need(len(b) >= 2, "sequence count")
        nseq, p, form = ((b[0] - 128) << 8) + b[1], 2, 2
    else:
        _need(len(b) >= 3, "sequence count")
        nseq, p, form = int.from_bytes(b[1:3], "little") + 0x7F00, 3, 3
    info.update(nseq=nseq, count_form=form, modes=None, accuracy=None, norms=[None] * 3)
    if nseq == 0:
        _need(p == len(b), "bytes behind an empty sequences section")
        return []
    _need(p < len(b), "modes")
    modes, p = b[p], p + 1
    _need(modes & 3 == 0, "reserved mode bits")
    names = []
    for t in range(3):
        mode = (modes >> (6 - 2 * t)) & 3
        max_sym, max_al, default, default_al = zf.TABLE_LIMITS[t]
        names.append(("predefined", "rle", "fse", "repeat")[mode])
        if mode == 0:
            st["tab"][t] = (zf.fse_table(default, default_al), default_al)
        elif mode == 1:
            _need(p < len(b) and b[p] <= max_sym, "rle symbol")
            st["tab"][t], p = ([(b[p], 0, 0)], 0), p + 1
        elif mode == 2:
            try:
                norm, al, used = zf._read_fse(b[p:], max_al, max_sym)
            except zf._Bad:
                raise Malformed("table description")
            st["tab"][t], p = (zf.fse_table(norm, al), al), p + used
            info["norms"][t] = norm
        else:
            _need(st["tab"][t] is not None, "repeat without a table")
    info.update(modes=tuple(names), accuracy=tuple(st["tab"][t][1] for t in range(3)))
    try:
        s = zf._Back(b[p:])
    except zf._Bad:
        raise Malformed("sequence bitstream")
    (tl, al_l), (to, al_o), (tm, al_m) = st["tab"]
    sl, so, sm = s.read(al_l), s.read(al_o), s.read(al_m)
    _need(s.left >= 0, "sequence bitstream")
    rep, seqs = st["rep"], []
    for i in range(nseq):
        cl, co, cm = tl[sl], to[so], tm[sm]
        ofv = (1 << co[0]) + s.read(co[0])
        ml = zf.ML_CODES[cm[0]][0] + s.read(zf.ML_CODES[cm[0]][1])
        ll = zf.LL_CODES[cl[0]][0] + s.read(zf.LL_CODES[cl[0]][1])
        if i + 1 < nseq:
            sl = cl[2] + s.read(cl[1])
            sm = cm[2] + s.read(cm[1])
            so = co[2] + s.read(co[1])
        _need(s.left >= 0, "sequence bitstream")
        before = tuple(rep)
        if ofv > 3:
            dist = ofv - 3
            rep[:] = [dist, rep[0], rep[1]]
        else:
            idx = ofv - 1 + (ll == 0)
            if idx == 0:
                dist = rep[0]
            else:
                dist = rep[idx] if idx < 3 else rep[0] - 1
                _need(dist != 0, "offset 0")
                rep[:] = [dist, rep[0], rep[2]] if idx == 1 else [dist, rep[0], rep[1]]
        seqs.append((ll, ml, ofv, dist, before))
    _need(s.left == 0, "sequence bitstream not used up")
    return seqs


def read(z):
    """-> list of frames: dict(single, window, fcs, fcs_bytes, checksum, checksum_value, header_bytes, blocks=[...], size);
    skippable frames are skipped.  A block: dict(type "raw" / "rle" / "compressed", last, size (the header's field), content
    (its bytes, raw and rle), and for a compressed block literals (info), lits (bytes), sequences, nseq, count_form, modes,
    accuracy)"""
    z = bytes(z)
    frames, p = [], 0
    while p < len(z):
        _need(len(z) - p >= 4, "magic")
        magic = int.from_bytes(z[p:p + 4], "little")
        if (magic & 0xFFFFFFF0) == 0x184D2A50:
            _need(len(z) - p >= 8, "skippable frame")
            p += 8 + int.from_bytes(z[p + 4:p + 8], "little")
            continue
        _need(magic == zf.MAGIC, "magic")
        p0, p = p, p + 4
        fhd, p = z[p], p + 1
        _need(not fhd & 8, "reserved bit")
        single, window, wbyte = (fhd >> 5) & 1, None, None
        if not single:
            wbyte, p = z[p], p + 1
            window = (1 << (10 + (wbyte >> 3))) // 8 * (8 + (wbyte & 7))
        n = (0, 1, 2, 4)[fhd & 3]
        did, p = int.from_bytes(z[p:p + n], "little"), p + n
        n = (1 << (fhd >> 6)) if fhd >> 6 else single
        fcs = int.from_bytes(z[p:p + n], "little") + (256 if n == 2 else 0) if n else None
        p += n
        f = dict(single=bool(single), window=window, window_byte=wbyte, fcs=fcs, fcs_bytes=n, did_bytes=(0, 1, 2, 4)[fhd & 3], did=did,
                 checksum=bool(fhd & 4), checksum_value=None, header_bytes=p - p0, blocks=[])
        st = dict(tree=None, tab=[None] * 3, rep=[1, 4, 8])
        while True:
            _need(len(z) - p >= 3, "block header")
            bh = int.from_bytes(z[p:p + 3], "little")
            last, kind, size = bh & 1, (bh >> 1) & 3, bh >> 3
            p += 3
            _need(kind != 3, "reserved block type")
            blk = dict(type=("raw", "rle", "compressed")[kind], last=bool(last), size=size, rep_before=tuple(st["rep"]))
            if kind == 0:
                _need(size <= len(z) - p, "raw block")
                blk["content"], p = z[p:p + size], p + size
            elif kind == 1:
                _need(p < len(z), "rle block")
                blk["content"], p = z[p:p + 1] * size, p + 1
            else:
                _need(size <= len(z) - p, "compressed block")
                body = z[p:p + size]
                info, lits, used = _literals(body, st)
                blk["literals"], blk["lits"] = info, lits
                blk["sequences"] = _sequences(body[used:], st, blk)
                p += size
            f["blocks"].append(blk)
            if last:
                break
        if fhd & 4:
            _need(len(z) - p >= 4, "checksum")
            f["checksum_value"], p = int.from_bytes(z[p:p + 4], "little"), p + 4
        f["size"] = p - p0
        frames.append(f)
    return frames


def replay(frames):
    """the bytes the frames stand for: every block's sequences executed over its literals"""
    out = bytearray()
    for f in frames:
        fo = len(out)
        for b in f["blocks"]:
            if b["type"] != "compressed":
                out += b["content"]
                continue
            lits, lp = b["lits"], 0
            for ll, ml, _, dist, _ in b["sequences"]:
                out += lits[lp:lp + ll]
                lp += ll
                _need(0 < dist <= len(out) - fo, "distance before the frame's start")
                if dist >= ml:
                    out += out[len(out) - dist:len(out) - dist + ml]
                else:
                    for _ in range(ml):
                        out.append(out[-dist])
            out += lits[lp:]
    return bytes(out)
