"""Archive-level batch path: index a ZIP, shard its entries, decode a whole shard in a few launches.

Host side of the "thousands of members in one launch" path (SURVEY 8b "Batching"): the central directory is
indexed once by the C indexer (mzhip_zip_index_mem), the archive bytes are placed in HBM as they are (the entry
payloads are used in place -- no repacking), and every entry of the shard is decoded by mzhip_inflate_batch /
mzhip_bzip2_batch / mzhip_zstd_batch / mzhip_lzma_batch / mzhip_xz_batch / mzhip_crc32_batch according to its method.  The per-entry CRC is compared with
the central-directory CRC exactly where the reference compares it (mz_zip.c:2116-2128); with verify_hash the first
Hash extrafield (0x1a51, doc/mz_extrafield.md) of each entry is checked against a device-computed SHA digest the way
mz_zip_reader_entry_open / _close do it on the CPU in a crypto build (mz_zip_rw.c:409-451,465-466).

Sharding: entries are independent, so ranks take contiguous slices of the entry table balanced by
compressed+uncompressed bytes; the only collective is the gather of the per-entry {crc, out_len, status} words.

The writer (encode_archive, at the end): one codec launch, one encrypt call (ZipCrypto / WinZip AES) and one copy back per
archive, the ZIP32 container assembled on the host (assemble_archive).
"""
import ctypes as C
import importlib
import mmap
import os

import numpy as np

_mz = importlib.import_module("minizip-ng_amd")

COL_METHOD, COL_FLAG, COL_CRC, COL_CSIZE, COL_USIZE, COL_LOCAL, COL_CDPOS, COL_PAYLOAD = range(8)
MZ_FORMAT_ERROR = -103
MZ_CRC_ERROR = -105       # mz.h:34
MZ_PASSWORD_ERROR = -108  # mz.h:37
MZ_SUPPORT_ERROR = -109   # mz.h:38
MZ_ZIP_EXTENSION_AES = 0x9901    # mz.h:114
MZ_COMPRESS_METHOD_AES = 99
MZ_ZIP_EXTENSION_HASH = 0x1A51   # mz.h:113
MZ_HASH_SHA1, MZ_HASH_SHA256 = 20, 23   # mz.h:127,131


def hash_fields(buf, table):
    """First Hash extrafield of every entry's central-directory record (mz_zip_reader_entry_get_first_hash,
    mz_zip_rw.c:560-600): -> (algorithm u16[n] (0 = none), digest_size u16[n], digest u8[n, 64])."""
    a = np.frombuffer(buf, dtype=np.uint8)
    n = len(table)
    alg = np.zeros(n, dtype=np.uint16)
    dsz = np.zeros(n, dtype=np.uint16)
    dig = np.zeros((n, 64), dtype=np.uint8)
    for i in range(n):
        p = int(table[i, COL_CDPOS])
        fn, ex = int(a[p + 28]) | int(a[p + 29]) << 8, int(a[p + 30]) | int(a[p + 31]) << 8
        q, end = p + 46 + fn, p + 46 + fn + ex
        while q + 4 <= end:
            fid, fsz = int(a[q]) | int(a[q + 1]) << 8, int(a[q + 2]) | int(a[q + 3]) << 8
            if fid == MZ_ZIP_EXTENSION_HASH and fsz >= 4 and q + 4 + fsz <= end:
                alg[i] = int(a[q + 4]) | int(a[q + 5]) << 8
                k = min(int(a[q + 6]) | int(a[q + 7]) << 8, fsz - 4, 64)
                dsz[i] = k
                dig[i, :k] = a[q + 8:q + 8 + k]
                break
            q += 4 + fsz
    return alg, dsz, dig


def crypt_fields(buf, table):
    """What the crypt streams of encrypted entries need from the central-directory records, per entry:
    verify u32[n]     mzhip_pkcrypt_batch's word: bits 0-7 the check byte for plain header byte 11, bits 8-15 the one for
                      byte 10 -- the CRC's two high bytes, or the DOS time's high and the date's low byte when flag bit 3
                      is set (mz_zip_get_pk_verify, mz_zip.c:192-198) -- bit 16 when version-needed is below 2
                      (mz_strm_pkcrypt.c:158);
    aes_version, aes_strength u8[n], method i64[n]   from the 0x9901 extrafield of method-99 entries (7 bytes, version 1
                      or 2, vendor "AE", strength, the real method; mz_zip.c:415-440), method = the table's otherwise;
    format_error bool[n]   a method-99 entry without such a field."""
    a = np.frombuffer(buf, dtype=np.uint8)
    n = len(table)
    verify = np.zeros(n, dtype=np.uint32)
    aes_version = np.zeros(n, dtype=np.uint8)
    aes_strength = np.zeros(n, dtype=np.uint8)
    method = np.array(table[:, COL_METHOD], dtype=np.int64)
    format_error = np.zeros(n, dtype=bool)

    def u16(q):
        return int(a[q]) | int(a[q + 1]) << 8

    for i in range(n):
        if not int(table[i, COL_FLAG]) & 1:
            continue
        p = int(table[i, COL_CDPOS])
        need, flag, dos_time, dos_date = u16(p + 6), u16(p + 8), u16(p + 12), u16(p + 14)
        crc = int(table[i, COL_CRC]) & 0xFFFFFFFF
        v10, v11 = (dos_date & 255, dos_time >> 8) if flag & 8 else ((crc >> 16) & 255, crc >> 24)
        verify[i] = v11 | v10 << 8 | (0x10000 if need < 2 else 0)
        if method[i] != MZ_COMPRESS_METHOD_AES:
            continue
        fn, ex = u16(p + 28), u16(p + 30)
        q, end = p + 46 + fn, p + 46 + fn + ex
        format_error[i] = True
        while q + 4 <= end:
            fid, fsz = u16(q), u16(q + 2)
            if fid == MZ_ZIP_EXTENSION_AES and q + 4 + fsz <= end:
                if fsz == 7 and u16(q + 4) in (1, 2) and bytes(a[q + 6:q + 8]) == b"AE":
                    aes_version[i], aes_strength[i], method[i] = u16(q + 4), a[q + 8], u16(q + 9)
                    format_error[i] = False
                break
            q += 4 + fsz
    return dict(verify=verify, aes_version=aes_version, aes_strength=aes_strength, method=method, format_error=format_error)


def index_bytes(buf):
    """Entry table [n, 8] int64 (columns COL_*) of the archive held in `buf` (bytes / mmap / uint8 array)."""
    a = np.frombuffer(buf, dtype=np.uint8)
    L = _mz.lib()
    L.mzhip_zip_index_mem.restype = C.c_int64
    L.mzhip_zip_index_mem.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int64]
    n = L.mzhip_zip_index_mem(a.ctypes.data, a.size, None, 0)
    if n < 0:
        raise _mz.MzHipError("mzhip_zip_index_mem: %d" % n)
    t = np.zeros((max(n, 1), 8), dtype=np.int64)
    n2 = L.mzhip_zip_index_mem(a.ctypes.data, a.size, t.ctypes.data, n)
    assert n2 == n
    return t[:n]


def index_file(path):
    with open(path, "rb") as f:
        if os.fstat(f.fileno()).st_size == 0:
            raise _mz.MzHipError("empty file")
        with mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as m:
            return index_bytes(m)


def shard_bounds(table, world):
    """Contiguous slices [b[r], b[r+1]) of the entry table, balanced by compressed + uncompressed bytes."""
    w = (table[:, COL_CSIZE] + table[:, COL_USIZE] + 64).astype(np.float64)
    cum = np.concatenate(([0.0], np.cumsum(w)))
    targets = cum[-1] * np.arange(1, world) / world
    cuts = np.searchsorted(cum, targets, side="left")
    return np.concatenate(([0], cuts, [len(table)])).astype(np.int64)


def gather_results(results, world, group=None):
    """results: int64 tensor [n_local, 3] = (crc, out_len, status) of this rank's slice, any device.
    All-gathers the (ragged) slices; returns the full [n, 3] table on every rank.  The ONLY collective."""
    import torch
    import torch.distributed as dist

    if world == 1:
        return results
    n_local = torch.tensor([results.shape[0]], dtype=torch.int64, device=results.device)
    counts = [torch.zeros_like(n_local) for _ in range(world)]
    dist.all_gather(counts, n_local, group=group)
    m = int(max(int(c.item()) for c in counts))
    pad = torch.zeros((m, 3), dtype=torch.int64, device=results.device)
    pad[: results.shape[0]] = results
    parts = [torch.zeros_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad, group=group)
    return torch.cat([p[: int(c.item())] for p, c in zip(parts, counts)], dim=0)


LARGE_ENTRY = 4 << 20   # compressed bytes from which a DEFLATE entry is decoded by a wave per block (as mzhip_prime_* does)
LARGE_ZSTD_ENTRY = 4 << 20   # ... and a Zstandard entry by a wave per block (mzhip_zstd_large)


class DeviceArchive:
    """A ZIP archive resident in HBM, decoded shard-wise by the batch kernels."""

    def __init__(self, path, device="cuda:0"):
        import torch

        _mz.require_gpu()
        self.path = path
        self.device = torch.device(device)
        self.table = index_file(path)
        self.h_file = np.fromfile(path, dtype=np.uint8)
        self.d_file = torch.from_numpy(self.h_file).to(self.device)

    def _decrypt(self, t, cf, password, stream):
        """Encrypted entries of the slice -> a device scratch buffer, one call per kind (mzhip_pkcrypt_batch, mzhip_wzaes_batch).
        Returns (d_scr, scr_off i64[n], plain_len i64[n], crypt_status i32[n]); entries that are not encrypted keep status 0."""
        import torch

        n = len(t)
        dev = self.device
        enc = (t[:, COL_FLAG] & 1) != 0
        is_aes = enc & (t[:, COL_METHOD] == MZ_COMPRESS_METHOD_AES)
        cst = np.zeros(n, dtype=np.int32)
        cst[is_aes & cf["format_error"]] = MZ_FORMAT_ERROR
        if (t[enc, COL_CSIZE] >= 2**32).any():
            raise _mz.MzHipError("entries >= 4 GiB are outside the batch path")
        slot = np.where(enc, (t[:, COL_CSIZE] + 15) // 16 * 16, 0)
        scr_off = np.zeros(n, dtype=np.int64)
        if n:
            np.cumsum(slot[:-1], out=scr_off[1:])
        d_scr = torch.empty(max(int(slot.sum()), 16), dtype=torch.uint8, device=dev)
        plain_len = np.zeros(n, dtype=np.int64)
        L = _mz.lib()
        pw = bytes(password)
        for kind, sel in (("pk", np.nonzero(enc & ~is_aes)[0]), ("aes", np.nonzero(is_aes & ~cf["format_error"])[0])):
            if len(sel) == 0:
                continue
            k = len(sel)
            d_in_off = torch.from_numpy(np.ascontiguousarray(t[sel, COL_PAYLOAD], dtype=np.int64)).to(dev)
            d_in_len = torch.from_numpy(t[sel, COL_CSIZE].astype(np.uint32).view(np.int32)).to(dev)
            d_out_off = torch.from_numpy(np.ascontiguousarray(scr_off[sel])).to(dev)
            r_len, r_st = (torch.zeros(k, dtype=torch.int32, device=dev) for _ in range(2))
            if kind == "pk":
                d_ver = torch.from_numpy(cf["verify"][sel].view(np.int32)).to(dev)
                rc = L.mzhip_pkcrypt_batch(self.d_file.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), d_scr.data_ptr(),
                                           d_out_off.data_ptr(), k, pw, len(pw), d_ver.data_ptr(), r_len.data_ptr(),
                                           r_st.data_ptr(), stream)
            else:
                d_str = torch.from_numpy(np.ascontiguousarray(cf["aes_strength"][sel])).to(dev)
                rc = L.mzhip_wzaes_batch(self.d_file.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), d_str.data_ptr(),
                                         d_scr.data_ptr(), d_out_off.data_ptr(), k, pw, len(pw), r_len.data_ptr(),
                                         r_st.data_ptr(), stream)
            if rc != 0:
                raise _mz.MzHipError("crypt batch failed: %d %s" % (rc, L.mzhip_last_error().decode()))
            torch.cuda.synchronize()
            plain_len[sel] = _mz.u32(r_len)
            cst[sel] = r_st.cpu().numpy()
        return d_scr, scr_off, plain_len, cst

    def decode(self, lo=0, hi=None, keep_output=True, verify_hash=False, password=None):
        """Decode entries [lo, hi).  Returns dict(crc u32[n], out_len i64[n], status i32[n], ok bool[n],
        out (uint8 CUDA tensor) , out_off i64[n]).  status: 0, MZ_* / zlib-numbered errors, MZ_CRC_ERROR when
        the CRC differs from the central directory, MZ_SUPPORT_ERROR for methods other than 0 (store) / 8 (DEFLATE) /
        12 (bzip2) / 14 (LZMA) / 93 (zstd) / 95 (xz), for a bzip2 block with the randomised bit and for a zstd frame that names
        a dictionary.
        verify_hash: entries carrying a Hash extrafield are also checked against a device-computed SHA-1 / SHA-256
        (mismatch -> MZ_CRC_ERROR, other algorithms -> MZ_SUPPORT_ERROR, as mz_zip_reader_entry_open / _close).
        password (bytes): ZipCrypto and WinZip-AES entries are decrypted on the device into a scratch buffer (one call per
        kind) and decoded from there by the same per-method launches, AES entries with the real method of their 0x9901
        field; a crypt status other than 0 (MZ_PASSWORD_ERROR, ...) is the entry's status and its codec is not run.  The
        CRC is compared for ZipCrypto and AE-1 and skipped for AE-2, whose CRC field is 0 (mz_zip_entry_read_close,
        mz_zip.c:2116-2128).  Without a password encrypted entries stay MZ_SUPPORT_ERROR."""
        import torch

        t = self.table[lo:hi]
        n = len(t)
        dev = self.device
        usize = t[:, COL_USIZE]
        out_off = np.zeros(n, dtype=np.int64)
        if n:
            np.cumsum(((usize + 15) // 16 * 16)[:-1], out=out_off[1:])
        total = int(out_off[-1] + (usize[-1] + 15) // 16 * 16) if n else 0
        d_out = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        crc = np.zeros(n, dtype=np.uint32)
        out_len = np.zeros(n, dtype=np.int64)
        status = np.full(n, MZ_SUPPORT_ERROR, dtype=np.int32)
        if (t[:, COL_PAYLOAD] < 0).any():
            raise _mz.MzHipError("entry without a usable local header")
        # sizes come from the archive: nothing negative, nothing that reaches past the file image (the indexer already
        # refuses both; a table handed in from elsewhere is checked again here before it becomes device offsets)
        flen = int(self.h_file.size)
        if n and ((t[:, COL_CSIZE] < 0).any() or (usize < 0).any() or (t[:, COL_PAYLOAD] + t[:, COL_CSIZE] > flen).any()):
            raise _mz.MzHipError("entry sizes outside the archive")
        L = _mz.lib()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def dev_i64(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)

        def dev_i32(a):
            return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(dev)

        # where each entry's codec reads its payload: the archive image as it lies in HBM, or -- for entries decrypted just
        # now -- the scratch buffer, the payload shorter by the crypt overhead ("whole entry consumed" is measured on that)
        plain = (t[:, COL_FLAG] & 1) == 0
        meth = np.array(t[:, COL_METHOD], dtype=np.int64)
        skip_crc = np.zeros(n, dtype=bool)
        sources = [(self.d_file, plain, np.array(t[:, COL_PAYLOAD], dtype=np.int64), np.array(t[:, COL_CSIZE], dtype=np.int64))]
        if password is not None and n and not plain.all():
            cf = crypt_fields(self.h_file, t)
            with torch.cuda.device(dev):
                d_scr, scr_off, plain_len, cst = self._decrypt(t, cf, password, stream)
            meth = cf["method"]
            skip_crc = ~plain & (cf["aes_version"] == 2)
            status[~plain & (cst != 0)] = cst[~plain & (cst != 0)]
            sources.append((d_scr, ~plain & (cst == 0), scr_off, plain_len))
        with torch.cuda.device(dev):
            for d_src, from_here, p_off, p_len in sources:
                # DEFLATE entries of LARGE_ENTRY compressed bytes and more: one wave per entry is 0.1 - 0.2 GB/s, so each of them
                # is decoded by a wave per DEFLATE block (mzhip_inflate_large, csrc/inflate_parallel.inc), one call per entry
                large = np.nonzero((meth == 8) & from_here & (p_len >= LARGE_ENTRY))[0]
                if len(large) and ((p_len[large] >= 2**32) | (usize[large] >= 2**32)).any():
                    raise _mz.MzHipError("entries >= 4 GiB are outside the batch path")
                L.mzhip_inflate_large.restype = C.c_int32
                L.mzhip_inflate_large.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
                for e in large:
                    ol, iu, ck, st1 = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int32()
                    rc = L.mzhip_inflate_large(d_src.data_ptr() + int(p_off[e]), int(p_len[e]),
                                               d_out.data_ptr() + int(out_off[e]), int(usize[e]), C.byref(ol), C.byref(iu), C.byref(ck),
                                               C.byref(st1), stream)
                    if rc != 0:
                        raise _mz.MzHipError("mzhip_inflate_large failed: %d %s" % (rc, L.mzhip_last_error().decode()))
                    crc[e], out_len[e] = ck.value, ol.value
                    status[e] = MZ_CRC_ERROR if (st1.value == 0 and iu.value == p_len[e] and not skip_crc[e] and ck.value != np.uint32(t[e, COL_CRC])) else st1.value
                # ... and Zstandard entries of LARGE_ZSTD_ENTRY compressed bytes and more by a wave per Zstandard block
                # (mzhip_zstd_large, csrc/zstd_parallel.inc): every field is what the batch launch gives for the entry
                large_z = np.nonzero((meth == 93) & from_here & (p_len >= LARGE_ZSTD_ENTRY))[0]
                if len(large_z) and ((p_len[large_z] >= 2**31) | (usize[large_z] >= 2**31)).any():
                    raise _mz.MzHipError("entries >= 2 GiB are outside the batch path")
                for e in large_z:
                    ol, iu, ck, st1 = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int32()
                    rc = L.mzhip_zstd_large(d_src.data_ptr() + int(p_off[e]), int(p_len[e]), d_out.data_ptr() + int(out_off[e]),
                                            int(usize[e]), 0, C.byref(ol), C.byref(iu), C.byref(ck), C.byref(st1), None, stream)
                    if rc != 0:
                        raise _mz.MzHipError("mzhip_zstd_large failed: %d %s" % (rc, L.mzhip_last_error().decode()))
                    crc[e], out_len[e] = ck.value, ol.value
                    status[e] = MZ_CRC_ERROR if (st1.value == 0 and iu.value == p_len[e] and not skip_crc[e] and ck.value != np.uint32(t[e, COL_CRC])) else st1.value
                routed = ((meth == 8) & (p_len >= LARGE_ENTRY)) | ((meth == 93) & (p_len >= LARGE_ZSTD_ENTRY))
                for method in (8, 12, 93, 14, 95, 0):
                    sel = np.nonzero((meth == method) & from_here & ~routed)[0]
                    if len(sel) == 0:
                        continue
                    k = len(sel)
                    if (p_len[sel] >= 2**31).any() or (usize[sel] >= 2**31).any():
                        raise _mz.MzHipError("entries >= 2 GiB are outside the batch path")
                    d_in_off, d_in_len = dev_i64(p_off[sel]), dev_i32(p_len[sel])
                    d_out_off, d_cap = dev_i64(out_off[sel]), dev_i32(usize[sel])
                    r_len, r_used, r_crc, r_st = (torch.zeros(k, dtype=torch.int32, device=dev) for _ in range(4))
                    if method in (8, 12, 93):   # bzip2: one stream per entry, as BZ2_bzDecompress reads it (mz_strm_bzip.c);
                        # zstd: the entry's frames, as ZSTD_decompress reads them (mz_strm_zstd.c)
                        fn = {8: L.mzhip_inflate_batch, 12: L.mzhip_bzip2_batch, 93: L.mzhip_zstd_batch}[method]
                        rc = fn(d_src.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(),
                                d_out.data_ptr(), d_out_off.data_ptr(), d_cap.data_ptr(), k,
                                r_len.data_ptr(), r_used.data_ptr(), r_crc.data_ptr(), r_st.data_ptr(),
                                stream)
                    elif method in (14, 95):
                        fn = L.mzhip_lzma_batch if method == 14 else L.mzhip_xz_batch
                        fn.restype = C.c_int32
                        fn.argtypes = [C.c_void_p] * 7 + [C.c_uint32] + [C.c_void_p] * 5
                        # TOTAL_OUT_MAX = uncompressed size when the EOS flag is set (mz_zip.c:1833-1846), else none
                        d_max = dev_i64(np.where(t[sel, COL_FLAG] & 2, usize[sel], -1))
                        rc = fn(d_src.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(),
                                d_out.data_ptr(), d_out_off.data_ptr(), d_cap.data_ptr(), d_max.data_ptr(),
                                k, r_len.data_ptr(), r_used.data_ptr(), r_crc.data_ptr(), r_st.data_ptr(), stream)
                    else:   # STORE: the payload IS the data (mz_stream_raw, mz_zip.c:1769); CRC in place, then copy
                        rc = L.mzhip_crc32_batch(d_src.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), k, None,
                                                 r_crc.data_ptr(), stream)
                        r_len = d_in_len.clone()
                        r_used = d_in_len.clone()
                        # a stored entry's two sizes must agree (the slot was sized from the uncompressed one): anything
                        # else is a format error and nothing is copied for it
                        same = p_len[sel] == usize[sel]
                        r_st = dev_i32(np.where(same, 0, MZ_FORMAT_ERROR))
                        if keep_output:
                            for j, e in enumerate(sel):   # host-driven D2D copies: STORE is the CPU-plumbing config
                                if not same[j]:
                                    continue
                                c0, cl = int(p_off[e]), int(p_len[e])
                                d_out[out_off[e]:out_off[e] + cl] = d_src[c0:c0 + cl]
                    if rc != 0:
                        raise _mz.MzHipError("batch launch failed: %d %s" % (rc, L.mzhip_last_error().decode()))
                    torch.cuda.synchronize()
                    crc[sel] = _mz.u32(r_crc)
                    out_len[sel] = r_len.cpu().numpy()
                    st = r_st.cpu().numpy().astype(np.int32)
                    used = r_used.cpu().numpy().astype(np.int64)
                    # mz_zip_entry_read_close: CRC is verified iff the whole entry was consumed (mz_zip.c:2116-2128)
                    bad_crc = (st == 0) & (used == p_len[sel]) & ~skip_crc[sel] & (crc[sel] != t[sel, COL_CRC].astype(np.uint32))
                    st[bad_crc] = MZ_CRC_ERROR
                    status[sel] = st
        if verify_hash and n:
            alg, dsz, dig = hash_fields(self.h_file, t)
            status[(alg != 0) & (alg != MZ_HASH_SHA1) & (alg != MZ_HASH_SHA256) & (status == 0)] = MZ_SUPPORT_ERROR
            L.mzhip_sha_batch.restype = C.c_int32
            L.mzhip_sha_batch.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 2
            with torch.cuda.device(dev):
                for a_id in (MZ_HASH_SHA1, MZ_HASH_SHA256):
                    sel = np.nonzero((alg == a_id) & (status == 0))[0]
                    if len(sel) == 0:
                        continue
                    if not keep_output and (t[sel, COL_METHOD] == 0).any():
                        raise _mz.MzHipError("verify_hash of STORE entries needs keep_output")
                    d_dig = torch.zeros(len(sel) * 32, dtype=torch.uint8, device=dev)
                    d_o, d_l = dev_i64(out_off[sel]), dev_i32(out_len[sel])   # keep both alive across the launch
                    rc = L.mzhip_sha_batch(d_out.data_ptr(), d_o.data_ptr(), d_l.data_ptr(), len(sel), a_id,
                                           d_dig.data_ptr(), stream)
                    if rc != 0:
                        raise _mz.MzHipError("mzhip_sha_batch failed: %d" % rc)
                    torch.cuda.synchronize()
                    got = d_dig.cpu().numpy().reshape(len(sel), 32)
                    for j, e in enumerate(sel):   # memcmp over the extrafield's digest size (mz_zip_rw.c:446-447)
                        k = min(int(dsz[e]), 32)
                        if not (got[j, :k] == dig[e, :k]).all():
                            status[e] = MZ_CRC_ERROR
        ok = (status == 0) & (out_len == usize)
        return dict(crc=crc, out_len=out_len, status=status, ok=ok, out=d_out if keep_output else None,
                    out_off=out_off)


# ---- the writer: compress -> encrypt -> container --------------------------------------------------------------------------

ZIP32_MAX = 0xFFFFFFFF        # a size or offset field holding this value announces ZIP64, which is not written
ZIP32_MAX_ENTRIES = 0xFFFF    # ... and so does an entry count of 65 535: the largest count written is 65 534


def crypt_overhead(kind, strength=3):
    """bytes the crypt stream adds to an entry's payload: 12 (ZipCrypto), 4 s + 16 (WinZip AES), 0"""
    return 0 if kind is None else 12 if kind == "pk" else 4 * strength + 16


ENCODE_ARCHIVE_METHODS = (0, 8, 12, 14)   # what encode_archive takes; encode_zstd_archive is the door to 93


def _check_writer_args(n, method, kind, strength, ae_version, allowed=ENCODE_ARCHIVE_METHODS):
    if method not in allowed:
        if allowed == ENCODE_ARCHIVE_METHODS:
            raise _mz.MzHipError("encode_archive writes methods 0, 8, 12 and 14, not %r" % (method,))
        raise _mz.MzHipError("methods %s are written, not %r" % (", ".join(str(m) for m in allowed), method))
    if kind not in (None, "pk", "aes"):
        raise _mz.MzHipError("kind is None, 'pk' or 'aes', not %r" % (kind,))
    if kind == "aes" and (strength not in (1, 2, 3) or ae_version not in (1, 2)):
        raise _mz.MzHipError("WinZip AES: strength 1..3 and AE-1 or AE-2")
    if n >= ZIP32_MAX_ENTRIES:
        raise _mz.MzHipError("%d entries need ZIP64, which is not written" % n)


def assemble_archive(names, payloads, crcs, usizes, method=8, kind=None, strength=3, ae_version=2, mtime=None):
    """The host side of encode_archive: local headers, the central directory and one end record around payloads that are
    already what the archive stores (compressed with `method`, then encrypted as `kind` says: mz_zip_entry_write_header,
    mz_zip.c).  crcs / usizes: CRC-32 and length of the plain data.  No data descriptor is written (sizes and CRCs are
    known before any header is), so flag bit 3 stays clear and ZipCrypto's check bytes are the CRC's two high bytes.  AES
    entries are method 99 with the 7-byte 0x9901 field (version, "AE", strength, the real method) in both headers, version
    needed 51, and -- AE-2 -- CRC 0.  Method 14 sets flag bit 1 (the stream ends in a marker) and needs version 63, method 12
    (bzip2) version 46 (mz_zip.c:710-712) and no flag bit of its own, method 93 (Zstandard) version 20 (mz_zip.c:704-723 has no
    case for it) and no flag bit either.  Whatever would need ZIP64 is refused."""
    import struct
    import time

    n = len(names)
    _check_writer_args(n, method, kind, strength, ae_version, ENCODE_ARCHIVE_METHODS + (93,))
    if not (len(payloads) == len(crcs) == len(usizes) == n):
        raise _mz.MzHipError("names, payloads, crcs and usizes differ in length")
    tm = time.localtime() if mtime is None else mtime
    dos_time = (tm[3] << 11) | (tm[4] << 5) | (tm[5] >> 1)
    dos_date = (max(tm[0] - 1980, 0) << 9) | (tm[1] << 5) | tm[2]
    out, cd = bytearray(), bytearray()
    for name, payload, crc, usize in zip(names, payloads, crcs, usizes):
        raw = name.encode("utf-8") if isinstance(name, str) else bytes(name)
        crc, usize = int(crc) & 0xFFFFFFFF, int(usize)
        flag = (1 if kind else 0) | (2 if method == 14 else 0) | (0 if raw.isascii() else 0x800)
        zmethod, extra, need = method, b"", 63 if method == 14 else 46 if method == 12 else 20
        if kind == "aes":
            extra = struct.pack("<HHH2sBH", MZ_ZIP_EXTENSION_AES, 7, ae_version, b"AE", strength, method)
            zmethod, need = MZ_COMPRESS_METHOD_AES, 51
            if ae_version == 2:
                crc = 0
        off = len(out)
        if max(usize, len(payload), off) >= ZIP32_MAX or len(raw) > 0xFFFF:
            raise _mz.MzHipError("entry %r needs ZIP64 (a size or offset of 4 GiB), which is not written" % (name,))
        out += struct.pack("<IHHHHHIIIHH", 0x04034B50, need, flag, zmethod, dos_time, dos_date, crc, len(payload), usize,
                           len(raw), len(extra))
        out += raw + extra
        out += payload
        cd += struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, need, need, flag, zmethod, dos_time, dos_date, crc,
                          len(payload), usize, len(raw), len(extra), 0, 0, 0, 0, off)
        cd += raw + extra
    if max(len(out), len(cd)) >= ZIP32_MAX:
        raise _mz.MzHipError("the archive needs ZIP64 (4 GiB), which is not written")
    cd_off = len(out)
    out += cd
    out += struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, n, n, len(cd), cd_off, 0)
    return bytes(out)


def encode_archive(entries, method=8, level=6, password=None, kind=None, strength=3, ae_version=2, entropy=os.urandom,
                   device="cuda:0"):
    """entries: (name, bytes-like) pairs -> the bytes of a ZIP archive, every entry compressed with `method` (0, 8, 12 or 14) at
    `level` (method 12: the block-size digit 1..9, -1 = 6) and, with a password, encrypted as `kind` says ("pk" = ZipCrypto,
    "aes" = WinZip AES of `strength` 1..3, AE-1 or AE-2).  One upload of the data, ONE codec launch (mzhip_deflate_batch_level,
    mzhip_bzip2_encode_batch with capacities from mzhip_bzip2_encode_bound, mzhip_lzma_encode_batch_preset in mode 0,
    mzhip_crc32_batch for STORE) whose CRC words are the entries' CRCs, ZipCrypto's check bytes derived from those words on
    the device, 10 n / 16 n bytes drawn from `entropy` (a callable: byte count -> bytes), ONE encrypt call
    (mzhip_pkcrypt_encrypt_batch / mzhip_wzaes_encrypt_batch) straight from the codec's output, one copy back, and
    assemble_archive on the host.  Not written: ZIP64 (65 535 entries or more, 4 GiB sizes or offsets: MzHipError), data
    descriptors, method 95, and -- through this function -- method 93 (encode_zstd_archive)."""
    return _encode_archive(ENCODE_ARCHIVE_METHODS, entries, method, level, 0, password, kind, strength, ae_version, entropy, device)


def encode_zstd_archive(entries, level=3, checksum=False, password=None, kind=None, strength=3, ae_version=2, entropy=os.urandom,
                        device="cuda:0"):
    """encode_archive for ZIP method 93: every entry one Zstandard frame through mzhip_zstd_encode_batch (capacities from
    mzhip_zstd_encode_bound) at `level` (1..22, -1 and 0 = 3), with the XXH64 content checksum if `checksum`; version needed 20,
    or method 99 / version 51 with the real method in the 0x9901 field behind WinZip AES.  Everything else -- upload, CRCs,
    encryption, container -- is encode_archive's own body.  It has a name of its own because encode_archive(method=93) is
    pinned to raise MzHipError (tests/test_gpu_bzip2_enc.py::test_encode_archive_still_refuses); lifting that refusal is a
    one-line change there once that test may change."""
    return _encode_archive((93,), entries, 93, level, 1 if checksum else 0, password, kind, strength, ae_version, entropy, device)


def _encode_archive(allowed, entries, method, level, zflags, password, kind, strength, ae_version, entropy, device):
    """the body of encode_archive and encode_zstd_archive; allowed: the methods the caller takes"""
    import torch

    entries = [(name, np.frombuffer(bytes(data), dtype=np.uint8)) for name, data in entries]
    n = len(entries)
    _check_writer_args(n, method, kind, strength, ae_version, allowed)
    if (kind is None) != (password is None):
        raise _mz.MzHipError("a kind needs a password and a password needs a kind")
    usize = np.array([d.size for _, d in entries], dtype=np.int64)
    over = crypt_overhead(kind, strength)
    slack = 0 if method == 0 else 64 if method == 8 else 1024          # include/mzhip.h: what always suffices
    cap = usize if method == 0 else usize + usize // 8 + slack
    if method == 12:
        if level != -1 and level not in range(1, 10):
            raise _mz.MzHipError("method 12: level is the block-size digit 1..9 (or -1 = 6), not %r" % (level,))
        cap = np.array([_mz.bzip2_encode_bound(int(u), level) for u in usize], dtype=np.int64)
    if method == 93:
        if level not in range(-1, 23):
            raise _mz.MzHipError("method 93: level is 1..22 (or -1 / 0 = 3), not %r" % (level,))
        cap = np.array([_mz.zstd_encode_bound(int(u)) for u in usize], dtype=np.int64)
    if n and int((cap + over).max()) >= ZIP32_MAX:
        raise _mz.MzHipError("an entry of 4 GiB needs ZIP64, which is not written")
    names = [name for name, _ in entries]
    if n == 0:
        return assemble_archive([], [], [], [], method, kind, strength, ae_version)
    _mz.require_gpu()
    dev = torch.device(device)
    L = _mz.lib()

    def offsets(sizes):   # 16-byte aligned slots -> (offsets, total)
        slot = (sizes + 15) // 16 * 16
        off = np.zeros(n, dtype=np.int64)
        np.cumsum(slot[:-1], out=off[1:])
        return off, int(off[-1] + slot[-1])

    def dev_u32(a):
        return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32).view(np.int32)).to(dev)

    in_off, in_total = offsets(usize)
    blob = np.zeros(max(in_total, 16), dtype=np.uint8)
    for o, (_, d) in zip(in_off, entries):
        blob[o:o + d.size] = d
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        d_in = torch.from_numpy(blob).to(dev)
        d_in_off, d_in_len = torch.from_numpy(in_off).to(dev), dev_u32(usize)
        r_len, r_crc, r_st = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
        if method == 0:
            rc = L.mzhip_crc32_batch(d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), n, None, r_crc.data_ptr(), stream)
            d_comp, d_comp_off, r_len = d_in, d_in_off, d_in_len
        else:
            comp_off, comp_total = offsets(cap)
            d_comp = torch.empty(max(comp_total, 16), dtype=torch.uint8, device=dev)
            d_comp_off, d_cap = torch.from_numpy(comp_off).to(dev), dev_u32(cap)
            if method == 8:
                rc = L.mzhip_deflate_batch_level(d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), d_comp.data_ptr(),
                                                 d_comp_off.data_ptr(), d_cap.data_ptr(), None, n, level, 15, r_len.data_ptr(),
                                                 r_crc.data_ptr(), r_st.data_ptr(), stream)
            elif method == 12:
                rc = L.mzhip_bzip2_encode_batch(d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), int(usize.max()),
                                                d_comp.data_ptr(), d_comp_off.data_ptr(), d_cap.data_ptr(), n, level,
                                                r_len.data_ptr(), r_crc.data_ptr(), r_st.data_ptr(), stream)
            elif method == 93:
                rc = L.mzhip_zstd_encode_batch(d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), int(usize.max()),
                                               d_comp.data_ptr(), d_comp_off.data_ptr(), d_cap.data_ptr(), n, level, zflags,
                                               r_len.data_ptr(), r_crc.data_ptr(), r_st.data_ptr(), stream)
            else:
                rc = L.mzhip_lzma_encode_batch_preset(d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), int(usize.max()),
                                                      d_comp.data_ptr(), d_comp_off.data_ptr(), d_cap.data_ptr(), None, n, level,
                                                      r_len.data_ptr(), r_crc.data_ptr(), r_st.data_ptr(), stream)
        if rc != 0:
            raise _mz.MzHipError("codec launch failed: %d %s" % (rc, L.mzhip_last_error().decode()))
        e_len, e_st = r_len, torch.zeros(n, dtype=torch.int32, device=dev)
        d_pay, pay_off = d_comp, None
        if kind is not None:
            pw = bytes(password)
            pay_off, pay_total = offsets(cap + over)
            d_pay = torch.empty(max(pay_total, 16), dtype=torch.uint8, device=dev)
            d_pay_off = torch.from_numpy(pay_off).to(dev)
            e_len = torch.zeros(n, dtype=torch.int32, device=dev)
            rnd = bytes(entropy((10 if kind == "pk" else 16) * n))
            if len(rnd) != (10 if kind == "pk" else 16) * n:
                raise _mz.MzHipError("entropy() returned %d bytes" % len(rnd))
            d_rnd = torch.from_numpy(np.frombuffer(rnd, dtype=np.uint8).copy()).to(dev)
            if kind == "pk":
                # plain header byte 11 = the CRC's top byte, byte 10 the next one (mz_zip_get_pk_verify, flag bit 3 clear)
                d_ver = (((r_crc >> 24) & 255) | (((r_crc >> 16) & 255) << 8)).to(torch.int32)
                rc = L.mzhip_pkcrypt_encrypt_batch(d_comp.data_ptr(), d_comp_off.data_ptr(), r_len.data_ptr(), d_pay.data_ptr(),
                                                   d_pay_off.data_ptr(), n, pw, len(pw), d_ver.data_ptr(), d_rnd.data_ptr(),
                                                   e_len.data_ptr(), e_st.data_ptr(), stream)
            else:
                d_str = torch.full((n,), strength, dtype=torch.uint8, device=dev)
                rc = L.mzhip_wzaes_encrypt_batch(d_comp.data_ptr(), d_comp_off.data_ptr(), r_len.data_ptr(), d_str.data_ptr(),
                                                 d_rnd.data_ptr(), d_pay.data_ptr(), d_pay_off.data_ptr(), n, pw, len(pw),
                                                 e_len.data_ptr(), e_st.data_ptr(), stream)
            if rc != 0:
                raise _mz.MzHipError("encrypt launch failed: %d %s" % (rc, L.mzhip_last_error().decode()))
        res = torch.stack((r_crc, r_st, e_len, e_st)).cpu().numpy()   # (synchronises with the stream)
        crc, c_st, p_len, p_st = res[0].view(np.uint32), res[1], res[2].view(np.uint32).astype(np.int64), res[3]
        if (c_st != 0).any() or (p_st != 0).any():
            i = int(np.flatnonzero((c_st != 0) | (p_st != 0))[0])
            raise _mz.MzHipError("entry %d (%r): codec status %d, crypt status %d" % (i, names[i], c_st[i], p_st[i]))
        if method == 0 and kind is None:
            payloads = [d.tobytes() for _, d in entries]   # the payload IS the data: nothing to copy back
        else:
            h_pay = d_pay.cpu().numpy()
            if pay_off is None:
                pay_off = comp_off
            payloads = [h_pay[int(o):int(o) + int(k)].tobytes() for o, k in zip(pay_off, p_len)]
    return assemble_archive(names, payloads, crc, usize, method, kind, strength, ae_version)
