// zstd_parallel.inc -- ONE large Zstandard entry decoded by a wave per block (host side, C++): the logic between the
// passes of zstd_par_core.h.
//
// The batch kernel gives an entry one wave, a few MiB/s on an entry of many MiB.  A Zstandard block's end stands in its
// header, so the blocks are known after one walk over the headers (scan); what a block takes from the blocks before it
// is named or computed HERE, in O(blocks), so that no wave waits for another:
//   definers   the nearest earlier block of the same frame that describes a Huffman tree (for treeless literals) or a
//              sequence table in a mode other than Repeat (Predefined and RLE are descriptions too), with at least one
//              sequence; a block without one where it needs one is a problem;
//   positions  the prefix sum of the bytes the count pass reports;
//   offsets    the count pass reports the three repeat offsets behind a block as a function of those in front of it
//              (a distance, or "incoming slot j minus k"); the functions are composed along each frame from (1, 4, 8);
//   windows    the source map costs 4 bytes per output byte, so emit and resolve run over windows of output, cut at block
//              boundaries; the history of a window is everything in front of it, resolved already, hence final.
// Any problem in any pass -- and an entry of more blocks than the arrays hold -- hands the WHOLE entry to the one-wave
// reader: its status rule is not restated here.
//
// The passes are the backend's (the device: kernel launches in mzhip_launch.inc; the tests: loops over the 64-lane
// emulation of the same device functions, tests/emul/emul_zstd_large.cpp).
//   scan(blk_cap, recs, frms, hdr)        records of MZ_ZSP_REC_WORDS / MZ_ZSP_FRM_WORDS words, hdr of MZ_ZSP_HDR_WORDS
//   blocks(mode, jobs, n, bias, res)      mode 1 count, 2 emit; the source map belongs to out[bias ..)
//   resolve(w0, w1, &rounds)              pointer jumping and the gather over out[w0 .. w1)
//   xxh(spans, n, vals)                   low 32 bits of XXH64 of out[spans[2 i] .. + spans[2 i + 1])
#include <stdint.h>
#include <vector>

struct MzZsLarge {
    uint32_t windows = 0, blocks = 0, borrowed = 0, rounds = 0;
    uint32_t fallback = 0; // 0 decoded here; 1 a problem was met; 2 the block cap
    uint32_t out_len = 0;  // fallback 0: the entry's bytes (the whole input was used)
};

template <class B>
static int32_t mz_zstd_large_entry(B &be, uint32_t in_len, uint32_t out_cap, uint32_t window, MzZsLarge *r) {
    *r = MzZsLarge();
    const auto give_up = [&](uint32_t why) {
        *r = MzZsLarge();
        r->fallback = why;
        return 0;
    };
    const uint32_t blk_cap = in_len / 3u + 1u < MZ_ZSP_BLOCK_CAP ? in_len / 3u + 1u : MZ_ZSP_BLOCK_CAP; // (a block is 3 bytes at least)
    std::vector<uint32_t> recs, frms;
    uint32_t hdr[MZ_ZSP_HDR_WORDS] = {0};
    int32_t rc = be.scan(blk_cap, recs, frms, hdr);
    if (rc) return rc;
    if (hdr[MZ_ZSP_H_STOP] == 1u) return give_up(2u);
    if (hdr[MZ_ZSP_H_STOP] != 0u) return give_up(1u);
    const uint32_t nblk = hdr[MZ_ZSP_H_NBLK], nfrm = hdr[MZ_ZSP_H_NFRM];
    if (recs.size() < (size_t)nblk * MZ_ZSP_REC_WORDS || frms.size() < (size_t)nfrm * MZ_ZSP_FRM_WORDS) return give_up(1u);

    // ---- definers
    std::vector<uint32_t> jobs((size_t)nblk * MZ_ZSP_JOB_WORDS, 0u);
    std::vector<uint32_t> comp; // the Compressed blocks: the count pass's work
    uint32_t borrowed = 0;
    {
        uint32_t frame = 0xFFFFFFFFu;
        const uint32_t *tree = nullptr, *tab[3] = {nullptr, nullptr, nullptr};
        for (uint32_t i = 0; i < nblk; i++) {
            const uint32_t *rec = &recs[(size_t)i * MZ_ZSP_REC_WORDS];
            uint32_t *job = &jobs[(size_t)i * MZ_ZSP_JOB_WORDS];
            if (rec[MZ_ZSP_R_FRAME] != frame) { // nothing crosses frames
                frame = rec[MZ_ZSP_R_FRAME];
                if (frame >= nfrm) return give_up(1u);
                tree = tab[0] = tab[1] = tab[2] = nullptr;
            }
            job[MZ_ZSP_J_OFF] = rec[MZ_ZSP_R_OFF];
            job[MZ_ZSP_J_SIZE] = rec[MZ_ZSP_R_SIZE];
            job[MZ_ZSP_J_TYPE] = rec[MZ_ZSP_R_TYPE] & 3u;
            job[MZ_ZSP_J_BLKMAX] = frms[(size_t)frame * MZ_ZSP_FRM_WORDS + MZ_ZSP_F_BLKMAX];
            job[MZ_ZSP_J_REGEN] = rec[MZ_ZSP_R_REGEN];
            job[MZ_ZSP_J_SEQ] = rec[MZ_ZSP_R_SEQ];
            if ((rec[MZ_ZSP_R_TYPE] & 3u) != 2u) continue;
            comp.push_back(i);
            bool borrows = false;
            const uint32_t lt = rec[MZ_ZSP_R_LIT] & 3u;
            if (lt == 2u) {
                tree = rec;
            } else if (lt == 3u) {
                if (!tree) return give_up(1u);
                job[MZ_ZSP_J_TREE] = tree[MZ_ZSP_R_TREE];
                job[MZ_ZSP_J_TREE_END] = tree[MZ_ZSP_R_TREE] + tree[MZ_ZSP_R_COMP];
                borrows = true;
            }
            if (rec[MZ_ZSP_R_NSEQ]) {
                for (uint32_t t = 0; t < 3u; t++) {
                    if (((rec[MZ_ZSP_R_MODES] >> (6u - 2u * t)) & 3u) != 3u) {
                        tab[t] = rec;
                        continue;
                    }
                    if (!tab[t]) return give_up(1u);
                    job[MZ_ZSP_J_DEF + 3u * t] = tab[t][MZ_ZSP_R_TABS];
                    job[MZ_ZSP_J_DEF + 3u * t + 1u] = tab[t][MZ_ZSP_R_MODES];
                    job[MZ_ZSP_J_DEF + 3u * t + 2u] = tab[t][MZ_ZSP_R_OFF] + 3u + tab[t][MZ_ZSP_R_SIZE];
                    borrows = true;
                }
            }
            borrowed += borrows ? 1u : 0u;
        }
    }

    // ---- count: the bytes of every Compressed block and its repeat-offset function
    std::vector<uint32_t> res((size_t)(comp.size() ? comp.size() : 1u) * MZ_ZSP_RES_WORDS, 0u);
    if (!comp.empty()) {
        std::vector<uint32_t> cj(comp.size() * (size_t)MZ_ZSP_JOB_WORDS);
        for (size_t k = 0; k < comp.size(); k++)
            std::copy(&jobs[(size_t)comp[k] * MZ_ZSP_JOB_WORDS], &jobs[(size_t)comp[k] * MZ_ZSP_JOB_WORDS] + MZ_ZSP_JOB_WORDS, &cj[k * MZ_ZSP_JOB_WORDS]);
        rc = be.blocks(1u, cj.data(), (uint32_t)comp.size(), 0u, res.data());
        if (rc) return rc;
    }

    // ---- positions, repeat offsets, frame sizes
    std::vector<uint32_t> spans;
    std::vector<uint32_t> checks;
    {
        uint64_t at = 0, fo = 0;
        uint32_t rep[3] = {1u, 4u, 8u}, frame = 0xFFFFFFFFu;
        size_t k = 0;
        for (uint32_t i = 0; i < nblk; i++) {
            const uint32_t *rec = &recs[(size_t)i * MZ_ZSP_REC_WORDS];
            uint32_t *job = &jobs[(size_t)i * MZ_ZSP_JOB_WORDS];
            uint32_t bytes = rec[MZ_ZSP_R_SIZE];
            if (rec[MZ_ZSP_R_FRAME] != frame) {
                frame = rec[MZ_ZSP_R_FRAME];
                fo = at;
                rep[0] = 1u;
                rep[1] = 4u;
                rep[2] = 8u;
            }
            job[MZ_ZSP_J_FO] = (uint32_t)fo;
            for (uint32_t s = 0; s < 3u; s++) job[MZ_ZSP_J_REP0 + s] = rep[s];
            if ((rec[MZ_ZSP_R_TYPE] & 3u) == 2u) {
                const uint32_t *o = &res[k * MZ_ZSP_RES_WORDS];
                uint32_t next[3];
                k++;
                if (o[MZ_ZSP_O_STATUS]) return give_up(1u);
                bytes = o[MZ_ZSP_O_BYTES];
                for (uint32_t s = 0; s < 3u; s++) {
                    const uint32_t src = o[MZ_ZSP_O_REP + 2u * s], val = o[MZ_ZSP_O_REP + 2u * s + 1u];
                    if (src == 3u) {
                        next[s] = val;
                    } else {
                        if (src > 2u || rep[src] <= val) return give_up(1u); // an offset that resolves to 0 (or below)
                        next[s] = rep[src] - val;
                    }
                }
                for (uint32_t s = 0; s < 3u; s++) rep[s] = next[s];
            }
            if (bytes > (uint64_t)out_cap - at) return give_up(1u);
            job[MZ_ZSP_J_POS] = (uint32_t)at;
            at += bytes;
            job[MZ_ZSP_J_END] = (uint32_t)at;
            if (rec[MZ_ZSP_R_TYPE] & 4u) { // the frame's last block
                const uint32_t *f = &frms[(size_t)frame * MZ_ZSP_FRM_WORDS];
                if ((f[MZ_ZSP_F_FLAGS] & 1u) && (at - fo) != (((uint64_t)f[MZ_ZSP_F_FCS_HI] << 32) | f[MZ_ZSP_F_FCS_LO])) return give_up(1u);
                if (f[MZ_ZSP_F_FLAGS] & 2u) {
                    spans.push_back((uint32_t)fo);
                    spans.push_back((uint32_t)(at - fo));
                    checks.push_back(f[MZ_ZSP_F_CHECK]);
                }
            }
        }
        r->out_len = (uint32_t)at;
    }

    // ---- emit and resolve, window after window
    const uint32_t win = window > MZ_ZS_BLOCK_MAX ? window : MZ_ZS_BLOCK_MAX; // (the map holds one block at least)
    std::vector<uint32_t> eres;
    for (uint32_t i0 = 0; i0 < nblk;) {
        const uint32_t w0 = jobs[(size_t)i0 * MZ_ZSP_JOB_WORDS + MZ_ZSP_J_POS];
        uint32_t i1 = i0 + 1u;
        while (i1 < nblk && jobs[(size_t)i1 * MZ_ZSP_JOB_WORDS + MZ_ZSP_J_END] - w0 <= window) i1++;
        const uint32_t w1 = jobs[(size_t)(i1 - 1u) * MZ_ZSP_JOB_WORDS + MZ_ZSP_J_END];
        if (w1 - w0 > win) return give_up(1u);
        eres.assign((size_t)(i1 - i0) * MZ_ZSP_RES_WORDS, 0u);
        rc = be.blocks(2u, &jobs[(size_t)i0 * MZ_ZSP_JOB_WORDS], i1 - i0, w0, eres.data());
        if (rc) return rc;
        for (uint32_t i = i0; i < i1; i++) {
            const uint32_t *o = &eres[(size_t)(i - i0) * MZ_ZSP_RES_WORDS], *job = &jobs[(size_t)i * MZ_ZSP_JOB_WORDS];
            if (o[MZ_ZSP_O_STATUS] || o[MZ_ZSP_O_BYTES] != job[MZ_ZSP_J_END] - job[MZ_ZSP_J_POS]) return give_up(1u);
        }
        if (w1 > w0) {
            rc = be.resolve(w0, w1, &r->rounds);
            if (rc) return rc;
        }
        r->windows++;
        i0 = i1;
    }

    // ---- content checksums: one wave per frame over the resolved bytes
    if (!checks.empty()) {
        std::vector<uint32_t> vals(checks.size(), 0u);
        rc = be.xxh(spans.data(), (uint32_t)checks.size(), vals.data());
        if (rc) return rc;
        for (size_t k = 0; k < checks.size(); k++)
            if (vals[k] != checks[k]) return give_up(1u);
    }
    r->blocks = nblk;
    r->borrowed = borrowed;
    return 0;
}
