// deflate_tokens.cpp -- a reader of raw DEFLATE that reports what a stream is MADE of: its blocks (kind, BFINAL, the bits they
// take, the bytes they stand for) and its matches (position, length, distance).  Written from RFC 1951 alone (the same text
// as appnote.txt:2030-2166): section 3.1.1 for the bit order, 3.2.2 for the canonical codes, 3.2.4 for stored blocks, 3.2.5
// for the length / distance alphabets, 3.2.6 for the fixed code and 3.2.7 for the dynamic header.  It shares nothing with the
// decoders of this project or with the oracle restatement: tests/deflate_tokens.py compiles it on first use and the encoder
// tests measure the encoder's promises (window, block choice, piece framing) with it.  Everything RFC 1951 forbids is an
// error with the bit and the output position it was seen at.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Block {
    uint64_t btype, bfinal, first_bit, end_bit, out_start, out_end;
};
struct Match {
    int64_t out_pos, length, distance;
};

struct Walk {
    std::vector<Block> blocks;
    std::vector<Match> matches;
    std::vector<uint8_t> bytes;
    uint64_t bits = 0, out = 0;
    int err = 0;
    char msg[200] = {0};
};

// 3.2.5: base values and extra bits of the length symbols 257..285 and the distance symbols 0..29
const uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
const uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const uint16_t DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                                4097, 6145, 8193, 12289, 16385, 24577};
const uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
// 3.2.7: the order in which the code lengths of the code-length alphabet are sent
const uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct Fail {};

struct Reader {
    const uint8_t *z;
    uint64_t nbits, pos = 0;
    Walk *w;

    [[noreturn]] void fail(const char *what) {
        w->err = 1;
        snprintf(w->msg, sizeof w->msg, "%s (bit %llu of %llu, output byte %llu)", what, (unsigned long long)pos, (unsigned long long)nbits,
                 (unsigned long long)w->out);
        throw Fail();
    }
    // up to 32 bits, least significant bit first (3.1.1); bits behind the input read as zeros, take() refuses to use them
    uint32_t peek(uint32_t n) const {
        uint64_t v = 0;
        const uint64_t byte = pos >> 3, total = (nbits + 7) >> 3;
        for (uint32_t k = 0; k < 6; k++)
            if (byte + k < total) v |= (uint64_t)z[byte + k] << (8 * k);
        return (uint32_t)((v >> (pos & 7)) & ((n == 32) ? 0xFFFFFFFFull : ((1ull << n) - 1)));
    }
    void skip(uint32_t n) {
        if (pos + n > nbits) fail("the input ends before the final block does");
        pos += n;
    }
    uint32_t take(uint32_t n) {
        const uint32_t v = peek(n);
        skip(n);
        return v;
    }
};

// One canonical prefix code (3.2.2) as a table over the next `maxbits` bits of the input: entry = symbol | length << 16, 0 =
// no code starts like this.
struct Code {
    std::vector<uint32_t> tab;
    uint32_t maxbits = 0;
    bool empty = true;

    // kind: what to call the set in a message.  one_bit_ok: a set made of a single code of one bit is taken as it is (what
    // zlib writes, and accepts, for the distances of a block with one distance); its other code stays unassigned.
    void build(Reader &r, const uint8_t *len, uint32_t n, const char *kind, bool one_bit_ok, bool none_ok) {
        uint32_t count[16] = {0};
        for (uint32_t s = 0; s < n; s++) count[len[s]]++;
        maxbits = 15;
        while (maxbits > 0 && count[maxbits] == 0) maxbits--;
        empty = maxbits == 0;
        char what[100];
        if (empty) {
            if (!none_ok) {
                snprintf(what, sizeof what, "the %s code set has no code at all", kind);
                r.fail(what);
            }
            tab.assign(1, 0);
            return;
        }
        uint64_t used = 0; /* in units of 2^-15 of the code space */
        for (uint32_t b = 1; b <= 15; b++) used += (uint64_t)count[b] << (15 - b);
        if (used > (1u << 15)) {
            snprintf(what, sizeof what, "the %s code set is over-subscribed", kind);
            r.fail(what);
        }
        if (used < (1u << 15) && !(one_bit_ok && maxbits == 1 && count[1] == 1)) {
            snprintf(what, sizeof what, "the %s code set is incomplete", kind);
            r.fail(what);
        }
        uint32_t next[16] = {0}, code = 0;
        for (uint32_t b = 1; b <= 15; b++) {
            code = (code + count[b - 1]) << 1;
            next[b] = code;
        }
        tab.assign((size_t)1 << maxbits, 0);
        for (uint32_t s = 0; s < n; s++) {
            const uint32_t b = len[s];
            if (!b) continue;
            const uint32_t c = next[b]++;
            uint32_t rev = 0; /* Huffman codes are packed starting with their most significant bit (3.1.1) */
            for (uint32_t k = 0; k < b; k++) rev |= ((c >> k) & 1u) << (b - 1 - k);
            for (uint32_t i = rev; i < tab.size(); i += 1u << b) tab[i] = s | (b << 16);
        }
    }
    uint32_t decode(Reader &r, const char *unassigned) const {
        if (empty) r.fail(unassigned);
        const uint32_t e = tab[r.peek(maxbits)];
        if (!e) r.fail(unassigned);
        r.skip(e >> 16);
        return e & 0xFFFFu;
    }
};

void put(Walk &w, bool keep, uint8_t b) {
    if (keep) w.bytes.push_back(b);
    w.out++;
}

void huffman_block(Reader &r, Walk &w, const Code &lit, const Code &dist, uint64_t history, const uint8_t *prefix, bool keep) {
    for (;;) {
        const uint32_t s = lit.decode(r, "a literal/length code that no symbol has");
        if (s < 256) {
            put(w, keep, (uint8_t)s);
            continue;
        }
        if (s == 256) return;
        if (s > 285) r.fail("length symbol 286 or 287, which does not exist");
        const uint32_t length = LEN_BASE[s - 257] + r.take(LEN_EXTRA[s - 257]);
        const uint32_t d = dist.decode(r, "a distance code that no symbol has");
        if (d > 29) r.fail("distance symbol 30 or 31, which does not exist");
        const uint32_t distance = DIST_BASE[d] + r.take(DIST_EXTRA[d]);
        if (distance > w.out + history) r.fail("a distance that reaches in front of the first byte");
        w.matches.push_back(Match{(int64_t)w.out, (int64_t)length, (int64_t)distance});
        if (keep) {
            for (uint32_t k = 0; k < length; k++) {
                const uint64_t at = w.out; /* the byte `distance` in front of it: in the output, or in the history in front of that */
                const uint8_t b = distance <= at ? w.bytes[at - distance] : prefix[history - (distance - at)];
                put(w, true, b);
            }
        } else {
            w.out += length;
        }
    }
}

void walk(Reader &r, Walk &w, uint64_t history, const uint8_t *prefix, bool keep, bool open_end) {
    uint8_t len[320];
    Code fixed_lit, fixed_dist, lit, dist, cl;
    bool have_fixed = false;
    for (;;) {
        if (open_end && r.pos == r.nbits && (r.pos & 7) == 0) break; /* a piece that is not the stream's last ends between blocks */
        Block b;
        b.first_bit = r.pos;
        b.out_start = w.out;
        b.bfinal = r.take(1);
        b.btype = r.take(2);
        if (b.btype == 3) r.fail("block type 3 (reserved)");
        if (b.btype == 0) {
            r.skip((uint32_t)((8 - (r.pos & 7)) & 7));
            const uint32_t n = r.take(16), nn = r.take(16);
            if ((n ^ 0xFFFFu) != nn) r.fail("a stored block whose NLEN is not the complement of LEN");
            if (r.pos + 8ull * n > r.nbits) r.fail("the input ends before the final block does");
            for (uint32_t k = 0; k < n; k++) put(w, keep, r.z[(r.pos >> 3) + k]);
            r.pos += 8ull * n;
        } else if (b.btype == 1) {
            if (!have_fixed) {
                for (uint32_t s = 0; s < 288; s++) len[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; /* 3.2.6 */
                fixed_lit.build(r, len, 288, "fixed literal/length", false, false);
                for (uint32_t s = 0; s < 32; s++) len[s] = 5;
                fixed_dist.build(r, len, 32, "fixed distance", false, false);
                have_fixed = true;
            }
            huffman_block(r, w, fixed_lit, fixed_dist, history, prefix, keep);
        } else {
            const uint32_t nlit = 257 + r.take(5), ndist = 1 + r.take(5), ncl = 4 + r.take(4);
            if (nlit > 286) r.fail("a dynamic header with more than 286 literal/length codes");
            if (ndist > 30) r.fail("a dynamic header with more than 30 distance codes");
            memset(len, 0, 19);
            for (uint32_t i = 0; i < ncl; i++) len[CL_ORDER[i]] = (uint8_t)r.take(3);
            cl.build(r, len, 19, "code-length", false, false);
            uint32_t i = 0;
            while (i < nlit + ndist) {
                const uint32_t s = cl.decode(r, "a code-length code that no symbol has");
                if (s < 16) {
                    len[i++] = (uint8_t)s;
                    continue;
                }
                uint32_t rep, v = 0;
                if (s == 16) {
                    if (i == 0) r.fail("a repeat of the previous code length in front of the first");
                    v = len[i - 1];
                    rep = 3 + r.take(2);
                } else if (s == 17) {
                    rep = 3 + r.take(3);
                } else {
                    rep = 11 + r.take(7);
                }
                if (i + rep > nlit + ndist) r.fail("a run of code lengths that goes beyond HLIT + HDIST");
                while (rep--) len[i++] = (uint8_t)v;
            }
            if (len[256] == 0) r.fail("a dynamic block without a code for end-of-block");
            lit.build(r, len, nlit, "literal/length", false, false);
            dist.build(r, len + nlit, ndist, "distance", true, true);
            huffman_block(r, w, lit, dist, history, prefix, keep);
        }
        b.end_bit = r.pos;
        b.out_end = w.out;
        w.blocks.push_back(b);
        if (b.bfinal) break;
    }
    w.bits = r.pos;
}

}  // namespace

extern "C" {

// keep: reconstruct the bytes (prefix = the `history` bytes in front of the stream, needed when history != 0).  open_end: the
// stream may stop at a byte-aligned block boundary without a final block (a piece of a longer stream).
void *dt_walk(const uint8_t *z, uint64_t n, uint64_t history, const uint8_t *prefix, int keep, int open_end) {
    Walk *w = new Walk();
    Reader r{z, 8ull * n, 0, w};
    try {
        walk(r, *w, history, prefix, keep != 0, open_end != 0);
    } catch (const Fail &) {
    }
    return w;
}

int dt_error(void *h, char *msg, uint64_t cap) {
    const Walk *w = (const Walk *)h;
    if (cap) snprintf(msg, (size_t)cap, "%s", w->msg);
    return w->err;
}

void dt_counts(void *h, uint64_t *c) {
    const Walk *w = (const Walk *)h;
    c[0] = w->blocks.size();
    c[1] = w->matches.size();
    c[2] = w->bytes.size();
    c[3] = w->bits;
    c[4] = w->out;
}

void dt_fetch(void *h, uint64_t *blocks, int64_t *matches, uint8_t *bytes) {
    const Walk *w = (const Walk *)h;
    if (!w->blocks.empty()) memcpy(blocks, w->blocks.data(), w->blocks.size() * sizeof(Block));
    if (!w->matches.empty()) memcpy(matches, w->matches.data(), w->matches.size() * sizeof(Match));
    if (!w->bytes.empty()) memcpy(bytes, w->bytes.data(), w->bytes.size());
}

void dt_free(void *h) { delete (Walk *)h; }
}
