// lzma_tokens.cpp -- a reader of LZMA1 and LZMA2 that reports what a stream is MADE of: its packets (output position, kind,
// length, distance), the bytes they stand for, the input they take and how the range coder ends.  Written from the LZMA
// specification (7-Zip's lzma-specification.txt: the range decoder with its normalisation behind every bit, the 12 states,
// the literal coder with its matched half, the two length coders, the distance slots with their reverse trees and aligned
// bits, the end marker) and from "The .xz File Format" 1.0.4 section 5.3.1 and liblzma's documented LZMA2 rules for the
// chunk headers (control byte, sizes, properties, what each control value resets).  It shares no code and no tables with
// lzma_core.h, lzma_enc_core.h, oracle/ or tests/lzma_packets.py: tests/lzma_tokens.py compiles it on first use and the
// encoder tests measure K6's promises (reach, seams, framing) with it.  Everything the format forbids is an error that
// names the rule, the input byte, the output byte and the packet it was seen at.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

enum Kind { LITERALS = 0, MATCH = 1, REP0 = 2, REP1 = 3, REP2 = 4, REP3 = 5, SHORTREP = 6, EOS = 7 };

struct Packet {
    int64_t out_pos, kind, length, distance; /* literal run: length = its count, distance 0; eos: distance 2^32 */
};
struct Chunk {
    int64_t control, usize, csize, props, stored, first_packet, npackets, out_start, in_start, code;
};

struct Walk {
    std::vector<Packet> packets;
    std::vector<int8_t> rep_hit; /* per packet: a MATCH whose distance is rep k of that moment -> k, else -1 */
    std::vector<Chunk> chunks;
    std::vector<uint8_t> bytes; /* [prefix | what the stream stands for] */
    uint64_t prefix = 0, used = 0, eos = 0, code = 0, end_byte = 0;
    int err = 0;
    char msg[240] = {0};
};

struct Fail {};

const uint32_t TOP = 1u << 24;
const uint16_t HALF = 1024; /* every probability starts at 1/2 of 2^11 */

struct LenCoder {
    uint16_t choice, choice2, low[16][8], mid[16][8], high[256];
    void reset() {
        choice = choice2 = HALF;
        for (auto &r : low)
            for (auto &p : r) p = HALF;
        for (auto &r : mid)
            for (auto &p : r) p = HALF;
        for (auto &p : high) p = HALF;
    }
};

struct Decoder {
    Walk *w;
    const uint8_t *z;
    uint64_t zend = 0, ip = 0; /* input: the coder may read z[ip .. zend) */
    uint32_t range = 0, code = 0;
    /* properties and model */
    uint32_t lc = 0, lp = 0, pb = 0;
    uint16_t is_match[12][16], is_rep[12], is_rep_g0[12], is_rep_g1[12], is_rep_g2[12], is_rep0_long[12][16];
    uint16_t pos_slot[4][64], pos_special[115], pos_align[16];
    LenCoder len_match, len_rep;
    std::vector<uint16_t> literal;
    uint32_t state = 0, rep[4] = {0, 0, 0, 0};
    /* dictionary: bytes[dict_start ..) of the output; positions (pos_state, literal position bits) count from pos_base */
    uint64_t dict_start = 0, pos_base = 0, dict_limit = 0;
    bool run_open = false; /* the last packet is a literal run that the next literal extends */

    [[noreturn]] void fail(const char *what) {
        w->err = 1;
        snprintf(w->msg, sizeof w->msg, "%s (input byte %llu, output byte %llu, packet %llu)", what, (unsigned long long)ip,
                 (unsigned long long)(w->bytes.size() - w->prefix), (unsigned long long)w->packets.size());
        throw Fail();
    }
    void set_props(uint32_t lc_, uint32_t lp_, uint32_t pb_) {
        lc = lc_;
        lp = lp_;
        pb = pb_;
        literal.assign((size_t)0x300 << (lc + lp), HALF);
    }
    void reset_state() {
        for (auto &r : is_match)
            for (auto &p : r) p = HALF;
        for (auto &r : is_rep0_long)
            for (auto &p : r) p = HALF;
        for (int s = 0; s < 12; s++) is_rep[s] = is_rep_g0[s] = is_rep_g1[s] = is_rep_g2[s] = HALF;
        for (auto &r : pos_slot)
            for (auto &p : r) p = HALF;
        for (auto &p : pos_special) p = HALF;
        for (auto &p : pos_align) p = HALF;
        len_match.reset();
        len_rep.reset();
        literal.assign(literal.size(), HALF);
        state = 0;
        rep[0] = rep[1] = rep[2] = rep[3] = 0;
    }

    /* ---- range decoder: five bytes to start with, the first of them zero; a byte more whenever range drops below 2^24 */
    uint8_t next_byte() {
        if (ip >= zend) fail("the input ends inside the range coder's data");
        return z[ip++];
    }
    void rc_init() {
        if (next_byte() != 0) fail("the coder's first byte is not zero");
        code = 0;
        for (int i = 0; i < 4; i++) code = (code << 8) | next_byte();
        range = 0xFFFFFFFFu;
    }
    void normalize() {
        if (range < TOP) {
            range <<= 8;
            code = (code << 8) | next_byte();
        }
    }
    uint32_t bit(uint16_t &p) {
        const uint32_t bound = (range >> 11) * p;
        uint32_t b;
        if (code < bound) {
            range = bound;
            p = (uint16_t)(p + ((2048 - p) >> 5));
            b = 0;
        } else {
            code -= bound;
            range -= bound;
            p = (uint16_t)(p - (p >> 5));
            b = 1;
        }
        normalize();
        return b;
    }
    uint32_t direct(uint32_t n) {
        uint32_t v = 0;
        while (n--) {
            range >>= 1;
            uint32_t b = 0;
            if (code >= range) {
                code -= range;
                b = 1;
            }
            normalize();
            v = (v << 1) | b;
        }
        return v;
    }
    uint32_t tree(uint16_t *p, uint32_t nbits) { /* most significant bit first */
        uint32_t m = 1;
        for (uint32_t i = 0; i < nbits; i++) m = (m << 1) | bit(p[m]);
        return m - (1u << nbits);
    }
    uint32_t tree_reverse(uint16_t *p, uint32_t nbits) { /* least significant bit first */
        uint32_t m = 1, v = 0;
        for (uint32_t i = 0; i < nbits; i++) {
            const uint32_t b = bit(p[m]);
            m = (m << 1) | b;
            v |= b << i;
        }
        return v;
    }
    uint32_t length(LenCoder &c, uint32_t ps) { /* -> length - 2 */
        if (!bit(c.choice)) return tree(c.low[ps], 3);
        if (!bit(c.choice2)) return 8 + tree(c.mid[ps], 3);
        return 16 + tree(c.high, 8);
    }
    uint32_t distance(uint32_t len_m2) { /* -> distance - 1 */
        const uint32_t slot = tree(pos_slot[len_m2 < 3 ? len_m2 : 3], 6);
        if (slot < 4) return slot;
        const uint32_t nb = (slot >> 1) - 1;
        uint32_t d = (2 | (slot & 1)) << nb;
        if (slot < 14) {
            d += tree_reverse(pos_special + d - slot, nb);
        } else {
            d += direct(nb - 4) << 4;
            d += tree_reverse(pos_align, 4);
        }
        return d;
    }

    /* ---- the dictionary ------------------------------------------------------------------------------------------- */
    uint64_t have() const { return w->bytes.size() - dict_start; }
    uint8_t back(uint64_t d) const { return w->bytes[w->bytes.size() - d - 1]; } /* d = distance - 1 < have() */
    void emit(int64_t kind, int64_t n, int64_t dist, int hit) {
        const int64_t at = (int64_t)(w->bytes.size() - w->prefix);
        if (kind == LITERALS && run_open) {
            w->packets.back().length++;
            return;
        }
        w->packets.push_back(Packet{at, kind, n, dist});
        w->rep_hit.push_back((int8_t)hit);
        run_open = kind == LITERALS;
    }
    void copy(uint64_t d, uint32_t n) {
        size_t from = w->bytes.size() - d - 1;
        for (uint32_t i = 0; i < n; i++) w->bytes.push_back(w->bytes[from++]); /* (a copy may read what it wrote) */
    }

    /* One packet.  room: bytes the stream may still produce (UINT64_MAX = as many as it likes); eos_ok: an end marker is legal
     * here.  -> false when the end marker was read. */
    bool packet(uint64_t room, bool eos_ok) {
        const uint64_t pos = w->bytes.size() - pos_base;
        const uint32_t ps = (uint32_t)(pos & ((1u << pb) - 1));
        if (!bit(is_match[state][ps])) {
            if (room == 0) fail("a literal beyond the size the stream states");
            const uint32_t prev = have() ? back(0) : 0;
            uint16_t *p = &literal[(size_t)0x300 * (((pos & ((1u << lp) - 1)) << lc) + (prev >> (8 - lc)))];
            uint32_t sym = 1;
            if (state >= 7) {
                uint32_t mb = rep[0] < have() ? back(rep[0]) : 0;
                do {
                    const uint32_t mbit = (mb >> 7) & 1;
                    mb <<= 1;
                    const uint32_t b = bit(p[((1 + mbit) << 8) + sym]);
                    sym = (sym << 1) | b;
                    if (mbit != b) break;
                } while (sym < 0x100);
            }
            while (sym < 0x100) sym = (sym << 1) | bit(p[sym]);
            emit(LITERALS, 1, 0, -1);
            w->bytes.push_back((uint8_t)sym);
            state = state < 4 ? 0 : (state < 10 ? state - 3 : state - 6);
            return true;
        }
        uint32_t n;
        int64_t kind;
        int hit = -1;
        if (bit(is_rep[state])) {
            if (have() == 0) fail("a rep before any byte is in the dictionary");
            if (!bit(is_rep_g0[state])) {
                if (!bit(is_rep0_long[state][ps])) {
                    if (room == 0) fail("a short rep beyond the size the stream states");
                    if (rep[0] >= have() || rep[0] >= dict_limit) fail("a short rep whose distance lies beyond the dictionary");
                    emit(SHORTREP, 1, (int64_t)rep[0] + 1, -1);
                    copy(rep[0], 1);
                    state = state < 7 ? 9 : 11;
                    return true;
                }
                kind = REP0;
            } else {
                uint32_t d;
                if (!bit(is_rep_g1[state])) {
                    d = rep[1];
                    kind = REP1;
                } else {
                    if (!bit(is_rep_g2[state])) {
                        d = rep[2];
                        kind = REP2;
                    } else {
                        d = rep[3];
                        rep[3] = rep[2];
                        kind = REP3;
                    }
                    rep[2] = rep[1];
                }
                rep[1] = rep[0];
                rep[0] = d;
            }
            n = length(len_rep, ps) + 2;
            state = state < 7 ? 8 : 11;
        } else {
            n = length(len_match, ps) + 2;
            const uint32_t d = distance(n - 2);
            if (d == 0xFFFFFFFFu) {
                if (!eos_ok) fail("an end marker where the format has none (inside an LZMA2 chunk)");
                emit(EOS, n, (int64_t)1 << 32, -1);
                return false;
            }
            for (int k = 0; k < 4; k++)
                if (hit < 0 && rep[k] == d && have()) hit = k;
            rep[3] = rep[2];
            rep[2] = rep[1];
            rep[1] = rep[0];
            rep[0] = d;
            state = state < 7 ? 7 : 10;
            kind = MATCH;
        }
        if (n > 273) fail("a length above 273");
        if (rep[0] >= have()) fail("a distance beyond the output so far");
        if (rep[0] >= dict_limit) fail("a distance beyond the dictionary");
        if (n > room) fail("a copy that runs beyond the size the stream states");
        emit(kind, n, (int64_t)rep[0] + 1, hit);
        copy(rep[0], n);
        return true;
    }
};

/* LZMA1: z[start ..) is the range coder's data under the given properties; usize < 0: the stream ends with its end marker */
void walk_lzma(Walk *w, const uint8_t *z, uint64_t n, uint64_t start, int lc, int lp, int pb, uint64_t dict_limit, int64_t usize) {
    Decoder *d = new Decoder();
    try {
        d->w = w;
        d->z = z;
        d->zend = n;
        d->ip = start < n ? start : n;
        if (lc < 0 || lc > 8 || lp < 0 || lp > 4 || pb < 0 || pb > 4) d->fail("properties out of range (lc <= 8, lp <= 4, pb <= 4)");
        d->set_props((uint32_t)lc, (uint32_t)lp, (uint32_t)pb);
        d->reset_state();
        d->dict_limit = dict_limit;
        d->dict_start = 0; /* the prefix is dictionary */
        d->pos_base = w->prefix;
        d->rc_init();
        uint64_t made = 0;
        for (;;) {
            if (usize >= 0 && made == (uint64_t)usize) break;
            const uint64_t before = w->bytes.size();
            if (!d->packet(usize >= 0 ? (uint64_t)usize - made : UINT64_MAX, true)) {
                w->eos = 1;
                break;
            }
            made += w->bytes.size() - before;
        }
        w->used = d->ip - start;
        w->code = d->code;
    } catch (Fail &) {
    }
    delete d;
}

/* LZMA2: a chunk sequence up to and with its end byte 0x00 */
void walk_lzma2(Walk *w, const uint8_t *z, uint64_t n, uint64_t start, uint64_t dict_limit) {
    Decoder *d = new Decoder();
    try {
        d->w = w;
        d->z = z;
        d->zend = n;
        d->ip = start < n ? start : n;
        d->dict_limit = dict_limit;
        d->set_props(0, 0, 0);
        d->reset_state();
        bool need_dict = true, need_props = true;
        for (;;) {
            d->zend = n;
            const uint32_t ctl = d->next_byte();
            if (ctl == 0) {
                w->end_byte = 1;
                break;
            }
            Chunk c;
            memset(&c, 0, sizeof c);
            c.control = ctl;
            c.props = -1;
            c.first_packet = (int64_t)w->packets.size();
            c.out_start = (int64_t)(w->bytes.size() - w->prefix);
            if (ctl >= 0xE0 || ctl == 1) {
                need_props = true; /* (an LZMA chunk of control 0xE0 brings them itself) */
                need_dict = false;
                d->dict_start = d->pos_base = w->bytes.size();
            } else if (need_dict) {
                d->fail("a chunk in front of the first dictionary reset");
            }
            if (ctl < 0x80) {
                if (ctl > 2) d->fail("a control byte that is neither an end, a stored chunk nor an LZMA chunk");
                uint32_t us = d->next_byte() << 8;
                us = (us | d->next_byte()) + 1;
                if (n - d->ip < us) d->fail("the input ends inside a stored chunk");
                c.usize = c.csize = us;
                c.stored = 1;
                c.in_start = (int64_t)d->ip;
                d->run_open = false;
                w->bytes.insert(w->bytes.end(), z + d->ip, z + d->ip + us);
                d->ip += us;
                w->chunks.push_back(c);
                continue;
            }
            uint32_t us = (ctl & 0x1F) << 16;
            us |= d->next_byte() << 8;
            us = (us | d->next_byte()) + 1;
            uint32_t cs = d->next_byte() << 8;
            cs = (cs | d->next_byte()) + 1;
            if (ctl >= 0xC0) {
                const uint32_t pbyte = d->next_byte();
                if (pbyte > 224) d->fail("a properties byte above 224");
                const uint32_t lc = pbyte % 9, lp = pbyte / 9 % 5, pb = pbyte / 45;
                if (lc + lp > 4) d->fail("properties with lc + lp > 4 in LZMA2");
                d->set_props(lc, lp, pb);
                c.props = pbyte;
                need_props = false;
            } else if (need_props) {
                d->fail("an LZMA chunk without properties behind a dictionary reset");
            }
            if (ctl >= 0xA0) d->reset_state();
            if (n - d->ip < cs) d->fail("the input ends inside an LZMA chunk");
            c.usize = us;
            c.csize = cs;
            c.in_start = (int64_t)d->ip;
            d->zend = d->ip + cs;
            d->run_open = false;
            d->rc_init();
            uint64_t made = 0;
            while (made < us) {
                const uint64_t before = w->bytes.size();
                d->packet(us - made, false);
                made += w->bytes.size() - before;
            }
            c.code = d->code;
            if (d->code != 0) d->fail("the range coder does not end on code 0 at the chunk's end");
            if (d->ip != d->zend) d->fail("the chunk's compressed size is not what its coder reads");
            c.npackets = (int64_t)w->packets.size() - c.first_packet;
            w->chunks.push_back(c);
        }
        w->used = d->ip - start;
    } catch (Fail &) {
    }
    delete d;
}

} // namespace

extern "C" {

void *lt_lzma(const uint8_t *z, uint64_t n, uint64_t start, int lc, int lp, int pb, uint64_t dict_limit, int64_t usize, const uint8_t *prefix,
              uint64_t prefix_len) {
    Walk *w = new Walk();
    if (prefix_len) w->bytes.assign(prefix, prefix + prefix_len);
    w->prefix = prefix_len;
    walk_lzma(w, z, n, start, lc, lp, pb, dict_limit, usize);
    return w;
}
void *lt_lzma2(const uint8_t *z, uint64_t n, uint64_t start, uint64_t dict_limit) {
    Walk *w = new Walk();
    walk_lzma2(w, z, n, start, dict_limit);
    return w;
}
int lt_error(void *h, char *buf, uint64_t n) {
    Walk *w = (Walk *)h;
    if (w->err && n) snprintf(buf, n, "%s", w->msg);
    return w->err;
}
/* c[0..7] = packets, bytes (without the prefix), input bytes used, end marker read, the coder's last code, chunks, LZMA2 end
 * byte read, 0 */
void lt_counts(void *h, uint64_t *c) {
    Walk *w = (Walk *)h;
    c[0] = w->packets.size();
    c[1] = w->bytes.size() - w->prefix;
    c[2] = w->used;
    c[3] = w->eos;
    c[4] = w->code;
    c[5] = w->chunks.size();
    c[6] = w->end_byte;
    c[7] = 0;
}
void lt_fetch(void *h, int64_t *packets, int8_t *rep_hit, uint8_t *bytes, int64_t *chunks) {
    Walk *w = (Walk *)h;
    if (!w->packets.empty()) {
        memcpy(packets, w->packets.data(), w->packets.size() * sizeof(Packet));
        memcpy(rep_hit, w->rep_hit.data(), w->rep_hit.size());
    }
    if (w->bytes.size() > w->prefix) memcpy(bytes, w->bytes.data() + w->prefix, w->bytes.size() - w->prefix);
    if (!w->chunks.empty()) memcpy(chunks, w->chunks.data(), w->chunks.size() * sizeof(Chunk));
}
void lt_free(void *h) { delete (Walk *)h; }
}
