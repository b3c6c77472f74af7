/* inflate_walk.inc -- the two walks of K1's chase window (inflate_chase.inc has the whole window; this is its first half):
 *   pass 1   every lane walks its own span of the compressed stream and records every step,
 *   pass 2   every lane that crossed into the next span keeps walking until it stands on a step start the lane there
 *            recorded too ("chase").
 * A function of its own, not inlined into mz_inflate_entry(): that function keeps ~230 values alive across a window (cursor,
 * CRC state, block and resume state, pointers) and its register allocation reloaded spilled ones inside these loops.  Here
 * only the walk's own state is alive.  Replaces, per window, what zlib's inflate_fast() does token by token behind
 * mz_stream_zlib_read (mz_strm_zlib.c:116-193). */
#if defined(MZ_PROF) && !defined(MZHIP_HOST_EMUL)
#define MZ_PROF_PARAMS , uint32_t &prof_acc, uint64_t &prof_t0
#define MZ_PROF_ARGS , prof_acc, prof_t0
#else
#define MZ_PROF_PARAMS
#define MZ_PROF_ARGS
#endif
/* what the walks leave behind, per lane (returned in registers) */
typedef struct mz_walk_result {
    PV(uint32_t, u);   /* where the lane's cursor ended up (after its chase) */
    PV(uint32_t, sn);  /* own walk: steps recorded, */
    PV(uint32_t, sfl); /* how it ended: 0 crossed into the next span, 1 end-of-block, 2 invalid code, 3 record cap, */
    PV(uint32_t, sxe); /* and where */
    PV(uint32_t, cm);  /* chase steps recorded */
    PV(uint32_t, cfl); /* how the chase ended: 0 met a lane's walk, 1 end-of-block, 2 invalid code, 3 record cap, 4 left the window */
    PV(uint32_t, csx); /* the lane it met ... */
    PV(uint32_t, cst); /* ... at the start of this step of that lane's walk */
} mz_walk_result;
MZ_DEV_NOINLINE mz_walk_result mz_chase_walk(mz_lds_handle L_, mz_glb_handle in_al_, uint32_t in_mis_, uint32_t in_len_, uint32_t Wu_,
                                             uint32_t Eu_, uint32_t S_, uint32_t nact_, mz_lds_handle tab_walk_, mz_glb_handle rec_, PVIN(uint32_t, ev) MZ_PROF_PARAMS) {
    MZ_LANE_DECL
    MZ_PRIO_AT(14); /* (measurement builds: pass 1 starts) */
    /* wave-uniform arguments, back in scalar registers (wave.h, MZ_UNIFORM64) */
    const uint32_t in_mis = MZ_UNIFORM(in_mis_), in_len = MZ_UNIFORM(in_len_), Wu = MZ_UNIFORM(Wu_), Eu = MZ_UNIFORM(Eu_), S = MZ_UNIFORM(S_),
                   nact = MZ_UNIFORM(nact_);
    mz_inflate_lds *const L = MZ_LDS_FROM(mz_inflate_lds, L_);
    uint32_t *const tab_walk = MZ_LDS_FROM(uint32_t, tab_walk_);
    const uint8_t *const in_al = MZ_GLB_FROM(const uint8_t, in_al_);
    uint8_t *const rec = MZ_GLB_FROM(uint8_t, rec_);
    PV(uint32_t, u);
    PV(uint32_t, sn);
    PV(uint32_t, sfl);
    PV(uint32_t, sxe);
    PV(uint32_t, cm);
    PV(uint32_t, cfl);
    PV(uint32_t, csx);
    PV(uint32_t, cst);
    uint32_t *const ring = MZ_L_WIN(L);
    uint8_t *const Rp = rec;                                   /* own walks:  quad q (steps 4q .. 4q + 3) of lane l at Rp + MZ_REC_ADDR(q, l) */
    uint8_t *const Cp = rec + MZ_REC_AREA(MZ_REC_CAP1);        /* chases:     the same */
    uint8_t *const Lp = Cp + MZ_REC_AREA(MZ_REC_CAP2);         /* K bytes of the own walks: step t of lane l at Lp + l * MZ_REC_CAP1 + t */
    uint8_t *const Lc = Lp + 64u * MZ_REC_CAP1;                /* ... and of the chases: Lc + l * MZ_REC_CAP2 + t */
    const uint32_t dw_lo = in_mis ? 1u : 0u, dw_hi = (in_mis + in_len) >> 2; /* dwords [dw_lo, dw_hi) lie entirely inside the input */
    /* Aligned groups of four stream dwords (the ring is filled and topped up in such groups).  A group that lies entirely
     * inside the input is one 16-byte load.  Only three kinds do not: the group of dword 0 when in[] does not start on a
     * dword boundary, the group that holds the last (partial) dword, and everything behind it (zeros).  The first two are
     * eight wave-uniform values (`ev`, lanes 0 .. 7: MZ_EDGE_GROUPS of mz_inflate_entry loads them once per view; scalar
     * registers here), masked as mz_load_stream_dword masks them.  MZ_CHASE_LOAD_DW4, the initial fill of a ring in front
     * of the loops, is ONE global load for every lane -- from a harmless interior address where the group is an edge --
     * and eight selects; the refills inside the two loops go through MZ_CHASE_RELOAD_DW4 below, a plain load with the
     * edges in a branch.  (The r3 refill
     * carried four masked loads with 64-bit address arithmetic, ~100 instructions and a dozen registers, through both walk
     * loops; a copy of the edge groups in LDS turns the load into a flat one -- a select between a global and an LDS
     * pointer -- and a copy in global scratch costs every window a store, a fence and a round trip before its first load:
     * 4 % on 8 KiB entries, profiles/r4/ab_k1_records.log.) */
    const uint32_t gl4 = dw_hi & ~3u; /* first dword of the group with the input's last dword */
    uint32_t e0[4], el[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) { /* (loaded once per view by mz_inflate_entry: MZ_EDGE_GROUPS) */
        e0[k] = MZ_READLANE(ev, k);
        el[k] = MZ_READLANE(ev, 4u + k);
    }
#define MZ_CHASE_LOAD_DW4(dst, o_, d_)                                                       \
    {                                                                                        \
        const uint32_t dd_ = (d_); /* a multiple of 4 */                                     \
        mz_dw4 v_;                                                                           \
        const uint32_t int_ = (dd_ >= dw_lo && dd_ + 4u <= dw_hi) ? 1u : 0u;                 \
        __builtin_memcpy(&v_, in_al + ((int_ ? dd_ : 4u) << 2), 16); /* (dwords 4 .. 7 are input: a window has 40 bytes in front of it) */ \
        const uint32_t z_ = (dd_ == 0u) ? 1u : 0u, l_ = (dd_ == gl4) ? 1u : 0u;              \
        P(dst)[(o_) + 0] = int_ ? v_.v[0] : z_ ? e0[0] : l_ ? el[0] : 0u;                    \
        P(dst)[(o_) + 1] = int_ ? v_.v[1] : z_ ? e0[1] : l_ ? el[1] : 0u;                    \
        P(dst)[(o_) + 2] = int_ ? v_.v[2] : z_ ? e0[2] : l_ ? el[2] : 0u;                    \
        P(dst)[(o_) + 3] = int_ ? v_.v[3] : z_ ? e0[3] : l_ ? el[3] : 0u;                    \
    }
    /* The same for the refills inside the two walk loops, without the selects.  A lane whose group lies inside the input
     * does its one 16-byte load and nothing else; a lane whose group does not loads nothing -- no byte outside the aligned
     * dwords of [in, in + in_len) is touched, and none from a stand-in address either -- and takes its values from `el` or
     * zeros in a branch of its own, which the wave jumps over when no lane is there.
     *   The group of dword 0 cannot occur here: a lane starts with hi = (first dword & ~3) + MZ_CRING_DW >= 16, hi only
     * grows, and a refill loads the groups at hi and hi + 4 >= 16.  So every d_ is above dw_lo (which is 0 or 1), `e0` is
     * never looked at, and "inside the input" is d_ + 4 <= dw_hi alone.  What is left of the edges: d_ == gl4, the
     * group with the last (partial) dword, already masked in `el`; and d_ > gl4, zeros.  (gl4 + 4 > dw_hi always, so the
     * three cases do not overlap.)
     * (Selects instead of the branch, MZ_CHASE_LOAD_DW4 in the refills too: ~50 of a check's ~70 vector instructions in
     * every wave at every check, the branch alone measured +5.4 % on 64 KiB entries: profiles/r9, DESIGN.md section 3 K1) */
#define MZ_CHASE_RELOAD_DW4(dst, o_, d_)                                                     \
    {                                                                                        \
        const uint32_t dd_ = (d_); /* a multiple of 4, >= MZ_CRING_DW */                     \
        if (dd_ + 4u <= dw_hi) {                                                             \
            mz_dw4 v_;                                                                       \
            __builtin_memcpy(&v_, in_al + (dd_ << 2), 16);                                   \
            P(dst)[(o_) + 0] = v_.v[0];                                                      \
            P(dst)[(o_) + 1] = v_.v[1];                                                      \
            P(dst)[(o_) + 2] = v_.v[2];                                                      \
            P(dst)[(o_) + 3] = v_.v[3];                                                      \
        } else {                                                                             \
            const uint32_t l_ = (dd_ == gl4) ? 1u : 0u;                                      \
            P(dst)[(o_) + 0] = l_ ? el[0] : 0u;                                              \
            P(dst)[(o_) + 1] = l_ ? el[1] : 0u;                                              \
            P(dst)[(o_) + 2] = l_ ? el[2] : 0u;                                              \
            P(dst)[(o_) + 3] = l_ ? el[3] : 0u;                                              \
        }                                                                                    \
    }

    PV(uint32_t, lim); /* where its span ends */
    PV(uint32_t, hi);  /* next stream dword the ring takes ... */
    PV(uint32_t, hs);  /* ... and the slot it goes to (0, 4, 8, 12) */
    /* The stream reaches a lane 16 bytes at a time, and 64 lanes stand in 64 different cache lines: a line was fetched eight
     * times over its sixteen steps, almost always from the fabric (the streams of the waves of an XCD do not fit its L2 --
     * round 5: refills + records were 46 % of K1's fabric reads).  So the NEXT TWO groups are loaded together, two 16-byte
     * loads of one instruction pair into the same line: half the line fetches.
     * (One group per load: 3.7 % more bytes read for the same time, profiles/r6/ab_k1_pf.log, DESIGN.md section 3 K1) */
    PV2(uint32_t, pf, 8); /* dwords hi .. hi + 3 and hi + 4 .. hi + 7, loaded at an earlier check */
    PV(uint32_t, ph);     /* 1: the first group has gone to the ring, pf[0 .. 3] holds the second */
    PV(uint32_t, run);
    PV2(uint32_t, rb, 4); /* the records of the current trip's four steps */
    PV(uint32_t *, row);
    MZ_LANES {
        P(row) = ring + (uint32_t)lane * MZ_CRING_RS;
        P(u) = Wu + (uint32_t)lane * S;
        P(lim) = P(u) + S;
        P(run) = ((uint32_t)lane < nact) ? 1u : 0u;
        P(sn) = 0u;
        P(sfl) = 0u; /* (while the walk runs: the last step's K byte, 0 = no valid step) */
        P(sxe) = P(u);
        P(hs) = (P(u) >> 5) & (MZ_CRING_DW - 1u) & ~3u; /* stream dword d lives in slot d & 15: the first refill goes where the span's first four dwords are */
        P(hi) = ((P(u) >> 5) & ~3u) + MZ_CRING_DW;
        P(pf)[0] = P(pf)[1] = P(pf)[2] = P(pf)[3] = 0u;
        P(pf)[4] = P(pf)[5] = P(pf)[6] = P(pf)[7] = 0u;
        P(ph) = 0u;
        P(rb)[0] = P(rb)[1] = P(rb)[2] = P(rb)[3] = 0u;
        if (P(run)) {
            const uint32_t a0 = (P(u) >> 5) & ~3u; /* the ring is filled and topped up in aligned groups of four dwords */
#pragma unroll
            for (uint32_t g = 0; g < MZ_CRING_DW / 4u; g++) {
                PV2(uint32_t, d, 4);
                MZ_CHASE_LOAD_DW4(d, 0, a0 + 4u * g)
                const uint32_t sl = (a0 + 4u * g) & (MZ_CRING_DW - 1u);
                P(row)[sl] = P(d)[0];
                P(row)[sl + 1u] = P(d)[1];
                P(row)[sl + 2u] = P(d)[2];
                P(row)[sl + 3u] = P(d)[3];
                if (sl == 0u) {
                    P(row)[MZ_CRING_DW] = P(d)[0];
                    P(row)[MZ_CRING_DW + 1u] = P(d)[1];
                }
            }
            MZ_CHASE_LOAD_DW4(pf, 0, P(hi))
            MZ_CHASE_LOAD_DW4(pf, 4, P(hi) + 4u)
        }
    }
    MZ_WAVE_SYNC();

    /* ONE refill check per trip of four steps (MZ_CRING_DW is 16).  Write c = u >> 5 for the dword the cursor stands in
     * and gap = hi - c for the dwords of the ring from there on (the ring holds dwords hi - 16 .. hi - 1).
     * The four slots at hs hold dwords hi - 16 .. hi - 13: dead when c >= hi - 12, gap <= 12; the four behind them too when
     * gap <= 8.  The check hands over
     *     both prefetched groups   when gap <= 8 and both are there (ph == 0),     gap' = gap + 8,
     *     one                      when gap <= 12 otherwise,                       gap' = gap + 4,
     *     none                     when gap >= 13,                                 gap' = gap.
     * INVARIANT: gap' >= 9 after any check, given gap >= 1 before it.
     *   (a) ph == 0: gap in 1 .. 8 gives gap' = gap + 8 >= 9; gap in 9 .. 12 gives gap' >= 13; gap >= 13 stays.
     *   (b) ph == 1 (one group handed over, the other still in pf): that state is entered by the middle line above, with
     *       gap' >= 13, and left by the first check that hands anything over.  Checks in between change nothing, so the
     *       trip before this check began with gap' >= 13, and a trip moves c by at most 8 (below): gap >= 5 here, and
     *       gap in 5 .. 12 gives gap' = gap + 4 >= 9; gap >= 13 stays.
     *   A trip is four steps of at most 63 bits: u grows by at most 252, so c by at most (31 + 252) >> 5 = 8, and
     *   gap >= 9 - 8 = 1 before the next check: the premise.  A step looks at dwords c, c + 1, c + 2 where it STARTS; the
     *   trip's last step starts at most 189 bits in, c has moved by at most (31 + 189) >> 5 = 6, and c + 6 + 2 < c + 9 <= hi:
     *   every dword a step looks at is in the ring (none older than hi - 16 either: gap' <= 16 because nothing is handed
     *   over above gap 12 and two groups only up to gap 8).  The bound is tight, so the ring cannot be smaller.
     * pf[0 .. 3] is always the next group: when one group goes, the other moves down (four copies in that branch only),
     * and the two groups of a line are still asked for together, when both have gone.
     * (A check every second step that hands over one group, picked with eight selects: the trip's one check alone measured
     * +3.5 % on 64 KiB entries, profiles/r9, DESIGN.md section 3 K1) */
/* (Reloading the prefetch registers in every lane at every check -- no merge copies, 13 vector instructions fewer per trip --
 * measured 5 % slower on 64 KiB entries: profiles/r5/call21_probe.log, call22) */
#define MZ_CHASE_REFILL_PUT(o_)                                                              \
    {                                                                                        \
        uint32_t *const w_ = P(row) + P(hs);                                                 \
        w_[0] = P(pf)[(o_) + 0];                                                             \
        w_[1] = P(pf)[(o_) + 1];                                                             \
        w_[2] = P(pf)[(o_) + 2];                                                             \
        w_[3] = P(pf)[(o_) + 3];                                                             \
        if (P(hs) == 0u) {                                                                   \
            P(row)[MZ_CRING_DW] = P(pf)[(o_) + 0];                                           \
            P(row)[MZ_CRING_DW + 1u] = P(pf)[(o_) + 1];                                      \
        }                                                                                    \
        P(hs) = (P(hs) + 4u) & (MZ_CRING_DW - 1u);                                           \
        P(hi) += 4u;                                                                         \
    }
#define MZ_CHASE_REFILL(active_)                                                             \
    if (active_) {                                                                           \
        const uint32_t gap_ = P(hi) - (P(u) >> 5);                                           \
        if (gap_ <= MZ_CRING_DW - 4u) {                                                      \
            const uint32_t two_ = (gap_ <= MZ_CRING_DW - 8u && P(ph) == 0u) ? 1u : 0u;       \
            MZ_CHASE_REFILL_PUT(0)                                                           \
            if (two_) MZ_CHASE_REFILL_PUT(4)                                                 \
            if (two_ | P(ph)) { /* both are in the ring: the next two groups, one line */    \
                P(ph) = 0u;                                                                  \
                MZ_CHASE_RELOAD_DW4(pf, 0, P(hi))                                            \
                MZ_CHASE_RELOAD_DW4(pf, 4, P(hi) + 4u)                                       \
            } else {                                                                         \
                P(pf)[0] = P(pf)[4];                                                         \
                P(pf)[1] = P(pf)[5];                                                         \
                P(pf)[2] = P(pf)[6];                                                         \
                P(pf)[3] = P(pf)[7];                                                         \
                P(ph) = 1u;                                                                  \
            }                                                                                \
        }                                                                                    \
    }
#define MZ_CHASE_ST16(p_, v_) __builtin_memcpy((p_), &(v_), 16);
#define MZ_CHASE_STORE_QUAD(base_, quad_)                                                    \
    if (P(lacc) != 0u) { /* (a lane that took no step in the trip has nothing to say: nobody reads behind its last record) */ \
        uint8_t *const p_ = (base_) + MZ_REC_ADDR((uint32_t)(quad_), (uint32_t)lane);       \
        mz_dw4 v_;                                                                           \
        v_.v[0] = P(rb)[0];                                                                  \
        v_.v[1] = P(rb)[1];                                                                  \
        v_.v[2] = P(rb)[2];                                                                  \
        v_.v[3] = P(rb)[3];                                                                  \
        MZ_CHASE_ST16(p_, v_)                                                                \
    }
    /* one step of a lane's own walk; B = 0 .. 3: which step of the trip (its record register, its byte of the K word) */
#define MZ_CHASE_OWN_STEP(B)                                                                 \
    if (P(run)) {                                                                            \
        const uint32_t *const rp_ = P(row) + ((P(u) >> 5) & (MZ_CRING_DW - 1u));             \
        uint32_t r_;                                                                         \
        const uint32_t k_ = mz_chase_step(L, rp_[0], rp_[1], rp_[2], P(u), P(lim) - P(u), &r_); \
        /* no valid step here (no bits), or one that would end behind the input: it stays undecoded, its leading literal \
         * too, and the walk ends.  (Written for the instruction count: every line here runs 170 times per lane and 64 KiB) */ \
        const uint32_t nu_ = P(u) + (k_ & 63u);                                              \
        const uint32_t ok_ = (((k_ & 63u) != 0u) & (nu_ <= Eu)) ? 1u : 0u;                   \
        const uint32_t kk_ = ok_ ? k_ : 0u; /* 1 .. 0x7F: went on, 0x80 ..: end of block, 0: invalid */ \
        P(rb)[(B)] = r_;                                                                     \
        P(lacc) |= kk_ << (8 * (B)); /* the step's bits (what a chasing lane needs to know of it) and kind */ \
        P(sn) += ok_;                                                                        \
        P(u) = ok_ ? nu_ : P(u);                                                             \
        P(sfl) = kk_; /* the last step's K byte: how the walk ended is read off it behind the loop */ \
        P(run) = (((kk_ - 1u) < 0x7Fu) & (nu_ < P(lim))) ? 1u : 0u;                          \
    }
    /* two steps */
#define MZ_CHASE_OWN_PAIR(B) /* (the trip's one check stands at its top) */                  \
    MZ_LANES { MZ_CHASE_OWN_STEP(B) }                                                        \
    MZ_LANES { MZ_CHASE_OWN_STEP((B) + 1) }
#define MZ_CHASE_STORE_LEN(base_, cap_, row_)                                                \
    {                                                                                        \
        mz_dw4 v_;                                                                           \
        v_.v[0] = P(la)[0];                                                                  \
        v_.v[1] = P(la)[1];                                                                  \
        v_.v[2] = P(la)[2];                                                                  \
        v_.v[3] = P(la)[3];                                                                  \
        MZ_CHASE_ST16((base_) + ((uint32_t)lane * (cap_) + ((uint32_t)(row_) << 4)), v_) \
    }

    /* ---- pass 1: every lane walks its own span, four steps per trip ---- */
    PV(uint32_t, lacc);   /* K bytes of the trip's four steps */
    PV2(uint32_t, la, 4); /* ... of the last sixteen steps: one 16-byte store per lane into its own row of the K stream */
    MZ_LANES { P(lacc) = P(la)[0] = P(la)[1] = P(la)[2] = P(la)[3] = 0u; }
    /* the trip before goes out at the top of the next one, right behind the refill's wait: its quad of records, and its
     * K word into the sixteen-step register (a scalar branch picks which) */
#define MZ_CHASE_RETIRE_TRIP(base_, t_)                                                      \
    {                                                                                        \
        const uint32_t j_ = (((t_) - 4u) >> 2) & 3u;                                         \
        MZ_LANES {                                                                           \
            MZ_CHASE_STORE_QUAD(base_, ((t_) - 4u) >> 2)                                     \
            if (j_ == 0u) P(la)[0] = P(lacc);                                                \
            else if (j_ == 1u) P(la)[1] = P(lacc);                                           \
            else if (j_ == 2u) P(la)[2] = P(lacc);                                           \
            else P(la)[3] = P(lacc);                                                         \
        }                                                                                    \
    }
    uint32_t t1 = 0;
    for (;;) {
        /* (one way out, at the top: a second one in the middle of the body cost the loop ~20 register copies per trip) */
        uint64_t live;
        MZ_BALLOT(live, P(run) != 0u);
        if (!live || t1 >= MZ_REC_CAP1) break;
        MZ_LANES { MZ_CHASE_REFILL(P(run)) }
        if (t1) {
            MZ_CHASE_RETIRE_TRIP(Rp, t1)
            if ((t1 & 15u) == 0u) {
                MZ_LANES { MZ_CHASE_STORE_LEN(Lp, MZ_REC_CAP1, (t1 >> 4) - 1u) }
            }
        }
        MZ_LANES { P(lacc) = 0u; }
        MZ_WAVE_SYNC();
        MZ_LANES { MZ_CHASE_OWN_STEP(0) }
        MZ_LANES { MZ_CHASE_OWN_STEP(1) }
        MZ_CHASE_OWN_PAIR(2)
        t1 += 4u;
    }
    MZ_LANES {
        if (P(run)) { /* the record cap ended the loop */
            P(sfl) = 0x300u; /* (3 below) */
            P(run) = 0u;
        }
    }
    if (t1) {
        MZ_CHASE_RETIRE_TRIP(Rp, t1)
        MZ_LANES { MZ_CHASE_STORE_LEN(Lp, MZ_REC_CAP1, (t1 - 1u) >> 4) } /* (words of the row that this window did not reach hold older bytes: never looked at) */
    }
    MZ_LANES {
        /* how it ended: 0 crossed into the next span (or went on), 1 end-of-block, 2 invalid code, 3 record cap */
        P(sfl) = (P(sfl) == 0x300u) ? 3u : (P(sfl) == 0u) ? 2u : (P(sfl) >> 7) & 1u;
        P(sxe) = P(u); /* where the own walk ended (the cursor goes on in pass 2) */
        tab_walk[lane] = P(sn) | (P(sfl) << 16);
    }
    MZ_STAT(5, t1);
    MZ_WAVE_SYNC();
    MZ_CHASE_FENCE(); /* the lengths (and, in the emit, the records) are read back through other lanes' addresses */
    MZ_PROF_MARK(4);  /* pass 1 */

    /* ---- pass 2: every lane that crossed keeps walking until it meets the walk of the lane whose span it is in ---- */
    PV(uint32_t, chs); /* chasing */
    PV(uint32_t, tj);  /* the lane whose walk is being replayed, */
    PV(uint32_t, tt);  /* the next of its steps, */
    PV(uint32_t, uo);  /* where that step starts, */
    PV(uint32_t, tn);  /* how many it has | how its walk ended << 16 */
    PV(uint32_t, lb);  /* first step of the 16 whose lengths are in lw */
    PV(uint32_t, pb);  /* ... and of those in flight into lp */
    PV2(uint32_t, lw, 4);
    PV2(uint32_t, lp, 4);
    /* 16 lengths of lane lane_'s walk from step t_ on (any t_: the rows are byte-addressed) */
#define MZ_CHASE_LOAD_LEN(dst, lane_, t_)                                                    \
    {                                                                                        \
        mz_dw4 v_;                                                                           \
        __builtin_memcpy(&v_, Lp + ((lane_) * MZ_REC_CAP1 + (t_)), 16);                             \
        P(dst)[0] = v_.v[0];                                                                 \
        P(dst)[1] = v_.v[1];                                                                 \
        P(dst)[2] = v_.v[2];                                                                 \
        P(dst)[3] = v_.v[3];                                                                 \
    }
    /* (a target is taken in front of a trip only, where the window of lengths moves on anyway -- its first sixteen lengths
     * are asked for as the load in flight, and the renewal right behind hands them over) */
#define MZ_CHASE_TARGET(lane_)                                                               \
    {                                                                                        \
        P(tt) = 0u;                                                                          \
        P(uo) = Wu + (lane_) * S;                                                            \
        P(tn) = tab_walk[(lane_)];                                                           \
        P(pb) = 0u;                                                                          \
        MZ_CHASE_LOAD_LEN(lp, (lane_), 0u)                                                   \
    }
    MZ_LANES {
        P(chs) = ((uint32_t)lane + 1u < nact && P(sfl) == 0u) ? 1u : 0u;
        P(cm) = 0u;
        P(cfl) = 4u;
        P(csx) = 0u;
        P(cst) = 0u;
        P(tj) = ((uint32_t)lane + 1u) & 63u;
        P(tt) = P(uo) = P(tn) = P(lb) = P(pb) = 0u;
        P(lw)[0] = P(lw)[1] = P(lw)[2] = P(lw)[3] = 0u;
        P(lp)[0] = P(lp)[1] = P(lp)[2] = P(lp)[3] = 0u;
        if (P(chs)) MZ_CHASE_TARGET(P(tj))
        P(lacc) = 0u;
    }
    /* one step of a chase; K = 0 / 1: which half of the pair.  A two-pointer merge of bit positions: the replay of the
     * other lane's steps may advance twice per step, the lane's own decode once; whichever pointer is behind moves,
     * equal positions end the chase.  (Twice: a replay that moves only as often as the decode never closes a gap, and
     * behind a gap equal positions are never seen.)  The lengths come from a 16-step window that is renewed every
     * fourth step from a load issued four steps earlier: at most 8 advances in between, so it never runs dry. */
#define MZ_CHASE_REPLAY_ONE                                                                  \
    if (P(chs) && P(tt) < (P(tn) & 0xFFFFu) && P(uo) < P(u)) {                               \
        const uint32_t ix_ = P(tt) - P(lb);                                                  \
        const uint32_t wa_ = (ix_ & 4u) ? P(lw)[1] : P(lw)[0], wb_ = (ix_ & 4u) ? P(lw)[3] : P(lw)[2]; \
        P(uo) += mz_bfe((ix_ & 8u) ? wb_ : wa_, 8u * (ix_ & 3u), 6); /* (the K byte's low six bits) */ \
        P(tt)++;                                                                             \
    }
    /* A step only ever STOPS a chase -- at a meeting point, an end of block, an invalid code -- and says how in cfl; it
     * takes no new target (MZ_CHASE_RETARGET, in front of the trip) and copies nothing: a lane that has stopped replays no
     * more, so tj and tt stay what they were at the meeting point and are read off behind the loop. */
#define MZ_CHASE_STEP(K)                                                                     \
    MZ_CHASE_REPLAY_ONE                                                                      \
    MZ_CHASE_REPLAY_ONE                                                                      \
    {                                                                                        \
        const uint32_t on_ = P(tn) & 0xFFFFu, of_ = P(tn) >> 16;                             \
        const uint32_t meet_ = (P(chs) != 0u && P(uo) == P(u) && (P(tt) < on_ || of_ == 0u)) ? 1u : 0u; \
        P(cfl) = meet_ ? 0u : P(cfl);                                                        \
        P(chs) = meet_ ? 0u : P(chs);                                                        \
    }                                                                                        \
    if (P(chs)) {                                                                            \
        const uint32_t *const rp_ = P(row) + ((P(u) >> 5) & (MZ_CRING_DW - 1u));             \
        uint32_t r_;                                                                         \
        const uint32_t k_ = mz_chase_step(L, rp_[0], rp_[1], rp_[2], P(u), 64u, &r_);        \
        const uint32_t ok_ = ((k_ & 63u) != 0u && P(u) + (k_ & 63u) <= Eu) ? 1u : 0u;        \
        const uint32_t kk_ = ok_ ? k_ : 0u;                                                  \
        P(rb)[(K)] = r_;                                                                     \
        P(lacc) |= kk_ << (8 * (K));                                                         \
        P(cm) += ok_;                                                                        \
        P(u) += kk_ & 63u;                                                                   \
        if (!ok_ || (k_ & MZ_K_EOB)) {                                                       \
            P(cfl) = ok_ ? 1u : 2u;                                                          \
            P(chs) = 0u;                                                                     \
        }                                                                                    \
    }
    /* In front of a trip: a lane whose target's walk is over (it crossed behind the lane, or stopped for a reason of its
     * own) and is no meeting point takes the next span's lane, or leaves the window.  See the proof at the loop. */
#define MZ_CHASE_RETARGET                                                                    \
    if (P(chs)) {                                                                            \
        const uint32_t on_ = P(tn) & 0xFFFFu, of_ = P(tn) >> 16;                             \
        if (P(tt) >= on_ && (P(uo) < P(u) || (P(uo) == P(u) && of_ != 0u))) {                \
            P(tj)++;                                                                         \
            MZ_STAT(27, 1); /* targets taken behind the first */                             \
            if (P(tj) >= nact) {                                                             \
                P(chs) = 0u; /* (cfl is still 4: only a lane that stops sets it) */          \
            } else {                                                                         \
                MZ_CHASE_TARGET(P(tj))                                                       \
            }                                                                                \
        }                                                                                    \
    }
    /* the trip before: its quad of records and its four K bytes (one dword into the lane's row of the chases' K stream) */
#define MZ_CHASE_RETIRE_CHASE_TRIP(t_)                                                       \
    MZ_LANES {                                                                               \
        MZ_CHASE_STORE_QUAD(Cp, ((t_) - 4u) >> 2)                                            \
        if (P(lacc) != 0u) mz_st4(Lc + ((uint32_t)lane * MZ_REC_CAP2 + ((t_) - 4u)), P(lacc)); \
    }
    /* ONE place per trip where a chase takes a new target, in front of the trip, and not one in each of its four steps.
     * (A retarget in every step -- a table read, a 16-byte load with its wait and ~18 register copies per step in every wave,
     * retarget or not -- measured 1.4 % slower on 64 KiB entries: profiles/r10, DESIGN.md section 3 K1)
     * WHAT CHANGES against a retarget in the step where the target ran out: only WHEN a lane starts to replay its next
     * target -- up to three steps later.  WHAT DOES NOT: what the lane decodes.  A chasing lane decodes one step per step of
     * the trip, with or without a target to replay, so u after k steps, the records rb / lacc, their
     * slots (step t2 + K of the chase is record t2 + K: no step is left out, so there are no holes in the quads or in the K
     * stream), cm, and an end of block or invalid code with its cfl = 1 / 2 are the same step for step.  A lane that idled
     * until the next trip instead would leave such holes; it must not.
     * PROOF that the result of the window is a true parse all the same.  The chain (inflate_chase.inc) asks of a chase
     * only this: cfl == 0 means that after cm recorded steps the cursor u stands where step cst of lane csx's own walk
     * starts (or, cst == sn of a lane that crossed, where that walk ended); cfl != 0 means that after cm recorded steps the
     * cursor is u, and why it stopped.  A step sets cfl = 0 under one condition only -- uo == u with uo the
     * sum of the first tt lengths of lane tj's walk from its span's start, tt < on or the walk crossed -- and csx / cst are tj
     * / tt of that moment, because a lane that stopped replays no more and takes no target (both ask for chs); they are
     * read off behind the loop.  So every meeting point reported is one.  It may be a LATER one of the same two walks than
     * an immediate retarget would find, or one with a later lane; the chain then follows this lane's records (the same tokens: two walks that stand
     * on one token start decode the same from there) for longer before it changes over.  Leaving the window (tj reaches
     * nact) is noticed up to three steps later: cm and u are those steps further on, valid steps each (ok_ asks for
     * every one to end inside the input), and the next window starts there.  The record cap: a chase still running at
     * t2 == MZ_REC_CAP2 gets cfl = 3, possibly one that an immediate retarget would have let meet in its last steps; the chain ends
     * there and the next window goes on from u with shorter spans -- slower, never different bytes.
     *   A target that is over but IS a meeting point (uo == u, the walk crossed, tt == on) is left for step 0 to report: the
     * retarget asks for uo < u, or uo == u behind a walk that stopped for a reason of its own.
     * The window of lengths: lw holds sixteen lengths from step lb of the target on, lp the load in flight from pb on.  A
     * trip advances tt by at most 8; lw was asked for one trip ago at tt of then, so tt - lb <= 15 throughout.  A new
     * target asks for its first sixteen as the load in flight and the renewal right behind it hands them over (lb = 0,
     * tt = 0) and asks again: no copy of the window outside the renewal. */
    uint32_t t2 = 0;
    for (;;) {
        MZ_LANES { MZ_CHASE_RETARGET }
        uint64_t live;
        MZ_BALLOT(live, P(chs) != 0u);
        if (!live || t2 >= MZ_REC_CAP2) break;
        /* the same renewal in two halves with the compiler's memory barrier between them: the load is to go straight into
         * lp's registers, which are free once lw has taken their values.  (In one piece the load was issued first, into
         * registers of its own, and waited for on the spot to be copied into lp: the prefetch hid nothing.) */
        MZ_LANES { /* (every lane, chasing or not: one wait for the load in flight that no path goes round) */
            P(lw)[0] = P(lp)[0];
            P(lw)[1] = P(lp)[1];
            P(lw)[2] = P(lp)[2];
            P(lw)[3] = P(lp)[3];
            P(lb) = P(pb);
            P(pb) = P(tt);
#if !defined(MZHIP_HOST_EMUL)
            /* (the copies stand HERE, with their wait, in front of the refill's loads: left to itself the compiler sinks them
             * behind the refill and waits for the groups it has just asked for) */
            asm volatile("" : "+v"(lw[0]), "+v"(lw[1]), "+v"(lw[2]), "+v"(lw[3]) : : "memory");
#endif
        }
        MZ_LANES { MZ_CHASE_REFILL(P(chs)) } /* (in front of the load: its wait for the prefetched groups would wait for the load too) */
        MZ_WAVE_SYNC();
        MZ_LANES {
            if (P(chs)) MZ_CHASE_LOAD_LEN(lp, P(tj), P(tt))
        }
        if (t2) MZ_CHASE_RETIRE_CHASE_TRIP(t2)
        MZ_LANES { P(lacc) = 0u; }
        MZ_WAVE_SYNC();
        MZ_LANES { MZ_CHASE_STEP(0) }
        MZ_LANES { MZ_CHASE_STEP(1) }
        MZ_LANES { MZ_CHASE_STEP(2) }
        MZ_LANES { MZ_CHASE_STEP(3) }
        t2 += 4u;
    }
    MZ_LANES {
        if (P(chs)) { /* the record cap ended the loop */
            P(cfl) = 3u;
            P(chs) = 0u;
        }
        if (P(cfl) == 0u) { /* met: the target and its step have not moved since */
            P(csx) = P(tj);
            P(cst) = P(tt);
        }
    }
    if (t2) MZ_CHASE_RETIRE_CHASE_TRIP(t2)
    MZ_STAT(7, t2);
    MZ_WAVE_SYNC();
    MZ_CHASE_FENCE();
    MZ_PROF_MARK(5); /* pass 2 */
#undef MZ_CHASE_REFILL
#undef MZ_CHASE_REFILL_PUT
#undef MZ_CHASE_OWN_STEP
#undef MZ_CHASE_OWN_PAIR
#undef MZ_CHASE_STORE_LEN
#undef MZ_CHASE_REPLAY_ONE
#undef MZ_CHASE_STEP
#undef MZ_CHASE_RETARGET
#undef MZ_CHASE_RETIRE_TRIP
#undef MZ_CHASE_RETIRE_CHASE_TRIP
#undef MZ_CHASE_STORE_QUAD
#undef MZ_CHASE_ST16
#undef MZ_CHASE_LOAD_LEN
#undef MZ_CHASE_TARGET
#undef MZ_CHASE_LOAD_DW4
#undef MZ_CHASE_RELOAD_DW4

    mz_walk_result wr;
    MZ_LANES {
        P(wr.u) = P(u);
        P(wr.sn) = P(sn);
        P(wr.sfl) = P(sfl);
        P(wr.sxe) = P(sxe);
        P(wr.cm) = P(cm);
        P(wr.cfl) = P(cfl);
        P(wr.csx) = P(csx);
        P(wr.cst) = P(cst);
    }
    return wr;
}
