/* inflate_chase.inc -- one span window of K1, round 3: DECODE ONCE, THEN CHASE.  Textually included by mz_inflate_entry()
 * (span path) with `remain` = bits from the cursor to the end of the view; uses that function's locals
 * (L, in_al, in_mis, in_len, bitpos, pbase, out, out_pos, out_cap, rec, sub_used, span_on, span_skip, crc_*).  Leaves with
 * `continue` (tokens committed, next window), `break` (the block ended inside the window) or by falling out of its
 * block (the step loop takes the next step).
 *
 * The round-2 window (deleted in round 5; git history has inflate_window.inc) let 64 lanes walk 64 spans of 256 bits again and again until no start moved:
 * 3.85 counting passes + 3.14 emitting passes, every token Huffman-decoded ~5 times (78 walk steps per 16 128 bits).
 * Here every token is decoded once, plus the self-synchronisation distance of DEFLATE once per span
 * (tests/study/span_chase.c: 21 steps per 16 128 bits when a 64 KiB entry is one window):
 *
 *   spans    the rest of the stream (minus a 64-bit margin: the longest token is 48 bits) is cut into <= 64 spans of S bits,
 *            128 <= S <= MZ_CHASE_SMAX, one per lane.  The stream reaches a lane through its own 12-dword LDS ring,
 *            topped up 16 bytes at a time every second step from a register that was loaded two steps earlier.
 *   pass 1   lane i walks from the first bit of span i (lane 0: the true cursor) until it crosses into span i + 1, meets an
 *            end-of-block or an invalid code, and RECORDS every step -- one dword (leading literal, literal byte or match
 *            length, distance: mz_chase_step) plus one byte (the step's bits and what its token is) -- in the wave's HBM
 *            scratch: four steps per 16-byte store, [quad][lane] so that a store instruction of the wave is 1 KiB
 *            contiguous (MZ_REC_ADDR); the bytes in a per-lane stream, sixteen steps per store.  (Round 3 wrote two
 *            dwords a step: twice the bytes, and FETCH_SIZE 4.4x of them on the way back.)
 *   pass 2   lane i keeps walking from its crossing (recording, too) and reads the records of the lane whose span it is
 *            in alongside ("chase": a two-pointer merge of bit positions) until it stands on a token start that lane's walk
 *            also visited.  From there that lane's records ARE the true parse, if lane i's were.
 *   chain    lane 0 is true; following "whom did you meet, at which step" from lane 0 yields the true parse as a list of
 *            segments: lane j's own records from its entry step on, then lane j's chase records, then the lane it met ...
 *   emit     the records of the chain are taken MZ_EMIT_GROUP at a time by 64 lanes in stream order (a lane finds its
 *            group by a binary search in the prefix sums of the lanes' group counts), counted, prefix-summed, cut where
 *            the pool is full -- at record granularity, so there is no "does not fit" failure -- and written as staging
 *            bytes / back-reference pieces; inflate_commit.inc (far, near, store, CRC) is the round-2 code unchanged.
 * Nothing is decoded twice; what the lanes wait for is the slowest walk (once) and the longest chase (once) per window.
 * The price: 5 bytes of HBM scratch written and read per step (~1.6 tokens), and two loops with global stores in them --
 * every wait for a load also waits for the stores (one counter on gfx9), so both are issued two steps before the wait.
 * Anything this path cannot decide exactly -- an invalid code on the true chain, output that does not fit the entry's
 * capacity, a distance that reaches before the entry -- is left to the step loop, which owns the verdicts in stream
 * order: the window ends in front of the emit round in question (nothing of a round leaves LDS before it is checked). */
{
    static_assert(MZ_EMIT_GROUP == 4u || MZ_EMIT_GROUP == 8u, "an emit group is one or two quads of records (and at most the eight K bytes of one load)");
    static_assert(MZ_REC_CAP1 % 16u == 0u && MZ_REC_CAP2 % 4u == 0u, "record caps: whole K-stream stores");
    uint32_t *const ring = MZ_L_WIN(L);
    /* while the records become bytes the rings are dead: the pool runs on through them -- staging bytes and pending bits
     * from the front, the chain's per-lane tables (1 KiB) at the very end, the piece list downwards from there
     * (inflate_emit.inc lays the same addresses out for itself) */
    uint32_t *const tab_n = ring + 64u * MZ_CRING_RS - 256u, *const tab_e = tab_n + 64, *const tab_m = tab_n + 128, *const tab_g = tab_n + 192;
    uint32_t *const tab_walk = L->u.b.x.pool; /* while the lanes walk (the pool is idle): steps | flag << 16 of every lane's own walk */
    /* Record scratch of the wave (MZ_REC_BYTES): own walks' records, chases' records -- four records of a lane are one
     * 16-byte quad, [quad][lane]: written by all lanes for the same quad at once (a wave's store is 1 KiB contiguous), read
     * back (emit) by ONE lane for MZ_EMIT_GROUP consecutive steps of one lane's walk: two 16-byte loads 1 KiB apart, half
     * of every 32-byte sector they touch (the round-3 layout, 8-byte records in [pair][lane], used a quarter; a per-lane
     * 64-byte-pieces layout measured 4 % slower, profiles/r3/ab_rec_layout.log) -- then the K bytes (bits | kind << 6,
     * mz_chase_step) of the own walks and of the chases, a per-lane stream each (inflate_walk.inc, inflate_emit.inc). */
    /* the rest of the stream in 64 spans (or fewer, of 128 bits at least; or only MZ_CHASE_SMAX bits each of a long one).
     * No margin at the end of the input: a step is taken only when its last bit lies inside the input (bytes behind the
     * end read as zero), so the last lane normally walks into the final end-of-block and the step loop never runs. */
    uint32_t S = (remain + 63u) >> 6;
    if (S > chase_smax) S = chase_smax; /* (MZ_CHASE_SMAX, less after a window of this entry ran into a record cap) */
    if (S < 128u) S = 128u;
    uint32_t nact = (remain + S - 1u) / S;
    if (nact > 64u) nact = 64u;
    const uint32_t Eu = total_bits + pbase; /* the end of the input ... */
    const uint32_t Wu = bitpos + pbase; /* ... and the cursor in "u" coordinates: stream bits counted from the aligned dword that holds in[0] */
    MZ_STAT(8, 1);
    /* the two walks (pass 1: every lane its own span; pass 2: the chase into the next one) are a function of their own,
     * NOT inlined: inside this function's register allocation the compiler reloaded spilled values in the middle of the walk
     * loops, each reload a vmcnt(0) behind the record stores (profiles/r4: pass 1 +50 % cycles); on its own the walk keeps
     * its state in registers and the call is paid once per window (inflate_walk.inc) */
    PV(uint32_t, u);   /* where the lane's cursor ended up (after its chase) */
    PV(uint32_t, sn);  /* own walk: steps recorded, */
    PV(uint32_t, sfl); /* how it ended: 0 crossed into the next span, 1 end-of-block, 2 invalid code, 3 record cap, */
    PV(uint32_t, sxe); /* and where */
    PV(uint32_t, cm);  /* chase steps recorded */
    PV(uint32_t, cfl); /* how the chase ended: 0 met a lane's walk, 1 end-of-block, 2 invalid code, 3 record cap, 4 left the window */
    PV(uint32_t, csx); /* the lane it met ... */
    PV(uint32_t, cst); /* ... at the start of this step of that lane's walk */
    {
        const mz_walk_result wr = mz_chase_walk(MZ_LDS_HANDLE(L), MZ_GLB_HANDLE(in_al), in_mis, in_len, Wu, Eu, S, nact, MZ_LDS_HANDLE(tab_walk), MZ_GLB_HANDLE(rec), edge_ev MZ_PROF_ARGS);
        MZ_LANES {
            P(u) = P(wr.u);
            P(sn) = P(wr.sn);
            P(sfl) = P(wr.sfl);
            P(sxe) = P(wr.sxe);
            P(cm) = P(wr.cm);
            P(cfl) = P(wr.cfl);
            P(csx) = P(wr.csx);
            P(cst) = P(wr.cst);
        }
    }

    /* ---- the chain: lane 0's walk is the true parse; whoever it met goes on from the step they met at, and so on ---- */
    PV(uint32_t, ent); /* lanes on the chain: 0x10000 | the step their records count from (| 0x8000: without that step's leading literal) */
    PV(uint32_t, hcm); /* ... and the chase steps that follow (0: the chain does not go through this lane's chase) */
    uint32_t capped = 0; /* the chain ends at a record cap: the lanes behind walked for nothing */
    uint32_t endu, endfl; /* where the chain ends, and how: 0 go on with the next window, 1 end of block, 2 the step loop has a verdict to give */
    MZ_LANES {
        P(ent) = 0u;
        P(hcm) = 0u;
    }
    {
        /* almost every lane crosses into the next span and meets the walk of the lane next to it: those runs of the chain
         * are marked by all lanes at once (lane l + 1 starts at the step lane l met it at); the scalar loop only stops
         * at the ends of such runs */
        PV(uint32_t, pst);
        MZ_GATHER4(pst, cst, (4u * ((uint32_t)lane - 1u)) & 255u);
        uint64_t reg;
        MZ_BALLOT(reg, P(sfl) == 0u && (uint32_t)lane + 1u < nact && P(cfl) == 0u && P(csx) == (uint32_t)lane + 1u);
        uint32_t on = 0, et = 0;
        for (;;) {
            const uint64_t m = ~(reg >> on);
            const uint32_t run = m ? mz_ctz64(m) : 64u; /* lanes on .. on + run - 1 hand the chain to their neighbour */
            MZ_LANES {
                if ((uint32_t)lane == on) P(ent) = 0x10000u | et;
                if ((uint32_t)lane > on && (uint32_t)lane <= on + run) P(ent) = 0x10000u | P(pst);
                if ((uint32_t)lane >= on && (uint32_t)lane < on + run) P(hcm) = P(cm);
            }
            if (run) {
                on += run;
                et = MZ_READLANE(cst, on - 1u);
            }
            /* lane `on` is on the chain (entered at step et) and does not simply hand over to lane on + 1 */
            const uint32_t f = MZ_READLANE(sfl, on);
            if (f != 0u || on + 1u >= nact) {
                endu = MZ_READLANE(sxe, on);
                endfl = (f == 3u) ? 0u : f;
                if (f == 3u) capped = 1u;
                break;
            }
            MZ_WRITELANE(hcm, on, MZ_READLANE(cm, on));
            const uint32_t cf = MZ_READLANE(cfl, on);
            if (cf != 0u) {
                endu = MZ_READLANE(u, on);
                endfl = (cf == 1u) ? 1u : (cf == 2u) ? 2u : 0u;
                if (cf == 3u) capped = 1u;
                break;
            }
            et = MZ_READLANE(cst, on); /* met a lane further on (the chase ran through a whole span) */
            on = MZ_READLANE(csx, on);
        }
    }
    /* a stream whose steps are so short that spans of S bits take more steps than a lane may record (long runs: a
     * 258-byte match can be 2 bits) gets shorter spans from here on -- otherwise every window would throw away what 63
     * of its lanes did */
    MZ_STAT(23, capped); /* windows whose chain ran into a record cap */
    if (capped && S > 128u) chase_smax = (S >> 1) < 128u ? 128u : (S >> 1);
    /* per-lane tables for the emit (the rings are dead): steps, entry, chase steps, inclusive sums of the group counts */
    PV(uint32_t, gcn);
    PV(uint32_t, gsc);
    MZ_LANES {
        uint32_t g = 0;
        if (P(ent)) {
            const uint32_t ts = P(ent) & 0x7FFFu;
            g = (P(sn) > ts) ? ((P(sn) + MZ_EMIT_GROUP - 1u) / MZ_EMIT_GROUP) - ts / MZ_EMIT_GROUP : 0u;
            g += (P(hcm) + MZ_EMIT_GROUP - 1u) / MZ_EMIT_GROUP;
        }
        P(gcn) = g;
    }
    MZ_INCL_SCAN(gsc, gcn);
    const uint32_t NG = MZ_READLANE(gsc, 63);
    MZ_WAVE_SYNC();
    MZ_LANES {
        tab_n[lane] = P(sn);
        tab_e[lane] = P(ent);
        tab_m[lane] = P(hcm);
        tab_g[lane] = P(gsc);
    }
    MZ_WAVE_SYNC();
    MZ_PROF_MARK(10); /* the chain */

    /* ---- emit rounds: the chain's records become bytes (inflate_emit.inc: like the walks a function of its own, with a
     * register allocation of its own) ---- */
    uint32_t cbits, fail, emitted_all;
    if (par) { /* a block of a large entry on a wave of its own: counted, or turned into a source map -- nothing is copied here */
        const mz_ptr_result pr = mz_chase_emit_ptr(MZ_LDS_HANDLE(L), MZ_GLB_HANDLE(rec), NG, par->mode, MZ_GLB_HANDLE(out),
                                                   MZ_GLB_HANDLE(par->ptr), out_pos);
        out_pos += MZ_UNIFORM(pr.bytes);
        cbits = endu - Wu;
        fail = MZ_UNIFORM(pr.bad);
        emitted_all = 1u;
        if (fail || endfl == 2u) { /* a distance in front of the buffer, an invalid code next: stream order has the verdict */
            status = MZHIP_PAR_BAIL;
            goto finish;
        }
    } else {
        const mz_emit_result er = mz_chase_emit(MZ_LDS_HANDLE(L), sub_used, MZ_GLB_HANDLE(rec), MZ_GLB_HANDLE(out), out_pos, out_cap, NG,
                                                crc_base, crc_done, crc_acc, MZ_LDS_HANDLE(crc_tab), MZ_GLB_HANDLE(tabs) MZ_PROF_ARGS);
        out_pos = MZ_UNIFORM(er.out_pos); /* (results come back in vector registers: wave.h, MZ_UNIFORM64) */
        crc_done = MZ_UNIFORM(er.crc_done);
        cbits = MZ_UNIFORM(er.cbits);
        fail = MZ_UNIFORM(er.fail);
        emitted_all = MZ_UNIFORM(er.all);
        MZ_LANES { P(crc_acc) = P(er.crc_acc); }
    }
    (void)emitted_all;
#if defined(MZHIP_HOST_EMUL)
    if (!fail && (!emitted_all || cbits != endu - Wu)) abort(); /* the records of the chain are exactly the bits up to its end */
#endif
    if (!fail) cbits = endu - Wu;
    if (cbits == 0u) {
        if (fail) span_on = 0; /* not even the first round could be committed here: the step loop serves the rest of the block */
        else span_skip = 1;    /* the very first step is the problem (an invalid code, no room): the step loop has the verdict */
    } else {
        bitpos += cbits;
        if (fail) {
            span_skip = 1; /* the step loop meets the token in question and reports it in stream order */
        } else {
            if (endfl == 1u) break;         /* the block ended inside the window */
            if (endfl == 2u) span_skip = 1; /* an invalid code is next: the step loop has the verdict */
        }
        continue;
    }
}
