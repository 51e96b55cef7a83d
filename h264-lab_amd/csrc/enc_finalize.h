/*
 * enc_finalize.h -- a job's finalizer, wave64 model: the slice splice (splice_frame / finalize_commit), the exact mv_clusters walk
 * (clusters_walk_range / JobWalk), the export of a finished frame (nal_escape_copy / export_frame), and job_finalize at the end, which
 * follows one frame row by row with those pieces and publishes its verdict and its result record.
 *
 * splice_frame = the tail of encode_slice (h264-lab.h:6451-6456): concatenates the row bit buffers behind
 * the slice header, resolves mb_skip_run across rows, adds the RBSP trailing bits, and evaluates the
 * mv_clusters speculation.
 *
 * job_finalize is written once.  Everything in it that touches time or memory ordering goes through a policy passed in by value, like
 * the hand-offs of the macroblock step (enc_row.h): FinalizerOnDevice (h264e_kernels.hip) on the GPU, FinalizerInOrder (tests/emu) in
 * the emulation.
 */
#ifndef H264E_ENC_FINALIZE_H
#define H264E_ENC_FINALIZE_H

#include "enc_row.h"

/* ------------------------------------------------------------------ slice splice (one wavefront per chain) */

struct SpliceState { GLOBAL_AS uint32_t *out; uint32_t wpos; uint32_t carry; int cbits; uint32_t cap_words; int overflow; };

/* append nbits (<= 64) right-aligned bits */
DEV void splice_put(SpliceState &s, int nbits, uint64_t v)
{
    while (nbits > 0)
    {
        int take = imin(nbits, 32 - s.cbits);
        uint32_t part = (uint32_t)((v >> (nbits - take)) & ((take == 32) ? 0xffffffffu : ((1u << take) - 1)));
        s.carry = (take == 32) ? part : ((s.carry << take) | part);
        s.cbits += take;
        nbits -= take;
        if (s.cbits == 32)
        {
            if (s.wpos < s.cap_words) s.out[s.wpos] = bswap32(s.carry); else s.overflow = 1;
            s.wpos++;
            s.carry = 0; s.cbits = 0;
        }
    }
}

/* append the first nbits of an MSB-first word buffer, 64 words per pass */
DEV void splice_words(SpliceState &s, const GLOBAL_AS uint32_t *w, uint32_t nbits)
{
    const uint32_t nfull = nbits >> 5;
    const int cb = s.cbits;
    const uint32_t carry = s.carry;
    for (uint32_t base = 0; base < nfull; base += 64)
    {
        WAVE_FOR(l)
        {
            uint32_t k = base + (uint32_t)l;
            if (k < nfull)
            {
                uint32_t prev = k ? w[k - 1] : carry, cur = w[k];
                uint32_t o = cb ? ((prev << (32 - cb)) | (cur >> cb)) : cur;
                if (s.wpos + k < s.cap_words) s.out[s.wpos + k] = bswap32(o);
            }
        }
    }
    if (s.wpos + nfull > s.cap_words) s.overflow = 1;
    if (nfull)
    {
        s.wpos += nfull;
        s.carry = cb ? (w[nfull - 1] & ((1u << cb) - 1)) : 0;
    }
    const int rem = (int)(nbits & 31);
    if (rem) splice_put(s, rem, (uint64_t)(w[nfull] >> (32 - rem)));
}

DEV void put_ue64(SpliceState &s, uint32_t v)
{
    int n = 2*(32 - clz32(v + 1)) - 1;
    splice_put(s, n, (uint64_t)v + 1);
}

DEV void clusters_step(mv32 c[2], mv32 mv)                                  /* h264-lab.h:5263-5278 */
{
    int n = mvx(mv)*mvx(mv) + mvy(mv)*mvy(mv);
    int n0 = mvx(c[0])*mvx(c[0]) + mvy(c[0])*mvy(c[0]), n1 = mvx(c[1])*mvx(c[1]) + mvy(c[1])*mvy(c[1]);
    if (n < n1) c[0] = mvmk((63*mvx(c[0]) + mvx(mv) + 32) >> 6, (63*mvy(c[0]) + mvy(mv) + 32) >> 6);
    if (n >= n0) c[1] = mvmk((63*mvx(c[1]) + mvx(mv) + 32) >> 6, (63*mvy(c[1]) + mvy(mv) + 32) >> 6);
}

/*
 * The exact mv_clusters walk of one frame on the device (what h264e_host.c clusters_walk does on the host): from state s, in
 * raster order -- restarting from s at every slice of a multi-slice frame -- compare the rounded candidates every macroblock
 * CONSUMED (the frame-constant pair or its entry of the per-macroblock array) with the exact ones, then apply its update
 * (h264-lab.h:5263-5278).  The chain is serial, but almost no macroblock moves the state: 64 macroblocks per pass, a ballot
 * finds the next one that moves it or mismatches, everything in front of it is settled at once.  traj (optional) receives the
 * state in front of every macroblock.  Returns the first mismatching macroblock or -1; s = state behind the frame.
 */
/* macroblocks [k0, k1) of one slice, continuing from state s / verdict first_bad (the finalizer walks a frame row by row as its rows
 * complete; batches of 64 inside the range) */
DEV void clusters_walk_range(const h264e_frame_task_t &T, const GLOBAL_AS h264e_mbrec_t *rec, mv32 s[2], int &first_bad, GLOBAL_AS mv32 *traj, int k0, int k1)
{
    const GLOBAL_AS mv32 *per_mb = (const GLOBAL_AS mv32 *)T.clusters_per_mb;
    const mv32 u_frame0 = T.clusters[0], u_frame1 = T.clusters[1];
    for (int base = k0; base < k1; base += 64)
    {
        int start = 0;
        /* the state in front of every macroblock of the batch, one per lane (wave.h V64) */
        V64 mine0 = v64_make([&](int) -> int { return s[0]; }), mine1 = v64_make([&](int) -> int { return s[1]; });
        for (;;)
        {
            const mv32 c0 = s[0], c1 = s[1];
            const int fb = first_bad;
            const uint64_t ev = wave_ballot([&](int l) -> int {
                const int k = base + l;
                if (l < start || k >= k1) return 0;
                const mv32 mv0 = rec[k].mv0;
                const int type = rec[k].type;
                int hit = 0;
                if (fb < 0 && rec[k].used_cand)
                {
                    const mv32 u0 = per_mb ? per_mb[2*k] : u_frame0, u1 = per_mb ? per_mb[2*k + 1] : u_frame1;
                    if (mvround(u0) != mvround(c0) || mvround(u1) != mvround(c1)) hit = 1;
                }
                if (type < 5)
                {
                    mv32 c[2] = { c0, c1 };
                    clusters_step(c, mv0);
                    if (c[0] != c0 || c[1] != c1) hit = 1;
                }
                return hit;
            });
            if (!ev) break;
            const int e = __builtin_ctzll(ev), ke = base + e;
            /* macroblock ke: mismatch check first (against the state in front of it), then its update */
            if (first_bad < 0 && rec[ke].used_cand)
            {
                const mv32 u0 = per_mb ? per_mb[2*ke] : u_frame0, u1 = per_mb ? per_mb[2*ke + 1] : u_frame1;
                if (mvround(u0) != mvround(s[0]) || mvround(u1) != mvround(s[1])) first_bad = ke;
            }
            if (rec[ke].type < 5) clusters_step(s, rec[ke].mv0);
            s[0] = (mv32)uni(s[0]); s[1] = (mv32)uni(s[1]); first_bad = uni(first_bad);
            start = e + 1;
            mine0 = v64_map(mine0, [&](int l, int v) -> int { return l >= start ? s[0] : v; });
            mine1 = v64_map(mine1, [&](int l, int v) -> int { return l >= start ? s[1] : v; });
            if (start >= 64) break;
        }
        if (traj)
        {
            v64_each(mine0, [&](int l, int v) { const int k = base + l; if (k < k1) traj[2*k] = v; });
            v64_each(mine1, [&](int l, int v) { const int k = base + l; if (k < k1) traj[2*k + 1] = v; });
        }
    }
}

/* the whole frame at once (the walk of a complete frame: tests, tools) */
DEV int device_clusters_walk(const h264e_geom_t &G, const h264e_frame_task_t &T, const GLOBAL_AS h264e_mbrec_t *rec, mv32 s[2], GLOBAL_AS mv32 *traj)
{
    const mv32 s0[2] = { s[0], s[1] };
    int first_bad = -1;
    for (int band = 0; band < T.nslices; band++)
    {
        s[0] = s0[0]; s[1] = s0[1];
        clusters_walk_range(T, rec, s, first_bad, traj, T.slice_row[band]*G.nmbx, T.slice_row[band + 1]*G.nmbx);
    }
    if (T.nslices > 1) { s[0] = s0[0]; s[1] = s0[1]; }      /* the parent's state never moves in the row-band build (h264-lab.h:6526) */
    wave_sync();
    return first_bad;
}

/*
 * The finalizer's walk, ROW BY ROW as the rows complete (JobWalk::rows is called from the splice below, for the rows whose counters say
 * complete, once the state in front of the frame is known): the verdict of a frame is known a walk of ONE row after its last row ended.
 * The walk goes on behind a mismatch, over every row, as the whole-frame walk does: the trajectory behind the mismatch is the speculation
 * for the next encode of those rows, and it is a good one (the vectors of macroblocks that consumed slightly wrong candidates are mostly
 * the right ones).  Stopping the launch as soon as the row with the first mismatch has ended, with the state at the stop as the
 * trajectory of everything behind it, was built and measured in round 4: it wins a little where a frame fails once (1080p 4 Mbit/s:
 * +2.5 %) and loses badly where the state keeps moving through a frame (8K 60 Mbit/s, two slices: 50 launches instead of 22, the
 * re-encodes advance two or three rows at a time) -- not kept.
 */
struct JobWalk
{
    mv32 s0[2], s[2];
    int first_bad, next_row;
    DEVM void begin(const mv32 st[2]) { s0[0] = s[0] = st[0]; s0[1] = s[1] = st[1]; first_bad = -1; next_row = 0; }
    /* walks the rows up to and including `upto` that have not been walked yet (all of them complete) */
    DEVM void rows(const h264e_geom_t &G, const h264e_frame_task_t &T, const GLOBAL_AS h264e_mbrec_t *rec, GLOBAL_AS mv32 *traj, int upto)
    {
        for (; next_row <= upto; next_row++)
        {
            const int r = next_row;
            for (int k = 0; k < T.nslices; k++) if (r == T.slice_row[k]) { s[0] = s0[0]; s[1] = s0[1]; }      /* every slice starts from the state in front of the frame */
            clusters_walk_range(T, rec, s, first_bad, traj, r*G.nmbx, (r + 1)*G.nmbx);
        }
    }
    /* behind the last row: the state to hand on */
    DEVM void end(const h264e_frame_task_t &T)
    {
        if (T.nslices > 1) { s[0] = s0[0]; s[1] = s0[1]; }      /* the parent's state never moves in the row-band build (h264-lab.h:6526) */
        wave_sync();
    }
};

struct SpliceOut { uint32_t start, nbytes; int overflow, all_skipped, far_reads; };

/* The slices' RBSPs from the row bit buffers.  on_row(first row of the slice, row) is called before a row is touched: the caller waits
 * for the row there (and walks it); a non-zero return ends the splice with that code (nothing is committed). */
template <class ROW> DEV int splice_frame(const h264e_geom_t &G, const ChainG &C, const h264e_frame_task_t &T, SpliceOut &o, ROW on_row)
{
    SpliceState s;
    const uint32_t start = T.arena_reset ? 0u : ((*C.cursor + 15u) & ~15u);
    uint32_t off = 0;                                                           /* of the current slice, relative to start */
    int overflow = 0, all_skipped = 0, spl_overflow = 0, far_reads = 0;
    GLOBAL_AS h264e_frameout_t &F = C.fout[T.frame_slot];
    /* one RBSP per slice (row band); the slices of a frame lie behind each other, each starting 16-byte aligned */
    for (int k = 0; k < T.nslices; k++)
    {
        const int r0 = T.slice_row[k], r1 = T.slice_row[k + 1];
        const uint32_t room = start + off < C.arena_cap ? C.arena_cap - (start + off) : 0u;
        s.out = (GLOBAL_AS uint32_t *)(C.arena + start + off);
        s.wpos = 0; s.carry = 0; s.cbits = 0; s.overflow = 0;
        s.cap_words = room >> 2;
        splice_put(s, 8, (uint64_t)(uint32_t)T.hdr_nal);
        put_ue64(s, (uint32_t)(r0*G.nmbx));                                     /* first_mb_in_slice, h264-lab.h:4247 */
        splice_put(s, T.hdr_nbits, T.hdr_bits);
        int run = 0;
        for (int row = r0; row < r1; row++)
        {
            const int stop = on_row(r0, row);
            if (stop) return stop;
            const GLOBAL_AS h264e_rowmeta_t &M = C.rowmeta[row];
            overflow |= M.overflow;
            far_reads += C.far_reads[row];      /* the frame's own rows only: a frame that was stopped leaves nothing behind in one that ends */
            run += M.lead_skips;
            if (M.lead_skips < G.nmbx || M.nbits)
            {
                if (T.slice_type != 2) put_ue64(s, (uint32_t)run);
                wave_sync();
                splice_words(s, C.rowbits + (size_t)row*G.row_words, M.nbits);
                wave_sync();
                run = M.trail_skips;
            }
        }
        /* rc_frame_end's skip flag (h264-lab.h:6596): in the row-band build the parent's skip_run is never touched, so it is 0 there */
        if (T.nslices == 1) all_skipped = run == G.nmb;
        if (run) put_ue64(s, (uint32_t)run);                                    /* h264-lab.h:6451-6454 */
        splice_put(s, 1, 1);                                                    /* rbsp_stop_one_bit, h264-lab.h:3999 */
        const uint32_t nbytes = s.wpos*4 + (uint32_t)((s.cbits + 7) >> 3);
        if (s.cbits) { int pad = 32 - s.cbits; splice_put(s, pad, 0); }
        spl_overflow |= s.overflow;
        F.slice_nbytes[k] = nbytes;
        if (k + 1 < T.nslices) off += (nbytes + 15u) & ~15u; else off += nbytes;
        wave_sync();
    }
    o.start = start; o.nbytes = off; o.overflow = overflow | spl_overflow; o.all_skipped = all_skipped; o.far_reads = far_reads;
    return 0;
}

/* mv_clusters speculation check of the frame-at-a-time path (its host walks exactly when this says "moved"): is the speculated state
 * a fixed point of every update of this frame?  Frames validated by the device walk do not need it. */
DEV int clusters_moved(const h264e_geom_t &G, const h264e_frame_task_t &T, const GLOBAL_AS h264e_mbrec_t *rec)
{
    int moved = 0;
    if (!T.clusters_per_mb && !T.walk_on_device)
    {
        for (int base = 0; base < G.nmb; base += 64)
        {
            uint64_t bad = wave_ballot([&](int l) -> int {
                int k = base + l;
                if (k >= G.nmb || rec[k].type >= 5) return 0;
                mv32 c[2] = { T.clusters[0], T.clusters[1] };
                clusters_step(c, rec[k].mv0);
                return c[0] != T.clusters[0] || c[1] != T.clusters[1];
            });
            if (bad) moved = 1;
        }
    }
    return moved;
}

/* ... and the frame's result record, once the frame stands */
DEV void finalize_commit(const h264e_geom_t &G, const ChainG &C, const h264e_frame_task_t &T, const SpliceOut &o, GLOBAL_AS int *stepflags)
{
    GLOBAL_AS h264e_frameout_t &F = C.fout[T.frame_slot];
    const int moved = clusters_moved(G, T, C.mbrec + (size_t)T.frame_slot*G.nmb);
    F.offset = o.start;
    F.nbytes = o.nbytes;
    F.nslices = T.nslices;
    F.all_skipped = o.all_skipped;
    F.clusters_moved = moved;
    F.overflow = o.overflow;
    F.far_reads = o.far_reads;
    *C.cursor = o.start + ((o.nbytes + 15u) & ~15u);
    stepflags[0] = moved;
    stepflags[1] = o.overflow;
    wave_sync();
}

/*
 * RBSP -> Annex-B NAL on the device: 4-byte start code + payload with emulation prevention (h264-lab.h:3926-4022 nal_count_esc /
 * nal_put_esc: a 0x03 goes in front of every byte <= 3 that follows two zero bytes; the zero count restarts behind it).
 * The escape automaton is sequential, but it can only fire where the RAW bytes read 00 00 0x -- once per ~4 MB of CAVLC data.
 * So: 256-byte blocks, one dword per lane; a ballot finds the blocks that contain such a triple (two bytes of look-back across
 * the block edge); all other blocks are copied by the whole wave (shifted by the escapes inserted so far), a block with a
 * candidate is run through the automaton byte by byte by one lane with the exact carried zero count.
 * dst: 16-byte aligned (host-mapped memory or HBM).  Returns the NAL size; sets overflow when it does not fit cap.
 */
DEV uint32_t nal_escape_copy(GLOBAL_AS uint8_t *dst, uint32_t cap, const GLOBAL_AS uint8_t *src, uint32_t n, int &overflow)
{
    uint32_t esc = 0;           /* escapes inserted so far (wave-uniform) */
    int cntz = 0;               /* the automaton's zero count in front of the current block (exact whenever it matters) */
    if (n + 4u > cap) { overflow = 1; return 0; }
    if (wave_lane() == 0) gstore32((gu8 *)dst, 0x01000000u);                /* 00 00 00 01 */
    for (uint32_t base = 0; base < n; base += 256)
    {
        const uint32_t len = n - base < 256u ? n - base : 256u;
        const uint64_t cand = wave_ballot([&](int l) -> int {
            const uint32_t o = base + 4u*(uint32_t)l;
            if (o >= n) return 0;
            /* six raw bytes: two of look-back (0xff in front of the payload) and this lane's dword (the arena is zero-padded to a
             * dword behind the payload: at worst a false candidate, which only selects the byte-wise path for this block) */
            const uint32_t cur = gload32((const gu8 *)(src + o)), prev = o ? gload32((const gu8 *)(src + o - 4)) : 0xffffffffu;
            const uint64_t w = ((uint64_t)cur << 16) | (uint64_t)(prev >> 16);
            int hit = 0;
            for (int k = 0; k < 4; k++)
                if (((w >> (8*k)) & 0xffffu) == 0 && ((w >> (8*(k + 2))) & 0xffu) <= 3u) hit = 1;
            return hit;
        });
        if (!cand)
        {
            /* no escape can fire inside this block: whole-wave copy, shifted by the escapes so far */
            if (4u + base + esc + len > cap) { overflow = 1; return 0; }
            WAVE_FOR(l)
            {
                const uint32_t o = 4u*(uint32_t)l;
                if (o < len)
                {
                    GLOBAL_AS uint8_t *d = dst + 4u + base + esc + o;
                    if (o + 4u <= len) gstore32((gu8 *)d, gload32((const gu8 *)(src + base + o)));
                    else for (uint32_t k = o; k < len; k++) dst[4u + base + esc + k] = src[base + k];
                }
            }
            /* zero count behind a block without escapes = its trailing raw zeros (at most 2, else it had a candidate) */
            {
                const uint32_t e = base + len;
                cntz = src[e - 1] ? 0 : (e >= 2 && src[e - 2] == 0) ? 2 : 1;
            }
        } else
        {
            if (4u + base + esc + len + len/2 + 2u > cap) { overflow = 1; return 0; }
            if (wave_lane() == 0)
            {
                uint32_t j = 4u + base + esc;
                for (uint32_t i = 0; i < len; i++)
                {
                    const uint8_t b = src[base + i];
                    if (cntz == 2 && b <= 3) { dst[j++] = 3; cntz = 0; esc++; }
                    cntz = b ? 0 : cntz + 1;
                    dst[j++] = b;
                }
            }
            esc = (uint32_t)uni((int)esc);       /* lane 0 ran the automaton: its counters are the wave's */
            cntz = uni(cntz);
        }
        wave_sync();
    }
    return 4u + n + esc;
}

/* finished frame -> every slice as a complete Annex-B NAL (start code + escaped payload) in the slot's device NAL arena, the NALs
 * behind each other at 16-byte aligned offsets; then NALs (when they fit the host-mapped mirror, which is sized for ordinary
 * frames: in_device = 0) and macroblock records to host-mapped memory, 16 bytes per lane per pass.  Returns the NAL sizes. */
DEV void export_frame(const h264e_geom_t &G, const ChainG &C, const h264e_frame_task_t &T, uint32_t *nal_bytes /* [H264E_MAX_SLICES], uniform */, uint32_t &total, int &overflow, int &in_device)
{
    const GLOBAL_AS h264e_frameout_t &F = C.fout[T.frame_slot];
    uint32_t soff = 0, doff = 0;
    overflow = 0;
    for (int k = 0; k < H264E_MAX_SLICES; k++)
    {
        nal_bytes[k] = 0;
        if (k < F.nslices)
        {
            const uint32_t n = F.slice_nbytes[k];
            const uint32_t room = doff < C.nal_cap ? C.nal_cap - doff : 0u;
            const uint32_t w = nal_escape_copy(C.nal_arena + doff, room, C.arena + F.offset + soff, n, overflow);
            nal_bytes[k] = w;
            soff += (n + 15u) & ~15u;
            doff += (w + 15u) & ~15u;
        }
    }
    total = doff;
    in_device = doff > T.host_rbsp_cap;
    if (!in_device)
    {
        drain_stores();                          /* the NAL arena was written by this wave just now */
        wave_sync();
        const uint32_t nw = (doff + 15u) >> 4;
        const GLOBAL_AS u32x4 *src = (const GLOBAL_AS u32x4 *)C.nal_arena;
        GLOBAL_AS u32x4 *dst = (GLOBAL_AS u32x4 *)T.host_rbsp;
        for (uint32_t base = 0; base < nw; base += 64)
        {
            WAVE_FOR(l) { if (base + (uint32_t)l < nw) dst[base + l] = src[base + l]; }
        }
    }
    const uint32_t nr = ((uint32_t)G.nmb*(uint32_t)sizeof(h264e_mbrec_t) + 15u) >> 4;
    const GLOBAL_AS u32x4 *rs = (const GLOBAL_AS u32x4 *)(C.mbrec + (size_t)T.frame_slot*G.nmb);
    GLOBAL_AS u32x4 *rd = (GLOBAL_AS u32x4 *)T.host_mbrec;
    for (uint32_t base = 0; base < nr; base += 64)
    {
        WAVE_FOR(l) { if (base + (uint32_t)l < nr) rd[base + l] = rs[base + l]; }
    }
    wave_sync();
}

/* ------------------------------------------------------------------ the job's finalizer */

/* what a frame's exact walk says: H264E_WALK_* (0 = nothing yet), the first mismatching macroblock, the state to hand on */
struct Verdict { int status, first_bad; mv32 state[2]; };

/* the verdict record, for the frame behind (its flag is the policy's to raise) */
DEV void walkrec_fill(GLOBAL_AS h264e_walkrec_t *w, const Verdict &v) { w->state_out[0] = v.state[0]; w->state_out[1] = v.state[1]; w->status = v.status; w->first_bad = v.first_bad; }

/* the host record (its done word is the policy's to raise): the verdict, and for a frame that stands its result record F and what export_frame said */
DEV void hostdone_fill(GLOBAL_AS h264e_hostdone_t *hd, const Verdict &v, bool stands, const GLOBAL_AS h264e_frameout_t *F = 0,
                       const uint32_t *nal_bytes = 0, uint32_t nal_total = 0, int exp_overflow = 0, int in_device = 0)
{
    if (stands)
    {
        hd->nbytes = nal_total; hd->all_skipped = F->all_skipped;
        hd->nslices = F->nslices; hd->in_device = in_device;
#pragma unroll
        for (int k = 0; k < H264E_MAX_SLICES; k++) hd->slice_nbytes[k] = nal_bytes[k];
        hd->clusters_moved = F->clusters_moved; hd->overflow = F->overflow | exp_overflow; hd->far_reads = F->far_reads;
    }
    hd->walk_status = v.status; hd->first_bad = v.first_bad; hd->state_out[0] = v.state[0]; hd->state_out[1] = v.state[1];
}

/*
 * One wavefront follows its frame ROW BY ROW: a row whose counter says complete is spliced while the rows below it are still being
 * encoded, and walked (exact mv_clusters validation, JobWalk) as soon as the state in front of the frame is known -- the verdict of the
 * frame in front, which usually arrives when this frame is nearly done: the rows completed by then are walked in one go (also while this
 * wave waits for its next row: the frame-to-frame chain of verdicts must carry the walk alone, never a wait or the splice), and the
 * verdict goes out right behind the walk of the last row.  Then the frame's result: the chain slot's record, the export, the host record.
 *
 * The body decides WHAT is walked when and which exit publishes what.  SYNC decides how: every wait, its bound and what runs while it
 * waits, every fence and scope, which lane stores.  Its members:
 *   int  rows_reached()          the optional wait for every row before anything else (G.fz_wait_all): 0, or a row's poison
 *   int  wait_row(r, idle)       row r complete and acquired: 0; the row's poison (< 0: -1 failed or the bound expired, -2 aborted); 1 when
 *                                idle(), called while waiting, says the frame does not stand
 *   bool prev_up()               one relaxed look at the verdict flag of the frame in front
 *   bool wait_prev()             the bounded wait for that flag; false = expired
 *   void acquire_prev()          the acquire in front of reading that verdict
 *   void converge()              this wave's stores drained, its lanes together
 *   void publish_verdict(w)      a filled verdict record goes out: release, drain, flag at agent scope
 *   void before_export()         what this wave and the rows wrote is visible to all its lanes
 *   void publish_host(hd, sign)  a filled host record goes out: release, drain, done = sign * launch id at system scope
 *   void raise_abort()           the launch's abort word
 *   void raise_err()             the launch's error flag
 *   void stamp(id)               phase stamps 32..37 of a -DH264E_STAMPS build
 */
template <class SYNC> DEV void job_finalize(const h264e_geom_t &G, const ChainG &C, const h264e_frame_task_t &T, SYNC sync)
{
    GLOBAL_AS h264e_hostdone_t *hd = (GLOBAL_AS h264e_hostdone_t *)T.host_done;
    GLOBAL_AS h264e_walkrec_t *wout = (GLOBAL_AS h264e_walkrec_t *)T.walk_out;
    const GLOBAL_AS h264e_walkrec_t *wp = (const GLOBAL_AS h264e_walkrec_t *)T.walk_prev;
    const GLOBAL_AS h264e_mbrec_t *rec = C.mbrec + (size_t)T.frame_slot*G.nmb;
    Verdict v = { 0, -1, { T.exact_state[0], T.exact_state[1] } };
    int have_prev = !(T.walk_on_device && T.walk_prev), published = 0;
    JobWalk W;
    W.begin(v.state);
    /* Row-band slices: every slice of every frame starts from the state in front of the STREAM (the parent's state never moves,
     * h264-lab.h:6526), so the walk needs nothing of the frame in front but its status, and only to publish: the chain of verdicts
     * carries no walk at all (it was what bounded an 8-slice stream: one walk of ~0.26 ms per frame, 3830 frames/s) */
    const bool state_fixed = T.nslices > 1;
    /* the verdict of the frame in front has arrived: take its state (or its failure) */
    const auto take_prev = [&]() {
        sync.acquire_prev();
        if (uni(wp->status) != H264E_WALK_OK) v.status = H264E_WALK_VOID;
        else if (!state_fixed) { v.state[0] = (mv32)uni(wp->state_out[0]); v.state[1] = (mv32)uni(wp->state_out[1]); W.begin(v.state); }
        have_prev = 1;
    };
    /* ... or wait for it first; one that never comes voids this frame */
    const auto await_prev = [&]() { if (sync.wait_prev()) take_prev(); else { v.status = H264E_WALK_VOID; have_prev = 1; } };
    /* this frame's verdict, for the frame behind */
    const auto publish_verdict = [&]() {
        sync.converge();
        if (wave_lane() == 0 && wout) { walkrec_fill(wout, v); sync.publish_verdict(wout); }
        published = 1;
    };
    /* rows up to `upto` are complete: walk what the walk may have; behind the last row the verdict goes out.  Returns non-zero
     * when the frame does not stand (mismatch, or void because the frame in front does not) */
    const auto walk_upto = [&](int upto) -> int {
        if (!T.walk_on_device || published) return 0;
        if (!have_prev && sync.prev_up()) take_prev();
        if (!have_prev && !state_fixed) return 0;
        if (!v.status)
        {
            W.rows(G, T, rec, (GLOBAL_AS mv32 *)T.traj_out, upto);
            if (W.next_row < G.nmby) return 0;
            /* walked to the end on the fixed state: the verdict still has to wait for the status of the frame in front */
            if (!have_prev) await_prev();
        }
        if (!v.status)
        {
            W.end(T);
            v.first_bad = W.first_bad;
            v.state[0] = W.s[0]; v.state[1] = W.s[1];
            v.status = v.first_bad >= 0 ? H264E_WALK_BAD : H264E_WALK_OK;
        }
        publish_verdict();
        return v.status != H264E_WALK_OK;
    };
    SpliceOut so;
    int st = G.fz_wait_all ? sync.rows_reached() : 0;
    if (!st) st = splice_frame(G, C, T, so, [&](int, int r) -> int {
        /* while waiting for row r: the rows above it are complete (and acquired) -- is their walk due? */
        const int stop = sync.wait_row(r, [&]() -> int { return r > 0 && walk_upto(r - 1); });
        return stop ? stop : walk_upto(r);
    });
    sync.stamp(32);                 /* followed the frame's rows: waits, the splice of every completed row, the walk once its start state was in */
    if (st >= 0 && T.walk_on_device && !published)
    {
        /* every row is spliced and the state in front of the frame is still out: wait for it, walk the frame in one go */
        if (!have_prev) await_prev();
        sync.stamp(33);             /* waited for the verdict of the frame in front */
        (void)walk_upto(G.nmby - 1);
        sync.stamp(34);             /* the exact walk behind the splice (the frame in front was late) */
    }
    if (st < 0 || (T.walk_on_device && v.status != H264E_WALK_OK))
    {
        /* the frame does not stand: a row of it was stopped or failed (st < 0), or its walk is void or bad */
        if (wave_lane() == 0)
        {
            if (st == -1) sync.raise_err();
            if (st < 0)
            {
                /* the frames behind wait for this verdict: never leave them spinning */
                v.status = H264E_WALK_VOID; v.first_bad = -1;
                if (T.walk_on_device && wout && !published) { walkrec_fill(wout, v); sync.publish_verdict(wout); }
            }
            /* a mismatch stops the whole launch through the abort word (a leaf's concerns nobody but itself) */
            else if (v.status == H264E_WALK_BAD && T.abort_word && !T.walk_quiet) sync.raise_abort();
            if (hd) { hostdone_fill(hd, v, false); sync.publish_host(hd, -1); }
        }
        return;
    }
    finalize_commit(G, C, T, so, (GLOBAL_AS int *)T.stepflags);
    sync.stamp(35);                 /* the last row's splice + the result record */
    if (hd)
    {
        uint32_t nal_bytes[H264E_MAX_SLICES], nal_total = 0;
        int exp_overflow = 0, in_device = 0;
        sync.before_export();
        export_frame(G, C, T, nal_bytes, nal_total, exp_overflow, in_device);
        sync.converge();
        if (wave_lane() == 0) { hostdone_fill(hd, v, true, &C.fout[T.frame_slot], nal_bytes, nal_total, exp_overflow, in_device); sync.publish_host(hd, 1); }
    }
    sync.stamp(36);                 /* NAL escaping + export to host-mapped memory */
    sync.stamp(37);                 /* (a count: frames that stood) */
}

#endif
