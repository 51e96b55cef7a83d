/*
 * enc_row.h -- row driver (row_begin / row_step / row_end), wave64 model.  What follows a frame's rows -- the slice splice, the exact
 * mv_clusters walk, the export -- is the finalizer's: enc_finalize.h.
 *
 * row_step = the reference's mb_encode (h264-lab.h:5724-5812) for macroblock (x, row): neighbour records of
 * the row above come from HBM (written by that row's wavefront), the left neighbour is in LDS.
 */
#ifndef H264E_ENC_ROW_H
#define H264E_ENC_ROW_H

#include "enc_mb.h"

#define GEOM_WIDE 0
#define GEOM_NARROW 1
#define GEOM_INTRA 2

/* the chain's buffers with explicit HBM address spaces (pointers loaded from a struct are generic otherwise: FLAT
 * instructions, and the compiler has to treat what they load as lane-varying) */
struct ChainG
{
    GLOBAL_AS h264e_mbbottom_t *bottom;
    GLOBAL_AS h264e_mbpend_t *pend;
    GLOBAL_AS int *progress;
    GLOBAL_AS uint32_t *rowbits;
    GLOBAL_AS h264e_rowmeta_t *rowmeta;
    GLOBAL_AS h264e_mbrec_t *mbrec;
    GLOBAL_AS uint8_t *arena;
    uint32_t arena_cap;
    GLOBAL_AS uint8_t *nal_arena;
    uint32_t nal_cap;
    GLOBAL_AS uint32_t *cursor;
    GLOBAL_AS h264e_frameout_t *fout;
    GLOBAL_AS int *far_reads;
    unsigned long long *prof;
};
DEV ChainG chain_view(const h264e_chain_dev_t &C)
{
    ChainG g;
    g.bottom = (GLOBAL_AS h264e_mbbottom_t *)C.bottom; g.pend = (GLOBAL_AS h264e_mbpend_t *)C.pend; g.progress = (GLOBAL_AS int *)C.progress;
    g.rowbits = (GLOBAL_AS uint32_t *)C.rowbits; g.rowmeta = (GLOBAL_AS h264e_rowmeta_t *)C.rowmeta;
    g.mbrec = (GLOBAL_AS h264e_mbrec_t *)C.mbrec; g.arena = (GLOBAL_AS uint8_t *)C.arena; g.arena_cap = C.arena_cap; g.nal_arena = (GLOBAL_AS uint8_t *)C.nal_arena; g.nal_cap = C.nal_cap;
    g.cursor = (GLOBAL_AS uint32_t *)C.cursor; g.fout = (GLOBAL_AS h264e_frameout_t *)C.fout; g.far_reads = (GLOBAL_AS int *)C.far_reads; g.prof = C.prof;
    return g;
}

DEV void row_begin(RowLds &L, const h264e_geom_t &G, const ChainG &C, const h264e_frame_task_t &T, int row)
{
    WAVE_FOR(l)
    {
        if (l < 4) { L.mv_left[l] = 0; L.mv_tl[l] = 0; L.i4_left[l] = -1; L.pix_tl[l] = 0; }
        if (l < 8) L.nnz_left[l] = NNZ_NA;
        if (l < 32) L.pix_left[l] = 0;
        if (l < 25) L.df_mv[l] = 0;
        L.strip_y[l] = 0;
        L.strip_c[l >> 5][l & 31] = 0;
    }
    L.df_nzflag = 0;
    L.left_type = 0;
    L.left_qp = T.qp;
    L.bw.acc = 0; L.bw.nacc = 0; L.bw.pos = 0; L.bw.overflow = 0;
    L.bw.cap = (uint32_t)G.row_words;
    L.bw.buf = C.rowbits + (size_t)row*G.row_words;
    L.skip_run = 0; L.lead_skips = 0; L.coded_any = 0; L.far_reads[0] = L.far_reads[1] = L.far_reads[2] = 0; L.far_fail[0] = L.far_fail[1] = L.far_fail[2] = 0;
    L.f_noskip = L.f_bound = L.f_inter = L.f_decided = L.f_wdone = L.f_stop = 0; L.early_bound = 0; L.f_t3req = L.f_t3done = L.f_front = 0;
    WAVE_FOR(l) { if (l <= H264E_MAX_SLICES) L.slice_row[l] = l <= T.nslices ? T.slice_row[l] : (int16_t)0x7fff; }
    WAVE_FOR(l)
    {
        for (int k = l; k < 84; k += 64) L.qdat[k/42][k%42] = T.qdat[k/42][k%42];
    }
    cavlc_tab_load(L.cavlc);
    df_tab_load(L.dftab);
    L.qconst[0] = k_lambda_mv_q4[T.qp]; L.qconst[1] = k_lambda_q4[T.qp]; L.qconst[2] = k_skip_thr_inter[T.qp];
    L.qconst[3] = k_skip_thr_i4x4[T.qp]; L.qconst[4] = k_lambda_i4_q4[T.qp]; L.qconst[5] = k_lambda_i16_q4[T.qp];
    L.win_x = -2;
#ifdef H264E_STAMPS
    for (int i = 0; i < 32; i++) L.prof[0][i] = L.prof[1][i] = L.prof[2][i] = L.prof[3][i] = 0;
    L.prof_last[0] = L.prof_last[1] = 0;
#endif
    PROF_ROW_BEGIN(L);
    wave_sync();
    PROF_ROW_SYNC(L);
}

/* neighbour record of the macroblock above -> LDS (h264-lab.h:742-745 contexts, :590-606 deblock state): 16 coherent dword
 * loads of the record (+2 of the record to its right), staged in LDS, then unpacked */
/* part: LOAD_TOP_ALL, or -- two waves per row -- LOAD_TOP_MV for the search wave (the vectors of the macroblock above and of the one to its
 * right: all the search needs, and available as soon as the row above has DECIDED them, h264e_kernels.hip) and LOAD_TOP_REST for the
 * reconstruction wave (samples, contexts, pending lines: what the row above writes at the end of its macroblock) */
#define LOAD_TOP_ALL 0
#define LOAD_TOP_MV 1
#define LOAD_TOP_REST 2
template <int PART> DEV void load_top(RowLds &L, MbBuf &B, const h264e_geom_t &G, const GLOBAL_AS h264e_mbbottom_t *above, const GLOBAL_AS h264e_mbpend_t *pend_above, int x, int have_top)
{
    if (PART == LOAD_TOP_MV)
    {
        WAVE_FOR(l)
        {
            if (l < 4) B.mv_top[l] = have_top ? (mv32)cload32((const gu8 *)(above + x) + 32 + 4*l) : 0;
            else if (l == 4) B.mv_top[4] = (have_top && x + 1 < G.nmbx) ? (mv32)cload32((const gu8 *)(above + x + 1) + 32) : 0;
        }
        wave_sync();
        return;
    }
    if (have_top)
    {
        WAVE_FOR(l)
        {
            if (l < 16) lds32_store(L.trec + 4*l, cload32((const gu8 *)(above + x) + 4*l));
            else if (l == 16) lds32_store(L.trec + 64, x + 1 < G.nmbx ? cload32((const gu8 *)(above + x + 1)) : 0u);                /* pix[0..3] of the above-right record */
            else if (l == 17) lds32_store(L.trec + 68, x + 1 < G.nmbx ? cload32((const gu8 *)(above + x + 1) + 32) : 0u);           /* its mv[0] */
            else if (l >= 32 && l < 56) lds32_store(B.ptop + 4*(l - 32), cload32((const gu8 *)(pend_above + x) + 4*(l - 32)));    /* for the deblocking at the end of the step */
        }
        wave_sync();
        WAVE_FOR(l)
        {
            if (l < 8) lds32_store(B.pix_top + 4*l, lds32(L.trec + 4*l));
            else if (l < 12) { if (PART == LOAD_TOP_ALL) B.mv_top[l - 8] = (mv32)lds32(L.trec + 32 + 4*(l - 8)); }
            else if (l < 20) B.nnz_top[l - 12] = L.trec[48 + l - 12];
            else if (l < 24) B.i4_top[l - 20] = (int8_t)L.trec[56 + l - 20];
            else if (l == 24) { B.df_nz_top = L.trec[60]; B.top_type = (int8_t)L.trec[61]; B.top_qp = L.trec[62]; }
            else if (l == 25) lds32_store(B.pix_top + 32, lds32(L.trec + 64));
            else if (l == 26) { if (PART == LOAD_TOP_ALL) B.mv_top[4] = (mv32)lds32(L.trec + 68); }
        }
    } else
    {
        WAVE_FOR(l)
        {
            if (l < 36) B.pix_top[l] = 0;
            if (l < 5 && PART == LOAD_TOP_ALL) B.mv_top[l] = 0;
            if (l < 8) B.nnz_top[l] = NNZ_NA;
            if (l < 4) B.i4_top[l] = -1;
            if (l == 0) { B.df_nz_top = 0; B.top_type = 0; B.top_qp = 0; }
        }
    }
    wave_sync();
}

/* h264-lab.h:5731-5740 + 3536-3562: input macroblock -> LDS, replicating the last valid column / row of cropped pictures */
DEV void load_input(MbBuf &B, const h264e_geom_t &G, const RowTask &T, int mbx, int mby)
{
    /* a macroblock that lies inside the picture (all but the last column / row of a cropped picture) is 96 dword loads; only the
     * cropped edge replicates sample by sample */
    const bool inside = (mbx + 1)*16 <= G.width && (mby + 1)*16 <= G.height;
    WAVE_FOR(l)
    {
        {
            int r = l >> 2, c = l & 3, yy = imin(mby*16 + r, G.height - 1);
            const gu8 *p = (const gu8 *)T.in[0] + (size_t)yy*T.in_stride[0];
            uint32_t v = 0;
            if (inside) v = gload32(p + mbx*16 + 4*c);
            else for (int k = 0; k < 4; k++) v |= (uint32_t)p[imin(mbx*16 + 4*c + k, G.width - 1)] << (8*k);
            lds32_store(B.inp + 16*r + 4*c, v);
        }
        if (l < 32)
        {
            int pl = l >> 4, r = (l >> 1) & 7, c = l & 1, yy = imin(mby*8 + r, G.height/2 - 1);
            /* (selected, not indexed: a lane-varying index would put the task copy into scratch memory) */
            const gu8 *p = (const gu8 *)(pl ? T.in[2] : T.in[1]) + (size_t)yy*(pl ? T.in_stride[2] : T.in_stride[1]);
            uint32_t v = 0;
            if (inside) v = gload32(p + mbx*8 + 4*c);
            else for (int k = 0; k < 4; k++) v |= (uint32_t)p[imin(mbx*8 + 4*c + k, G.width/2 - 1)] << (8*k);
            lds32_store(B.inp_c + 16*r + 8*pl + 4*c, v);
        }
    }
    wave_sync();
}

/* What macroblock (x, row) needs that does not depend on the row above: its input samples and, for P slices, the
 * reference window (the caller has waited for the temporal dependency).  Issued BEFORE the wait for the row above, so
 * the HBM latency of these loads overlaps with that wait.
 * The window SLIDES (enc_kernels.h wave_slide_window: one strip of 16 new columns instead of the whole window) when the window of
 * x - 1 is what this workgroup loaded last (L.win_x: never for the first macroblock a workgroup encodes, wherever its row starts) and
 * both windows lie inside the picture's columns; otherwise -- at the left and right border with their clamped loads, in pictures
 * narrower than the window -- it is loaded whole. */
template <int GEOM> DEV void row_prefetch(RowLds &L, const h264e_geom_t &G, const RowTask &T, int row, int x)
{
    load_input(L.mb[x & 1], G, T, x, row);
    if (GEOM != GEOM_INTRA && T.slice_type == 0)
    {
        Plane P;
        P.p = (const gu8 *)T.ref[0]; P.w = G.W; P.h = G.H; P.stride = G.W;
        const int wx0 = x*16 - WIN_M;
        if (uni(L.win_x) == x - 1 && wx0 - 16 >= 0 && wx0 + WIN_W <= P.w) wave_slide_window<GEOM == GEOM_NARROW>(L.win, P, wx0, row*16 - WIN_M);
        else wave_load_window(L.win, P, wx0, row*16 - WIN_M, T.narrow);
        L.win_x = x;
    }
}

/*
 * One macroblock = three phases (the reference's mb_encode, h264-lab.h:5724-5812, cut where its data flow allows two instruction streams):
 *   mb_search        neighbour records of the row above -> LDS, inter decision (H:5283-5524)                     [search side]
 *   mb_intra_decide  intra 16x16 / 4x4 candidates (H:5748-5762), the final decision, contexts for the next one   [reconstruction side]
 *   mb_recon_write   chroma prediction, mb_write (H:4378-4715), deblocking (H:5535-5716), stores                 [reconstruction side]
 * The search of macroblock x + 1 needs nothing of x but the predictor context that mb_intra_decide leaves behind, and the intra
 * candidates of x + 1 need the reconstruction of x (left column) -- so with two wavefronts per row (h264e_kernels.hip) the search
 * wave works on x + 1 while the reconstruction wave writes x, then tests the intra candidates of x + 1.  With one wavefront (and in
 * the emulation) the three run one after the other; the decisions are the same either way.
 * GEOM: compile-time kernel variant -- GEOM_WIDE / GEOM_NARROW = the reference-window geometry (h264e_dev.h); GEOM_INTRA = a launch of
 * intra frames only: the inter decision, the reference window and the inter chroma prediction are compiled out (and with them most of
 * the register pressure: that variant runs at twice the waves per SIMD).
 * row0 / row1: first row and end row of the slice (row band) this row belongs to -- the whole picture for one slice per frame.
 * A slice is encoded like a picture of its own as far as neighbour availability, contexts and deblocking are concerned
 * (h264-lab.h:3605-3622 mb_avail_flag relative to slice.start_mb_num, h264-lab.h:5799-5808 no filtering across its top edge).
 */
template <int GEOM> DEV void mb_ctx_init(MbCtx &m, RowLds &L, const h264e_geom_t &G, const RowTask &T, int row, int x, int row0, int side)
{
    const bool have_top = row > row0;
    m.G = &G;
    m.speed = T.speed; m.slice_type = T.slice_type; m.clu[0] = T.clusters[0]; m.clu[1] = T.clusters[1]; m.clu_per_mb = T.clusters_per_mb;
    for (int c = 0; c < 3; c++)
    {
        m.ref[c].p = (const gu8 *)T.ref[c];
        m.ref[c].w = G.W >> (c ? 1 : 0); m.ref[c].h = G.H >> (c ? 1 : 0); m.ref[c].stride = m.ref[c].w;
        m.dec[c] = (gu8 *)T.dec[c];
    }
    m.x = x; m.y = row; m.num = row*G.nmbx + x;
    m.avail = (have_top ? AV_T : 0) | (have_top && x != G.nmbx - 1 ? AV_TR : 0) | (x > 0 ? AV_L : 0) | (have_top && x > 0 ? AV_TL : 0);
    m.slice_top = !have_top;
    m.cropped = G.cropping && ((x + 1)*16 > G.width || (row + 1)*16 > G.height);
    m.type = 0; m.cost = 0x7FFFFFFF; m.i16_mode = 0; m.used_cand = 0; m.mv_skip_pred = 0; m.nz_mask = 0;
    m.qp = T.qp;
    m.lambda_mv = uni(L.qconst[0]); m.lambda_q4 = uni(L.qconst[1]); m.skip_thr = uni(L.qconst[2]);
    m.skip_thr_i4 = uni(L.qconst[3]); m.lambda_i4 = uni(L.qconst[4]); m.lambda_i16 = uni(L.qconst[5]);
    m.rv.dep = (const GLOBAL_AS int *)T.dep_progress; m.rv.nmbx = G.nmbx; m.rv.nmby = G.nmby;
    m.rv.P = m.ref[0]; m.rv.win = (const lu8 *)L.win + win_org(x*16 - WIN_M); m.rv.has_win = GEOM != GEOM_INTRA && T.slice_type == 0; m.rv.wx0 = x*16 - WIN_M; m.rv.wy0 = row*16 - WIN_M;
    m.rv.vw = GEOM == GEOM_NARROW ? H264E_NARROW_VW : WIN_W; m.rv.vh = GEOM == GEOM_NARROW ? H264E_NARROW_VH : WIN_W; m.rv.far = &L.far_reads[side]; m.rv.fail = &L.far_fail[side]; m.rv.slice_row = L.slice_row; m.rv.nslices = T.nslices; m.rv.spin_limit = G.spin_limit;
}

/* search side.  The input macroblock, the reference window (row_prefetch) and the records of the row above (load_top) are already in
 * LDS.  sig (inter_choose): sig.noskip() is called once the
 * early-skip test has failed (the reconstruction side may start on the intra candidates then). */
struct NoSignals { DEVM void noskip() const {} DEVM void bound(int) const {} DEVM bool helper() const { return false; } DEVM void t3_request(mv32, int, const rect_t &) const {} DEVM bool t3_wait() const { return true; } };
template <int GEOM, class SIG> DEV void mb_search(RowLds &L, MbBuf &B, const h264e_geom_t &G, const RowTask &T, int row, int x, int row0, SIG sig)
{
    MbCtx m;
    mb_ctx_init<GEOM>(m, L, G, T, row, x, row0, 0);
    STAMP(L, 1);
    if (GEOM != GEOM_INTRA && T.slice_type == 0) inter_choose(L, B, m, sig);
    STAMP(L, 7);
    B.type = m.type; B.cost = m.cost; B.used_cand = m.used_cand; B.mv_skip_pred = m.mv_skip_pred;
    wave_sync();
}

/* How the reconstruction side learns about the inter decision: it is simply there (one wavefront, emulation) ... */
struct InterIsThere
{
    DEVM bool ready() const { return true; }
    DEVM bool wait_noskip_or_ready() const { return true; }
    DEVM bool wait_bound_or_ready() const { return true; }
    DEVM bool wait_ready() const { return true; }
    DEVM int early_bound() const { return 0x7fffffff; }
    DEVM bool before_decide() const { return true; }
};

/* reconstruction side, first half: the intra candidates and the final decision.  The intra candidates do not need the inter decision
 * -- only the comparison at the end does -- so with a search wave still at work (P.ready() false) they start as soon as the early-skip
 * test has failed, bounded by the 16x16 intra cost until the inter cost arrives.  Returns false when the row has to stop. */
template <class P> DEV bool mb_intra_decide(RowLds &L, MbBuf &B, MbCtx &m, const RowTask &T, P pol)
{
    bool have = pol.ready();
    if (!have)
    {
        if (!pol.wait_noskip_or_ready()) return false;
        have = pol.ready();
    }
    STAMP(L, 15);               /* two waves: waited for the search wave's early-skip test */
    if (have) { m.type = uni(B.type); m.cost = uni(B.cost); }
    if (m.type >= 0)
    {
        const int cost16 = intra16_cost(L, B, m);
        STAMP(L, 8);
        int cost4 = I4_LOST, bnd = imin(m.cost, cost16);
        unsigned nz4 = 0;
        /* the 4x4 candidates cost three times the 16x16 one and lose against most inter decisions after a few blocks -- once there is a
         * bound to lose against: wait for the search wave's first one (it follows the early-skip test by one candidate scan) */
        if (!have && !pol.wait_bound_or_ready()) return false;
#ifdef H264E_ABLATE
        if (H264E_ABLATE != 2)
#endif
        if (T.speed < 2 || T.slice_type != 0)
            cost4 = intra4_choose(L, B, m, [&]() -> int {
                if (!have)
                {
                    if (pol.ready()) { have = true; bnd = imin(bnd, uni(B.cost)); }
                    else bnd = imin(bnd, pol.early_bound());         /* the search wave's upper bound of the inter cost, once it has one */
                }
                return bnd;
            }, nz4);
        STAMP(L, 9);
        if (!pol.wait_ready()) return false;
        STAMP(L, 16);           /* two waves: waited for the inter decision */
        m.type = uni(B.type); m.cost = uni(B.cost);
        if (!pol.before_decide()) return false;
        if (m.type >= 0) intra_merge(L, B, m, cost16, cost4, nz4);
    } else if (!pol.before_decide()) return false;
    m.used_cand = uni(B.used_cand); m.mv_skip_pred = (mv32)uni(B.mv_skip_pred);
    mb_decide(L, B, m);
    return true;
}

/* reconstruction side, second half */
struct NoHook { DEVM void operator()() const {} };
/* ... in two parts, because a fourth wave can take the second one (h264e_kernels.hip, the latency variant): mb_recon_front = chroma
 * prediction, mb_write, the validation record, the unfiltered edges the next macroblock's intra prediction needs; mb_recon_back =
 * deblocking and every store of the macroblock (picture, pending lines, the record for the row below) -- nothing the front part of the
 * NEXT macroblock needs before its mb_decide */
template <int GEOM, class HOOK> DEV void mb_recon_front(RowLds &L, MbBuf &B, MbCtx &m, const h264e_geom_t &G, const ChainG &C, const RowTask &T, int row, int x, int row0, int row1, HOOK after_prediction)
{
    if (GEOM == GEOM_INTRA || m.type >= 5) wave_pred_chroma(L.pred_c, L.pix_left + 16, B.pix_top + 16, m.avail, m.i16_mode);
    else predict_chroma_inter(B, m, L.pred_c);
    after_prediction();             /* two waves per row: the `decided` counter (h264e_kernels.hip) */

    STAMP(L, 10);
    BitW bw = bw_uniform(L.bw);
    mb_write(L, B, m, bw);
    L.bw = bw;
    STAMP(L, 11);

    /* record for the mv_clusters validation (h264-lab.h:5776-5779 updates them with mv[0] of every non-intra MB) */
    {
        GLOBAL_AS h264e_mbrec_t *rec = C.mbrec + (size_t)T.frame_slot*G.nmb + m.num;
        const uint32_t mv0 = m.type < 5 ? (uint32_t)B.mv[0] : 0u;
        const uint64_t w = (uint64_t)mv0 | ((uint64_t)(uint8_t)(int8_t)m.type << 32) | ((uint64_t)(m.used_cand & 255) << 40);
        cstore64((gu8 *)rec, w);                /* (every lane the same word: no divergent branch, see enc_kernels.h bw_put) */
    }

    /* keep the UNFILTERED right column / bottom row for intra prediction (h264-lab.h:4693-4714) */
    uint8_t *ty = L.ytile + 4*YT_STRIDE + 4;
    uint8_t *tc0 = L.ctile[0] + 2*CT_STRIDE + 2, *tc1 = L.ctile[1] + 2*CT_STRIDE + 2;
    /* the record for the row below is assembled in LDS (L.brec) and stored at the end of the step */
    WAVE_FOR(l)
    {
        if (l < 16)
        {
            L.pix_left[l] = ty[YT_STRIDE*l + 15];
            L.brec[l] = ty[YT_STRIDE*15 + l];
        } else if (l < 32)
        {
            int pl = (l >> 3) & 1, i = l & 7;
            const uint8_t *t = pl ? tc1 : tc0;
            L.pix_left[16 + 8*pl + i] = t[CT_STRIDE*i + 7];
            L.brec[16 + 8*pl + i] = t[CT_STRIDE*7 + i];
        } else if (l < 35)
        {
            int c = l - 32;
            L.pix_tl[c] = B.pix_top[c == 0 ? 15 : 15 + 8*c];
        }
    }
    wave_sync();

}

template <int GEOM> DEV void mb_recon_back(RowLds &L, MbBuf &B, MbCtx &m, const h264e_geom_t &G, const ChainG &C, const RowTask &T, int row, int x, int row0, int row1)
{
    const bool have_top = row > row0;
    GLOBAL_AS h264e_mbbottom_t *rowrec = C.bottom + (size_t)row*G.nmbx;
    uint8_t *ty = L.ytile + 4*YT_STRIDE + 4;
    uint8_t *tc0 = L.ctile[0] + 2*CT_STRIDE + 2, *tc1 = L.ctile[1] + 2*CT_STRIDE + 2;
    /* deblock on the LDS tiles: left strips from LDS (previous macroblock), top strips from the pending lines of the
     * row above (h264e_mbpend_t) */
    const int W = G.W, Wc = G.W >> 1;
    gu8 *dy = m.dec[0] + (size_t)(row*16)*W + x*16;
    gu8 *du = m.dec[1] + (size_t)(row*8)*Wc + x*8, *dv = m.dec[2] + (size_t)(row*8)*Wc + x*8;
    GLOBAL_AS h264e_mbpend_t *pend_row = C.pend + (size_t)row*G.nmbx;
    const bool direct = T.no_deblock || row == row1 - 1;        /* nothing below will filter the bottom lines (picture or slice end): they are final now */
    if (!T.no_deblock)
    {
        df_strength(L, m, B.top_type);
        WAVE_FOR(l)
        {
            if (l < 16) lds32_store(L.ytile + (4 + l)*YT_STRIDE, lds32(L.strip_y + 4*l));
            else if (l < 32)
            {
                int pl = (l >> 3) & 1, i = l & 7;
                uint8_t *t = L.ctile[pl] + (2 + i)*CT_STRIDE;
                t[0] = L.strip_c[pl][4*i + 2]; t[1] = L.strip_c[pl][4*i + 3];
            } else if (l < 48)
            {
                int r = (l - 32) >> 2, c = l & 3;
                uint32_t v = 0;
                if (have_top) v = lds32(B.ptop + 16*r + 4*c);
                lds32_store(L.ytile + r*YT_STRIDE + 4 + 4*c, v);
            } else if (l < 56)
            {
                int pl = (l >> 2) & 1, r = (l >> 1) & 1, c = l & 1;
                uint32_t v = 0;
                if (have_top) v = lds32(B.ptop + 64 + 16*pl + 8*r + 4*c);
                memcpy(L.ctile[pl] + r*CT_STRIDE + 2 + 4*c, &v, 4);
            }
        }
        wave_sync();
        wave_deblock(L.ytile, L.ctile[0], L.ctile[1], L.bs, T.qp, L.left_qp, B.top_qp, L.dftab);
    }
    /* write the macroblock: final lines into the picture, the bottom lines into the pending record; 8 bytes per lane (every
     * store is one write-through fabric request, whatever its width) */
    WAVE_FOR(l)
    {
        if (l < 32)
        {
            const int r = l >> 1, hf = l & 1;
            const uint64_t v = (uint64_t)lds32(ty + YT_STRIDE*r + 8*hf) | ((uint64_t)lds32(ty + YT_STRIDE*r + 8*hf + 4) << 32);
            if (r < 12 || direct) cstore64(dy + (size_t)r*W + 8*hf, v);
            else cstore64((gu8 *)pend_row[x].y + 16*(r - 12) + 8*hf, v);
        } else if (l < 48)
        {
            const int pl = (l - 32) >> 3, rr = l & 7;
            const uint8_t *t = (pl ? tc1 : tc0) + CT_STRIDE*rr;
            const uint64_t u = (uint64_t)lds32(t) | ((uint64_t)lds32(t + 4) << 32);
            if (rr < 6 || direct) cstore64((pl ? dv : du) + (size_t)rr*Wc, u);
            else cstore64((gu8 *)pend_row[x].c[pl] + 8*(rr - 6), u);
        }
    }
    if (!T.no_deblock)
    {
        /* the neighbour samples the filter changed: 3 luma / 1 chroma columns of the left macroblock (picture, or its pending
         * record for the bottom lines) -- unless the left edge was not filtered at all (strength 0 on all of it: two skipped
         * macroblocks side by side), then what the left macroblock stored itself stands -- and the 4 luma / 2 chroma lines above,
         * which are final now */
        const bool left_filtered = x > 0 && uni(lds32(L.bs)) != 0;
        WAVE_FOR(l)
        {
            if (l < 16)
            {
                if (left_filtered)
                {
                    uint32_t v = lds32(L.ytile + (4 + l)*YT_STRIDE);
                    if (l < 12 || direct) cstore32(dy + (size_t)l*W - 4, v);
                    else cstore32((gu8 *)pend_row[x - 1].y + 16*(l - 12) + 12, v);
                }
            } else if (l < 24)
            {
                int r = (l - 16) >> 1, hf = l & 1;                          /* tile rows 0..3 = picture rows -4..-1 */
                if (have_top)
                {
                    const uint8_t *t = L.ytile + r*YT_STRIDE + 4 + 8*hf;
                    cstore64(dy - (size_t)(4 - r)*W + 8*hf, (uint64_t)lds32(t) | ((uint64_t)lds32(t + 4) << 32));
                }
            } else if (l < 32)
            {
            } else if (l < 48)
            {
                int pl = (l - 32) >> 3, i = (l - 32) & 7;
                if (left_filtered)
                {
                    /* columns 4..7 of the left macroblock as one dword: 4..6 as it left them, 7 as this filter left it */
                    const uint32_t v = (uint32_t)L.strip_c[pl][4*i] | ((uint32_t)L.strip_c[pl][4*i + 1] << 8) | ((uint32_t)L.strip_c[pl][4*i + 2] << 16) |
                                       ((uint32_t)L.ctile[pl][(2 + i)*CT_STRIDE + 1] << 24);
                    if (i < 6 || direct) cstore32((pl ? dv : du) + (size_t)i*Wc - 4, v);
                    else cstore32((gu8 *)pend_row[x - 1].c[pl] + 8*(i - 6) + 4, v);
                }
            } else if (l < 52)
            {
                int pl = (l - 48) >> 1, r = l & 1;                          /* tile rows 0..1 = picture rows -2..-1 */
                if (have_top)
                {
                    uint32_t lo, hi;
                    memcpy(&lo, L.ctile[pl] + r*CT_STRIDE + 2, 4); memcpy(&hi, L.ctile[pl] + r*CT_STRIDE + 6, 4);
                    cstore64((pl ? dv : du) - (size_t)(2 - r)*Wc, (uint64_t)lo | ((uint64_t)hi << 32));
                }
            }
        }
    }
    /* carried deblock state: deblocked right columns of this macroblock; rest of the record for the row below */
    WAVE_FOR(l)
    {
        if (l < 16) lds32_store(L.strip_y + 4*l, lds32(ty + YT_STRIDE*l + 12));
        else if (l < 32)
        {
            int pl = (l >> 3) & 1, i = l & 7;
            const uint8_t *t = (pl ? tc1 : tc0) + CT_STRIDE*i + 4;
            L.strip_c[pl][4*i] = t[0]; L.strip_c[pl][4*i + 1] = t[1]; L.strip_c[pl][4*i + 2] = t[2]; L.strip_c[pl][4*i + 3] = t[3];
        } else if (l < 36) lds32_store(L.brec + 32 + 4*(l - 32), (uint32_t)B.mv_top[l - 32]);
        else if (l < 44) L.brec[48 + l - 36] = B.nnz_top[l - 36];
        else if (l < 48) L.brec[56 + l - 44] = (uint8_t)B.i4_top[l - 44];
        else if (l == 48)
        {
            L.brec[60] = (uint8_t)(L.df_nzflag >> 20);
            L.brec[61] = (uint8_t)(int8_t)m.type;
            L.brec[62] = (uint8_t)T.qp;
            L.brec[63] = 0;
        }
    }
    wave_sync();
    WAVE_FOR(l) { if (l < 16) cstore32((gu8 *)(rowrec + x) + 4*l, lds32(L.brec + 4*l)); }
    L.left_type = m.type;
    L.left_qp = T.qp;
    wave_sync();
    STAMP(L, 12);
#ifndef H264E_TYPES_PROBE
    PCOUNT(L, 20 + (m.type < 0 ? 0 : m.type < 5 ? 1 : 2));
#endif
}

template <int GEOM, class HOOK> DEV void mb_recon_write(RowLds &L, MbBuf &B, MbCtx &m, const h264e_geom_t &G, const ChainG &C, const RowTask &T, int row, int x, int row0, int row1, HOOK after_prediction)
{
    mb_recon_front<GEOM>(L, B, m, G, C, T, row, x, row0, row1, after_prediction);
    mb_recon_back<GEOM>(L, B, m, G, C, T, row, x, row0, row1);
}

/* the three phases one after the other: one wavefront per row, and the emulation */
template <int GEOM> DEV void row_step(RowLds &L, const h264e_geom_t &G, const ChainG &C, const RowTask &T, int row, int x, int row0, int row1)
{
    MbBuf &B = L.mb[x & 1];
    MbCtx m;
    load_top<LOAD_TOP_ALL>(L, B, G, C.bottom + (size_t)(row - 1)*G.nmbx, C.pend + (size_t)(row - 1)*G.nmbx, x, row > row0);
    mb_search<GEOM>(L, B, G, T, row, x, row0, NoSignals());
    mb_ctx_init<GEOM>(m, L, G, T, row, x, row0, 1);
    mb_intra_decide(L, B, m, T, InterIsThere());
    mb_recon_write<GEOM>(L, B, m, G, C, T, row, x, row0, row1, NoHook{});
}

DEV void row_end(RowLds &L, const h264e_geom_t &G, const ChainG &C, int row)
{
    BitW bw = bw_uniform(L.bw);
    const uint32_t nbits = bw_bits(bw);
    if (bw.nacc)
    {
        const int pad = 32 - bw.nacc;
        bw_put(bw, pad, 0);
    }
    gu8 *M = (gu8 *)(C.rowmeta + row);       /* {nbits, lead_skips, trail_skips, overflow}: read by the finalizer workgroup */
    if (wave_lane() == 0)
    {
        g_atomic_store(C.far_reads + row, L.far_reads[0] + L.far_reads[1] + L.far_reads[2]);      /* stays with the row, like its bits, when the frame goes again from a lower one */
        cstore32(M, nbits);
        cstore32(M + 4, (uint32_t)(L.coded_any ? L.lead_skips : G.nmbx));
        cstore32(M + 8, (uint32_t)(L.coded_any ? L.skip_run : 0));
        cstore32(M + 12, (uint32_t)bw.overflow);
    }
    wave_sync();
    PROF_ROW_END(L, C);
}

#endif
