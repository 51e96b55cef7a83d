/*
 * enc_selftest.h -- device-level code that only tests and the bench input use: the per-stage test hook (one wave-level stage of the
 * macroblock pipeline on caller-supplied operands), the finalizer test hook and the synth_v1 clip generator.  Wave64 model like the rest (wave.h).
 * Not here: the hand-offs between the waves of a row (what the reconstruction wave knows of the inter decision, and when) -- their arrival
 * orders are scripted in the emulation, tests/emu/emu_handoffs.h, and tested by tests/test_emu_handoffs.py and tests/test_gpu_handoffs.py.
 */
#ifndef H264E_ENC_SELFTEST_H
#define H264E_ENC_SELFTEST_H
#include "enc_row.h"
#include "enc_finalize.h"

/* ------------------------------------------------------------------ per-stage test hook (tests/test_stages.py, tests/test_stage_edges.py)
 * Runs ONE of the macroblock pipeline's wave-level stages on caller-supplied operands, so that each can be compared with the
 * reference's own function of the same stage (tests/golden/stages.json and stage_edges.json, made by oracle/stage_harness.c):
 *   1 SAD quadrants (wave_sad_ref_q)           in: picture 64x64 | block 16x16         args: x, y, window      out: int32 sad4[4], sum
 *   2 luma quarter-sample (wave_interp_luma)   in: picture 64x64                       args: x, y, w, h, dx, dy, window   out: 16x16 (stride 16)
 *   3 chroma bilinear (wave_interp_chroma)     in: picture 64x64 (used as U and V)     args: x, y, w, h, dx, dy           out: 16x16: U cols 0-7, V cols 8-15
 *   4 transform/quant/dequant/recon            in: inp 256 | pred 256 | qdat 42 x u16  args: mode              out: int32 nz, dcflag | qblk_t q[16] | i16 dc[16] | i16 lev[16] | recon 256
 *   5 CAVLC block (cavlc_block)                in: int16 coef[16]                      args: first, maxn, nctx, bits already in the buffer (ones)   out: int32 nnz, nbits | bytes
 *   8 motion search of one partition (diamond)  in: picture 96x96 | macroblock 16x16      args: px, py, w, h, mv x/y, pred x/y, min_sad, qp, speed, range[4], limit[4], window
 *                                                out: int32 cost, mv x, mv y | prediction 16x16 (stride 16)
 *   7 deblock one macroblock (wave_deblock)     in: luma tile 20x24 | U tile 10x12 | V tile 10x12 | bs 32   args: qp, qp_left, qp_top   out: the three tiles
 *   6 intra 4x4 mode choice (wave_i4_choose)   in: edge 13 (L3..L0, UL, U0..U7) | block 4x4 stride 16   args: avail, mpred, penalty   out: int32 mode, cost | prediction 4x4 stride 16
 *   9 intra 16x16 (intra16_cost, wave_pred16)  in: block 16x16 | left 16 | top 16      args: avail, qp         out: int32 mode, cost | prediction 16x16
 *  10 chroma prediction (wave_pred_chroma)     in: left 8 U, 8 V | top 8 U, 8 V        args: avail, mode (luma numbering)   out: 8 rows of U cols 0-7, V cols 8-15
 *  11 vector predictor (mvp_get_arr / _put_arr) in: int32 mv_left[4], mv_tl[4], mv_top[8] | n x (x, y, w, h, mv) in 4x4-block units   args: avail, n
 *                                               out: int32 predictor[16] | the context after the last put, as given
 *  12 boundary strengths (df_strength)         in: int32 df_mv[25]                     args: df_nzflag, left_type, top_type, type, x, slice_top   out: bs 32
 *  13 partition_hints                          in: n x int32 sad[4]                    args: n <= 64           out: n x int32 mode[4]
 *  14 mv_cost                                  in: n x int32 (mv x, y, pred x, y, qp)  args: n <= 256          out: n x int32 cost
 *  15 bit writer (bw_put, bw_ue, bw_se)        in: n x int32 (kind 0/1/2, value, length)   args: n <= 64       out: int32 nbits, overflow | bytes
 *  16 packed byte average (avg4_u8)            in: none (the 65 536 byte pairs are made on the device)   out: 16 384 dwords, pair n = 256*x + y in byte n
 * `window` = 1 reads the reference samples through the LDS window like the macroblock loop, 0 through the HBM path.
 */
struct StageLds
{
    alignas(16) uint8_t win[WIN_W*WIN_STRIDE + 16];
    alignas(16) uint8_t a[256], b[256], o[256];
    alignas(16) qblk_t q[16];
    alignas(4) int16_t dc[16], lev[16], coef[16];
    alignas(4) uint16_t qdat[42];
    CavlcTab ct;
    I4Scratch i4s;
    DfTab df;
    alignas(16) uint8_t yt[20*YT_STRIDE];
    alignas(16) uint8_t ctile[2][10*CT_STRIDE];
    alignas(4) uint8_t bs[32];
    alignas(4) uint8_t nb[5*24];         /* the block's neighbourhood as intra4_choose keeps it: row stride 24, block at row 1, column 4 */
};
#define STAGE_IN_MAX (96*96 + 256)
#define STAGE_NARGS 24
#define STAGE_OUT_MAX (16 + 16*64 + 32 + 32 + 256)
#define STAGE_AVG4_DWORDS 16384         /* stage 16 alone writes more than STAGE_OUT_MAX: 4 bytes each */
DEV void stage_selftest(StageLds &S, RowLds &L, int stage, const GLOBAL_AS uint8_t *in, const int *args, GLOBAL_AS uint8_t *out)
{
    int a[STAGE_NARGS];
    for (int i = 0; i < STAGE_NARGS; i++) a[i] = uni(args[i]);
    Plane P = { (const gu8 *)in, 64, 64, 64 };
    RefView R;
    R.P = P; R.win = (const lu8 *)S.win; R.has_win = 0; R.wx0 = 0; R.wy0 = 0; R.dep = 0; R.nmbx = 4; R.nmby = 4; R.vw = WIN_W; R.vh = WIN_W;
    R.far = 0; R.fail = 0; R.slice_row = 0; R.nslices = 0; R.spin_limit = 0;
    GLOBAL_AS int32_t *oi = (GLOBAL_AS int32_t *)out;
    if (stage == 1 || stage == 2)
    {
        const int x = a[0], y = a[1], window = stage == 1 ? a[2] : a[6];
        if (window) { R.has_win = 1; R.wx0 = x - WIN_M; R.wy0 = y - WIN_M; R.win = (const lu8 *)S.win + win_org(R.wx0); wave_load_window(S.win, P, R.wx0, R.wy0, 0); wave_sync(); }
        if (stage == 1)
        {
            int s4[4];
            WAVE_FOR(l) { lds32_store(S.b + 4*l, gload32((const gu8 *)in + 4096 + 4*l)); }
            wave_sync();
            const int tot = wave_sad_ref_q(R, x, y, S.b, s4);
            if (wave_lane() == 0) { oi[0] = s4[0]; oi[1] = s4[1]; oi[2] = s4[2]; oi[3] = s4[3]; oi[4] = tot; }
        } else
        {
            WAVE_FOR(l) { lds32_store(S.o + 4*l, 0u); }
            wave_sync();
            wave_interp_luma(R, 0, 0, mvmk(4*x + a[4], 4*y + a[5]), a[2], a[3], S.o);
            wave_sync();
            WAVE_FOR(l) { gstore32((gu8 *)out + 4*l, lds32(S.o + 4*l)); }
        }
    } else if (stage == 3)
    {
        WAVE_FOR(l) { lds32_store(S.o + 4*l, 0u); }
        wave_sync();
        wave_interp_chroma(R, P, P, 0, 0, mvmk(8*a[0] + a[4], 8*a[1] + a[5]), a[2], a[3], S.o);
        wave_sync();
        WAVE_FOR(l) { gstore32((gu8 *)out + 4*l, lds32(S.o + 4*l)); }
    } else if (stage == 4)
    {
        const int mode = a[0], side = mode >> 1;
        WAVE_FOR(l)
        {
            lds32_store(S.a + 4*l, gload32((const gu8 *)in + 4*l));
            lds32_store(S.b + 4*l, gload32((const gu8 *)in + 256 + 4*l));
            if (l < 21) lds32_store((uint8_t *)S.qdat + 4*l, gload32((const gu8 *)in + 512 + 4*l));
            if (l < 8) { lds32_store((uint8_t *)S.dc + 4*l, 0u); lds32_store((uint8_t *)S.lev + 4*l, 0u); }
            for (int k = l; k < 256; k += 64) lds32_store((uint8_t *)S.q + 4*k, 0u);
        }
        wave_sync();
        /* the product's paths: mb_write's fused pass (transform -> dead zone -> quantiser -> DC path -> reconstruction) for the inter, intra 16x16
         * and chroma modes, intra4_choose's block coder for the intra 4x4 mode; q (levels + dequantised coefficients), the DC levels and the
         * reconstruction are what the reference's functions leave (h264-lab.h:2619-2681, 4428-4433, 4468-4488, 4809-4811) */
        unsigned nz = 0;
        int dcflag = 0;
        WAVE_FOR(l) { lds32_store(S.o + 4*l, lds32(S.b + 4*l)); }
        wave_sync();
        if (mode == QMODE_INTER) nz = wave_xform_quant_recon<QMODE_INTER>(S.a, S.b, S.o, 16, S.q, S.dc, S.lev, S.qdat, (int *)0);
        else if (mode == QMODE_I16) nz = wave_xform_quant_recon<QMODE_I16>(S.a, S.b, S.o, 16, S.q, S.dc, S.lev, S.qdat, (int *)0);
        else if (mode == QMODE_CHROMA) nz = wave_xform_quant_recon<QMODE_CHROMA>(S.a, S.b, S.o, 16, S.q, S.dc, S.lev, S.qdat, &dcflag);
        else nz = i4_block_code(i4q_make(S.qdat), S.a, S.b, S.o, 16, S.q);
        wave_sync();
        WAVE_FOR(l)
        {
            for (int k = l; k < 256; k += 64) gstore32((gu8 *)out + 8 + 4*k, lds32((const uint8_t *)S.q + 4*k));
            if (l < 8) { gstore32((gu8 *)out + 8 + 1024 + 4*l, lds32((const uint8_t *)S.dc + 4*l)); gstore32((gu8 *)out + 8 + 1056 + 4*l, lds32((const uint8_t *)S.lev + 4*l)); }
        }
        wave_sync();
        WAVE_FOR(l) { gstore32((gu8 *)out + 8 + 1088 + 4*l, lds32(S.o + 4*l)); }
        if (wave_lane() == 0) { oi[0] = (int32_t)nz; oi[1] = dcflag; }
        (void)side;
    } else if (stage == 5)
    {
        cavlc_tab_load(S.ct);
        WAVE_FOR(l) { if (l < 8) lds32_store((uint8_t *)S.coef + 4*l, gload32((const gu8 *)in + 4*l)); }
        wave_sync();
        BitW b;
        b.acc = 0; b.nacc = 0; b.pos = 0; b.cap = 60; b.overflow = 0; b.buf = (GLOBAL_AS uint32_t *)(out + 8);
        if (a[3] > 0) bw_put(b, imin(a[3], 31), (1u << imin(a[3], 31)) - 1u);          /* bits already in the buffer: ones, so that a lost or smeared bit shows */
        const int nnz = cavlc_block(b, S.ct, S.coef, a[0], a[1], a[2]);
        const uint32_t nbits = bw_bits(b);
        if (b.nacc) bw_put(b, 32 - b.nacc, 0);
        if (wave_lane() == 0) { oi[0] = nnz; oi[1] = (int32_t)nbits; }
    } else if (stage == 6)
    {
        WAVE_FOR(l)
        {
            if (l < 13)
            {
                const uint8_t e = in[l];
                if (l < 4) S.nb[24*(4 - l) + 3] = e;            /* L3..L0: the column left of the block, bottom-up */
                else S.nb[3 + (l - 4)] = e;                     /* UL, U0..U7: the row above */
            }
            if (l < 16) lds32_store(S.a + 4*l, gload32((const gu8 *)in + 16 + 4*l));
            if (l < 16) lds32_store(S.o + 4*l, 0u);
        }
        wave_sync();
        const int res = wave_i4_choose(S.a, S.o, a[0], S.nb + 24 + 4, a[1], a[2], S.i4s, i4_lanes_make(24));
        wave_sync();
        WAVE_FOR(l) { if (l < 16) gstore32((gu8 *)out + 8 + 4*l, lds32(S.o + 4*l)); }
        if (wave_lane() == 0) { oi[0] = res & 15; oi[1] = res >> 4; }
    } else if (stage == 7)
    {
        const int ny = 20*YT_STRIDE, nc = 10*CT_STRIDE;
        df_tab_load(S.df);
        WAVE_FOR(l)
        {
            for (int k = l; k < ny; k += 64) S.yt[k] = in[k];
            for (int k = l; k < nc; k += 64) { S.ctile[0][k] = in[ny + k]; S.ctile[1][k] = in[ny + nc + k]; }
            if (l < 32) S.bs[l] = in[ny + 2*nc + l];
        }
        wave_sync();
        wave_deblock(S.yt, S.ctile[0], S.ctile[1], S.bs, a[0], a[1], a[2], S.df);
        wave_sync();
        WAVE_FOR(l)
        {
            for (int k = l; k < ny; k += 64) out[k] = S.yt[k];
            for (int k = l; k < nc; k += 64) { out[ny + k] = S.ctile[0][k]; out[ny + nc + k] = S.ctile[1][k]; }
        }
    } else if (stage == 8)
    {
        /* the macroblock at (32,32) of a 96x96 reference picture, as row_step sets a macroblock up for inter_choose */
        h264e_geom_t Gs;
        MbCtx m;
        Plane P8 = { (const gu8 *)in, 96, 96, 96 };
        Gs.width = Gs.W = 96; Gs.height = Gs.H = 96; Gs.nmbx = Gs.nmby = 6; Gs.nmb = 36; Gs.cropping = 0;
        Gs.lim_x0 = a[15]; Gs.lim_y0 = a[16]; Gs.lim_x1 = a[17]; Gs.lim_y1 = a[18];
        m.G = &Gs; m.speed = a[10]; m.slice_type = 0; m.x = 2; m.y = 2; m.num = 14; m.qp = a[9];
        m.lambda_mv = k_lambda_mv_q4[a[9]];
        m.rv = R; m.rv.P = P8; m.rv.nmbx = 6; m.rv.nmby = 6;
        if (a[19]) { m.rv.has_win = 1; m.rv.wx0 = 32 - WIN_M; m.rv.win = (const lu8 *)L.win + win_org(m.rv.wx0); m.rv.wy0 = 32 - WIN_M; wave_load_window(L.win, P8, m.rv.wx0, m.rv.wy0, 0); }
        WAVE_FOR(l) { lds32_store(L.mb[0].inp + 4*l, gload32((const gu8 *)in + 96*96 + 4*l)); lds32_store(L.gtest[0] + 4*l, 0u); }
        wave_sync();
        const rect_t range = { a[11], a[12], a[13], a[14] };
        /* the search is lane-group code (wave.h): group a[20] runs it, the other three idle */
        GRP_EACH(grp)
        {
            if (grp == (a[20] & 3))
            {
                mv32 mv = mvmk(a[4], a[5]);
                const int cost = diamond_g(L, L.mb[0], m, a[0], a[1], mv, range, mvmk(a[6], a[7]), a[8], a[2], a[3], L.gtest[0] + 16*a[1] + a[0], L.gscr);
                L.gcost[0] = cost; L.gcost[1] = mvx(mv); L.gcost[2] = mvy(mv);
            }
        }
        wave_sync();
        WAVE_FOR(l) { gstore32((gu8 *)out + 16 + 4*l, lds32(L.gtest[0] + 4*l)); }
        if (wave_lane() == 0) { oi[0] = L.gcost[0]; oi[1] = L.gcost[1]; oi[2] = L.gcost[2]; }
    } else if (stage == 9 || stage == 10)
    {
        /* the macroblock's input and its neighbours' reconstructed edge lines where row_step keeps them: L.pix_left / B.pix_top, 16 Y | 8 U | 8 V */
        MbBuf &B = L.mb[0];
        WAVE_FOR(l)
        {
            if (stage == 9)
            {
                lds32_store(B.inp + 4*l, gload32((const gu8 *)in + 4*l));
                if (l < 4) { lds32_store(L.pix_left + 4*l, gload32((const gu8 *)in + 256 + 4*l)); lds32_store(B.pix_top + 4*l, gload32((const gu8 *)in + 272 + 4*l)); }
            } else if (l < 4) { lds32_store(L.pix_left + 16 + 4*l, gload32((const gu8 *)in + 4*l)); lds32_store(B.pix_top + 16 + 4*l, gload32((const gu8 *)in + 16 + 4*l)); }
        }
        wave_sync();
        if (stage == 9)
        {
            MbCtx m;
            m.avail = a[0]; m.qp = imin(imax(a[1], 0), 51); m.i16_mode = -1;
            m.lambda_q4 = k_lambda_q4[m.qp]; m.lambda_i16 = k_lambda_i16_q4[m.qp];
            const int cost = intra16_cost(L, B, m);
            wave_sync();
            WAVE_FOR(l) { gstore32((gu8 *)out + 8 + 4*l, lds32(L.i16pred + 4*l)); }
            if (wave_lane() == 0) { oi[0] = m.i16_mode; oi[1] = cost; }
        } else
        {
            WAVE_FOR(l) { if (l < 32) lds32_store(L.pred_c + 4*l, 0u); }
            wave_sync();
            wave_pred_chroma(L.pred_c, L.pix_left + 16, B.pix_top + 16, a[0], a[1]);
            WAVE_FOR(l) { if (l < 32) gstore32((gu8 *)out + 4*l, lds32(L.pred_c + 4*l)); }
        }
    } else if (stage == 11)
    {
        /* one macroblock's partitions in coding order: every partition reads its predictor, then puts its vector (mb_write's sequence) */
        MbBuf &B = L.mb[0];
        const GLOBAL_AS int32_t *ii = (const GLOBAL_AS int32_t *)in;
        const int n = imin(imax(a[1], 0), 16);
        WAVE_FOR(l)
        {
            if (l < 4) { L.mv_left[l] = ii[l]; L.mv_tl[l] = ii[4 + l]; }
            if (l < 8) B.mv_top[l] = ii[8 + l];
        }
        wave_sync();
        for (int k = 0; k < n; k++)
        {
            const int x = uni(ii[16 + 5*k]) & 3, y = uni(ii[17 + 5*k]) & 3, w = imin(uni(ii[18 + 5*k]), 4 - x), h = imin(uni(ii[19 + 5*k]), 4 - y);
            const mv32 pred = (mv32)uni(mvp_get_arr(L.mv_left, L.mv_tl, B.mv_top, a[0], x, y, w, h));
            if (wave_lane() == 0) oi[k] = pred;
            wave_sync();
            mvp_put_arr(L.mv_left, L.mv_tl, B.mv_top, x, y, w, h, (mv32)uni(ii[20 + 5*k]));
            wave_sync();
        }
        WAVE_FOR(l)
        {
            if (l < 4) { oi[16 + l] = L.mv_left[l]; oi[20 + l] = L.mv_tl[l]; }
            if (l < 8) oi[24 + l] = B.mv_top[l];
        }
    } else if (stage == 12)
    {
        const GLOBAL_AS int32_t *ii = (const GLOBAL_AS int32_t *)in;
        MbCtx m;
        WAVE_FOR(l) { if (l < 25) L.df_mv[l] = ii[l]; if (l < 8) lds32_store(L.bs + 4*l, 0xeeeeeeeeu); }
        if (wave_lane() == 0) { L.df_nzflag = (uint32_t)a[0]; L.left_type = a[1]; }
        wave_sync();
        m.type = a[3]; m.x = a[4]; m.slice_top = a[5];
        df_strength(L, m, a[2]);
        WAVE_FOR(l) { if (l < 8) gstore32((gu8 *)out + 4*l, lds32(L.bs + 4*l)); }
    } else if (stage == 13 || stage == 14)
    {
        /* scalars of the decision, a[0] records per launch, one lane each: 13 partition_hints (4 SADs -> 4 flags), 14 mv_cost (vector, predictor, QP) */
        const GLOBAL_AS int32_t *ii = (const GLOBAL_AS int32_t *)in;
        const int n = imin(imax(a[0], 0), stage == 13 ? 64 : 256);
        WAVE_FOR(l)
        {
            for (int k = l; k < n; k += 64)
            {
                if (stage == 13)
                {
                    const int sad[4] = { ii[4*k], ii[4*k + 1], ii[4*k + 2], ii[4*k + 3] };
                    int mode[4] = { 0, 0, 0, 0 };
                    partition_hints(sad, mode);
                    for (int j = 0; j < 4; j++) oi[4*k + j] = mode[j];
                } else
                {
                    MbCtx m;
                    m.lambda_mv = k_lambda_mv_q4[imin(imax(ii[5*k + 4], 0), 51)];
                    oi[k] = mv_cost(m, mvmk(ii[5*k], ii[5*k + 1]), mvmk(ii[5*k + 2], ii[5*k + 3]));
                }
            }
        }
    } else if (stage == 15)
    {
        /* a list of puts: (kind, value, length) with kind 0 bw_put, 1 bw_ue, 2 bw_se */
        const GLOBAL_AS int32_t *ii = (const GLOBAL_AS int32_t *)in;
        const int n = imin(imax(a[0], 0), 64);
        BitW b;
        b.acc = 0; b.nacc = 0; b.pos = 0; b.cap = 60; b.overflow = 0; b.buf = (GLOBAL_AS uint32_t *)(out + 8);
        for (int k = 0; k < n; k++)
        {
            const int kind = uni(ii[3*k]), v = uni(ii[3*k + 1]), len = uni(ii[3*k + 2]);
            if (kind == 0) bw_put(b, imin(imax(len, 0), 32), (uint32_t)v);
            else if (kind == 1) bw_ue(b, (uint32_t)v);
            else bw_se(b, v);
        }
        const uint32_t nbits = bw_bits(b);
        if (b.nacc) bw_put(b, 32 - b.nacc, 0);
        if (wave_lane() == 0) { oi[0] = (int32_t)nbits; oi[1] = b.overflow; }
    } else if (stage == 16)
    {
        /* every pair of bytes once: byte j of dword k holds the pair number n = 4*k + j, x = n >> 8 and y = n & 255 */
        WAVE_FOR(l)
        {
            for (int k = l; k < STAGE_AVG4_DWORDS; k += 64)
            {
                const uint32_t x = (uint32_t)(k >> 6)*0x01010101u, y = (uint32_t)((4*k) & 255)*0x01010101u + 0x03020100u;
                gstore32((gu8 *)out + 4*k, avg4_u8(x, y));
            }
        }
    }
}

/* ------------------------------------------------------------------ finalizer test hook (tests/test_finalizer.py)
 * Runs the finalizer wave's own functions (enc_finalize.h, from "slice splice" up to export_frame) on caller-supplied operands, in the geometry of the pool (nmbx, nmby,
 * row_words).  The host side (h264e_pool.h h264e_hip_selftest_finalizer) builds the task and the chain descriptor in device memory as a
 * submit would, pointing at the operands; nothing here waits: on_row returns 0 at once, no counter, abort word or verdict is polled.
 *   1 splice   splice_frame (splice_put / splice_words / put_ue64) over C.rowmeta / C.far_reads / C.rowbits into C.arena
 *              hdr: int32 status, start, nbytes, overflow, all_skipped, far_reads, 0, 0, slice_nbytes[16]
 *   2 walk     JobWalk begin / rows(upto) ... / end, device_clusters_walk and clusters_moved over C.mbrec
 *              args: [2..3] start state, [6] n, [32..32+n) the upto values      traj: JobWalk's [nmb][2], then the whole-frame walk's
 *              hdr: int32 JobWalk first_bad, state[2] | whole-frame walk first_bad, state[2] | moved
 *   3 step     clusters_step and mvround            args: [0] n      in: n x int32 (c0, c1, mv)
 *              out: n x int32 (c0', c1', mvround(c0), mvround(c1), mvround(mv))
 */
#define FZ_NARGS 96
#define FZ_HDR_INTS 32
#define FZ_STEP_MAX 4096
DEV void finalizer_selftest(const h264e_geom_t &G, const h264e_frame_task_t &T, int mode, const int *args, const GLOBAL_AS int32_t *in, GLOBAL_AS int32_t *hdr, GLOBAL_AS mv32 *traj)
{
    if (mode == 1)
    {
        const ChainG C = chain_view(*T.chain_desc);
        SpliceOut so = { 0, 0, 0, 0, 0 };
        const int st = splice_frame(G, C, T, so, [&](int, int) -> int { return 0; });
        drain_stores();
        wave_sync();
        if (wave_lane() == 0)
        {
            hdr[0] = st; hdr[1] = (int32_t)so.start; hdr[2] = (int32_t)so.nbytes; hdr[3] = so.overflow; hdr[4] = so.all_skipped; hdr[5] = so.far_reads;
            for (int k = 0; k < H264E_MAX_SLICES; k++) hdr[8 + k] = k < T.nslices ? (int32_t)C.fout[T.frame_slot].slice_nbytes[k] : 0;
        }
    } else if (mode == 2)
    {
        const ChainG C = chain_view(*T.chain_desc);
        const GLOBAL_AS h264e_mbrec_t *rec = C.mbrec + (size_t)T.frame_slot*G.nmb;
        const mv32 s0[2] = { (mv32)uni(args[2]), (mv32)uni(args[3]) };
        const int n = uni(args[6]);
        JobWalk W;
        W.begin(s0);
        for (int i = 0; i < n; i++) W.rows(G, T, rec, traj, uni(args[32 + i]));
        W.end(T);
        mv32 s[2] = { s0[0], s0[1] };
        const int fb = device_clusters_walk(G, T, rec, s, traj + 2*(size_t)G.nmb);
        const int moved = clusters_moved(G, T, rec);
        if (wave_lane() == 0)
        {
            hdr[0] = W.first_bad; hdr[1] = W.s[0]; hdr[2] = W.s[1];
            hdr[3] = fb; hdr[4] = s[0]; hdr[5] = s[1];
            hdr[6] = moved;
        }
    } else if (mode == 3)
    {
        const int n = uni(args[0]);
        for (int base = 0; base < n; base += 64)
        {
            WAVE_FOR(l)
            {
                const int k = base + l;
                if (k < n)
                {
                    mv32 c[2] = { in[3*k], in[3*k + 1] };
                    const mv32 mv = in[3*k + 2];
                    clusters_step(c, mv);
                    hdr[5*k] = c[0]; hdr[5*k + 1] = c[1];
                    hdr[5*k + 2] = mvround(in[3*k]); hdr[5*k + 3] = mvround(in[3*k + 1]); hdr[5*k + 4] = mvround(mv);
                }
            }
        }
    }
}

/* synth_v1 generator, one sample per call */
DEV uint32_t sv_h32(uint32_t a)
{
    a ^= a >> 16; a *= 0x7feb352du; a ^= a >> 15; a *= 0x846ca68bu; a ^= a >> 16;
    return a;
}
DEV int sv_lattice(int32_t ix, int32_t iy, uint32_t seed) { return (int)(sv_h32((uint32_t)ix*0x9E3779B1u ^ (uint32_t)iy*0x85EBCA77u ^ seed) & 255); }
DEV int sv_tex(int32_t X, int32_t Y, uint32_t seed, int lg)
{
    int32_t c = 1 << lg, ix = X >> lg, iy = Y >> lg, fx = X & (c - 1), fy = Y & (c - 1);
    int32_t a = sv_lattice(ix, iy, seed), b = sv_lattice(ix + 1, iy, seed), cc = sv_lattice(ix, iy + 1, seed), d = sv_lattice(ix + 1, iy + 1, seed);
    int32_t top = a*(c - fx) + b*fx, bot = cc*(c - fx) + d*fx;
    return (top*(c - fy) + bot*fy + (1 << (2*lg - 1))) >> (2*lg);
}
DEV uint8_t sv_sample(int w, int h, int t, uint32_t seed, int idx)
{
    const int32_t OFF = 1 << 20;
    if (idx < w*h)
    {
        int x = idx % w, y = idx / w, fw = w/8 > 32 ? w/8 : 32, fh = h/6 > 32 ? h/6 : 32;
        int fx0 = (w/2 + ((10*t) >> 2)) % (w - fw), fy0 = h/3, v;
        if (x >= fx0 && x < fx0 + fw && y >= fy0 && y < fy0 + fh) v = sv_tex(4*x - 10*t + OFF, 4*y + OFF, seed + 1, 5);
        else v = (sv_tex(4*x + 5*t + OFF, 4*y + 3*t + OFF, seed, 6)*3 >> 2) + 32;
        v += (int)(sv_h32((uint32_t)x ^ ((uint32_t)y << 12) ^ ((uint32_t)t << 24) ^ (uint32_t)(seed*7919u)) % 5) - 2;
        return (uint8_t)clip255(v);
    }
    idx -= w*h;
    const int cw = w/2, ch = h/2, pl = idx >= cw*ch;
    if (pl) idx -= cw*ch;
    int x = idx % cw, y = idx / cw;
    if (!pl) return (uint8_t)(128 + ((sv_tex(8*x + 5*t + OFF, 8*y + 3*t + OFF, seed + 2, 7) - 128) >> 2));
    return (uint8_t)(128 - ((sv_tex(8*x + 5*t + OFF, 8*y + 3*t + OFF, seed + 3, 7) - 128) >> 3));
}

#endif
