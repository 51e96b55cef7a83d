/*
 * stage_harness.c -- TEST INFRASTRUCTURE.  Generator of tests/golden/stages.json: inputs and outputs of the REFERENCE's own
 * per-stage functions, obtained by compiling the reference header into this translation unit (a TU
 * that includes h264-lab.h sees every `static` function).  Built and run in the build container only (`make -C oracle stages`):
 * the reference sources do not travel; the JSON it prints -- data: seeded inputs, the reference's outputs -- is committed.
 * Nothing of the reference is copied here: this file only CALLS
 *   h264e_sad_mb_unlaign_8x8            h264-lab.h:2178     16x16 SAD as four 8x8 quadrant sums
 *   h264e_qpel_interpolate_luma         h264-lab.h:2079     the 16 quarter-sample positions
 *   h264e_qpel_interpolate_chroma       h264-lab.h:2133     eighth-sample bilinear
 *   h264e_transform_sub_quant_dequant   h264-lab.h:2619     forward transform, dead-zone quantiser, dequantiser (4 modes)
 *   h264e_quant_luma_dc / _chroma_dc    h264-lab.h:2344/2355
 *   h264e_transform_add                 h264-lab.h:2638     reconstruction
 *   h264e_vlc_encode                    h264-lab.h:2775     one CAVLC residual block
 *   h264e_intra_choose_4x4              h264-lab.h:1810     intra 4x4 mode decision: nine predictors, tie-breaks, prediction
 *   me_search_diamond + me_mv_set_range h264-lab.h:4973/5181 full-sample diamond search (SAD cache, diagonal probe) + the seven sub-sample probes
 *   df_strength + mb_deblock            h264-lab.h:5532/5642 boundary strengths of a macroblock and its in-loop filter (luma + chroma)
 *   rc_set_qp                           h264-lab.h:5839     the quantiser tables of a QP
 * `stage_harness edges` prints tests/golden/stage_edges.json instead (own seed; edges() at the end of this file): the same functions at
 * the edges of their input ranges -- footprints across the picture borders on a picture padded by h264e_copy_borders (h264-lab.h:2232),
 * reconstructions and filters that clip at 0 and 255, 13..16 coefficients, escape levels, writers that start mid-word, searches that end
 * on their limits -- and the decision functions the first file has no case of:
 *   intra_choose_16x16 (intra_estimate_16x16, h264e_intra_predict_16x16)   h264-lab.h:4876 (4838, 1677)
 *   h264e_intra_predict_chroma          h264-lab.h:1716
 *   me_mv_medianpredictor_get / _put    h264-lab.h:3720/3696
 *   df_strength                         h264-lab.h:5535     here for the strengths themselves
 *   mb_inter_partition, me_mv_cost      h264-lab.h:5224/4952
 *   h264e_bs_put_bits / _golomb / _sgolomb   h264-lab.h:2688/2738/2760
 * `stage_harness finalizer` prints tests/golden/finalizer.json (own seed; finalizer() at the end of this file): what the frame finalizer's
 * exact mv_clusters walk restates, from the reference's own
 *   mv_clusters_update                  h264-lab.h:5263     single steps at the edges of both comparisons and of the vector range, seeded sequences
 *   mv_round_qpel                       h264-lab.h:3498     every component in -8..8
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#define MINIH264_IMPLEMENTATION
#include "h264-lab.h"

static uint32_t g_seed = 12345;
static uint32_t rnd(void) { g_seed = g_seed*1664525u + 1013904223u; return g_seed >> 8; }

static void hex(const char *name, const void *p, size_t n, int last)
{
    const uint8_t *b = (const uint8_t *)p;
    size_t i;
    printf("   \"%s\": \"", name);
    for (i = 0; i < n; i++) printf("%02x", b[i]);
    printf("\"%s\n", last ? "" : ",");
}

/* smooth + noise picture, so that interpolation and SAD see edges as well as flat areas */
static void fill_pic(uint8_t *p, int w, int h, int amp)
{
    int x, y;
    for (y = 0; y < h; y++)
        for (x = 0; x < w; x++)
        {
            int v = 128 + (int)(60*((x*7 + y*3) % 32)/32) - 30 + (int)(rnd() % (unsigned)(2*amp + 1)) - amp;
            if ((x / 8 + y / 8) & 1) v += 40;
            p[y*w + x] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
        }
}

static int edges(h264e_enc_t *enc);
static int finalizer(h264e_enc_t *enc);

int main(int argc, char **argv)
{
    static uint8_t pic[64*64];
    ALIGN(16) static uint8_t blk[16*16] ALIGN2(16), dst[16*16] ALIGN2(16);
    int i, k, first = 1;
    H264E_create_param_t cp;
    h264e_enc_t *enc;
    void *scratch;
    int sizeof_persist = 0, sizeof_scratch = 0;

    memset(&cp, 0, sizeof(cp));
    cp.width = 64; cp.height = 64; cp.gop = 1; cp.vbv_size_bytes = 100000; cp.max_long_term_reference_frames = 0;
    if (H264E_sizeof(&cp, &sizeof_persist, &sizeof_scratch)) return 1;
    enc = (h264e_enc_t *)calloc(1, (size_t)sizeof_persist);
    scratch = calloc(1, (size_t)sizeof_scratch);
    if (!enc || !scratch || H264E_init(enc, &cp)) return 1;
    if (argc > 1 && !strcmp(argv[1], "edges"))
    {
        int r;
        enc->scratch = (scratch_t *)scratch;
        r = edges(enc);
        free(scratch); free(enc);
        return r;
    }

    if (argc > 1 && !strcmp(argv[1], "finalizer"))
    {
        int r = finalizer(enc);
        free(scratch); free(enc);
        return r;
    }

    printf("{\n \"generator\": \"oracle/stage_harness.c against the reference header (h264-lab.h), make -C oracle stages\",\n");

    /* ---- SAD quadrants */
    printf(" \"sad\": [\n");
    for (i = 0; i < 8; i++)
    {
        int sad4[4], tot, ox = (int)(rnd() % 40), oy = (int)(rnd() % 40);
        fill_pic(pic, 64, 64, 4 + 6*i);
        for (k = 0; k < 256; k++) blk[k] = (uint8_t)(pic[(oy + (k >> 4) + ((i & 1) ? 1 : 0))*64 + ox + (k & 15) + ((i & 2) ? 2 : 0)] + (int)(rnd() % 7) - 3);
        tot = h264e_sad_mb_unlaign_8x8(pic + oy*64 + ox, 64, blk, sad4);
        printf("  {\n");
        hex("pic", pic, sizeof(pic), 0);
        hex("blk", blk, 256, 0);
        printf("   \"ox\": %d, \"oy\": %d, \"sad4\": [%d, %d, %d, %d], \"sad\": %d\n  }%s\n", ox, oy, sad4[0], sad4[1], sad4[2], sad4[3], tot, i == 7 ? "" : ",");
    }
    printf(" ],\n");

    /* ---- luma interpolation: all 16 quarter-sample positions at 16x16, the full / half-sample ones at 16x8, 8x16, 8x8 */
    printf(" \"qpel_luma\": [\n");
    fill_pic(pic, 64, 64, 12);
    printf("  {\n");
    hex("pic", pic, sizeof(pic), 0);
    printf("   \"cases\": [\n");
    first = 1;
    for (k = 0; k < 4; k++)
    {
        const int w = (k & 2) ? 8 : 16, h = (k & 1) ? 8 : 16;
        int dx, dy;
        for (dy = 0; dy < 4; dy++)
            for (dx = 0; dx < 4; dx++)
            {
                point_t wh, dxdy;
                const int x0 = 20 + 3*k, y0 = 18 + 5*k;
                if (k && ((dx | dy) & 1)) continue;        /* the quarter-sample positions exist for 16x16 only (h264-lab.h:2114) */
                wh.u32 = 0; dxdy.u32 = 0;
                wh.s.x = (int16_t)w; wh.s.y = (int16_t)h; dxdy.s.x = (int16_t)dx; dxdy.s.y = (int16_t)dy;
                memset(dst, 0, sizeof(dst));
                h264e_qpel_interpolate_luma(pic + y0*64 + x0, 64, dst, wh, dxdy);
                printf("%s    {\"x\": %d, \"y\": %d, \"w\": %d, \"h\": %d, \"dx\": %d, \"dy\": %d,\n ", first ? "" : ",\n", x0, y0, w, h, dx, dy);
                hex("dst", dst, 256, 1);
                printf("    }");
                first = 0;
            }
    }
    printf("\n   ]\n  }\n ],\n");

    /* ---- chroma eighth-sample interpolation */
    printf(" \"qpel_chroma\": [\n");
    fill_pic(pic, 64, 64, 10);
    printf("  {\n");
    hex("pic", pic, sizeof(pic), 0);
    printf("   \"cases\": [\n");
    first = 1;
    for (k = 0; k < 16; k++)
    {
        point_t wh, dxdy;
        const int w = (k & 8) ? 4 : 8, h = (k & 4) ? 4 : 8, dx = (int)(rnd() % 8), dy = (k == 0) ? 0 : (int)(rnd() % 8), x0 = 10 + k, y0 = 30 - k;
        wh.u32 = 0; dxdy.u32 = 0;
        wh.s.x = (int16_t)w; wh.s.y = (int16_t)h; dxdy.s.x = (int16_t)(k == 0 ? 0 : dx); dxdy.s.y = (int16_t)dy;
        memset(dst, 0, sizeof(dst));
        h264e_qpel_interpolate_chroma(pic + y0*64 + x0, 64, dst, wh, dxdy);
        printf("%s    {\"x\": %d, \"y\": %d, \"w\": %d, \"h\": %d, \"dx\": %d, \"dy\": %d,\n ", first ? "" : ",\n", x0, y0, w, h, dxdy.s.x, dxdy.s.y);
        hex("dst", dst, 256, 1);
        printf("    }");
        first = 0;
    }
    printf("\n   ]\n  }\n ],\n");

    /* ---- transform + quantise + dequantise + reconstruct, the four modes, several QPs, residuals from tiny to large */
    printf(" \"quant\": [\n");
    first = 1;
    {
        static const int qps[] = { 10, 22, 26, 33, 40, 51 };
        static const int modes[] = { QDQ_MODE_INTER, QDQ_MODE_INTRA_16, QDQ_MODE_INTRA_4, QDQ_MODE_CHROMA };
        unsigned qi, mi, p_slice;
        for (qi = 0; qi < sizeof(qps)/sizeof(qps[0]); qi++)
            for (p_slice = 0; p_slice < 2; p_slice++)
                for (mi = 0; mi < 4; mi++)
                {
                    const int mode = modes[mi], qp = qps[qi], side = mode >> 1, nblk = (mode == QDQ_MODE_INTRA_4) ? 1 : side*side;
                    const int amp = 2 + (int)((qi*7 + mi*3 + p_slice) % 5)*9;
                    ALIGN(16) static uint8_t inp[16*16] ALIGN2(16), pred[16*16] ALIGN2(16), out[16*16] ALIGN2(16);
                    /* the DC coefficients of the INTRA_16 / CHROMA modes are written in FRONT of the block array (h264-lab.h:2626) */
                    static struct { int16_t dc[16]; quant_t q[16]; } Q, Qsnap;
                    int16_t deq_dc[16];
                    int nz, dcflag = 0;
                    if (mode == QDQ_MODE_INTER && !p_slice) continue;          /* inter blocks exist in P slices only */
                    enc->run_param.qp_min = enc->run_param.qp_max = (uint8_t)qp;
                    enc->slice.type = p_slice ? SLICE_TYPE_P : SLICE_TYPE_I;
                    enc->rc.qp = 0;
                    rc_set_qp(enc, qp);
                    for (k = 0; k < 256; k++)
                    {
                        pred[k] = (uint8_t)(100 + (k & 15)*3 + (int)(rnd() % 9));
                        inp[k] = (uint8_t)(pred[k] + (int)(rnd() % (unsigned)(2*amp + 1)) - amp + (((k >> 6) & 1) ? amp/2 : 0));
                    }
                    memset(&Q, 0, sizeof(Q));
                    memset(deq_dc, 0, sizeof(deq_dc));
                    nz = h264e_transform_sub_quant_dequant(inp, pred, 16, mode, Q.q, enc->rc.qdat[mode == QDQ_MODE_CHROMA ? 1 : 0]);
                    if (mode == QDQ_MODE_INTRA_16) h264e_quant_luma_dc(Q.q, deq_dc, enc->rc.qdat[0]);
                    if (mode == QDQ_MODE_CHROMA) dcflag = h264e_quant_chroma_dc(Q.q, deq_dc, enc->rc.qdat[1]);
                    memcpy(&Qsnap, &Q, sizeof(Q));               /* the reconstruction transforms dq in place */
                    /* reconstruction exactly as mb_write / intra_choose_4x4 call it (h264-lab.h:4428-4433, 4468-4488, 4809-4811) */
                    memcpy(out, pred, sizeof(out));
                    if (mode == QDQ_MODE_INTER) h264e_transform_add(out, 16, pred, Q.q, 4, nz << 16);
                    else if (mode == QDQ_MODE_INTRA_16) h264e_transform_add(out, 16, pred, Q.q, 4, 0xFFFF << 16);
                    else if (mode == QDQ_MODE_INTRA_4) { if (nz & 1) h264e_transform_add(out, 16, pred, Q.q, 1, ~0); }
                    else if (dcflag | nz)
                    {
                        int m = nz, b4;
                        if (dcflag)
                        {
                            for (b4 = 0; b4 < 4; b4++) if (~nz & (8 >> b4)) memset(Q.q[b4].dq + 1, 0, (16 - 1)*sizeof(int16_t));
                            m = 15;
                        }
                        h264e_transform_add(out, 16, pred, Q.q, 2, m << 28);
                    }
                    printf("%s  {\"qp\": %d, \"p_slice\": %u, \"mode\": %d, \"nz\": %d, \"dcflag\": %d,\n", first ? "" : ",\n", qp, p_slice, mode, nz, dcflag);
                    hex("inp", inp, 256, 0);
                    hex("pred", pred, 256, 0);
                    hex("qdat", enc->rc.qdat[mode == QDQ_MODE_CHROMA ? 1 : 0], sizeof(enc->rc.qdat[0]), 0);
                    hex("dc", Qsnap.dc, sizeof(Q.dc), 0);
                    hex("deq_dc", deq_dc, sizeof(deq_dc), 0);
                    hex("q", Qsnap.q, sizeof(quant_t)*(size_t)nblk, 0);
                    hex("out", out, 256, 1);
                    printf("  }");
                    first = 0;
                }
    }
    printf("\n ],\n");

    /* ---- one CAVLC residual block: every table (nC ranges, chroma DC), densities from empty to full, large levels */
    printf(" \"cavlc\": [\n");
    first = 1;
    for (i = 0; i < 96; i++)
    {
        static const int maxn[] = { 16, 15, 4 };
        const int mn = maxn[i % 3], dens = 1 + (i / 3) % 8, big = (i % 7) == 0;
        int16_t q[32], q_in[16];
        uint8_t nzc[3];
        uint8_t buf[256];
        bs_t bs;
        unsigned nbits;
        memset(q, 0, sizeof(q));
        for (k = 0; k < 16; k++)
            if ((int)(rnd() % 9) < dens)
            {
                int v = (int)(rnd() % 3) - 1;
                if ((rnd() % 4) == 0) v = (int)(rnd() % 9) - 4;
                if (big && (rnd() % 3) == 0) v = (int)(rnd() % 4001) - 2000;
                q[k] = (int16_t)v;
            }
        if (i == 0) memset(q, 0, sizeof(q));
        if (mn == 4) { nzc[0] = 17; nzc[2] = 17; }                                    /* the chroma-DC table (h264-lab.h:4477) */
        else { nzc[0] = (uint8_t)(rnd() % 17); nzc[2] = (uint8_t)((rnd() % 5) == 0 ? 64 : rnd() % 17); if ((rnd() % 5) == 0) nzc[0] = 64; }
        nzc[1] = 0xee;
        memcpy(q_in, q, sizeof(q_in));                  /* the function packs the levels into the array it is given */
        memset(buf, 0, sizeof(buf));
        h264e_bs_init_bits(&bs, buf);
        {
            const uint8_t l = nzc[0], t = nzc[2];
            h264e_vlc_encode(&bs, q, mn, nzc + 1);
            nbits = h264e_bs_get_pos_bits(&bs);
            h264e_bs_flush(&bs);
            printf("%s  {\"maxn\": %d, \"left\": %d, \"top\": %d, \"nnz\": %d, \"nbits\": %u,\n", first ? "" : ",\n", mn, l, t, nzc[1], nbits);
        }
        hex("coef", q_in, 32, 0);
        hex("bits", buf, (nbits + 7)/8 + 4, 1);
        printf("  }");
        first = 0;
    }
    printf("\n ],\n");

    /* ---- intra 4x4 mode choice: every neighbour availability, every predicted mode, edges from flat to steep */
    printf(" \"intra4\": [\n");
    first = 1;
    for (i = 0; i < 160; i++)
    {
        ALIGN(16) static uint8_t in4[16*4] ALIGN2(16), pr4[16*4] ALIGN2(16);
        ALIGN(4) uint8_t edge_store[16] ALIGN2(4);          /* [0..3] = L3..L0, [4] = UL, [5..12] = U0..U7 (h264-lab.h:1163-1175) */
        uint8_t edge_in[16];
        const int avail = (i < 16) ? i : (int)(rnd() % 16), mpred = (int)(rnd() % 9), penalty = (i % 5 == 0) ? 0 : (int)(rnd() % 40);
        const int slope = (int)(rnd() % 7) - 3, base = 40 + (int)(rnd() % 160), noise = 1 + (int)(rnd() % 12);
        int ret, y, x;
        for (k = 0; k < 13; k++) { int v = base + slope*(k - 4)*3 + (int)(rnd() % (unsigned)(2*noise + 1)) - noise; edge_store[k] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
        for (k = 13; k < 16; k++) edge_store[k] = 0;
        memset(in4, 0, sizeof(in4)); memset(pr4, 0, sizeof(pr4));
        for (y = 0; y < 4; y++)
            for (x = 0; x < 4; x++)
            {
                int v = base + slope*(x - y)*3 + (int)(rnd() % (unsigned)(2*noise + 1)) - noise;
                if (i % 7 == 3) v = edge_store[5 + x];                          /* exactly vertical: ties between modes */
                if (i % 7 == 5) v = edge_store[3 - y];                          /* exactly horizontal */
                in4[16*y + x] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
            }
        memcpy(edge_in, edge_store, sizeof(edge_in));
        ret = h264e_intra_choose_4x4(in4, pr4, avail, edge_store + 5, mpred, penalty);
        printf("%s  {\"avail\": %d, \"mpred\": %d, \"penalty\": %d, \"mode\": %d, \"cost\": %d,\n", first ? "" : ",\n", avail, mpred, penalty, ret & 15, ret >> 4);
        hex("edge", edge_in, 13, 0);
        hex("in", in4, 64, 0);
        hex("pred", pr4, 64, 1);
        printf("  }");
        first = 0;
    }
    printf("\n ],\n");

    /* ---- deblocking of one macroblock: strengths from df_strength, then mb_deblock on a 32x32 luma / 16x16 chroma neighbourhood
     * (macroblock at (8,8) / (4,4)); macroblock types, coded-block flags, vectors and QPs vary */
    printf(" \"deblock\": [\n");
    first = 1;
    for (i = 0; i < 36; i++)
    {
        static const int types[] = { -1, 0, 1, 2, 3, 5, 6 };
        static uint8_t Yp[32*32], Up[16*16], Vp[16*16], Yin[32*32], Uin[16*16], Vin[16*16];        /* (U0.. are macros of the reference header) */
        deblock_filter_t df, df2;
        uint8_t dfqp[4], dfqp2[4], dfnz[4], dfnz2[4], strength[32];
        int8_t mbt[4], mbt2[4];
        H264E_io_yuv_t io;
        const int mb_type = types[rnd() % 7], qp = 14 + (int)(rnd() % 36), amp = 2 + (int)(rnd() % 24);
        memset(&df, 0, sizeof(df));
        df.df_qp = dfqp + 1; df.mb_type = mbt + 1; df.df_nzflag = dfnz + 1;
        for (k = 0; k < 4; k++)
        {
            int q2 = qp + (int)(rnd() % 7) - 3;
            dfqp[k] = (uint8_t)(q2 < 10 ? 10 : q2 > 51 ? 51 : q2); mbt[k] = (int8_t)types[rnd() % 7]; dfnz[k] = (uint8_t)(rnd() % 16);
        }
        df.nzflag = (i % 4 == 0) ? 0 : (rnd() & 0x1ffffff) & ((rnd() & 1) ? 0x1ffffff : (rnd() & 0x1ffffff));
        for (k = 0; k < 24; k++)
        {
            df.df_mv[k].s.x = (int16_t)(8 + ((rnd() % 5) == 0 ? (int)(rnd() % 9) - 4 : 0));
            df.df_mv[k].s.y = (int16_t)(-4 + ((rnd() % 5) == 0 ? (int)(rnd() % 9) - 4 : 0));
        }
        fill_pic(Yp, 32, 32, amp); fill_pic(Up, 16, 16, amp/2 + 1); fill_pic(Vp, 16, 16, amp/2 + 1);
        /* blocky content: steps at the 4x4 grid, which is what the filter is for */
        for (k = 0; k < 32*32; k++) Yp[k] = (uint8_t)((Yp[k] >> 1) + 40 + (int)(((k & 31) >> 2) + ((k >> 5) >> 2))*((i % 3) + 1));
        memcpy(Yin, Yp, sizeof(Yp)); memcpy(Uin, Up, sizeof(Up)); memcpy(Vin, Vp, sizeof(Vp));
        /* the strengths this state gives (df_strength updates the state: run it on a copy) */
        df2 = df; memcpy(dfqp2, dfqp, 4); memcpy(mbt2, mbt, 4); memcpy(dfnz2, dfnz, 4);
        df2.df_qp = dfqp2 + 1; df2.mb_type = mbt2 + 1; df2.df_nzflag = dfnz2 + 1;
        memset(strength, 0, sizeof(strength));
        df_strength(&df2, mb_type, 1, strength, 0);
        io.yuv[0] = Yp + 8*32 + 8; io.yuv[1] = Up + 4*16 + 4; io.yuv[2] = Vp + 4*16 + 4;
        io.stride[0] = 32; io.stride[1] = 16; io.stride[2] = 16;
        {
            const int qp_left = dfqp[1], qp_top = dfqp[2];
            mb_deblock(&df, mb_type, qp, 1, 1, &io, 0);
            printf("%s  {\"mb_type\": %d, \"qp\": %d, \"qp_left\": %d, \"qp_top\": %d,\n", first ? "" : ",\n", mb_type, qp, qp_left, qp_top);
        }
        hex("bs", strength, 32, 0);
        hex("y_in", Yin, sizeof(Yin), 0); hex("u_in", Uin, sizeof(Uin), 0); hex("v_in", Vin, sizeof(Vin), 0);
        hex("y_out", Yp, sizeof(Yp), 0); hex("u_out", Up, sizeof(Up), 0); hex("v_out", Vp, sizeof(Vp), 1);
        printf("  }");
        first = 0;
    }
    printf("\n ],\n");

    /* ---- motion search of one partition: a 96x96 reference picture, the macroblock at (32,32) displaced by a known motion */
    {
        /* four reference pictures, shared by the cases */
        static uint8_t refs[4][96*96];
        int r4, x, y;
        printf(" \"diamond_refs\": [\n");
        for (r4 = 0; r4 < 4; r4++)
        {
            const int smooth = 3 + r4;
            for (y = 0; y < 96; y++)
                for (x = 0; x < 96; x++)
                {
                    int a = (x*smooth + y*2) % 64, b = (y*smooth - x + 960) % 48, v;
                    a = a < 32 ? a : 63 - a; b = b < 24 ? b : 47 - b;
                    v = 60 + 3*a + 2*b + (int)(rnd() % 5);
                    refs[r4][y*96 + x] = (uint8_t)(v > 255 ? 255 : v);
                }
            printf("  {\n"); hex("pic", refs[r4], sizeof(refs[r4]), 1); printf("  }%s\n", r4 == 3 ? "" : ",");
        }
        printf(" ],\n");
    printf(" \"diamond\": [\n");
    first = 1;
    for (i = 0; i < 64; i++)
    {
        const uint8_t *refp = refs[i & 3];
        ALIGN(16) static uint8_t cur[256] ALIGN2(16), store[8*256] ALIGN2(16);
        static const int parts[9][4] = { {0,0,16,16}, {0,0,16,8}, {0,8,16,8}, {0,0,8,16}, {8,0,8,16}, {0,0,8,8}, {8,0,8,8}, {0,8,8,8}, {8,8,8,8} };
        const int *pt = parts[i < 16 ? 0 : i % 9], px = pt[0], py = pt[1], w = pt[2], h = pt[3];
        const int tx = (int)(rnd() % 13) - 6, ty = (int)(rnd() % 13) - 6, qx = (int)(rnd() % 4), qy = (int)(rnd() % 4);
        const int qp = 18 + (int)(rnd() % 24), noise = (int)(rnd() % 6);
        point_t mv, mv_pred, wh, dd;
        rectangle_t range;
        pix_t *pbest = 0;
        int ret, min_sad, sx, sy;
        /* the input macroblock: the reference displaced by (tx + qx/4, ty + qy/4) samples, plus noise */
        wh.u32 = 0; wh.s.x = 16; wh.s.y = 16; dd.u32 = 0; dd.s.x = (int16_t)qx; dd.s.y = (int16_t)qy;
        h264e_qpel_interpolate_luma(refp + (32 + ty)*96 + 32 + tx, 96, cur, wh, dd);
        for (k = 0; k < 256; k++) { int v = cur[k] + (noise ? (int)(rnd() % (unsigned)(2*noise + 1)) - noise : 0); cur[k] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
        enc->run_param.encode_speed = (i % 16 == 15) ? 9 : 0;                 /* speed 9: no sub-sample search */
        enc->frame.mv_limit.tl = point(8*4, 8*4); enc->frame.mv_limit.br = point((96 - 16 - 8)*4, (96 - 16 - 8)*4);
        enc->frame.mv_qpel_limit.tl = mv_add(enc->frame.mv_limit.tl, point(4*4, 4*4));
        enc->frame.mv_qpel_limit.br = mv_add(enc->frame.mv_limit.br, point(-4*4, -4*4));
        sx = tx + (int)(rnd() % 7) - 3; sy = ty + (int)(rnd() % 7) - 3;        /* start: near the truth, sometimes on it */
        if (i % 5 == 0) { sx = 0; sy = 0; }
        mv = point((32 + sx)*4, (32 + sy)*4);
        me_mv_set_range(&mv, &range, &enc->frame.mv_limit, 32*4 + py*4);
        mv_pred = point((32 + tx)*4 + (int)(rnd() % 17) - 8, (32 + ty)*4 + (int)(rnd() % 17) - 8);
        wh.s.x = (int16_t)w; wh.s.y = (int16_t)h;
        min_sad = h264e_sad_mb_unlaign_wh(refp + ((mv.s.y >> 2) + py)*96 + (mv.s.x >> 2) + px, 96, cur + py*16 + px, wh) + me_mv_cost(mv, mv_pred, qp);
        if (i % 4 == 1) min_sad = 0x7fffff;
        printf("%s  {\"ref\": %d, \"px\": %d, \"py\": %d, \"w\": %d, \"h\": %d, \"qp\": %d, \"speed\": %d, \"mv_in\": [%d, %d], \"mv_pred\": [%d, %d], \"min_sad_in\": %d,\n"
               "   \"range\": [%d, %d, %d, %d], \"limit\": [%d, %d, %d, %d],\n", first ? "" : ",\n", i & 3, px, py, w, h, qp, enc->run_param.encode_speed,
               mv.s.x, mv.s.y, mv_pred.s.x, mv_pred.s.y, min_sad, range.tl.s.x, range.tl.s.y, range.br.s.x, range.br.s.y,
               enc->frame.mv_limit.tl.s.x, enc->frame.mv_limit.tl.s.y, enc->frame.mv_limit.br.s.x, enc->frame.mv_limit.br.s.y);
        memset(store, 0, sizeof(store));
        ret = me_search_diamond(enc, refp + py*96 + px, cur + py*16 + px, 96, &mv, &range, qp, mv_pred, min_sad, wh, store, &pbest,
                                (w == 16 && h == 16) ? 256 : (w == 8 && h == 16) ? 8 : 128);
        printf("   \"cost\": %d, \"mv\": [%d, %d],\n", ret, mv.s.x, mv.s.y);
        {
            uint8_t blk[256];
            memset(blk, 0, sizeof(blk));
            for (y = 0; y < h; y++) memcpy(blk + 16*y, pbest + 16*y, (size_t)w);
            hex("cur", cur, 256, 0);
            hex("pred", blk, 256, 1);
        }
        printf("  }");
        first = 0;
    }
    }
    enc->run_param.encode_speed = 0;
    printf("\n ]\n}\n");
    free(scratch); free(enc);
    return 0;
}

/* ================================================================== `stage_harness edges` -> tests/golden/stage_edges.json
 * Candidates are generated deterministically; where a section is about a property of the RESULT (a search ending on its limit, an intra
 * mode chosen) the candidates that show it are kept until a quota is full.  Only the bytes a test compares are printed. */
#define PADG 32
#define PADS (64 + 2*PADG)
static uint8_t g_pad[(64 + 2*PADG)*PADS];
#define PADP(x, y) (g_pad + (PADG + (y))*PADS + PADG + (x))

static int clipi(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
/* between two cases; small cases go four to a line */
static int g_per_line = 1, g_on_line;
static void sep(int *first)
{
    if (*first) g_on_line = 0;
    else printf(++g_on_line % g_per_line ? ", " : ",\n");
    *first = 0;
}
static void ints(const char *name, const int *v, int n, const char *end)
{
    int i;
    printf("\"%s\": [", name);
    for (i = 0; i < n; i++) printf("%s%d", i ? "," : "", v[i]);
    printf("]%s", end);
}
/* rows of w bytes out of a stride-s block, as one hex string; a run of 6 or more equal bytes is written "(count*xx)" */
static void hexwh(const char *name, const uint8_t *p, int s, int w, int h, const char *end)
{
    static uint8_t b[4096];
    int x, y, n = 0, i, j;
    for (y = 0; y < h; y++) for (x = 0; x < w; x++) b[n++] = p[y*s + x];
    printf("\"%s\": \"", name);
    for (i = 0; i < n; i = j)
    {
        for (j = i + 1; j < n && b[j] == b[i]; j++) ;
        if (j - i >= 6) printf("(%d*%02x)", j - i, b[i]);
        else { printf("%02x", b[i]); j = i + 1; }
    }
    printf("\"%s", end);
}

/* the same rows as one 64-bit FNV-1a digest: for outputs a test only compares as a whole */
static void digwh(const char *name, const uint8_t *p, int s, int w, int h, const char *end)
{
    uint64_t d = 0xcbf29ce484222325ull;
    int x, y;
    for (y = 0; y < h; y++) for (x = 0; x < w; x++) d = (d ^ p[y*s + x])*0x100000001b3ull;
    printf("\"%s\": \"%016llx\"%s", name, (unsigned long long)d, end);
}

static void edge_luma(int x0, int y0, int w, int h, int dx, int dy, int *first)
{
    ALIGN(16) static uint8_t dst[256] ALIGN2(16);
    point_t wh, dxdy;
    wh.u32 = 0; dxdy.u32 = 0;
    wh.s.x = (int16_t)w; wh.s.y = (int16_t)h; dxdy.s.x = (int16_t)dx; dxdy.s.y = (int16_t)dy;
    memset(dst, 0, sizeof(dst));
    h264e_qpel_interpolate_luma(PADP(x0, y0), PADS, dst, wh, dxdy);
    sep(first);
    printf("    {\"x\": %d, \"y\": %d, \"w\": %d, \"h\": %d, \"dx\": %d, \"dy\": %d, ", x0, y0, w, h, dx, dy);
    digwh("dst", dst, 16, w, h, "}");
}

static void edge_chroma(int x0, int y0, int w, int h, int dx, int dy, int *first)
{
    ALIGN(16) static uint8_t dst[256] ALIGN2(16);
    point_t wh, dxdy;
    wh.u32 = 0; dxdy.u32 = 0;
    wh.s.x = (int16_t)w; wh.s.y = (int16_t)h; dxdy.s.x = (int16_t)dx; dxdy.s.y = (int16_t)dy;
    memset(dst, 0, sizeof(dst));
    h264e_qpel_interpolate_chroma(PADP(x0, y0), PADS, dst, wh, dxdy);
    sep(first);
    printf("    {\"x\": %d, \"y\": %d, \"w\": %d, \"h\": %d, \"dx\": %d, \"dy\": %d, ", x0, y0, w, h, dx, dy);
    digwh("dst", dst, 16, w, h, "}");
}

/* one quantiser case: the flow of main()'s "quant" section on given input and prediction */
static void edge_quant(h264e_enc_t *enc, int qp, int p_slice, int mode, const uint8_t *inp_, const uint8_t *pred_, const char *what, int *first, int *maxlev)
{
    ALIGN(16) static uint8_t inp[16*16] ALIGN2(16), pred[16*16] ALIGN2(16), out[16*16] ALIGN2(16);
    static struct { int16_t dc[16]; quant_t q[16]; } Q, Qsnap;
    const int side = mode >> 1, nblk = (mode == QDQ_MODE_INTRA_4) ? 1 : side*side;
    int16_t deq_dc[16];
    int nz, dcflag = 0, k, b;
    memcpy(inp, inp_, 256); memcpy(pred, pred_, 256);
    enc->run_param.qp_min = enc->run_param.qp_max = (uint8_t)qp;
    enc->slice.type = p_slice ? SLICE_TYPE_P : SLICE_TYPE_I;
    enc->rc.qp = 0;
    rc_set_qp(enc, qp);
    memset(&Q, 0, sizeof(Q));
    memset(deq_dc, 0, sizeof(deq_dc));
    nz = h264e_transform_sub_quant_dequant(inp, pred, 16, mode, Q.q, enc->rc.qdat[mode == QDQ_MODE_CHROMA ? 1 : 0]);
    if (mode == QDQ_MODE_INTRA_16) h264e_quant_luma_dc(Q.q, deq_dc, enc->rc.qdat[0]);
    if (mode == QDQ_MODE_CHROMA) dcflag = h264e_quant_chroma_dc(Q.q, deq_dc, enc->rc.qdat[1]);
    memcpy(&Qsnap, &Q, sizeof(Q));
    memcpy(out, pred, sizeof(out));
    if (mode == QDQ_MODE_INTER) h264e_transform_add(out, 16, pred, Q.q, 4, nz << 16);
    else if (mode == QDQ_MODE_INTRA_16) h264e_transform_add(out, 16, pred, Q.q, 4, 0xFFFF << 16);
    else if (mode == QDQ_MODE_INTRA_4) { if (nz & 1) h264e_transform_add(out, 16, pred, Q.q, 1, ~0); }
    else if (dcflag | nz)
    {
        int m = nz, b4;
        if (dcflag)
        {
            for (b4 = 0; b4 < 4; b4++) if (~nz & (8 >> b4)) memset(Q.q[b4].dq + 1, 0, (16 - 1)*sizeof(int16_t));
            m = 15;
        }
        h264e_transform_add(out, 16, pred, Q.q, 2, m << 28);
    }
    for (b = 0; b < nblk; b++) for (k = 0; k < 16; k++) { int v = Qsnap.q[b].qv[k]; if (v < 0) v = -v; if (v > *maxlev) *maxlev = v; }
    for (k = 0; k < 16; k++) { int v = deq_dc[k]; if (v < 0) v = -v; if (v > *maxlev) *maxlev = v; }
    sep(first);
    printf("  {\"what\": \"%s\", \"qp\": %d, \"p_slice\": %d, \"mode\": %d, \"nz\": %d, \"dcflag\": %d,\n", what, qp, p_slice, mode, nz, dcflag);
    /* (the samples the mode works on: 4x4, 8x8 or all; the rest of `out` is the prediction) */
    printf("   "); hexwh("inp", inp, 16, 4*side, 4*side, ",\n   "); hexwh("pred", pred, 16, 4*side, 4*side, ",\n");
    printf("   "); hexwh("qdat", (const uint8_t *)enc->rc.qdat[mode == QDQ_MODE_CHROMA ? 1 : 0], 0, (int)sizeof(enc->rc.qdat[0]), 1, ", ");
    hexwh("dc", (const uint8_t *)Qsnap.dc, 0, (int)sizeof(Q.dc), 1, ", "); hexwh("deq_dc", (const uint8_t *)deq_dc, 0, (int)sizeof(deq_dc), 1, ",\n   ");
    hexwh("q", (const uint8_t *)Qsnap.q, 0, (int)sizeof(quant_t)*nblk, 1, ",\n   "); hexwh("out", out, 16, 4*side, 4*side, "\n");
    printf("  }");
}

static void edge_cavlc(const int16_t *q_in, int mn, int left, int top, int start, int *first)
{
    int16_t q[32];
    uint8_t nzc[3], buf[256];
    bs_t bs;
    unsigned nbits;
    memset(q, 0, sizeof(q));
    memcpy(q, q_in, 32);
    nzc[0] = (uint8_t)left; nzc[1] = 0xee; nzc[2] = (uint8_t)top;
    memset(buf, 0, sizeof(buf));
    h264e_bs_init_bits(&bs, buf);
    if (start) h264e_bs_put_bits(&bs, (unsigned)start, (1u << start) - 1u);
    h264e_vlc_encode(&bs, q, mn, nzc + 1);
    nbits = h264e_bs_get_pos_bits(&bs);
    h264e_bs_flush(&bs);
    sep(first);
    printf("  {\"maxn\": %d, \"left\": %d, \"top\": %d, \"start\": %d, \"nnz\": %d, \"nbits\": %u, ", mn, left, top, start, nzc[1], nbits);
    hexwh("coef", (const uint8_t *)q_in, 32, 32, 1, ", ");
    hexwh("bits", buf, 0, (int)((nbits + 7)/8), 1, "}");
}

/* a block with `total` coefficients of which the last t1 in coding order (highest indices) are +-1 */
static void cavlc_block_make(int16_t *q, int mn, int total, int t1)
{
    const int lo = mn == 15 ? 1 : 0, hi = mn == 4 ? 3 : 15;
    int k, zeros = mn - total, seen = 0;
    memset(q, 0, 32);
    for (k = hi; k >= lo; k--)
    {
        int v;
        if (zeros && seen && (rnd() % 3) == 0) { zeros--; continue; }
        if (k - lo + 1 <= zeros) { zeros--; continue; }
        if (seen < t1) v = 1;
        else if (seen == t1 && t1 < 3) v = 2 + (int)(rnd() % 3);
        else v = 1 + (int)(rnd() % 4);
        if (rnd() & 1) v = -v;
        q[k] = (int16_t)v;
        if (++seen == total) break;
    }
}

static void plane_make(uint8_t *p, int n, int org, int kind, int s0)
{
    int x, y;
    for (y = 0; y < n; y++)
        for (x = 0; x < n; x++)
        {
            const int bx = x >> 2, by = y >> 2, lev = (int)((unsigned)(bx*7 + by*13 + bx*by) % 4u);
            static const int lows[4] = { 0, 0, 6, 12 };
            int v;
            switch (kind)
            {
            case 0: v = lows[lev] + (int)(rnd() % 8); break;                                  /* near 0 */
            case 1: v = 255 - lows[lev] - (int)(rnd() % 8); break;                            /* near 255 */
            case 2: v = (x < n/2) ? lows[lev] + (int)(rnd() % 8) : 255 - lows[lev] - (int)(rnd() % 8); break;
            case 3: v = 100 + lev + (int)(rnd() % 2); break;                                  /* steps the first non-zero alpha still passes */
            case 4: v = x < org ? 100 : 100 + s0 + (y - org); break;                          /* a flat step across the left edge, one size per row */
            case 7: v = y < org ? 100 : 100 + s0 + (x - org);                                 /* ... across the top edge, the third sample off by 2..5 */
                    if (y == org - 3 || y == org + 2) v += ((x & 3) + 2)*((x & 4) ? -1 : 1);
                    break;
            case 9:
            {
                /* flat 0 (upper half) / 255 (lower half); at the left edge and the middle vertical edge the second sample before (p1) or
                 * after (q1) the edge is 7 off, alternating by block row: a normal filter's delta is then -+1 with p0 = q0 on the end of
                 * the range, so p0 + delta or q0 - delta leaves 0..255 and the clip has to act */
                const int base = y < n/2 ? 0 : 255, e0 = org, e1 = org + n/4, pat = ((y - org) >> (n == 32 ? 2 : 1)) & 1;
                v = base;
                if (pat ? (x == e0 + 1 || x == e1 + 1) : (x == e0 - 2 || x == e1 - 2)) v = base ? 248 : 7;
                break;
            }
            default: v = 128 + (lev - 2)*55 + (int)(rnd() % 61) - 30; break;                  /* blocky over the whole range */
            }
            p[y*n + x] = (uint8_t)clipi(v);
        }
}

/* index of the input macroblock whose corner / centre-line gradients add up to (X, Y), made on first use (no stored block: the test
 * builds the same) */
static int i16_block(uint8_t blocks[][256], int *bx, int *by, int *nb, int X, int Y)
{
    const int x1 = X/2 < 110 ? X/2 : 110, y1 = Y/2 < 110 ? Y/2 : 110;
    uint8_t *p = blocks[*nb];
    int j, k;
    for (j = 0; j < *nb; j++) if (bx[j] == X && by[j] == Y) return j;
    for (k = 0; k < 256; k++) p[k] = (uint8_t)(90 + (k*29 + X*7 + Y*13) % 41);
    p[0] = 0; p[15] = (uint8_t)x1; p[15*16] = (uint8_t)y1; p[15*16 + 15] = (uint8_t)(x1 + y1);
    p[8*16] = 0; p[8*16 + 15] = (uint8_t)(X - 2*x1); p[8] = 0; p[15*16 + 8] = (uint8_t)(Y - 2*y1);
    bx[*nb] = X; by[*nb] = Y;
    return (*nb)++;
}

static int edges(h264e_enc_t *enc)
{
    static uint8_t pic[64*64];
    int i, k, first, maxlev = 0;
    g_seed = 0x5eed0e;
    printf("{\n \"generator\": \"oracle/stage_harness.c edges against the reference header (h264-lab.h), make -C oracle stages\",\n");

    /* ---- footprints across the picture borders: the reference reads a copy padded by replication, the hooks the bare 64x64 picture */
    fill_pic(pic, 64, 64, 12);
    for (i = 0; i < 64; i++) memcpy(PADP(0, i), pic + 64*i, 64);
    h264e_copy_borders(PADP(0, 0), 64, 64, PADG);
    g_per_line = 4; printf(" \"border\": {\n");
    hex("pic", pic, sizeof(pic), 0);
    printf("   \"sad\": [\n");
    first = 1;
    {
        static const int pos[][2] = {
            {-14,20},{-8,21},{-5,22},{-4,23},{-3,24},{-1,25},{45,26},{48,27},{49,28},{50,29},{53,30},{56,31},{57,32},{58,33},{61,34},{62,35},
            {24,-14},{25,-8},{26,-5},{27,-4},{29,-3},{30,-1},{31,49},{33,51},{34,52},{35,53},{37,56},{38,62},
            {-14,-14},{62,62},{-3,62},{58,-5} };
        for (i = 0; i < (int)(sizeof(pos)/sizeof(pos[0])); i++)
        {
            ALIGN(16) static uint8_t blk[256] ALIGN2(16);
            int sad4[4], tot;
            const int x = pos[i][0], y = pos[i][1];
            /* the block: the padded picture one sample to the right and two down, low bits stirred (the test builds the same) */
            for (k = 0; k < 256; k++) blk[k] = (uint8_t)(*PADP(x + (k & 15) + 1, y + (k >> 4) + 2) ^ ((k*37) & 7));
            tot = h264e_sad_mb_unlaign_8x8(PADP(x, y), PADS, blk, sad4);
            sep(&first);
            printf("    {\"x\": %d, \"y\": %d, \"sad4\": [%d, %d, %d, %d], \"sad\": %d}", x, y, sad4[0], sad4[1], sad4[2], sad4[3], tot);
        }
    }
    printf("\n   ],\n   \"luma\": [\n");
    first = 1;
    {
        static const int anchor[6][2] = { {-10,20}, {58,24}, {22,-10}, {20,58}, {-10,-10}, {58,58} };
        static const int depth[5] = { 1, 3, 4, 5, 8 };
        static const int fr[5][2] = { {2,0}, {0,2}, {2,2}, {1,1}, {3,3} };
        static const int far[6][2] = { {-14,20}, {62,21}, {22,-14}, {23,62}, {-14,-14}, {62,62} };
        int a, d, s;
        for (a = 0; a < 6; a++) for (k = 0; k < 16; k++) edge_luma(anchor[a][0], anchor[a][1], 16, 16, k & 3, k >> 2, &first);
        for (d = 0; d < 5; d++)
            for (s = 0; s < 4; s++)
            {
                const int dd = depth[d], x0 = s == 0 ? -dd : s == 1 ? 48 + dd : 20 + dd, y0 = s == 2 ? -dd : s == 3 ? 48 + dd : 21 + dd;
                edge_luma(x0, y0, 16, 16, 0, 0, &first);
                edge_luma(x0, y0, 16, 16, fr[(d + s) % 5][0], fr[(d + s) % 5][1], &first);
            }
        for (a = 0; a < 6; a++) edge_luma(far[a][0], far[a][1], 16, 16, 0, 0, &first);
        for (k = 53; k <= 60; k++) { edge_luma(k, 30, 16, 16, 0, 0, &first); if (k <= 58) edge_luma(k, 30, 16, 16, 2, 0, &first); }
        for (s = 1; s < 4; s++)
            for (a = 0; a < 2; a++)           /* two opposite corners, the block half inside the picture */
                for (k = 0; k < 4; k++) edge_luma(a ? 59 : -3, a ? 58 : -2, (s & 2) ? 8 : 16, (s & 1) ? 8 : 16, 2*(k & 1), k & 2, &first);
    }
    printf("\n   ],\n   \"chroma\": [\n");
    first = 1;
    {
        static const int lo[5] = { -7, -5, -4, -3, -1 }, hi[5] = { 57, 59, 60, 61, 63 };
        int sz, n = 0;
        for (sz = 8; sz >= 4; sz -= 4)
        {
            for (k = 0; k < 10; k++, n++)
            {
                const int c = k < 5 ? lo[k] : hi[k - 5] + (8 - sz), dx = (n % 4 == 0) ? 0 : (int)(rnd() % 8), dy = (n % 4 == 1) ? 0 : (int)(rnd() % 8);
                edge_chroma(c, 20 + k, sz, sz, dx, dy, &first);
                edge_chroma(24 + k, c, sz, sz, dy, dx, &first);
            }
            edge_chroma(-7, -7, sz, sz, 3, 5, &first);
            edge_chroma(63 + (8 - sz), 63 + (8 - sz), sz, sz, 6, 1, &first);
        }
    }
    printf("\n   ]\n },\n");

    /* ---- transform / quantiser / reconstruction where the final clip acts */
    g_per_line = 1; printf(" \"quant\": [\n");
    first = 1;
    {
        static const int modes[] = { QDQ_MODE_INTER, QDQ_MODE_INTRA_16, QDQ_MODE_INTRA_4, QDQ_MODE_CHROMA };
        static const char *names[] = { "+255 qp10", "+255 qp51", "-255 qp10", "-255 qp51", "zero", "single +-1", "dc only", "near the range qp22", "near the range qp40" };
        static const int qps[] = { 10, 51, 10, 51, 26, 10, 26, 22, 40 };
        int scn, mi;
        for (scn = 0; scn < 9; scn++)
            for (mi = 0; mi < 4; mi++)
            {
                uint8_t inp[256], pred[256];
                for (k = 0; k < 256; k++)
                {
                    const int mid = 100 + (k & 15)*3 + (int)(rnd() % 9);
                    int p = mid, v = mid;
                    if (scn < 2) { p = 0; v = 255; }
                    else if (scn < 4) { p = 255; v = 0; }
                    else if (scn == 5) v = mid + (k == 5*16 + 6) - (k == 10*16 + 9) + (k == 0);
                    else if (scn == 6) v = mid + 5;
                    else if (scn >= 7)
                    {
                        const int amp = scn == 7 ? 30 : 90;
                        p = ((k >> 5) ^ (k >> 1)) & 1 ? 250 + (int)(rnd() % 6) : (int)(rnd() % 6);        /* 2x2 patches: both ends of the range in every 4x4 block */
                        v = p + (int)(rnd() % (unsigned)(2*amp + 1)) - amp;
                    }
                    pred[k] = (uint8_t)clipi(p); inp[k] = (uint8_t)clipi(v);
                }
                edge_quant(enc, qps[scn], modes[mi] == QDQ_MODE_INTER ? 1 : (scn & 1), modes[mi], inp, pred, names[scn], &first, &maxlev);
            }
    }
    printf("\n ],\n \"quant_max_level\": %d,\n", maxlev);

    /* ---- CAVLC: 13..16 coefficients, every count of trailing ones, the four table ranges, levels through the escape codes, mid-word starts */
    g_per_line = 4; printf(" \"cavlc\": [\n");
    first = 1;
    {
        static const int ctx[4][2] = { {0, 0}, {2, 3}, {5, 6}, {9, 12} };
        int16_t q[16];
        int n = 0, total, t1, c, m;
        for (total = 13; total <= 16; total++)
            for (t1 = 0; t1 < 4; t1++)
                for (c = 0; c < 4; c++, n++) { cavlc_block_make(q, 16, total, t1); edge_cavlc(q, 16, ctx[c][0], ctx[c][1], n % 32, &first); }
        for (total = 13; total <= 15; total++)
            for (t1 = 0; t1 < 4; t1++, n++) { cavlc_block_make(q, 15, total, t1); edge_cavlc(q, 15, ctx[n % 4][0], ctx[n % 4][1], n % 32, &first); }
        for (t1 = 0; t1 < 4; t1++, n++) { cavlc_block_make(q, 4, 4, t1); edge_cavlc(q, 4, 17, 17, n % 32, &first); }
        {
            int mags[32], nm = 0;
            static const int fixed[] = { 2, 3, 7, 8, 15, 16, 31, 32, 33, 64, 255 };
            for (k = 0; k < (int)(sizeof(fixed)/sizeof(fixed[0])); k++) if (fixed[k] < maxlev) mags[nm++] = fixed[k];
            mags[nm++] = maxlev - 1; mags[nm++] = maxlev;
            for (m = 0; m < nm; m++)
            {
                const int v = (m & 1) ? -mags[m] : mags[m];
                /* coding order runs from index 15 down: the level under test first / after three trailing ones / first of twelve */
                memset(q, 0, sizeof(q)); q[9] = (int16_t)v;
                edge_cavlc(q, 16, ctx[m % 4][0], ctx[m % 4][1], n++ % 32, &first);
                memset(q, 0, sizeof(q)); q[15] = 1; q[13] = -1; q[12] = 1; q[8] = (int16_t)v; q[3] = (int16_t)-v;
                edge_cavlc(q, 16, ctx[(m + 1) % 4][0], ctx[(m + 1) % 4][1], n++ % 32, &first);
                for (k = 0; k < 16; k++) q[k] = (int16_t)(k >= 4 ? ((k & 1) ? 15 - k + 2 : -(15 - k + 2)) : 0);
                q[15] = (int16_t)v;
                edge_cavlc(q, 16, ctx[(m + 2) % 4][0], ctx[(m + 2) % 4][1], n++ % 32, &first);
            }
        }
    }
    printf("\n ],\n");

    /* ---- intra 4x4: directional content over the whole sample range, kept until every mode has been chosen 8 times */
    g_per_line = 4; printf(" \"intra4\": [\n");
    first = 1;
    {
        int count[9] = { 0 }, kept = 0;
        static const int dir[8][2] = { {1,0}, {0,1}, {1,1}, {1,-1}, {2,1}, {1,2}, {2,-1}, {1,-2} };
        static const int levels[6] = { 0, 255, 40, 200, 128, 90 };
        for (i = 0; i < 20000 && kept < 9*8; i++)
        {
            ALIGN(16) static uint8_t in4[16*4] ALIGN2(16), pr4[16*4] ALIGN2(16);
            ALIGN(4) uint8_t edge_store[16] ALIGN2(4);
            uint8_t edge_in[16];
            const int *d = dir[rnd() % 8];
            const int period = 2 + (int)(rnd() % 4), phase = (int)(rnd() % 8), lo = levels[rnd() % 6], hi = levels[rnd() % 6], noise = (int)(rnd() % 4), soft = (int)(rnd() % 3) == 0;
            const int avail = (i < 32) ? i % 16 : ((rnd() % 4) ? 15 : (int)(rnd() % 16)), mpred = (int)(rnd() % 9), penalty = (i % 5 == 0) ? 0 : (int)(rnd() % 40);
            int ret, x, y, mode;
#define F(x, y) clipi((soft ? lo + (hi - lo)*(((d[0]*(x) + d[1]*(y) + phase + 64) % (2*period)))/(2*period) : ((((d[0]*(x) + d[1]*(y) + phase + 64)/period) & 1) ? hi : lo)) + (noise ? (int)(rnd() % (unsigned)(2*noise + 1)) - noise : 0))
            memset(edge_store, 0, sizeof(edge_store));
            for (k = 0; k < 4; k++) edge_store[k] = (uint8_t)F(-1, 3 - k);
            edge_store[4] = (uint8_t)F(-1, -1);
            for (k = 0; k < 8; k++) edge_store[5 + k] = (uint8_t)F(k, -1);
            memset(in4, 0, sizeof(in4)); memset(pr4, 0, sizeof(pr4));
            for (y = 0; y < 4; y++) for (x = 0; x < 4; x++) in4[16*y + x] = (uint8_t)F(x, y);
#undef F
            memcpy(edge_in, edge_store, sizeof(edge_in));
            ret = h264e_intra_choose_4x4(in4, pr4, avail, edge_store + 5, mpred, penalty);
            mode = ret & 15;
            if (mode > 8 || count[mode] >= 8) continue;
            count[mode]++; kept++;
            sep(&first);
            printf("  {\"avail\": %d, \"mpred\": %d, \"penalty\": %d, \"mode\": %d, \"cost\": %d, ", avail, mpred, penalty, mode, ret >> 4);
            hexwh("edge", edge_in, 0, 13, 1, ", ");
            hexwh("in", in4, 16, 4, 4, ", ");
            hexwh("pred", pr4, 16, 4, 4, "}");
        }
    }
    printf("\n ],\n");

    /* ---- deblocking: samples at both ends of the range, table indices at the first non-zero entries, far-apart QPs, flat steps around
     * the strong-filter conditions.  Printed: the macroblock with 4 (luma) / 2 (chroma) samples of its left and top neighbours */
    g_per_line = 1; printf(" \"deblock\": [\n");
    first = 1;
    {
        /* mb_type, left type, top type, qp, qp_left, qp_top, flags (0 none, 1 random, 2 all), vectors (0 equal, 1 some differ), picture kind, first step */
        static const int sc[][10] = {
            {5,0,0, 51,51,51, 0,0, 0,0}, {6,5,5, 51,51,51, 0,0, 1,0}, {0,0,0, 51,51,51, 1,1, 0,0}, {1,0,5, 45,48,51, 2,1, 2,0},
            {5,0,0, 16,16,16, 0,0, 3,0}, {5,0,0, 15,15,15, 0,0, 3,0},
            {5,0,0, 10,51,51, 0,0, 8,0}, {0,5,5, 51,10,10, 1,1, 8,0},
            {5,0,0, 24,24,24, 0,0, 4,1}, {5,0,0, 32,32,32, 0,0, 7,2},
            {2,0,6, 36,36,40, 1,1, 8,0}, {0,0,0, 51,51,51, 2,0, 9,0}, {1,0,0, 45,45,45, 2,0, 9,0} };
        for (i = 0; i < (int)(sizeof(sc)/sizeof(sc[0])); i++)
        {
            static uint8_t Yp[32*32], Up[16*16], Vp[16*16], Yin[32*32], Uin[16*16], Vin[16*16];
            deblock_filter_t df, df2;
            uint8_t dfqp[4], dfqp2[4], dfnz[4], dfnz2[4], strength[32];
            int8_t mbt[4], mbt2[4];
            H264E_io_yuv_t io;
            const int *s = sc[i], mb_type = s[0], qp = s[3];
            memset(&df, 0, sizeof(df));
            df.df_qp = dfqp + 1; df.mb_type = mbt + 1; df.df_nzflag = dfnz + 1;
            for (k = 0; k < 4; k++) { dfqp[k] = (uint8_t)qp; mbt[k] = 0; dfnz[k] = (uint8_t)(rnd() % 16); }
            dfqp[1] = (uint8_t)s[4]; dfqp[2] = (uint8_t)s[5]; mbt[1] = (int8_t)s[1]; mbt[2] = (int8_t)s[2];
            df.nzflag = s[6] == 0 ? 0 : s[6] == 2 ? 0x1ffffff : (rnd() & rnd() & 0x1ffffff);
            for (k = 0; k < 24; k++)
            {
                df.df_mv[k].s.x = (int16_t)(8 + (s[7] && (rnd() % 3) == 0 ? (int)(rnd() % 9) - 4 : 0));
                df.df_mv[k].s.y = (int16_t)(-4 + (s[7] && (rnd() % 3) == 0 ? (int)(rnd() % 9) - 4 : 0));
            }
            plane_make(Yp, 32, 8, s[8], s[9]); plane_make(Up, 16, 4, s[8], s[9]); plane_make(Vp, 16, 4, s[8] == 0 ? 1 : s[8], s[9] + 1);
            if (s[8] == 9) for (k = 0; k < 16*16; k++) Vp[k] = (uint8_t)(255 - Vp[k]);               /* V: the ends of the range the other way up */
            memcpy(Yin, Yp, sizeof(Yp)); memcpy(Uin, Up, sizeof(Up)); memcpy(Vin, Vp, sizeof(Vp));
            df2 = df; memcpy(dfqp2, dfqp, 4); memcpy(mbt2, mbt, 4); memcpy(dfnz2, dfnz, 4);
            df2.df_qp = dfqp2 + 1; df2.mb_type = mbt2 + 1; df2.df_nzflag = dfnz2 + 1;
            memset(strength, 0, sizeof(strength));
            df_strength(&df2, mb_type, 1, strength, 0);
            io.yuv[0] = Yp + 8*32 + 8; io.yuv[1] = Up + 4*16 + 4; io.yuv[2] = Vp + 4*16 + 4;
            io.stride[0] = 32; io.stride[1] = 16; io.stride[2] = 16;
            mb_deblock(&df, mb_type, qp, 1, 1, &io, 0);
            sep(&first);
            printf("  {\"mb_type\": %d, \"qp\": %d, \"qp_left\": %d, \"qp_top\": %d, \"kind\": %d,\n   ", mb_type, qp, s[4], s[5], s[8]);
            hexwh("bs", strength, 0, 32, 1, ",\n   ");
            hexwh("y_in", Yin + 4*32 + 4, 32, 20, 20, ",\n   "); hexwh("u_in", Uin + 2*16 + 2, 16, 10, 10, ", "); hexwh("v_in", Vin + 2*16 + 2, 16, 10, 10, ",\n   ");
            hexwh("y_out", Yp + 4*32 + 4, 32, 20, 20, ",\n   "); hexwh("u_out", Up + 2*16 + 2, 16, 10, 10, ", "); hexwh("v_out", Vp + 2*16 + 2, 16, 10, 10, "\n  }");
        }
    }
    printf("\n ],\n");

    /* ---- motion search with tight limits: true motion beyond them, starts on them, results on the range; and, per side of the sub-sample
     * limit, a full-sample result exactly on it (the seven sub-sample probes are taken and change the result) and one a sample beyond it
     * (none is taken, though they would change it).  The full-sample result is what the same search returns without its sub-sample part
     * (speed 9), "would change it" what it returns with the sub-sample limit opened up to the vector limit. */
    {
        static uint8_t ref[96*96];
        int x, y, n_edge = 0, n_q = 0, n_other = 0, shape[9] = { 0 }, qdone[4][2] = { {0} };
        for (y = 0; y < 96; y++)
            for (x = 0; x < 96; x++)
            {
                int a = (x*4 + y*2) % 64, b = (y*4 - x + 960) % 48, v;
                a = a < 32 ? a : 63 - a; b = b < 24 ? b : 47 - b;
                v = 60 + 3*a + 2*b + (x*131 + y*71) % 5;              /* (no stored picture: the test builds the same) */
                ref[y*96 + x] = (uint8_t)(v > 255 ? 255 : v);
            }
        g_per_line = 1; printf(" \"diamond\": [\n");
        first = 1;
        for (i = 0; i < 40000 && (n_edge < 9 || n_q < 8 || n_other < 2); i++)
        {
            ALIGN(16) static uint8_t cur[256] ALIGN2(16), store[8*256] ALIGN2(16);
            static const int parts[9][4] = { {0,0,16,16}, {0,0,16,8}, {0,8,16,8}, {0,0,8,16}, {8,0,8,16}, {0,0,8,8}, {8,0,8,8}, {0,8,8,8}, {8,8,8,8} };
            const int *pt = parts[i % 9], px = pt[0], py = pt[1], w = pt[2], h = pt[3];
            /* every second candidate is aimed at one side of the sub-sample limit: its true motion a quarter or three quarters of a sample
             * from the full-sample position (fx, fy) on that side (qbeyond: one sample outside it) */
            const int aimed = (i & 1) && n_q < 8, qside = (i >> 1) & 3, qbeyond = (i >> 3) & 1;
            int tx = (int)(rnd() % 17) - 8, ty = (int)(rnd() % 17) - 8, qx = (int)(rnd() % 4), qy = (int)(rnd() % 4);
            const int qp = 18 + (int)(rnd() % 24), noise = aimed ? 0 : (int)(rnd() % 4), speed = (!aimed && i % 16 == 15) ? 9 : 0;
            const int lmin = aimed ? 6 : 2, lvar = aimed ? 4 : 8;
            const int la = lmin + (int)(rnd() % lvar), lb = lmin + (int)(rnd() % lvar), lc = lmin + (int)(rnd() % lvar), ld = lmin + (int)(rnd() % lvar), st = aimed ? 3 : (int)(rnd() % 4);
            point_t mv, mv_pred, wh, dd, mv_in, fs, wide;
            rectangle_t range, ql;
            pix_t *pbest = 0, *pb2 = 0;
            int ret, min_sad, min_sad_in, sx, sy, on_edge, fx = 0, fy = 0;
            if (aimed)
            {
                if (qdone[qside][qbeyond]) continue;
                fx = qside == 0 ? -la + 4 - qbeyond : qside == 1 ? lc - 4 + qbeyond : (int)(rnd() % 3) - 1;
                fy = qside == 2 ? -lb + 4 - qbeyond : qside == 3 ? ld - 4 + qbeyond : (int)(rnd() % 3) - 1;
                qx = (rnd() & 1) ? 1 : 3; qy = (rnd() & 1) ? 1 : 3;
                tx = fx - (qx == 3); ty = fy - (qy == 3);
            }
            wh.u32 = 0; wh.s.x = 16; wh.s.y = 16; dd.u32 = 0; dd.s.x = (int16_t)qx; dd.s.y = (int16_t)qy;
            h264e_qpel_interpolate_luma(ref + (32 + ty)*96 + 32 + tx, 96, cur, wh, dd);
            for (k = 0; k < 256; k++) cur[k] = (uint8_t)clipi(cur[k] + (noise ? (int)(rnd() % (unsigned)(2*noise + 1)) - noise : 0));
            enc->run_param.encode_speed = speed;
            enc->frame.mv_limit.tl = point((32 - la)*4, (32 - lb)*4); enc->frame.mv_limit.br = point((32 + lc)*4, (32 + ld)*4);
            enc->frame.mv_qpel_limit.tl = mv_add(enc->frame.mv_limit.tl, point(4*4, 4*4));
            enc->frame.mv_qpel_limit.br = mv_add(enc->frame.mv_limit.br, point(-4*4, -4*4));
            sx = tx + (int)(rnd() % 5) - 2; sy = ty + (int)(rnd() % 5) - 2;
            if (st == 0) { sx = -la; sy = -lb; } else if (st == 1) { sx = lc; sy = (int)(rnd() % 3) - 1; } else if (st == 2) { sx = 0; sy = 0; }
            mv = point((32 + sx)*4, (32 + sy)*4);
            me_mv_set_range(&mv, &range, &enc->frame.mv_limit, 32*4 + py*4);
            mv_in = mv;
            mv_pred = point((32 + tx)*4 + (int)(rnd() % 17) - 8, (32 + ty)*4 + (int)(rnd() % 17) - 8);
            wh.s.x = (int16_t)w; wh.s.y = (int16_t)h;
            min_sad = h264e_sad_mb_unlaign_wh(ref + ((mv.s.y >> 2) + py)*96 + (mv.s.x >> 2) + px, 96, cur + py*16 + px, wh) + me_mv_cost(mv, mv_pred, qp);
            if (i % 4 == 1) min_sad = 0x7fffff;
            min_sad_in = min_sad;
            memset(store, 0, sizeof(store));
#define SEARCH(mvp, pb) me_search_diamond(enc, ref + py*96 + px, cur + py*16 + px, 96, mvp, &range, qp, mv_pred, min_sad, wh, store, pb, \
                                    (w == 16 && h == 16) ? 256 : (w == 8 && h == 16) ? 8 : 128)
            fs = wide = mv;
            if (aimed)
            {
                enc->run_param.encode_speed = 9; SEARCH(&fs, &pb2);
                ql = enc->frame.mv_qpel_limit; enc->frame.mv_qpel_limit = enc->frame.mv_limit;
                enc->run_param.encode_speed = 0; SEARCH(&wide, &pb2);
                enc->frame.mv_qpel_limit = ql;
                memset(store, 0, sizeof(store));
            }
            ret = SEARCH(&mv, &pbest);
#undef SEARCH
            on_edge = mv.s.x == range.tl.s.x || mv.s.x == range.br.s.x || mv.s.y == range.tl.s.y || mv.s.y == range.br.s.y;
            if (aimed)
            {
                if (fs.s.x != (32 + fx)*4 || fs.s.y != (32 + fy)*4 || wide.u32 == fs.u32 || (qbeyond ? mv.u32 != fs.u32 : mv.u32 == fs.u32)) continue;
                qdone[qside][qbeyond] = 1; n_q++;
            } else
            {
                if (on_edge ? shape[i % 9] >= 1 : n_other >= 2) continue;
                if (on_edge) { n_edge++; shape[i % 9]++; } else n_other++;
            }
            sep(&first);
            printf("  {\"px\": %d, \"py\": %d, \"w\": %d, \"h\": %d, \"qp\": %d, \"speed\": %d, \"mv_in\": [%d, %d], \"mv_pred\": [%d, %d], \"min_sad_in\": %d,\n"
                   "   \"range\": [%d, %d, %d, %d], \"limit\": [%d, %d, %d, %d], \"on_edge\": %d, \"qside\": %d, \"qbeyond\": %d, \"fs_mv\": [%d, %d],\n", px, py, w, h, qp, speed,
                   mv_in.s.x, mv_in.s.y, mv_pred.s.x, mv_pred.s.y, min_sad_in, range.tl.s.x, range.tl.s.y, range.br.s.x, range.br.s.y,
                   enc->frame.mv_limit.tl.s.x, enc->frame.mv_limit.tl.s.y, enc->frame.mv_limit.br.s.x, enc->frame.mv_limit.br.s.y, on_edge, aimed ? qside : -1, aimed ? qbeyond : 0, fs.s.x, fs.s.y);
            printf("   \"cost\": %d, \"mv\": [%d, %d], ", ret, mv.s.x, mv.s.y);
            hexwh("cur", cur, 16, 16, 16, ",\n   ");
            hexwh("pred", pbest, 16, w, h, "\n  }");
        }
        enc->run_param.encode_speed = 0;
        printf("\n ],\n");
    }

    /* ---- intra 16x16: the gradient thresholds of the mode estimate, every availability, edges where the DC sum rounds */
    {
        static uint8_t blocks[32][256];
        int nb = 0, bx[32], by[32], qi, c, n = 0;
        static const int qps[3] = { 10, 26, 51 };
        struct { int b, qp; } cs[64];
        int ncs = 0;
        for (qi = 0; qi < 3; qi++)
            for (c = 0; c < 12; c++)
            {
                /* a: second gradient 6, first at 30 + 3*6 - 1, +0, +1; b: second at 150 - qp - 1, +0, +1 with the first just above 30 + 3*second; x first, then y first */
                const int g2 = (c % 6) < 3 ? 6 : 150 - qps[qi] - 1 + (c % 3), g1 = (c % 6) < 3 ? 30 + 3*6 - 1 + (c % 3) : 30 + 3*g2 + 2;
                int idx;
                idx = c < 6 ? i16_block(blocks, bx, by, &nb, g1, g2) : i16_block(blocks, bx, by, &nb, g2, g1);
                cs[ncs].b = idx; cs[ncs++].qp = qps[qi];
            }
        cs[ncs].b = i16_block(blocks, bx, by, &nb, 0, 0); cs[ncs++].qp = 26;
        printf(" \"intra16_blocks\": [\n");
        for (k = 0; k < nb; k++) printf("%s{\"dx\": %d, \"dy\": %d}%s", k % 8 ? " " : "  ", bx[k], by[k], k == nb - 1 ? "\n" : k % 8 == 7 ? ",\n" : ",");
        g_per_line = 4; printf(" ],\n \"intra16\": [\n");
        first = 1;
        for (c = 0; c < ncs + 9 + 23; c++)
        {
            /* every threshold case with both neighbours, nine of them again with the availability rotating, then the flat block: availability x edge set */
            const int ci = c < ncs ? c : c < ncs + 9 ? 4*(c - ncs) + 2 : ncs - 1;
            const int avail = c < ncs - 1 ? ((c & 1) ? 7 : 3) : c < ncs ? 0 : c < ncs + 9 ? (c - ncs) % 3 : ((c - ncs - 9 + 1) & 3) | ((c & 8) ? 4 : 0);
            const int es = c < ncs + 9 ? n++ % 6 : (c - ncs - 9 + 1) >> 2;
            ALIGN(16) uint8_t left[16] ALIGN2(16), top[16] ALIGN2(16);
            int sl = 0, stp = 0;
            for (k = 0; k < 16; k++)
            {
                left[k] = (uint8_t)(es == 0 ? 0 : es == 1 ? 255 : es == 2 ? 0 : 60 + rnd() % 120);
                top[k] = (uint8_t)(es == 0 ? 0 : es == 1 ? 255 : es == 2 ? 255 : 60 + rnd() % 120);
            }
            if (es >= 4)
            {
                /* sums that sit exactly on the rounding step: top = 8 (mod 16), left = 8 (mod 16) (es 4) or 7 (es 5) */
                for (k = 0; k < 16; k++) { sl += left[k]; stp += top[k]; }
                top[3] = (uint8_t)(top[3] + ((8 - stp) & 15)); left[5] = (uint8_t)(left[5] + (((es == 4 ? 8 : 7) - sl) & 15));
            }
            memcpy(enc->scratch->mb_pix_inp, blocks[cs[ci].b], 256);
            enc->run_param.qp_min = enc->run_param.qp_max = (uint8_t)cs[ci].qp;
            enc->rc.qp = 0;
            rc_set_qp(enc, cs[ci].qp);
            enc->pbest = enc->scratch->mb_pix_store; enc->ptest = enc->pbest + 256;
            memset(enc->pbest, 0, 512);
            enc->mb.cost = 0x7fffffff; enc->mb.type = 0;
            intra_choose_16x16(enc, (avail & 2) ? left : NULL, (avail & 1) ? top : NULL, avail);
            sep(&first);
            printf("  {\"block\": %d, \"avail\": %d, \"qp\": %d, \"mode\": %d, \"cost\": %d, ", cs[ci].b, avail, cs[ci].qp, enc->mb.i16.pred_mode_luma, enc->mb.cost);
            hexwh("left", left, 0, 16, 1, ", "); hexwh("top", top, 0, 16, 1, ", ");
            digwh("pred", enc->pbest, 16, 16, 16, "}");
        }
        printf("\n ],\n");
    }

    /* ---- chroma prediction: three modes, four availabilities for DC, every quadrant's neighbours different */
    g_per_line = 2; printf(" \"pred_chroma\": [\n");
    first = 1;
    {
        static const int mode_av[][2] = { {0,1}, {0,3}, {1,2}, {1,3}, {2,0}, {2,1}, {2,2}, {2,3}, {2,7}, {2,15} };
        int es, c;
        for (es = 0; es < 2; es++)
            for (c = 0; c < 10; c++)
            {
                ALIGN(16) uint8_t left[16] ALIGN2(16), top[16] ALIGN2(16), pred[128] ALIGN2(16);
                const int mode = mode_av[c][0], avail = mode_av[c][1];
                for (k = 0; k < 16; k++)
                {
                    left[k] = (uint8_t)(es == 0 ? 10 + 40*(k >> 2) + (int)(rnd() % 4) : (k >> 2) & 1 ? 255 : 0);
                    top[k] = (uint8_t)(es == 0 ? 170 + 27*(k >> 2) + (int)(rnd() % 4) : (k >> 2) == 1 || (k >> 2) == 2 ? 0 : 255);
                }
                memset(pred, 0, sizeof(pred));
                h264e_intra_predict_chroma(pred, (avail & 2) ? left : NULL, (avail & 1) ? top : NULL, mode);
                sep(&first);
                printf("  {\"mode\": %d, \"avail\": %d, ", mode, avail);
                hexwh("left", left, 0, 16, 1, ", "); hexwh("top", top, 0, 16, 1, ", ");
                hexwh("pred", pred, 16, 16, 8, "}");
            }
    }
    printf("\n ],\n");

    /* ---- the median vector predictor: one macroblock per case, its partitions in coding order (get, then put) */
    g_per_line = 3; printf(" \"mvp\": [\n");
    first = 1;
    {
        static const int parts[4][4][4] = { { {0,0,4,4} }, { {0,0,4,2}, {0,2,4,2} }, { {0,0,2,4}, {2,0,2,4} }, { {0,0,2,2}, {2,0,2,2}, {0,2,2,2}, {2,2,2,2} } };
        static const int np[4] = { 1, 2, 2, 4 };
        static const int16_t pool[][2] = { {0,0}, {4,-4}, {-56,-56}, {248,184}, {-3,7}, {-128,127}, {511,-512}, {1,0}, {0,-1}, {-2047,2047}, {32767,-32767}, {12,12} };
        const int npool = (int)(sizeof(pool)/sizeof(pool[0]));
        static point_t store[8 + 4*4 + 8];         /* left 4 | top-left 4 | the top row, four per macroblock column (h264-lab.h:3649-3715) */
        int flag, t, v, j;
        enc->mv_pred = store;
        for (flag = 0; flag < 16; flag++)
                for (t = 0; t < 4; t++)
                {
                    v = (flag + t) % 3;
                    int ctx[13], mvs[4], preds[4], after[13];
                    for (j = 0; j < 13; j++)
                    {
                        const int16_t *pv = pool[rnd() % (unsigned)npool];
                        point_t p = point(pv[0], pv[1]);
                        if (v == 0 ? (rnd() % 3) == 0 : (rnd() % 6) == 0) p.u32 = MV_NA;          /* an intra neighbour */
                        enc->mv_pred[j] = p;
                    }
                    if (v == 1) { enc->mv_pred[8] = enc->mv_pred[0]; enc->mv_pred[12] = enc->mv_pred[9]; enc->mv_pred[4] = enc->mv_pred[11]; }      /* equal pairs */
                    if (v == 2) for (j = 0; j < 13; j++) if (enc->mv_pred[j].u32 != MV_NA && (j & 1)) enc->mv_pred[j] = point(pool[9 + (j >> 1) % 2][0], pool[9 + (j >> 2) % 2][1]);
                    for (j = 0; j < 13; j++) ctx[j] = (int)enc->mv_pred[j].u32;
                    enc->mb.x = 0; enc->mb.avail = flag;
                    for (j = 0; j < np[t]; j++)
                    {
                        const int *r = parts[t][j];
                        const int16_t *pv = pool[rnd() % (unsigned)npool];
                        const point_t mv = point(pv[0], pv[1]);
                        preds[j] = (int)me_mv_medianpredictor_get(enc, point(4*r[0], 4*r[1]), point(4*r[2], 4*r[3])).u32;
                        mvs[j] = (int)mv.u32;
                        me_mv_medianpredictor_put(enc, r[0], r[1], r[2], r[3], mv);
                    }
                    for (j = 0; j < 13; j++) after[j] = (int)enc->mv_pred[j].u32;
                    sep(&first);
                    printf("  {\"avail\": %d, \"type\": %d, ", flag, t);
                    ints("ctx", ctx, 13, ", "); ints("mv", mvs, np[t], ", "); ints("pred", preds, np[t], ", "); ints("after", after, 13, "}");
                }
    }
    printf("\n ],\n");

    /* ---- boundary strengths of df_strength, the left column cleared at mbx = 0 and the top row at a slice's top as mb_deblock does */
    g_per_line = 4; printf(" \"strength\": [\n");
    first = 1;
    {
        static const int types[7] = { -1, 0, 1, 2, 3, 5, 6 };
        static const int pos[3] = { 3, 9, 15 };           /* above, left of, inside the macroblock */           /* positions k of the 5x5 vector array whose vector is changed */
        int c, ncase = 49 + 25 + 3*8 + 12;
        for (c = 0; c < ncase; c++)
        {
            deblock_filter_t df;
            uint8_t dfqp[4], dfnz[4], strength[32];
            int8_t mbt[4];
            int mb_type = 0, lt = 0, tt = 0, mbx = 1, slice_top = 0, diff = 0, mvv[24];
            memset(&df, 0, sizeof(df)); memset(dfqp, 26, 4); memset(dfnz, 0, 4);
            df.df_qp = dfqp + 1; df.mb_type = mbt + 1; df.df_nzflag = dfnz + 1;
            for (k = 0; k < 24; k++) df.df_mv[k] = point(8, -4);
            if (c < 49) { mb_type = types[c / 7]; lt = types[c % 7]; tt = types[(c / 7 + 3*(c % 7)) % 7]; }
            else if (c < 74) df.nzflag = 1u << (c - 49);
            else if (c < 98)
            {
                /* one vector off by exactly 3 or 4, in x or in y, either sign */
                const int j = c - 74, kk = pos[j / 8], d = ((j & 1) ? 4 : 3)*((j & 4) ? -1 : 1);
                if (j & 2) df.df_mv[kk].s.y = (int16_t)(df.df_mv[kk].s.y + d); else df.df_mv[kk].s.x = (int16_t)(df.df_mv[kk].s.x + d);
                diff = (j & 1) ? 4 : 3;
            } else
            {
                const int j = c - 98;
                mb_type = types[1 + j % 6]; lt = types[(j + 3) % 7]; tt = types[(j + 5) % 7];
                if (j < 6) mbx = 0; else slice_top = 1;
                df.nzflag = rnd() & rnd() & 0x1ffffff;
                for (k = 0; k < 24; k++) if ((rnd() % 4) == 0) df.df_mv[k].s.x = (int16_t)(df.df_mv[k].s.x + (int)(rnd() % 9) - 4);
            }
            mbt[0] = mbt[1] = mbt[2] = mbt[3] = 0;
            mbt[mbx] = (int8_t)lt; mbt[mbx + 1] = (int8_t)tt;
            for (k = 0; k < 24; k++) mvv[k] = (int)df.df_mv[k].u32;
            memset(strength, 0, sizeof(strength));
            {
                const unsigned nz = df.nzflag;
                df_strength(&df, mb_type, mbx, strength, 0);
                /* what mb_deblock does with them before it filters (h264-lab.h:5653-5661; mby = 0 also stands for a slice's top row, 5799-5808);
                 * mb_deblock keeps the strengths to itself, so these two lines are the harness's own */
                if (!mbx) memset(strength, 0, 4);
                if (slice_top) memset(strength + 16, 0, 4);
                sep(&first);
                printf("  {\"type\": %d, \"left\": %d, \"top\": %d, \"x\": %d, \"slice_top\": %d, \"nz\": %u, \"diff\": %d, ", mb_type, lt, tt, mbx, slice_top, nz, diff);
            }
            if (c >= 74) ints("mv", mvv, 24, ", ");            /* (the others: every vector (8, -4)) */
            hexwh("bs", strength, 0, 32, 1, "}");
        }
    }
    printf("\n ],\n");

    /* ---- scalars of the decision */
    {
        int cls[12] = { 0 }, kept = 0, sads[96][4], modes[96][4];
        for (i = 0; i < 200000 && kept < 72; i++)
        {
            int sad[4], mode[4] = { 0, 0, 0, 0 }, sum, slope, skew, T, c = -1;
            const int scale = (i & 1) ? 40 : 4000;
            for (k = 0; k < 4; k++) sad[k] = (int)(rnd() % (unsigned)scale) + ((i & 2) ? scale : 0);
            sum = sad[0] + sad[1] + sad[2] + sad[3]; T = sum >> 4;
            slope = abs((sad[0] - sad[2]) + (sad[1] - sad[3])) - abs((sad[0] - sad[1]) + (sad[2] - sad[3]));
            skew = abs(abs(sad[3] - sad[0]) - abs(sad[2] - sad[1]));
            /* CHOICE of the candidates only (the expected flags come from the call below): this restates mb_inter_partition's three figures to
             * find quadruples AT its thresholds, which its four output flags alone cannot tell from quadruples far from them.
             * which threshold this quadruple sits at: slope - T, slope + T, |skew| - T in -1, 0, 1 (the latter with |slope| <= T), |slope| - T in 0, 1 with |skew| > T */
            if (slope - T >= -1 && slope - T <= 1) c = slope - T + 1;
            else if (slope + T >= -1 && slope + T <= 1) c = 3 + slope + T + 1;
            else if (skew - T >= -1 && skew - T <= 1 && abs(slope) <= T) c = 6 + skew - T + 1;
            if (skew > T && (abs(slope) - T == 0 || abs(slope) - T == 1)) c = 9 + abs(slope) - T;
            if (c < 0) { if ((i % 1000) != 7) continue; c = 11; }
            if (cls[c] >= 6) continue;
            cls[c]++;
            mb_inter_partition(sad, mode);
            memcpy(sads[kept], sad, sizeof(sad)); memcpy(modes[kept], mode, sizeof(mode)); kept++;
        }
        printf(" \"hints\": [\n");
        for (i = 0; i < kept; i++) { printf("%s{", i % 4 ? " " : "  "); ints("sad", sads[i], 4, ", "); ints("mode", modes[i], 4, i == kept - 1 ? "}\n" : i % 4 == 3 ? "},\n" : "},"); }
        printf(" ],\n");
    }
    {
        int diffs[64], nd = 0, qp;
        diffs[nd++] = 0;
        for (k = 0; k <= 9; k++) { const int p = 1 << k; diffs[nd++] = p; diffs[nd++] = -p; if (k > 1) { diffs[nd++] = p - 1; diffs[nd++] = -(p - 1); } }
        printf(" \"mv_cost\": {\"pred\": [13, -7], "); ints("diffs", diffs, nd, ",\n  \"cost\": [\n");
        for (qp = 10; qp <= 51; qp++)
        {
            /* y differs by entry k, x by entry k + qp */
            printf("   [");
            for (k = 0; k < nd; k++) printf("%s%d", k ? "," : "", me_mv_cost(point(13 + diffs[(k + qp) % nd], -7 + diffs[k]), point(13, -7), qp));
            printf("]%s\n", qp == 51 ? "" : ",");
        }
        printf("  ]\n },\n");
    }

    /* ---- the bit writer from every bit offset: kind 0 put (value, length), 1 golomb, 2 signed golomb */
    g_per_line = 4; printf(" \"bitwriter\": [\n");
    first = 1;
    {
        int off, s, c;
        static const int uev[] = { 0, 1, 2, 3, 6, 7, 14, 15, 30, 31, 62, 63, 126, 127, 254, 255, 510, 511, 1022, 1023, 2046, 2047, 4094, 4095, 8190, 8191, 16382, 16383, 32766, 32767, 65534 };
        const int nue = (int)(sizeof(uev)/sizeof(uev[0]));
        for (off = 0; off < 32; off++)
            for (s = 0; s < 6; s++)
            {
                int ops[16][3], n = 0;
                uint8_t buf[256];
                bs_t bs;
                unsigned nbits;
                if (off) { ops[n][0] = 0; ops[n][1] = (int)((1u << off) - 1u); ops[n++][2] = off; }
                if (s < 3 && s != off % 3) continue;
                if (s < 3)
                {
                    /* golomb codes of 0, 1, 2^k - 1, 2^k - 2 ... up to the 31-bit code, signed ones of either sign */
                    for (c = 0; c < 5; c++)
                    {
                        const int u = uev[(off*5 + s*11 + c*7) % nue];
                        if (c & 1) { ops[n][0] = 2; ops[n][1] = ((c & 2) ? -1 : 1)*((u + 1)/2 > 16383 ? 16383 : (u + 1)/2); ops[n++][2] = 0; }
                        else { ops[n][0] = 1; ops[n][1] = u; ops[n++][2] = 0; }
                    }
                } else
                {
                    /* a put that ends one before, exactly on and one after the word boundary, then one more to show the state behind it */
                    const int len = 32 - off + (s - 4);
                    if (len < 1 || len > 32) continue;
                    /* (the reference's writer takes at most 31 bits of a non-zero value: its own `val >> n` check shifts by the type's width at 32) */
                    if (len == 32) { ops[n][0] = 0; ops[n][1] = 0xa5a5; ops[n++][2] = 16; ops[n][0] = 0; ops[n][1] = 0x5a5b; ops[n++][2] = 16; }
                    else { ops[n][0] = 0; ops[n][1] = (int)(0xa5a5a5a5u >> (32 - len)); ops[n++][2] = len; }
                    ops[n][0] = 0; ops[n][1] = 0x15; ops[n++][2] = 5;
                    ops[n][0] = 0; ops[n][1] = 0x7fffffff; ops[n++][2] = 31;
                }
                memset(buf, 0, sizeof(buf));
                h264e_bs_init_bits(&bs, buf);
                for (c = 0; c < n; c++)
                {
                    if (ops[c][0] == 0) h264e_bs_put_bits(&bs, (unsigned)ops[c][2], (unsigned)ops[c][1]);
                    else if (ops[c][0] == 1) h264e_bs_put_golomb(&bs, (unsigned)ops[c][1]);
                    else h264e_bs_put_sgolomb(&bs, ops[c][1]);
                }
                nbits = h264e_bs_get_pos_bits(&bs);
                h264e_bs_flush(&bs);
                sep(&first);
                printf("  {\"ops\": [");
                for (c = 0; c < n; c++) printf("%s[%d,%d,%d]", c ? "," : "", ops[c][0], ops[c][1], ops[c][2]);
                printf("], \"nbits\": %u, ", nbits);
                hexwh("bits", buf, 0, (int)((nbits + 7)/8), 1, "}");
            }
    }
    {
        static const int offs[6] = { 0, 7, 15, 16, 24, 31 };
        int j, c;
        for (j = 0; j < 6; j++)
        {
            /* se(0) is the mb_qp_delta of every coded macroblock */
            const int ops[6][3] = { {0, (int)((1u << offs[j]) - 1u), offs[j]}, {2, 0, 0}, {2, 1, 0}, {2, -1, 0}, {1, 0, 0}, {2, 0, 0} };
            uint8_t buf[64];
            bs_t bs;
            unsigned nbits;
            memset(buf, 0, sizeof(buf));
            h264e_bs_init_bits(&bs, buf);
            for (c = offs[j] ? 0 : 1; c < 6; c++)
            {
                if (ops[c][0] == 0) h264e_bs_put_bits(&bs, (unsigned)ops[c][2], (unsigned)ops[c][1]);
                else if (ops[c][0] == 1) h264e_bs_put_golomb(&bs, (unsigned)ops[c][1]);
                else h264e_bs_put_sgolomb(&bs, ops[c][1]);
            }
            nbits = h264e_bs_get_pos_bits(&bs);
            h264e_bs_flush(&bs);
            sep(&first);
            printf("  {\"ops\": [");
            for (c = offs[j] ? 0 : 1; c < 6; c++) printf("%s[%d,%d,%d]", c > (offs[j] ? 0 : 1) ? "," : "", ops[c][0], ops[c][1], ops[c][2]);
            printf("], \"nbits\": %u, ", nbits);
            hexwh("bits", buf, 0, (int)((nbits + 7)/8), 1, "}");
        }
    }
    printf("\n ]\n}\n");
    return 0;
}

/* ================================================================== `stage_harness finalizer` -> tests/golden/finalizer.json
 * The two functions the finalizer's mv_clusters walk restates (oracle, host and device each have their own copy): inputs and the
 * reference's outputs, vectors as [x, y] in quarter samples. */
static int finalizer(h264e_enc_t *enc)
{
    /* states (short | long): zero; ordinary; all negative (the >> 6 acts on a negative sum); long shorter than short (a vector can move
     * neither); mixed signs; +-2048; the int16 extremes (never both components -32768: the squared norm would leave int) */
    static const int st[][4] = {
        { 0, 0, 0, 0 }, { 3, 4, 30, 40 }, { -3, -4, -30, -40 }, { 40, 30, 3, 4 }, { -7, 9, 64, -64 }, { 2048, -2048, -2048, 2048 },
        { 32767, -32768, -32768, 32767 }, { -32768, 0, 0, 32767 }, { 1, -1, -1, 1 }, { 0, 0, -2048, 2048 }, { -129, 63, -1, -63 } };
    /* vectors: norms equal to, just under and over those of the states above (25, 2500), every sign, the same extremes */
    static const int vs[][2] = {
        { 0, 0 }, { 5, 0 }, { -4, 3 }, { 0, -5 }, { 4, -2 }, { 50, 0 }, { -30, -40 }, { 10, 0 }, { -1, -1 }, { 1, 1 }, { -33, 31 }, { 31, -33 },
        { 2048, 2048 }, { -2048, -2048 }, { 2048, -2048 }, { 32767, 32767 }, { -32768, 32767 }, { 32767, -32768 }, { -32768, 0 }, { 0, -32768 },
        { -64, 64 }, { 63, -63 }, { 49, 9 }, { 51, 0 } };
    int i, j, k, first = 1;
    g_seed = 24680;
    printf("{\n \"generator\": \"oracle/stage_harness.c finalizer against the reference header (h264-lab.h), make -C oracle finalizer\",\n");
    printf(" \"round\": [");                                     /* [v, x of mv_round_qpel(v, -v), y of it] */
    for (i = -8; i <= 8; i++)
    {
        const point_t r = mv_round_qpel(point(i, -i));
        printf("%s[%d,%d,%d]", i > -8 ? "," : "", i, r.s.x, r.s.y);
    }
    printf("],\n \"steps\": [\n");                              /* [short, long, vector, short', long'] */
    for (i = 0; i < (int)(sizeof(st)/sizeof(st[0])); i++)
        for (j = 0; j < (int)(sizeof(vs)/sizeof(vs[0])); j++)
        {
            enc->mv_clusters[0] = point(st[i][0], st[i][1]); enc->mv_clusters[1] = point(st[i][2], st[i][3]);
            mv_clusters_update(enc, point(vs[j][0], vs[j][1]));
            printf("%s  [%d,%d,%d,%d,%d,%d,%d,%d,%d,%d]", first ? "" : ",\n", st[i][0], st[i][1], st[i][2], st[i][3], vs[j][0], vs[j][1],
                   enc->mv_clusters[0].s.x, enc->mv_clusters[0].s.y, enc->mv_clusters[1].s.x, enc->mv_clusters[1].s.y);
            first = 0;
        }
    printf("\n ],\n \"sequences\": [\n");
    for (k = 0; k < 3; k++)
    {
        /* 0: small vectors around zero with a rare long one; 1: two populations, a short and a long one; 2: the whole +-2048 range */
        static const int start[3][4] = { { 0, 0, 0, 0 }, { 2, 1, -100, 36 }, { -600, 200, 900, -1500 } };
        enc->mv_clusters[0] = point(start[k][0], start[k][1]); enc->mv_clusters[1] = point(start[k][2], start[k][3]);
        printf("  {\"steps\": [\n");                            /* [short, long in front of the vector, vector] */
        for (i = 0; i < 300; i++)
        {
            int x, y;
            if (k == 0) { const int big = rnd() % 16 == 0; x = (int)(rnd() % (big ? 257u : 33u)) - (big ? 128 : 16); y = (int)(rnd() % (big ? 257u : 33u)) - (big ? 128 : 16); }
            else if (k == 1) { const int lg = rnd() % 3 == 0; x = (lg ? -120 : 2) + (int)(rnd() % 9u) - 4; y = (lg ? 40 : 1) + (int)(rnd() % 9u) - 4; }
            else { x = (int)(rnd() % 4097u) - 2048; y = (int)(rnd() % 4097u) - 2048; }
            printf("%s   [%d,%d,%d,%d,%d,%d]", i ? ",\n" : "", enc->mv_clusters[0].s.x, enc->mv_clusters[0].s.y, enc->mv_clusters[1].s.x, enc->mv_clusters[1].s.y, x, y);
            mv_clusters_update(enc, point(x, y));
        }
        printf("\n  ], \"end\": [%d,%d,%d,%d]}%s\n", enc->mv_clusters[0].s.x, enc->mv_clusters[0].s.y, enc->mv_clusters[1].s.x, enc->mv_clusters[1].s.y, k < 2 ? "," : "");
    }
    printf(" ]\n}\n");
    return 0;
}
