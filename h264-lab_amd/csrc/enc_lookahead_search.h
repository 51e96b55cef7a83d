/*
 * enc_lookahead_search.h -- the cost pass of the lookahead rate control with a motion search (H264E_clip_set_lookahead_search): the three
 * sums of enc_lookahead.h from a searched inter cost, and a motion field, one cell per block.
 *
 * L_f, the blocks b = (bx, by) of nbx x nby, m(b) and intra(b) are enc_lookahead.h's.  With A = [0, 8*nbx) x [0, 8*nby) -- the part of
 * L_{f-1} that the ring keeps -- and a range R in 1..8 (tests/lookahead_motion_model.py restates this):
 *     candidates d = (dx, dy), |dx|, |dy| <= R, whose 8x8 block at (8bx + dx, 8by + dy) lies wholly inside A (left out, not clamped,
 *                otherwise; (0, 0) always counts)
 *     sad(b, d)  = sum over the block of |L_f(x, y) - L_{f-1}(x + dx, y + dy)|
 *     inter(b)   = the smallest sad; mv(b) = the candidate that reaches it and comes first by (|dx| + |dy|, dy, dx): no vector
 *                penalty in the cost, a flat area gives (0, 0) through the order
 *     frame 0 of the clip: inter(b) = intra(b), mv(b) = (0, 0)
 *     I(f), P(f) = sum min(intra, inter), N(f) = #{intra < inter} as before; field cell of b: int8 dx, int8 dy, uint16 inter(b) (<= 16320)
 * Smallest sad and order are ONE minimum, over the key (sad << 15) | ((|dx| + |dy|) << 10) | ((dy + 8) << 5) | (dx + 8): the vector is read
 * back from the winning key, and a candidate that does not count holds LOOKAHEAD_SEARCH_NO_KEY.
 *
 * A workgroup is ONE wave and takes a strip of LOOKAHEAD_SEARCH_STRIP = 8 blocks of one block row.
 *   1. lane = (block of the strip, row of the block): lookahead_row as in the pass without search -- the input slot is read once, the
 *      frame's entry is written in the same layout, so frames analysed with and without the search may follow each other in the ring --
 *      then m and intra through the butterflies inside 8 lanes; the row goes into LDS (cur), intra(b) too.
 *   2. the previous frame's entry for the strip and one block of halo around it (R <= 8) goes from its block order into LDS as a linear
 *      picture, 10 blocks x 3 block rows = 80 x 24 samples, 8-byte cells (lookahead_search_stage); halo blocks outside A are not loaded
 *      (zeros stand there) and the candidates that would read them do not count.
 *   3. block after block: lanes are candidates, (2R + 1)^2 <= 289 of them in rounds of 64.  A candidate's row is the 8 bytes at any
 *      alignment of a row of the LDS picture: the three aligned dwords around them shifted into place (v_alignbyte), then two v_sad_u8
 *      against the block's row, which every lane reads from the same LDS address -- 16 v_sad_u8 per candidate.  The minimum over the
 *      wave is DPP inside rows of 16 and four v_readlane; lane i keeps the key of block i.
 *   4. lanes 0..7 write their block's field cell (a vector store of one dword each, 32 contiguous bytes), I / P / N go through a wave
 *      reduction and three 64-bit vector atomics into the frame's record.  Nothing scalar writes memory.
 * h264e_kernels.hip runs it as h264e_lookahead_search_kernel, h264e_pool.h's emulation launch (H264E_EMU) as lane loops over the strips.
 */
#ifndef H264E_ENC_LOOKAHEAD_SEARCH_H
#define H264E_ENC_LOOKAHEAD_SEARCH_H
#include "enc_lookahead.h"

#define LOOKAHEAD_SEARCH_MAX_RANGE 8
#define LOOKAHEAD_SEARCH_STRIP 8
#define LOOKAHEAD_SEARCH_PITCH ((LOOKAHEAD_SEARCH_STRIP + 2)*8)                     /* bytes per row of the LDS picture */
#define LOOKAHEAD_SEARCH_CELLS ((LOOKAHEAD_SEARCH_STRIP + 2)*3*8)                   /* its 8-byte cells */
#define LOOKAHEAD_SEARCH_PREV_DWORDS (LOOKAHEAD_SEARCH_PITCH*24/4 + 1)              /* + the dword behind an aligned last row, read and shifted out */
#define LOOKAHEAD_SEARCH_ROUNDS 5                                                   /* 289 candidates, 64 at a time */
#define LOOKAHEAD_SEARCH_NO_KEY 0x7fffffff
#define LOOKAHEAD_FIELD_CELL_BYTES 4

typedef struct
{
    lookahead_args_t a;                 /* as for the pass without search */
    uint32_t *field;                    /* this frame's field, [nblk] cells */
    int range, nby;
} lookahead_search_args_t;

typedef struct
{
    uint32_t prev[LOOKAHEAD_SEARCH_PREV_DWORDS];        /* L_{f-1}: strip + halo, rows of LOOKAHEAD_SEARCH_PITCH bytes */
    uint32_t cur[LOOKAHEAD_SEARCH_STRIP*16];            /* L_f: row r of strip block i at dwords 16i + 2r */
    int intra[LOOKAHEAD_SEARCH_STRIP];
} lookahead_search_lds_t;

/* cell c (< LOOKAHEAD_SEARCH_CELLS) of the LDS picture for the strip that starts at block (bx0, by): row c & 7 of halo block c >> 3 */
DEV void lookahead_search_stage(const lookahead_search_args_t &S, int bx0, int by, int c, LDS_AS uint32_t *prev)
{
    const int hb = c >> 3, r = c & 7, hy = hb/(LOOKAHEAD_SEARCH_STRIP + 2), hx = hb - hy*(LOOKAHEAD_SEARCH_STRIP + 2);
    const int bx = bx0 - 1 + hx, byy = by - 1 + hy;
    uint32_t v0 = 0, v1 = 0;
    if (bx >= 0 && bx < S.a.nbx && byy >= 0 && byy < S.nby)
    {
        const GLOBAL_AS uint32_t *q = (const GLOBAL_AS uint32_t *)((const gu8 *)S.a.prev + (size_t)(byy*S.a.nbx + bx)*LOOKAHEAD_BLOCK_BYTES + 8*(size_t)r);
        EMU_GLOBAL(q, 8);
        v0 = q[0]; v1 = q[1];
    }
    LDS_AS uint32_t *d = prev + ((hy*8 + r)*LOOKAHEAD_SEARCH_PITCH + hx*8)/4;
    d[0] = v0; d[1] = v1;
}

/* candidate i of the range's (2R + 1)^2, row by row: (dx + 8) | (dy + 8) << 5, or -1 behind the last */
DEV int lookahead_search_candidate(int range, int i)
{
    const int side = 2*range + 1, row = i/side;
    return i < side*side ? (i - row*side - range + 8) | ((row - range + 8) << 5) : -1;
}

/* the candidate's block lies wholly inside A */
DEV int lookahead_search_inside(const lookahead_search_args_t &S, int bx, int by, int dx, int dy)
{
    return 8*bx + dx >= 0 && 8*bx + dx + 8 <= 8*S.a.nbx && 8*by + dy >= 0 && 8*by + dy + 8 <= 8*S.nby;
}

/* sad of strip block i against the LDS picture displaced by (dx, dy), both inside -8..8 */
DEV int lookahead_search_sad(const LDS_AS uint32_t *prev, const LDS_AS uint32_t *cur, int i, int dx, int dy)
{
    const int off = (8 + dy)*LOOKAHEAD_SEARCH_PITCH + 8*(i + 1) + dx;
    const unsigned mis = (unsigned)off & 3u;
    const LDS_AS uint32_t *p = prev + (off >> 2), *c = cur + 16*i;
    uint32_t sad = 0;
#pragma unroll
    for (int r = 0; r < 8; r++, p += LOOKAHEAD_SEARCH_PITCH/4)
    {
        const uint32_t a0 = p[0], a1 = p[1], a2 = p[2];
        sad = sad4_u8(c[2*r], alignbyte32(a1, a0, mis), sad);
        sad = sad4_u8(c[2*r + 1], alignbyte32(a2, a1, mis), sad);
    }
    return (int)sad;
}

DEV int lookahead_search_key(int sad, int dx, int dy) { return (sad << 15) | ((iabs(dx) + iabs(dy)) << 10) | ((dy + 8) << 5) | (dx + 8); }

/* the field cell of a winning key: int8 dx, int8 dy, uint16 cost */
DEV uint32_t lookahead_search_cell(int key)
{
    return (uint32_t)(((key & 31) - 8) & 0xff) | ((uint32_t)((((key >> 5) & 31) - 8) & 0xff) << 8) | ((uint32_t)(key >> 15) << 16);
}

/* the key of block (bx, by) = strip block i for the candidates of one lane slot, cand[k] as lookahead_search_candidate gives them */
DEV int lookahead_search_lane(const lookahead_search_args_t &S, const LDS_AS uint32_t *prev, const LDS_AS uint32_t *cur, int bx, int by, int i, const int cand[LOOKAHEAD_SEARCH_ROUNDS], int rounds)
{
    int best = LOOKAHEAD_SEARCH_NO_KEY;
#pragma unroll
    for (int k = 0; k < LOOKAHEAD_SEARCH_ROUNDS; k++)
    {
        if (k >= rounds) break;
        const int dx = (cand[k] & 31) - 8, dy = ((cand[k] >> 5) & 31) - 8;
        const int on = cand[k] >= 0 && lookahead_search_inside(S, bx, by, dx, dy);
        /* a lane without a candidate reads where (0, 0) reads: inside the LDS picture */
        const int sad = lookahead_search_sad(prev, cur, i, on ? dx : 0, on ? dy : 0);
        const int key = on ? lookahead_search_key(sad, dx, dy) : LOOKAHEAD_SEARCH_NO_KEY;
        best = imin(best, key);
    }
    return best;
}

DEV void lookahead_search_field_store(const lookahead_search_args_t &S, int b, uint32_t cell)
{
    GLOBAL_AS uint32_t *q = (GLOBAL_AS uint32_t *)S.field + b;
    EMU_GLOBAL(q, 4);
    *q = cell;
}

#endif
