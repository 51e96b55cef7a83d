/*
 * enc_lookahead_tree.h -- the cost tree of the lookahead rate control (H264E_clip_set_lookahead_tree): cost propagated backwards through
 * the motion field of the searched cost pass (enc_lookahead_search.h), summed to one number per frame.  The reference has no such pass;
 * this integer definition IS the definition (tests/lookahead_tree_model.py restates it, include/h264e_mi355x.h gives the controller's
 * use of it).
 *
 * L_f, the blocks b of nbx x nby, intra(b), inter(b), mv(b) = (dx, dy) and A are enc_lookahead_search.h's.  For a run over frames
 * [a, e) with key(f) the key-frame schedule: in_f(t) = 0 for every block t of every frame; then for f = e - 1 down to a + 1, unless
 * key(f), every block s = (sx, sy) of frame f passes on
 *     i = intra_f(s), c = min(i, inter_f(s)), g = min(in_f(s), 2^40)
 *     amt = g when i == 0, else ((i + g)*(i - c))/i, floored                                   (i + g)*(i - c) < 2^55
 *     x = 8sx + dx, y = 8sy + dy (inside A by the search's rule), tx = x >> 3, ox = x & 7, ty = y >> 3, oy = y & 7
 *     in_{f-1}(tx + u, ty + v) += (amt*wx*wy) >> 6 for u, v in {0, 1}, wx = u ? ox : 8 - ox, wy = v ? oy : 8 - oy, weight 0 left out
 * and S(f) = min(sum_t min(in_f(t), 2^40), 2^48).  Up to nine source blocks reach one target, each with at most 2^40 + 2^14: every cell
 * and every sum stays far below 2^64, and the additions are order independent.
 *
 * One launch per frame, in REVERSE frame order on the pool's stream: the launch of frame f reads in_f, complete since the launch of
 * frame f + 1 has ended, adds min(in_f, 2^40) into the frame's sum and scatters into in_{f-1}; for a key frame and for frame a the
 * scatter is switched off (out == NULL) and the launch only sums.  A workgroup is ONE wave and takes 8 consecutive blocks:
 *   1. lane = (block, row): the row's 8 samples of L_f from the frame's entry of the half-resolution ring (64 contiguous bytes per block,
 *      512 per wave), m(b) and intra(b) through the cost pass' butterflies inside 8 lanes (lookahead_oct_sum) -- the cost pass keeps
 *      inter(b) and mv(b) in the field cell but not intra(b), and recomputing it costs two v_sad_u8 and six DPP steps.
 *   2. the lane with row 0 reads in_f(b) and the field cell, forms amt in 64-bit integers (one 64-by-32-bit division per block) and adds
 *      its up to four contributions to in_{f-1} with 64-bit vector atomics (lookahead_record_add): a target outside the grid -- which
 *      the search's rule excludes -- would be dropped, never written.
 *   3. the frame's sum: g in three fields of 21 bits through the wave reduction, one 64-bit vector atomic per workgroup.
 * No floats, no LDS, nothing scalar writes memory.  h264e_kernels.hip runs it as h264e_lookahead_tree_kernel, h264e_pool.h's emulation
 * launch (H264E_EMU) as lane loops over the waves.
 */
#ifndef H264E_ENC_LOOKAHEAD_TREE_H
#define H264E_ENC_LOOKAHEAD_TREE_H
#include "enc_lookahead_search.h"

#define LOOKAHEAD_TREE_WAVE_BLOCKS 8
#define LOOKAHEAD_TREE_CELL_BYTES 8
#define LOOKAHEAD_TREE_IN_MAX (1ull << 40)              /* what a block passes on of what it received, at most */
#define LOOKAHEAD_TREE_SUM_MAX (1ull << 48)             /* S(f), at most */

typedef struct
{
    const uint8_t *lo;                  /* frame f's half-resolution entry */
    const uint32_t *field;              /* ... its field, [nblk] cells */
    const unsigned long long *in;       /* in_f [nblk] */
    unsigned long long *out;            /* in_{f-1} [nblk]; NULL = no scatter (a key frame, the run's first frame) */
    unsigned long long *sum;            /* sum of min(in_f, 2^40): zeroed by the host in front of the launches */
    int nbx, nby, nblk;
} lookahead_tree_args_t;

/* row r (0..7) of block b (< nblk) from the frame's entry */
DEV lookahead_row_t lookahead_tree_row(const lookahead_tree_args_t &T, int b, int r)
{
    lookahead_row_t R;
    const GLOBAL_AS uint32_t *q = (const GLOBAL_AS uint32_t *)((const gu8 *)T.lo + (size_t)b*LOOKAHEAD_BLOCK_BYTES + 8*(size_t)r);
    EMU_GLOBAL(q, 8);
    R.lo[0] = q[0]; R.lo[1] = q[1]; R.pv[0] = R.pv[1] = 0;
    return R;
}

/* what a block of intra cost i and coded cost c = min(intra, inter) passes on of its own cost and of the g it received */
DEV unsigned long long lookahead_tree_amount(int i, int c, unsigned long long g)
{
    return i ? ((unsigned long long)i + g)*(unsigned long long)(i - c)/(unsigned)i : g;
}

/* block b, whose intra cost is `intra`: min(in_f(b), 2^40), and its contributions into in_{f-1} when the scatter is on */
DEV unsigned long long lookahead_tree_block(const lookahead_tree_args_t &T, int b, int intra)
{
    const GLOBAL_AS unsigned long long *pin = (const GLOBAL_AS unsigned long long *)T.in + b;
    EMU_GLOBAL(pin, 8);
    unsigned long long g = *pin;
    if (g > LOOKAHEAD_TREE_IN_MAX) g = LOOKAHEAD_TREE_IN_MAX;
    if (!T.out) return g;
    const GLOBAL_AS uint32_t *pc = (const GLOBAL_AS uint32_t *)T.field + b;
    EMU_GLOBAL(pc, 4);
    const uint32_t cell = *pc;
    const int inter = (int)(cell >> 16), dx = (int)(int8_t)(cell & 0xffu), dy = (int)(int8_t)((cell >> 8) & 0xffu);
    const unsigned long long amt = lookahead_tree_amount(intra, intra < inter ? intra : inter, g);
    const int sy = b/T.nbx, sx = b - sy*T.nbx, x = 8*sx + dx, y = 8*sy + dy;
    const int tx = x >> 3, ox = x & 7, ty = y >> 3, oy = y & 7;
    if (!amt) return g;
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        const int u = k & 1, v = k >> 1, wx = u ? ox : 8 - ox, wy = v ? oy : 8 - oy, px = tx + u, py = ty + v;
        if (wx && wy && px >= 0 && px < T.nbx && py >= 0 && py < T.nby)
            lookahead_record_add(T.out + (size_t)py*(size_t)T.nbx + (size_t)px, (amt*(unsigned)(wx*wy)) >> 6);
    }
    return g;
}

#endif
