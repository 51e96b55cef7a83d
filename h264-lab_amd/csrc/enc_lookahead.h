/*
 * enc_lookahead.h -- the cost pass of the lookahead rate control (H264E_clip_set_lookahead): three integer sums per input frame.
 *
 * The reference has no such pass; like enc_scenecut.h, this integer definition IS the definition (tests/lookahead_model.py restates it).
 * With Y the luma of the RAW input frame f (width x height, before the denoiser), w2 = width/2, h2 = height/2:
 *     L_f(x,y) = (Y(2x,2y) + Y(2x+1,2y) + Y(2x,2y+1) + Y(2x+1,2y+1) + 2) >> 2           x < w2, y < h2
 *     blocks b = (bx, by), 8x8 samples of L_f, wholly inside it: bx < w2 >> 3, by < h2 >> 3
 *     m(b)     = (sum of L_f over b + 32) >> 6
 *     intra(b) = sum over b of |L_f - m(b)|
 *     inter(b) = sum over b of |L_f - L_{f-1}|, co-located, no search; for the clip's frame 0 inter(b) = intra(b)
 *     I(f) = sum_b intra(b)      P(f) = sum_b min(intra(b), inter(b))      N(f) = #{b : intra(b) < inter(b)}
 * The sums are 64-bit (I passes 2^32 at 8K) and order independent.  Zero-motion inter cost overestimates pans; the controller's
 * per-window calibration absorbs a steady bias.  The controller itself -- budgets, predicted bits, one QP per window within 6 of the
 * window before it, calibration -- is host code (h264e_host.c clip_la_plan_window / clip_la_close_window) and is defined in
 * include/h264e_mi355x.h at H264E_clip_set_lookahead.
 *
 * The input slot of frame f is read ONCE.  What later frames need of it is the part of L_f that the blocks cover, and the pass writes
 * that into a ring of half-resolution pictures owned by the pool, one entry per resident input slot (two for a single-slot pool), frame f
 * in entry f % entries -- block by block, 64 bytes per block, row r of block b at 64*b + 8*r: every lane then writes and reads whole
 * aligned 8-byte cells.  Frame f-1's entry is overwritten when frame f-1+entries is analysed, after f (frames are analysed in order),
 * so the pass never reads another frame's input slot and a bounded input ring needs no second picture.
 *
 * A lane owns one row of one block: 8 samples of L_f = 2 x 16 luma samples.  The 16 bytes start at an even address that is not always a
 * dword (a slot starts at frame_bytes = width*height*3/2 times its index, a row at a multiple of the even width): as in
 * enc_scenecut.h they are read as the aligned dwords that enclose them -- five when misaligned, else four, both rows' loads issued
 * before the first is used -- and shifted into place (v_alignbyte); the up to three bytes in front and behind belong to the
 * neighbouring rows, the frame before it in the ring or this frame's chroma, all inside the pool's allocation, and are dropped.
 *   lookahead_row     : lane level.  Loads, the 2x2 means as two packed dwords, the store into this frame's entry, the previous
 *                       frame's cell.
 *   lookahead_row_sum / _intra / _inter : lane level.  v_sad_u8 (wave.h sad4_u8) over the two dwords.
 * Eight consecutive lanes make a block, so the block sums are three xor-butterfly steps inside a row of 8 lanes (DPP / swizzle, no LDS);
 * the lane with r = 0 keeps I, P, N of its blocks, a wave reduction and one LDS cell per wave make the workgroup's sums, and thread 0 adds
 * them to the frame's record with three 64-bit vector global atomics.  Nothing scalar writes memory.
 * h264e_kernels.hip runs it as h264e_lookahead_kernel, h264e_pool.h's emulation launch (H264E_EMU) as a lane loop over the blocks.
 * enc_lookahead_search.h is the same pass with a motion search in inter(b) (H264E_clip_set_lookahead_search); it uses lookahead_row, the
 * row sums and the record as they stand here and writes the same entries.
 */
#ifndef H264E_ENC_LOOKAHEAD_H
#define H264E_ENC_LOOKAHEAD_H
#include "wave.h"

#define LOOKAHEAD_BLOCK_BYTES 64
#define LOOKAHEAD_MIN_SIDE 16           /* pictures below 16x16 have no block (the rule SSIM has) */

typedef struct
{
    const uint8_t *luma;                /* the frame's input slot: width x height luma samples, rows packed */
    const uint8_t *prev;                /* the previous frame's half-resolution entry, or NULL for the clip's frame 0 */
    uint8_t *cur;                       /* this frame's entry */
    unsigned long long *record;         /* [3] I, P, N: zeroed by the host in front of the launch */
    int width, nbx, nblk;               /* luma row length; blocks per row, blocks */
} lookahead_args_t;

typedef struct { uint32_t lo[2], pv[2]; } lookahead_row_t;     /* 8 samples of L_f and of L_{f-1}, packed */

/* the 16 bytes at p (any alignment) from the aligned dwords around them */
DEV void lookahead_load16(const gu8 *p, uint32_t out[4])
{
    const unsigned mis = (unsigned)((uintptr_t)p & 3);
    const gu8 *q = p - mis;
    EMU_GLOBAL(q, mis ? 20 : 16);
    const GLOBAL_AS uint32_t *d = (const GLOBAL_AS uint32_t *)q;
    const uint32_t a0 = d[0], a1 = d[1], a2 = d[2], a3 = d[3], a4 = mis ? d[4] : 0u;
    out[0] = alignbyte32(a1, a0, mis); out[1] = alignbyte32(a2, a1, mis); out[2] = alignbyte32(a3, a2, mis); out[3] = alignbyte32(a4, a3, mis);
}

/* the sums of horizontal pairs of two rows' dwords (4 + 4 samples): two 2x2 sums in 16-bit fields */
DEV uint32_t lookahead_quad(uint32_t a, uint32_t b)
{
    return (a & 0x00ff00ffu) + ((a >> 8) & 0x00ff00ffu) + (b & 0x00ff00ffu) + ((b >> 8) & 0x00ff00ffu);
}

/* ... of 8 + 8 samples rounded into four samples of L_f, packed */
DEV uint32_t lookahead_mean4(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1)
{
    const uint32_t r0 = ((lookahead_quad(a0, b0) + 0x00020002u) >> 2) & 0x00ff00ffu, r1 = ((lookahead_quad(a1, b1) + 0x00020002u) >> 2) & 0x00ff00ffu;
    return (r0 & 0xffu) | ((r0 >> 8) & 0xff00u) | ((r1 & 0xffu) << 16) | ((r1 << 8) & 0xff000000u);
}

/* row r (0..7) of block b (< nblk): its 8 samples of L_f into the frame's entry, and the previous frame's */
DEV lookahead_row_t lookahead_row(const lookahead_args_t &A, int b, int r)
{
    lookahead_row_t R;
    const int by = b/A.nbx, bx = b - by*A.nbx;
    const gu8 *p = (const gu8 *)A.luma + (size_t)(2*(8*by + r))*(size_t)A.width + 16*(size_t)bx;
    const size_t cell = (size_t)b*LOOKAHEAD_BLOCK_BYTES + 8*(size_t)r;
    uint32_t t[4], u[4];
    lookahead_load16(p, t);
    lookahead_load16(p + A.width, u);
    R.pv[0] = R.pv[1] = 0;
    if (A.prev)
    {
        const GLOBAL_AS uint32_t *q = (const GLOBAL_AS uint32_t *)((const gu8 *)A.prev + cell);
        EMU_GLOBAL(q, 8);
        R.pv[0] = q[0]; R.pv[1] = q[1];
    }
    R.lo[0] = lookahead_mean4(t[0], t[1], u[0], u[1]);
    R.lo[1] = lookahead_mean4(t[2], t[3], u[2], u[3]);
    {
        GLOBAL_AS uint32_t *q = (GLOBAL_AS uint32_t *)((gu8 *)A.cur + cell);
        EMU_GLOBAL(q, 8);
        q[0] = R.lo[0]; q[1] = R.lo[1];
    }
    return R;
}

DEV int lookahead_row_sum(const lookahead_row_t &R) { return (int)sad4_u8(R.lo[1], 0u, sad4_u8(R.lo[0], 0u, 0u)); }
/* m: the block's mean, 0..255 */
DEV int lookahead_row_intra(const lookahead_row_t &R, int m) { const uint32_t m4 = (uint32_t)m*0x01010101u; return (int)sad4_u8(R.lo[1], m4, sad4_u8(R.lo[0], m4, 0u)); }
DEV int lookahead_row_inter(const lookahead_row_t &R) { return (int)sad4_u8(R.lo[1], R.pv[1], sad4_u8(R.lo[0], R.pv[0], 0u)); }

/* a sum into the frame's record, which other workgroups add to at the same time */
#ifdef H264E_EMU
DEV void lookahead_record_add(unsigned long long *p, unsigned long long v) { EMU_GLOBAL(p, 8); *p += v; }
#else
DEV void lookahead_record_add(unsigned long long *p, unsigned long long v) { if (v) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif

#endif
