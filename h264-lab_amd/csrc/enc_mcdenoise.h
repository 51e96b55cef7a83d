/*
 * enc_mcdenoise.h -- the motion-compensated temporal denoiser (H264E_clip_set_denoise_motion): enc_denoise.h's filter with the previous
 * denoised picture displaced, block by block, by the motion field of the lookahead's searched cost pass (enc_lookahead_search.h).
 *
 * The reference has no such filter; this integer definition IS the definition (tests/mcdenoise_model.py restates it).  Per frame f:
 * cur = the RAW input (Y w x h, U and V w/2 x h/2), D_{f-1} = the previous OUTPUT of this filter (zeros in front of frame 0),
 * mv(b) = (dx, dy) the field cell of block b = (bx, by), nbx = (w/2) >> 3, nby = (h/2) >> 3 (frame 0 of a clip has a zero field).
 *   luma vector of the 16x16 block at (16bx, 16by):
 *     mode 1: v = (2dx, 2dy);
 *     mode 2: candidates (0, 0), then (2dx + rx, 2dy + ry), (rx, ry) in {-1, 0, 1}^2 in the order (|rx| + |ry|, ry, rx): ten of them.  A
 *             candidate counts when its displaced block lies wholly inside the plane (left out, not clamped, otherwise; (0, 0) and
 *             (2dx, 2dy) always count); sad(b, v) = sum over the block of |Y_f(x, y) - D_{f-1}(x + vx, y + vy)| <= 65280; v = the first
 *             candidate with the smallest sad -- ONE minimum over the key (sad << 4) | candidate index;
 *   chroma vector of the 8x8 block (bx, by): (dx, dy) as it stands, in both modes;
 *   samples that no block covers (luma outside [0, 16nbx) x [0, 16nby), chroma outside [0, 8nbx) x [0, 8nby)): the vector (0, 0);
 *   filter, per plane, sample s with the vector v of ITS OWN block: first / last row and column out = cur; otherwise
 *     out = denoise_px(T, cur(s), D_{f-1}(clamp(s + v)), sum over the four neighbours n of cur(n) - D_{f-1}(clamp(n + v)))
 *     with both coordinates clamped to the plane: the centre's vector applies to its neighbours, so a block reads ONE displaced window.
 *   cell of block b: int8 vx, int8 vy, uint16 sad of the luma vector (mode 1: of (2dx, 2dy)).
 * With an all-zero field this is enc_denoise.h's filter sample for sample.
 *
 * A workgroup is ONE wave and takes the tile (bx, by) of a grid of ceil(w/16) x ceil(h/16): 16x16 luma samples and 8x8 of each chroma
 * plane, cut at the plane's right and bottom edge; tiles outside the blocks take the zero vector and write no cell.  Plane after plane:
 *   1. the windows go into LDS as rows of MCD_PITCH dwords, the tile's column 0 at byte 4 of a row, so the tile's own groups of four are
 *      aligned dwords: cur with a ring of one row and four columns around the tile, D_{f-1} around the displaced tile with a ring of two
 *      rows (every refinement plus the neighbour ring), in mode 2 a second D_{f-1} window at displacement zero for the (0, 0) candidate.
 *      A window dword is the two aligned dwords around its four bytes shifted into place (v_alignbyte; a slot starts on an even address,
 *      not always a dword); a window that comes within four bytes of the plane's edge is loaded byte by byte with clamped coordinates
 *      instead -- which is exactly the clamp of the definition, so the filter never clamps.
 *   2. luma refinement: lane = (row, group of four columns), one v_sad_u8 per candidate against the window dword at the candidate's
 *      byte offset (two LDS dwords + v_alignbyte); per-lane sums <= 1020, the ten block sums come out of wave_sum8 / wave_sum4 (two sums
 *      per register through the DPP / v_readlane reduction), every lane then holds all ten and takes the minimum key itself.
 *   3. filter: lane = (row, group of four columns), enc_denoise.h's denoise_quad on dwords, one dword store per lane (bytes where the
 *      address is not a dword or the row ends).  Lane 0 stores the cell with one vector dword store.  Nothing scalar writes memory.
 * cur, D_{f-1} and D_f are three different frames and every tile writes only its own samples: no traffic between workgroups.
 * mcdenoise_block is the whole workgroup in wave.h's model (WAVE_FOR sections, wave_sync between LDS writes and reads):
 * h264e_kernels.hip runs it as h264e_mcdenoise_kernel<MODE>, h264e_pool.h's emulation launch (H264E_EMU) as a loop over the tiles.  The
 * mode is a template parameter: mode 1's code has no second window and no candidate loop -- and, as templates, the two kernels are
 * emitted behind every kernel the library had, which keep their places in the code object.
 */
#ifndef H264E_ENC_MCDENOISE_H
#define H264E_ENC_MCDENOISE_H
#include "enc_denoise.h"

#define MCD_PITCH 6                         /* dwords per window row: four columns in front of the tile, 16, four behind */
#define MCD_NO_KEY 0x7fffffff
#define MCDENOISE_MIN_SIDE 16               /* pictures below 16x16 have no block (the cost pass' rule) */
#define MCDENOISE_CELL_BYTES 4

typedef struct
{
    const uint8_t *cur;                 /* the frame's input slot, packed I420 */
    const uint8_t *prev;                /* D_{f-1}, packed I420 */
    uint8_t *out;                       /* D_f */
    const uint32_t *field;              /* [nbx*nby] the frame's motion field (enc_lookahead_search.h cells) */
    uint32_t *cells;                    /* [nbx*nby] this filter's vectors */
    int width, height, nbx, nby;
} mcdenoise_args_t;

typedef struct
{
    uint32_t cur[18*MCD_PITCH];         /* rows -1..16 of the tile */
    uint32_t prev[20*MCD_PITCH];        /* rows -2..17 of the displaced tile */
    uint32_t zero[20*MCD_PITCH];        /* mode 2: the same at displacement zero */
    uint32_t T[64];                     /* k_denoise_gain */
} mcdenoise_lds_t;

/* refinement of candidate k = 1..9 in the order (|rx| + |ry|, ry, rx): (0,0) (0,-1) (-1,0) (1,0) (0,1) (-1,-1) (1,-1) (-1,1) (1,1), two bits
 * per candidate holding r + 1; candidate 0 is the vector (0, 0) itself and reads its own window at refinement (0, 0) */
DEV int mcd_rx(int k) { return (int)((0x88615u >> (2*k)) & 3u) - 1; }
DEV int mcd_ry(int k) { return (int)((0xA0945u >> (2*k)) & 3u) - 1; }

/* the four samples (x .. x + 3, y) of a plane as a dword.  fast: they and four bytes on either side lie inside the row */
DEV uint32_t mcd_load4(const gu8 *pl, int w, int h, int x, int y, int fast)
{
    if (fast)
    {
        const gu8 *p = pl + (size_t)y*(size_t)w + (size_t)x;
        const unsigned mis = (unsigned)((uintptr_t)p & 3);
        const GLOBAL_AS uint32_t *q = (const GLOBAL_AS uint32_t *)(p - mis);
        EMU_GLOBAL(q, 8);
        return alignbyte32(q[1], q[0], mis);
    }
    const gu8 *r = pl + (size_t)clip3(0, h - 1, y)*(size_t)w;
    uint32_t v = 0;
    for (int k = 0; k < 4; k++)
    {
        const gu8 *p = r + clip3(0, w - 1, x + k);
        EMU_GLOBAL(p, 1);
        v |= (uint32_t)*p << (8*k);
    }
    return v;
}

/* a window of ROWS rows x ND dwords whose first sample is (ox, oy) of the plane, coordinates clamped to the plane */
template <int ROWS, int ND> DEV void mcd_stage(LDS_AS uint32_t *dst, const gu8 *pl, int w, int h, int ox, int oy)
{
    const int fast = ox >= 4 && ox + 4*ND + 4 <= w && oy >= 0 && oy + ROWS <= h;
    WAVE_FOR(l)
        for (int i = l; i < ROWS*ND; i += 64)
        {
            const int r = i/ND, j = i - r*ND;
            dst[r*MCD_PITCH + j] = mcd_load4(pl, w, h, ox + 4*j, oy + r, fast);
        }
}

/* the dword at byte offset off of a window */
DEV uint32_t mcd_lds4(const LDS_AS uint32_t *win, int off)
{
    const LDS_AS uint32_t *p = win + (off >> 2);
    return alignbyte32(p[1], p[0], (unsigned)off & 3u);
}

/* byte offset in a D_{f-1} window of sample (4g, r) of the tile at refinement (rx, ry) */
DEV int mcd_off(int r, int g, int rx, int ry) { return (r + 2 + ry)*(4*MCD_PITCH) + 4 + 4*g + rx; }

/* lane l = (row l >> 2, group l & 3) of the 16x16 block: its four samples' part of the sad at refinement (rx, ry) */
DEV int mcd_sad(const LDS_AS uint32_t *cur, const LDS_AS uint32_t *win, int l, int rx, int ry)
{
    const int r = l >> 2, g = l & 3;
    return (int)sad4_u8(cur[(r + 1)*MCD_PITCH + 1 + g], mcd_lds4(win, mcd_off(r, g, rx, ry)), 0u);
}

/* the tile of T x T samples at (x0, y0) of one plane, cut at the plane's edge, filtered against the window at refinement (rx, ry) */
template <int T> DEV void mcd_filter(const LDS_AS uint8_t *gain, const LDS_AS uint32_t *cur, const LDS_AS uint32_t *win, int rx, int ry,
                                     gu8 *out, int w, int h, int x0, int y0)
{
    WAVE_FOR(l)
    {
        const int r = l/(T/4), g = l - r*(T/4), x = x0 + 4*g, y = y0 + r;
        if (r < T && x < w && y < h)
        {
            const LDS_AS uint32_t *c = cur + (r + 1)*MCD_PITCH + 1 + g;
            const int n = imin(4, w - x);
            uint32_t o = c[0];                      /* first / last row: out = cur */
            if (y > 0 && y < h - 1)
            {
                const int off = mcd_off(r, g, rx, ry);
                const LDS_AS uint8_t *pb = (const LDS_AS uint8_t *)win;
                o = denoise_quad(gain, c[-MCD_PITCH], mcd_lds4(win, off - 4*MCD_PITCH), c[0], mcd_lds4(win, off), c[MCD_PITCH], mcd_lds4(win, off + 4*MCD_PITCH),
                                 (int)(c[-1] >> 24), pb[off - 1], (int)(c[1] & 255u), pb[off + 4], x, w);
            }
            gu8 *q = out + (size_t)y*(size_t)w + (size_t)x;
            EMU_GLOBAL(q, n);
            if (n == 4 && !((uintptr_t)q & 3)) *(GLOBAL_AS uint32_t *)q = o;
            else for (int k = 0; k < n; k++) q[k] = (uint8_t)(o >> (8*k));
        }
    }
}

DEV void mcd_cell_store(const mcdenoise_args_t &A, int b, uint32_t cell)
{
    GLOBAL_AS uint32_t *q = (GLOBAL_AS uint32_t *)A.cells + b;
    EMU_GLOBAL(q, 4);
    *q = cell;
}

/* one workgroup: tile (bx, by) of all three planes.  MODE 1 = the field's vectors, 2 = refined */
template <int MODE> DEV void mcdenoise_block(const mcdenoise_args_t &A, LDS_AS mcdenoise_lds_t *sh, int bx, int by)
{
    const int w = A.width, h = A.height, cw = w >> 1, ch = h >> 1;
    const int covered = bx < A.nbx && by < A.nby;
    LDS_AS uint32_t *cur = (LDS_AS uint32_t *)sh->cur, *prev = (LDS_AS uint32_t *)sh->prev, *zero = (LDS_AS uint32_t *)sh->zero;
    const LDS_AS uint8_t *gain = (const LDS_AS uint8_t *)sh->T;
    int dx = 0, dy = 0;
    WAVE_FOR(l)
        ((LDS_AS uint32_t *)sh->T)[l] = (uint32_t)k_denoise_gain[4*l] | ((uint32_t)k_denoise_gain[4*l + 1] << 8) | ((uint32_t)k_denoise_gain[4*l + 2] << 16) | ((uint32_t)k_denoise_gain[4*l + 3] << 24);
    if (covered)
    {
        const GLOBAL_AS uint32_t *q = (const GLOBAL_AS uint32_t *)A.field + (by*A.nbx + bx);
        EMU_GLOBAL(q, 4);
        const uint32_t c = (uint32_t)uni((int)*q);
        dx = (int)(int8_t)(c & 255u); dy = (int)(int8_t)((c >> 8) & 255u);
    }
    /* luma */
    int vx = 2*dx, vy = 2*dy, rx = 0, ry = 0, at_zero = 0;
    mcd_stage<18, 6>(cur, (const gu8 *)A.cur, w, h, 16*bx - 4, 16*by - 1);
    mcd_stage<20, 6>(prev, (const gu8 *)A.prev, w, h, 16*bx + vx - 4, 16*by + vy - 2);
    if (MODE == 2 && covered) mcd_stage<20, 6>(zero, (const gu8 *)A.prev, w, h, 16*bx - 4, 16*by - 2);
    wave_sync();
    if (covered)
    {
        int sad;
        if (MODE == 2)
        {
            int s[8], t[4], key = MCD_NO_KEY;
            wave_sum8([&](int l, int v[8]) {
                v[0] = mcd_sad(cur, zero, l, 0, 0);
#pragma unroll
                for (int k = 1; k < 8; k++) v[k] = mcd_sad(cur, prev, l, mcd_rx(k), mcd_ry(k));
            }, s);
            wave_sum4([&](int l, int v[4]) { v[0] = mcd_sad(cur, prev, l, mcd_rx(8), mcd_ry(8)); v[1] = mcd_sad(cur, prev, l, mcd_rx(9), mcd_ry(9)); }, t);
#pragma unroll
            for (int k = 0; k < 10; k++)
            {
                const int cx = 16*bx + (k ? vx + mcd_rx(k) : 0), cy = 16*by + (k ? vy + mcd_ry(k) : 0);
                if (cx >= 0 && cx + 16 <= w && cy >= 0 && cy + 16 <= h) key = imin(key, ((k < 8 ? s[k] : t[k - 8]) << 4) | k);
            }
            const int k = key & 15;
            sad = key >> 4;
            if (k) { rx = mcd_rx(k); ry = mcd_ry(k); } else { at_zero = 1; vx = vy = 0; }
        }
        else sad = wave_sum([&](int l) { return mcd_sad(cur, prev, l, 0, 0); });
        const uint32_t cell = (uint32_t)((vx + rx) & 0xff) | ((uint32_t)((vy + ry) & 0xff) << 8) | ((uint32_t)sad << 16);
        WAVE_FOR(l) if (l == 0) mcd_cell_store(A, by*A.nbx + bx, cell);
    }
    mcd_filter<16>(gain, cur, at_zero ? zero : prev, rx, ry, (gu8 *)A.out, w, h, 16*bx, 16*by);
    /* chroma: the field's vector as it stands */
    for (int pl = 1; pl <= 2; pl++)
    {
        const size_t off = (size_t)w*(size_t)h + (pl == 2 ? (size_t)cw*(size_t)ch : 0);
        wave_sync();
        mcd_stage<10, 4>(cur, (const gu8 *)A.cur + off, cw, ch, 8*bx - 4, 8*by - 1);
        mcd_stage<12, 4>(prev, (const gu8 *)A.prev + off, cw, ch, 8*bx + dx - 4, 8*by + dy - 2);
        wave_sync();
        mcd_filter<8>(gain, cur, prev, 0, 0, (gu8 *)A.out + off, cw, ch, 8*bx, 8*by);
    }
}

#endif
