/*
 * enc_ssim.h -- structural similarity of two 8-bit planes in HBM: the 8x8-window, step-4 SSIM that x264 prints and ffmpeg's `ssim` filter
 * computes, per plane.  The reference has no quality metric: this IS the definition (tests/ssim_model.py restates it).  A = the input
 * plane, B = the reconstruction, both w x h samples of the PICTURE (cropped size), rows a_stride / b_stride bytes apart:
 *
 *     block (i, j), i < bw = w >> 2, j < bh = h >> 2: the 4x4 samples at (4i, 4j); four integer sums  S a, S b, S (a^2 + b^2), S ab
 *     window (i, j), i < bw - 1, j < bh - 1: blocks (i..i+1, j..j+1); s1, s2, ss, s12 = the sums of theirs (64 samples)
 *     vars = 64 ss - s1^2 - s2^2, covar = 64 s12 - s1 s2, c1 = 416, c2 = 235963
 *     v = ((2 s1 s2 + c1) (2 covar + c2)) / ((s1^2 + s2^2 + c1) (vars + c2))
 *     the plane's value = (sum of v over the N = (bw - 1)(bh - 1) windows) / N
 *
 * Samples right of 4 bw and below 4 bh take no part.  The four factors are exact integers below 2^30 in magnitude (s1, s2 <= 16320,
 * ss <= 8323200), vars >= 0; they are converted to float64, then two float64 products and one float64 division (correctly rounded: hipcc's
 * v_div_scale / v_div_fmas / v_div_fixup sequence).  Identical planes give numerator == denominator, so exactly 1.0.
 *
 * One workgroup of 256 lanes makes a tile of SSIM_TW x SSIM_TW windows of one plane of one frame, in three steps with barriers between them:
 *   ssim_block   lane t takes block (t & 15, t >> 4) of the tile's SSIM_TB x SSIM_TB blocks (the tile's windows need one more block to the
 *                right and below: that halo row and column is the only source data two workgroups both read): four rows of four bytes of
 *                A and of B, as dwords where base and stride of both planes are dword aligned (the input slot's rows are w bytes apart:
 *                an 18-wide picture is not) and under enc_ingest.h's rule otherwise (ing_fetch: never a byte outside the block),
 *                v_sad_u8 for the two sums, v_dot4_u32_u8 for squares and products -> one 16-byte record in LDS;
 *   ssim_window  lane t takes window (t & 15, t >> 4) where there is one: four records from LDS (16-byte reads), v in float64 -> LDS
 *                (0.0 where the lane has no window);
 *   ssim_reduce  a tree over the lane index through LDS: step s = 128, 64 .. 1 adds red[t + s] to red[t] for t < s.  Lane 0 stores
 *                red[0] as the tile's partial.  The order of the additions is fixed by the indices alone.
 * A second launch (one workgroup per frame and plane) adds the partials: lane t those of tiles t, t + 256, ... in that order (ssim_gather),
 * then the same tree, then lane 0 divides by N and stores the plane's value.  No atomics: no result depends on which workgroup finishes
 * first, and h264e_pool.h's emulation launch (H264E_EMU), which runs these same functions as lane loops, adds in the same order.
 * LDS records: lane t reads and writes record t (+1, +16, +17 for a window), 16 bytes each: consecutive lanes, consecutive 16-byte words,
 * the conflict-free pattern of ds_read_b128 / ds_write_b128.
 */
#ifndef H264E_ENC_SSIM_H
#define H264E_ENC_SSIM_H
#include "enc_ingest.h"
#include "h264e_dev.h"

#define SSIM_TB 16                      /* blocks per tile side: 256 blocks, one per lane */
#define SSIM_TW (SSIM_TB - 1)           /* windows per tile side */
#define SSIM_C1 416                     /* (0.01 * 255)^2 * 64 + 0.5 */
#define SSIM_C2 235963                  /* (0.03 * 255)^2 * 64 * 63 + 0.5 */
#define SSIM_MIN_DIM 8                  /* one window */

/* what a launch compares.  chains != NULL: frame i of n, plane pl of 3 -- A = plane pl of the packed I420 input slot (in0 + i) % in_mod
 * (rows w bytes apart), B = the first picture of chain (pic0 + i) % pic_mod (coded pitch W): h264e_ssd_kernel's pair.  chains == NULL:
 * one pair of planes, a and b with their own strides. */
typedef struct
{
    const uint8_t *a;
    size_t frame_bytes;
    int in0, in_mod;
    const h264e_chain_dev_t *chains;
    int pic0, pic_mod;
    const uint8_t *b;
    int a_stride, b_stride;
    int width, height, W;               /* the picture (plane pair: the plane), and the coded pitch of its luma */
    int max_tiles;                      /* partials per frame and plane */
    double *partial;                    /* [n][planes][max_tiles] */
    double *out;                        /* [n][planes] */
} h264e_ssim_args_t;

typedef struct { const uint8_t *a, *b; int a_stride, b_stride, bw, bh, aligned; } ssim_plane_t;

/* a block's record: x = S a, y = S b, z = S (a^2 + b^2), w = S ab -- 16 bytes, 16-byte aligned: one LDS access each way */
#ifdef H264E_EMU
typedef struct __attribute__((aligned(16))) { uint32_t x, y, z, w; } ssim_blk_t;
#else
typedef uint32_t ssim_blk_t __attribute__((ext_vector_type(4)));
#endif
typedef struct
{
    ssim_blk_t blk[SSIM_TB*SSIM_TB];
    double red[256];
} SsimLds;

#define ssim_tiles(nwin) (((nwin) + SSIM_TW - 1)/SSIM_TW)      /* tiles along one axis (a macro: the host sizes the grid with it too) */

/* plane pl of frame i */
DEV ssim_plane_t ssim_plane(const h264e_ssim_args_t &A, int i, int pl)
{
    ssim_plane_t P;
    const int sh = pl ? 1 : 0, w = A.width >> sh, h = A.height >> sh;
    if (A.chains)
    {
        const GLOBAL_AS h264e_chain_dev_t *c = (const GLOBAL_AS h264e_chain_dev_t *)A.chains + (A.pic0 + i) % A.pic_mod;
        EMU_GLOBAL(c, sizeof(*c));
        P.a = A.a + A.frame_bytes*(size_t)((A.in0 + i) % A.in_mod) + (pl ? (size_t)A.width*A.height + (pl == 2 ? (size_t)(A.width/2)*(A.height/2) : 0) : 0);
        P.b = c->rec[0][pl];
        P.a_stride = w; P.b_stride = A.W >> sh;
    } else { P.a = A.a; P.b = A.b; P.a_stride = A.a_stride; P.b_stride = A.b_stride; }
    P.bw = w >> 2; P.bh = h >> 2;
    P.aligned = !((((uintptr_t)P.a | (uintptr_t)P.b) & 3) | ((P.a_stride | P.b_stride) & 3));
    return P;
}

#ifdef H264E_EMU
DEV uint32_t ssim_sum4(uint32_t v) { return (v & 255u) + ((v >> 8) & 255u) + ((v >> 16) & 255u) + (v >> 24); }
DEV uint32_t ssim_dot4(uint32_t a, uint32_t b, uint32_t acc)
{
    for (int k = 0; k < 4; k++) acc += ((a >> (8*k)) & 255u)*((b >> (8*k)) & 255u);
    return acc;
}
#else
DEV uint32_t ssim_sum4(uint32_t v) { return __builtin_amdgcn_sad_u8(v, 0u, 0u); }
DEV uint32_t ssim_dot4(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_udot4(a, b, acc, false); }
#endif

/* step 1, lane t: the sums of block (t & 15, t >> 4) of tile (tx, ty); zeros where the plane has no such block (no window uses them) */
DEV void ssim_block(LDS_AS SsimLds *L, const ssim_plane_t &P, int tx, int ty, int t)
{
    const int gx = tx*SSIM_TW + (t & (SSIM_TB - 1)), gy = ty*SSIM_TW + (t >> 4);
    ssim_blk_t r = { 0, 0, 0, 0 };
    if (gx < P.bw && gy < P.bh)
    {
        const gu8 *pa = (const gu8 *)P.a + (size_t)(4*gy)*(size_t)P.a_stride + (size_t)(4*gx);
        const gu8 *pb = (const gu8 *)P.b + (size_t)(4*gy)*(size_t)P.b_stride + (size_t)(4*gx);
        uint32_t va[4], vb[4];
        /* one decision per plane pair (base and stride of both dword aligned: every block row of both is), not one per row: the eight
         * loads of the usual case are issued back to back */
        if (P.aligned)
        {
#pragma unroll
            for (int y = 0; y < 4; y++)
            {
                EMU_GLOBAL(pa + (size_t)y*(size_t)P.a_stride, 4);
                EMU_GLOBAL(pb + (size_t)y*(size_t)P.b_stride, 4);
                va[y] = *(const GLOBAL_AS uint32_t *)(pa + (size_t)y*(size_t)P.a_stride);
                vb[y] = *(const GLOBAL_AS uint32_t *)(pb + (size_t)y*(size_t)P.b_stride);
            }
        } else
        {
#pragma unroll
            for (int y = 0; y < 4; y++)
            {
                ing_fetch<4>(pa + (size_t)y*(size_t)P.a_stride, 4, &va[y]);
                ing_fetch<4>(pb + (size_t)y*(size_t)P.b_stride, 4, &vb[y]);
            }
        }
#pragma unroll
        for (int y = 0; y < 4; y++)
        {
            r.x += ssim_sum4(va[y]);
            r.y += ssim_sum4(vb[y]);
            r.z = ssim_dot4(va[y], va[y], ssim_dot4(vb[y], vb[y], r.z));
            r.w = ssim_dot4(va[y], vb[y], r.w);
        }
    }
    L->blk[t] = r;
}

/* one window's value from its 64-sample sums */
DEV double ssim_value(uint32_t s1, uint32_t s2, uint32_t ss, uint32_t s12)
{
    const int32_t p12 = (int32_t)(s1*s2), sq = (int32_t)(s1*s1 + s2*s2);
    const int32_t vars = (int32_t)(64u*ss) - sq, covar = (int32_t)(64u*s12) - p12;
    const double num = (double)(2*p12 + SSIM_C1)*(double)(2*covar + SSIM_C2);
    const double den = (double)(sq + SSIM_C1)*(double)(vars + SSIM_C2);
    return num/den;
}

/* step 2, lane t: window (t & 15, t >> 4) of the tile, or 0.0 */
DEV void ssim_window(LDS_AS SsimLds *L, const ssim_plane_t &P, int tx, int ty, int t)
{
    const int bx = t & (SSIM_TB - 1), by = t >> 4;
    double v = 0.0;
    if (bx < SSIM_TW && by < SSIM_TW && tx*SSIM_TW + bx < P.bw - 1 && ty*SSIM_TW + by < P.bh - 1)
    {
        const ssim_blk_t a = L->blk[t], b = L->blk[t + 1], c = L->blk[t + SSIM_TB], d = L->blk[t + SSIM_TB + 1];
        v = ssim_value(a.x + b.x + c.x + d.x, a.y + b.y + c.y + d.y, a.z + b.z + c.z + d.z, a.w + b.w + c.w + d.w);
    }
    L->red[t] = v;
}

/* step 3, lane t, for s = 128, 64 .. 1 with a barrier after each */
DEV void ssim_reduce(LDS_AS double *red, int t, int s)
{
    if (t < s) red[t] += red[t + s];
}

/* the second launch, lane t: the partials of tiles t, t + 256, ... in that order */
DEV void ssim_gather(LDS_AS double *red, const GLOBAL_AS double *partial, int ntiles, int t)
{
    double acc = 0.0;
    for (int k = t; k < ntiles; k += 256) { EMU_GLOBAL(partial + k, sizeof(double)); acc += partial[k]; }
    red[t] = acc;
}

DEV void ssim_store(GLOBAL_AS double *dst, double v) { EMU_GLOBAL(dst, sizeof(double)); *dst = v; }

#endif
