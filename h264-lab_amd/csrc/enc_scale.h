/*
 * enc_scale.h -- device-resident input of another size: a window of one source frame in HBM (I420 or NV12, arbitrary row strides) is
 * reduced to the encoder's picture by an exact area (box) filter and written to the resident input slot, packed I420 -- the slot that
 * enc_ingest.h writes for a source of the picture's own size.  The reference has no scaler: this integer definition IS the definition
 * (tests/scale_model.py restates it).  Per plane, with the plane window Sw x Sh samples at (cx, cy), the destination Dw x Dh
 * (Dw <= Sw, Dh <= Sh), k a source column of the window and i a destination column:
 *
 *     wx(i,k)  = max(0, min((i+1) Sw, (k+1) Dw) - max(i Sw, k Dw))            (sum over k = Sw; wy(j,l) likewise with Sh, Dh)
 *     out(i,j) = floor((sum_l sum_k wy(j,l) wx(i,k) src(cx+k, cy+l) + ((Sw Sh) >> 1)) / (Sw Sh))
 *
 * S == D is a copy (a pure crop), 2:1 in both axes is (a + b + c + d + 2) >> 2, a constant plane stays constant, results are in 0..255
 * without a clamp.  Chroma: the same formula on Sw/2 x Sh/2 -> Dw/2 x Dh/2 at (cx/2, cy/2); the half-sample shift between the chroma
 * siting of the source and of the scaled picture is IGNORED (chroma is treated as co-sited with its own sample grid, as a plain box
 * filter per plane does).  NV12 chroma is de-interleaved on the way.  Limits: cx, cy, Sw, Sh even, the window inside the source,
 * Sw, Sh <= 4096 (the numerator stays below 2^32: 255 * 2^24 + 2^23), Sw <= 16 Dw and Sh <= 16 Dh (at most 17 taps per axis), no upscaling.
 *
 * One workgroup of 256 lanes makes a tile of SCL_TW x th destination samples of one plane (th <= SCL_TH_MAX, chosen by the host so that
 * the tile's source rows fit SCL_ROWS), in three steps with a barrier between them:
 *   scale_tables  the first and last tap of each of the tile's columns and rows: the only divisions by Dw / Dh, one pair per column / row;
 *   scale_hpass   one lane per (source row, destination column): the row's taps, fetched as the aligned dwords that enclose them
 *                 (bytes outside the taps masked away; byte loads only where such a dword would leave the window's bytes), summed
 *                 with weight Dw and corrected for the partial first and last tap -> a 32-bit sum (<= 255 Sw) in LDS;
 *   scale_vpass   one lane per (destination row, four columns): the column sums of the row's taps from LDS (16 bytes per read) with
 *                 their weights, rounded, divided by Sw Sh (a float estimate, corrected to the exact quotient), out as one dword.
 * No byte outside [first byte of the window's first row, last byte of its last row] is read -- the padding between the window's rows
 * may be (aligned dwords), so a source may end with its allocation; nothing is asked of the alignment of pointers or strides.
 * h264e_kernels.hip runs it as h264e_scale_kernel, h264e_pool.h's emulation launch (H264E_EMU) as lane loops.  Planar RGB sources go
 * through the same steps per channel and are converted from LDS: enc_scale_rgb.h.
 */
#ifndef H264E_ENC_SCALE_H
#define H264E_ENC_SCALE_H
#include "enc_ingest.h"

#define SCL_TW 64                       /* destination columns of a tile */
#define SCL_TH_MAX 32                   /* most destination rows of a tile */
#define SCL_ROWS 72                     /* most source rows of a tile: >= 4*16 + 2 */
#define SCL_MAX_DIM 4096
#define SCL_MAX_RATIO 16

/* one destination plane's source: sample (k, l) of the window is the byte at base + l*stride + k*step */
typedef struct
{
    const uint8_t *base;
    const uint8_t *lo, *hi;             /* the bytes that may be read: [lo, hi) */
    int stride, step;                   /* step 2: one half of NV12's interleaved chroma */
} h264e_scale_comp_t;

typedef struct
{
    h264e_scale_comp_t c[3];            /* Y, U, V */
    int sw, sh, dw, dh;                 /* luma window and picture, all even; the chroma planes have half of each */
    int th;                             /* destination rows per tile */
    h264e_color_t cm;                   /* planar RGB only (enc_scale_rgb.h) */
    int sample;                         /* H264E_SAMPLE_*: planar RGB only; float planes have step = the sample's bytes */
    int depth, c444, thc, tiles_y;      /* enc_hbd.h: 16-bit samples (0: 8-bit); 4:4:4 chroma, its destination rows per tile, and the rows of tiles of the plane with the most */
    int qround, qshift;                 /* ... the 16-bit quantiser: 1 << (depth - 9), depth - 8 */
    int c422, pack;                     /* enc_422.h: 4:2:2 chroma (rows per tile in thc); the three components share one packed plane */
} h264e_scale_src_t;

typedef struct
{
    uint32_t hsum[SCL_ROWS][SCL_TW];
    int ck0[SCL_TW], ck1[SCL_TW];       /* first and last tap (window column) of the tile's columns */
    int rl0[SCL_TH_MAX], rl1[SCL_TH_MAX];
} ScaleLds;

/* the plane's geometry and the tile's place in it */
struct ScaleTile
{
    int sw, sh, dw, dh;                 /* this plane's window and destination */
    int i0, j0, ncols, nrows;           /* the tile: first destination column / row, how many of each */
};
DEV int scale_tile(const h264e_scale_src_t &S, int comp, int tx, int ty, ScaleTile &T)
{
    const int sh = comp ? 1 : 0;
    T.sw = S.sw >> sh; T.sh = S.sh >> sh; T.dw = S.dw >> sh; T.dh = S.dh >> sh;
    T.i0 = tx*SCL_TW; T.j0 = ty*S.th;
    if (T.i0 >= T.dw || T.j0 >= T.dh) return 0;
    T.ncols = T.dw - T.i0 < SCL_TW ? T.dw - T.i0 : SCL_TW;
    T.nrows = T.dh - T.j0 < S.th ? T.dh - T.j0 : S.th;
    return 1;
}

/* step 1, lane t of 256: the taps of column t (t < 64) or of row t - 64 */
DEV void scale_tables(LDS_AS ScaleLds *L, const ScaleTile &T, int t)
{
    if (t < SCL_TW)
    {
        if (t >= T.ncols) return;
        const uint32_t a0 = (uint32_t)(T.i0 + t)*(uint32_t)T.sw;
        L->ck0[t] = (int)(a0/(uint32_t)T.dw);
        L->ck1[t] = (int)((a0 + (uint32_t)T.sw - 1u)/(uint32_t)T.dw);
    } else if (t - SCL_TW < T.nrows)
    {
        const uint32_t b0 = (uint32_t)(T.j0 + t - SCL_TW)*(uint32_t)T.sh;
        L->rl0[t - SCL_TW] = (int)(b0/(uint32_t)T.dh);
        L->rl1[t - SCL_TW] = (int)((b0 + (uint32_t)T.sh - 1u)/(uint32_t)T.dh);
    }
}
DEV int scale_src_rows(const LDS_AS ScaleLds *L, const ScaleTile &T) { return L->rl1[T.nrows - 1] - L->rl0[0] + 1; }

#ifdef H264E_EMU
DEV uint32_t scl_sum4(uint32_t v) { return (v & 255u) + ((v >> 8) & 255u) + ((v >> 16) & 255u) + (v >> 24); }
#else
DEV uint32_t scl_sum4(uint32_t v) { return __builtin_amdgcn_sad_u8(v, 0u, 0u); }
#endif

/* step 2, item = r*64 + column: the horizontal sum of source row rl0[0] + r for one destination column */
DEV void scale_hpass(LDS_AS ScaleLds *L, const h264e_scale_comp_t &C, const ScaleTile &T, int item)
{
    const int r = item >> 6, t = item & (SCL_TW - 1);
    if (t >= T.ncols || r >= scale_src_rows(L, T)) return;
    const int k0 = L->ck0[t], k1 = L->ck1[t];
    const uint32_t dw = (uint32_t)T.dw, a0 = (uint32_t)(T.i0 + t)*(uint32_t)T.sw;
    const gu8 *row = (const gu8 *)C.base + (size_t)(L->rl0[0] + r)*(size_t)C.stride;
    const gu8 *p0 = row + (size_t)k0*(size_t)C.step, *p1 = row + (size_t)k1*(size_t)C.step;        /* first and last tap */
    const gu8 *q0 = p0 - ((uintptr_t)p0 & 3), *q1 = p1 - ((uintptr_t)p1 & 3);                       /* ... and the dwords they lie in */
    uint32_t sum = 0, first, last;
    if (q0 >= (const gu8 *)C.lo && q1 + 4 <= (const gu8 *)C.hi)
    {
        /* the taps' bytes in an aligned dword: all of them, or every other one from p0's parity on */
        const uint32_t taps = C.step == 1 ? 0xffffffffu : ((uintptr_t)p0 & 1) ? 0xff00ff00u : 0x00ff00ffu;
        const uint32_t m0 = 0xffffffffu << (8*(unsigned)((uintptr_t)p0 & 3)), m1 = 0xffffffffu >> (8*(3 - (unsigned)((uintptr_t)p1 & 3)));
        EMU_GLOBAL(q0, (size_t)(q1 - q0) + 4);
        uint32_t v = *(const GLOBAL_AS uint32_t *)q0;
        first = (v >> (8*(unsigned)((uintptr_t)p0 & 3))) & 255u;
        if (q0 == q1) sum = scl_sum4(v & taps & m0 & m1);
        else
        {
            sum = scl_sum4(v & taps & m0);
            for (const gu8 *q = q0 + 4; q < q1; q += 4) sum += scl_sum4(*(const GLOBAL_AS uint32_t *)q & taps);
            v = *(const GLOBAL_AS uint32_t *)q1;
            sum += scl_sum4(v & taps & m1);
        }
        last = (v >> (8*(unsigned)((uintptr_t)p1 & 3))) & 255u;
    } else
    {
        EMU_GLOBAL(p0, (size_t)(p1 - p0) + 1);
        for (const gu8 *p = p0; p <= p1; p += C.step) sum += *p;
        first = *p0; last = *p1;
    }
    /* every tap with weight Dw, less what the first and the last tap have outside the column [a0, a0 + Sw) */
    L->hsum[r][t] = dw*sum - (a0 - (uint32_t)k0*dw)*first - (((uint32_t)k1 + 1u)*dw - (a0 + (uint32_t)T.sw))*last;
}

/* n / d for n < 2^32 and 0 < d <= 2^24 with a quotient <= 255: the float estimate (rd = 1.0f / d) is off by one at most, the remainder says which way */
DEV uint32_t scl_div(uint32_t n, uint32_t d, float rd)
{
    uint32_t q = (uint32_t)((float)n*rd);
    if ((uint64_t)q*d > n) q--;
    else if (n - q*d >= d) q++;
    return q;
}

/* four destination samples (columns x0 .. x0 + 3 of row jj of the tile), packed: the column sums of the row's taps from LDS with their weights,
 * rounded and divided */
DEV uint32_t scale_vrow(const LDS_AS ScaleLds *L, const ScaleTile &T, int jj, int x0)
{
    const int l0 = L->rl0[jj], l1 = L->rl1[jj], lbase = L->rl0[0];
    const uint32_t dh = (uint32_t)T.dh, b0 = (uint32_t)(T.j0 + jj)*(uint32_t)T.sh, b1 = b0 + (uint32_t)T.sh;
    uint32_t acc[4] = { 0, 0, 0, 0 };
    for (int l = l0; l <= l1; l++)
    {
        const uint32_t lo = (uint32_t)l*dh, hi = lo + dh, w = (hi < b1 ? hi : b1) - (lo > b0 ? lo : b0);
        const LDS_AS uint32_t *h = &L->hsum[l - lbase][x0];
        for (int k = 0; k < 4; k++) acc[k] += w*h[k];
    }
    const uint32_t area = (uint32_t)T.sw*(uint32_t)T.sh;
    const float rd = 1.0f/(float)area;
    uint32_t o = 0;
    for (int k = 0; k < 4; k++) o |= scl_div(acc[k] + (area >> 1), area, rd) << (8*k);
    return o;
}

/* step 3, item = row*16 + g: destination samples 4g .. 4g + 3 of one row of the tile into the slot's plane at dst (rows packed) */
DEV void scale_vpass(const LDS_AS ScaleLds *L, const ScaleTile &T, GLOBAL_AS uint8_t *dst, int item)
{
    const int jj = item >> 4, x0 = 4*(item & 15);
    if (jj >= T.nrows || x0 >= T.ncols) return;
    const int n = T.ncols - x0 < 4 ? T.ncols - x0 : 4;
    ing_store((gu8 *)dst + (size_t)(T.j0 + jj)*(size_t)T.dw + T.i0 + x0, n, scale_vrow(L, T, jj, x0));
}

/* where plane `comp` of the packed I420 slot starts */
DEV size_t scale_plane_offset(const h264e_scale_src_t &S, int comp)
{
    return comp ? (size_t)S.dw*(size_t)S.dh + (comp == 2 ? (size_t)(S.dw/2)*(size_t)(S.dh/2) : 0) : 0;
}

#endif
