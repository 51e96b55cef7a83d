/*
 * enc_scale_rgb.h -- device-resident planar RGB input of another size: a window of three 8-bit planes R, G, B in HBM (a CHW tensor or
 * three allocations, arbitrary row strides) is reduced to the encoder's picture and converted to the packed I420 input slot.  The
 * definition is the composition of the two the project has (tests/rgbp_model.py restates it):
 *
 *     1. each of R, G, B: the window Sw x Sh at (cx, cy) -> Dw x Dh by enc_scale.h's exact area filter, rounded to 8 bits -- all three at
 *        luma geometry;
 *     2. that Dw x Dh RGB picture -> I420 by enc_ingest.h's matrix (the launch's h264e_color_t, as there): Y per pixel, U and V from the rounded 2x2 mean of each (already
 *        rounded) channel.  The double rounding of chroma is part of the definition: it is what scaling first and converting afterwards
 *        in two steps gives.
 *
 * Float planes (H264E_SAMPLE_F16 / _BF16 / _F32) are quantised by enc_ingest.h's fq_quant as the horizontal pass loads them
 * (scale_hpass_float): the filter works on the QUANTISED samples, so the slot is exactly that of the quantised 8-bit planes.
 *
 * So S == D is the plain planar ingest of the cropped region, and a constant colour stays that colour's Y, U, V at every ratio.  Limits
 * as for I420 (enc_scale.h).
 *
 * One workgroup of 256 lanes makes a tile of SCL_TW x th destination pixels of ALL THREE output planes (th even, <= SCL_TH_MAX, chosen by
 * the host so that the tile's source rows fit SCL_ROWS): scale_tables once -- the geometry is the same for the three channels -- then per
 * channel scale_hpass into hsum, a barrier, the vertical pass into an LDS tile of 8-bit samples instead of memory, a barrier (hsum is
 * reused by the next channel); then the conversion from the LDS tile: one lane per four luma samples of a row, one lane per four chroma
 * samples of a chroma row (U and V, from the 2x2 blocks), stored under ing_store's rules for ragged edges and unaligned slots.  Tiles
 * start at even rows and multiples of 64 columns of an even-sized picture, so every 2x2 block lies inside one tile.  The source is read
 * by scale_hpass alone: no byte outside [first byte of the window's first row, last byte of its last row] of each plane.
 * h264e_kernels.hip runs it as h264e_scale_rgb_kernel, h264e_pool.h's emulation launch (H264E_EMU) as lane loops.
 */
#ifndef H264E_ENC_SCALE_RGB_H
#define H264E_ENC_SCALE_RGB_H
#include "enc_scale.h"

typedef struct
{
    ScaleLds s;                                     /* the taps and one channel's horizontal sums at a time */
    uint32_t rgb[3][SCL_TH_MAX][SCL_TW/4];          /* the scaled tile: four 8-bit samples of a row per dword */
} ScaleRgbLds;

/* scale_hpass for float planes, item = r*64 + column: the same sum over the row's taps, every tap one sample-aligned load, quantised.
 * C.step is the sample's size; no byte outside the taps is read */
template <int ST> DEV void scale_hpass_float(LDS_AS ScaleLds *L, const h264e_scale_comp_t &C, const ScaleTile &T, int item)
{
    constexpr int SB = fs_bytes<ST>();
    const int r = item >> 6, t = item & (SCL_TW - 1);
    if (t >= T.ncols || r >= scale_src_rows(L, T)) return;
    const int k0 = L->ck0[t], k1 = L->ck1[t];
    const uint32_t dw = (uint32_t)T.dw, a0 = (uint32_t)(T.i0 + t)*(uint32_t)T.sw;
    const gu8 *row = (const gu8 *)C.base + (size_t)(L->rl0[0] + r)*(size_t)C.stride;
    uint32_t sum = 0, first = 0, last = 0;
    for (int k = k0; k <= k1; k++)
    {
        last = fq_quant(fs_load<ST>(row + (size_t)k*SB));
        if (k == k0) first = last;
        sum += last;
    }
    L->hsum[r][t] = dw*sum - (a0 - (uint32_t)k0*dw)*first - (((uint32_t)k1 + 1u)*dw - (a0 + (uint32_t)T.sw))*last;
}

/* the vertical pass of channel ch, item = row*16 + g: samples 4g .. 4g + 3 of one row of the tile into the LDS tile (whole dwords: what
 * lies beyond the tile's last column is never used) */
DEV void scale_rgb_vpass(LDS_AS ScaleRgbLds *L, const ScaleTile &T, int ch, int item)
{
    const int jj = item >> 4, g = item & 15;
    if (jj >= T.nrows || 4*g >= T.ncols) return;
    L->rgb[ch][jj][g] = scale_vrow(&L->s, T, jj, 4*g);
}

/* luma, item = row*16 + g: samples 4g .. 4g + 3 of one row of the tile into the slot at dst */
DEV void scale_rgb_luma(const h264e_color_t &C, const LDS_AS ScaleRgbLds *L, const ScaleTile &T, GLOBAL_AS uint8_t *dst, int item)
{
    const int jj = item >> 4, g = item & 15, x0 = 4*g;
    if (jj >= T.nrows || x0 >= T.ncols) return;
    const int n = T.ncols - x0 < 4 ? T.ncols - x0 : 4;
    const uint32_t r = L->rgb[0][jj][g], gr = L->rgb[1][jj][g], b = L->rgb[2][jj][g];
    uint32_t o = 0;
    for (int k = 0; k < 4; k++) o |= ing_y(C, ing_byte(&r, k), ing_byte(&gr, k), ing_byte(&b, k)) << (8*k);
    ing_store((gu8 *)dst + (size_t)(T.j0 + jj)*(size_t)T.dw + T.i0 + x0, n, o);
}

/* chroma, item = chroma row*8 + g: samples 4g .. 4g + 3 of one chroma row of the tile, U and V, from rows 2*row and 2*row + 1 of the LDS tile */
DEV void scale_rgb_chroma(const h264e_color_t &C, const LDS_AS ScaleRgbLds *L, const ScaleTile &T, GLOBAL_AS uint8_t *dst, int item)
{
    const int jc = item >> 3, g = item & 7, x0 = 4*g, ccols = T.ncols >> 1, cw = T.dw >> 1, ch = T.dh >> 1;
    if (2*jc >= T.nrows || x0 >= ccols) return;
    const int n = ccols - x0 < 4 ? ccols - x0 : 4;
    uint32_t a[3][2], b[3][2], ou, ov;
    for (int c = 0; c < 3; c++)
        for (int i = 0; i < 2; i++) { a[c][i] = L->rgb[c][2*jc][2*g + i]; b[c][i] = L->rgb[c][2*jc + 1][2*g + i]; }
    ing_rgbp_matrix(C, a, b, ou, ov);
    gu8 *du = (gu8 *)dst + (size_t)T.dw*(size_t)T.dh + (size_t)((T.j0 >> 1) + jc)*(size_t)cw + (T.i0 >> 1) + x0;
    ing_store(du, n, ou);
    ing_store(du + (size_t)cw*(size_t)ch, n, ov);
}

/* the conversion's work items of a tile: nrows*16 luma groups, then (nrows/2)*8 chroma groups */
DEV int scale_rgb_items(const ScaleTile &T) { return T.nrows*16 + (T.nrows >> 1)*8; }
DEV void scale_rgb_convert(const h264e_color_t &C, const LDS_AS ScaleRgbLds *L, const ScaleTile &T, GLOBAL_AS uint8_t *dst, int item)
{
    if (item < T.nrows*16) scale_rgb_luma(C, L, T, dst, item);
    else scale_rgb_chroma(C, L, T, dst, item - T.nrows*16);
}

#endif
