/*
 * enc_422.h -- device-resident input in 4:2:2, as capture hardware, pro-video decoders and cameras leave it: chroma of the luma's height
 * and half its width, in three planes (I422, ffmpeg's yuv422p), as a plane of U,V pairs (NV16, P210 / P216) or packed into ONE plane with
 * the luma (YUYV = YUY2: Y0 U Y1 V; UYVY: U Y0 V Y1; Y210 / Y216 the same of 16-bit words), 8-bit samples or 16-bit words of 9 .. 16
 * significant bits.  Next to the kernels of enc_ingest.h, enc_scale.h and enc_hbd.h, which stay the code they are; like them the frame is
 * reduced to the 8-bit 4:2:0 picture as the samples are loaded, and from there on it IS the 8-bit frame, byte for byte.  The reference has
 * none of this: this integer definition is the definition (tests/c422_model.py restates it).
 *
 *   - luma: copied, or quantised by hbd_quant (enc_hbd.h: the only quantiser);
 *   - chroma at the picture's size: U(i,j) = (a + b + 1) >> 1 with a = U422(i, 2j), b = U422(i, 2j + 1), the two 8-bit (quantised first)
 *     samples of one column in the row pair 2j, 2j + 1; V likewise; semi-planar and packed layouts are de-interleaved on the way;
 *   - through a window: enc_scale.h's exact area filter on the quantised samples, per plane.  A 4:2:2 chroma plane's window is
 *     Sw/2 x Sh at (cx/2, cy), reduced directly to Dw/2 x Dh/2 -- at Sw = Dw, Sh = Dh that is floor((2a + 2b + 2) / 4) = (a + b + 1) >> 1,
 *     so the at-size result, the pure crop and the plain ingest of the cropped region agree by construction.  No plane is reduced by
 *     more than 16:1: a 4:2:2 window may be 16 times the picture in width and 8 times in height.
 *
 * At the picture's size the ingest's shape is kept: one lane makes four consecutive output samples and writes them as one dword through
 * ing_store.  Four chroma samples come from two source rows; per row that is 4 bytes of a plane, 8 bytes of NV16, 16 bytes of a packed
 * row (twice that for 16-bit words), four packed luma samples are 8 source bytes: ONE wide load where all samples are wanted (ing_fetch for
 * 8-bit sources, which ask nothing of alignment; hbd_fetch for 16-bit ones, whose pointers and strides are multiples of 2), else sample
 * by sample, never a byte beyond the last sample of a row (a surface may end with its allocation).  Through the window the three steps of
 * enc_scale.h remain: scale_tile_422 gives the chroma planes their own geometry (half the width, the whole height) and rows per tile
 * (S.thc: their vertical ratio is twice the luma's); a packed source is three h264e_scale_comp_t over the one plane, step 2 (luma) and 4
 * (a chroma half) samples, base offset by the sample's place in its group; scale_hpass_pk is the 8-bit horizontal pass for those steps
 * (one byte load per tap: nothing outside the taps is read), 16-bit taps go through scale_hpass_hbd at any step.  h264e_kernels.hip runs
 * these as h264e_ingest_422_kernel<SB, PACK> and h264e_scale_422_kernel<SB>, h264e_pool.h's emulation launch (H264E_EMU) as lane loops.
 */
#ifndef H264E_ENC_422_H
#define H264E_ENC_422_H
#include "enc_hbd.h"

#define H264E_PACK_NONE 0               /* h264e_ingest_src_t.pack: planes (I422) or a plane of U,V pairs (NV16), by S.format */
#define H264E_PACK_YUYV 1               /* Y0 U Y1 V */
#define H264E_PACK_UYVY 2               /* U Y0 V Y1 */

/* the first ns <= 16 samples of SB bytes at p as 8-bit samples in v[4]: two fetches of eight (16 bytes each for 16-bit words), ONE of 16
 * bytes for an 8-bit source */
template <int SB> DEV void c422_fetch16(const h264e_ingest_src_t &S, const gu8 *p, int ns, uint32_t *v)
{
    if (SB == 1) { ing_fetch<16>(p, ns, v); return; }
    const int n0 = ns < 8 ? ns : 8;
    hbd_fetch8<SB>(S, p, n0, v);
    v[2] = v[3] = 0;
    if (ns > 8) hbd_fetch8<SB>(S, p + 8*SB, ns - 8, v + 2);
}

/* luma samples 4g .. min(4g + 3, width - 1) of row y into the slot at dst.  PACK: every other sample of the 2n at the group's place in
 * the packed row (width is even, so n is 2 or 4 and all 2n lie inside the row) */
template <int SB, int PACK> DEV void ingest_422_luma(const h264e_ingest_src_t &S, GLOBAL_AS uint8_t *dst, int g, int y)
{
    const int x0 = 4*g;
    if (x0 >= S.width || y >= S.height) return;
    const int n = S.width - x0 < 4 ? S.width - x0 : 4;
    const gu8 *row = (const gu8 *)S.plane[0] + (size_t)y*(size_t)S.stride[0];
    uint32_t o = 0;
    if (PACK)
    {
        uint32_t v[2];
        hbd_fetch8<SB>(S, row + (size_t)(2*x0)*SB, 2*n, v);
#pragma unroll
        for (int k = 0; k < 4; k++) o |= (uint32_t)ing_byte(v, 2*k + (PACK == H264E_PACK_UYVY)) << (8*k);
    } else o = hbd_fetch4<SB>(S, row + (size_t)x0*SB, n);
    ing_store(dst + (size_t)y*(size_t)S.width + x0, n, o);
}

/* chroma samples 4g .. of chroma row y of the PICTURE (width/2 x height/2 per plane), U and V: the rounded mean of source rows 2y and
 * 2y + 1, n samples per plane and row (I422), n U,V pairs (NV16) or n groups of four samples (packed) */
template <int SB, int PACK> DEV void ingest_422_chroma(const h264e_ingest_src_t &S, GLOBAL_AS uint8_t *dst, int g, int y)
{
    const int cw = S.width >> 1, ch = S.height >> 1, x0 = 4*g;
    if (x0 >= cw || y >= ch) return;
    const int n = cw - x0 < 4 ? cw - x0 : 4;
    uint32_t o[2] = { 0, 0 };
    if (PACK)
    {
        const gu8 *p0 = (const gu8 *)S.plane[0] + (size_t)(2*y)*(size_t)S.stride[0] + (size_t)(4*x0)*SB;
        const int iu = PACK == H264E_PACK_YUYV ? 1 : 0;             /* U at 4k + iu, V two samples on */
        uint32_t a[4], b[4];
        c422_fetch16<SB>(S, p0, 4*n, a);
        c422_fetch16<SB>(S, p0 + S.stride[0], 4*n, b);
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            o[0] |= (uint32_t)((ing_byte(a, 4*k + iu) + ing_byte(b, 4*k + iu) + 1) >> 1) << (8*k);
            o[1] |= (uint32_t)((ing_byte(a, 4*k + iu + 2) + ing_byte(b, 4*k + iu + 2) + 1) >> 1) << (8*k);
        }
    } else if (S.format == H264E_INGEST_NV12)
    {
        const gu8 *p0 = (const gu8 *)S.plane[1] + (size_t)(2*y)*(size_t)S.stride[1] + (size_t)(2*x0)*SB;
        uint32_t a[2], b[2];
        hbd_fetch8<SB>(S, p0, 2*n, a);
        hbd_fetch8<SB>(S, p0 + S.stride[1], 2*n, b);
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            o[0] |= (uint32_t)((ing_byte(a, 2*k) + ing_byte(b, 2*k) + 1) >> 1) << (8*k);
            o[1] |= (uint32_t)((ing_byte(a, 2*k + 1) + ing_byte(b, 2*k + 1) + 1) >> 1) << (8*k);
        }
    } else
    {
#pragma unroll
        for (int c = 0; c < 2; c++)
        {
            const gu8 *p0 = (const gu8 *)S.plane[1 + c] + (size_t)(2*y)*(size_t)S.stride[1 + c] + (size_t)x0*SB;
            const uint32_t a = hbd_fetch4<SB>(S, p0, n), b = hbd_fetch4<SB>(S, p0 + S.stride[1 + c], n);
#pragma unroll
            for (int k = 0; k < 4; k++) o[c] |= (uint32_t)((ing_byte(&a, k) + ing_byte(&b, k) + 1) >> 1) << (8*k);
        }
    }
    gu8 *du = dst + (size_t)S.width*(size_t)S.height + (size_t)y*(size_t)cw + x0;       /* samples beyond n are means of zeros: never stored */
    ing_store(du, n, o[0]);
    ing_store(du + (size_t)cw*(size_t)ch, n, o[1]);
}

/* ---- through a window */

/* scale_tile with a source geometry per plane and separate shifts per axis: a 4:2:2 chroma plane's window has half the luma's width and
 * ALL of its height, its destination half the picture in both, and rows per tile of its own (S.thc) */
DEV int scale_tile_422(const h264e_scale_src_t &S, int comp, int tx, int ty, ScaleTile &T)
{
    const int dsh = comp ? 1 : 0, shx = comp ? 1 : 0, shy = 0, th = comp ? S.thc : S.th;
    T.sw = S.sw >> shx; T.sh = S.sh >> shy; T.dw = S.dw >> dsh; T.dh = S.dh >> dsh;
    T.i0 = tx*SCL_TW; T.j0 = ty*th;
    if (T.i0 >= T.dw || T.j0 >= T.dh) return 0;
    T.ncols = T.dw - T.i0 < SCL_TW ? T.dw - T.i0 : SCL_TW;
    T.nrows = T.dh - T.j0 < th ? T.dh - T.j0 : th;
    return 1;
}

/* scale_hpass for the 8-bit samples of a packed row, item = r*64 + column: the same sum over the row's taps, every tap one byte load
 * at C.step 2 (luma) or 4 (a chroma half); no byte outside the taps is read, so the pass stays inside [C.lo, C.hi) */
DEV void scale_hpass_pk(LDS_AS ScaleLds *L, const h264e_scale_comp_t &C, const ScaleTile &T, int item)
{
    const int r = item >> 6, t = item & (SCL_TW - 1);
    if (t >= T.ncols || r >= scale_src_rows(L, T)) return;
    const int k0 = L->ck0[t], k1 = L->ck1[t];
    const uint32_t dw = (uint32_t)T.dw, a0 = (uint32_t)(T.i0 + t)*(uint32_t)T.sw;
    const gu8 *row = (const gu8 *)C.base + (size_t)(L->rl0[0] + r)*(size_t)C.stride;
    uint32_t sum = 0, first = 0, last = 0;
    for (int k = k0; k <= k1; k++)
    {
        const gu8 *p = row + (size_t)k*(size_t)C.step;
        EMU_GLOBAL(p, (size_t)1);
        last = *p;
        if (k == k0) first = last;
        sum += last;
    }
    L->hsum[r][t] = dw*sum - (a0 - (uint32_t)k0*dw)*first - (((uint32_t)k1 + 1u)*dw - (a0 + (uint32_t)T.sw))*last;
}

#endif
