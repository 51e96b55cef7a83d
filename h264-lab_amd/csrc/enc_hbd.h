/*
 * enc_hbd.h -- device-resident input as video decoders leave it: 16-bit samples (P010 / P012 / P016 surfaces, yuv420p10le tensors) and
 * 4:4:4 chroma, next to the 8-bit 4:2:0 kernels of enc_ingest.h and enc_scale.h, which stay the code they are.  Both are reduced to the
 * 8-bit 4:2:0 picture as the samples are loaded; from there on the frame IS the 8-bit frame, byte for byte.  The reference has neither:
 * this integer definition is the definition (tests/hbd_model.py restates it).
 *
 *   - 16-bit samples: unsigned little-endian words with d significant bits (9 .. 16), LSB aligned (an MSB-aligned P010 surface is d = 16),
 *         q = min(255, (v + (1 << (d - 9))) >> (d - 8))
 *     -- round half up, one clamp; words above 2^d - 1 saturate to 255.  hbd_quant below; the rounding constant and the shift are
 *     wave-uniform launch arguments.
 *   - 4:4:4 (U and V of the luma's size; the I420 layout only) at the picture's size: U(i,j) = (a + b + c + d + 2) >> 2 over the 2x2 block
 *     of the 8-bit (quantised) chroma samples, the rounded mean the RGB path uses; V likewise.
 *   - through a window: enc_scale.h's exact area filter on the quantised samples, per plane.  A 4:4:4 chroma plane's window is the
 *     luma's, Sw x Sh at (cx, cy), reduced directly to Dw/2 x Dh/2 -- at Sw = Dw that is exactly the 2x2 rounded mean, so the at-size
 *     result and the pure crop agree by construction.  No plane is reduced by more than 16:1, so a 4:4:4 window may be 8 times the
 *     picture at most.
 *
 * At the picture's size the ingest's shape is kept: one lane makes four consecutive output samples and writes them as one dword through
 * ing_store.  Four 16-bit samples are 8 bytes, four U,V pairs of P016 chroma 16 bytes, the 8 x 2 samples of a 4:4:4 chroma group 16 bytes
 * per row: ONE load of 8 or 16 bytes where all are wanted -- pointers and strides are multiples of the sample's 2 bytes (the host refuses
 * anything else), which is all such a load of global memory asks -- else sample by sample, never a byte beyond the last sample of a row
 * (a surface may end with its allocation).  Through the window the three steps of enc_scale.h remain; scale_tile_hbd gives every plane
 * its own source geometry and rows per tile, scale_hpass_hbd quantises the taps as it loads them (one 16-bit load per tap; step 4 for one
 * half of P016's interleaved chroma).  h264e_kernels.hip runs these as h264e_ingest_hbd_kernel<SB, C444> and h264e_scale_hbd_kernel<SB>,
 * h264e_pool.h's emulation launch (H264E_EMU) as lane loops.
 */
#ifndef H264E_ENC_HBD_H
#define H264E_ENC_HBD_H
#include "enc_scale.h"

/* THE quantiser of a 16-bit word: r = 1 << (d - 9), s = d - 8.  v + r < 2^17, the shifted value is at most 256 (d = 16 only) and the
 * clamp takes that.  The opaque barrier behind the shift keeps hipcc from folding "shift, clamp, pack" into v_ashr_pk_u8_i32
 * (tests/test_isa_tripwire.py) */
DEV uint32_t hbd_quant(uint32_t v, int r, int s)
{
    const int t = opaque_int((int)((v + (uint32_t)r) >> s));
    return (uint32_t)(t < 255 ? t : 255);
}

/* 16-bit sample k of the dwords w (as loaded) */
DEV uint32_t hbd_word(const uint32_t *w, int k) { return (w[k >> 1] >> (16*(k & 1))) & 0xffffu; }

/* one 16-bit sample at p (2-byte aligned) */
DEV uint32_t hbd_load(const gu8 *p)
{
    EMU_GLOBAL(p, (size_t)2);
    return *(const GLOBAL_AS uint16_t *)p;
}

#ifndef H264E_EMU
typedef uint32_t hbd_u32x4 __attribute__((ext_vector_type(4), aligned(2)));
#endif
/* the first ns of NS (4 or 8) 16-bit samples at p into w, two per dword: one load of 2 NS bytes where all are wanted, else sample by
 * sample (never a byte beyond p + 2 ns) */
template <int NS> DEV void hbd_fetch(const gu8 *p, int ns, uint32_t *w)
{
    if (ns == NS)
    {
        EMU_GLOBAL(p, (size_t)(2*NS));
#ifdef H264E_EMU
        memcpy(w, p, 2*NS);
#else
        if (NS == 8) { const hbd_u32x4 t = *(const GLOBAL_AS hbd_u32x4 *)p; w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w; }
        else { const fs_u32x2 t = *(const GLOBAL_AS fs_u32x2 *)p; w[0] = t.x; w[1] = t.y; }
#endif
        return;
    }
    for (int i = 0; i < NS/2; i++) w[i] = 0;
    for (int k = 0; k < NS; k++) if (k < ns) w[k >> 1] |= hbd_load(p + 2*k) << (16*(k & 1));
}

/* the first n <= 4 samples of SB bytes at p as 8-bit samples, sample k in bits 8k (what ing_fetch<4> makes of four bytes) */
template <int SB> DEV uint32_t hbd_fetch4(const h264e_ingest_src_t &S, const gu8 *p, int n)
{
    uint32_t o = 0;
    if (SB == 1) { ing_fetch<4>(p, n, &o); return o; }
    uint32_t w[2];
    hbd_fetch<4>(p, n, w);
#pragma unroll
    for (int k = 0; k < 4; k++) o |= hbd_quant(hbd_word(w, k), S.qround, S.qshift) << (8*k);
    return o;                                       /* samples beyond n are quantised zeros: never stored */
}

/* the first ns <= 8 samples of SB bytes at p as 8-bit samples in v[2] (what ing_fetch<8> makes of eight bytes) */
template <int SB> DEV void hbd_fetch8(const h264e_ingest_src_t &S, const gu8 *p, int ns, uint32_t *v)
{
    if (SB == 1) { ing_fetch<8>(p, ns, v); return; }
    uint32_t w[4];
    hbd_fetch<8>(p, ns, w);
    v[0] = v[1] = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) v[k >> 2] |= hbd_quant(hbd_word(w, k), S.qround, S.qshift) << (8*(k & 3));
}

/* ingest_luma for SB-byte samples: luma samples 4g .. min(4g + 3, width - 1) of row y into the slot at dst */
template <int SB> DEV void ingest_hbd_luma(const h264e_ingest_src_t &S, GLOBAL_AS uint8_t *dst, int g, int y)
{
    const int x0 = 4*g;
    if (x0 >= S.width || y >= S.height) return;
    const int n = S.width - x0 < 4 ? S.width - x0 : 4;
    const uint32_t o = hbd_fetch4<SB>(S, (const gu8 *)S.plane[0] + (size_t)y*(size_t)S.stride[0] + (size_t)x0*SB, n);
    ing_store(dst + (size_t)y*(size_t)S.width + x0, n, o);
}

/* ingest_chroma: chroma samples 4g .. of chroma row y, U and V.  C444: the rounded mean of the 2x2 blocks of 2n x 2 samples per plane;
 * else n samples per plane (I420) or n U,V pairs (NV12) */
template <int SB, int C444> DEV void ingest_hbd_chroma(const h264e_ingest_src_t &S, GLOBAL_AS uint8_t *dst, int g, int y)
{
    const int cw = S.width >> 1, ch = S.height >> 1, x0 = 4*g;
    if (x0 >= cw || y >= ch) return;
    const int n = cw - x0 < 4 ? cw - x0 : 4;
    uint32_t o[2] = { 0, 0 };
    if (C444)
    {
#pragma unroll
        for (int c = 0; c < 2; c++)
        {
            const gu8 *p0 = (const gu8 *)S.plane[1 + c] + (size_t)(2*y)*(size_t)S.stride[1 + c] + (size_t)(2*x0)*SB;
            uint32_t a[2], b[2];
            hbd_fetch8<SB>(S, p0, 2*n, a);
            hbd_fetch8<SB>(S, p0 + S.stride[1 + c], 2*n, b);
#pragma unroll
            for (int k = 0; k < 4; k++)
                o[c] |= (uint32_t)((ing_byte(a, 2*k) + ing_byte(a, 2*k + 1) + ing_byte(b, 2*k) + ing_byte(b, 2*k + 1) + 2) >> 2) << (8*k);
        }
    } else if (S.format == H264E_INGEST_NV12)
    {
        uint32_t v[2];
        hbd_fetch8<SB>(S, (const gu8 *)S.plane[1] + (size_t)y*(size_t)S.stride[1] + (size_t)(2*x0)*SB, 2*n, v);
#pragma unroll
        for (int k = 0; k < 4; k++) { o[0] |= (uint32_t)ing_byte(v, 2*k) << (8*k); o[1] |= (uint32_t)ing_byte(v, 2*k + 1) << (8*k); }
    } else
    {
        o[0] = hbd_fetch4<SB>(S, (const gu8 *)S.plane[1] + (size_t)y*(size_t)S.stride[1] + (size_t)x0*SB, n);
        o[1] = hbd_fetch4<SB>(S, (const gu8 *)S.plane[2] + (size_t)y*(size_t)S.stride[2] + (size_t)x0*SB, n);
    }
    gu8 *du = dst + (size_t)S.width*(size_t)S.height + (size_t)y*(size_t)cw + x0;
    ing_store(du, n, o[0]);
    ing_store(du + (size_t)cw*(size_t)ch, n, o[1]);
}

/* ---- through a window */

/* scale_tile with a source geometry per plane: a 4:4:4 chroma plane has the luma's window and half the picture, and rows per tile of
 * its own (S.thc: its ratio is twice the luma's) */
DEV int scale_tile_hbd(const h264e_scale_src_t &S, int comp, int tx, int ty, ScaleTile &T)
{
    const int dsh = comp ? 1 : 0, ssh = comp && !S.c444 ? 1 : 0, th = comp && S.c444 ? S.thc : S.th;
    T.sw = S.sw >> ssh; T.sh = S.sh >> ssh; T.dw = S.dw >> dsh; T.dh = S.dh >> dsh;
    T.i0 = tx*SCL_TW; T.j0 = ty*th;
    if (T.i0 >= T.dw || T.j0 >= T.dh) return 0;
    T.ncols = T.dw - T.i0 < SCL_TW ? T.dw - T.i0 : SCL_TW;
    T.nrows = T.dh - T.j0 < th ? T.dh - T.j0 : th;
    return 1;
}

/* scale_hpass for 16-bit samples, item = r*64 + column: the same sum over the row's taps, every tap one 2-byte load, quantised.  C.step
 * is 2, or 4 for one half of interleaved chroma; no byte outside the taps is read */
DEV void scale_hpass_hbd(LDS_AS ScaleLds *L, const h264e_scale_comp_t &C, const ScaleTile &T, int qround, int qshift, int item)
{
    const int r = item >> 6, t = item & (SCL_TW - 1);
    if (t >= T.ncols || r >= scale_src_rows(L, T)) return;
    const int k0 = L->ck0[t], k1 = L->ck1[t];
    const uint32_t dw = (uint32_t)T.dw, a0 = (uint32_t)(T.i0 + t)*(uint32_t)T.sw;
    const gu8 *row = (const gu8 *)C.base + (size_t)(L->rl0[0] + r)*(size_t)C.stride;
    uint32_t sum = 0, first = 0, last = 0;
    for (int k = k0; k <= k1; k++)
    {
        last = hbd_quant(hbd_load(row + (size_t)k*(size_t)C.step), qround, qshift);
        if (k == k0) first = last;
        sum += last;
    }
    L->hsum[r][t] = dw*sum - (a0 - (uint32_t)k0*dw)*first - (((uint32_t)k1 + 1u)*dw - (a0 + (uint32_t)T.sw))*last;
}

#endif
