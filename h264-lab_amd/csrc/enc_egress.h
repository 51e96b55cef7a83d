/*
 * enc_egress.h -- device-resident output, the counterpart of enc_ingest.h: one reconstructed picture as the pool keeps it (packed I420 at
 * the coded size W x H: W*H luma, then two (W/2)*(H/2) chroma planes, rows packed, W and H multiples of 16) is cropped to the picture's
 * width x height samples (both even, down to 2 x 2) and written into memory the caller owns, with the caller's strides:
 *
 *   - I420: three planes, each with its own pointer and stride: a cropping strided copy;
 *   - NV12: the luma plane as above, U and V interleaved into plane[1];
 *   - RGB:  interleaved 8-bit R,G,B of pixel_bytes 3 or 4 (the fourth byte is written as 255);
 *   - RGBP: three planes R, G, B (a CHW tensor, or three allocations), any channel and row strides -- 8-bit samples, or the same 8-bit
 *     values v as float32 v / 255 (ONE correctly rounded division), or as that float32 rounded to nearest even to float16 / bfloat16:
 *     (u8.float() / 255).to(dtype), bit for bit (tests/float_model.py).
 *
 * RGB and RGBP convert -- the reference has no such conversion, this integer definition IS the definition (tests/egress_model.py restates
 * it): every chroma sample serves its 2x2 block by replication (the counterpart of the ingest's 2x2 mean, no interpolation), and per pixel,
 * with C = Y - yo, D = U - 128, E = V - 128,
 *         R = clamp8((ky C + rv E + 128) >> 8),   G = clamp8((ky C + gu D + gv E + 128) >> 8),   B = clamp8((ky C + bu D + 128) >> 8)
 * (arithmetic shifts; the clamp to 0..255 is real: a coded picture can hold any Y, U, V triple).  The six numbers are the inverse of the
 * stream's matrix in 1/256 (h264e_icolor_t: BT.601 or BT.709, limited or full range, the rows of DESIGN.md 4.5g), launch arguments like
 * the forward matrix of the ingest.
 *
 * One lane makes four consecutive destination samples of a row (egress_luma, egress_chroma: the same four samples of U AND V) -- for RGB
 * and RGBP four pixels of TWO rows (egress_rgb): the two U and two V samples they share are fetched and multiplied once.  The source is
 * read as aligned dwords, which are always whole (rows of W or W/2 bytes, multiples of 8); the destination is stored as dwords where the
 * address is dword aligned and the group is whole, byte by byte otherwise (ing_store's rule: 101-byte chroma rows, 3-byte pixels on odd
 * strides, the ragged last group), and never outside [row start, row start + row bytes) of a row: the padding between rows is the
 * caller's.  Only raw addresses: nothing here knows how the destination was allocated.  h264e_kernels.hip runs it as h264e_egress_kernel,
 * h264e_pool.h's emulation launch (H264E_EMU) as a lane loop.
 */
#ifndef H264E_ENC_EGRESS_H
#define H264E_ENC_EGRESS_H
#include "enc_ingest.h"

/* the YCbCr -> RGB matrix in 1/256.  Wave-uniform launch arguments: they sit in SGPRs and feed the 24-bit multiplies directly (every
 * coefficient is below 2^10 in magnitude, every sample difference below 2^8: tests/test_egress_model.py, all 2^24 inputs) */
typedef struct { int ky, yo, rv, gu, gv, bu; } h264e_icolor_t;

typedef struct
{
    uint8_t *plane[3];
    int stride[3];                      /* bytes from row to row */
    int format, pixel_bytes;            /* H264E_INGEST_*; bytes per interleaved RGB pixel (3 or 4), ignored otherwise */
    int width, height;                  /* the picture: luma samples, both even */
    int W, H;                           /* the coded size of the source: multiples of 16 */
    h264e_icolor_t cm;                  /* RGB / RGBP only */
    int sample;                         /* H264E_SAMPLE_*: RGBP only, the launch picks the kernel by it (strides stay in bytes) */
} h264e_egress_dst_t;

/* the aligned dword at byte offset 4*i of a source row */
DEV uint32_t egr_dword(const gu8 *row, int i)
{
    EMU_GLOBAL(row + 4*i, 4);
    return *(const GLOBAL_AS uint32_t *)(row + 4*i);
}

/* the first nb of NB bytes of v (byte k in bits 8*(k & 3) of v[k >> 2]) to d: dwords where d is dword aligned and all NB bytes go out */
template <int NB> DEV void egr_store(gu8 *d, int nb, const uint32_t *v)
{
    EMU_GLOBAL(d, (size_t)nb);
    if (nb == NB && !((uintptr_t)d & 3))
    {
        for (int i = 0; i < NB/4; i++) *(GLOBAL_AS uint32_t *)(d + 4*i) = v[i];
        return;
    }
    for (int k = 0; k < NB; k++) if (k < nb) d[k] = (uint8_t)(v[k >> 2] >> (8*(k & 3)));
}

/* shift, then clamp: the opaque barrier behind the shift keeps hipcc from folding shift + clamp + pack into v_ashr_pk_u8_i32
 * (tests/test_isa_tripwire.py) */
DEV uint32_t egr_clamp8(int v)
{
    v = opaque_int(v >> 8);
    return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

/* what two pixels next to each other (and the two below them) share: the chroma terms of R, G and B, rounding included */
typedef struct { int r, g, b; } egr_chroma_t;
DEV egr_chroma_t egr_chroma_terms(const h264e_icolor_t &C, int u, int v)
{
    const int d = u - 128, e = v - 128;
    egr_chroma_t t;
    t.r = mul24(C.rv, e) + 128;
    t.g = mul24(C.gu, d) + mul24(C.gv, e) + 128;
    t.b = mul24(C.bu, d) + 128;
    return t;
}

/* luma samples 4g .. min(4g + 3, width - 1) of row y */
DEV void egress_luma(const h264e_egress_dst_t &D, const GLOBAL_AS uint8_t *src, int g, int y)
{
    const int x0 = 4*g;
    if (x0 >= D.width || y >= D.height) return;
    const int n = D.width - x0 < 4 ? D.width - x0 : 4;
    const uint32_t o = egr_dword(src + (size_t)y*(size_t)D.W, g);
    ing_store((gu8 *)D.plane[0] + (size_t)y*(size_t)D.stride[0] + x0, n, o);
}

/* chroma samples 4g .. of chroma row y (width/2 x height/2 samples per plane), U and V: two planes (I420) or interleaved pairs (NV12) */
DEV void egress_chroma(const h264e_egress_dst_t &D, const GLOBAL_AS uint8_t *src, int g, int y)
{
    const int cw = D.width >> 1, ch = D.height >> 1, x0 = 4*g;
    if (x0 >= cw || y >= ch) return;
    const int n = cw - x0 < 4 ? cw - x0 : 4;
    const gu8 *su = src + (size_t)D.W*(size_t)D.H + (size_t)y*(size_t)(D.W >> 1);
    const uint32_t u = egr_dword(su, g), v = egr_dword(su + (size_t)(D.W >> 1)*(size_t)(D.H >> 1), g);
    if (D.format == H264E_INGEST_NV12)
    {
        uint32_t o[2] = { 0, 0 };
#pragma unroll
        for (int k = 0; k < 4; k++) o[k >> 1] |= (((u >> (8*k)) & 255u) | (((v >> (8*k)) & 255u) << 8)) << (16*(k & 1));
        egr_store<8>((gu8 *)D.plane[1] + (size_t)y*(size_t)D.stride[1] + 2*x0, 2*n, o);
        return;
    }
    ing_store((gu8 *)D.plane[1] + (size_t)y*(size_t)D.stride[1] + x0, n, u);
    ing_store((gu8 *)D.plane[2] + (size_t)y*(size_t)D.stride[2] + x0, n, v);
}

/* the 8-bit value v as a float sample of type ST, in the low bits: float32 v / 255 -- a true division, correctly rounded, NOT v * (1 / 255.f), which differs
 * for 126 of the 256 values -- then narrowed.  "/" is that division in the emulation's compiler and, by default, in hipcc; the product's
 * Makefile names the option (-fhip-fp32-correctly-rounded-divide-sqrt) so that no other flag takes it away unnoticed, and
 * tests/test_gpu_float_io.py compares every one of the 256 quotients on the device */
template <int ST> DEV uint32_t egr_float_sample(uint32_t v)
{
    const float f = (float)(int)v/255.0f;
    return ST == H264E_SAMPLE_F32 ? fs_to_bits(f) : ST == H264E_SAMPLE_F16 ? fs_float_to_half(f) : fs_float_to_bf16(f);
}

/* n (2 or 4) samples c[] of a row as float samples to d: one store of 8 or 16 bytes where the group is whole -- d is a multiple of the
 * sample size, which is all such a store to global memory asks -- else sample by sample; never a byte beyond d + n samples */
template <int ST> DEV void egr_store_float(gu8 *d, int n, const uint32_t c[4])
{
    constexpr int SB = fs_bytes<ST>();
    EMU_GLOBAL(d, (size_t)(n*SB));
    uint32_t s[4];
#pragma unroll
    for (int k = 0; k < 4; k++) s[k] = egr_float_sample<ST>(c[k]);
    if (n == 4)
    {
#ifdef H264E_EMU
        if (SB == 4) memcpy(d, s, 16);
        else { const uint32_t t[2] = { s[0] | (s[1] << 16), s[2] | (s[3] << 16) }; memcpy(d, t, 8); }
#else
        if (SB == 4) { u32x4 t; t.x = s[0]; t.y = s[1]; t.z = s[2]; t.w = s[3]; *(GLOBAL_AS u32x4 *)d = t; }
        else { fs_u32x2 t; t.x = s[0] | (s[1] << 16); t.y = s[2] | (s[3] << 16); *(GLOBAL_AS fs_u32x2 *)d = t; }
#endif
        return;
    }
    for (int k = 0; k < 4; k++)
        if (k < n)
        {
            if (SB == 4) *(GLOBAL_AS uint32_t *)(d + 4*k) = s[k]; else *(GLOBAL_AS uint16_t *)(d + 2*k) = (uint16_t)s[k];
        }
}

/* pixels 4g .. min(4g + 3, width - 1) of rows 2y and 2y + 1, interleaved (PB = bytes per pixel) or planar (PB = 0, samples of type ST): n is
 * 2 or 4, the two rows share chroma row y, whose samples 2g and 2g + 1 are one half of an aligned dword */
template <int PB, int ST = H264E_SAMPLE_U8> DEV void egress_rgb(const h264e_egress_dst_t &D, const GLOBAL_AS uint8_t *src, int g, int y)
{
    const int x0 = 4*g;
    if (x0 >= D.width || 2*y >= D.height) return;
    const int n = D.width - x0 < 4 ? D.width - x0 : 4;
    const gu8 *su = src + (size_t)D.W*(size_t)D.H + (size_t)y*(size_t)(D.W >> 1);
    const uint32_t u = egr_dword(su, g >> 1) >> (16*(g & 1)), v = egr_dword(su + (size_t)(D.W >> 1)*(size_t)(D.H >> 1), g >> 1) >> (16*(g & 1));
    egr_chroma_t t[2];
#pragma unroll
    for (int k = 0; k < 2; k++) t[k] = egr_chroma_terms(D.cm, (int)((u >> (8*k)) & 255u), (int)((v >> (8*k)) & 255u));
#pragma unroll
    for (int r = 0; r < 2; r++)
    {
        const int row = 2*y + r;
        const uint32_t yy = egr_dword(src + (size_t)row*(size_t)D.W, g);
        uint32_t c[3][4];
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            const int l = mul24(D.cm.ky, (int)((yy >> (8*k)) & 255u) - D.cm.yo);
            c[0][k] = egr_clamp8(l + t[k >> 1].r); c[1][k] = egr_clamp8(l + t[k >> 1].g); c[2][k] = egr_clamp8(l + t[k >> 1].b);
        }
        if (PB == 0)
        {
#pragma unroll
            for (int ch = 0; ch < 3; ch++)
            {
                gu8 *d = (gu8 *)D.plane[ch] + (size_t)row*(size_t)D.stride[ch];
                if (ST == H264E_SAMPLE_U8) ing_store(d + x0, n, c[ch][0] | (c[ch][1] << 8) | (c[ch][2] << 16) | (c[ch][3] << 24));
                else egr_store_float<ST>(d + (size_t)x0*fs_bytes<ST>(), n, c[ch]);
            }
        } else
        {
            constexpr int NB = PB ? 4*PB : 4;
            uint32_t o[NB/4];
#pragma unroll
            for (int i = 0; i < NB/4; i++) o[i] = 0;
#pragma unroll
            for (int k = 0; k < 4; k++)
            {
#pragma unroll
                for (int ch = 0; ch < PB; ch++)
                {
                    const int at = PB*k + ch;
                    o[at >> 2] |= (ch < 3 ? c[ch][k] : 255u) << (8*(at & 3));
                }
            }
            egr_store<NB>((gu8 *)D.plane[0] + (size_t)row*(size_t)D.stride[0] + (size_t)x0*PB, n*PB, o);
        }
    }
}

/* what lane g of row y does, by format: part 0 = luma rows, 1 = chroma rows of I420 / NV12; the RGB formats have one part of height/2 rows */
DEV void egress_group(const h264e_egress_dst_t &D, const GLOBAL_AS uint8_t *src, int g, int y, int part)
{
    if (D.format == H264E_INGEST_RGBP) { if (!part) egress_rgb<0>(D, src, g, y); }
    else if (D.format == H264E_INGEST_RGB) { if (!part) { if (D.pixel_bytes == 4) egress_rgb<4>(D, src, g, y); else egress_rgb<3>(D, src, g, y); } }
    else if (part) egress_chroma(D, src, g, y);
    else egress_luma(D, src, g, y);
}

#endif
