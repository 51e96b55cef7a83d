/*
 * enc_ingest.h -- device-resident input: one source frame in HBM (I420, NV12, interleaved or planar RGB, arbitrary row strides) into the
 * encoder's resident input slot, packed I420 (width*height luma, then two (width/2)*(height/2) chroma planes, rows packed: exactly
 * what h264e_hip_upload_i420 leaves there), per sample group.
 *
 *   - I420: three planes, each with its own pointer and stride: a strided copy;
 *   - NV12: a luma plane and one plane of interleaved U,V pairs: the chroma rows are de-interleaved;
 *   - RGB:  interleaved 8-bit R,G,B, pixel_bytes = 3 or 4 (a fourth byte is ignored), BT.601 limited range in integers unless the caller
 *     chose another matrix -- the reference has no colour conversion, this IS the definition (tests/ingest_model.py restates it):
 *         Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16                                  per pixel,
 *         m = (a + b + c + d + 2) >> 2                                                 per channel over each 2x2 block, then
 *         U = ((-38 Rm - 74 Gm + 112 Bm + 128) >> 8) + 128,  V = ((112 Rm - 94 Gm - 18 Bm + 128) >> 8) + 128
 *     (arithmetic shifts; Y lands in 16..235, U and V in 16..240: nothing to clamp).  Width and height are even, so every block is whole.
 *     The nine coefficients and the luma offset are launch arguments (h264e_color_t: BT.601 or BT.709, limited or full range, the rows
 *     of DESIGN.md 4.5f, tests/color_model.py); every row keeps its results inside 8 bits without a clamp.
 *   - RGBP: planar 8-bit R, G, B (a CHW tensor, or three allocations), each plane with its own pointer and stride; the same arithmetic,
 *     so byte for byte what RGB gives for the same image.
 *   - RGBP with float samples (H264E_SAMPLE_F16 / _BF16 / _F32: a float tensor in [0, 1]): every sample is quantised to 8 bits as it is
 *     loaded -- fq_quant below IS the definition, tests/float_model.py restates it -- and from there on it is RGBP, byte for byte.
 *
 * One lane makes four consecutive output samples of one row: ingest_luma for the Y plane, ingest_chroma for the same four samples of
 * U AND V (both come from the same source bytes in NV12 and RGB).  Source bytes are fetched as dwords where the lane's source address
 * is dword aligned and the group is whole, byte by byte otherwise (101-byte chroma rows, 3-byte pixels on odd strides, the last group
 * of a row); the four output samples go out as one dword under the same rule.  Only raw addresses: nothing here knows how the source
 * was allocated.  h264e_kernels.hip runs it as h264e_ingest_kernel, h264e_pool.h's emulation launch (H264E_EMU) as a lane loop.
 */
#ifndef H264E_ENC_INGEST_H
#define H264E_ENC_INGEST_H
#include "wave.h"

#define H264E_INGEST_I420 0
#define H264E_INGEST_NV12 1
#define H264E_INGEST_RGB  2
#define H264E_INGEST_RGBP 3
/* the sample type of planar RGB (bits 4-5 of H264E_dev_frame_t.format, shifted down): 8-bit, or float16 / bfloat16 / float32 in [0, 1] */
#define H264E_SAMPLE_U8   0
#define H264E_SAMPLE_F16  1
#define H264E_SAMPLE_BF16 2
#define H264E_SAMPLE_F32  3

/* the RGB -> YCbCr matrix in 1/256: Y = ((y . RGB + 128) >> 8) + yo, U = ((u . RGBm + 128) >> 8) + 128, V likewise.  Wave-uniform launch
 * arguments: they sit in SGPRs and feed the 24-bit multiplies directly (every coefficient is below 2^8 in magnitude) */
typedef struct { int y[3], u[3], v[3], yo; } h264e_color_t;

typedef struct
{
    const uint8_t *plane[3];
    int stride[3];                      /* bytes from row to row */
    int format, pixel_bytes;            /* H264E_INGEST_*; bytes per interleaved RGB pixel (3 or 4), ignored otherwise */
    int width, height;                  /* luma samples: both even */
    h264e_color_t cm;                   /* RGB / RGBP only */
    int sample;                         /* H264E_SAMPLE_*: RGBP only, the launch picks the kernel by it (strides stay in bytes) */
    int depth, c444;                    /* enc_hbd.h: 16-bit samples with `depth` significant bits (0: 8-bit samples); U and V of the luma's size */
    int qround, qshift;                 /* ... and their quantiser: 1 << (depth - 9), depth - 8 */
    int c422, pack;                     /* enc_422.h: U and V of the luma's height and half its width; H264E_PACK_*: all three in plane[0] */
} h264e_ingest_src_t;

/* the first nb of NB source bytes at p into v, byte k in bits 8*(k & 3) of v[k >> 2]: dwords where p is dword aligned and all NB
 * bytes are wanted, else byte loads (never a byte beyond p + nb: the last row may end with its allocation) */
template <int NB> DEV void ing_fetch(const gu8 *p, int nb, uint32_t *v)
{
    EMU_GLOBAL(p, (size_t)nb);
    if (nb == NB && !((uintptr_t)p & 3))
    {
        for (int i = 0; i < NB/4; i++) v[i] = *(const GLOBAL_AS uint32_t *)(p + 4*i);
        return;
    }
    for (int i = 0; i < NB/4; i++) v[i] = 0;
    for (int k = 0; k < NB; k++) if (k < nb) v[k >> 2] |= (uint32_t)p[k] << (8*(k & 3));
}
DEV int ing_byte(const uint32_t *v, int k) { return (int)((v[k >> 2] >> (8*(k & 3))) & 255u); }

/* n <= 4 output samples (packed in o) to d: one dword where d is dword aligned and n = 4 */
DEV void ing_store(gu8 *d, int n, uint32_t o)
{
    EMU_GLOBAL(d, (size_t)n);
    if (n == 4 && !((uintptr_t)d & 3)) { *(GLOBAL_AS uint32_t *)d = o; return; }
    for (int k = 0; k < 4; k++) if (k < n) d[k] = (uint8_t)(o >> (8*k));
}

/* the matrix rows: results are in 0..255 by construction of every row the host hands over (no clamp); the opaque barrier keeps hipcc from
 * folding shift + pack into v_ashr_pk_u8_i32 (tests/test_isa_tripwire.py) */
DEV int ing_row(const int *c, int r, int g, int b) { return opaque_int((mul24(c[0], r) + mul24(c[1], g) + mul24(c[2], b) + 128) >> 8); }
DEV uint32_t ing_y(const h264e_color_t &C, int r, int g, int b) { return (uint32_t)(ing_row(C.y, r, g, b) + C.yo); }
DEV uint32_t ing_u(const h264e_color_t &C, int r, int g, int b) { return (uint32_t)(ing_row(C.u, r, g, b) + 128); }
DEV uint32_t ing_v(const h264e_color_t &C, int r, int g, int b) { return (uint32_t)(ing_row(C.v, r, g, b) + 128); }

/* PB = bytes per pixel: four luma samples from four pixels */
template <int PB> DEV uint32_t ing_rgb_luma(const h264e_color_t &C, const gu8 *p, int n)
{
    uint32_t v[PB], o = 0;
    ing_fetch<4*PB>(p, n*PB, v);
#pragma unroll
    for (int k = 0; k < 4; k++) o |= ing_y(C, ing_byte(v, PB*k), ing_byte(v, PB*k + 1), ing_byte(v, PB*k + 2)) << (8*k);
    return o;
}

/* ... and four U and four V samples from the 8 x 2 pixels at p0 (even row) and p1 (the row below it) */
template <int PB> DEV void ing_rgb_chroma(const h264e_color_t &C, const gu8 *p0, const gu8 *p1, int n, uint32_t &ou, uint32_t &ov)
{
    uint32_t a[2*PB], b[2*PB];
    ing_fetch<8*PB>(p0, 2*n*PB, a);
    ing_fetch<8*PB>(p1, 2*n*PB, b);
    ou = ov = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        int m[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
            m[ch] = (ing_byte(a, 2*PB*k + ch) + ing_byte(a, 2*PB*k + PB + ch) + ing_byte(b, 2*PB*k + ch) + ing_byte(b, 2*PB*k + PB + ch) + 2) >> 2;
        ou |= ing_u(C, m[0], m[1], m[2]) << (8*k);
        ov |= ing_v(C, m[0], m[1], m[2]) << (8*k);
    }
}

/* the same from three planes: four luma samples from the four bytes at r, g and b */
DEV uint32_t ing_rgbp_luma(const h264e_color_t &C, const gu8 *r, const gu8 *g, const gu8 *b, int n)
{
    uint32_t v[3], o = 0;
    ing_fetch<4>(r, n, &v[0]);
    ing_fetch<4>(g, n, &v[1]);
    ing_fetch<4>(b, n, &v[2]);
#pragma unroll
    for (int k = 0; k < 4; k++) o |= ing_y(C, ing_byte(&v[0], k), ing_byte(&v[1], k), ing_byte(&v[2], k)) << (8*k);
    return o;
}

/* four U and four V samples from the 2x2 block means of three channels: a[ch] holds 8 samples of the even row, b[ch] of the row below */
DEV void ing_rgbp_matrix(const h264e_color_t &C, const uint32_t a[3][2], const uint32_t b[3][2], uint32_t &ou, uint32_t &ov)
{
    ou = ov = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        int m[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) m[ch] = (ing_byte(a[ch], 2*k) + ing_byte(a[ch], 2*k + 1) + ing_byte(b[ch], 2*k) + ing_byte(b[ch], 2*k + 1) + 2) >> 2;
        ou |= ing_u(C, m[0], m[1], m[2]) << (8*k);
        ov |= ing_v(C, m[0], m[1], m[2]) << (8*k);
    }
}

/* luma samples 4g .. min(4g + 3, width - 1) of row y into the slot at dst */
DEV void ingest_luma(const h264e_ingest_src_t &S, GLOBAL_AS uint8_t *dst, int g, int y)
{
    const int x0 = 4*g;
    if (x0 >= S.width || y >= S.height) return;
    const int n = S.width - x0 < 4 ? S.width - x0 : 4;
    const gu8 *row = (const gu8 *)S.plane[0] + (size_t)y*(size_t)S.stride[0];
    uint32_t o;
    if (S.format == H264E_INGEST_RGB) o = S.pixel_bytes == 4 ? ing_rgb_luma<4>(S.cm, row + (size_t)x0*4, n) : ing_rgb_luma<3>(S.cm, row + (size_t)x0*3, n);
    else if (S.format == H264E_INGEST_RGBP)
        o = ing_rgbp_luma(S.cm, row + x0, (const gu8 *)S.plane[1] + (size_t)y*(size_t)S.stride[1] + x0, (const gu8 *)S.plane[2] + (size_t)y*(size_t)S.stride[2] + x0, n);
    else ing_fetch<4>(row + x0, n, &o);
    ing_store(dst + (size_t)y*(size_t)S.width + x0, n, o);
}

/* chroma samples 4g .. of chroma row y (width/2 x height/2 samples per plane), U and V */
DEV void ingest_chroma(const h264e_ingest_src_t &S, GLOBAL_AS uint8_t *dst, int g, int y)
{
    const int cw = S.width >> 1, ch = S.height >> 1, x0 = 4*g;
    if (x0 >= cw || y >= ch) return;
    const int n = cw - x0 < 4 ? cw - x0 : 4;
    uint32_t ou, ov;
    if (S.format == H264E_INGEST_RGB)
    {
        const gu8 *p0 = (const gu8 *)S.plane[0] + (size_t)(2*y)*(size_t)S.stride[0] + (size_t)(2*x0)*(size_t)S.pixel_bytes, *p1 = p0 + S.stride[0];
        if (S.pixel_bytes == 4) ing_rgb_chroma<4>(S.cm, p0, p1, n, ou, ov); else ing_rgb_chroma<3>(S.cm, p0, p1, n, ou, ov);
    } else if (S.format == H264E_INGEST_RGBP)
    {
        uint32_t a[3][2], b[3][2];
#pragma unroll
        for (int c = 0; c < 3; c++)
        {
            const gu8 *p0 = (const gu8 *)S.plane[c] + (size_t)(2*y)*(size_t)S.stride[c] + 2*x0;
            ing_fetch<8>(p0, 2*n, a[c]);
            ing_fetch<8>(p0 + S.stride[c], 2*n, b[c]);
        }
        ing_rgbp_matrix(S.cm, a, b, ou, ov);
    } else if (S.format == H264E_INGEST_NV12)
    {
        uint32_t v[2];
        ing_fetch<8>((const gu8 *)S.plane[1] + (size_t)y*(size_t)S.stride[1] + 2*x0, 2*n, v);
        ou = ov = 0;
        for (int k = 0; k < 4; k++) { ou |= (uint32_t)ing_byte(v, 2*k) << (8*k); ov |= (uint32_t)ing_byte(v, 2*k + 1) << (8*k); }
    } else
    {
        ing_fetch<4>((const gu8 *)S.plane[1] + (size_t)y*(size_t)S.stride[1] + x0, n, &ou);
        ing_fetch<4>((const gu8 *)S.plane[2] + (size_t)y*(size_t)S.stride[2] + x0, n, &ov);
    }
    gu8 *du = dst + (size_t)S.width*(size_t)S.height + (size_t)y*(size_t)cw + x0;
    ing_store(du, n, ou);
    ing_store(du + (size_t)cw*(size_t)ch, n, ov);
}

/* ---- float samples (planar RGB only).  ST = H264E_SAMPLE_*; a sample has fs_bytes<ST>() bytes, and pointers and strides are multiples of
 * that (the host refuses anything else), so a sample never straddles its own alignment. */
template <int ST> DEV constexpr int fs_bytes() { return ST == H264E_SAMPLE_F32 ? 4 : ST == H264E_SAMPLE_U8 ? 1 : 2; }

DEV float fs_from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
DEV uint32_t fs_to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

/* float16 <-> float32.  Widening is exact; narrowing rounds to nearest, ties to even.  TWO implementations of one function each: the
 * device's instructions (v_cvt_f32_f16, v_cvt_f16_f32), and integer code for the emulation, whose compiler need not know _Float16.  Both
 * results are fully determined by IEEE 754, and each is held to tests/float_model.py (itself checked against exact arithmetic by
 * tests/test_float_model.py): the integer code by tests/test_emu_float_io.py, the instructions by tests/test_gpu_float_io.py, both with
 * all 65536 patterns on the way in and all 256 values on the way out.  The emulation does not run the device's conversions. */
#ifdef H264E_EMU
DEV float fs_half_to_float(uint32_t h)
{
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
    if (e == 31) return fs_from_bits(sign | 0x7f800000u | (m << 13));                   /* inf, NaN */
    if (e) return fs_from_bits(sign | ((e + 112u) << 23) | (m << 13));
    if (!m) return fs_from_bits(sign);
    int sh = 0;                                                                          /* a denormal: normal in float32 */
    uint32_t mm = m;
    while (!(mm & 1024u)) { mm <<= 1; sh++; }
    return fs_from_bits(sign | ((uint32_t)(113 - sh) << 23) | ((mm & 1023u) << 13));
}
/* ONLY for f = 0 and 1/255 <= |f| <= 1, what the egress writes: normal in float16, no overflow, no NaN.  Anything else needs the
 * denormal and overflow cases this leaves out */
DEV uint32_t fs_float_to_half(float f)
{
    const uint32_t u = fs_to_bits(f);
    if (!(u & 0x7fffffffu)) return u >> 16;
    const uint32_t r = u + 0xfffu + ((u >> 13) & 1u);                                   /* nearest even at bit 13: a carry runs into the exponent, as it should */
    return ((u >> 16) & 0x8000u) | ((((r >> 23) & 255u) - 112u) << 10) | ((r >> 13) & 1023u);
}
#else
DEV float fs_half_to_float(uint32_t h) { const uint16_t b = (uint16_t)h; _Float16 x; __builtin_memcpy(&x, &b, 2); return (float)x; }
DEV uint32_t fs_float_to_half(float f) { const _Float16 x = (_Float16)f; uint16_t b; __builtin_memcpy(&b, &x, 2); return b; }
#endif
/* bfloat16 is the upper half of a float32; narrowing to nearest even (no NaN comes this way) */
DEV float fs_bf16_to_float(uint32_t h) { return fs_from_bits(h << 16); }
DEV uint32_t fs_float_to_bf16(float f) { const uint32_t u = fs_to_bits(f); return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16; }

/* THE quantiser: q = clamp(rint(x * 255), 0, 255) with ONE float32 multiply and round-to-nearest-even; NaN, -inf, negative values and
 * -0.0 give 0 (every comparison with a NaN is false), +inf and values above 1 give 255.  The clamp comes first -- 0 and 255 are integers
 * and rint is monotonic, so the result is the same -- which keeps the conversion in range.  Nothing to contract: the product feeds
 * comparisons, not an addition.  A denormal x (or a product that is one) rounds to 0 whether the hardware flushes it or not: 255 times
 * the largest float16 denormal is 0.016.  The opaque barrier keeps hipcc from looking through "convert, clamp, pack" (DESIGN.md 4.1). */
DEV uint32_t fq_quant(float x)
{
    float t = x*255.0f;
    t = t > 0.0f ? t : 0.0f;
    t = t < 255.0f ? t : 255.0f;
    return (uint32_t)opaque_int((int)__builtin_rintf(t));
}

/* sample k of the dwords v (as loaded) to float32 */
template <int ST> DEV float fs_sample(const uint32_t *v, int k)
{
    if (ST == H264E_SAMPLE_F32) return fs_from_bits(v[k]);
    const uint32_t h = (v[k >> 1] >> (16*(k & 1))) & 0xffffu;
    return ST == H264E_SAMPLE_F16 ? fs_half_to_float(h) : fs_bf16_to_float(h);
}

/* one sample at p (sample aligned) */
template <int ST> DEV float fs_load(const gu8 *p)
{
    EMU_GLOBAL(p, (size_t)fs_bytes<ST>());
    uint32_t v;
    if (ST == H264E_SAMPLE_F32) v = *(const GLOBAL_AS uint32_t *)p; else v = *(const GLOBAL_AS uint16_t *)p;
    return fs_sample<ST>(&v, 0);
}

/* the first n <= 4 samples at p, quantised, sample k in bits 8k (the packed dword ing_rgbp_luma makes of its bytes and ing_rgbp_matrix takes): ONE load of 8 or 16
 * bytes where all four are wanted -- p is a multiple of the sample size, which is all such a load of global memory asks -- else sample
 * by sample, never a byte beyond p + n samples (the last row may end with its allocation) */
#ifndef H264E_EMU
typedef uint32_t fs_u32x2 __attribute__((ext_vector_type(2), aligned(2)));
#endif
template <int ST> DEV uint32_t fin_fetch(const gu8 *p, int n)
{
    constexpr int SB = fs_bytes<ST>();
    uint32_t o = 0;
    if (n == 4)
    {
        uint32_t v[SB];
        EMU_GLOBAL(p, (size_t)(4*SB));
#ifdef H264E_EMU
        memcpy(v, p, 4*SB);
#else
        if (SB == 4) { const u32x4 t = *(const GLOBAL_AS u32x4 *)p; v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
        else { const fs_u32x2 t = *(const GLOBAL_AS fs_u32x2 *)p; v[0] = t.x; v[1] = t.y; }
#endif
#pragma unroll
        for (int k = 0; k < 4; k++) o |= fq_quant(fs_sample<ST>(v, k)) << (8*k);
        return o;
    }
    for (int k = 0; k < 4; k++) if (k < n) o |= fq_quant(fs_load<ST>(p + k*SB)) << (8*k);
    return o;
}

/* ingest_luma for float planes: luma samples 4g .. min(4g + 3, width - 1) of row y */
template <int ST> DEV void ingest_float_luma(const h264e_ingest_src_t &S, GLOBAL_AS uint8_t *dst, int g, int y)
{
    constexpr int SB = fs_bytes<ST>();
    const int x0 = 4*g;
    if (x0 >= S.width || y >= S.height) return;
    const int n = S.width - x0 < 4 ? S.width - x0 : 4;
    uint32_t v[3], o = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = fin_fetch<ST>((const gu8 *)S.plane[c] + (size_t)y*(size_t)S.stride[c] + (size_t)x0*SB, n);
#pragma unroll
    for (int k = 0; k < 4; k++) o |= ing_y(S.cm, ing_byte(&v[0], k), ing_byte(&v[1], k), ing_byte(&v[2], k)) << (8*k);      /* ing_rgbp_luma's row */
    ing_store(dst + (size_t)y*(size_t)S.width + x0, n, o);
}

/* ingest_chroma for float planes: chroma samples 4g .. of chroma row y, U and V, from 2n x 2 samples of each channel */
template <int ST> DEV void ingest_float_chroma(const h264e_ingest_src_t &S, GLOBAL_AS uint8_t *dst, int g, int y)
{
    constexpr int SB = fs_bytes<ST>();
    const int cw = S.width >> 1, ch = S.height >> 1, x0 = 4*g;
    if (x0 >= cw || y >= ch) return;
    const int n = cw - x0 < 4 ? cw - x0 : 4, n0 = 2*n < 4 ? 2*n : 4, n1 = 2*n - n0;
    uint32_t a[3][2], b[3][2], ou, ov;
#pragma unroll
    for (int c = 0; c < 3; c++)
    {
        const gu8 *p0 = (const gu8 *)S.plane[c] + (size_t)(2*y)*(size_t)S.stride[c] + (size_t)(2*x0)*SB, *p1 = p0 + S.stride[c];
        a[c][0] = fin_fetch<ST>(p0, n0); a[c][1] = n1 ? fin_fetch<ST>(p0 + 4*SB, n1) : 0u;
        b[c][0] = fin_fetch<ST>(p1, n0); b[c][1] = n1 ? fin_fetch<ST>(p1 + 4*SB, n1) : 0u;
    }
    ing_rgbp_matrix(S.cm, a, b, ou, ov);
    gu8 *du = dst + (size_t)S.width*(size_t)S.height + (size_t)y*(size_t)cw + x0;
    ing_store(du, n, ou);
    ing_store(du + (size_t)cw*(size_t)ch, n, ov);
}

#endif
