/*
 * enc_tonemap.h -- HDR10 device input: a 16-bit 4:2:0 decoder surface (I420 or NV12 layout, 10 .. 16 significant bits) that holds PQ
 * (SMPTE ST 2084) code values with BT.2020 non-constant-luminance chroma in limited range is tone-mapped to an 8-bit SDR R'G'B' picture
 * with BT.709 primaries and transfer, and that picture is converted to the encoder's input slot by the integer rows of h264e_color_t,
 * exactly as the RGB ingest (enc_ingest.h) converts an RGB picture.  A setting of the pool (h264e_hip_tonemap_set), not a format bit; a
 * pre-pass kernel next to the other ingests, which stay the code they are.  The reference has none of this: this definition is the
 * definition (tests/tonemap_model.py restates it in numpy, bit for bit).  Everything is integer arithmetic or single, individually
 * rounded float32 operations; the kernel holds no transcendental, no division and no fused multiply-add.
 *
 * Per 2x2 luma block with its one chroma pair (chroma is replicated over the block; the siting shift is ignored, as elsewhere):
 *   1. word to 10-bit code: c = min(1023, (v + r) >> s), s = d - 10, r = s ? 1 << (s - 1) : 0 (a 12-bit source is reduced to 10-bit codes);
 *   2. Y'CbCr to R'G'B' codes 0 .. 1023, full range, in Q14: with y = Y - 64, u = Cb - 512, v = Cr - 512
 *          R = clamp((ky y + crv v + 8192) >> 14), G = clamp((ky y - cgu u - cgv v + 8192) >> 14), B = clamp((ky y + cbu u + 8192) >> 14)
 *      (arithmetic shift, clamp to 0 .. 1023); ky, crv, cgu, cgv, cbu = TM_KY .. TM_CBU below.  |y| < 2^10, |u|, |v| <= 2^9 and every
 *      coefficient is below 2^16, so a product is below 2^26 and a sum of three with the rounding constant below 2^28: 32 bits hold it;
 *   3. linear light and the tone scale, by table: m = max(R, G, B) of the codes (the EOTF is monotone), L_ch = eotf[ch] * scale[m], one
 *      float32 multiply per channel; eotf[c] = 10000 PQ_EOTF(c / 1023) / ref_white, scale[c] = t(min(x, p)) / x with x that value and
 *      p = peak / ref_white (1 where x = 0), t the curve (tonemap_tables below);
 *   4. gamut, BT.2020 to BT.709, BT.2087's matrix as float32 constants: o = (m0 L_R + m1 L_G) + m2 L_B, three multiplies and two adds,
 *      each rounded on its own (tm_mul / tm_add).  Out-of-gamut values are clipped by step 5;
 *   5. BT.709 OETF to the 8-bit code, exactly rounded by threshold: code = #{k in 1 .. 255 : o >= thresh[k]}, thresh[k] the float32 of
 *      the inverse OETF at (k - 0.5) / 255.  thresh is non-decreasing, so the count is a binary search of 8 compares; negative values
 *      give 0, over-range values 255, and a NaN cannot occur (every table entry is finite and not negative);
 *   6. to the slot: Y per pixel, U and V from the rounded 2x2 mean of each channel, by ing_y / ing_u / ing_v of enc_ingest.h.
 *
 * One lane makes two blocks: the 4 x 2 luma samples at column 4g of the row pair 2j, 2j + 1 and their two chroma samples per plane.  A
 * luma row of the lane is ONE 8-byte load, its chroma one 4-byte load per plane (I420) or one 8-byte load (NV12); pointers and strides
 * are multiples of the sample's 2 bytes (the host refuses anything else), which is all such a load of global memory asks.  Width is
 * even, so the last lane of a row has 4 or 2 samples, and then loads exactly those: never a byte beyond a row's last sample (a surface
 * may end with its allocation).  The three tables (TM_TABLE_FLOATS floats, 9 KB) are staged in LDS once per workgroup.  Four luma
 * samples of a row go out as one dword through ing_store, the two chroma samples per plane as bytes.  The destination is a packed I420
 * picture of S.width x S.height: the input slot, or for a window the pool's scratch surface, from which enc_scale.h's kernel runs as for
 * any 8-bit I420 source.  h264e_kernels.hip runs this as h264e_tonemap_kernel<LAYOUT>, h264e_pool.h's emulation launch (H264E_EMU) as a
 * lane loop.
 */
#ifndef H264E_ENC_TONEMAP_H
#define H264E_ENC_TONEMAP_H
#include "enc_hbd.h"

#define H264E_TM_OFF 0                  /* = H264E_TONEMAP_* and H264E_TONECURVE_* of include/h264e_mi355x.h */
#define H264E_TM_PQ 1
#define H264E_TM_HABLE 0
#define H264E_TM_REINHARD 1
#define H264E_TM_CLIP 2

/* rint(16384 x) of ky = 1023/876, crv = 1.4746 * 1023/896, cgu = (0.0593 * 1.8814 / 0.6780) * 1023/896,
 * cgv = (0.2627 * 1.4746 / 0.6780) * 1023/896, cbu = 1.8814 * 1023/896: ycc[0 .. 4]; ycc[5 .. 7] = the luma offset, the chroma offset, the shift */
#define TM_KY  19133
#define TM_CRV 27584
#define TM_CGU 3078
#define TM_CGV 10688
#define TM_CBU 35194
#define TM_YOFF 64
#define TM_COFF 512
#define TM_SHIFT 14

#define TM_EOTF 0                       /* the tables in one array: eotf[1024], scale[1024], thresh[256] (thresh[0] is not used) */
#define TM_SCALE 1024
#define TM_THRESH 2048
#define TM_TABLE_FLOATS 2304

typedef struct
{
    const uint8_t *plane[3];            /* the first sample of the picture (or of the window) in every plane */
    int stride[3];                      /* bytes from row to row */
    int format;                         /* H264E_INGEST_I420 or H264E_INGEST_NV12 */
    int width, height;                  /* luma samples: both even */
    int qround, qshift;                 /* step 1: r and s */
    h264e_color_t cm;                   /* step 6 */
    const float *tables;                /* device memory: TM_TABLE_FLOATS floats */
} h264e_tonemap_src_t;

/* one float32 multiply / add, rounded on its own: nothing may fuse the two.  The device build switches contraction off where the
 * operation is written (the flag sits on the instruction, so inlining does not bring it back); the emulation's compiler gets a barrier
 * behind every result */
#ifdef H264E_EMU
DEV float tm_mul(float a, float b) { float r = a*b; __asm__ volatile("" : "+m"(r)); return r; }
DEV float tm_add(float a, float b) { float r = a + b; __asm__ volatile("" : "+m"(r)); return r; }
#else
DEV float tm_mul(float a, float b)
{
#pragma clang fp contract(off)
    return a*b;
}
DEV float tm_add(float a, float b)
{
#pragma clang fp contract(off)
    return a + b;
}
typedef uint32_t tm_u32a2 __attribute__((aligned(2)));
#endif

/* entry t of the tables into LDS, t = the lane of 256: 9 floats each */
DEV void tm_stage(LDS_AS float *L, const float *tables, int t)
{
    for (int i = t; i < TM_TABLE_FLOATS; i += 256)
    {
        const GLOBAL_AS float *p = (const GLOBAL_AS float *)tables + i;
        EMU_GLOBAL(p, (size_t)4);
        L[i] = *p;
    }
}

/* ns = 4, 2 or 1 16-bit samples at p (2-byte aligned) into w, two per dword: ONE load of exactly 2 ns bytes */
DEV void tm_fetch(const gu8 *p, int ns, uint32_t *w)
{
    EMU_GLOBAL(p, (size_t)(2*ns));
    w[0] = w[1] = 0;
#ifdef H264E_EMU
    memcpy(w, p, (size_t)(2*ns));
#else
    if (ns == 4) { const fs_u32x2 t = *(const GLOBAL_AS fs_u32x2 *)p; w[0] = t.x; w[1] = t.y; }
    else if (ns == 2) w[0] = *(const GLOBAL_AS tm_u32a2 *)p;
    else w[0] = *(const GLOBAL_AS uint16_t *)p;
#endif
}

/* step 1 */
DEV int tm_code(uint32_t v, int r, int s)
{
    const int t = (int)((v + (uint32_t)r) >> s);
    return t < 1023 ? t : 1023;
}
DEV int tm_clamp10(int v) { return v < 0 ? 0 : v > 1023 ? 1023 : v; }

/* step 5: the number of thresholds 1 .. 255 that o reaches; lo + step never exceeds 255 */
DEV int tm_oetf(const LDS_AS float *th, float o)
{
    int lo = 0;
#pragma unroll
    for (int step = 128; step; step >>= 1) if (o >= th[lo + step]) lo += step;
    return lo;
}

/* steps 2 to 5 of one pixel: the luma term l = ky y + 8192 and the block's chroma terms in, the 8-bit R'G'B' out */
DEV void tm_pixel(const LDS_AS float *T, int l, int rv, int guv, int bu, int *rgb)
{
    const int R = tm_clamp10((l + rv) >> TM_SHIFT), G = tm_clamp10((l - guv) >> TM_SHIFT), B = tm_clamp10((l + bu) >> TM_SHIFT);
    const int m = R > G ? (R > B ? R : B) : (G > B ? G : B);
    const float sc = T[TM_SCALE + m];
    const float lr = tm_mul(T[TM_EOTF + R], sc), lg = tm_mul(T[TM_EOTF + G], sc), lb = tm_mul(T[TM_EOTF + B], sc);
    const LDS_AS float *th = T + TM_THRESH;
    rgb[0] = tm_oetf(th, tm_add(tm_add(tm_mul(1.6605f, lr), tm_mul(-0.5876f, lg)), tm_mul(-0.0728f, lb)));
    rgb[1] = tm_oetf(th, tm_add(tm_add(tm_mul(-0.1246f, lr), tm_mul(1.1329f, lg)), tm_mul(-0.0083f, lb)));
    rgb[2] = tm_oetf(th, tm_add(tm_add(tm_mul(-0.0182f, lr), tm_mul(-0.1006f, lg)), tm_mul(1.1187f, lb)));
}

/* luma samples 4g .. 4g + n - 1 (n = 4, or 2 at the end of a row) of rows 2j and 2j + 1 and chroma samples 2g .. of chroma row j, into
 * the packed I420 picture at dst; T = the staged tables */
DEV void tonemap_group(const h264e_tonemap_src_t &S, const LDS_AS float *T, GLOBAL_AS uint8_t *dst, int g, int j)
{
    const int x0 = 4*g, cw = S.width >> 1, ch = S.height >> 1;
    if (x0 >= S.width || j >= ch) return;
    const int n = S.width - x0 < 4 ? 2 : 4, nb = n >> 1;
    uint32_t wy[2][2], wc[2][2];
    const gu8 *py = (const gu8 *)S.plane[0] + (size_t)(2*j)*(size_t)S.stride[0] + (size_t)x0*2;
    tm_fetch(py, n, wy[0]);
    tm_fetch(py + S.stride[0], n, wy[1]);
    if (S.format == H264E_INGEST_NV12)
    {
        uint32_t w[2];
        tm_fetch((const gu8 *)S.plane[1] + (size_t)j*(size_t)S.stride[1] + (size_t)x0*2, n, w);
        wc[0][0] = hbd_word(w, 0) | hbd_word(w, 2) << 16; wc[1][0] = hbd_word(w, 1) | hbd_word(w, 3) << 16;
    } else
    {
        tm_fetch((const gu8 *)S.plane[1] + (size_t)j*(size_t)S.stride[1] + (size_t)x0, nb, wc[0]);
        tm_fetch((const gu8 *)S.plane[2] + (size_t)j*(size_t)S.stride[2] + (size_t)x0, nb, wc[1]);
    }
    uint32_t oy[2] = { 0, 0 }, ou = 0, ov = 0;
#pragma unroll
    for (int k = 0; k < 2; k++)                     /* block k: a block beyond nb is made of zero words and never stored */
    {
        const int u = tm_code(hbd_word(wc[0], k), S.qround, S.qshift) - TM_COFF, v = tm_code(hbd_word(wc[1], k), S.qround, S.qshift) - TM_COFF;
        const int rv = TM_CRV*v, guv = TM_CGU*u + TM_CGV*v, bu = TM_CBU*u;
        int sum[3] = { 2, 2, 2 };
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int i = 0; i < 2; i++)
            {
                int rgb[3];
                tm_pixel(T, TM_KY*(tm_code(hbd_word(wy[r], 2*k + i), S.qround, S.qshift) - TM_YOFF) + (1 << (TM_SHIFT - 1)), rv, guv, bu, rgb);
                oy[r] |= ing_y(S.cm, rgb[0], rgb[1], rgb[2]) << (8*(2*k + i));
                sum[0] += rgb[0]; sum[1] += rgb[1]; sum[2] += rgb[2];
            }
        ou |= ing_u(S.cm, sum[0] >> 2, sum[1] >> 2, sum[2] >> 2) << (8*k);
        ov |= ing_v(S.cm, sum[0] >> 2, sum[1] >> 2, sum[2] >> 2) << (8*k);
    }
    gu8 *dy = dst + (size_t)(2*j)*(size_t)S.width + x0;
    ing_store(dy, n, oy[0]);
    ing_store(dy + S.width, n, oy[1]);
    gu8 *du = dst + (size_t)S.width*(size_t)S.height + (size_t)j*(size_t)cw + (x0 >> 1);
    ing_store(du, nb, ou);
    ing_store(du + (size_t)cw*(size_t)ch, nb, ov);
}

/* ---- the tables, on the host in double: ONE function for H264E_tonemap_tables and for the encoder (h264e_hip_tonemap_set) */
#include <math.h>

/* SMPTE ST 2084: the display light of the signal e in [0, 1], as a fraction of 10000 cd/m2 */
static double tm_pq_eotf(double e)
{
    const double m1 = 2610.0/16384.0, m2 = 2523.0/4096.0*128.0, c1 = 3424.0/4096.0, c2 = 2413.0/4096.0*32.0, c3 = 2392.0/4096.0*32.0;
    const double q = pow(e, 1.0/m2), num = q - c1 > 0.0 ? q - c1 : 0.0;
    return pow(num/(c2 - c3*q), 1.0/m1);
}
static double tm_hable(double x)
{
    const double A = 0.15, B = 0.50, C = 0.10, D = 0.20, E = 0.02, F = 0.30;
    return (x*(A*x + C*B) + D*E)/(x*(A*x + B) + D*F) - E/F;
}
/* the tone curve t on [0, p], p = peak / ref_white: t(p) = 1 for every curve */
static double tm_curve(int curve, double x, double p)
{
    if (curve == H264E_TM_CLIP) return x < 1.0 ? x : 1.0;
    if (curve == H264E_TM_REINHARD) return x*(1.0 + x/(p*p))/(1.0 + x);
    return tm_hable(x)/tm_hable(p);
}
/* the parameters with their defaults filled in, or the refusal: who names the caller, err takes the text (the value in it) */
static int tonemap_params(const char *who, int transfer, int curve, double *peak, double *ref_white, char *err, size_t nerr)
{
    if (transfer != H264E_TM_OFF && transfer != H264E_TM_PQ) { snprintf(err, nerr, "%s: transfer %d (0 = off, 1 = PQ)", who, transfer); return -1; }
    if (curve != H264E_TM_HABLE && curve != H264E_TM_REINHARD && curve != H264E_TM_CLIP) { snprintf(err, nerr, "%s: curve %d (0 = hable, 1 = reinhard, 2 = clip)", who, curve); return -1; }
    if (!(*ref_white == *ref_white) || *ref_white - *ref_white != 0.0) { snprintf(err, nerr, "%s: ref_white_nits %g is not finite", who, *ref_white); return -1; }
    if (!(*peak == *peak) || *peak - *peak != 0.0) { snprintf(err, nerr, "%s: peak_nits %g is not finite", who, *peak); return -1; }
    if (*ref_white == 0.0) *ref_white = 203.0;
    if (*peak == 0.0) *peak = 1000.0;
    if (*ref_white < 50.0 || *ref_white > 1000.0) { snprintf(err, nerr, "%s: ref_white_nits %g (50 .. 1000, or 0 for 203)", who, *ref_white); return -1; }
    if (*peak < *ref_white || *peak > 10000.0) { snprintf(err, nerr, "%s: peak_nits %g (the reference white %g .. 10000, or 0 for 1000)", who, *peak, *ref_white); return -1; }
    return 0;
}
/* tables = TM_TABLE_FLOATS floats: eotf, scale, thresh (the parameters have passed tonemap_params) */
static void tonemap_tables(int curve, double peak, double ref_white, int ycc[8], float *tables)
{
    const double p = peak/ref_white;
    ycc[0] = TM_KY; ycc[1] = TM_CRV; ycc[2] = TM_CGU; ycc[3] = TM_CGV; ycc[4] = TM_CBU; ycc[5] = TM_YOFF; ycc[6] = TM_COFF; ycc[7] = TM_SHIFT;
    for (int c = 0; c < 1024; c++)
    {
        const double x = 10000.0*tm_pq_eotf(c/1023.0)/ref_white;
        tables[TM_EOTF + c] = (float)x;
        tables[TM_SCALE + c] = x > 0.0 ? (float)(tm_curve(curve, x < p ? x : p, p)/x) : 1.0f;
    }
    tables[TM_THRESH] = 0.0f;
    for (int k = 1; k < 256; k++)
    {
        const double e = (k - 0.5)/255.0;
        tables[TM_THRESH + k] = (float)(e < 4.5*0.018 ? e/4.5 : pow((e + 0.099)/1.099, 1.0/0.45));
    }
}

#endif
