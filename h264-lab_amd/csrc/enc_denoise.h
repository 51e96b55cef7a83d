/*
 * enc_denoise.h -- the temporal denoiser (reference h264-lab.h:1547-1621 h264e_denoise_run), per sample group.
 *
 * Applied to each plane independently, out of place: `cur` is the raw input, `prev` the previous denoised picture (the encoder's
 * state, all zeros after H264E_set_denoise / H264E_clip_set_denoise), `out` the new denoised picture -- which becomes both the
 * picture that is encoded and the next frame's `prev`.  Every `prev` sample is the old state (the reference's in-place, row-lagged
 * loop is a storage trick only).
 *   - first / last row and column: out = cur;
 *   - interior: d = |cur - prev|, n = |sum over the 4 neighbours of (cur - prev)| >> 2 (signed sum, absolute value after summing),
 *     gd = 255 - T[d], gn = 255 - min(255, T[n] << 2), g = gn * gd, out = (prev * g + (65535 - g) * cur + 32768) >> 16  (<= 255);
 *   - a plane with w <= 2 or h <= 2 is left unchanged: out = prev.
 * T = k_denoise_gain (tables.h).  One lane handles four consecutive samples of a row (denoise_group); h264e_kernels.hip runs it as
 * h264e_denoise_kernel, h264e_pool.h's emulation launch (H264E_EMU) as a lane loop.
 */
#ifndef H264E_ENC_DENOISE_H
#define H264E_ENC_DENOISE_H
#include "wave.h"
#include "tables.h"

/* one interior sample: c = raw, p = previous denoised, nsum = signed sum of (raw - previous) over the four neighbours */
DEV uint32_t denoise_px(const LDS_AS uint8_t *T, int c, int p, int nsum)
{
    const int d = c > p ? c - p : p - c;
    const int n = (nsum < 0 ? -nsum : nsum) >> 2;                  /* <= 1020 >> 2 = 255 */
    const uint32_t gd = 255u - T[d];
    uint32_t tn = (uint32_t)T[n] << 2;
    if (tn > 255u) tn = 255u;
    const uint32_t g = (255u - tn)*gd;                             /* Q16 */
    return ((uint32_t)p*g + (65535u - g)*(uint32_t)c + 32768u) >> 16;
}

DEV int dn_byte(uint32_t v, int k) { return (int)((v >> (8*k)) & 255u); }

/* four samples x0 .. x0 + 3 of row y (1 <= y <= h - 2, x0 + 3 < w): the rows above / at / below as dwords (cu/pu, cc/pc, cd/pd: raw /
 * previous), the left and right neighbours of the group as single samples (ignored where the group touches the first / last column) */
DEV uint32_t denoise_quad(const LDS_AS uint8_t *T, uint32_t cu, uint32_t pu, uint32_t cc, uint32_t pc, uint32_t cd, uint32_t pd,
                          int cl, int pl, int cr, int pr, int x0, int w)
{
    int dr[6];
    dr[0] = cl - pl;
    for (int k = 0; k < 4; k++) dr[k + 1] = dn_byte(cc, k) - dn_byte(pc, k);
    dr[5] = cr - pr;
    uint32_t o = 0;
    for (int k = 0; k < 4; k++)
    {
        const int c = dn_byte(cc, k), x = x0 + k;
        const int nsum = dr[k] + dr[k + 2] + (dn_byte(cu, k) - dn_byte(pu, k)) + (dn_byte(cd, k) - dn_byte(pd, k));
        /* the value is <= 255 by construction: no clamp.  The opaque barrier keeps hipcc from folding shift + pack into
         * v_ashr_pk_u8_i32 (tests/test_isa_tripwire.py) */
        const uint32_t v = (x == 0 || x == w - 1) ? (uint32_t)c : (uint32_t)opaque_int((int)denoise_px(T, c, dn_byte(pc, k), nsum));
        o |= v << (8*k);
    }
    return o;
}

/* Group g of row y of one plane (w x h samples, rows packed: stride = w): samples 4g .. min(4g + 3, w - 1).  `aligned`: the three
 * plane pointers and w are multiples of 4, so rows load and store as dwords; otherwise sample by sample (e.g. 202-wide pictures:
 * 101-byte chroma rows). */
DEV void denoise_group(const LDS_AS uint8_t *T, const GLOBAL_AS uint8_t *cur, const GLOBAL_AS uint8_t *prev, GLOBAL_AS uint8_t *out,
                       int w, int h, int g, int y, int aligned)
{
    const int x0 = 4*g;
    if (x0 >= w || y >= h) return;
    const size_t r = (size_t)y*(size_t)w;
    const int n = w - x0 < 4 ? w - x0 : 4;
    if (w <= 2 || h <= 2 || y == 0 || y == h - 1)
    {
        /* degenerate plane: the state stays (out = prev); first / last row: out = cur */
        const GLOBAL_AS uint8_t *src = (w <= 2 || h <= 2) ? prev : cur;
        if (aligned) *(GLOBAL_AS uint32_t *)(out + r + x0) = *(const GLOBAL_AS uint32_t *)(src + r + x0);
        else for (int k = 0; k < n; k++) out[r + x0 + k] = src[r + x0 + k];
        return;
    }
    const int cl = x0 > 0 ? cur[r + x0 - 1] : 0, pl = x0 > 0 ? prev[r + x0 - 1] : 0;
    const int cr = x0 + 4 < w ? cur[r + x0 + 4] : 0, pr = x0 + 4 < w ? prev[r + x0 + 4] : 0;
    if (aligned)
    {
        const GLOBAL_AS uint32_t *c4 = (const GLOBAL_AS uint32_t *)(cur + r + x0), *p4 = (const GLOBAL_AS uint32_t *)(prev + r + x0);
        const int s = w >> 2;
        *(GLOBAL_AS uint32_t *)(out + r + x0) = denoise_quad(T, c4[-s], p4[-s], c4[0], p4[0], c4[s], p4[s], cl, pl, cr, pr, x0, w);
        return;
    }
    uint32_t cu = 0, pu = 0, cc = 0, pc = 0, cd = 0, pd = 0;
    for (int k = 0; k < n; k++)
    {
        const size_t i = r + (size_t)(x0 + k);
        cu |= (uint32_t)cur[i - w] << (8*k); pu |= (uint32_t)prev[i - w] << (8*k);
        cc |= (uint32_t)cur[i] << (8*k);     pc |= (uint32_t)prev[i] << (8*k);
        cd |= (uint32_t)cur[i + w] << (8*k); pd |= (uint32_t)prev[i + w] << (8*k);
    }
    const uint32_t o = denoise_quad(T, cu, pu, cc, pc, cd, pd, cl, pl, cr, pr, x0, w);
    for (int k = 0; k < n; k++) out[r + x0 + k] = (uint8_t)(o >> (8*k));
}

#endif
