/*
 * h264e_host.c -- C host side of the MI355X encoder: the reference's public API (include/h264e_mi355x.h)
 * over the HIP C ABI (include/h264e_hip.h).
 *
 * What stays on the host, as in the reference: frame-type / GOP bookkeeping (h264-lab.h:6725-6811), SPS / PPS /
 * slice header syntax (h264-lab.h:4040-4333), NAL framing with emulation prevention (h264-lab.h:3926-4022),
 * frame-level rate control (h264-lab.h:5924-6141) and the quantizer tables (h264-lab.h:5839-5912).
 * What runs on the GPU: the whole macroblock loop (encode_slice -> mb_encode) and the slice splice.
 *
 * mv_clusters (h264-lab.h:766) is the one raster-serial state the GPU cannot carry: macroblocks are encoded
 * with a SPECULATED value and the host validates it afterwards: exact trajectory from the
 * per-macroblock records, comparison of the rounded start candidates actually consumed, re-encode of the frame
 * with the exact per-macroblock values when they differ.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <sched.h>
#include <pthread.h>
#include "../../include/h264e_mi355x.h"
#include "../../include/h264e_hip.h"

#define MAGIC 0x4D493335u   /* "MI35" */
#define SLICE_P 0
#define SLICE_I 2

static int g_device = -1;
static __thread char g_host_err[256];       /* per calling thread: encoders on different threads do not share error text */

static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }

const char *H264E_last_error(void) { return g_host_err[0] ? g_host_err : h264e_hip_last_error(); }
void H264E_set_device(int device) { g_device = device; }
int H264E_device_count(void) { return h264e_hip_device_count(); }

static int pick_device(void)
{
    const char *e;
    if (g_device >= 0) return g_device;
    e = getenv("H264E_DEVICE");
    return e ? atoi(e) : 0;
}

/* ------------------------------------------------------------------ tables needed on the host */

/* per-QP rounding / dead-zone constants of the reference (h264-lab.h:993-1030, 1083-1094) */
static const uint16_t k_rnd_inter[52] = {
    11665, 11665, 11665, 11665, 11665, 11665, 11665, 11665, 11665, 11665, 11665, 12868, 14071, 15273, 16476, 17679, 17740, 17801,
    17863, 17924, 17985, 17445, 16904, 16364, 15823, 15283, 15198, 15113, 15027, 14942, 14857, 15667, 16478, 17288, 18099, 18909,
    19213, 19517, 19822, 20126, 20430, 16344, 12259, 8173, 4088, 4088, 4088, 4088, 4088, 4088, 4088, 4088 };
static const uint16_t k_thr_inter[52] = {
    31878, 31878, 31878, 31878, 31878, 31878, 31878, 31878, 31878, 31878, 31878, 33578, 35278, 36978, 38678, 40378, 41471, 42563,
    43656, 44748, 45841, 46432, 47024, 47615, 48207, 48798, 49354, 49911, 50467, 51024, 51580, 51580, 51580, 51580, 51580, 51580,
    52222, 52864, 53506, 54148, 54790, 45955, 37120, 28286, 19451, 10616, 9326, 8036, 6745, 5455, 4165, 4165 };
static const uint16_t k_thr_inter2[52] = {
    45352, 45352, 45352, 45352, 45352, 45352, 45352, 45352, 45352, 45352, 45352, 41100, 36848, 32597, 28345, 24093, 25904, 27715,
    29525, 31336, 33147, 33429, 33711, 33994, 34276, 34558, 32902, 31246, 29590, 27934, 26278, 26989, 27700, 28412, 29123, 29834,
    29038, 28242, 27445, 26649, 25853, 23440, 21028, 18615, 16203, 13790, 11137, 8484, 5832, 3179, 526, 526 };
static const uint16_t k_deadzonei[52] = {
    3419, 3419, 3419, 3419, 3419, 3419, 3419, 3419, 3419, 3419, 30550, 8845, 14271, 19698, 25124, 30550, 29556, 28562, 27569, 26575,
    25581, 25284, 24988, 24691, 24395, 24098, 24116, 24134, 24153, 24171, 24189, 24010, 23832, 23653, 23475, 23296, 23569, 23842,
    24115, 24388, 24661, 19729, 14797, 9865, 4933, 24661, 3499, 6997, 10495, 13993, 17491, 17491 };
static const uint8_t k_qpc[52] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29, 30, 31, 32, 32,
    33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39 };
/* rate-control model: bits per macroblock at QP 10..50 for P / I frames (h264-lab.h:933-938) */
static const uint16_t k_bits_per_mb[2][41] = {
    { 664, 597, 530, 484, 432, 384, 341, 297, 262, 235, 198, 173, 153, 131, 114, 102, 84, 74, 64, 54, 47, 42, 35, 31, 26, 22, 20, 17,
      15, 13, 12, 10, 9, 9, 7, 7, 6, 5, 4, 1, 1 },
    { 1057, 975, 925, 868, 803, 740, 694, 630, 586, 547, 496, 457, 420, 378, 345, 318, 284, 258, 234, 210, 190, 178, 155, 141, 129,
      115, 102, 95, 82, 75, 69, 60, 55, 51, 45, 41, 40, 35, 31, 28, 24 } };

/* h264-lab.h:5822-5834 */
static uint16_t rnd2thr(int round, int q)
{
    int b, thr = 0;
    for (b = 0x8000; b; b >>= 1)
        if ((thr | b)*q <= 0x10000 - round) thr |= b;
    return (uint16_t)thr;
}

/* h264-lab.h:5839-5912 rc_set_qp: quantizer tables for luma [0] and chroma [1] */
static void build_qdat(uint16_t qdat[2][42], int qp, int p_slice)
{
    static const int16_t qc[6][6] = {
        { 13107, 10, 8066, 13, 5243, 16 }, { 11916, 11, 7490, 14, 4660, 18 }, { 10082, 13, 6554, 16, 4194, 20 },
        {  9362, 14, 5825, 18, 3647, 23 }, {  8192, 16, 5243, 20, 3355, 25 }, {  7282, 18, 4559, 23, 2893, 29 } };
    int c, i, k;
    for (c = 0; c < 2; c++)
    {
        uint16_t *d = qdat[c];
        int div6 = qp*86 >> 9, mod6 = qp - div6*6;
        for (i = 0; i < 3; i++)
        {
            d[2*i]     = (uint16_t)(qc[mod6][2*i] << 1 >> div6);
            d[2*i + 1] = (uint16_t)(qc[mod6][2*i + 1] << div6);
        }
        d[6] = p_slice ? k_rnd_inter[qp] : k_deadzonei[qp];
        d[7] = k_deadzonei[qp];
        d[8] = (uint16_t)(k_thr_inter[qp] - 0x7fff);
        d[9] = (uint16_t)(k_thr_inter2[qp] - 0x7fff);
        for (k = 0; k < 2; k++)
        {
            uint16_t *t = d + 10 + 8*k;
            int r = (k ? k_thr_inter2[qp] : k_thr_inter[qp]) - 0x7fff;
            t[0] = t[2] = rnd2thr(r, d[0]);
            t[1] = t[3] = t[4] = t[6] = rnd2thr(r, d[2]);
            t[5] = t[7] = rnd2thr(r, d[4]);
        }
        for (k = 0; k < 2; k++)
        {
            uint16_t *t = d + 26 + 8*k;
            t[0] = t[2] = d[k]; t[1] = t[3] = t[4] = t[6] = d[2 + k]; t[5] = t[7] = d[4 + k];
        }
        qp = k_qpc[qp];
    }
}

/* ------------------------------------------------------------------ header bits / NAL */

typedef struct { uint64_t acc; int n; uint8_t *buf; size_t pos; } hbits_t;     /* small MSB-first writer */

static void hb_put(hbits_t *b, int n, uint32_t v)
{
    b->acc = (b->acc << n) | v;
    b->n += n;
    while (b->buf && b->n >= 8)
    {
        b->n -= 8;
        b->buf[b->pos++] = (uint8_t)(b->acc >> b->n);
    }
}
static void hb_ue(hbits_t *b, uint32_t v)
{
    int size = 0;
    uint32_t t = v + 1;
    do size++; while (t >>= 1);
    hb_put(b, 2*size - 1, v + 1);
}
static void hb_se(hbits_t *b, int v) { hb_ue(b, (uint32_t)(v > 0 ? 2*v - 1 : -2*v)); }

/* h264-lab.h:3926-4022: 4-byte start code + payload with emulation prevention; returns bytes written */
static size_t nal_emit(uint8_t *d, const uint8_t *p, size_t n)
{
    size_t i, j = 4;
    int zeros = 0;
    d[0] = d[1] = d[2] = 0; d[3] = 1;
    for (i = 0; i < n; i++)
    {
        if (zeros == 2 && p[i] <= 3) { d[j++] = 3; zeros = 0; }
        zeros = p[i] ? 0 : zeros + 1;
        d[j++] = p[i];
    }
    return j;
}

typedef struct
{
    int width, height, nmbx, nmby, nmb, w, h, cropping;
    int vbv_size_bytes, sps_id;
    /* what the SPS says about the samples (H264E_set_color / _set_frame_rate): all zero = no VUI at all.  seq_init leaves them alone */
    int matrix, full_range, fps_num, fps_den;
} seq_t;

static void seq_init(seq_t *s, int width, int height, int vbv, int sps_id)
{
    s->width = width; s->height = height;
    s->nmbx = (width + 15) >> 4; s->nmby = (height + 15) >> 4; s->nmb = s->nmbx*s->nmby;
    s->w = s->nmbx*16; s->h = s->nmby*16;
    s->cropping = !!((width | height) & 15);
    s->vbv_size_bytes = vbv; s->sps_id = sps_id;
}

/* h264-lab.h:4040-4141 encode_sps (profile 66) + h264-lab.h:4147-4176 encode_pps; returns bytes appended to d */
typedef void (*nalu_cb_t)(const unsigned char *nalu_data, int sizeof_nalu_data, void *token);

/* cb (optional): the reference's nal_end() hands EVERY finished NAL -- parameter sets included -- to run_param.nalu_callback,
 * pointer behind the start code, escaped length (h264-lab.h:4014-4018) */
static size_t write_sps_pps(const seq_t *s, int pic_init_qp, uint8_t *d, nalu_cb_t cb, void *token)
{
    static const struct { uint8_t level; uint16_t max_fs, max_vbvdiv5; uint32_t max_dpb; } lim[] = {
        { 10, 99, 175/5, 396 }, { 10, 99, 350/5, 396 }, { 11, 396, 500/5, 900 }, { 12, 396, 1000/5, 2376 },
        { 13, 396, 2000/5, 2376 }, { 20, 396, 2000/5, 2376 }, { 21, 792, 4000/5, 4752 }, { 22, 1620, 4000/5, 8100 },
        { 30, 1620, 10000/5, 8100 }, { 31, 3600, 14000/5, 18000 }, { 32, 5120, 20000/5, 20480 }, { 40, 8192, 25000/5, 32768 },
        { 41, 8192, 62500/5, 32768 }, { 42, 8704, 62500/5, 34816 }, { 50, 22080, 135000/5, 110400 }, { 51, 36864, 240000/5, 184320 } };
    uint8_t tmp[64];                                /* the SPS: at most 13 bytes + 13 of VUI */
    hbits_t b;
    size_t n = 0;
    int k = 0;
    const int vui = s->matrix || s->fps_num;
    while (lim[k].level < 51 && (s->nmb > lim[k].max_fs || s->vbv_size_bytes > lim[k].max_vbvdiv5*(5*1000/8) ||
                                 (unsigned)s->nmb > lim[k].max_dpb)) k++;
    memset(&b, 0, sizeof(b)); b.buf = tmp;
    hb_put(&b, 8, 0x67); hb_put(&b, 8, 66); hb_put(&b, 8, 0); hb_put(&b, 8, lim[k].level);
    hb_ue(&b, (uint32_t)s->sps_id);
    hb_ue(&b, 1);                                   /* log2_max_frame_num_minus4 */
    hb_ue(&b, 2);                                   /* pic_order_cnt_type */
    hb_ue(&b, 1);                                   /* num_ref_frames */
    hb_put(&b, 1, 0);
    hb_ue(&b, (uint32_t)(s->nmbx - 1));
    hb_ue(&b, (uint32_t)(s->nmby - 1));
    hb_put(&b, 3, (uint32_t)(6 + s->cropping));
    if (s->cropping)
    {
        hb_ue(&b, 0); hb_ue(&b, (uint32_t)((s->w - s->width) >> 1));
        hb_ue(&b, 0); hb_ue(&b, (uint32_t)((s->h - s->height) >> 1));
    }
    hb_put(&b, 1, (uint32_t)vui);                   /* vui_parameters_present_flag */
    if (vui)
    {
        /* E.1.1 in order: no aspect ratio, no overscan, the signal type with a colour description, no chroma location, the timing
         * (a frame is two ticks: time_scale = 2 fps), no HRD, no pic_struct, no bitstream restriction */
        hb_put(&b, 2, 0);
        hb_put(&b, 1, (uint32_t)(s->matrix != 0));
        if (s->matrix)
        {
            hb_put(&b, 3, 5); hb_put(&b, 1, (uint32_t)s->full_range); hb_put(&b, 1, 1);
            hb_put(&b, 8, (uint32_t)s->matrix); hb_put(&b, 8, (uint32_t)s->matrix); hb_put(&b, 8, (uint32_t)s->matrix);
        }
        hb_put(&b, 1, 0);
        hb_put(&b, 1, (uint32_t)(s->fps_num != 0));
        if (s->fps_num)
        {
            hb_put(&b, 32, (uint32_t)s->fps_den); hb_put(&b, 32, 2u*(uint32_t)s->fps_num);
            hb_put(&b, 1, 1);
        }
        hb_put(&b, 4, 0);
    }
    hb_put(&b, 1, 1);
    if (b.n) hb_put(&b, 8 - b.n, 0);
    n += nal_emit(d + n, tmp, b.pos);
    if (cb) cb(d + 4, (int)(n - 4), token);

    memset(&b, 0, sizeof(b)); b.buf = tmp;
    hb_put(&b, 8, 0x68);
    hb_ue(&b, (uint32_t)(s->sps_id*4)); hb_ue(&b, (uint32_t)s->sps_id);
    hb_put(&b, 1, 0); hb_put(&b, 1, 0);
    hb_ue(&b, 0); hb_ue(&b, 0); hb_ue(&b, 0);
    hb_put(&b, 1, 0); hb_put(&b, 2, 0);
    hb_se(&b, pic_init_qp - 26);
    hb_put(&b, 5, 0x1C);
    hb_put(&b, 1, 1);
    if (b.n) hb_put(&b, 8 - b.n, 0);
    {
        const size_t n0 = n;
        n += nal_emit(d + n, tmp, b.pos);
        if (cb) cb(d + n0 + 4, (int)(n - n0 - 4), token);
    }
    return n;
}

/* h264-lab.h:4182-4333 encode_slice_header for KEY / P frames as a template: the NAL header byte, then (written by the
 * kernel for every slice) ue(first_mb_in_slice), then the tail returned here.  nslices > 1: the row-band build's
 * disable_deblocking_filter_idc = 2 (h264-lab.h:4315-4323) */
static void slice_header_bits(const seq_t *s, int key, int frame_num, int idr_pic_id, int qp, int pic_init_qp, int no_deblock, int nslices,
                              int *nal, uint64_t *bits, int *nbits)
{
    hbits_t b;
    const int idc = nslices > 1 ? (no_deblock ? 1 : 2) : no_deblock;
    memset(&b, 0, sizeof(b));
    *nal = key ? 0x65 : 0x61;
    hb_ue(&b, key ? SLICE_I : SLICE_P);
    hb_ue(&b, (uint32_t)(s->sps_id*4));
    hb_put(&b, 5, (uint32_t)(frame_num & 31));
    if (key) hb_ue(&b, (uint32_t)idr_pic_id);
    if (!key) hb_put(&b, 2, 0);
    if (key) hb_put(&b, 2, 0); else hb_put(&b, 1, 0);
    hb_se(&b, qp - pic_init_qp);
    hb_ue(&b, (uint32_t)idc);
    if (no_deblock != 1) hb_put(&b, 2, 3);
    *bits = b.acc;
    *nbits = b.n;
}

/* the slices of one frame as the kernel exports them (h264e_hip_result_t): complete NALs -- start code + payload with the
 * emulation-prevention bytes already inserted on the device (enc_finalize.h nal_escape_copy) -- behind each other at 16-byte
 * aligned offsets; they are concatenated in order (h264-lab.h:6565-6569), cb as in nal_end.  Returns bytes written, 0 when
 * cap is too small */
static size_t emit_slices(uint8_t *d, size_t cap, const uint8_t *nals, const h264e_hip_result_t *r, nalu_cb_t cb, void *token)
{
    size_t pos = 0, off = 0;
    int k;
    for (k = 0; k < r->nslices; k++)
    {
        const size_t n = r->slice_nbytes[k];
        if (n < 5 || pos + n > cap) return 0;
        memcpy(d + pos, nals + off, n);
        if (cb) cb(d + pos + 4, (int)(n - 4), token);
        pos += n;
        off += (n + 15) & ~(size_t)15;
    }
    return pos;
}

/* where a finished frame's NALs are: in the slot's host-mapped mirror, or -- larger than the mirror, which is sized for ordinary
 * frames -- copied from the slot's device NAL arena into buf.  NULL when buf cannot hold them or the copy fails */
static const uint8_t *frame_nals(h264e_hip_pool_t *pool, int slot, const h264e_hip_result_t *r, uint8_t *buf, size_t buf_cap)
{
    if (!r->in_device) return h264e_hip_stream_rbsp(pool, slot);
    if (!buf || r->nbytes > buf_cap || h264e_hip_stream_fetch_nals(pool, slot, buf, r->nbytes)) return NULL;
    return buf;
}

/* ------------------------------------------------------------------ mv_clusters validation */

static int mvx(int32_t v) { return (int16_t)(v & 0xffff); }
static int mvy(int32_t v) { return (int16_t)((uint32_t)v >> 16); }
static int32_t mvmk(int x, int y) { return (int32_t)(((uint32_t)y << 16) | ((uint32_t)x & 0xffff)); }
static int32_t mvround(int32_t a) { return mvmk((mvx(a) + 1) & ~3, (mvy(a) + 1) & ~3); }

/* h264-lab.h:5263-5278 mv_clusters_update */
static void clusters_step(int32_t c[2], int32_t mv)
{
    int n = mvx(mv)*mvx(mv) + mvy(mv)*mvy(mv);
    int n0 = mvx(c[0])*mvx(c[0]) + mvy(c[0])*mvy(c[0]), n1 = mvx(c[1])*mvx(c[1]) + mvy(c[1])*mvy(c[1]);
    if (n < n1) c[0] = mvmk((63*mvx(c[0]) + mvx(mv) + 32) >> 6, (63*mvy(c[0]) + mvy(mv) + 32) >> 6);
    if (n >= n0) c[1] = mvmk((63*mvx(c[1]) + mvx(mv) + 32) >> 6, (63*mvy(c[1]) + mvy(mv) + 32) >> 6);
}

/*
 * Walk one frame's macroblock records from state `c` (updated in place).  `used` is what the kernel was
 * given: one pair for the whole frame (per_mb = 0) or one pair per macroblock.  traj (optional, [nmb][2])
 * receives the exact value in front of every macroblock.  Returns the first macroblock whose consumed,
 * rounded candidates differ from the exact ones, or -1.
 * nslices > 1 (row bands): every band is encoded by a copy of the encoder that is thrown away (h264-lab.h:6526), so the
 * walk restarts from the frame's start state at every band and `c` comes back unchanged.
 */
static int clusters_walk(int32_t c[2], const h264e_hip_mbrec_t *rec, int nmbx, int nmby, int nslices, const int32_t *used, int per_mb, int32_t *traj)
{
    const int32_t c0[2] = { c[0], c[1] };
    int band, row0 = 0, first_bad = -1;
    if (nslices < 1) nslices = 1;
    for (band = 0; band < nslices; band++)
    {
        const int row1 = row0 + (nmby - row0)/(nslices - band);
        int i;
        c[0] = c0[0]; c[1] = c0[1];
        for (i = row0*nmbx; i < row1*nmbx; i++)
        {
            const int32_t *u = per_mb ? used + 2*i : used;
            if (traj) { traj[2*i] = c[0]; traj[2*i + 1] = c[1]; }
            if (rec[i].used_cand && first_bad < 0 && (mvround(u[0]) != mvround(c[0]) || mvround(u[1]) != mvround(c[1]))) first_bad = i;
            if (rec[i].type < 5) clusters_step(c, rec[i].mv0);
        }
        row0 = row1;
    }
    if (nslices > 1) { c[0] = c0[0]; c[1] = c0[1]; }
    return first_bad;
}

/* test hook: clusters_walk itself (tests/test_finalizer.py compares it with the device's walks and the plain model) */
int h264e_hip_selftest_host_clusters_walk(int32_t state[2], const h264e_hip_mbrec_t *rec, int nmbx, int nmby, int nslices, const int32_t *used, int per_mb, int32_t *traj)
{
    return clusters_walk(state, rec, nmbx, nmby, nslices, used, per_mb, traj);
}

/* ------------------------------------------------------------------ rate control (frame level) */

typedef struct { int qp, prev_qp, vbv_bits, qp_smooth, dqp_smooth, max_dqp, bit_budget, vbv_target_level; } rc_t;

static uint32_t mul32x32shr16(uint32_t x, uint32_t y)               /* h264-lab.h:3420 */
{
    return (x >> 16)*(y & 0xFFFFu) + x*(y >> 16) + ((y & 0xFFFFu)*(x & 0xFFFFu) >> 16);
}
static uint32_t div_q16(uint32_t numer, uint32_t denum)             /* h264-lab.h:3430 */
{
    unsigned f = 1u << __builtin_clz(denum);
    do
    {
        denum = denum*f >> 16;
        numer = mul32x32shr16(numer, f);
        f = ((1 << 17) - denum);
    } while (denum != 0xffff);
    return numer;
}

/* h264-lab.h:5924-6070 rc_frame_start without long-term references; returns the frame QP */
static int rc_frame_start(rc_t *rc, int gop, int nmb, int vbv_size_bytes, int desired_frame_bytes, int qp_min, int qp_max, int is_intra)
{
    unsigned np = (unsigned)(gop - 1u) < 63u ? (unsigned)(gop - 1u) : 63u;
    int qp = -1, add_bits, bit_budget = desired_frame_bytes*8, nominal_p, gop_bits, stationary;
    uint32_t peak_q16;
    do
    {
        qp++;
        gop_bits = (int)(k_bits_per_mb[0][qp]*np + k_bits_per_mb[1][qp]);
    } while (gop_bits*nmb > (int)(np + 1)*desired_frame_bytes*8 && qp < 40);
    peak_q16 = div_q16((uint32_t)k_bits_per_mb[1][qp] << 16, (uint32_t)k_bits_per_mb[0][qp] << 16);
    if (np)
    {
        uint32_t ratio = div_q16((np + 1) << 16, (np << 16) + peak_q16);
        nominal_p = (int)mul32x32shr16((uint32_t)(desired_frame_bytes*8), ratio);
    } else
        nominal_p = 0;
    stationary = imin(vbv_size_bytes*8 >> 4, desired_frame_bytes*8);
    if (is_intra)
        add_bits = (int)mul32x32shr16((uint32_t)nominal_p, peak_q16) - bit_budget;
    else
    {
        add_bits = nominal_p - bit_budget;
        if (vbv_size_bytes) add_bits += (rc->vbv_target_level - rc->vbv_bits) >> 4;
    }
    if (vbv_size_bytes) add_bits = imin(add_bits, (vbv_size_bytes*8*7 >> 3) - rc->vbv_bits);
    bit_budget += add_bits;
    bit_budget = imin(bit_budget, desired_frame_bytes*8*16);
    bit_budget = imax(bit_budget, desired_frame_bytes*8 >> 2);
    if (is_intra) rc->vbv_target_level = rc->vbv_bits + bit_budget - desired_frame_bytes*8;
    rc->vbv_target_level -= desired_frame_bytes*8 - nominal_p;
    rc->vbv_target_level = imax(rc->vbv_target_level, stationary);
    rc->bit_budget = bit_budget;
    {
        const uint16_t *bits = k_bits_per_mb[!!is_intra];
        for (qp = 0; qp < 42 - 1; qp++)
            if (bits[qp]*nmb < bit_budget) break;
    }
    qp += 10;
    qp += rc->dqp_smooth;
    if (rc->prev_qp > qp + 1) qp = (rc->prev_qp + qp + 1)/2;
    qp = imin(qp, qp_max); qp = imax(qp, qp_min); qp = imin(qp, 51);             /* h264-lab.h:5841-5843 */
    rc->qp = qp;
    rc->qp_smooth = qp << 8;
    rc->prev_qp = qp;
    return qp;
}

/* h264-lab.h:6075-6141 rc_frame_end (stuffing / empty-frame options are refused at init) */
static void rc_frame_end(rc_t *rc, int nmb, int vbv_size_bytes, int desired_frame_bytes, int out_bytes, int intra, int all_skipped)
{
    if (!all_skipped)
    {
        int qp;
        for (qp = 0; qp != 41 && k_bits_per_mb[intra][qp]*nmb > out_bytes*8 - 32; qp++) {}
        qp += 10;
        if ((rc->qp_smooth >> 8) - rc->dqp_smooth < qp - 1) rc->dqp_smooth--;
        else if ((rc->qp_smooth >> 8) - rc->dqp_smooth > qp + 1) rc->dqp_smooth++;
        if (intra) rc->max_dqp = rc->dqp_smooth;
        else rc->max_dqp = imax(rc->max_dqp, (rc->qp_smooth >> 8) - qp);
    }
    rc->vbv_bits += out_bytes*8 - desired_frame_bytes*8;
    if (vbv_size_bytes)
    {
        if (rc->vbv_bits < 0) rc->vbv_bits = 0;
        if (rc->vbv_bits > vbv_size_bytes*8) rc->vbv_bits = vbv_size_bytes*8;
    } else
        rc->vbv_bits = 0;
}

/* ------------------------------------------------------------------ one frame on one chain, validated */

/*
 * One frame on chain 0 (the frame-at-a-time path) with the mv_clusters speculation made exact.
 * state[] holds the state in front of the frame; the kernel uses it for every macroblock.  A frame that moves the
 * state is walked exactly; where a consumed rounded candidate differs, the frame is encoded again with the walked
 * per-macroblock values, until the walk is consistent -- every pass fixes at least the first offending macroblock,
 * so this terminates.  state[] is advanced to the state behind the frame.
 */
static int frame_exact(h264e_hip_pool_t *pool, h264e_hip_task_t *task, int nmbx, int nmby, int32_t state[2])
{
    const int nmb = nmbx*nmby;
    int32_t *arr = NULL, *traj = NULL;      /* per macroblock: what the last pass consumed (NULL: state[]) / what its walk found */
    int rc = -1, pass;
    task->mv_clusters_per_mb = NULL;
    task->mv_clusters[0] = state[0]; task->mv_clusters[1] = state[1];
    for (pass = 0;; pass++)
    {
        int32_t cc[2] = { state[0], state[1] };
        h264e_hip_result_t r1;
        const h264e_hip_mbrec_t *recs;
        if (pass > nmb + 2) { snprintf(g_host_err, sizeof(g_host_err), "mv_clusters re-encode does not converge"); goto done; }
        if (h264e_hip_submit(pool, task) || h264e_hip_sync(pool)) goto done;
        /* results come through host-mapped memory, written by the frame's finalizer workgroup (no device-to-host copies) */
        if (h264e_hip_stream_done(pool, 0, &r1) != 1) { snprintf(g_host_err, sizeof(g_host_err), "frame did not complete"); goto done; }
        if (r1.overflow) { snprintf(g_host_err, sizeof(g_host_err), "bit buffer overflow"); goto done; }
        if (!arr && !r1.clusters_moved) break;                                  /* fixed point: state unchanged */
        if (!traj) traj = (int32_t *)malloc(sizeof(int32_t)*2*(size_t)nmb);
        recs = h264e_hip_stream_mbrec(pool, 0);
        if (!traj || !recs) goto done;
        if (clusters_walk(cc, recs, nmbx, nmby, task->nslices, arr ? arr : state, arr != NULL, traj) < 0)
        {
            state[0] = cc[0]; state[1] = cc[1];
            break;
        }
        if (!arr) arr = (int32_t *)malloc(sizeof(int32_t)*2*(size_t)nmb);
        if (!arr) goto done;
        memcpy(arr, traj, sizeof(int32_t)*2*(size_t)nmb);
        task->mv_clusters_per_mb = arr;
        if (h264e_hip_rewind_frame(pool, 0)) goto done;
    }
    rc = 0;
done:
    if (rc) h264e_hip_release(pool);
    free(arr); free(traj);
    return rc;
}

/* ------------------------------------------------------------------ drop-in API */

typedef struct
{
    uint32_t magic, serial;
    int impl;                               /* index into g_impl: device resources live OUTSIDE the caller's blob */
    H264E_create_param_t param;
    H264E_run_param_t run_param;
    seq_t seq;
    int frame_num, next_idr_pic_id, pic_init_qp;
    int32_t clusters[2];
    rc_t rc;
    int slices;                             /* row-band slices per frame (H264E_set_slices), 0 / 1 = one */
    int frames_in;                          /* frames H264E_encode has taken since H264E_init */
    int denoise, den_started;               /* temporal denoiser on (H264E_set_denoise); its state has left zero */
    int parent_all_skipped;                 /* row bands: what the reference's parent encoder holds in mb.skip_run == nmb (encode_frame) */
    int have_recon;                         /* a frame has been encoded: the pool holds its reconstruction (H264E_read_recon_device) */
} henc_t;

/* The reference API has no destructor and callers simply free() the blob, so nothing that needs
 * releasing may be reachable only through it: pools and staging buffers sit in this registry, keyed by blob address.
 * The registry grows on demand and is guarded by one mutex (H264E_init / H264E_close / H264E_encode's lookup may run on
 * different threads for different encoders, like the reference's re-entrant instances).  An entry is reclaimed when
 * H264E_close is called, when the same blob is initialised again, or when a NEW blob overlaps its address range (the
 * caller freed the old blob and the allocator handed the memory out again: the old encoder cannot be alive). */
typedef struct { void *owner; size_t owner_bytes; uint32_t serial; h264e_hip_pool_t *pool; uint8_t *rbsp; size_t rbsp_cap; uint8_t *recon; } impl_t;
static impl_t *g_impl;
static int g_impl_cap;
static uint32_t g_serial;
static int g_atexit;
static pthread_mutex_t g_reg_lock = PTHREAD_MUTEX_INITIALIZER;

static void impl_release(impl_t *m)
{
    if (m->pool) h264e_hip_pool_destroy(m->pool);
    free(m->rbsp); free(m->recon);
    memset(m, 0, sizeof(*m));
}

static void release_all(void)
{
    int i;
    pthread_mutex_lock(&g_reg_lock);
    for (i = 0; i < g_impl_cap; i++) if (g_impl[i].owner) impl_release(g_impl + i);
    pthread_mutex_unlock(&g_reg_lock);
}

/* copy of the entry (the table may be reallocated by another thread's H264E_init): pointers inside stay valid as long as
 * this encoder is not closed concurrently, which the API forbids per instance as the reference does */
static int impl_of(const henc_t *e, impl_t *out)
{
    int ok = 0;
    if (!e || e->magic != MAGIC) return 0;
    pthread_mutex_lock(&g_reg_lock);
    if (e->impl >= 0 && e->impl < g_impl_cap && g_impl[e->impl].owner == (const void *)e && g_impl[e->impl].serial == e->serial)
    {
        *out = g_impl[e->impl];
        ok = 1;
    }
    pthread_mutex_unlock(&g_reg_lock);
    return ok;
}

/* with the lock held: release every entry whose persist blob [owner, owner + owner_bytes) OVERLAPS [p, p + n): the memory of an abandoned
 * encoder may begin below a new allocation and still reach into it */
static void reclaim_range(const void *p, size_t n)
{
    const char *lo = (const char *)p, *hi = lo + (n ? n : 1);
    int i;
    for (i = 0; i < g_impl_cap; i++)
        if (g_impl[i].owner)
        {
            const char *olo = (const char *)g_impl[i].owner, *ohi = olo + (g_impl[i].owner_bytes ? g_impl[i].owner_bytes : 1);
            if (olo < hi && lo < ohi) impl_release(g_impl + i);
        }
}

void H264E_close(H264E_persist_t *p)
{
    if (!p) return;
    pthread_mutex_lock(&g_reg_lock);
    reclaim_range(p, 1);
    pthread_mutex_unlock(&g_reg_lock);
}

/* h264-lab.h:6252-6286 enc_check_create_params (+ the options this implementation refuses) */
static int check_params(const H264E_create_param_t *par)
{
    if (!par) return H264E_STATUS_BAD_ARGUMENT;
    if ((int)(par->vbv_size_bytes | par->gop) < 0) return H264E_STATUS_BAD_PARAMETER;
    if (par->width <= 0 || par->height <= 0) return H264E_STATUS_BAD_PARAMETER;
    if ((unsigned)(par->const_input_flag | par->fine_rate_control_flag | par->vbv_overflow_empty_frame_flag | par->vbv_underflow_stuffing_flag) > 1)
        return H264E_STATUS_BAD_PARAMETER;
    if ((unsigned)par->max_long_term_reference_frames > 8) return H264E_STATUS_BAD_PARAMETER;
    if ((par->width | par->height) & 1) return H264E_STATUS_SIZE_NOT_MULTIPLE_2;
    if (((par->width | par->height) & 15) && !par->const_input_flag) return H264E_STATUS_SIZE_NOT_MULTIPLE_16;
    return H264E_STATUS_SUCCESS;
}

static int unsupported(const H264E_create_param_t *par)
{
    return par->max_long_term_reference_frames || par->temporal_denoise_flag || par->fine_rate_control_flag ||
           par->vbv_overflow_empty_frame_flag || par->vbv_underflow_stuffing_flag || par->num_layers > 1;
}

/* the reference's blob sizes (h264-lab.h:6191-6230 enc_alloc / enc_alloc_scratch with sizeof(h264e_enc_t) = 1184,
 * sizeof(scratch_t) = 2962 on LP64): encode_app prints them, and callers size their buffers with them */
static void ref_sizes(const H264E_create_param_t *par, int *persist, int *scratch)
{
    int nmbx = (par->width + 15) >> 4, nmby = (par->height + 15) >> 4, p = 1;
    int nref = 1 + par->max_long_term_reference_frames + par->const_input_flag + !!par->temporal_denoise_flag;
    static const int a16 = 15;
    *persist = (((16 + (nmbx + 2)*(nmby + 2)*384*nref) - 1 + 15) & ~15) + 1184;
#define ALLOC(sz) p = (p + a16) & ~a16; p += (sz)
    ALLOC(2962);
    ALLOC(nmbx*nmby*(384 + 2 + 10)*3/2);
    ALLOC(nmbx*8 + 8);
    ALLOC((nmbx*4 + 8)*4);
    ALLOC(nmbx*4 + 4);
    ALLOC(nmbx);
    ALLOC(nmbx);
    ALLOC(nmbx);
    ALLOC(nmbx*32 + 32 + 16);
#undef ALLOC
    *scratch = p - 1;
}

int H264E_sizeof(const H264E_create_param_t *par, int *sizeof_persist, int *sizeof_scratch)
{
    int err = check_params(par);
    if (!sizeof_persist || !sizeof_scratch) err = H264E_STATUS_BAD_ARGUMENT;
    if (err) return err;
    ref_sizes(par, sizeof_persist, sizeof_scratch);
    return H264E_STATUS_SUCCESS;
}

int H264E_init(H264E_persist_t *p, const H264E_create_param_t *par)
{
    henc_t *e = (henc_t *)p;
    impl_t fresh;
    int i, sp, ss, err = check_params(par);
    g_host_err[0] = 0;
    if (!e) return H264E_STATUS_BAD_ARGUMENT;
    if (err) return err;
    if (unsupported(par))
    {
        snprintf(g_host_err, sizeof(g_host_err), "option outside the MI355X encode path (long-term refs, denoise, MB-level RC, VBV stuffing/empty frames, SVC)");
        return H264E_STATUS_BAD_PARAMETER;
    }
    ref_sizes(par, &sp, &ss);
    /* whatever lived in this memory goes FIRST (re-init of the same blob, or of memory an abandoned encoder lived in): a re-init does not
     * need the device memory twice, and a failure below does not leave an entry registered for a blob that has been zeroed */
    pthread_mutex_lock(&g_reg_lock);
    reclaim_range(p, (size_t)sp);
    pthread_mutex_unlock(&g_reg_lock);
    memset(e, 0, sizeof(*e));
    e->param = *par;
    seq_init(&e->seq, par->width, par->height, par->vbv_size_bytes, par->sps_id);
    /* device resources are created outside the lock (slow), registered under it */
    memset(&fresh, 0, sizeof(fresh));
    if (h264e_hip_pool_create(&fresh.pool, pick_device(), par->width, par->height, 1, 1))
        return H264E_STATUS_BAD_ARGUMENT;       /* no device: the HIP path is the only path */
    fresh.rbsp_cap = (size_t)e->seq.nmb*660 + 8192;
    fresh.rbsp = (uint8_t *)malloc(fresh.rbsp_cap);
    if (!par->const_input_flag) fresh.recon = (uint8_t *)malloc((size_t)e->seq.w*e->seq.h*3/2);
    fresh.owner = e; fresh.owner_bytes = (size_t)sp;
    pthread_mutex_lock(&g_reg_lock);
    reclaim_range(p, (size_t)sp);               /* (another thread may have registered an overlapping blob meanwhile) */
    for (i = 0; i < g_impl_cap && g_impl[i].owner; i++) {}
    if (i == g_impl_cap)
    {
        const int ncap = g_impl_cap ? 2*g_impl_cap : 16;
        impl_t *t = (impl_t *)realloc(g_impl, sizeof(impl_t)*(size_t)ncap);
        if (!t)
        {
            pthread_mutex_unlock(&g_reg_lock);
            impl_release(&fresh);
            snprintf(g_host_err, sizeof(g_host_err), "out of host memory");
            return H264E_STATUS_BAD_ARGUMENT;
        }
        memset(t + g_impl_cap, 0, sizeof(impl_t)*(size_t)(ncap - g_impl_cap));
        g_impl = t; g_impl_cap = ncap;
    }
    fresh.serial = e->serial = ++g_serial;
    g_impl[i] = fresh;
    e->impl = i;
    e->magic = MAGIC;
    if (!g_atexit) { atexit(release_all); g_atexit = 1; }
    pthread_mutex_unlock(&g_reg_lock);
    return H264E_STATUS_SUCCESS;
}

int H264E_set_slices(H264E_persist_t *p, int nslices)
{
    henc_t *e = (henc_t *)p;
    if (!e || e->magic != MAGIC || nslices < 0 || nslices > H264E_HIP_MAX_SLICES) return H264E_STATUS_BAD_PARAMETER;
    e->slices = nslices;
    return H264E_STATUS_SUCCESS;
}

/* The reference's temporal denoiser (h264-lab.h:6684-6695, create parameter temporal_denoise_flag, which H264E_init keeps refusing):
 * before the first frame only; zeroes the state.  Frames with encode_speed < 2 are then denoised on the device and the denoised
 * picture is encoded; other frames are encoded raw and leave the state alone. */
int H264E_set_denoise(H264E_persist_t *p, int on)
{
    henc_t *e = (henc_t *)p;
    impl_t mm;
    g_host_err[0] = 0;
    if (!impl_of(e, &mm) || e->frames_in) return H264E_STATUS_BAD_PARAMETER;
    if (on && h264e_hip_denoise_reset(mm.pool)) return H264E_STATUS_BAD_ARGUMENT;
    e->denoise = !!on;
    e->den_started = 0;
    return H264E_STATUS_SUCCESS;
}

/* what both encoders refuse of a colour / a frame rate: the offending value goes into the error text, nothing is changed */
static int color_refused(const char *who, int matrix, int full_range)
{
    if (matrix != H264E_MATRIX_UNSPECIFIED && matrix != H264E_MATRIX_BT709 && matrix != H264E_MATRIX_BT601)
        snprintf(g_host_err, sizeof(g_host_err), "%s: matrix %d (0 = unspecified, 1 = BT.709, 6 = BT.601)", who, matrix);
    else if (full_range != 0 && full_range != 1) snprintf(g_host_err, sizeof(g_host_err), "%s: full_range %d (0 or 1)", who, full_range);
    else if (!matrix && full_range) snprintf(g_host_err, sizeof(g_host_err), "%s: full_range %d needs a matrix (1 or 6), not matrix 0", who, full_range);
    else return 0;
    return 1;
}
static int fps_refused(const char *who, int num, int den)
{
    if (!num && !den) return 0;
    if (num <= 0 || num > (1 << 30)) snprintf(g_host_err, sizeof(g_host_err), "%s: numerator %d (1..2^30, or 0/0 for none)", who, num);
    else if (den <= 0) snprintf(g_host_err, sizeof(g_host_err), "%s: denominator %d (1..2^31 - 1, or 0/0 for none)", who, den);
    else return 0;
    return 1;
}
static int color_apply(seq_t *s, h264e_hip_pool_t *pool, int matrix, int full_range)
{
    if (h264e_hip_set_color(pool, matrix == H264E_MATRIX_BT709, full_range)) return -1;
    s->matrix = matrix; s->full_range = full_range;
    return 0;
}

/* Colour of the stream: how RGB / RGBP device input is converted from now on, and what every SPS says.  Like
 * H264E_set_denoise only between H264E_init and the first frame: the SPS is repeated at every key frame and must not change. */
int H264E_set_color(H264E_persist_t *p, int matrix, int full_range)
{
    henc_t *e = (henc_t *)p;
    impl_t mm;
    g_host_err[0] = 0;
    if (!impl_of(e, &mm)) return H264E_STATUS_BAD_PARAMETER;
    if (e->frames_in) { snprintf(g_host_err, sizeof(g_host_err), "set_color: only before the first frame (%d encoded)", e->frames_in); return H264E_STATUS_BAD_PARAMETER; }
    if (color_refused("set_color", matrix, full_range)) return H264E_STATUS_BAD_PARAMETER;
    return color_apply(&e->seq, mm.pool, matrix, full_range) ? H264E_STATUS_BAD_ARGUMENT : H264E_STATUS_SUCCESS;
}

/* HDR10 device input (include/h264e_mi355x.h): the pool holds the setting, so both encoders' device frames go the same way.  The rule
 * and the statuses are H264E_set_color's; the refusals of the values are the device layer's (H264E_last_error -> its text) */
int H264E_set_tonemap(H264E_persist_t *p, int transfer, int curve, double peak_nits, double ref_white_nits)
{
    henc_t *e = (henc_t *)p;
    impl_t mm;
    g_host_err[0] = 0;
    if (!impl_of(e, &mm)) return H264E_STATUS_BAD_PARAMETER;
    if (e->frames_in) { snprintf(g_host_err, sizeof(g_host_err), "set_tonemap: only before the first frame (%d encoded)", e->frames_in); return H264E_STATUS_BAD_PARAMETER; }
    if (h264e_hip_tonemap_check("set_tonemap", transfer, curve, peak_nits, ref_white_nits)) return H264E_STATUS_BAD_PARAMETER;
    return h264e_hip_tonemap_set(mm.pool, "set_tonemap", transfer, curve, peak_nits, ref_white_nits) ? H264E_STATUS_BAD_ARGUMENT : H264E_STATUS_SUCCESS;
}

int H264E_tonemap_tables(int transfer, int curve, double peak_nits, double ref_white_nits, int ycc[8], float eotf[1024], float scale[1024], float thresh[256])
{
    g_host_err[0] = 0;
    return h264e_hip_tonemap_tables(transfer, curve, peak_nits, ref_white_nits, ycc, eotf, scale, thresh);
}

int H264E_tonemap_state(H264E_persist_t *p, long long state[3])
{
    impl_t mm;
    g_host_err[0] = 0;
    if (!impl_of((henc_t *)p, &mm)) return H264E_STATUS_BAD_PARAMETER;
    return h264e_hip_tonemap_state(mm.pool, state) ? H264E_STATUS_BAD_ARGUMENT : H264E_STATUS_SUCCESS;
}

int H264E_set_frame_rate(H264E_persist_t *p, int num, int den)
{
    henc_t *e = (henc_t *)p;
    impl_t mm;
    g_host_err[0] = 0;
    if (!impl_of(e, &mm)) return H264E_STATUS_BAD_PARAMETER;
    if (e->frames_in) { snprintf(g_host_err, sizeof(g_host_err), "set_frame_rate: only before the first frame (%d encoded)", e->frames_in); return H264E_STATUS_BAD_PARAMETER; }
    if (fps_refused("set_frame_rate", num, den)) return H264E_STATUS_BAD_PARAMETER;
    e->seq.fps_num = num; e->seq.fps_den = den;
    return H264E_STATUS_SUCCESS;
}

void H264E_set_vbv_state(H264E_persist_t *p, int vbv_size_bytes, int vbv_fullness_bytes)
{
    henc_t *e = (henc_t *)p;
    if (!e || e->magic != MAGIC) return;
    e->param.vbv_size_bytes = vbv_size_bytes;
    e->seq.vbv_size_bytes = vbv_size_bytes;
    if (vbv_fullness_bytes >= 0)
    {
        e->rc.vbv_bits = vbv_fullness_bytes*8;
        e->rc.vbv_target_level = e->rc.vbv_bits;
    }
}

/* the frame into the pool's input slot: from the caller's host planes, or from device memory (H264E_encode_device) */
static int put_frame(h264e_hip_pool_t *pool, const H264E_io_yuv_t *in, const H264E_dev_frame_t *dev, const H264E_dev_window_t *win)
{
    const uint8_t *yuv[3];
    if (dev && win) return h264e_hip_scale_device(pool, 0, dev->format, dev->plane, dev->stride, (const int *)win, dev->producer_stream);
    if (dev) return h264e_hip_ingest_device(pool, 0, dev->format, dev->plane, dev->stride, dev->pixel_bytes, dev->producer_stream);
    yuv[0] = in->yuv[0]; yuv[1] = in->yuv[1]; yuv[2] = in->yuv[2];
    return h264e_hip_upload_planes(pool, 0, yuv, in->stride);
}

/* H264E_encode (dev = NULL), H264E_encode_device (in = NULL) and H264E_encode_device_scaled (in = NULL, a window) */
static int encode_frame(H264E_persist_t *p, H264E_scratch_t *scratch, const H264E_run_param_t *opt, H264E_io_yuv_t *in, const H264E_dev_frame_t *dev,
                        const H264E_dev_window_t *win, unsigned char **coded_data, int *sizeof_coded_data)
{
    henc_t *e = (henc_t *)p;
    impl_t mm, *m = impl_of(e, &mm) ? &mm : NULL;
    uint8_t *out = (uint8_t *)scratch;
    size_t out_pos = 0, cap;
    int frame_type, key, qp, sp, ss, den;
    h264e_hip_task_t task;
    h264e_hip_result_t res;
    g_host_err[0] = 0;
    if (!m || !scratch || (!in && !dev) || !coded_data || !sizeof_coded_data) return H264E_STATUS_BAD_ARGUMENT;
    if (dev)
    {
        if (!e->param.const_input_flag)
        {
            snprintf(g_host_err, sizeof(g_host_err), "H264E_encode_device needs const_input_flag = 1: the reconstruction is not written back to device planes");
            return H264E_STATUS_BAD_PARAMETER;
        }
        /* refused before the stream state moves */
        if (win ? h264e_hip_scale_check(m->pool, 0, dev->format, dev->plane, dev->stride, (const int *)win)
                : h264e_hip_ingest_check(m->pool, 0, dev->format, dev->plane, dev->stride, dev->pixel_bytes)) return H264E_STATUS_BAD_ARGUMENT;
    }
    ref_sizes(&e->param, &sp, &ss);
    cap = (size_t)ss;
    /* frame types outside this encode path (I, DROPPABLE, GOLDEN, RECOVERY, CUSTOM) are refused before anything moves: the stored run
     * parameters included, so a later run_param == NULL repeats the last ACCEPTED call */
    frame_type = (opt ? opt : &e->run_param)->frame_type;
    if (frame_type != H264E_FRAME_TYPE_DEFAULT && frame_type != H264E_FRAME_TYPE_KEY && frame_type != H264E_FRAME_TYPE_P) return H264E_STATUS_BAD_FRAME_TYPE;
    if (opt) e->run_param = *opt;                                                         /* h264-lab.h:6701-6705 */
    opt = &e->run_param;
    if (!e->run_param.qp_max || e->run_param.qp_max > 51) e->run_param.qp_max = 51;       /* h264-lab.h:6707-6715 */
    if (!e->run_param.qp_min || e->run_param.qp_min < 10) e->run_param.qp_min = 10;
    if (opt->desired_nalu_bytes)
    {
        snprintf(g_host_err, sizeof(g_host_err), "desired_nalu_bytes (multi-slice) is outside the MI355X encode path");
        return H264E_STATUS_BAD_ARGUMENT;
    }

    frame_type = opt->frame_type;
    if (frame_type == H264E_FRAME_TYPE_DEFAULT) frame_type = e->frame_num ? H264E_FRAME_TYPE_P : H264E_FRAME_TYPE_KEY;
    key = frame_type == H264E_FRAME_TYPE_KEY;
    if (key)
    {
        e->pic_init_qp = imax(imin(30, e->run_param.qp_max), e->run_param.qp_min);       /* h264-lab.h:6768-6775 */
        e->next_idr_pic_id ^= 1;
        e->frame_num = 0;
        out_pos += write_sps_pps(&e->seq, e->pic_init_qp, out + out_pos, e->run_param.nalu_callback, e->run_param.nalu_callback_token);
    } else if (!e->pic_init_qp)
        return H264E_STATUS_BAD_FRAME_TYPE;                                              /* h264-lab.h:6801-6804 */

    qp = rc_frame_start(&e->rc, e->param.gop, e->seq.nmb, e->param.vbv_size_bytes, opt->desired_frame_bytes,
                        e->run_param.qp_min, e->run_param.qp_max, key);

    memset(&task, 0, sizeof(task));
    task.active = 1; task.frame_index = 0;
    task.slice_type = key ? SLICE_I : SLICE_P;
    task.qp = qp; task.speed = opt->encode_speed;
    task.nslices = e->slices > 1 ? imin(e->slices, e->seq.nmby) : 1;
    slice_header_bits(&e->seq, key, e->frame_num, e->next_idr_pic_id, qp, e->pic_init_qp,
                      (opt->encode_speed == 8 || opt->encode_speed == 10), task.nslices, &task.hdr_nal, &task.hdr_bits, &task.hdr_nbits);
    build_qdat(task.qdat, qp, !key);

    memset(&res, 0, sizeof(res));
    /* h264-lab.h:6684-6695: the denoiser runs first (also in front of a transparent VBV-overflow frame) and its output is what gets encoded */
    den = e->denoise && opt->encode_speed < 2;
    if (den)
    {
        if (put_frame(m->pool, in, dev, win) || h264e_hip_denoise_frames(m->pool, 0, 1, !e->den_started)) return H264E_STATUS_BAD_ARGUMENT;
        e->den_started = 1;
        task.denoised = 1;
    }
    e->frames_in++;
    if (e->param.vbv_size_bytes && !key && e->rc.vbv_bits - opt->desired_frame_bytes*8 > e->param.vbv_size_bytes*8)
    {
        /* h264-lab.h:6497-6510 "encode transparent frame on VBV overflow" -- reachable only right after H264E_set_vbv_state (rc_frame_end
         * clamps the fullness to the VBV size): one slice whose whole payload is a skip run over the picture, the reference picture as
         * the reconstruction.  P frames only: h264-lab.h:6497 asks for !long_term_idx_use, which is -1 on a key frame (:6738), so a key
         * frame is coded in full however far the VBV has overflowed.  Nothing for the device to do: the pool's reference / reconstruction pair is
         * simply not swapped, so the next frame predicts from the same picture; mv_clusters do not move (no macroblock was encoded). */
        uint8_t rb[32];
        hbits_t b;
        size_t w;
        memset(&b, 0, sizeof(b));
        b.buf = rb;
        hb_put(&b, 8, (uint32_t)task.hdr_nal);
        hb_ue(&b, 0);                                                   /* first_mb_in_slice */
        hb_put(&b, task.hdr_nbits > 32 ? task.hdr_nbits - 32 : 0, (uint32_t)(task.hdr_nbits > 32 ? task.hdr_bits >> 32 : 0));
        hb_put(&b, task.hdr_nbits > 32 ? 32 : task.hdr_nbits, (uint32_t)task.hdr_bits);
        hb_ue(&b, (uint32_t)e->seq.nmb);                                /* mb_skip_run = every macroblock */
        hb_put(&b, 1, 1);                                               /* rbsp_stop_one_bit */
        if (b.n) hb_put(&b, 8 - b.n, 0);
        if (out_pos + 2*b.pos + 8 > cap) { snprintf(g_host_err, sizeof(g_host_err), "coded frame does not fit the scratch blob"); return H264E_STATUS_BAD_ARGUMENT; }
        w = nal_emit(out + out_pos, rb, b.pos);
        if (opt->nalu_callback) opt->nalu_callback(out + out_pos + 4, (int)(w - 4), opt->nalu_callback_token);
        out_pos += w;
        res.all_skipped = 1;
        /* nothing is encoded, but the call's input still goes into the slot: H264E_read_quality compares it with the unchanged picture */
        if (!den && put_frame(m->pool, in, dev, win)) return H264E_STATUS_BAD_ARGUMENT;
    } else
    {
    if (!den && put_frame(m->pool, in, dev, win)) return H264E_STATUS_BAD_ARGUMENT;
    if (frame_exact(m->pool, &task, e->seq.nmbx, e->seq.nmby, e->clusters) || h264e_hip_stream_done(m->pool, 0, &res) != 1) return H264E_STATUS_BAD_ARGUMENT;
    {
        const uint8_t *nals = frame_nals(m->pool, 0, &res, m->rbsp, m->rbsp_cap);
        size_t w;
        if (!nals) return H264E_STATUS_BAD_ARGUMENT;
        w = emit_slices(out + out_pos, cap - out_pos, nals, &res, opt->nalu_callback, opt->nalu_callback_token);
        if (!w)
        {
            snprintf(g_host_err, sizeof(g_host_err), "coded frame does not fit the scratch blob");
            return H264E_STATUS_BAD_ARGUMENT;
        }
        out_pos += w;
    }
    }

    /* h264-lab.h:6596 reads the PARENT encoder's mb.skip_run.  One slice: this frame's.  Row bands are coded by copies of the encoder
     * (:6526-6560), so the parent keeps what it had: 0 at first, and nmb from a transparent frame on -- every later frame of a row-band
     * stream then ends like an all-skipped one */
    if (task.nslices == 1 || res.all_skipped) e->parent_all_skipped = res.all_skipped;
    rc_frame_end(&e->rc, e->seq.nmb, e->param.vbv_size_bytes, opt->desired_frame_bytes, (int)out_pos, key, e->parent_all_skipped);

    if (!e->param.const_input_flag && in)
    {
        /* h264-lab.h:6719-6723: the reconstruction replaces the caller's input picture (encode_app --psnr relies on it) */
        int c, y;
        const uint8_t *s = m->recon;
        if (h264e_hip_read_recon(m->pool, 0, m->recon)) return H264E_STATUS_BAD_ARGUMENT;
        for (c = 0; c < 3; c++)
        {
            int w = e->seq.w >> (c ? 1 : 0), h = e->seq.h >> (c ? 1 : 0);
            for (y = 0; y < h; y++) memcpy(in->yuv[c] + (size_t)y*in->stride[c], s + (size_t)y*w, (size_t)w);
            s += (size_t)w*h;
        }
    }
    if (++e->frame_num >= e->param.gop && e->param.gop && e->run_param.frame_type == H264E_FRAME_TYPE_DEFAULT) e->frame_num = 0;
    e->have_recon = 1;
    *coded_data = out;
    *sizeof_coded_data = (int)out_pos;
    return H264E_STATUS_SUCCESS;
}

int H264E_encode(H264E_persist_t *p, H264E_scratch_t *scratch, const H264E_run_param_t *opt, H264E_io_yuv_t *in,
                 unsigned char **coded_data, int *sizeof_coded_data)
{
    return encode_frame(p, scratch, opt, in, NULL, NULL, coded_data, sizeof_coded_data);
}

/* H264E_encode with the frame taken from device memory by the ingest kernel (enc_ingest.h) instead of a host-to-device copy */
int H264E_encode_device(H264E_persist_t *p, H264E_scratch_t *scratch, const H264E_run_param_t *opt, const H264E_dev_frame_t *frame,
                        unsigned char **coded_data, int *sizeof_coded_data)
{
    return encode_frame(p, scratch, opt, NULL, frame, NULL, coded_data, sizeof_coded_data);
}

/* ... by the scaling kernel (enc_scale.h): a window of a frame of another size, reduced to the encoder's picture */
int H264E_encode_device_scaled(H264E_persist_t *p, H264E_scratch_t *scratch, const H264E_run_param_t *opt, const H264E_dev_frame_t *frame,
                               const H264E_dev_window_t *win, unsigned char **coded_data, int *sizeof_coded_data)
{
    if (!frame || !win)
    {
        snprintf(g_host_err, sizeof(g_host_err), "H264E_encode_device_scaled: null %s", frame ? "window" : "frame");
        return H264E_STATUS_BAD_ARGUMENT;
    }
    return encode_frame(p, scratch, opt, NULL, frame, win, coded_data, sizeof_coded_data);
}

/* The reconstruction of the last frame -- the picture const_input_flag = 0 writes back for host input -- into device memory, by the egress
 * kernel (enc_egress.h).  A transparent VBV-overflow frame left the pool's pictures alone: the last reconstruction is what it shows. */
int H264E_read_recon_device(H264E_persist_t *p, const H264E_dev_frame_t *dst)
{
    henc_t *e = (henc_t *)p;
    impl_t mm;
    g_host_err[0] = 0;
    if (!impl_of(e, &mm)) return H264E_STATUS_BAD_ARGUMENT;
    if (!dst) { snprintf(g_host_err, sizeof(g_host_err), "H264E_read_recon_device: null destination"); return H264E_STATUS_BAD_ARGUMENT; }
    if (!e->have_recon)
    {
        snprintf(g_host_err, sizeof(g_host_err), "H264E_read_recon_device: no frame has been encoded yet");
        return H264E_STATUS_BAD_ARGUMENT;
    }
    return h264e_hip_egress_last(mm.pool, 0, dst->format, (void *const *)dst->plane, dst->stride, dst->pixel_bytes, dst->producer_stream) ? H264E_STATUS_BAD_ARGUMENT
                                                                                                                                     : H264E_STATUS_SUCCESS;
}

/* Quality of the last frame: the call's input as it lies in the pool's input slot against the picture H264E_read_recon_device reads */
int H264E_read_quality(H264E_persist_t *p, uint64_t ssd[3], double ssim[3])
{
    henc_t *e = (henc_t *)p;
    impl_t mm;
    g_host_err[0] = 0;
    if (!impl_of(e, &mm)) return H264E_STATUS_BAD_ARGUMENT;
    if (!ssd && !ssim) { snprintf(g_host_err, sizeof(g_host_err), "H264E_read_quality: both outputs are NULL"); return H264E_STATUS_BAD_ARGUMENT; }
    if (!e->have_recon)
    {
        snprintf(g_host_err, sizeof(g_host_err), "H264E_read_quality: no frame has been encoded yet");
        return H264E_STATUS_BAD_ARGUMENT;
    }
    return h264e_hip_quality_last(mm.pool, 0, ssd, ssim) ? H264E_STATUS_BAD_ARGUMENT : H264E_STATUS_SUCCESS;
}

/* The same SSIM for any pair of 8-bit planes in device memory (h264e_hip_ssim_planes).  The launch needs a stream and the partials
 * buffer of a pool: a one-slot 16 x 16 pool lives for the length of the call (nothing stays behind that would hold the device's process
 * guard); an application with many pairs to compare pays that once per call. */
int H264E_ssim_planes(int device, const void *a, int a_stride, const void *b, int b_stride, int width, int height, double *ssim)
{
    h264e_hip_pool_t *pool = NULL;
    int rc;
    g_host_err[0] = 0;
    if (h264e_hip_pool_create(&pool, device < 0 ? pick_device() : device, 16, 16, 1, 1)) return -1;
    rc = h264e_hip_ssim_planes(pool, a, a_stride, b, b_stride, width, height, ssim);
    h264e_hip_pool_destroy(pool);
    return rc;
}

void *H264E_dev_malloc(int device, size_t bytes) { g_host_err[0] = 0; return h264e_hip_dev_malloc(device, bytes); }
void H264E_dev_free(void *p) { h264e_hip_dev_free(p); }
int H264E_dev_memcpy(void *dst, const void *src, size_t bytes, int to_device) { g_host_err[0] = 0; return h264e_hip_dev_memcpy(dst, src, bytes, to_device); }

/* ------------------------------------------------------------------ whole-clip encode: temporal wavefront */

/*
 * The clip is ONE stream, encoded in stream order, but many consecutive frames are in flight at once: each frame is a
 * job of the same launch and starts a few macroblock rows behind the frame it references (h264e_kernels.hip), key
 * frames start immediately.  All frames of a launch speculate the mv_clusters state known when the launch starts;
 * afterwards the host validates them in order (exact walk of the per-macroblock records) and relaunches from the
 * first frame whose consumed candidates differ -- that frame with exact per-macroblock values.
 *
 * The encoder is resumable: H264E_clip_encode() encodes the frames that have been uploaded and not yet encoded (or as many
 * as fit the caller's output buffer) and keeps every piece of stream state -- position, mv_clusters, idr parity, rate
 * control, reference pictures -- for the next call.  Input frames live in a ring of `resident` HBM slots, so a file of any
 * length streams through a bounded amount of host and device memory (encode_app --clip).
 */
#define CLIP_KEEP_MAX 96        /* key frames of one stopped launch whose rows are kept: up to 64 led ones (h264e_pool.h H264E_LEAD_MAX_JOBS: small pictures,
                                   a budget of 384 rows at 9+ rows each) and the whole ones in front of and between them */
/* the progress of one frame pass: frames [0, done) are made, [ring_lo, done) still have their entries on the device,
 * which keeps `entries` of them, frame f in entry f % entries (0: the results live on the host only) */
typedef struct { int done, ring_lo, entries; } clip_pass_t;
struct H264E_clip_tag
{
    H264E_clip_param_t par;
    seq_t seq;
    int nframes, ring;
    int resident;                           /* input frames kept in HBM (ring): frame f lives in slot f % resident */
    int time_input;                         /* H264E_clip_input_time: time the launches of the device uploads */
    double input_ms;
    long long input_frames;
    h264e_hip_pool_t *pool;
    /* ---- stream state, kept across H264E_clip_encode calls */
    int next;                               /* next frame to encode */
    int avail;                              /* frames [0, avail) have been uploaded / generated */
    int pending_avail;                      /* ... once the asynchronous uploads in flight have landed */
    void (*idle_hook)(void *token); void *idle_token;   /* called while the encoder waits for the GPU (the app feeds uploads from it) */
    int32_t state[2];                       /* exact mv_clusters in front of frame `next` */
    int first_dev;                          /* the next launch's first frame is encoded again with the per-macroblock trajectory its walk left on the device */
    int first_row;                          /* ... which restarts at this macroblock row */
    int32_t after[2]; int have_after;       /* predicted state behind that frame */
    int narrow;                             /* reference-window geometry in use (h264e_dev.h) */
    int narrow_ok;                          /* the picture size allows the narrow geometry at all, and H264E_WIDE_WINDOW was not set when the clip was opened */
    int wide_until, wide_hold;              /* wide geometry until this frame; length of the next wide spell (doubles when narrow fails again) */
    int launch_base, launch_frames;         /* frames per launch: the pipeline depth after a mis-speculation, growing after clean launches (H264E_clip_open) */
    int stopped_before;                     /* the previous launch was stopped before its last frame (statistics: the next one pays a pipeline refill) */
    long long far_acc; int far_frames;      /* far reads / frames since the last decision */
    int rc_on;                              /* frame-level rate control: kbps > 0, or qp 0 (QP 10..51 without a byte target, as H264E_encode) */
    rc_t rcs; int rc_frame, rc_qp;          /* rate control: state, the frame rc_frame_start has run for, its QP */
    int rc_last_bytes[2];                   /* size of the last accepted P / key frame: what a frame still in flight is predicted to weigh */
    /* keep_records: what every accepted frame consumed, so that a different start state can be validated later (GOP shards) */
    h264e_hip_mbrec_t **rec_store;          /* [nframes] macroblock records of the accepted encode, or NULL */
    int32_t (*used_store)[2];               /* [nframes] frame-constant candidates it was given ... */
    int32_t **permb_store;                  /* [nframes] ... or the per-macroblock trajectory it was given */
    uint64_t *ssd_out;                      /* optional: [3] sums of squared differences input vs reconstruction per encoded frame of a call */
    double *ssim_out;                       /* optional: [3] SSIM values of the same pairs, indexed the same way (H264E_clip_set_ssim_output) */
    int recon_floor;                        /* rate control: frames below this one may have been overwritten by hedge leaves (H264E_clip_read_recon) */
    int32_t *traj;                          /* scratch: walked trajectory [nmb][2] */
    uint8_t *big; size_t big_cap;           /* scratch: NALs of a frame that did not fit the host mirror */
    h264e_hip_task_t *tasks;                /* scratch [ring] */
    int32_t (*used)[2];                     /* scratch [ring] */
    clip_pass_t sc, la, den;                /* the frame passes' progress: scene cut, cost pass, denoiser */
    /* temporal denoiser (H264E_clip_set_denoise), and the kernel that fills its ring (H264E_clip_set_denoise_motion): 0 = the plain
     * denoiser, 1 / 2 = enc_mcdenoise.h, from the motion field of the searched cost pass */
    int denoise, den_motion;
    /* The key-frame schedule: what H264E_encode would make of frame f when it is handed H264E_FRAME_TYPE_KEY on the frames of the
     * explicit list (H264E_clip_set_key_frames) and on the detected scene cuts, and H264E_FRAME_TYPE_DEFAULT on all others
     * (h264-lab.h:6725-6775, :6611-6614).  [nframes + 1]; built by clip_sched_build, the ONLY place that knows the rule; everything
     * that needs a frame's kind, frame_num or idr_pic_id reads it here. */
    struct clip_sched { uint8_t key, idr; int frame_num; } *sched;      /* idr: parity of the key frames up to and including this one */
    int *forced, nforced;                   /* the explicit list, ascending */
    int all_key;                            /* every frame is a key frame (launches as long as memory allows: nothing to mis-speculate) */
    /* scene-cut detection (H264E_clip_set_scenecut, enc_scenecut.h).  The arrays exist once the detector has been switched on. */
    int scenecut;                           /* threshold (0 = off) */
    uint32_t *sc_hist;                      /* [nframes][64] */
    int *sc_dist; uint8_t *sc_cut;          /* [nframes] D(f); f was made a key frame by the detector */
    double sc_kernel_ms; long long sc_frames;   /* HIP-event time of the detector's launches and the frames they analysed, since open */
    /* a QP per frame (H264E_clip_set_qp_schedule, or written window by window by the lookahead controller): frame f is coded as
     * H264E_encode codes it with qp_min = qp_max = qp_sched[f]; NULL = the clip's own QP / rate control */
    uint8_t *qp_sched;                      /* [nframes] */
    int qp_explicit;                        /* the caller's schedule (kept across a rewind), not the controller's */
    /* lookahead rate control (H264E_clip_set_lookahead): the project's own controller, defined in include/h264e_mi355x.h */
    int la_kbps, la_window, la_qmin, la_qmax;   /* la_kbps 0 = off */
    uint64_t *la_rec;                       /* [nframes][3] I, P, N */
    int *la_bits;                           /* [nframes] coded bits of the accepted frames of the current pass */
    int la_planned, la_closed;              /* windows whose QP has been chosen / whose frames have all been accepted (calibration and carry done) */
    uint64_t la_k[2];                       /* the calibration factors, P and key frames */
    long long la_debt;                      /* sum over the closed windows of target - actual bits */
    double la_kernel_ms; long long la_frames;
    /* motion search in the cost pass (H264E_clip_set_lookahead_search): the range, 0 = off; a frame has been analysed since open (its
     * records belong to that range) */
    int la_search, la_any;
    /* cost tree over the motion field (H264E_clip_set_lookahead_tree, enc_lookahead_tree.h): per-frame QP offsets inside a window.  The
     * arrays exist once the tree has been switched on; tr counts the frames of the planned windows, whose block maps are in the pool */
    int la_tree, la_ahead;                  /* strength in quarter QP steps per doubling (0 = off); frames behind a window that its tree starts from */
    uint64_t *tr_sum;                       /* [nframes] S(f) of the run that planned f's window */
    int8_t *tr_delta;                       /* [nframes] the offset it became */
    uint8_t *tr_base, *tr_key;              /* [nframes] the base QP of f's window; scratch: the schedule's key flags for a run */
    clip_pass_t tr;
    double tr_kernel_ms; long long tr_steps;
    /* Key frames that a stopped launch left encoded, wholly or down to some macroblock row: a key frame reads no reference
     * picture and no mv_clusters candidates, so what the next launch would make of those rows is what already lies in the frame's slot.
     * Collected when a launch has stopped cleanly (clip_keep_collect), used and forgotten by the next plan (clip_plan_launch); an entry
     * carries everything the rows' bits depend on besides the input picture. */
    int keep_on;                            /* H264E_KEEP_KEY_ROWS, read once at open */
    int key_lead;                           /* H264E_KEY_LEAD, read with it: -1 the default budget, 0 off, N row workgroups */
    int nkeep;
    struct clip_keep { int frame, rows, qp, nslices, speed, denoised; } keep[CLIP_KEEP_MAX];
};

/* the kept rows of frames `from` and later are void: their inputs are being replaced, or the stream goes back */
static void clip_keep_drop(H264E_clip_t *c, int from)
{
    int i, k = 0;
    for (i = 0; i < c->nkeep; i++) if (c->keep[i].frame < from) c->keep[k++] = c->keep[i];
    c->nkeep = k;
}

/* ---- the frame passes' bookkeeping; the passes themselves are further down (clip_prepass_*) */

/* How many frames a call with frames [0, limit) uploaded has to make, from p->done on: 0 = none, -1 = more than the input ring holds.
 * (An upload is checked against the frames not encoded yet at its upper end only, so a caller can get here.) */
static int clip_pass_pending(const H264E_clip_t *c, const clip_pass_t *p, const char *pass, int limit)
{
    if (limit - p->done > c->resident) { snprintf(g_host_err, sizeof(g_host_err), "%s: frames %d..%d do not fit the input ring", pass, p->done, limit - 1); return -1; }
    return imax(limit - p->done, 0);
}

/* frames [a, limit) have been made */
static void clip_pass_made(clip_pass_t *p, int a, int limit)
{
    p->done = limit;
    /* frames a.. took the entries of frames a - entries..: what was intact in front of a still is, from limit - entries on (no entries: nothing) */
    p->ring_lo = imax(imin(p->ring_lo, a), limit - p->entries);
}

/* is `frame` among the frames whose entries are still on the device?  If not, the reader's error text */
static int clip_pass_resident(const clip_pass_t *p, int frame, const char *who, const char *what)
{
    const int hi = p->done, lo = imin(p->ring_lo, hi);
    if (frame >= lo && frame < hi) return 1;
    if (lo < hi) snprintf(g_host_err, sizeof(g_host_err), "%s: frame %d has no %s on the device (frames %d..%d have)", who, frame, what, lo, hi - 1);
    else snprintf(g_host_err, sizeof(g_host_err), "%s: frame %d has no %s on the device (no frame has)", who, frame, what);
    return 0;
}

/* new inputs from frame `first` on: what the passes made of them, and of all behind them, is made again, and no row of an earlier
 * encode of theirs stands */
static void clip_inputs_replaced(H264E_clip_t *c, int first)
{
    if (first < c->sc.done) c->sc.done = first;
    if (first < c->la.done) c->la.done = first;
    if (first < c->den.done) c->den.done = first;
    clip_keep_drop(c, first);
}

/* frame `first` would be made again, from what the pass kept of frame first - 1: refused when that has left the ring */
static int clip_pass_predecessor_gone(const clip_pass_t *p, int first, const char *made, const char *kept, const char *ring)
{
    if (first <= 0 || first >= p->done || first - 1 >= p->done - p->entries) return 0;
    snprintf(g_host_err, sizeof(g_host_err), "upload: frame %d would be %s again, but the %s in front of it has left the %s (rewind and upload from frame 0)", first, made, kept, ring);
    return -1;
}

/* The schedule rule, once.  frame_num restarts at every key frame, and so does the periodic counter: the next periodic key frame
 * comes `gop` frames after the last key frame of either kind.  The wrap of the counter (h264-lab.h:6611) happens only on a DEFAULT
 * call: with gop = 1 the frame behind a forced key frame is a P frame.  A detected cut is a forced key frame on a frame that would
 * not be one anyway. */
static void clip_sched_build(H264E_clip_t *c)
{
    const int gop = c->par.gop;
    int f, k = 0, fn = 0, parity = 0, all = 1;
    for (f = 0; f <= c->nframes; f++)
    {
        int forced, key;
        while (k < c->nforced && c->forced[k] < f) k++;
        forced = k < c->nforced && c->forced[k] == f;
        if (c->sc_cut && f < c->nframes)
        {
            c->sc_cut[f] = (uint8_t)(!forced && fn && c->scenecut && f < c->sc.done && c->sc_dist[f] > c->scenecut);
            forced |= c->sc_cut[f];
        }
        key = forced || fn == 0;
        if (key) { fn = 0; parity ^= 1; }
        c->sched[f].key = (uint8_t)key; c->sched[f].idr = (uint8_t)parity; c->sched[f].frame_num = fn;
        if (f < c->nframes) all &= key;
        if (++fn >= gop && gop && !forced) fn = 0;
    }
    c->all_key = all;
}

static int clip_nslices(const H264E_clip_t *c) { return c->par.slices > 1 ? imin(imin(c->par.slices, H264E_HIP_MAX_SLICES), c->seq.nmby) : 1; }

/* frames per launch at frame 0: optimistic where mis-speculations are rare by construction (row bands restart the state, intra frames
 * do not read it): as long as memory allows; else the pipeline depth, growing with every clean launch */
static void clip_launch_frames_reset(H264E_clip_t *c) { c->launch_frames = (c->par.slices > 1 || c->all_key) ? c->ring - 1 : c->launch_base; }

/* the HBM budget of the slot ring and what one slot takes: two pictures, records, row bit buffers (2 KB per macroblock), arenas */
#define CLIP_DEV_BUDGET (24.0*1073741824.0)
static double clip_dev_slot_bytes(int nmb) { return (double)nmb*256.0*3.0 + (double)nmb*(64 + 96 + 8 + 640 + 660 + 2048 + 64) + 65536.0; }

int H264E_struct_size(int which) { return which == 0 ? (int)sizeof(H264E_clip_param_t) : which == 1 ? (int)sizeof(H264E_clip_stats_t) : which == 2 ? (int)sizeof(H264E_dev_frame_t) : -1; }

static double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec*1e3 + ts.tv_nsec*1e-6;
}

/* the lookahead controller's initial calibration factors, P and key frames (bits << 24 per unit of cost x the reference's
 * bits-per-macroblock entry): medians over the test clips at CIF, QP 20..38 (tools/lookahead_calibrate.py); every
 * accepted window replaces them */
#define LOOKAHEAD_K0_P 15086u
#define LOOKAHEAD_K0_KEY 14322u
/* ... of P frames when the cost pass searches (H264E_clip_set_lookahead_search): the same medians over the searched P(f), range 8 */
#define LOOKAHEAD_K0_SEARCH 53818u

void H264E_clip_rewind(H264E_clip_t *c)
{
    if (!c) return;
    c->next = 0;
    c->state[0] = c->par.mv_clusters_in[0]; c->state[1] = c->par.mv_clusters_in[1];
    c->first_dev = 0;
    c->first_row = 0; c->have_after = 0; c->recon_floor = 0; c->stopped_before = 0;
    clip_keep_drop(c, 0);
    /* reference-window geometry (h264e_dev.h): narrow = consecutive frames 4 macroblock steps apart, as long as vectors rarely
     * reach more than 12 samples right / down of their macroblock; wide (7 steps) for the rest of the clip otherwise.  Large
     * pictures already fill the GPU's resident workgroups with the wide geometry: the narrow one only pays below ~12k macroblocks */
    c->narrow = c->narrow_ok;
    c->wide_until = 0; c->wide_hold = 30; c->far_acc = 0; c->far_frames = 0;
    clip_launch_frames_reset(c);
    memset(&c->rcs, 0, sizeof(c->rcs));
    c->rc_frame = -1; c->rc_qp = c->par.qp; c->rc_last_bytes[0] = c->rc_last_bytes[1] = 0;
    /* lookahead controller: every pass starts from the same factors and no carry, so it chooses the same QPs again */
    c->la_planned = c->la_closed = 0; c->la_debt = 0;
    c->tr.done = c->tr.ring_lo = 0;                     /* no window is planned: no frame has a sum, an offset or a map */
    c->la_k[0] = c->la_search ? LOOKAHEAD_K0_SEARCH : LOOKAHEAD_K0_P; c->la_k[1] = LOOKAHEAD_K0_KEY;
}

int H264E_clip_open(H264E_clip_t **out, const H264E_clip_param_t *par, int nframes)
{
    H264E_clip_t *c;
    g_host_err[0] = 0;
    if (!out || !par || nframes <= 0 || par->width <= 0 || par->height <= 0 || ((par->width | par->height) & 1) || par->gop < 0) return -1;
    c = (H264E_clip_t *)calloc(1, sizeof(*c));
    if (!c) return -1;
    c->par = *par;
    /* encode_app passes qp_min = qp_max = --qp to H264E_encode, which widens 0 (and only 0) to 10..51 (h264-lab.h:6707-6715): the
     * controller picks every QP then; any other value outside 10..51 is a constant QP at the nearer end */
    c->rc_on = par->kbps > 0 || par->qp == 0;
    c->par.qp = imin(imax(par->qp, 10), 51);
    seq_init(&c->seq, par->width, par->height, par->vbv_size_bytes, 0);
    c->nframes = nframes;
    /* H264E_WIDE_WINDOW is read here, once: the clip keeps the answer for life, whatever the variable says at a later rewind (clips
     * opened with and without it can share a launch group) */
    c->narrow_ok = (getenv("H264E_WIDE_WINDOW") || c->seq.nmb > 12000) ? 0 : 1;
    /* ... and so is H264E_KEEP_KEY_ROWS (0 = every launch encodes its key frames from row 0) */
    c->keep_on = getenv("H264E_KEEP_KEY_ROWS") ? atoi(getenv("H264E_KEEP_KEY_ROWS")) != 0 : 1;
    /* ... and H264E_KEY_LEAD: the coming key frames' rows at the front of every launch's dispatch order (h264e_hip_set_key_lead: 0 off,
     * N a budget of N row workgroups, unset the default budget).  Off without keeping: what a stopped launch led would be encoded again */
    c->key_lead = !c->keep_on ? 0 : getenv("H264E_KEY_LEAD") ? imax(atoi(getenv("H264E_KEY_LEAD")), 0) : -1;
    /* ring of picture / result slots = frames per launch + 1.  Not bounded by residency: workgroups only wait for lower
     * block indices, so a launch larger than the GPU simply streams through it in order. */
    /* default: 96 frames per launch at 1080p and above; small pictures have short pipelines and cheap slots, so they get
     * proportionally more (fewer launch boundaries), up to 1024 */
    {
        const int nmb = c->seq.nmb;
        /* large pictures: the ~2000 resident workgroups hold only a few frames (4K 33, 8K 16 at one workgroup per row), so slots
         * beyond that only cost memory: at most 6500 rows' worth */
        /* (row-band slices: relaunches are rare and every frame offers several wavefronts, twice as many slots pay) */
        /* (measured: 1080p 160 frames per launch after an event beat 96 by 2.5 %, 4K 96 beat 49 by 3 %; 8K is bound by the resident
         * workgroups, 25 frames beat 49 by 8 %) */
        const int rows_budget = (par->slices > 1 || c->seq.nmby <= 135) ? 13000 : 6500;
        c->launch_base = par->max_chains > 0 ? par->max_chains : imax(imin(161, imax(13, rows_budget/imax(c->seq.nmby, 1) + 1)), imin(1025, 97*8160/imax(nmb, 1))) - 1;
        /* That is the pipeline's depth: what a launch needs to keep the chip busy, and what a launch gets right after a
         * mis-speculation (everything behind the failed frame is thrown away, so a short launch wastes less set-up and drain).
         * But a launch BOUNDARY without an event costs a pipeline drain and refill too (one frame latency), so event-free stretches
         * -- row-band slices, all-intra streams, quiet content -- want launches as long as memory allows: the ring is sized by a
         * memory budget (896 MB of host-mapped mirrors, 24 GB of HBM) and the frames per launch grow again after every clean launch
         * (measured at 1080p x 600: 8 slices 14.5 -> 18.3 M MB/s, all-intra 14.2 -> 19.6 M, single slice 6.77 -> 6.94 M). */
        {
            const double host_slot = (double)nmb*168.0 + 65536.0 + 4096.0;
            const double dev_slot = clip_dev_slot_bytes(nmb);
            const double by_host = 896.0*1048576.0/host_slot, by_dev = CLIP_DEV_BUDGET/dev_slot;
            int cap = (int)(by_host < by_dev ? by_host : by_dev);
            cap = imin(imax(cap, c->launch_base), 1024);
            c->ring = (par->max_chains > 0 ? par->max_chains : cap) + 1;
        }
    }
    if (getenv("H264E_RING")) { c->ring = atoi(getenv("H264E_RING")); c->launch_base = imin(c->launch_base, imax(c->ring - 1, 1)); }      /* experiments */
    c->ring = imax(2, imin(c->ring, nframes + 1));
    if (getenv("H264E_LAUNCH_BASE")) c->launch_base = atoi(getenv("H264E_LAUNCH_BASE"));      /* experiments */
    c->launch_base = imax(1, imin(c->launch_base, c->ring - 1));
    c->resident = par->resident_frames > 0 ? imin(par->resident_frames, nframes) : nframes;
    c->den.entries = c->resident; c->la.entries = c->tr.entries = imax(c->resident, 2);         /* as the pool sizes its rings (h264e_pool.h) */
    c->traj = (int32_t *)malloc(sizeof(int32_t)*2*(size_t)c->seq.nmb);
    c->tasks = (h264e_hip_task_t *)calloc((size_t)c->ring, sizeof(*c->tasks));
    c->used = (int32_t (*)[2])calloc((size_t)c->ring, sizeof(int32_t[2]));
    c->sched = (struct clip_sched *)calloc((size_t)nframes + 1, sizeof(*c->sched));
    if (!c->traj || !c->tasks || !c->used || !c->sched) { free(c->traj); free(c->tasks); free(c->used); free(c->sched); free(c); return -1; }
    clip_sched_build(c);
    /* the ring is sized for speed, not for need: when the device (or the pinned host memory) cannot spare that much, halve it down
     * to the pipeline depth before giving up */
    while (h264e_hip_pool_create(&c->pool, par->device, par->width, par->height, c->ring, c->resident))
    {
        if (c->ring <= c->launch_base + 1 || par->max_chains > 0)
        {
            free(c->traj); free(c->tasks); free(c->used); free(c->sched); free(c);
            return -1;
        }
        c->ring = imax(c->launch_base + 1, c->ring/2);
    }
    h264e_hip_set_key_lead(c->pool, c->key_lead);
    if (par->keep_records)
    {
        c->rec_store = (h264e_hip_mbrec_t **)calloc((size_t)nframes, sizeof(*c->rec_store));
        c->used_store = (int32_t (*)[2])calloc((size_t)nframes, sizeof(int32_t[2]));
        c->permb_store = (int32_t **)calloc((size_t)nframes, sizeof(*c->permb_store));
        if (!c->rec_store || !c->used_store || !c->permb_store) { H264E_clip_close(c); return -1; }
    }
    H264E_clip_rewind(c);
    *out = c;
    return 0;
}

void H264E_clip_close(H264E_clip_t *c)
{
    if (!c) return;
    h264e_hip_pool_destroy(c->pool);
    if (c->rec_store) { int f; for (f = 0; f < c->nframes; f++) { free(c->rec_store[f]); if (c->permb_store) free(c->permb_store[f]); } }
    free(c->rec_store); free(c->used_store); free(c->permb_store);
    free(c->traj); free(c->tasks); free(c->used); free(c->big);
    free(c->sched); free(c->forced); free(c->sc_hist); free(c->sc_dist); free(c->sc_cut);
    free(c->qp_sched); free(c->la_rec); free(c->la_bits);
    free(c->tr_sum); free(c->tr_delta); free(c->tr_base); free(c->tr_key);
    free(c);
}

/* may frames [first, first + n) of the stream go into their ring slots?  A slot may only be overwritten once its old frame is encoded */
static int clip_put_allowed(const H264E_clip_t *c, int first, int n)
{
    if (!c || first < 0 || n < 0 || first + n > c->nframes) { snprintf(g_host_err, sizeof(g_host_err), "upload: bad frame range"); return -1; }
    if (first + n - c->resident > c->next) { snprintf(g_host_err, sizeof(g_host_err), "upload: input ring full (frames %d.. are not encoded yet)", c->next); return -1; }
    if (c->denoise && clip_pass_predecessor_gone(&c->den, first, "denoised", "denoised picture", "input ring")) return -1;
    /* the cost pass measures frame `first` against the half-resolution picture of the frame in front of it (enc_lookahead.h) */
    if ((c->la_kbps || c->den_motion) && clip_pass_predecessor_gone(&c->la, first, "analysed", "half-resolution picture", "ring")) return -1;
    return 0;
}

/* the input ring wraps: the slot of frame f, and in *run how many of the n frames from f on lie in consecutive slots */
static int clip_ring_piece(const H264E_clip_t *c, int f, int n, int *run)
{
    *run = imin(n, c->resident - f % c->resident);
    return f % c->resident;
}

/* frames [first, first + n) of the stream into their ring slots */
static int clip_put(H264E_clip_t *c, int first, int n, const uint8_t *i420, int async)
{
    size_t fsz;
    int done, slot, run;
    if (clip_put_allowed(c, first, n)) return -1;
    fsz = (size_t)c->seq.width*c->seq.height*3/2;
    for (done = 0; done < n; done += run)
    {
        slot = clip_ring_piece(c, first + done, n - done, &run);
        if (async ? h264e_hip_upload_i420_async(c->pool, slot, run, i420 + fsz*(size_t)done) : h264e_hip_upload_i420(c->pool, slot, run, i420 + fsz*(size_t)done))
        {
            g_host_err[0] = 0;          /* H264E_last_error() -> the device layer's text */
            return -1;
        }
    }
    if (async) { if (first + n > c->pending_avail) c->pending_avail = first + n; }
    else if (first + n > c->avail) c->avail = first + n;
    clip_inputs_replaced(c, first);
    return 0;
}

int H264E_clip_upload(H264E_clip_t *c, int first, int nframes, const uint8_t *i420)
{
    if (clip_put(c, first, nframes, i420, 0)) return -1;
    return h264e_hip_sync(c->pool);
}

/* The same from device memory, for a range that clip_put_allowed has passed: one ingest kernel per frame on the pool's copy stream
 * (enc_ingest.h) -- with a window one scaling kernel (enc_scale.h) -- all of them complete on return.  Every frame is checked before
 * the first one is launched, so a refused call leaves the input ring as it was. */
static int clip_put_device(H264E_clip_t *c, int first, int nframes, const H264E_dev_frame_t *frames, const H264E_dev_window_t *win)
{
    int i, rc = 0;
    double ms = 0;
    for (i = 0; i < nframes; i++)
    {
        const H264E_dev_frame_t *f = &frames[i];
        if (win ? h264e_hip_scale_check(c->pool, (first + i) % c->resident, f->format, f->plane, f->stride, (const int *)win)
                : h264e_hip_ingest_check(c->pool, (first + i) % c->resident, f->format, f->plane, f->stride, f->pixel_bytes)) return -1;
    }
    if (c->time_input && h264e_hip_copy_timer_start(c->pool)) return -1;
    for (i = 0; i < nframes && !rc; i++)
    {
        const H264E_dev_frame_t *f = &frames[i];
        rc = win ? h264e_hip_scale_device_async(c->pool, (first + i) % c->resident, f->format, f->plane, f->stride, (const int *)win, f->producer_stream)
                 : h264e_hip_ingest_device_async(c->pool, (first + i) % c->resident, f->format, f->plane, f->stride, f->pixel_bytes, f->producer_stream);
    }
    if (c->time_input && !h264e_hip_copy_timer_stop(c->pool, &ms)) { c->input_ms += ms; c->input_frames += i; }
    if (h264e_hip_upload_wait(c->pool) || rc) return -1;        /* (after a failure too: what was launched has read its source) */
    if (first + nframes > c->avail) c->avail = first + nframes;
    clip_inputs_replaced(c, first);
    return 0;
}

int H264E_clip_upload_device(H264E_clip_t *c, int first, int nframes, const H264E_dev_frame_t *frames)
{
    g_host_err[0] = 0;
    if (clip_put_allowed(c, first, nframes)) return -1;
    if (!frames) { snprintf(g_host_err, sizeof(g_host_err), "upload_device: null argument"); return -1; }
    return clip_put_device(c, first, nframes, frames, NULL);
}

int H264E_clip_upload_device_scaled(H264E_clip_t *c, int first, int nframes, const H264E_dev_frame_t *frames, const H264E_dev_window_t *win)
{
    g_host_err[0] = 0;
    if (clip_put_allowed(c, first, nframes)) return -1;
    if (!frames || !win) { snprintf(g_host_err, sizeof(g_host_err), "upload_device_scaled: null %s", frames ? "window" : "frames"); return -1; }
    return clip_put_device(c, first, nframes, frames, win);
}

/* diagnostic: HIP-event time of the ingest / scale launches of the device uploads made while `enable` was set */
int H264E_clip_input_time(H264E_clip_t *c, int enable, double *kernel_ms, long long *frames)
{
    if (!c) return -1;
    c->time_input = enable != 0;
    if (kernel_ms) *kernel_ms = c->input_ms;
    if (frames) *frames = c->input_frames;
    return 0;
}

/* the same from pinned host memory (H264E_clip_host_alloc) on the pool's copy stream: returns at once, the frames count as
 * uploaded after H264E_clip_upload_wait() */
int H264E_clip_upload_async(H264E_clip_t *c, int first, int nframes, const uint8_t *pinned_i420) { return clip_put(c, first, nframes, pinned_i420, 1); }
int H264E_clip_upload_wait(H264E_clip_t *c)
{
    if (!c || h264e_hip_upload_wait(c->pool)) return -1;
    if (c->pending_avail > c->avail) c->avail = c->pending_avail;
    return 0;
}
/* 1 = every asynchronous upload has landed (the frames now count as uploaded), 0 = still copying */
int H264E_clip_upload_poll(H264E_clip_t *c)
{
    int busy;
    if (!c) return -1;
    busy = h264e_hip_upload_busy(c->pool);
    if (busy < 0) { g_host_err[0] = 0; return -1; }     /* the copy stream failed: H264E_last_error() carries the HIP text */
    if (busy) return 0;
    if (c->pending_avail > c->avail) c->avail = c->pending_avail;
    return 1;
}
void H264E_clip_position(const H264E_clip_t *c, int *next_frame, int *uploaded_frames)
{
    if (next_frame) *next_frame = c ? c->next : 0;
    if (uploaded_frames) *uploaded_frames = c ? c->avail : 0;
}
void H264E_clip_set_idle_hook(H264E_clip_t *c, void (*hook)(void *token), void *token) { if (c) { c->idle_hook = hook; c->idle_token = token; } }
void *H264E_clip_host_alloc(size_t bytes) { return h264e_hip_host_alloc(bytes); }
void H264E_clip_host_free(void *p) { h264e_hip_host_free(p); }

int H264E_clip_generate_synth(H264E_clip_t *c, int first, int nframes, int t0, uint32_t seed)
{
    int done, slot, run;
    if (clip_put_allowed(c, first, nframes)) return -1;
    for (done = 0; done < nframes; done += run)
    {
        slot = clip_ring_piece(c, first + done, nframes - done, &run);
        if (h264e_hip_generate_synth(c->pool, slot, run, t0 + done, seed)) { g_host_err[0] = 0; return -1; }
    }
    if (first + nframes > c->avail) c->avail = first + nframes;
    clip_inputs_replaced(c, first);
    return h264e_hip_sync(c->pool);
}

/* reconstruction of an already encoded frame (coded size, packed I420), while its picture slot has not been reused: the last
 * ring - 1 frames */
/* the resident input frames back (measurement helper for bench.py's PCIe-inclusive pass) */
int H264E_clip_download(H264E_clip_t *c, int first, int nframes, uint8_t *i420)
{
    if (!c || c->resident < c->nframes) return -1;
    return h264e_hip_download_i420(c->pool, first, nframes, i420);
}

int H264E_clip_read_recon(H264E_clip_t *c, int frame, uint8_t *dst)
{
    if (!c || !dst || frame < 0 || frame >= c->next || frame < c->next - (c->ring - 1)) return -1;
    /* rate control: the launches' hedge leaves (alternative QPs of frames in flight) are encoded in spare slots of the ring, i.e. over
     * the pictures of older frames -- only the frames accepted since the last launch's first frame are guaranteed to be intact */
    if (c->rc_on && frame < c->recon_floor) return -1;
    return h264e_hip_read_recon_slot(c->pool, frame % c->ring, dst);
}

/* the same picture, cropped to the clip's width x height, into device memory by the egress kernel (enc_egress.h): the window of
 * H264E_clip_read_recon, every refusal with its reason */
int H264E_clip_read_recon_device(H264E_clip_t *c, int frame, const H264E_dev_frame_t *dst)
{
    g_host_err[0] = 0;
    if (!c || !dst) { snprintf(g_host_err, sizeof(g_host_err), "clip_read_recon_device: null %s", c ? "destination" : "clip"); return -1; }
    if (frame < 0 || frame >= c->next)
    {
        snprintf(g_host_err, sizeof(g_host_err), "clip_read_recon_device: frame %d has not been encoded (%d frames have)", frame, c->next);
        return -1;
    }
    if (frame < c->next - (c->ring - 1))
    {
        snprintf(g_host_err, sizeof(g_host_err), "clip_read_recon_device: the picture of frame %d has been overwritten (the last %d frames are kept: %d..%d)", frame, c->ring - 1,
                 imax(c->next - (c->ring - 1), 0), c->next - 1);
        return -1;
    }
    if (c->rc_on && frame < c->recon_floor)
    {
        snprintf(g_host_err, sizeof(g_host_err), "clip_read_recon_device: the picture of frame %d may have been overwritten by the rate control's alternative encodes (frames %d..%d are intact)",
                 frame, c->recon_floor, c->next - 1);
        return -1;
    }
    return h264e_hip_egress_slot(c->pool, frame % c->ring, dst->format, (void *const *)dst->plane, dst->stride, dst->pixel_bytes, dst->producer_stream);
}

/* diagnostic: HIP-event time of the egress launches made while `enable` was set (tools/egress_probe.py) */
int H264E_clip_output_time(H264E_clip_t *c, int enable, double *kernel_ms, long long *frames)
{
    if (!c) return -1;
    return h264e_hip_egress_time(c->pool, enable, kernel_ms, frames);
}

/* [3] sums of squared differences (Y, U, V; input vs reconstruction) per frame encoded by the following H264E_clip_encode calls,
 * computed on the device (encode_app --psnr); NULL switches it off */
void H264E_clip_set_ssd_output(H264E_clip_t *c, uint64_t *ssd) { if (c) c->ssd_out = ssd; }

/* ... and [3] SSIM values per frame (enc_ssim.h), filled next to the sums in clip_settle; NULL switches it off */
int H264E_clip_set_ssim_output(H264E_clip_t *c, double *ssim)
{
    g_host_err[0] = 0;
    if (!c) { snprintf(g_host_err, sizeof(g_host_err), "H264E_clip_set_ssim_output: null clip"); return -1; }
    if (ssim && (c->seq.width < 16 || c->seq.height < 16))
    {
        snprintf(g_host_err, sizeof(g_host_err), "H264E_clip_set_ssim_output: a %d x %d picture has a chroma plane without an 8 x 8 window: SSIM needs 16 x 16 at least", c->seq.width, c->seq.height);
        return -1;
    }
    c->ssim_out = ssim;
    return 0;
}

/* diagnostic: HIP-event time of the SSD and SSIM launches made while `enable` was set (tools/quality_probe.py) */
int H264E_clip_quality_time(H264E_clip_t *c, int enable, double *ssd_ms, double *ssim_ms, long long *frames)
{
    if (!c) return -1;
    return h264e_hip_quality_time(c->pool, enable, ssd_ms, ssim_ms, frames);
}

/*
 * GOP sharding of ONE stream: a shard that started from a SPECULATED mv_clusters state is checked once the
 * exact state in front of its first frame is known (the end state of the shard before it).  Walks every accepted frame from
 * exact_in with the records kept by keep_records and compares the rounded candidates each macroblock consumed with the exact
 * ones.  All equal: *restart_frame = -1, the shard's bytes stand, end_state = the exact state behind its last
 * frame (which becomes the encoder's own state).  Otherwise *restart_frame = first frame of the GOP that holds the first
 * divergent macroblock and restart_state = the exact state in front of it: everything from there on has to be encoded again
 * (H264E_clip_restart, then H264E_clip_encode); the frames before it stand.
 */
int H264E_clip_revalidate(H264E_clip_t *c, const int32_t exact_in[2], int *restart_frame, int32_t restart_state[2], int32_t end_state[2])
{
    int32_t s[2], gop_state[2];
    int f, nslices;
    if (!c || !c->rec_store || !exact_in || !restart_frame) return -1;
    nslices = clip_nslices(c);
    s[0] = gop_state[0] = exact_in[0]; s[1] = gop_state[1] = exact_in[1];
    *restart_frame = -1;
    for (f = 0; f < c->next; f++)
    {
        if (c->sched[f].key) { gop_state[0] = s[0]; gop_state[1] = s[1]; }
        if (!c->rec_store[f]) return -1;
        if (clusters_walk(s, c->rec_store[f], c->seq.nmbx, c->seq.nmby, nslices, c->permb_store[f] ? c->permb_store[f] : c->used_store[f], c->permb_store[f] != NULL, NULL) >= 0)
        {
            while (!c->sched[f].key) f--;
            *restart_frame = f;
            if (restart_state) { restart_state[0] = gop_state[0]; restart_state[1] = gop_state[1]; }
            return 0;
        }
    }
    if (end_state) { end_state[0] = s[0]; end_state[1] = s[1]; }
    c->state[0] = s[0]; c->state[1] = s[1];
    return 0;
}

/* the kept macroblock records of an accepted frame (keep_records): {mv[0] packed (y << 16) | (x & 0xffff), type -1 skip / 0..3 inter
 * partitioning / 5 I4x4 / 6 I16x16, consumed-the-cluster-candidates flag} per macroblock -- what a per-macroblock comparison with another
 * implementation's trace needs (tests) */
int H264E_clip_read_records(H264E_clip_t *c, int frame, void *dst /* nmb x 8 bytes */)
{
    if (!c || !dst || !c->rec_store || frame < 0 || frame >= c->next || !c->rec_store[frame]) return -1;
    memcpy(dst, c->rec_store[frame], sizeof(h264e_hip_mbrec_t)*(size_t)c->seq.nmb);
    return 0;
}

/* continue (again) at `frame`, which must start a GOP, with `state` in front of it; the frames behind it are encoded again by the
 * next H264E_clip_encode calls (their inputs must be resident / uploaded again) */
int H264E_clip_restart(H264E_clip_t *c, int frame, const int32_t state[2])
{
    if (!c || !state || frame < 0 || frame > c->avail || frame > c->nframes || !c->sched[frame].key) return -1;
    if (c->denoise && frame) { snprintf(g_host_err, sizeof(g_host_err), "restart: a denoised stream restarts at frame 0 only"); return -1; }
    c->next = frame;
    if (c->resident < c->nframes) c->avail = c->pending_avail = frame;      /* a ring: the inputs from here on have to be uploaded again */
    c->state[0] = state[0]; c->state[1] = state[1];
    c->first_dev = 0;
    c->first_row = 0; c->have_after = 0;
    clip_keep_drop(c, 0);
    c->rc_frame = -1;
    return 0;
}

/* diagnostic (stamps build): per-phase cycle sums since the last call */
/* The temporal denoiser for the clip encoder (see H264E_set_denoise): while the clip stands at frame 0.  With speed < 2 every frame is
 * denoised on the device, in stream order, before the launch that first encodes it; the denoised pictures are a pure function of the
 * inputs, so a rewind keeps them until frames are uploaded again.  Refused together with keep_records (a GOP shard's first frame
 * would need the denoised picture of the frame in front of it, which lives in another encoder). */
/* the denoised ring of a clip whose denoiser is off: the budget check, the allocation, the zero state */
static int clip_denoise_ring(H264E_clip_t *c, const char *who)
{
    /* the denoised frames (one per resident input slot + the zero state) count in the HBM budget that sized the slot ring */
    const double fsz = (double)c->seq.width*c->seq.height*3/2, den = fsz*(c->resident == 1 ? 3 : c->resident + 1);
    if (c->par.max_chains <= 0 && (double)c->ring*clip_dev_slot_bytes(c->seq.nmb) + den > CLIP_DEV_BUDGET)
    {
        snprintf(g_host_err, sizeof(g_host_err), "%s: %d slots + %.0f MB of denoised frames exceed the %.0f GB budget: open with max_chains or resident_frames",
                 who, c->ring, den/1048576.0, CLIP_DEV_BUDGET/1073741824.0);
        return -1;
    }
    if (h264e_hip_denoise_reset(c->pool)) return -1;
    c->den.done = c->den.ring_lo = 0;
    return 0;
}

int H264E_clip_set_denoise(H264E_clip_t *c, int on)
{
    g_host_err[0] = 0;
    if (!c) return -1;
    if (c->next) { snprintf(g_host_err, sizeof(g_host_err), "set_denoise: only at frame 0 (after open or rewind)"); return -1; }
    if (on && c->par.keep_records) { snprintf(g_host_err, sizeof(g_host_err), "set_denoise: not with keep_records (GOP shards)"); return -1; }
    if (on && !c->denoise && clip_denoise_ring(c, "set_denoise")) return -1;
    c->denoise = !!on;
    if (!on) c->den_motion = 0;         /* off is off for the motion-compensated filter too; on leaves the kernel that fills the ring as it is */
    return 0;
}

/* Colour and frame rate of the clip's stream (see H264E_set_color): while the clip stands at frame 0; kept across a rewind.  Frames
 * uploaded before the call keep the bytes they were converted to. */
int H264E_clip_set_color(H264E_clip_t *c, int matrix, int full_range)
{
    g_host_err[0] = 0;
    if (!c) return -1;
    if (c->next) { snprintf(g_host_err, sizeof(g_host_err), "clip_set_color: only at frame 0 (after open or rewind), not at frame %d", c->next); return -1; }
    if (color_refused("clip_set_color", matrix, full_range)) return -1;
    return color_apply(&c->seq, c->pool, matrix, full_range);
}

/* H264E_set_tonemap for the clip: while it stands at frame 0; the pool keeps the setting, so a rewind does.  Frames uploaded before the
 * call keep the bytes they were converted to */
int H264E_clip_set_tonemap(H264E_clip_t *c, int transfer, int curve, double peak_nits, double ref_white_nits)
{
    g_host_err[0] = 0;
    if (!c) return -1;
    if (c->next) { snprintf(g_host_err, sizeof(g_host_err), "clip_set_tonemap: only at frame 0 (after open or rewind), not at frame %d", c->next); return -1; }
    return h264e_hip_tonemap_set(c->pool, "clip_set_tonemap", transfer, curve, peak_nits, ref_white_nits);
}

int H264E_clip_tonemap_state(H264E_clip_t *c, long long state[3])
{
    g_host_err[0] = 0;
    if (!c) return -1;
    return h264e_hip_tonemap_state(c->pool, state);
}

int H264E_clip_set_frame_rate(H264E_clip_t *c, int num, int den)
{
    g_host_err[0] = 0;
    if (!c) return -1;
    if (c->next) { snprintf(g_host_err, sizeof(g_host_err), "clip_set_frame_rate: only at frame 0 (after open or rewind), not at frame %d", c->next); return -1; }
    if (fps_refused("clip_set_frame_rate", num, den)) return -1;
    c->seq.fps_num = num; c->seq.fps_den = den;
    return 0;
}

/* The key-frame schedule of the clip: frames[0..n) become key frames in addition to the periodic ones, exactly as
 * H264E_FRAME_TYPE_KEY on those frames does in H264E_encode.  While the clip stands at frame 0; kept across a rewind; n = 0 clears
 * the list.  Refused with keep_records: GOP shards (H264E_clip_revalidate / _restart) assume fixed GOP blocks. */
int H264E_clip_set_key_frames(H264E_clip_t *c, const int *frames, int n)
{
    int *copy = NULL, i;
    g_host_err[0] = 0;
    if (!c || n < 0 || (n && !frames)) { snprintf(g_host_err, sizeof(g_host_err), "set_key_frames: bad argument"); return -1; }
    if (c->next) { snprintf(g_host_err, sizeof(g_host_err), "set_key_frames: only at frame 0 (after open or rewind)"); return -1; }
    if (c->par.keep_records) { snprintf(g_host_err, sizeof(g_host_err), "set_key_frames: not with keep_records (GOP shards assume fixed GOP blocks)"); return -1; }
    for (i = 0; i < n; i++)
    {
        if (frames[i] < 0 || frames[i] >= c->nframes) { snprintf(g_host_err, sizeof(g_host_err), "set_key_frames: frame %d is outside the clip (%d frames)", frames[i], c->nframes); return -1; }
        if (i && frames[i] <= frames[i - 1]) { snprintf(g_host_err, sizeof(g_host_err), "set_key_frames: the list must be ascending (%d after %d)", frames[i], frames[i - 1]); return -1; }
    }
    if (n)
    {
        copy = (int *)malloc(sizeof(int)*(size_t)n);
        if (!copy) { snprintf(g_host_err, sizeof(g_host_err), "out of host memory"); return -1; }
        memcpy(copy, frames, sizeof(int)*(size_t)n);
    }
    free(c->forced);
    c->forced = copy; c->nforced = n;
    clip_sched_build(c);
    clip_launch_frames_reset(c);
    return 0;
}

/* Scene-cut detection (enc_scenecut.h): threshold in 1/1024 of the picture, 0 = off.  While the clip stands at frame 0; refused with
 * keep_records like the explicit list.  Histograms that were made before stay valid: only the cuts are decided again. */
int H264E_clip_set_scenecut(H264E_clip_t *c, int threshold)
{
    g_host_err[0] = 0;
    if (!c || threshold < 0) { snprintf(g_host_err, sizeof(g_host_err), "set_scenecut: bad argument"); return -1; }
    if (c->next) { snprintf(g_host_err, sizeof(g_host_err), "set_scenecut: only at frame 0 (after open or rewind)"); return -1; }
    if (threshold && c->par.keep_records) { snprintf(g_host_err, sizeof(g_host_err), "set_scenecut: not with keep_records (GOP shards assume fixed GOP blocks)"); return -1; }
    if (threshold && !c->sc_hist)
    {
        c->sc_hist = (uint32_t *)calloc((size_t)c->nframes*64, sizeof(uint32_t));
        c->sc_dist = (int *)calloc((size_t)c->nframes, sizeof(int));
        c->sc_cut = (uint8_t *)calloc((size_t)c->nframes, 1);
        if (!c->sc_hist || !c->sc_dist || !c->sc_cut)
        {
            free(c->sc_hist); free(c->sc_dist); free(c->sc_cut);
            c->sc_hist = NULL; c->sc_dist = NULL; c->sc_cut = NULL;
            snprintf(g_host_err, sizeof(g_host_err), "out of host memory");
            return -1;
        }
    }
    c->scenecut = threshold;
    clip_sched_build(c);
    clip_launch_frames_reset(c);
    return 0;
}

int H264E_clip_read_scenecut(H264E_clip_t *c, int first, int n, int *dist, uint8_t *is_cut)
{
    int i;
    g_host_err[0] = 0;
    if (!c || !c->sc_dist) { snprintf(g_host_err, sizeof(g_host_err), "read_scenecut: the detector has not been switched on"); return -1; }
    if (first < 0 || n < 0 || first + n > c->sc.done) { snprintf(g_host_err, sizeof(g_host_err), "read_scenecut: frames %d..%d have not been analysed (%d have)", first, first + n - 1, c->sc.done); return -1; }
    for (i = 0; i < n; i++)
    {
        if (dist) dist[i] = c->sc_dist[first + i];
        if (is_cut) is_cut[i] = c->sc_cut[first + i];
    }
    return 0;
}

/* diagnostic (tools/scenecut_probe.py): HIP-event time of the detector's kernel launches since open, and the frames they analysed */
int H264E_clip_scenecut_time(H264E_clip_t *c, double *kernel_ms, long long *frames)
{
    if (!c) return -1;
    if (kernel_ms) *kernel_ms = c->sc_kernel_ms;
    if (frames) *frames = c->sc_frames;
    return 0;
}

/* ---- a QP per frame, and the lookahead controller that writes one (include/h264e_mi355x.h has the definitions) */

/* what both calls refuse: the reference's own controller, GOP shards, a clip that has moved */
static int clip_qp_mode_refused(const H264E_clip_t *c, const char *who)
{
    if (c->next) { snprintf(g_host_err, sizeof(g_host_err), "%s: only at frame 0 (after open or rewind), not at frame %d", who, c->next); return -1; }
    if (c->par.kbps > 0) { snprintf(g_host_err, sizeof(g_host_err), "%s: not with kbps = %d (the reference's rate control chooses the QPs)", who, c->par.kbps); return -1; }
    if (c->rc_on) { snprintf(g_host_err, sizeof(g_host_err), "%s: not with qp = 0 (the reference's rate control chooses the QPs)", who); return -1; }
    if (c->par.keep_records) { snprintf(g_host_err, sizeof(g_host_err), "%s: not with keep_records = %d (GOP shards)", who, c->par.keep_records); return -1; }
    return 0;
}

static int clip_qp_arrays(H264E_clip_t *c)
{
    if (!c->qp_sched) c->qp_sched = (uint8_t *)calloc((size_t)c->nframes, 1);
    if (!c->qp_sched) { snprintf(g_host_err, sizeof(g_host_err), "out of host memory"); return -1; }
    return 0;
}

int H264E_clip_set_qp_schedule(H264E_clip_t *c, const uint8_t *qp, int n)
{
    int i;
    g_host_err[0] = 0;
    if (!c || n < 0 || (n && !qp)) { snprintf(g_host_err, sizeof(g_host_err), "set_qp_schedule: bad argument"); return -1; }
    if (clip_qp_mode_refused(c, "set_qp_schedule")) return -1;
    if (!n) { c->qp_explicit = 0; return 0; }
    if (c->la_kbps) { snprintf(g_host_err, sizeof(g_host_err), "set_qp_schedule: not together with the lookahead controller (%d kbps)", c->la_kbps); return -1; }
    if (n != c->nframes) { snprintf(g_host_err, sizeof(g_host_err), "set_qp_schedule: %d values for a clip of %d frames", n, c->nframes); return -1; }
    for (i = 0; i < n; i++)
        if (qp[i] < 10 || qp[i] > 51) { snprintf(g_host_err, sizeof(g_host_err), "set_qp_schedule: QP %d of frame %d is outside 10..51", qp[i], i); return -1; }
    if (clip_qp_arrays(c)) return -1;
    memcpy(c->qp_sched, qp, (size_t)n);
    c->qp_explicit = 1;
    return 0;
}

#define LOOKAHEAD_WINDOW_DEFAULT 32
#define LOOKAHEAD_QP_STEP 6             /* a window's QP is within this of the window's before it */
#define LOOKAHEAD_K_MAX ((uint64_t)1 << 40)
#define LOOKAHEAD_BITS_MAX ((uint64_t)1 << 50)

/* the host's cost records, for the controller or for the cost pass run for its motion field alone (H264E_clip_set_denoise_motion) */
static int clip_la_arrays(H264E_clip_t *c)
{
    if (c->la_rec) return 0;
    c->la_rec = (uint64_t *)calloc((size_t)c->nframes*3, sizeof(uint64_t));
    c->la_bits = (int *)calloc((size_t)c->nframes, sizeof(int));
    if (!c->la_rec || !c->la_bits)
    {
        free(c->la_rec); free(c->la_bits); c->la_rec = NULL; c->la_bits = NULL;
        snprintf(g_host_err, sizeof(g_host_err), "out of host memory");
        return -1;
    }
    return 0;
}

int H264E_clip_set_lookahead(H264E_clip_t *c, int kbps, int window, int qp_min, int qp_max)
{
    g_host_err[0] = 0;
    if (!c || kbps < 0 || window < 0) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead: bad argument"); return -1; }
    if (clip_qp_mode_refused(c, "set_lookahead")) return -1;
    if (!kbps && c->la_tree) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead: kbps 0 while the cost tree (strength %d) offsets the controller's QPs: H264E_clip_set_lookahead_tree(clip, 0, 0) first", c->la_tree); return -1; }
    if (!kbps) { c->la_kbps = 0; return 0; }
    if (c->qp_explicit) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead: not together with an explicit QP schedule"); return -1; }
    if (c->par.width < 16 || c->par.height < 16) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead: pictures below 16x16 have no cost block (%dx%d)", c->par.width, c->par.height); return -1; }
    if (!qp_min) qp_min = 10;
    if (!qp_max) qp_max = 50;
    if (qp_min < 10 || qp_max > 51 || qp_min > qp_max) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead: QP range %d..%d is not inside 10..51", qp_min, qp_max); return -1; }
    if (!window) window = imin(LOOKAHEAD_WINDOW_DEFAULT, imin(c->resident, c->ring - 1));
    if (c->resident < c->nframes && window > c->resident) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead: a window of %d frames does not fit the input ring (%d resident frames)", window, c->resident); return -1; }
    if (window > c->ring - 1) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead: a window of %d frames does not fit one launch (%d slots)", window, c->ring - 1); return -1; }
    if (c->la_tree && c->resident < c->nframes && window + c->la_ahead > c->resident) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead: a window of %d frames and the cost tree's %d ahead do not fit the input ring (%d resident frames)", window, c->la_ahead, c->resident); return -1; }
    if (clip_qp_arrays(c) || clip_la_arrays(c)) return -1;
    c->la_kbps = kbps; c->la_window = window; c->la_qmin = qp_min; c->la_qmax = qp_max;
    return 0;
}

int H264E_clip_read_lookahead(H264E_clip_t *c, int first, int n, uint64_t *intra, uint64_t *inter, int *intra_blocks, uint8_t *qp)
{
    int i;
    g_host_err[0] = 0;
    if (!c || first < 0 || n < 0) { snprintf(g_host_err, sizeof(g_host_err), "read_lookahead: bad argument"); return -1; }
    if (intra || inter || intra_blocks)
    {
        const int have = c->la_rec ? c->la.done : 0;
        if (first + n > have) { snprintf(g_host_err, sizeof(g_host_err), "read_lookahead: frames %d..%d have not been analysed (%d have)", first, first + n - 1, have); return -1; }
    }
    if (qp)
    {
        const int have = c->qp_explicit ? c->nframes : c->la_kbps ? imin(c->la_planned*c->la_window, c->nframes) : 0;
        if (first + n > have) { snprintf(g_host_err, sizeof(g_host_err), "read_lookahead: frames %d..%d have no QP yet (%d have)", first, first + n - 1, have); return -1; }
    }
    for (i = 0; i < n; i++)
    {
        if (intra) intra[i] = c->la_rec[3*(size_t)(first + i)];
        if (inter) inter[i] = c->la_rec[3*(size_t)(first + i) + 1];
        if (intra_blocks) intra_blocks[i] = (int)c->la_rec[3*(size_t)(first + i) + 2];
        if (qp) qp[i] = c->qp_sched[first + i];
    }
    return 0;
}

int H264E_clip_set_lookahead_search(H264E_clip_t *c, int range)
{
    g_host_err[0] = 0;
    if (!c) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead_search: bad argument"); return -1; }
    if (range < 0 || range > 8) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead_search: range %d is outside 0..8", range); return -1; }
    if (c->next) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead_search: only at frame 0 (after open or rewind), not at frame %d", c->next); return -1; }
    if (c->par.keep_records) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead_search: not with keep_records = %d (GOP shards)", c->par.keep_records); return -1; }
    if (!range && c->den_motion) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead_search: range 0 while the motion-compensated denoiser (mode %d) reads the motion field: H264E_clip_set_denoise_motion(clip, 0) first", c->den_motion); return -1; }
    if (!range && c->la_tree) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead_search: range 0 while the cost tree (strength %d) reads the motion field: H264E_clip_set_lookahead_tree(clip, 0, 0) first", c->la_tree); return -1; }
    if (range != c->la_search && c->la_any)
    {
        snprintf(g_host_err, sizeof(g_host_err), "set_lookahead_search: range %d after frames have been analysed with range %d (their records cannot be made again)", range, c->la_search);
        return -1;
    }
    c->la_search = range;
    c->la_k[0] = range ? LOOKAHEAD_K0_SEARCH : LOOKAHEAD_K0_P;      /* (the clip stands at frame 0: no window has been planned) */
    return 0;
}

int H264E_clip_read_lookahead_motion(H264E_clip_t *c, int frame, void *dst, int *nbx, int *nby)
{
    g_host_err[0] = 0;
    if (!c) { snprintf(g_host_err, sizeof(g_host_err), "read_lookahead_motion: bad argument"); return -1; }
    if (nbx) *nbx = (c->par.width >> 1) >> 3;
    if (nby) *nby = (c->par.height >> 1) >> 3;
    if (!dst) { snprintf(g_host_err, sizeof(g_host_err), "read_lookahead_motion: bad argument"); return -1; }
    if (!c->la_search) { snprintf(g_host_err, sizeof(g_host_err), "read_lookahead_motion: the search is off (H264E_clip_set_lookahead_search), no frame has a motion field"); return -1; }
    if (!clip_pass_resident(&c->la, frame, "read_lookahead_motion", "motion field")) return -1;
    return h264e_hip_lookahead_read_field(c->pool, frame, dst);
}

/* diagnostic (tools/lookahead_probe.py): HIP-event time of the cost pass' kernel launches since open, and the frames they analysed */
int H264E_clip_lookahead_time(H264E_clip_t *c, double *kernel_ms, long long *frames)
{
    if (!c) return -1;
    if (kernel_ms) *kernel_ms = c->la_kernel_ms;
    if (frames) *frames = c->la_frames;
    return 0;
}

/* ---- the cost tree over the motion field (include/h264e_mi355x.h, enc_lookahead_tree.h): per-frame QP offsets inside a window */

int H264E_clip_set_lookahead_tree(H264E_clip_t *c, int strength, int ahead)
{
    g_host_err[0] = 0;
    if (!c) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead_tree: bad argument"); return -1; }
    if (strength < 0 || strength > 16) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead_tree: strength %d is outside 0..16", strength); return -1; }
    if (ahead > 255) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead_tree: ahead %d is outside 0..255 (below 0: the default)", ahead); return -1; }
    if (c->next) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead_tree: only at frame 0 (after open or rewind), not at frame %d", c->next); return -1; }
    if (!strength) { c->la_tree = 0; return 0; }
    if (c->par.keep_records) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead_tree: not with keep_records = %d (GOP shards)", c->par.keep_records); return -1; }
    if (!c->la_kbps) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead_tree: the lookahead controller is off (0 kbps): call H264E_clip_set_lookahead first"); return -1; }
    if (!c->la_search) { snprintf(g_host_err, sizeof(g_host_err), "set_lookahead_tree: lookahead search range 0, no frame has a motion field: call H264E_clip_set_lookahead_search first"); return -1; }
    if (ahead < 0) ahead = imin(imax(imin(c->la_window, c->resident - c->la_window), 0), 255);
    if (c->resident < c->nframes && c->la_window + ahead > c->resident)
    {
        snprintf(g_host_err, sizeof(g_host_err), "set_lookahead_tree: a window of %d frames and %d ahead do not fit the input ring (%d resident frames)", c->la_window, ahead, c->resident);
        return -1;
    }
    if (!c->tr_sum)
    {
        c->tr_sum = (uint64_t *)calloc((size_t)c->nframes, sizeof(uint64_t));
        c->tr_delta = (int8_t *)calloc((size_t)c->nframes, 1);
        c->tr_base = (uint8_t *)calloc((size_t)c->nframes, 1);
        c->tr_key = (uint8_t *)calloc((size_t)c->nframes, 1);
        if (!c->tr_sum || !c->tr_delta || !c->tr_base || !c->tr_key)
        {
            free(c->tr_sum); free(c->tr_delta); free(c->tr_base); free(c->tr_key);
            c->tr_sum = NULL; c->tr_delta = NULL; c->tr_base = c->tr_key = NULL;
            snprintf(g_host_err, sizeof(g_host_err), "out of host memory");
            return -1;
        }
    }
    c->la_tree = strength; c->la_ahead = ahead;
    return 0;
}

int H264E_clip_read_lookahead_tree(H264E_clip_t *c, int frame, void *dst, int *nbx, int *nby)
{
    g_host_err[0] = 0;
    if (!c) { snprintf(g_host_err, sizeof(g_host_err), "read_lookahead_tree: bad argument"); return -1; }
    if (nbx) *nbx = (c->par.width >> 1) >> 3;
    if (nby) *nby = (c->par.height >> 1) >> 3;
    if (!dst) { snprintf(g_host_err, sizeof(g_host_err), "read_lookahead_tree: bad argument"); return -1; }
    if (!c->la_tree) { snprintf(g_host_err, sizeof(g_host_err), "read_lookahead_tree: the cost tree is off (H264E_clip_set_lookahead_tree), no frame has a block map"); return -1; }
    if (!clip_pass_resident(&c->tr, frame, "read_lookahead_tree", "block map")) return -1;
    if (h264e_hip_lookahead_read_tree(c->pool, frame, dst)) { g_host_err[0] = 0; return -1; }
    return 0;
}

int H264E_clip_read_lookahead_tree_sums(H264E_clip_t *c, int first, int n, uint64_t *sum, int8_t *delta, uint8_t *base_qp)
{
    int i;
    g_host_err[0] = 0;
    if (!c || first < 0 || n < 0) { snprintf(g_host_err, sizeof(g_host_err), "read_lookahead_tree_sums: bad argument"); return -1; }
    if (!c->la_tree) { snprintf(g_host_err, sizeof(g_host_err), "read_lookahead_tree_sums: the cost tree is off (H264E_clip_set_lookahead_tree), no frame has a sum"); return -1; }
    if (first + n > c->tr.done) { snprintf(g_host_err, sizeof(g_host_err), "read_lookahead_tree_sums: the windows of frames %d..%d have not been planned (%d frames have)", first, first + n - 1, c->tr.done); return -1; }
    for (i = 0; i < n; i++)
    {
        if (sum) sum[i] = c->tr_sum[first + i];
        if (delta) delta[i] = c->tr_delta[first + i];
        if (base_qp) base_qp[i] = c->tr_base[first + i];
    }
    return 0;
}

/* diagnostic (tools/lookahead_probe.py): HIP-event time of the tree's kernel launches since open, and the frame steps they made */
int H264E_clip_lookahead_tree_time(H264E_clip_t *c, double *kernel_ms, long long *steps)
{
    if (!c) return -1;
    if (kernel_ms) *kernel_ms = c->tr_kernel_ms;
    if (steps) *steps = c->tr_steps;
    return 0;
}

/* The motion-compensated temporal denoiser (include/h264e_mi355x.h, enc_mcdenoise.h): a mode of the denoiser.  It shares the plain
 * denoiser's ring, budget check, flag (c->denoise) and pre-pass; den_motion selects the kernel that fills the ring. */
int H264E_clip_set_denoise_motion(H264E_clip_t *c, int mode)
{
    g_host_err[0] = 0;
    if (!c) { snprintf(g_host_err, sizeof(g_host_err), "set_denoise_motion: bad argument"); return -1; }
    if (mode < 0 || mode > 2) { snprintf(g_host_err, sizeof(g_host_err), "set_denoise_motion: mode %d is outside 0..2", mode); return -1; }
    if (c->next) { snprintf(g_host_err, sizeof(g_host_err), "set_denoise_motion: only at frame 0 (after open or rewind), not at frame %d", c->next); return -1; }
    if (!mode)
    {
        if (c->den_motion) c->denoise = c->den_motion = 0;
        return 0;
    }
    if (c->par.keep_records) { snprintf(g_host_err, sizeof(g_host_err), "set_denoise_motion: not with keep_records = %d (GOP shards)", c->par.keep_records); return -1; }
    if (!c->la_search) { snprintf(g_host_err, sizeof(g_host_err), "set_denoise_motion: lookahead search range 0, no frame has a motion field: call H264E_clip_set_lookahead_search first"); return -1; }
    if (c->par.width < 16 || c->par.height < 16) { snprintf(g_host_err, sizeof(g_host_err), "set_denoise_motion: pictures below 16x16 have no block (%dx%d)", c->par.width, c->par.height); return -1; }
    if (c->par.speed >= 2) { snprintf(g_host_err, sizeof(g_host_err), "set_denoise_motion: speed %d: the denoiser runs for speed 0 and 1 only, no frame would be filtered", c->par.speed); return -1; }
    if (clip_la_arrays(c)) return -1;
    if (!c->denoise && clip_denoise_ring(c, "set_denoise_motion")) return -1;
    if (c->den_motion != mode) c->den.done = c->den.ring_lo = 0;       /* pictures of another kernel: made again from the zero state */
    c->denoise = 1; c->den_motion = mode;
    return 0;
}

int H264E_clip_read_denoised(H264E_clip_t *c, int frame, uint8_t *i420)
{
    g_host_err[0] = 0;
    if (!c || !i420) { snprintf(g_host_err, sizeof(g_host_err), "read_denoised: bad argument"); return -1; }
    if (!c->denoise) { snprintf(g_host_err, sizeof(g_host_err), "read_denoised: the denoiser is off (H264E_clip_set_denoise, H264E_clip_set_denoise_motion)"); return -1; }
    if (!clip_pass_resident(&c->den, frame, "read_denoised", "denoised picture")) return -1;
    if (h264e_hip_read_denoised(c->pool, frame % c->resident, i420)) { g_host_err[0] = 0; return -1; }
    return 0;
}

int H264E_clip_read_denoise_motion(H264E_clip_t *c, int frame, void *dst, int *nbx, int *nby)
{
    g_host_err[0] = 0;
    if (!c) { snprintf(g_host_err, sizeof(g_host_err), "read_denoise_motion: bad argument"); return -1; }
    if (nbx) *nbx = (c->par.width >> 1) >> 3;
    if (nby) *nby = (c->par.height >> 1) >> 3;
    if (!dst) { snprintf(g_host_err, sizeof(g_host_err), "read_denoise_motion: bad argument"); return -1; }
    if (!c->den_motion) { snprintf(g_host_err, sizeof(g_host_err), "read_denoise_motion: the motion-compensated denoiser is off (H264E_clip_set_denoise_motion), no frame has vectors"); return -1; }
    if (!clip_pass_resident(&c->den, frame, "read_denoise_motion", "vectors")) return -1;
    if (h264e_hip_mcdenoise_read_vectors(c->pool, frame, dst)) { g_host_err[0] = 0; return -1; }
    return 0;
}

/* diagnostic (tools/mcdenoise_probe.py): HIP-event time of the motion-compensated filter's launches since open, and the frames they filtered */
int H264E_clip_denoise_time(H264E_clip_t *c, double *kernel_ms, long long *frames)
{
    g_host_err[0] = 0;
    if (!c) return -1;
    if (h264e_hip_mcdenoise_time(c->pool, kernel_ms, frames)) return -1;
    return 0;
}

/* ---- the frame passes: what is uploaded and not yet made, in stream order, in front of the launch that first encodes it */

/* the detector, in front of the tasks: the histograms read back, D(f) from consecutive records, and the schedule with the cuts among
 * them -- all before the tasks of the launch that first encodes the frames are built */
static int clip_prepass_scenecut(H264E_clip_t *c, int limit)
{
    const int n = c->scenecut ? clip_pass_pending(c, &c->sc, "scenecut", limit) : 0, a = limit - n;
    float ms = 0;
    int f, b;
    if (n <= 0) return n;
    if (h264e_hip_scenecut_frames(c->pool, a % c->resident, n, c->sc_hist + (size_t)a*64, &ms)) return -1;
    for (f = a; f < limit; f++)
    {
        const uint32_t *h = c->sc_hist + (size_t)f*64;
        uint64_t sum = 0;
        for (b = 0; f && b < 64; b++) sum += h[b] > h[b - 64] ? h[b] - h[b - 64] : h[b - 64] - h[b];
        c->sc_dist[f] = (int)(sum*1024u/(2u*(uint64_t)c->seq.width*(uint64_t)c->seq.height));
    }
    c->sc_kernel_ms += ms; c->sc_frames += n;
    clip_pass_made(&c->sc, a, limit);
    clip_sched_build(c);
    return 0;
}

/* the cost pass, in front of a window's plan (or of the motion-compensated denoiser): the cost records read back */
static int clip_prepass_lookahead(H264E_clip_t *c, int limit)
{
    const int n = clip_pass_pending(c, &c->la, "lookahead", limit), a = limit - n;
    float ms = 0;
    if (n <= 0) return n;
    if (c->la_search ? h264e_hip_lookahead_search_frames(c->pool, a, n, c->la_search, (unsigned long long *)(c->la_rec + 3*(size_t)a), &ms)
                     : h264e_hip_lookahead_frames(c->pool, a, n, (unsigned long long *)(c->la_rec + 3*(size_t)a), &ms)) return -1;
    c->la_kernel_ms += ms; c->la_frames += n;
    c->la_any = 1;
    clip_pass_made(&c->la, a, limit);
    return 0;
}

/* the denoiser, in front of the submit */
static int clip_prepass_denoise(H264E_clip_t *c, int limit)
{
    const int n = c->denoise && c->par.speed < 2 ? clip_pass_pending(c, &c->den, "denoise", limit) : 0, a = limit - n;
    if (n <= 0) return n;
    if (c->den_motion)
    {
        /* the searched cost pass comes first, also with the controller off and constant QP: it then runs for its motion field alone */
        if (clip_prepass_lookahead(c, limit) || h264e_hip_mcdenoise_frames(c->pool, a, n, c->den_motion, a == 0)) return -1;
    }
    else if (h264e_hip_denoise_frames(c->pool, a % c->resident, n, a == 0)) return -1;
    clip_pass_made(&c->den, a, limit);
    return 0;
}

/* the bits the host itself writes for a frame, independent of its QP: start code and NAL header of every slice, and a key frame's
 * parameter sets at their size for pic_init_qp 26 */
static int clip_la_header_bits(const H264E_clip_t *c, int key)
{
    uint8_t ps[128];
    return 40*clip_nslices(c) + (key ? 8*(int)write_sps_pps(&c->seq, 26, ps, NULL, NULL) : 0);
}

static uint64_t clip_la_texture_bits(uint64_t k, uint64_t cost, int q, int key)
{
    const unsigned __int128 v = ((unsigned __int128)k*cost*k_bits_per_mb[key][imin(q, 50) - 10]) >> 24;
    return v > LOOKAHEAD_BITS_MAX ? LOOKAHEAD_BITS_MAX : (uint64_t)v;
}

/* piecewise-linear log2 of (I + S)/I in 1/256 units, 0 for I = 0 (S <= 2^48 and I < 2^40: the shifted sum fits 64 bits) */
static int clip_la_tree_log(uint64_t I, uint64_t S)
{
    uint64_t r;
    int e2 = 0;
    if (!I) return 0;
    r = ((I + S) << 8)/I;
    while ((r >> e2) >= 512) e2++;
    return 256*e2 + (int)((r >> e2) - 256);
}

/* the tree of window [a, b), run over the frames up to its horizon e: S and the offset of the window's frames; the window's block maps
 * take the entries of the frames `entries` in front of them */
static int clip_la_tree_window(H264E_clip_t *c, int a, int b, int e)
{
    float ms = 0;
    int f;
    if (a < imin(c->la.ring_lo, c->la.done) || e > c->la.done)
    {
        snprintf(g_host_err, sizeof(g_host_err), "lookahead tree: frames %d..%d are not all in the cost pass' ring (frames %d..%d are)", a, e - 1, imin(c->la.ring_lo, c->la.done), c->la.done - 1);
        return -1;
    }
    for (f = a; f < e; f++) c->tr_key[f] = c->sched[f].key;
    if (h264e_hip_lookahead_tree_frames(c->pool, a, e - a, c->tr_key + a, (unsigned long long *)(c->tr_sum + a), &ms)) return -1;
    c->tr_kernel_ms += ms; c->tr_steps += e - a;
    for (f = a; f < b; f++)
        c->tr_delta[f] = (int8_t)-imin(LOOKAHEAD_QP_STEP, (c->la_tree*clip_la_tree_log(c->la_rec[3*(size_t)f], c->tr_sum[f]) + 512) >> 10);
    c->tr.ring_lo = imax(imin(c->tr.ring_lo, a), e - c->tr.entries);
    c->tr.done = b;
    return 0;
}

/* window j = frames [j*W, (j + 1)*W): one QP, the smallest whose predicted bits fit the window's budget and the clamped carry -- with the
 * cost tree one BASE QP, every frame at base + its offset, clamped to the QP range */
static int clip_la_plan_window(H264E_clip_t *c, int j)
{
    const int W = c->la_window, a = j*W, b = imin(a + W, c->nframes), dfb = c->la_kbps*1000/8/30;
    const long long T = 8LL*dfb*W, carry = c->la_debt > T/2 ? T/2 : c->la_debt < -(T/2) ? -(T/2) : c->la_debt, Tj = 8LL*dfb*(b - a) + carry;
    const int hk = clip_la_header_bits(c, 1), hp = clip_la_header_bits(c, 0);
    /* the factors were measured at the QP of the window before: the table does not carry them far from it */
    const int tree = c->la_tree, prev = !j ? 0 : tree ? c->tr_base[a - 1] : c->qp_sched[a - 1], qlo = prev ? imax(c->la_qmin, prev - LOOKAHEAD_QP_STEP) : c->la_qmin, qhi = prev ? imin(c->la_qmax, prev + LOOKAHEAD_QP_STEP) : c->la_qmax;
    int q, f;
    if (tree && clip_la_tree_window(c, a, b, imin(b + c->la_ahead, c->nframes))) return -1;
    for (q = qlo; q < qhi; q++)
    {
        long long sum = 0;
        for (f = a; f < b; f++)
        {
            const int key = c->sched[f].key, qf = tree ? imax(c->la_qmin, imin(c->la_qmax, q + c->tr_delta[f])) : q;
            sum += (key ? hk : hp) + (long long)clip_la_texture_bits(c->la_k[key], c->la_rec[3*(size_t)f + (key ? 0 : 1)], qf, key);
        }
        if (sum <= Tj) break;
    }
    for (f = a; f < b; f++) c->qp_sched[f] = (uint8_t)(tree ? imax(c->la_qmin, imin(c->la_qmax, q + c->tr_delta[f])) : q);
    if (tree) memset(c->tr_base + a, q, (size_t)(b - a));
    c->la_planned = j + 1;
    return 0;
}

/* window j has been accepted: what it missed goes into the carry, and the factors become what would have predicted its frames */
static void clip_la_close_window(H264E_clip_t *c, int j)
{
    const int W = c->la_window, a = j*W, b = imin(a + W, c->nframes), dfb = c->la_kbps*1000/8/30;
    const int hk = clip_la_header_bits(c, 1), hp = clip_la_header_bits(c, 0);
    long long actual = 0, num[2] = { 0, 0 };
    unsigned __int128 den[2] = { 0, 0 };
    int present[2] = { 0, 0 }, f, t;
    for (f = a; f < b; f++)
    {
        const int key = c->sched[f].key;
        actual += c->la_bits[f];
        num[key] += c->la_bits[f] - (key ? hk : hp);
        den[key] += (unsigned __int128)c->la_rec[3*(size_t)f + (key ? 0 : 1)]*k_bits_per_mb[key][imin(c->qp_sched[f], 50) - 10];
        present[key] = 1;
    }
    c->la_debt += 8LL*dfb*(b - a) - actual;
    for (t = 0; t < 2; t++)
        if (present[t] && den[t])
        {
            const uint64_t old = c->la_k[t], lo = old/4, hi = old*4 > LOOKAHEAD_K_MAX ? LOOKAHEAD_K_MAX : old*4;
            const unsigned __int128 kn = ((unsigned __int128)(num[t] > 0 ? num[t] : 0) << 24)/den[t];
            uint64_t k = kn > hi ? hi : (uint64_t)kn;
            if (k < lo) k = lo;
            c->la_k[t] = k ? k : 1;
        }
    c->la_closed = j + 1;
}

int H264E_clip_stamps(H264E_clip_t *c, unsigned long long *dst) { return c ? h264e_hip_stamps_read(c->pool, dst, 1) : -1; }

/* ---- H264E_clip_encode: launches until the uploaded frames are encoded or the caller's buffer is full; every launch is
 * plan -> pre-pass -> submit -> consume -> settle -> adapt */

#define CLIP_RC_DEPTH_MAX 8     /* rate control: frames per launch, at most (H264E_RC_DEPTH) */
#define CLIP_HEDGE_MAX 32       /* ... and hedge leaves */

/* what a consumed frame means for its launch; the stops in the words of the H264E_DEBUG line */
typedef enum
{
    CLIP_GO_ON,                 /* accepted: on to the chain's next frame, if there is one */
    CLIP_TAKE_LEAF,             /* accepted, and the frame behind it got another QP than the exact one: the leaf that has it comes next */
    CLIP_STOP_LEAF_LOST, CLIP_STOP_MISSPEC, CLIP_STOP_QP_MISS, CLIP_STOP_QP_LEAF, CLIP_STOP_FULL,
    CLIP_RELAUNCH,              /* a bounded wait expired on the device: the frames accepted so far stand, the others are launched again */
    CLIP_ERROR
} clip_step_t;
static const char *const k_clip_ended_by[CLIP_ERROR] = {
    [CLIP_GO_ON] = "all frames delivered",
    [CLIP_STOP_LEAF_LOST] = "the hedge leaf with the exact QP did not complete (its own mv_clusters validation, or stopped)",
    [CLIP_STOP_MISSPEC] = "mv_clusters mis-speculation",
    [CLIP_STOP_QP_MISS] = "QP miss, no hedge leaf with the exact QP",
    [CLIP_STOP_QP_LEAF] = "QP miss covered by a hedge leaf (nothing behind a leaf)",
    [CLIP_STOP_FULL] = "output buffer full",
    [CLIP_RELAUNCH] = "all frames delivered" };     /* (the line has always said so: the expired wait is in the error text and in spin_relaunches) */

/* one H264E_clip_encode call: what it was given, the constants it derives from the clip's parameters, what it keeps from launch to launch */
typedef struct
{
    uint8_t *out; size_t cap, pos;
    int *frame_bytes;                       /* [frame - first], or NULL */
    int first;                              /* the call's first frame */
    int nslices, no_deblock, idr_state;
    /* frame-level rate control (encode_app --kbps, minih264e_test.c:596-600: desired_frame_bytes = kbps*1000/8/30, QP 10..50):
     * a frame's QP is a function of the byte count of the frame before it (h264-lab.h:5924-6141) and moves almost every
     * frame: the frames behind the first one of a launch run on a speculated QP (clip_plan_launch), the controller on the host */
    int desired_frame_bytes, qp_min, qp_max, pic_init_qp;
    uint16_t qdat_i[2][42], qdat_p[2][42];  /* constant QP: the quantizer tables of every I / P frame */
    int spin_retries;                       /* launches in a row that a bounded wait ended before a single frame got through */
    long long far_reads;                    /* of the frames the current launch delivered (0 when it delivered none) */
    int debug;                              /* H264E_DEBUG: one line per launch and one per delivered frame */
    H264E_clip_stats_t stats;
} clip_call_t;

/* one launch: the plan -- frames n .. n + F - 1 are tasks 0 .. F - 1 (the chain), task F + k is hedge leaf k -- and how it went */
typedef struct
{
    int n, limit;                           /* first frame; frames [n, limit) were uploaded when the launch was planned */
    int F, nh;                              /* frames in the chain, hedge leaves */
    int qp_task[CLIP_RC_DEPTH_MAX];         /* rate control: the QP the chain's frames were given */
    int hedge_level[CLIP_HEDGE_MAX], hedge_qp[CLIP_HEDGE_MAX];      /* the chain index of the frame a leaf encodes, and its QP */
    int kept_frames, kept_rows;             /* key frames that start below row 0 on what the stopped launch in front left of them, and those rows */
    int led_frames, led_rows, led_last;     /* key frames whose rows the launch dispatched first (h264e_hip_last_lead), their rows, the last such task (-1: none) */
    int after_stop;                         /* follows a launch that was stopped (mis-speculation, rate-control miss): its first frame pays the refill */
    double t_submit, t_first, t_last;       /* submit; first and last frame consumed */
    double t_prev;                          /* ... and the one in front of the last */
    int nvalid;                             /* frames accepted */
    int leaf;                               /* CLIP_TAKE_LEAF: the task to take */
    int moved_from, moved_to;               /* an accepted leaf's slot, and the slot its frame number owns */
    clip_step_t step;                       /* of the last frame consumed: what ended the launch */
} clip_launch_t;

/* a failure between submit and sync gives the device's launch lock back; the statistics so far go out either way */
static int clip_end(H264E_clip_t *c, const clip_call_t *x, H264E_clip_stats_t *st, int rc)
{
    if (rc) { h264e_hip_release(c->pool); c->nkeep = 0; }
    if (st) *st = x->stats;
    return rc;
}

/* stop the running launch and wait until it is gone, whatever either call answers: the failure has been reported */
static clip_step_t clip_abort_launch(H264E_clip_t *c)
{
    (void)h264e_hip_stream_abort(c->pool);
    (void)h264e_hip_sync(c->pool);
    return CLIP_ERROR;
}

/* a task's QP: quantizer tables and slice header.  frame_num restarts at every key frame; idr_pic_id toggles with every key frame
 * (h264-lab.h:6774-6775) */
/* a QP per frame is in force (the caller's schedule or the lookahead controller's) */
static int clip_qp_per_frame(const H264E_clip_t *c) { return c->qp_explicit || c->la_kbps; }

/* pic_init_qp of the parameter sets in force at frame f: one value per call, or -- with a QP per frame -- a property of the last key
 * frame: clamp(30, qp_min, qp_max) with qp_min = qp_max = that frame's QP (h264-lab.h:6766-6773) */
static int clip_pic_init_qp(const H264E_clip_t *c, const clip_call_t *x, int f)
{
    if (!clip_qp_per_frame(c)) return x->pic_init_qp;
    while (f > 0 && !c->sched[f].key) f--;
    return c->qp_sched[f];
}

static void clip_task_set_qp(const H264E_clip_t *c, const clip_call_t *x, h264e_hip_task_t *t, int f, int qp)
{
    const struct clip_sched *s = c->sched + f;
    t->qp = qp;
    if (c->rc_on || clip_qp_per_frame(c)) build_qdat(t->qdat, qp, !s->key);
    else memcpy(t->qdat, s->key ? x->qdat_i : x->qdat_p, sizeof(t->qdat));
    slice_header_bits(&c->seq, s->key, s->frame_num, x->idr_state ^ s->idr, qp, clip_pic_init_qp(c, x, f), x->no_deblock, x->nslices, &t->hdr_nal, &t->hdr_bits, &t->hdr_nbits);
}

/* the launch that starts at frame l->n: how many frames, and their tasks */
static void clip_plan_launch(H264E_clip_t *c, const clip_call_t *x, clip_launch_t *l)
{
    const struct clip_sched *sched = c->sched;
    const int nmb = c->seq.nmb, K = c->ring, n = l->n, rc_on = c->rc_on;
    /* rate control: frame n+1's QP is a function of frame n's size (h264-lab.h:5924-6141), so the frames behind the first one of
     * a launch run on a SPECULATED QP: the controller is run ahead on predicted sizes (the last frame of the same kind); when a
     * frame's real size is in, the exact QP of the next one is computed and compared with what it was given -- a mismatch stops
     * the launch there (measured hit rates of the one-ahead guess: 15-66 %) */
    const int rc_depth = imax(1, imin(CLIP_RC_DEPTH_MAX, getenv("H264E_RC_DEPTH") ? atoi(getenv("H264E_RC_DEPTH")) : (nmb >= 60000 ? 3 : 6)));     /* measured optima: 8K 3, below 6 */
    const int F = rc_on ? imax(1, imin(imin(K - 1, rc_depth), l->limit - n)) : imin(imin(K - 1, c->launch_frames), l->limit - n);
    h264e_hip_task_t *tasks = c->tasks;
    int32_t (*used)[2] = c->used;
    rc_t rc_ahead;
    int i, qp = c->rc_qp;
    memset(tasks, 0, sizeof(*tasks)*(size_t)K);
    if (rc_on && c->rc_frame != n)
    {
        qp = c->rc_qp = rc_frame_start(&c->rcs, c->par.gop, nmb, c->par.vbv_size_bytes, x->desired_frame_bytes, x->qp_min, x->qp_max, sched[n].key);
        c->rc_frame = n;
    }
    rc_ahead = c->rcs;
    for (i = 0; i < F; i++)
    {
        h264e_hip_task_t *t = tasks + i;
        const int f = n + i, key = sched[f].key;
        if (rc_on)
        {
            if (i > 0)
            {
                /* the controller, run ahead: the frame in front is predicted to weigh what the last frame of its kind did */
                const int pkey = sched[f - 1].key, pred = c->rc_last_bytes[pkey] > 0 ? c->rc_last_bytes[pkey] : x->desired_frame_bytes;
                rc_frame_end(&rc_ahead, nmb, c->par.vbv_size_bytes, x->desired_frame_bytes, pred, pkey, 0);
                qp = rc_frame_start(&rc_ahead, c->par.gop, nmb, c->par.vbv_size_bytes, x->desired_frame_bytes, x->qp_min, x->qp_max, key);
            }
            l->qp_task[i] = qp;
        } else if (clip_qp_per_frame(c)) qp = c->qp_sched[f];
        t->active = 1; t->frame_index = f % c->resident;
        t->slice_type = key ? SLICE_I : SLICE_P;
        t->speed = c->par.speed;
        t->nslices = x->nslices;
        clip_task_set_qp(c, x, t, f, qp);
        t->stream_mode = 1; t->slot = f % K;
        t->ref_slot = key ? -1 : (f - 1) % K;
        t->ref_in_flight = !key && i > 0;
        /* frame 0 of the launch gets the exact state; the frames behind it the best prediction of what it leaves */
        t->mv_clusters[0] = used[i][0] = (i && c->have_after) ? c->after[0] : c->state[0];
        t->mv_clusters[1] = used[i][1] = (i && c->have_after) ? c->after[1] : c->state[1];
        /* validation on the device: the frame's finalizer walks its records exactly (task 0 from the exact state, the others from
         * the verdict in front of them) and stops the launch itself when a macroblock consumed the wrong candidates */
        t->walk_on_device = 1;
        t->exact_state[0] = c->state[0]; t->exact_state[1] = c->state[1];
        t->mv_clusters_per_mb = NULL;
        t->traj_from_device = (i == 0) && c->first_dev;
        t->first_row = (i == 0 && c->first_dev) ? c->first_row : 0;
        t->narrow_window = c->narrow;
        t->denoised = c->denoise && c->par.speed < 2;
    }
    /* Hedges (rate control): the speculated QP of a frame is usually off by one or two when it is off, so every frame behind the
     * first one is ALSO encoded with the neighbouring QPs, as leaves in spare slots (same reference, same mv_clusters
     * speculation; the chip is nearly empty in this mode).  When the chain breaks at a frame, the leaf with the exact QP -- if
     * there is one -- is the frame; its picture then moves to the slot the frame number owns and the launch ends there. */
    l->nh = 0;
    if (rc_on && F > 1)
    {
        static const int dq[4] = { -1, 1, -2, 2 };
        const int rc_hedge = imax(0, imin(4, getenv("H264E_RC_HEDGE") ? atoi(getenv("H264E_RC_HEDGE")) : (nmb >= 60000 ? 0 : nmb >= 20000 ? 2 : 4)));      /* measured: 8K is bound by the resident workgroups, leaves only cost there */
        int k, a;
        for (k = 1; k < F; k++)
            for (a = 0; a < rc_hedge; a++)
            {
                const int q = l->qp_task[k] + dq[a], j = F + l->nh;
                h264e_hip_task_t *t = tasks + j;
                if (q < x->qp_min || q > x->qp_max || l->nh >= CLIP_HEDGE_MAX || j + 2 >= K) continue;
                *t = tasks[k];
                clip_task_set_qp(c, x, t, n + k, q);
                t->slot = (n + j) % K;              /* a slot no frame of this launch owns */
                t->walk_parent = k;                 /* = index of the chain's frame in front of it, + 1 */
                t->walk_quiet = 1;                  /* its own validation failing stops nobody else */
                used[j][0] = used[k][0]; used[j][1] = used[k][1];
                l->hedge_level[l->nh] = k; l->hedge_qp[l->nh] = q; l->nh++;
            }
    }
    if (l->nh) c->recon_floor = n;              /* the leaves' slots held the pictures of frames n - K + F .. : gone now */
    /* Key frames the stopped launch in front left in their slots: the same frame lands in the same slot (f % K), and with the same QP,
     * slices, speed and input it makes the same rows again, so it starts at the first row that was not complete -- below the last row:
     * only its finalizer runs.  Not next to hedge leaves: their spare slots are other frames' slots.  What is not used now is dropped:
     * the launch resets every counter. */
    l->kept_frames = l->kept_rows = 0;
    for (i = 0; i < c->nkeep && !l->nh; i++)
    {
        const struct clip_keep *k = c->keep + i;
        const int ti = k->frame - n;
        h264e_hip_task_t *t = tasks + imax(imin(ti, F - 1), 0);
        if (ti < 0 || ti >= F || !sched[k->frame].key || t->traj_from_device) continue;
        if (t->qp != k->qp || t->nslices != k->nslices || t->speed != k->speed || t->denoised != k->denoised) continue;
        t->first_row = k->rows;
        l->kept_frames++; l->kept_rows += k->rows;
    }
    c->nkeep = 0;
    l->F = F;
    l->after_stop = c->stopped_before;
    c->have_after = 0;
    l->t_first = l->t_last = l->t_prev = 0;
    l->nvalid = 0; l->leaf = l->moved_from = l->moved_to = -1;
    l->step = CLIP_GO_ON;
}

/* wait for a job of the running launch, as h264e_hip_stream_done: 1 finished (r filled), 2 aborted, < 0 failed; 0: the launch ended
 * without finishing it */
static int clip_wait_frame(H264E_clip_t *c, int slot, h264e_hip_result_t *r)
{
    int dn, idle = 0;
    memset(r, 0, sizeof(*r));
    while ((dn = h264e_hip_stream_done(c->pool, slot, r)) == 0)
    {
        if (!h264e_hip_busy(c->pool) && ++idle > 2) break;      /* the launch ended without finishing this job */
        if (c->idle_hook) c->idle_hook(c->idle_token);
        sched_yield();
    }
    return dn ? dn : h264e_hip_stream_done(c->pool, slot, r);
}

/* task ti did not finish (dn != 1): why, and what becomes of the launch */
static clip_step_t clip_frame_stopped(H264E_clip_t *c, clip_call_t *x, const clip_launch_t *l, int ti, int dn, const h264e_hip_result_t *r)
{
    if (dn < 0) return CLIP_ERROR;
    /* a leaf did not make it (its own mv_clusters validation failed, or the launch was stopped): the frame is simply encoded in the
     * next launch */
    if (ti >= l->F) return h264e_hip_stream_abort(c->pool) ? CLIP_ERROR : CLIP_STOP_LEAF_LOST;
    if (dn == 2 && r->walk_status == 2)
    {
        /* the device's exact walk found a macroblock of this frame that consumed other rounded candidates than the exact
         * ones and stopped the launch.  Every macroblock before first_bad consumed the right ones: its row and
         * the rows above are bit-identical in the next encode and are kept; the frame goes again from that row with the
         * walked per-macroblock trajectory (it stays on the device), the frames behind it with the walk's end state */
        c->first_row = r->first_bad/c->seq.nmbx;
        c->first_dev = 1;
        c->after[0] = r->state_out[0]; c->after[1] = r->state_out[1]; c->have_after = 1;
        x->stats.reencoded_gops++;          /* counts relaunches */
        return CLIP_STOP_MISSPEC;
    }
    /* The frame did not complete and nobody asked it to stop.  When the kernel reports that a bounded wait expired -- workgroups
     * starved of wave slots, e.g. by another process' launch on the same device -- nothing wrong was returned: every frame
     * accepted so far stands, and the unfinished ones are simply launched again (a fresh launch in this process).  Anything
     * else, and a wait that keeps expiring without a single frame getting through, is an error. */
    if (h264e_hip_sync(c->pool) && strstr(h264e_hip_last_error(), "bounded spin expired") && x->spin_retries < 3)
    {
        x->spin_retries++;
        x->stats.spin_relaunches++;
        return CLIP_RELAUNCH;
    }
    if (!g_host_err[0] && !h264e_hip_last_error()[0]) snprintf(g_host_err, sizeof(g_host_err), "frame %d did not complete", l->n + ti);
    return CLIP_ERROR;
}

/* task ti finished: its NALs into the caller's buffer, the exact rate controller, the records, the stream state behind the frame */
static clip_step_t clip_take_frame(H264E_clip_t *c, clip_call_t *x, clip_launch_t *l, int ti, const h264e_hip_result_t *r)
{
    const int nmb = c->seq.nmb, F = l->F, is_hedge = ti >= F;
    const int f = l->n + (is_hedge ? l->hedge_level[ti - F] : ti), key = c->sched[f].key, slot = c->tasks[ti].slot, per_mb = (ti == 0 && c->first_dev);
    const size_t start = x->pos, need = (key ? 64 : 0) + r->nbytes;       /* 64: the parameter sets stay below it with a VUI too (write_sps_pps) */
    const uint8_t *nals;
    const double t0 = now_ms();
    size_t w;
    int rc_miss = 0;
    l->leaf = -1;
    l->t_prev = l->t_last; l->t_last = t0;
    if (ti == 0) l->t_first = t0;
    if (r->overflow) { snprintf(g_host_err, sizeof(g_host_err), "bit buffer overflow (frame %d)", f); return clip_abort_launch(c); }
    /* the frame as the kernel exported it: complete NALs (start codes and emulation prevention done on the device) */
    if (r->in_device && c->big_cap < r->nbytes) { free(c->big); c->big_cap = (size_t)r->nbytes*2; c->big = (uint8_t *)malloc(c->big_cap); }
    nals = frame_nals(c->pool, slot, r, c->big, c->big_cap);
    if (!nals) { c->big_cap = 0; return clip_abort_launch(c); }
    /* the caller's buffer is full: stop here, the stream continues with this frame in the next call */
    if (x->pos + need > x->cap) return h264e_hip_stream_abort(c->pool) ? CLIP_ERROR : CLIP_STOP_FULL;
    if (key) x->pos += write_sps_pps(&c->seq, clip_pic_init_qp(c, x, f), x->out + x->pos, NULL, NULL);
    w = emit_slices(x->out + x->pos, x->cap - x->pos, nals, r, NULL, NULL);
    if (!w) { snprintf(g_host_err, sizeof(g_host_err), "malformed frame export"); return clip_abort_launch(c); }
    x->pos += w;
    if (x->frame_bytes) x->frame_bytes[f - x->first] = (int)(x->pos - start);
    if (c->la_kbps) c->la_bits[f] = 8*(int)(x->pos - start);
    if (c->rc_on)
    {
        rc_frame_end(&c->rcs, nmb, c->par.vbv_size_bytes, x->desired_frame_bytes, (int)(x->pos - start), key, r->all_skipped);
        c->rc_last_bytes[key] = (int)(x->pos - start);
        /* (scene-cut detection: a frame that has not been analysed has no kind yet -- the launch that analyses it runs its
         * rc_frame_start, on the same controller state) */
        if (f + 1 < c->nframes && (!c->scenecut || f + 1 < c->sc.done))
        {
            /* the exact QP of the next frame; a frame of this launch that was given another one is stopped */
            const int qp = c->rc_qp = rc_frame_start(&c->rcs, c->par.gop, nmb, c->par.vbv_size_bytes, x->desired_frame_bytes, x->qp_min, x->qp_max, c->sched[f + 1].key);
            c->rc_frame = f + 1;
            if (is_hedge) rc_miss = 1;                  /* a leaf has nothing behind it */
            else if (ti + 1 < F && l->qp_task[ti + 1] != qp)
            {
                int hh;
                rc_miss = 1;
                for (hh = 0; hh < l->nh; hh++) if (l->hedge_level[hh] == ti + 1 && l->hedge_qp[hh] == qp) { l->leaf = F + hh; rc_miss = 0; }
            }
        } else if (is_hedge) rc_miss = 1;
    }
    if (c->rec_store)
    {
        /* what this accepted frame consumed: records + the candidates it was given (H264E_clip_revalidate) */
        const size_t rb = sizeof(h264e_hip_mbrec_t)*(size_t)nmb;
        if (!c->rec_store[f]) c->rec_store[f] = (h264e_hip_mbrec_t *)malloc(rb);
        if (!c->rec_store[f]) return CLIP_ERROR;
        memcpy(c->rec_store[f], h264e_hip_stream_mbrec(c->pool, slot), rb);
        c->used_store[f][0] = c->used[ti][0]; c->used_store[f][1] = c->used[ti][1];
        free(c->permb_store[f]); c->permb_store[f] = NULL;
        if (per_mb)
        {
            c->permb_store[f] = (int32_t *)malloc(sizeof(int32_t)*2*(size_t)nmb);
            if (!c->permb_store[f] || h264e_hip_stream_fetch_traj(c->pool, slot, 1, c->permb_store[f])) return CLIP_ERROR;
        }
    }
    c->state[0] = r->state_out[0]; c->state[1] = r->state_out[1];      /* exact state behind this frame (device walk), committed now that the frame is accepted */
    if (ti == 0) c->first_dev = 0;
    x->stats.assemble_ms += now_ms() - t0;
    l->nvalid++;
    x->far_reads += r->far_reads;           /* delivered frames only: what clip_adapt divides by */
    if (x->debug) fprintf(stderr, "clip frame %d: %d far reads\n", f, r->far_reads);
    /* a key frame behind the launch's first frame: when it came, next to when the frame in front of it did (a key frame that the launch
     * encodes from row 0 is what the stream waits for after a relaunch) */
    if (x->debug && key && ti > 0 && !is_hedge)
        fprintf(stderr, "clip key frame %d (task %d, first row %d): taken %.2f ms after the submit, %.2f ms after frame %d\n", f, ti, c->tasks[ti].first_row, t0 - l->t_submit, t0 - l->t_prev, f - 1);
    if (is_hedge) { l->moved_from = slot; l->moved_to = f % c->ring; }
    if (rc_miss)
    {
        if (h264e_hip_stream_abort(c->pool)) return CLIP_ERROR;
        x->stats.reencoded_gops++;
        return is_hedge ? CLIP_STOP_QP_LEAF : CLIP_STOP_QP_MISS;
    }
    return l->leaf >= 0 ? CLIP_TAKE_LEAF : CLIP_GO_ON;
}

/* The launch was stopped cleanly -- a mis-speculation, a full output buffer, a QP miss without hedge leaves -- and has drained: what is
 * left of the key frames it did not deliver.  A frame whose done word is up is whole (h264e_hip_stream_rows_complete); of the others a row
 * is complete when its counter says so; the counters are read with one small copy per
 * key frame, after the drain, when no row moves any more (the finalizer of a stopped job could report the count instead, but it leaves as
 * soon as the verdict in front of its frame is void, at whatever row it follows then, and would under-count; and it would be a change to the
 * kernel; the copy costs some 20 us next to a relaunch of 8 ms).  Key frames are asked in stream order until one behind the last LED
 * one has no complete row: the frames behind it were dispatched later still (the led ones -- the nearest key frames, h264e_pool.h
 * lead_jobs -- started together at the front of the order, so one of them without a row says nothing about the next).
 * The launch's chain owns F different slots, so no other job of it wrote a key frame's slot. */
static int clip_keep_collect(H264E_clip_t *c, const clip_launch_t *l)
{
    int ti;
    c->nkeep = 0;
    if (!c->keep_on || l->nh || (l->step != CLIP_STOP_MISSPEC && l->step != CLIP_STOP_FULL && l->step != CLIP_STOP_QP_MISS)) return 0;
    for (ti = l->nvalid; ti < l->F && c->nkeep < CLIP_KEEP_MAX; ti++)
    {
        const h264e_hip_task_t *t = c->tasks + ti;
        struct clip_keep *k = c->keep + c->nkeep;
        int rows = 0;
        if (t->slice_type != SLICE_I) continue;
        if (h264e_hip_stream_rows_complete(c->pool, t->slot, &rows)) return -1;
        if (rows <= 0) { if (ti > l->led_last) break; continue; }
        k->frame = l->n + ti; k->rows = rows; k->qp = t->qp; k->nslices = t->nslices; k->speed = t->speed; k->denoised = t->denoised;
        c->nkeep++;
    }
    return 0;
}

/* the launch is over: drained, an accepted leaf's picture in the slot its frame owns, the stream position behind the accepted frames */
static int clip_settle(H264E_clip_t *c, clip_call_t *x, const clip_launch_t *l)
{
    const int K = c->ring, n = l->n, nvalid = l->nvalid;
    if (l->step == CLIP_RELAUNCH) (void)clip_abort_launch(c);       /* (the failure was reported by the sync that found it; the launch is over) */
    else if (h264e_hip_sync(c->pool)) return -1;    /* the launch has drained (immediately after an abort) */
    if (nvalid) x->spin_retries = 0;
    if (clip_keep_collect(c, l)) return -1;
    if (l->moved_from >= 0 && h264e_hip_stream_copy_picture(c->pool, l->moved_from, l->moved_to)) return -1;
    x->stats.encode_ms += now_ms() - l->t_submit;
    /* device-side sums of squared differences of the frames just validated: their pictures are still in their slots */
    if (c->ssd_out && nvalid && h264e_hip_ssd_frames(c->pool, nvalid, n % c->resident, c->resident, n % K, K, c->ssd_out + 3*(size_t)(n - x->first))) return -1;
    if (c->ssim_out && nvalid && h264e_hip_ssim_frames(c->pool, nvalid, n % c->resident, c->resident, n % K, K, c->ssim_out + 3*(size_t)(n - x->first))) return -1;
    c->next = n + nvalid;
    if (l->after_stop && nvalid) { x->stats.relaunches_timed++; x->stats.first_frame_ms_after_relaunch += l->t_first - l->t_submit; }
    c->stopped_before = nvalid < l->F && l->step != CLIP_STOP_FULL;
    return 0;
}

/* what the launch teaches the next one: frames per launch, window geometry */
static void clip_adapt(H264E_clip_t *c, const clip_call_t *x, const clip_launch_t *l)
{
    const int K = c->ring, nvalid = l->nvalid;
    /* frames per launch: back to the pipeline depth after a mis-speculation, twice as many after a clean launch */
    /* (after an event: twice the frames the stopped launch got through, an estimate of the spacing of the events) */
    if (nvalid < l->F && l->step != CLIP_STOP_FULL) c->launch_frames = imin(imax(c->launch_base, 2*nvalid), K - 1);
    else if (nvalid == l->F) c->launch_frames = imin(2*c->launch_frames, K - 1);
    /* Window geometry for the next launch.  More than one macroblock in eight leaving the narrow window over at least 8 frames:
     * the wide one pays -- for a while: such motion is often a transient (a scene cut, an object wrapping around), so the narrow
     * geometry is tried again after wide_hold frames, a spell that doubles every time it fails again. */
    if (c->narrow)
    {
        c->far_acc += x->far_reads; c->far_frames += nvalid;
        if (c->far_frames >= 8)
        {
            if (c->far_acc > (long long)c->far_frames*c->seq.nmb/8)
            {
                c->narrow = 0;
                c->wide_until = c->next + c->wide_hold;
                c->wide_hold = imin(c->wide_hold*2, 960);
            } else if (c->far_frames >= 64) c->wide_hold = 30;
            c->far_acc = 0; c->far_frames = 0;
        }
    } else if (c->narrow_ok && c->next >= c->wide_until) { c->narrow = 1; c->far_acc = 0; c->far_frames = 0; }
}

/* H264E_DEBUG: one line per launch */
static void clip_debug_line(const H264E_clip_t *c, const clip_call_t *x, const clip_launch_t *l)
{
    const double t_end = now_ms();
    const int nvalid = l->nvalid;
    const double t_first = nvalid ? l->t_first : t_end, t_last = nvalid ? l->t_last : t_end;     /* no frame of it was delivered: "first frame after" = when its verdict was in */
    fprintf(stderr, "clip launch %d (first row %d, %s window, %lld far reads): %d frames in flight, %d valid, next %d; first frame after %.2f ms, then %.3f ms/frame, drained %.2f ms after the last, %d key rows kept in %d frames, led %d key frames, %d rows; ended by: %s%s\n",
            x->stats.rounds, c->tasks[0].first_row, c->tasks[0].narrow_window ? "narrow" : "wide", x->far_reads, l->F, nvalid, c->next, t_first - l->t_submit, nvalid > 1 ? (t_last - t_first)/(nvalid - 1 + (nvalid < l->F)) : 0.0, t_end - t_last, l->kept_rows, l->kept_frames, l->led_frames, l->led_rows,
            k_clip_ended_by[l->step], l->nh ? " (+ hedge leaves)" : "");
}

int H264E_clip_encode(H264E_clip_t *c, uint8_t *out, size_t cap, size_t *out_bytes, int *frame_bytes, int profile, H264E_clip_stats_t *st)
{
    clip_call_t x;
    clip_launch_t l;
    memset(&x, 0, sizeof(x));
    g_host_err[0] = 0;
    x.out = out; x.cap = cap; x.frame_bytes = frame_bytes; x.first = c->next;
    x.nslices = clip_nslices(c);
    x.no_deblock = (c->par.speed == 8 || c->par.speed == 10);
    x.idr_state = c->par.first_idr_pic_id_state & 1;
    x.desired_frame_bytes = c->par.kbps > 0 ? c->par.kbps*1000/8/30 : 0;
    x.qp_min = c->rc_on ? 10 : c->par.qp; x.qp_max = c->par.kbps > 0 ? 50 : c->rc_on ? 51 : c->par.qp;     /* qp 0: 10..51, h264-lab.h:6707-6715 */
    x.pic_init_qp = imax(imin(30, x.qp_max), x.qp_min);     /* h264-lab.h:6768-6770 */
    build_qdat(x.qdat_i, c->rc_qp, 0);
    build_qdat(x.qdat_p, c->rc_qp, 1);
    h264e_hip_profile(c->pool, profile);
    x.stats.chains = c->ring - 1;
    x.stats.first_frame = x.first;
    x.debug = getenv("H264E_DEBUG") != NULL;
    l.step = CLIP_GO_ON;

    while (c->next < c->avail && l.step != CLIP_STOP_FULL)
    {
        int ti = 0;
        l.n = c->next; l.limit = c->avail;          /* frames uploaded from the idle hook during this launch join the next one */
        if (clip_prepass_scenecut(c, l.limit)) return clip_end(c, &x, st, -1);
        if (c->la_kbps)
        {
            /* the lookahead controller: window j is planned once, when its first frame is, from the windows up to j - 1 -- and only
             * when all its frames are there; a launch never crosses a window boundary */
            const int j = l.n/c->la_window, wend = imin((j + 1)*c->la_window, c->nframes);
            if (c->la_planned <= j)
            {
                /* (with the cost tree: its frames up to the window's horizon, which the tree starts from) */
                if (c->avail < imin(wend + (c->la_tree ? c->la_ahead : 0), c->nframes)) break;
                if (clip_prepass_lookahead(c, l.limit) || clip_la_plan_window(c, j)) return clip_end(c, &x, st, -1);
            }
            l.limit = wend;
        }
        clip_plan_launch(c, &x, &l);
        x.stats.rounds++;
        x.stats.kept_key_frames += l.kept_frames; x.stats.kept_key_rows += l.kept_rows;
        x.far_reads = 0;
        l.t_submit = now_ms();
        if (clip_prepass_denoise(c, l.limit) || h264e_hip_submit(c->pool, c->tasks)) return clip_end(c, &x, st, -1);
        h264e_hip_last_lead(c->pool, &l.led_frames, &l.led_rows, &l.led_last);
        /* consume the frames in stream order while the launch is still running */
        do
        {
            h264e_hip_result_t r;
            const int dn = clip_wait_frame(c, c->tasks[ti].slot, &r);
            l.step = dn == 1 ? clip_take_frame(c, &x, &l, ti, &r) : clip_frame_stopped(c, &x, &l, ti, dn, &r);
            ti = l.step == CLIP_TAKE_LEAF ? l.leaf : ti + 1;        /* the chain ends here: one more round, for the leaf */
        } while (l.step == CLIP_TAKE_LEAF || (l.step == CLIP_GO_ON && ti < l.F));
        if (l.step == CLIP_ERROR || clip_settle(c, &x, &l)) return clip_end(c, &x, st, -1);
        clip_adapt(c, &x, &l);
        while (c->la_kbps && c->la_closed < c->la_planned && c->next >= imin((c->la_closed + 1)*c->la_window, c->nframes)) clip_la_close_window(c, c->la_closed);
        if (x.debug) clip_debug_line(c, &x, &l);
        if (l.step == CLIP_STOP_FULL && c->next == x.first)
        {
            snprintf(g_host_err, sizeof(g_host_err), "output buffer too small for one frame");
            return clip_end(c, &x, st, -1);
        }
    }
    x.stats.frames = c->next - x.first;
    x.stats.delivered_mbs = (long long)x.stats.frames*c->seq.nmb;
    {
        unsigned long long pm = 0;
        if (!h264e_hip_mb_counter(c->pool, &pm, 1)) x.stats.processed_mbs = (long long)pm;
    }
    x.stats.mv_clusters_out[0] = c->state[0]; x.stats.mv_clusters_out[1] = c->state[1];
    x.stats.next_idr_pic_id_state = c->next ? x.idr_state ^ c->sched[c->next - 1].idr : x.idr_state;
    h264e_hip_profile_read(c->pool, &x.stats.mb_kernel_ms, &x.stats.splice_kernel_ms, &x.stats.kernel_launches);
    if (out_bytes) *out_bytes = x.pos;
    return clip_end(c, &x, st, 0);
}


/* ------------------------------------------------------------------ several clips of one picture size on ONE device at once */

typedef struct
{
    H264E_clip_t *clip; h264e_hip_group_t *group;
    uint8_t *out; size_t cap; size_t *out_bytes; int *frame_bytes; H264E_clip_stats_t *st;
    int rc; char err[256];
} multi_arg_t;

static void *multi_thread(void *p)
{
    multi_arg_t *a = (multi_arg_t *)p;
    a->rc = H264E_clip_encode(a->clip, a->out, a->cap, a->out_bytes, a->frame_bytes, 0, a->st);
    if (a->rc) snprintf(a->err, sizeof(a->err), "%s", H264E_last_error());
    h264e_hip_group_leave(a->group, a->clip->pool);     /* the others no longer wait for this one's launches */
    return NULL;
}

/*
 * A single-slice stream spends most of a pass in pipeline drains and refills (one per mis-speculated mv_clusters state);
 * independent streams fill each other's gaps when their frames share ONE launch (include/h264e_hip.h launch groups): every clip is
 * encoded by its own host thread exactly like H264E_clip_encode does, the device layer merges the threads' launches round by round.
 * Same bytes per clip as H264E_clip_encode.
 */
int H264E_clip_encode_multi(H264E_clip_t **clips, int nclips, uint8_t **out, const size_t *cap, size_t *out_bytes, int **frame_bytes, H264E_clip_stats_t *stats)
{
    multi_arg_t *a;
    pthread_t *th;
    int i, rc = 0, done = 0, saved_base[8] = { 0 };
    g_host_err[0] = 0;
    if (!clips || nclips <= 0 || nclips > 8 || !out || !cap || !out_bytes) { snprintf(g_host_err, sizeof(g_host_err), "clip_encode_multi: bad argument"); return -1; }
    for (i = 0; i < nclips; i++) if (!clips[i]) { snprintf(g_host_err, sizeof(g_host_err), "clip_encode_multi: clip %d is NULL", i); return -1; }
    if (nclips == 1) return H264E_clip_encode(clips[0], out[0], cap[0], &out_bytes[0], frame_bytes ? frame_bytes[0] : NULL, 0, stats);
    a = (multi_arg_t *)calloc((size_t)nclips, sizeof(*a));
    th = (pthread_t *)calloc((size_t)nclips, sizeof(*th));
    if (!a || !th) { free(a); free(th); snprintf(g_host_err, sizeof(g_host_err), "out of host memory"); return -1; }
    /* one launch group per batch: a group holds as many streams of this picture size as one grid can carry safely (h264e_pool.h
     * h264e_hip_group_join: 5 at 1080p, 2 at 4K, 1 at 8K); the clips that do not fit go in the next batch */
    while (done < nclips && !rc)
    {
        h264e_hip_group_t *g = NULL;
        int first = done, n = 0, started = 0;
        if (h264e_hip_group_create(&g, clips[first]->par.device)) { snprintf(g_host_err, sizeof(g_host_err), "clip_encode_multi: %s", h264e_hip_last_error()); rc = -1; break; }
        while (first + n < nclips && !h264e_hip_group_join(g, clips[first + n]->pool)) n++;
        if (!n) { snprintf(g_host_err, sizeof(g_host_err), "clip_encode_multi: clip %d cannot join a launch group (%s)", first, h264e_hip_last_error()); h264e_hip_group_destroy(g); rc = -1; break; }
        for (i = first; i < first + n; i++)
        {
            /* The members' launches run in lock step, so a member that was stopped by a mis-speculation idles until the round's longest
             * launch is over: streams with frequent events (single slice, constant QP) get shorter launches inside a group -- a third of
             * the pipeline depth -- which costs streams WITHOUT staggered events a few percent and gives staggered ones 13 %
             * (measured, 4 different 1080p clips: 12.8 -> 14.6 M MB/s aggregate; 4 identical ones 21.4 -> 20.7 M) */
            saved_base[i] = clips[i]->launch_base;
            if (n > 1 && clips[i]->par.slices <= 1 && !clips[i]->all_key && !clips[i]->rc_on)
            {
                clips[i]->launch_base = imax(8, clips[i]->launch_base/3);
                clips[i]->launch_frames = imin(clips[i]->launch_frames, clips[i]->launch_base);
            }
            a[i].clip = clips[i]; a[i].group = g; a[i].out = out[i]; a[i].cap = cap[i]; a[i].out_bytes = &out_bytes[i];
            a[i].frame_bytes = frame_bytes ? frame_bytes[i] : NULL; a[i].st = stats ? &stats[i] : NULL;
            if (pthread_create(&th[i], NULL, multi_thread, &a[i])) { snprintf(g_host_err, sizeof(g_host_err), "clip_encode_multi: cannot start a thread"); rc = -1; break; }
            started++;
        }
        /* a clip whose thread never started must not be waited for by the others */
        for (i = first + started; i < first + n; i++) h264e_hip_group_leave(g, clips[i]->pool);
        for (i = first; i < first + started; i++)
        {
            pthread_join(th[i], NULL);
            if (a[i].rc && !rc) { rc = a[i].rc; snprintf(g_host_err, sizeof(g_host_err), "clip %d: %s", i, a[i].err); }
        }
        for (i = first; i < first + n; i++) if (saved_base[i] > 0) clips[i]->launch_base = saved_base[i];
        h264e_hip_group_destroy(g);
        done = first + n;
    }
    free(a); free(th);
    return rc;
}
