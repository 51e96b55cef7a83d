/*
 * api_harness.c -- TEST INFRASTRUCTURE.  Generator of tests/golden/run_params.json: streams of the REFERENCE encoder whose run parameters
 * change from frame to frame -- frame_type, encode_speed, desired_frame_bytes, the QP window, run_param == NULL, H264E_set_vbv_state in
 * front of a frame (h264-lab.h:6701-6775, :6497, :6611).  The reference CLI sets one H264E_run_param_t for the whole stream, so its
 * binary cannot produce these.  Compiles the reference header into this translation unit and only CALLS its public API;
 * the input is the synth_v1 clip of oracle/synth_v1.c.  Built and run in the build container only (`make -C oracle api`,
 * tests/golden/make_golden_run_params.py); what it prints -- data -- is committed.
 *
 *   api_harness script.txt [out.264]
 *
 * script, whitespace-separated integers:
 *   line 1:      width height gop vbv_size_bytes const_input_flag temporal_denoise_flag slices
 *   every other: frame_type encode_speed desired_frame_bytes qp_min qp_max vbv_size vbv_fullness null_run_param
 *                (vbv_size < 0: no H264E_set_vbv_state in front of this frame; null_run_param 1: H264E_encode(run_param = NULL))
 * A line whose frame_type is none of DEFAULT (0), P (2), KEY (6) is a call the product refuses: the reference is NOT called for it, so
 * that the stream printed here is the reference's stream WITHOUT those calls; the picture it would have taken goes to the next line.
 * Pictures are synth_v1 frames 0, 1, 2, ... of seed 1, one per call made.
 *
 * output, one line per script line:  frame=N status=S key=K bytes=B md5=<coded bytes> [recon=<the three planes after the call>]
 *                                    frame=N refused
 * (key: the coded data starts with an SPS; recon only with const_input_flag = 0: the reconstruction, h264-lab.h:6719-6723; after a transparent frame the reference picture,
 * :6505-6508).  Slices (> 1) need the binary built with -DH264E_MAX_THREADS=8 (api_harness_thr): its run_func_in_thread is a plain serial
 * loop, so the row bands are coded without pthreads.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <math.h>
#define MINIH264_IMPLEMENTATION
#include "h264-lab.h"
#include "synth_v1.h"

/* RFC 1321 */
static void md5_block(uint32_t h[4], const uint8_t *p)
{
    static const uint8_t rot[4][4] = { {7, 12, 17, 22}, {5, 9, 14, 20}, {4, 11, 16, 23}, {6, 10, 15, 21} };
    static uint32_t K[64];
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], m[16];
    int i;
    if (!K[0]) for (i = 0; i < 64; i++) { double s = sin((double)(i + 1)); K[i] = (uint32_t)((s < 0 ? -s : s)*4294967296.0); }
    for (i = 0; i < 16; i++) m[i] = (uint32_t)p[4*i] | (uint32_t)p[4*i + 1] << 8 | (uint32_t)p[4*i + 2] << 16 | (uint32_t)p[4*i + 3] << 24;
    for (i = 0; i < 64; i++)
    {
        uint32_t f, t;
        int g, r = rot[i >> 4][i & 3];
        if (i < 16)      { f = (b & c) | (~b & d); g = i; }
        else if (i < 32) { f = (d & b) | (~d & c); g = (5*i + 1) & 15; }
        else if (i < 48) { f = b ^ c ^ d;          g = (3*i + 5) & 15; }
        else             { f = c ^ (b | ~d);       g = (7*i) & 15; }
        t = a + f + K[i] + m[g];
        a = d; d = c; c = b;
        b += (t << r) | (t >> (32 - r));
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d;
}
static void md5_hex(const uint8_t *p, size_t n, char hex[33])
{
    uint32_t h[4] = { 0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u };
    uint8_t tail[128];
    size_t i, full = n & ~(size_t)63, rest = n - full, tn;
    uint64_t bits = (uint64_t)n*8;
    for (i = 0; i < full; i += 64) md5_block(h, p + i);
    memset(tail, 0, sizeof(tail));
    memcpy(tail, p + full, rest);
    tail[rest] = 0x80;
    tn = rest + 9 <= 64 ? 64 : 128;
    for (i = 0; i < 8; i++) tail[tn - 8 + i] = (uint8_t)(bits >> (8*i));
    for (i = 0; i < tn; i += 64) md5_block(h, tail + i);
    for (i = 0; i < 16; i++) sprintf(hex + 2*i, "%02x", (unsigned)((h[i >> 2] >> (8*(i & 3))) & 255));
}

#if H264E_MAX_THREADS
static void run_serial(void *token, void (*job)(void *), void *data[], int njobs)
{
    int i;
    (void)token;
    for (i = 0; i < njobs; i++) job(data[i]);
}
#endif

int main(int argc, char **argv)
{
    H264E_create_param_t cp;
    H264E_run_param_t rp;
    H264E_io_yuv_t io;
    H264E_persist_t *enc;
    H264E_scratch_t *scratch;
    int sp = 0, ss = 0, w, h, gop, vbv, cinp, den, slices, line = 0, t = 0, v[8];
    uint8_t *frame;
    size_t fsz;
    char hex[33], hex2[33];
    FILE *f, *o = NULL;
    if (argc < 2 || !(f = fopen(argv[1], "r"))) { fprintf(stderr, "usage: api_harness script.txt [out.264]\n"); return 2; }
    if (argc > 2 && !(o = fopen(argv[2], "wb"))) return 2;
    if (fscanf(f, "%d %d %d %d %d %d %d", &w, &h, &gop, &vbv, &cinp, &den, &slices) != 7) return 2;
    memset(&cp, 0, sizeof(cp));
    cp.width = w; cp.height = h; cp.gop = gop; cp.vbv_size_bytes = vbv; cp.const_input_flag = cinp; cp.temporal_denoise_flag = den;
    cp.enableNEON = 1; cp.num_layers = 1;
#if H264E_MAX_THREADS
    cp.max_threads = slices > 1 ? slices : 0;
    cp.run_func_in_thread = run_serial;
#else
    if (slices > 1) { fprintf(stderr, "slices need the -DH264E_MAX_THREADS build\n"); return 2; }
#endif
    if (H264E_sizeof(&cp, &sp, &ss)) return 1;
    fsz = (size_t)w*h*3/2;
    enc = (H264E_persist_t *)malloc((size_t)sp + 64);
    scratch = (H264E_scratch_t *)malloc((size_t)ss + 64);
    frame = (uint8_t *)malloc(fsz);
    if (!enc || !scratch || !frame || H264E_init(enc, &cp)) return 1;
    while (fscanf(f, "%d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7) == 8)
    {
        unsigned char *coded = NULL;
        int bytes = 0, status, key;
        if (v[0] != H264E_FRAME_TYPE_DEFAULT && v[0] != H264E_FRAME_TYPE_P && v[0] != H264E_FRAME_TYPE_KEY)
        {
            printf("frame=%d refused\n", line++);
            continue;
        }
        if (v[5] >= 0) H264E_set_vbv_state(enc, v[5], v[6]);
        synth_v1_frame(frame, w, h, t++, 1);
        io.yuv[0] = frame; io.yuv[1] = frame + (size_t)w*h; io.yuv[2] = io.yuv[1] + (size_t)(w/2)*(h/2);
        io.stride[0] = w; io.stride[1] = io.stride[2] = w/2;
        memset(&rp, 0, sizeof(rp));
        rp.frame_type = v[0]; rp.encode_speed = v[1]; rp.desired_frame_bytes = v[2]; rp.qp_min = v[3]; rp.qp_max = v[4];
        status = H264E_encode(enc, scratch, v[7] ? NULL : &rp, &io, &coded, &bytes);
        if (status) bytes = 0;
        if (o) fwrite(coded, 1, (size_t)bytes, o);
        key = bytes > 4 && (coded[4] & 31) == 7;
        md5_hex(coded, (size_t)bytes, hex);
        if (!cinp)
        {
            md5_hex(frame, fsz, hex2);
            printf("frame=%d status=%d key=%d bytes=%d md5=%s recon=%s\n", line++, status, key, bytes, hex, hex2);
        } else
            printf("frame=%d status=%d key=%d bytes=%d md5=%s\n", line++, status, key, bytes, hex);
    }
    fclose(f);
    if (o) fclose(o);
    return 0;
}
