/*
 * enc_scenecut.h -- scene-cut detection: the luma histogram of one resident input frame (H264E_clip_set_scenecut).
 *
 * The reference has no scene-cut detector; like the RGB conversion in enc_ingest.h, this integer definition IS the definition
 * (tests/scenecut_model.py restates it):
 *     H_f[b] = number of luma samples of the RAW input frame f (width x height, before the denoiser) with Y >> 2 == b, b = 0..63
 *     D(f)   = (sum over b of |H_f[b] - H_{f-1}[b]|) * 1024 / (2 * width * height)      (floor, 64-bit), D(0) = 0
 * and frame f > 0 that is not a key frame already becomes one when D(f) > threshold.  The device makes H_f -- one 64-dword record
 * per frame, so a bounded input ring never needs two pictures --, the host makes D from consecutive records (h264e_host.c).
 * A histogram distance ignores motion, which a frame difference does not: at 352x288 and above the test clips stay below 22
 * between consecutive frames and reach 280 at a cut.  Tiny pictures are another matter -- at 64x48 a histogram has 3072 samples
 * and is noisy (a pan reaches 160, a cut 175): they are for parity tests against the model, not for claims about detection.
 *
 * The luma plane of a slot is width*height contiguous bytes (rows packed); it is read ONCE, as aligned dwords, four samples per
 * lane.  A slot starts on an even address, not always a dword (frame_bytes = width*height*3/2): the dwords are those of the
 * enclosing aligned range and the bytes outside the plane -- up to two in front (the frame before it in the ring), up to two behind
 * (this frame's chroma) -- are masked out; both lie inside the pool's allocation.
 *   scenecut_load  : lane level.  Dword i of the range; the kernel issues eight of them per lane before it counts the first, so that
 *                    a lane has 32 bytes in flight (one dependent load per pass would leave the kernel waiting for HBM eight times).
 *   scenecut_count : lane level.  The four samples of such a dword -> four adds into the workgroup's LDS histogram.  The histogram is kept in
 *                    32 replicas, bin b of replica r at dword 32*b + r, and a lane uses replica (lane & 31): the 32 lanes that
 *                    share an LDS cycle always hit 32 different banks, whatever their bins -- neighbouring samples of a smooth
 *                    picture fall into ONE bin, which would serialise a single histogram 32 ways.  (The two lanes l and l + 32 that share
 *                    a replica are served in different cycles; LDS atomics make the sharing correct across the workgroup's waves.)
 *   scenecut_flush : thread b < 64 sums bin b over the replicas, starting at replica b (rotated: conflict-free again), and adds the
 *                    sum to the frame's record with one vector global atomic.  Nothing scalar writes memory.
 * h264e_kernels.hip runs it as h264e_scenecut_kernel, h264e_pool.h's emulation launch (H264E_EMU) as a lane loop.
 */
#ifndef H264E_ENC_SCENECUT_H
#define H264E_ENC_SCENECUT_H
#include "wave.h"

#define SCENECUT_BINS 64
#define SCENECUT_REPLICAS 32
#define SCENECUT_LDS_DWORDS (SCENECUT_BINS*SCENECUT_REPLICAS)

/* an add to the workgroup's LDS that other lanes may hit at the same time; the emulation's lanes run one after the other */
#ifdef H264E_EMU
DEV void wg_atomic_add(LDS_AS uint32_t *p, uint32_t v) { *p += v; }
#else
DEV void wg_atomic_add(LDS_AS uint32_t *p, uint32_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
#endif

/* dwords of the aligned range that encloses the n bytes at `plane` */
DEV uint32_t scenecut_dwords(const gu8 *plane, uint32_t n) { return (uint32_t)(((uintptr_t)plane & 3) + n + 3) >> 2; }

/* dword i (< scenecut_dwords) of the aligned range around the luma plane [plane, plane + n) */
DEV uint32_t scenecut_load(const gu8 *plane, uint32_t i)
{
    const gu8 *q = plane - ((uintptr_t)plane & 3) + 4*(size_t)i;
    EMU_GLOBAL(q, 4);
    return *(const GLOBAL_AS uint32_t *)q;
}

/* ... and its samples (v = scenecut_load(plane, i)) into the LDS histogram, replica `rep` (< SCENECUT_REPLICAS) */
DEV void scenecut_count(LDS_AS uint32_t *hist, const gu8 *plane, uint32_t n, uint32_t i, uint32_t v, int rep)
{
    const uint32_t mis = (uint32_t)((uintptr_t)plane & 3);
    const uint32_t b0 = 4*i - mis;                                  /* index of byte 0 in the plane (wraps below zero in dword 0) */
    if (4*i >= mis && b0 + 4 <= n)
    {
        for (int k = 0; k < 4; k++) wg_atomic_add(hist + (((v >> (8*k + 2)) & 63u) << 5) + rep, 1u);
        return;
    }
    for (int k = 0; k < 4; k++)
        if (4*i + (uint32_t)k >= mis && b0 + (uint32_t)k < n) wg_atomic_add(hist + (((v >> (8*k + 2)) & 63u) << 5) + rep, 1u);
}

/* bin b of the workgroup's histogram, summed over the replicas, into the frame's record */
DEV void scenecut_flush(const LDS_AS uint32_t *hist, GLOBAL_AS int *record, int b)
{
    uint32_t s = 0;
    for (int j = 0; j < SCENECUT_REPLICAS; j++) s += hist[(b << 5) + ((j + b) & (SCENECUT_REPLICAS - 1))];
    g_atomic_add(record + b, (int)s);                               /* (skips a zero sum) */
}

#endif
