/*
 * h264e_kernels.hip -- HIP kernels of the per-frame encode path and their C-ABI launcher (include/h264e_hip.h).
 *
 * Kernels (gfx950, wave64):
 *   h264e_mb_kernel      one 64-lane workgroup per (job, macroblock row) + one finalizer workgroup per job; rows of one
 *                        picture run as a wavefront behind each other: row r may encode macroblock x once row r-1 has
 *                        published x+2 macroblocks (left, top-left, top, top-right neighbours + in-loop deblocking order);
 *                        consecutive frames of a stream run as a temporal wavefront a few steps apart.  Hand-off: per-row
 *                        progress counters, payload stored write-through (sc1), relaxed polls, one acquire per hand-off
 *                        (cdna_hip_programming.md Guideline 16 R1).  The finalizer splices the row bit buffers into the
 *                        slice RBSP (there is no separate splice kernel) and exports the frame to host-mapped memory: its body is
 *                        enc_finalize.h job_finalize, shared with the emulation; its waits, fences and scopes are FinalizerOnDevice below.
 *   h264e_synth_kernel   fills resident input frames with the synth_v1 clip (bench / test input in HBM).
 *   h264e_denoise_kernel the temporal denoiser (enc_denoise.h) over one frame: raw input + previous denoised picture -> new
 *                        denoised picture, out of place, one launch per frame in stream order.
 *   h264e_ingest_kernel  device-resident input (enc_ingest.h): one I420 / NV12 / RGB frame in HBM -> the packed I420 input slot.
 *   h264e_egress_kernel  device-resident output (enc_egress.h): a reconstructed picture -> I420 / NV12 / RGB / planar RGB in the caller's HBM.
 *   h264e_scale_kernel   the same as the ingest for a source of another size (enc_scale.h): a window of an I420 / NV12 frame, box-filtered down to the slot.
 *   h264e_scale_rgb_kernel  ... of a planar RGB frame (enc_scale_rgb.h): the three channels box-filtered into LDS, converted to I420 from there.
 *   h264e_ingest_hbd_kernel<SB, C444>, h264e_scale_hbd_kernel<SB>  the I420 / NV12 paths for 16-bit samples and 4:4:4 chroma (enc_hbd.h).
 *   h264e_ingest_422_kernel<SB, PACK>, h264e_scale_422_kernel<SB>  4:2:2 input: I422, NV16 and packed YUYV / UYVY, 8- or 16-bit (enc_422.h).
 *   h264e_tonemap_kernel<LAYOUT>  HDR10 input (enc_tonemap.h): a 16-bit PQ / BT.2020 surface tone-mapped to the 8-bit picture, at size or into the scratch surface of a window.
 *   h264e_ingest_float_kernel<ST>, h264e_scale_rgb_float_kernel<ST>, h264e_egress_float_kernel<ST>  the planar RGB paths for float16 /
 *                        bfloat16 / float32 samples in [0, 1], quantised on the way in and divided by 255 on the way out.
 *   h264e_scenecut_kernel scene-cut detection (enc_scenecut.h): the 64-bin luma histogram of one resident input frame.
 *   h264e_lookahead_kernel the cost pass of the lookahead rate control (enc_lookahead.h): intra / inter cost sums of one resident input frame.
 *   h264e_lookahead_search_kernel the same pass with a motion search of up to +-8 half-resolution samples per block
 *                        (enc_lookahead_search.h): the sums from the searched inter cost, and a motion field.
 *   h264e_lookahead_tree_kernel the cost tree over that field (enc_lookahead_tree.h): one frame step of the backward propagation, and
 *                        the frame's sum of what it received.
 *   h264e_mcdenoise_kernel the motion-compensated temporal denoiser (enc_mcdenoise.h): the denoiser's filter against the previous
 *                        denoised picture displaced by that motion field, refined by one sample per 16x16 block.
 *
 * HIP only (hipcc --offload-arch=gfx950).  The host side of the boundary is h264e_pool.h, included at the end; the test-only
 * emulation of tests/emu compiles the same kernel HEADERS with its own launch functions and never sees this file.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "enc_row.h"
#include "enc_finalize.h"
#include "enc_selftest.h"
#include "enc_denoise.h"
#include "enc_ingest.h"
#include "enc_egress.h"
#include "enc_scale.h"
#include "enc_scale_rgb.h"
#include "enc_hbd.h"
#include "enc_422.h"
#include "enc_tonemap.h"
#include "enc_scenecut.h"
#include "enc_lookahead.h"
#include "enc_lookahead_search.h"
#include "enc_lookahead_tree.h"
#include "enc_mcdenoise.h"
#include "enc_ssim.h"
#include "../../include/h264e_hip.h"

#include <hip/hip_runtime.h>


/* ------------------------------------------------------------------ device code */



/* relaxed poll of one progress counter until it reaches `need`.  Returns 0 = reached, -1 = producer failed or the
 * bound expired, -2 = producer was aborted (negative counters are poison left behind by a row that stopped). */
#ifndef H264E_POLL_SLEEP
/* x 64 cycles between two polls of a counter in device memory.  Measured in round 4 (gpurun_out/sleep_ab, sleep2): 1, 2, 8, 16, 32 are level
 * within 0.3 % in every regime (stream, 8 slices, rate control, lone frame: the round trip of the poll itself is what a hand-off costs);
 * what changes is what the parked waves issue meanwhile: with 16 here and 4 for the LDS hand-off words below, the scalar instructions
 * per delivered macroblock go from 10.6 k to 9.2 k (LDS 1.86 k -> 1.66 k) at the same speed */
#define H264E_POLL_SLEEP 16
#endif
DEV int poll_progress(const GLOBAL_AS int *flag, int need, int &seen, unsigned spin_limit)
{
    unsigned spins = 0;
    for (;;)
    {
        seen = uni(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));     /* uni: the loop control is scalar */
        if (seen >= need) return 0;
        if (seen < 0) return seen;
        if (++spins > spin_limit) return -1;
        __builtin_amdgcn_s_sleep(H264E_POLL_SLEEP);
    }
}

/* a progress counter of this row, for other workgroups (relaxed, agent scope; the payload in front of it was stored write-through and drained).
 * Every lane stores the same value to the same word -- one memory request for the wave: a store under "lane 0 only" is a divergent
 * branch, and behind one the compiler keeps the surrounding wave-uniform state (loop counters, the bit writer) in vector registers. */
DEV void publish(GLOBAL_AS int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

/* ---- hand-off words of the two-wave pipeline (LDS): release / acquire at workgroup scope, polled with s_sleep */
DEV int flag_get(const int *p) { return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); }
DEV void flag_set(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
#ifndef H264E_LDS_SLEEP
#define H264E_LDS_SLEEP 4            /* x 64 cycles between two looks at a hand-off word in LDS (1, 2, 4 measured level, see H264E_POLL_SLEEP) */
#endif
#define LDS_SPIN_LIMIT (1u << 26)       /* the partner wave is resident: this bound only ever ends a wait when something is badly wrong */
/* 0 = *flag reached need; otherwise the stop code the partner wave (or this bound) left: -1 failure, -2 abort */
DEV int lds_wait(const int *flag, int need, int *stop)
{
    for (unsigned spins = 0;; spins++)
    {
        if (uni(flag_get(flag)) >= need) return 0;
        const int s = uni(flag_get(stop));
        if (s) return s;
        if (spins > LDS_SPIN_LIMIT) { flag_set(stop, -1); return -1; }
        __builtin_amdgcn_s_sleep(H264E_LDS_SLEEP);
    }
}
/* what the search wave tells the reconstruction wave while it is still searching macroblock need - 1 (enc_mb.h inter_choose) */
struct SearchSignals
{
    RowLds *L;
    int need;
    bool help;          /* three waves per row: a helper wave searches the 8x8 partition type */
    DEVM void noskip() const { flag_set(&L->f_noskip, need); }
    DEVM void bound(int u) const { L->early_bound = u; flag_set(&L->f_bound, need); }
    DEVM bool helper() const { return help; }
    DEVM void t3_request(mv32 mv_best, int sad_best, const rect_t &lim) const
    {
        L->t3_mv_best = mv_best; L->t3_sad_best = sad_best;
        L->t3_lim[0] = lim.x0; L->t3_lim[1] = lim.y0; L->t3_lim[2] = lim.x1; L->t3_lim[3] = lim.y1;
        flag_set(&L->f_t3req, need);            /* release: the request and the predictor context copy (inter_choose) are visible with it */
    }
    DEVM bool t3_wait() const { return lds_wait(&L->f_t3done, need, &L->f_stop) == 0; }
};
/* the reconstruction wave's view of the inter decision of macroblock need - 1 (enc_row.h mb_intra_decide) */
struct InterFromSearchWave
{
    RowLds *L;
    int need;
    bool back_wave;     /* four waves per row: mb_recon_back of the previous macroblock runs on the fourth wave */
    /* ... which reads the deblocking inputs mb_decide is about to overwrite: wait until it is done with macroblock need - 2 */
    DEVM bool before_decide() const { return !back_wave || need < 2 || lds_wait(&L->f_wdone, need - 1, &L->f_stop) == 0; }
    DEVM bool ready() const { return uni(flag_get(&L->f_inter)) >= need; }
    DEVM bool wait_ready() const { return lds_wait(&L->f_inter, need, &L->f_stop) == 0; }
    DEVM int early_bound() const { return uni(flag_get(&L->f_bound)) >= need ? uni(L->early_bound) : 0x7fffffff; }
    DEVM bool wait_either(const int *f) const
    {
        for (unsigned spins = 0;; spins++)
        {
            if (uni(flag_get(&L->f_inter)) >= need || uni(flag_get(f)) >= need) return true;
            if (uni(flag_get(&L->f_stop))) return false;
            if (spins > LDS_SPIN_LIMIT) { flag_set(&L->f_stop, -1); return false; }
            __builtin_amdgcn_s_sleep(H264E_LDS_SLEEP);
        }
    }
    DEVM bool wait_noskip_or_ready() const { return wait_either(&L->f_noskip); }
    DEVM bool wait_bound_or_ready() const { return wait_either(&L->f_bound); }
};
/* the finalizer's view of time and memory (enc_finalize.h job_finalize lists the members): relaxed polls of counters and flags at agent
 * scope with s_sleep between them, every spin bounded by G.spin_limit, ONE acquire behind a poll that succeeded; a record goes out as
 * plain stores of one lane (the caller's guard), a release fence, a drain and the relaxed store of its flag -- at agent scope for the
 * frame behind, at system scope for the host */
struct FinalizerOnDevice
{
    const h264e_geom_t &G;
    const ChainG &C;
    const h264e_frame_task_t &T;
    GLOBAL_AS int *errflag;
    DEVM const GLOBAL_AS int *prev_flag() const { return &((const GLOBAL_AS h264e_walkrec_t *)T.walk_prev)->flag; }
    DEVM void converge() const { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }
    DEVM void acquire() const { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); converge(); }
    DEVM int rows_reached() const
    {
        int st = 0, seen = 0;
        for (int r = G.nmby - 1; r >= 0 && !st; r--) st = poll_progress(C.progress + r, G.nmbx + 1, seen, G.spin_limit);
        return st;
    }
    template <class IDLE> DEVM int wait_row(int r, IDLE idle) const
    {
        for (unsigned spins = 0;; spins++)
        {
            const int seen = uni(__hip_atomic_load(C.progress + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (seen >= G.nmbx + 1) break;
            if (seen < 0) return seen;
            if (spins > G.spin_limit) return -1;
            if (idle()) return 1;
            __builtin_amdgcn_s_sleep(H264E_POLL_SLEEP);
        }
        acquire();
        return 0;
    }
    DEVM bool prev_up() const { return uni(__hip_atomic_load(prev_flag(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >= T.launch_id; }
    DEVM bool wait_prev() const { int sf = 0; return poll_progress(prev_flag(), T.launch_id, sf, G.spin_limit) == 0; }
    DEVM void acquire_prev() const { acquire(); }
    DEVM void publish_verdict(GLOBAL_AS h264e_walkrec_t *w) const
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(&w->flag, T.launch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    DEVM void before_export() const { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent"); converge(); }
    DEVM void publish_host(GLOBAL_AS h264e_hostdone_t *hd, int sign) const
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");                 /* system scope: the host reads these */
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(&hd->done, sign*T.launch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    DEVM void raise_abort() const { __hip_atomic_store((GLOBAL_AS int *)T.abort_word, T.launch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    DEVM void raise_err() const { *errflag = 1; }
#ifdef H264E_STAMPS
    unsigned long long fz_t = wall_clock64();
    /* 32..36: the time since the stamp before; 37: a count */
    DEVM void stamp(int id)
    {
        if (id == 37) { if (LANE == 0 && C.prof) atomicAdd(C.prof + 37, 1ull); return; }
        const unsigned long long n = wall_clock64();
        if (LANE == 0 && C.prof) atomicAdd(C.prof + id, n - fz_t);
        fz_t = n;
    }
#else
    DEVM void stamp(int) const {}
#endif
};

/*
 * Grid: njobs x (nmby + 1) workgroups of one wavefront -- or of two (WAVES = 2): the macroblock loop as a two-stage pipeline, one
 * wavefront searching macroblock x + 1 while the other reconstructs and writes x (enc_row.h).  Workgroup `row < nmby` encodes macroblock row
 * `row` of its job's frame; workgroup `nmby` is the job's finalizer: it follows the frame's rows as they end -- splices each into the
 * slice (enc_finalize.h splice_frame), walks its records (exact mv_clusters validation, JobWalk) -- and, in streaming use, exports the result
 * to host-mapped memory and raises the job's done word, so the host consumes frames while later frames of the same launch are still
 * being encoded.  Padding entries of a banded dispatch order (H264E_ORDER_PAD) are workgroups that exit at once.
 * Every workgroup waits for workgroups with a lower index (rows above; rows of the reference frame's job inside the
 * static lag; rows of the own job for the finalizer) -- with ONE exception: a reference read that leaves the LDS window
 * (a long vector) waits dynamically for the exact rows it touches, which can lie a bounded distance AHEAD in the dispatch
 * order (enc_kernels.h rv_wait_rect).  All spins are bounded; an expired one poisons the row counter and sets errflag.
 */
/* wavefronts per SIMD the register allocation aims at.  Measured (gpurun_out/r3_wpe3): the two-wave pipeline at 3 (168 VGPRs, a few
 * spills, 6 rows per CU) beats 2 everywhere -- 1080p single slice 8.2 -> 8.9 M MB/s, 4K 10.8 -> 12.9 M; the one-wave kernel is
 * better off at 2 (256 VGPRs): at 3 it spills 131 registers. */
#ifndef H264E_WPE2
#define H264E_WPE2 3
#endif
#ifndef H264E_WPE1
#define H264E_WPE1 2
#endif
#ifndef H264E_WPEI
#define H264E_WPEI 4
#endif
/* OCC: wavefronts per SIMD the register allocation aims at.  The two-wave kernel exists twice: at 3 (164 VGPRs, nothing spilled) and at 4
 * (128 VGPRs, ~30 spilled); h264e_hip_submit picks per launch (more residency wins where a launch is bound by the rows in flight, fewer
 * spills where it is pure latency). */
template <int GEOM, int WAVES, int OCC>
__global__ void __launch_bounds__(64*WAVES, OCC) h264e_mb_kernel(h264e_geom_t G, const h264e_frame_task_t *tasks, const uint32_t *order)
{
    /* (the intra-only variant allocates the row state without the search-side buffers at its end: enc_mb.h ROWLDS_INTRA_BYTES) */
    __shared__ __attribute__((aligned(16))) unsigned char L_bytes[GEOM == GEOM_INTRA ? ROWLDS_INTRA_BYTES : sizeof(RowLds)];
    RowLds &L = *reinterpret_cast<RowLds *>(L_bytes);
    const int wv = WAVES >= 2 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;     /* which wavefront of the workgroup */
#ifdef H264E_LDS_PAD
    /* diagnostic build (Makefile `halfres`): extra LDS per workgroup so that fewer workgroups fit a CU -- what single-stream throughput
     * does when the resident rows are halved with the macroblock latency unchanged (the price of a multi-wave workgroup) */
    __shared__ volatile char lds_pad[H264E_LDS_PAD];
    if (G.nmbx < 0) lds_pad[LANE] = 1;
#endif
    /* workgroups are dispatched in index order: `order` lists (job, row) by the step at which the row can start
     * (H264E_FRAME_LAG*job + 2*row), so the resident workgroups are the ones that can make progress */
    const uint32_t jr = order[blockIdx.x];
    if (jr == H264E_ORDER_PAD) return;        /* padding of a banded dispatch order (h264e_pool.h build_order) */
    const int job = (int)(jr >> 16), row = (int)(jr & 0xffffu);
    const h264e_frame_task_t &T = tasks[job];
    if (!T.active) return;
    const ChainG C = chain_view(*T.chain_desc);
    GLOBAL_AS int *errflag = (GLOBAL_AS int *)uniptr(T.errflag);

    /* ---- finalizer (one wavefront; the others of a multi-wave workgroup have nothing to do here) */
    if (row == G.nmby) { if (!wv) job_finalize(G, C, T, FinalizerOnDevice{ G, C, T, errflag }); return; }

    /* ---- macroblock row */
    if (row < T.first_row) return;          /* kept from the previous encode of this frame (its counter already says complete) */
    if (job == 0 && row == G.test_stall_row) return;    /* fault injection: a producer that never publishes (tests/test_gpu_failures.py) */
    if (wv == 0) row_begin(L, G, C, T, row);
    if (WAVES >= 2) __syncthreads();         /* the one workgroup barrier: all wavefronts see the row's tables and initial state */
    const RowTask RT = rowtask_load(T);      /* the task's hot fields, once, in registers */
    int row0 = 0, row1 = G.nmby;            /* the slice (row band) this row belongs to */
    for (int k = 0; k < T.nslices; k++)
        if (row >= T.slice_row[k] && row < T.slice_row[k + 1]) { row0 = T.slice_row[k]; row1 = T.slice_row[k + 1]; }
    row0 = uni(row0); row1 = uni(row1);
    GLOBAL_AS int *my_progress = C.progress + row;
    /* bookkeeping: the wave that reconstructs adds the macroblocks this row got through, once, when the row ends or stops */
    GLOBAL_AS unsigned long long *mb_counter = (GLOBAL_AS unsigned long long *)uniptr(T.mb_counter);
    const auto count_mbs = [&](int n) { if (mb_counter && n > 0 && LANE == 0) __hip_atomic_fetch_add(mb_counter, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };

    if (WAVES == 1 || wv == 0)
    {
        /* ---- the wave that waits for the neighbours and searches (with one wave per row: does everything) */
        const GLOBAL_AS int *abort_word = (const GLOBAL_AS int *)uniptr(T.abort_word);
        const int launch_id = uni(T.launch_id);
        int seen = 0, seen_dep = 0;
        constexpr bool NARROW = GEOM == GEOM_NARROW;
        constexpr int DEP_ROWS = NARROW ? H264E_NARROW_DEP_ROWS : H264E_DEP_ROWS, DEP_COLS = NARROW ? H264E_NARROW_DEP_COLS : H264E_DEP_COLS;
        /* temporal wavefront: the reference window covers macroblock rows row-2 .. row+DEP_ROWS of the frame being referenced.
         * Inside one slice the lowest of them is the last to get there; with row-band slices the bands advance independently, so
         * every band the window touches is waited for at its lowest row inside the window (10 bits per row, lowest row first) */
        unsigned long long deps = 0;
        int ndeps = 0;
        if (T.dep_progress)
        {
            const int lo = imax(row - 2, 0), hi = imin(row + DEP_ROWS, G.nmby - 1);
            deps = (unsigned long long)hi; ndeps = 1;
            for (int k = T.nslices - 1; k >= 1; k--)
            {
                const int last = T.slice_row[k] - 1;            /* last row of slice k-1 */
                if (last >= lo && last < hi) { deps |= (unsigned long long)last << (10*ndeps); ndeps++; }
            }
            ndeps = uni(ndeps);
        }
        for (int x = 0; x < G.nmbx; x++)
        {
            /* consumer: relaxed sc1 polls, then sc1 loads of everything handed over */
            const int need = row > row0 ? imin(x + 2, G.nmbx) : 0;
            const int need_dep = RT.dep_progress ? imin(x + DEP_COLS, G.nmbx) : 0;     /* temporal wavefront: h264e_dev.h */
            int st = 0;
            /* the abort word lives in device memory (raised by a finalizer whose mv_clusters walk failed, or by the host): one L2 read per
             * macroblock, ISSUED here and looked at behind the window loads -- as is the first look at the row above's counter: three
             * round trips to L2 / HBM in flight together instead of one after the other (the records above are still loaded BEHIND the
             * counter that covers them, and behind the acquire) */
            const int abort_v = abort_word ? __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : launch_id - 1;
            const GLOBAL_AS int *above = C.progress + (WAVES >= 2 ? G.nmby : 0) + (row - 1);
            const int early = seen < need ? __hip_atomic_load(above, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : seen;
            /* temporal dependency first, then the loads that only need it (input, reference window) ... */
            if (seen_dep < need_dep)
            {
                int lowest = 0x7fffffff;
                for (int k = 0; k < ndeps && !st; k++)
                {
                    int sk = 0;
                    st = poll_progress((const GLOBAL_AS int *)RT.dep_progress + (int)((deps >> (10*k)) & 1023), need_dep, sk, G.spin_limit);
                    lowest = imin(lowest, sk);
                }
                seen_dep = lowest;
                if (!st) consumer_acquire();
            }
            /* two waves: macroblock x uses the hand-off buffer of x - 2, which the reconstruction wave must have left behind */
            STAMP(L, 13);
            if (WAVES >= 2 && !st && x >= 2) st = lds_wait(&L.f_wdone, x - 1, &L.f_stop);
            STAMP(L, 23);
            if (!st) row_prefetch<GEOM>(L, G, RT, row, x);
            STAMP(L, 0);
            if (uni(abort_v) == launch_id) st = -2;
            /* ... so that their latency overlaps with the wait for the row above */
            /* two waves: the search needs only the VECTORS of the row above, which that row's reconstruction wave hands over as soon as
             * they are decided (its `decided` counter, behind the progress counters) -- a transform / CAVLC / deblocking earlier than
             * the rest of the record, which this row's reconstruction wave waits for */
            if (!st && seen < need)
            {
                seen = uni(early);
                if (seen < 0) st = seen;
                else if (seen < need) st = poll_progress(above, need, seen, G.spin_limit);
                if (!st) consumer_acquire();
            }
            STAMP(L, 13);
            if (!st) load_top<WAVES >= 2 ? LOAD_TOP_MV : LOAD_TOP_ALL>(L, L.mb[x & 1], G, C.bottom + (size_t)(row - 1)*G.nmbx, C.pend + (size_t)(row - 1)*G.nmbx, x, row > row0);
            /* two waves: the search of x starts from the predictor context the decision of x - 1 leaves behind */
            STAMP(L, 0);
            if (WAVES >= 2 && !st && x >= 1) st = lds_wait(&L.f_decided, x, &L.f_stop);
            STAMP(L, 6);
            if (st)
            {
                /* stop: leave poison in this row's counter so everything behind it stops too (-1 failure, -2 abort); with two waves the
                 * reconstruction wave is the one that publishes, so it also leaves the poison (after what it is publishing right now) */
                if (WAVES >= 2) { flag_set(&L.f_stop, st); return; }
                if (LANE == 0)
                {
                    if (st == -1) *errflag = 1;
                    __hip_atomic_store(my_progress, st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                count_mbs(x);
                return;
            }
            if (WAVES == 1) row_step<GEOM>(L, G, C, RT, row, x, row0, row1);
            else mb_search<GEOM>(L, L.mb[x & 1], G, RT, row, x, row0, SearchSignals{ &L, x + 1, WAVES >= 3 });
            if (WAVES >= 3 && uni(flag_get(&L.f_stop))) return;         /* stopped while waiting for the helper wave */
            {
                /* a far reference read of this macroblock waited in vain (rv_wait_rect): what it encoded is not trustworthy */
                const int ff = uni(L.far_fail[0]) | (WAVES == 1 ? uni(L.far_fail[1]) : 0);
                if (ff)
                {
                    if (WAVES >= 2) { flag_set(&L.f_stop, ff < -2 ? -2 : ff); return; }
                    if (LANE == 0)
                    {
                        if (ff == -1) *errflag = 1;
                        __hip_atomic_store(my_progress, ff < -2 ? -2 : ff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    count_mbs(x);
                    return;
                }
            }
            if (WAVES >= 2) { flag_set(&L.f_inter, x + 1); STAMP(L, 14); continue; }
            /* producer: every handed-off byte was stored write-through (sc1, wave.h cstore*): drain them, then the counter --
             * no agent-scope release (L2 write-back) needed */
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            publish(my_progress, x + 1);
            STAMP(L, 14);
        }
        if (WAVES >= 2)
        {
#ifdef H264E_STAMPS
            if (LANE < 32 && C.prof) atomicAdd(C.prof + LANE, L.prof[0][LANE]);
#endif
            return;
        }
    } else if (WAVES >= 3 && wv == 2)
    {
        /* ---- the helper wave of the three-wave variant (launches of one or a few frames, where only the latency counts and the chip
         * is empty): searches the 8x8 partition type of macroblock x when the search wave asks for it */
        for (int x = 0; x < G.nmbx; x++)
        {
            int req = 0, st = 0;
            for (unsigned spins = 0;; spins++)
            {
                /* f_t3req is monotonic and carries the macroblock index (+1) of the LATEST request: only an exact match is a request for x.
                 * A larger value means the search wave finished x without asking and has already asked for a later macroblock -- skip x
                 * (running the 8x8 search with the context of x and the request data of x + 1 would also write into the hand-off
                 * buffer the reconstruction wave is reading).  A request for x precedes f_inter of x, and the search wave does not get
                 * past x while its request is unanswered, so "f_inter >= x + 1 without a request" is final. */
                const int r3 = uni(flag_get(&L.f_t3req));
                if (r3 == x + 1) { req = 1; break; }
                if (r3 > x + 1) break;
                if (uni(flag_get(&L.f_inter)) >= x + 1) break;                      /* the search wave is done with x without asking */
                if (uni(flag_get(&L.f_stop))) { st = 1; break; }
                if (spins > LDS_SPIN_LIMIT) { flag_set(&L.f_stop, -1); st = 1; break; }
                __builtin_amdgcn_s_sleep(H264E_LDS_SLEEP);
            }
            if (st) return;
            if (!req) continue;
            MbCtx m;
            mb_ctx_init<GEOM>(m, L, G, RT, row, x, row0, 2);
            const rect_t lim = { uni(L.t3_lim[0]), uni(L.t3_lim[1]), uni(L.t3_lim[2]), uni(L.t3_lim[3]) };
            const mv32 mv_best = (mv32)uni(L.t3_mv_best);
            const int sad_best = uni(L.t3_sad_best);
            GRP_EACH(t)
            {
                if (t == 3) search_type(L, L.mb[x & 1], m, 3, mv_best, sad_best, lim, 0);
            }
            wave_sync();
            const int ff = uni(L.far_fail[2]);
            if (ff) { flag_set(&L.f_stop, ff < -2 ? -2 : ff); return; }
            flag_set(&L.f_t3done, x + 1);
        }
#ifdef H264E_STAMPS
        if (LANE < 32 && C.prof) atomicAdd(C.prof + LANE, L.prof[2][LANE]);
#endif
        return;
    } else if (WAVES == 4 && wv == 3)
    {
        /* ---- the fourth wave of the latency variant: deblocking and every store of macroblock x (mb_recon_back) while the
         * reconstruction wave is already at the intra candidates of x + 1; owns the row's progress counter */
        for (int x = 0; x < G.nmbx; x++)
        {
            const int st = lds_wait(&L.f_front, x + 1, &L.f_stop);
            if (st)
            {
                if (LANE == 0) __hip_atomic_store(my_progress, st == -2 ? -2 : -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);        /* the row is being stopped: poison for everything behind it */
                return;
            }
            MbCtx m;
            mb_ctx_init<GEOM>(m, L, G, RT, row, x, row0, 1);
            m.type = uni(L.d_type[x & 1]);
            mb_recon_back<GEOM>(L, L.mb[x & 1], m, G, C, RT, row, x, row0, row1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            publish(my_progress, x + 1);
            flag_set(&L.f_wdone, x + 1);
        }
#ifdef H264E_STAMPS
        if (LANE < 32 && C.prof) atomicAdd(C.prof + LANE, L.prof[3][LANE]);
#endif
        return;
    } else
    {
        /* ---- the reconstruction wave of the two-wave pipeline: intra candidates + decision of x, then transform / CAVLC / deblocking /
         * stores of x while the search wave is already on x + 1 */
        GLOBAL_AS int *my_decided = my_progress + G.nmby;
        GLOBAL_AS h264e_mbbottom_t *rowrec = C.bottom + (size_t)row*G.nmbx;
        int seen = 0;
        for (int x = 0; x < G.nmbx; x++)
        {
            MbBuf &B = L.mb[x & 1];
            MbCtx m;
            mb_ctx_init<GEOM>(m, L, G, RT, row, x, row0, 1);
            int ff = 0;
            /* samples, contexts and pending lines of the row above: complete when its reconstruction wave has published x + 1 */
            const int need = row > row0 ? imin(x + 2, G.nmbx) : 0;
            if (seen < need)
            {
                ff = poll_progress(C.progress + (row - 1), need, seen, G.spin_limit);
                if (!ff) consumer_acquire();
                else flag_set(&L.f_stop, ff);
            }
            STAMP(L, 17);
            if (!ff)
            {
                load_top<LOAD_TOP_REST>(L, B, G, C.bottom + (size_t)(row - 1)*G.nmbx, C.pend + (size_t)(row - 1)*G.nmbx, x, row > row0);
                if (!mb_intra_decide(L, B, m, RT, InterFromSearchWave{ &L, x + 1, WAVES == 4 })) ff = uni(flag_get(&L.f_stop));
                else
                {
                    flag_set(&L.f_decided, x + 1);
                    /* the vectors of this macroblock's bottom row, for the search of the row below: on their way while the chroma
                     * prediction runs, published before the transform starts */
                    WAVE_FOR(l) { if (l < 4) cstore32((gu8 *)(rowrec + x) + 32 + 4*l, (uint32_t)B.mv_top[l]); }
                    const auto publish_decided = [&]() {
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        __builtin_amdgcn_wave_barrier();
                        publish(my_decided, x + 1);
                    };
                    if (WAVES == 4)
                    {
                        /* deblocking and the macroblock's stores go to the fourth wave; this one moves on to the intra candidates of x + 1 */
                        mb_recon_front<GEOM>(L, B, m, G, C, RT, row, x, row0, row1, publish_decided);
                        L.d_type[x & 1] = m.type;
                    } else mb_recon_write<GEOM>(L, B, m, G, C, RT, row, x, row0, row1, publish_decided);
                    ff = uni(L.far_fail[1]);
                    if (ff) { ff = ff < -2 ? -2 : ff; flag_set(&L.f_stop, ff); }
                    else if (WAVES == 4) flag_set(&L.f_front, x + 1);
                }
            }
            if (ff)
            {
                if (LANE == 0)
                {
                    if (ff == -1) *errflag = 1;
                    __hip_atomic_store(my_decided, ff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (WAVES != 4) __hip_atomic_store(my_progress, ff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      /* (four waves: the fourth one owns the progress counter, poison included) */
                }
                count_mbs(x);
                return;
            }
            if (WAVES == 4) { STAMP(L, 14); continue; }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            publish(my_progress, x + 1);
            flag_set(&L.f_wdone, x + 1);
            STAMP(L, 14);
        }
        /* four waves: the row ends when the fourth wave has stored the last macroblock */
        if (WAVES == 4 && lds_wait(&L.f_wdone, G.nmbx, &L.f_stop)) { count_mbs(G.nmbx); return; }
    }
    count_mbs(G.nmbx);
    row_end(L, G, C, row);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if (LANE == 0) __hip_atomic_store(my_progress, G.nmbx + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   /* row buffer + meta complete */
}


__global__ void __launch_bounds__(64) h264e_nal_escape_selftest_kernel(uint8_t *dst, uint32_t cap, const uint8_t *src, uint32_t n, uint32_t *out)
{
    int overflow = 0;
    const uint32_t w = nal_escape_copy((GLOBAL_AS uint8_t *)dst, cap, (const GLOBAL_AS uint8_t *)src, n, overflow);
    if (threadIdx.x == 0) { out[0] = w; out[1] = (uint32_t)overflow; }
}

__global__ void __launch_bounds__(64) h264e_stage_selftest_kernel(int stage, const uint8_t *in, const int *args, uint8_t *out)
{
    __shared__ StageLds S;
    __shared__ RowLds L;
    stage_selftest(S, L, stage, (const GLOBAL_AS uint8_t *)in, args, (GLOBAL_AS uint8_t *)out);
}

__global__ void __launch_bounds__(64) h264e_finalizer_selftest_kernel(h264e_geom_t G, const h264e_frame_task_t *task, int mode, const int *args, const int32_t *in, int32_t *hdr, mv32 *traj)
{
    finalizer_selftest(G, *task, mode, args, (const GLOBAL_AS int32_t *)in, (GLOBAL_AS int32_t *)hdr, (GLOBAL_AS mv32 *)traj);
}

__global__ void h264e_synth_kernel(uint8_t *dst, int w, int h, int t, uint32_t seed)
{
    const int n = w*h*3/2;
    for (int i = (int)(blockIdx.x*blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x*blockDim.x))
        dst[i] = sv_sample(w, h, t, seed, i);
}

/* sum of squared differences of one plane pair; grid.y = frame, grid.z = plane, grid.x strides over the samples */
__global__ void h264e_ssd_kernel(const uint8_t *clip, size_t frame_bytes, int width, int height, int in0, int in_mod,
                                 const h264e_chain_dev_t *chains, int pic0, int pic_mod, int W, unsigned long long *out)
{
    const int i = (int)blockIdx.y, pl = (int)blockIdx.z;
    const int w = width >> (pl ? 1 : 0), h = height >> (pl ? 1 : 0), ps = W >> (pl ? 1 : 0);
    const uint8_t *a = clip + frame_bytes*(size_t)((in0 + i) % in_mod) + (pl ? (size_t)width*height + (pl == 2 ? (size_t)(width/2)*(height/2) : 0) : 0);
    const uint8_t *b = chains[(pic0 + i) % pic_mod].rec[0][pl];
    unsigned long long s = 0;
    for (int k = (int)(blockIdx.x*blockDim.x + threadIdx.x); k < w*h; k += (int)(gridDim.x*blockDim.x))
    {
        const int y = k / w, x = k - y*w, d = (int)a[k] - (int)b[(size_t)y*ps + x];
        s += (unsigned long long)(d*d);
    }
    for (int o = 32; o; o >>= 1) s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out + 3*i + pl, s);
}

/* structural similarity (enc_ssim.h): grid.x = tile of SSIM_TW x SSIM_TW windows, grid.y = frame, grid.z = plane.  Block sums into LDS, one
 * window per lane, the tile's values added by a tree over the lane index: one float64 partial per workgroup, no atomics.  PLANES = 3 (the
 * frames of a clip, or the last frame of an encoder) or 1 (a plane pair).  Templates, like the float kernels: the compiler emits them behind
 * every kernel the project had, whose places in the code object therefore stay what they were. */
template <int PLANES> __global__ void __launch_bounds__(256) h264e_ssim_kernel(h264e_ssim_args_t A)
{
    __shared__ __attribute__((aligned(16))) SsimLds lds;
    LDS_AS SsimLds *L = (LDS_AS SsimLds *)&lds;
    const int t = (int)threadIdx.x, i = (int)blockIdx.y, pl = (int)blockIdx.z;
    const ssim_plane_t P = ssim_plane(A, i, pl);
    const int ntx = ssim_tiles(P.bw - 1), nty = ssim_tiles(P.bh - 1);
    if ((int)blockIdx.x >= ntx*nty) return;                 /* chroma planes have fewer tiles (uniform per workgroup) */
    const int ty = (int)blockIdx.x/ntx, tx = (int)blockIdx.x - ty*ntx;
    ssim_block(L, P, tx, ty, t);
    __syncthreads();
    ssim_window(L, P, tx, ty, t);
    __syncthreads();
    for (int s = 128; s; s >>= 1) { ssim_reduce(L->red, t, s); __syncthreads(); }
    if (t == 0) ssim_store((GLOBAL_AS double *)A.partial + ((size_t)i*PLANES + pl)*(size_t)A.max_tiles + blockIdx.x, L->red[0]);
}

/* ... its second launch: grid.x = frame, grid.y = plane; the partials in tile order (lane t: t, t + 256, ...), the same tree, the mean */
template <int PLANES> __global__ void __launch_bounds__(256) h264e_ssim_mean_kernel(h264e_ssim_args_t A)
{
    __shared__ double red[256];
    const int t = (int)threadIdx.x, i = (int)blockIdx.x, pl = (int)blockIdx.y;
    const ssim_plane_t P = ssim_plane(A, i, pl);
    const int ntiles = ssim_tiles(P.bw - 1)*ssim_tiles(P.bh - 1);
    ssim_gather((LDS_AS double *)red, (const GLOBAL_AS double *)A.partial + ((size_t)i*PLANES + pl)*(size_t)A.max_tiles, ntiles, t);
    __syncthreads();
    for (int s = 128; s; s >>= 1) { ssim_reduce((LDS_AS double *)red, t, s); __syncthreads(); }
    if (t == 0) ssim_store((GLOBAL_AS double *)A.out + (size_t)i*PLANES + pl, red[0]/((double)(P.bw - 1)*(double)(P.bh - 1)));
}

/* the temporal denoiser over one packed I420 frame (width x height): grid.z = plane, grid.y = row, grid.x * 256 lanes x 4 samples along
 * the row; the gain table is staged in LDS.  in / prev / out are separate frames (no inter-workgroup traffic). */
__global__ void __launch_bounds__(256) h264e_denoise_kernel(const uint8_t *in, const uint8_t *prev, uint8_t *out, int width, int height)
{
    __shared__ uint8_t T[256];
    const int pl = (int)blockIdx.z, y = (int)blockIdx.y;
    const int w = width >> (pl ? 1 : 0), h = height >> (pl ? 1 : 0);
    if (y >= h) return;                         /* chroma planes have half the rows (uniform per workgroup) */
    T[threadIdx.x] = k_denoise_gain[threadIdx.x];
    __syncthreads();
    const size_t off = pl ? (size_t)width*height + (pl == 2 ? (size_t)(width/2)*(height/2) : 0) : 0;
    const int aligned = !((((uintptr_t)in + off) | ((uintptr_t)prev + off) | ((uintptr_t)out + off) | (uintptr_t)w) & 3);
    denoise_group((const LDS_AS uint8_t *)T, (const GLOBAL_AS uint8_t *)(in + off), (const GLOBAL_AS uint8_t *)(prev + off), (GLOBAL_AS uint8_t *)(out + off),
                  w, h, (int)(blockIdx.x*blockDim.x + threadIdx.x), y, aligned);
}

/* device-resident input over one frame: grid.z = 0 luma / 1 both chroma planes, grid.y = row, grid.x * 256 lanes x 4 samples along the
 * row.  Every workgroup reads its own source bytes and writes its own bytes of the slot (no inter-workgroup traffic). */
__global__ void __launch_bounds__(256) h264e_ingest_kernel(h264e_ingest_src_t S, uint8_t *dst)
{
    const int g = (int)(blockIdx.x*blockDim.x + threadIdx.x), y = (int)blockIdx.y;
    if (blockIdx.z == 0) ingest_luma(S, (GLOBAL_AS uint8_t *)dst, g, y);
    else ingest_chroma(S, (GLOBAL_AS uint8_t *)dst, g, y);
}

/* ... of float planar RGB (ST = H264E_SAMPLE_F16 / _BF16 / _F32): kernels of their own, so that the 8-bit kernel has no branch per sample */
template <int ST> __global__ void __launch_bounds__(256) h264e_ingest_float_kernel(h264e_ingest_src_t S, uint8_t *dst)
{
    const int g = (int)(blockIdx.x*blockDim.x + threadIdx.x), y = (int)blockIdx.y;
    if (blockIdx.z == 0) ingest_float_luma<ST>(S, (GLOBAL_AS uint8_t *)dst, g, y);
    else ingest_float_chroma<ST>(S, (GLOBAL_AS uint8_t *)dst, g, y);
}

/* ... of 16-bit samples (SB = 2) and / or 4:4:4 chroma (enc_hbd.h): the same grid; kernels of their own, so that the 8-bit 4:2:0 kernel
 * stays the code it is */
template <int SB, int C444> __global__ void __launch_bounds__(256) h264e_ingest_hbd_kernel(h264e_ingest_src_t S, uint8_t *dst)
{
    const int g = (int)(blockIdx.x*blockDim.x + threadIdx.x), y = (int)blockIdx.y;
    if (blockIdx.z == 0) ingest_hbd_luma<SB>(S, (GLOBAL_AS uint8_t *)dst, g, y);
    else ingest_hbd_chroma<SB, C444>(S, (GLOBAL_AS uint8_t *)dst, g, y);
}

/* ... of 4:2:2 sources (enc_422.h): the same grid (a chroma row of the picture is a pair of source rows); PACK = H264E_PACK_*: the one
 * plane of YUYV / UYVY.  Kernels of their own again: the existing formats launch what they launched */
template <int SB, int PACK> __global__ void __launch_bounds__(256) h264e_ingest_422_kernel(h264e_ingest_src_t S, uint8_t *dst)
{
    const int g = (int)(blockIdx.x*blockDim.x + threadIdx.x), y = (int)blockIdx.y;
    if (blockIdx.z == 0) ingest_422_luma<SB, PACK>(S, (GLOBAL_AS uint8_t *)dst, g, y);
    else ingest_422_chroma<SB, PACK>(S, (GLOBAL_AS uint8_t *)dst, g, y);
}

/* HDR10 input (enc_tonemap.h): grid.y = TM_WG_ROWS PAIRS of rows (chroma rows), grid.x * 256 lanes x 4 luma columns along them; LAYOUT =
 * H264E_INGEST_I420 / _NV12.  The tables are staged once per workgroup (9 KB for up to 48 KB of samples in and out); from there every
 * workgroup reads its own source bytes and writes its own bytes of the destination (no inter-workgroup traffic).  No lane leaves before
 * the barrier; tonemap_group itself refuses a row pair or a column beyond the picture */
#define TM_WG_ROWS 4
template <int LAYOUT> __global__ void __launch_bounds__(256) h264e_tonemap_kernel(h264e_tonemap_src_t S, uint8_t *dst)
{
    __shared__ float tab[TM_TABLE_FLOATS];
    tm_stage((LDS_AS float *)tab, S.tables, (int)threadIdx.x);
    __syncthreads();
    S.format = LAYOUT;
    for (int i = 0; i < TM_WG_ROWS; i++)
        tonemap_group(S, (const LDS_AS float *)tab, (GLOBAL_AS uint8_t *)dst, (int)(blockIdx.x*blockDim.x + threadIdx.x), (int)blockIdx.y*TM_WG_ROWS + i);
}

/* device-resident output over one picture (enc_egress.h): grid.z = 0 luma / 1 both chroma planes for I420 and NV12, grid.y = row; the RGB
 * formats have grid.z = 0 alone and grid.y = a PAIR of rows (one chroma row); grid.x * 256 lanes x 4 samples along the row.  Every workgroup
 * reads its own bytes of the picture and writes its own bytes of the destination (no inter-workgroup traffic, no LDS). */
__global__ void __launch_bounds__(256) h264e_egress_kernel(h264e_egress_dst_t D, const uint8_t *src)
{
    egress_group(D, (const GLOBAL_AS uint8_t *)src, (int)(blockIdx.x*blockDim.x + threadIdx.x), (int)blockIdx.y, (int)blockIdx.z);
}

/* ... to float planar RGB: grid.y = a pair of rows, as for the 8-bit RGB formats */
template <int ST> __global__ void __launch_bounds__(256) h264e_egress_float_kernel(h264e_egress_dst_t D, const uint8_t *src)
{
    egress_rgb<0, ST>(D, (const GLOBAL_AS uint8_t *)src, (int)(blockIdx.x*blockDim.x + threadIdx.x), (int)blockIdx.y);
}

/* device-resident input of another size (enc_scale.h): grid.z = plane, grid.x / grid.y = the tile of 64 x S.th destination samples.  Column
 * and row taps once per tile, then the horizontal sums of the tile's source rows into LDS, then the vertical pass from LDS.  Every
 * workgroup reads its own source bytes and writes its own bytes of the slot (no inter-workgroup traffic). */
__global__ void __launch_bounds__(256) h264e_scale_kernel(h264e_scale_src_t S, uint8_t *dst)
{
    __shared__ __attribute__((aligned(16))) ScaleLds lds;
    LDS_AS ScaleLds *L = (LDS_AS ScaleLds *)&lds;
    const int comp = (int)blockIdx.z;
    ScaleTile T;
    if (!scale_tile(S, comp, (int)blockIdx.x, (int)blockIdx.y, T)) return;      /* chroma planes have fewer tiles (uniform per workgroup) */
    scale_tables(L, T, (int)threadIdx.x);
    __syncthreads();
    const int items = scale_src_rows(L, T) << 6;
    for (int it = (int)threadIdx.x; it < items; it += 256) scale_hpass(L, S.c[comp], T, it);
    __syncthreads();
    for (int it = (int)threadIdx.x; it < T.nrows*16; it += 256) scale_vpass(L, T, (GLOBAL_AS uint8_t *)(dst + scale_plane_offset(S, comp)), it);
}

/* ... of 16-bit samples and / or 4:4:4 chroma (enc_hbd.h): the same three steps with a source geometry per plane; SB = 2 quantises the
 * taps as the horizontal pass loads them.  grid.y covers the plane with the most rows of tiles */
template <int SB> __global__ void __launch_bounds__(256) h264e_scale_hbd_kernel(h264e_scale_src_t S, uint8_t *dst)
{
    __shared__ __attribute__((aligned(16))) ScaleLds lds;
    LDS_AS ScaleLds *L = (LDS_AS ScaleLds *)&lds;
    const int comp = (int)blockIdx.z;
    ScaleTile T;
    if (!scale_tile_hbd(S, comp, (int)blockIdx.x, (int)blockIdx.y, T)) return;  /* uniform per workgroup */
    scale_tables(L, T, (int)threadIdx.x);
    __syncthreads();
    const int items = scale_src_rows(L, T) << 6;
    for (int it = (int)threadIdx.x; it < items; it += 256)
    {
        if (SB == 2) scale_hpass_hbd(L, S.c[comp], T, S.qround, S.qshift, it); else scale_hpass(L, S.c[comp], T, it);
    }
    __syncthreads();
    for (int it = (int)threadIdx.x; it < T.nrows*16; it += 256) scale_vpass(L, T, (GLOBAL_AS uint8_t *)(dst + scale_plane_offset(S, comp)), it);
}

/* ... of 4:2:2 sources (enc_422.h): the chroma planes have half the window's width and all of its height.  8-bit taps of planes and U,V
 * pairs go through scale_hpass as they are, those of a packed row (steps 2 and 4) through scale_hpass_pk, 16-bit taps through
 * scale_hpass_hbd at any step.  S.pack is uniform per launch */
template <int SB> __global__ void __launch_bounds__(256) h264e_scale_422_kernel(h264e_scale_src_t S, uint8_t *dst)
{
    __shared__ __attribute__((aligned(16))) ScaleLds lds;
    LDS_AS ScaleLds *L = (LDS_AS ScaleLds *)&lds;
    const int comp = (int)blockIdx.z;
    ScaleTile T;
    if (!scale_tile_422(S, comp, (int)blockIdx.x, (int)blockIdx.y, T)) return;  /* uniform per workgroup */
    scale_tables(L, T, (int)threadIdx.x);
    __syncthreads();
    const int items = scale_src_rows(L, T) << 6;
    for (int it = (int)threadIdx.x; it < items; it += 256)
    {
        if (SB == 2) scale_hpass_hbd(L, S.c[comp], T, S.qround, S.qshift, it);
        else if (S.pack) scale_hpass_pk(L, S.c[comp], T, it);
        else scale_hpass(L, S.c[comp], T, it);
    }
    __syncthreads();
    for (int it = (int)threadIdx.x; it < T.nrows*16; it += 256) scale_vpass(L, T, (GLOBAL_AS uint8_t *)(dst + scale_plane_offset(S, comp)), it);
}

/* planar RGB input of another size (enc_scale_rgb.h): grid.x / grid.y = the tile of 64 x S.th destination pixels, all three output planes
 * of it.  The taps once, then per channel the horizontal sums and the vertical pass into the LDS tile (hsum is reused, hence the second
 * barrier), then the conversion from LDS.  Every workgroup reads its own source bytes and writes its own bytes of the slot. */
__global__ void __launch_bounds__(256) h264e_scale_rgb_kernel(h264e_scale_src_t S, uint8_t *dst)
{
    __shared__ __attribute__((aligned(16))) ScaleRgbLds lds;
    LDS_AS ScaleRgbLds *L = (LDS_AS ScaleRgbLds *)&lds;
    ScaleTile T;
    if (!scale_tile(S, 0, (int)blockIdx.x, (int)blockIdx.y, T)) return;
    scale_tables(&L->s, T, (int)threadIdx.x);
    __syncthreads();
    const int items = scale_src_rows(&L->s, T) << 6;
    for (int ch = 0; ch < 3; ch++)
    {
        for (int it = (int)threadIdx.x; it < items; it += 256) scale_hpass(&L->s, S.c[ch], T, it);
        __syncthreads();
        for (int it = (int)threadIdx.x; it < T.nrows*16; it += 256) scale_rgb_vpass(L, T, ch, it);
        __syncthreads();
    }
    for (int it = (int)threadIdx.x; it < scale_rgb_items(T); it += 256) scale_rgb_convert(S.cm, L, T, (GLOBAL_AS uint8_t *)dst, it);
}

/* ... of float planes: the same steps, the horizontal pass quantises as it loads (scale_hpass_float).  A kernel of its own, so that the
 * 8-bit kernel above stays the code it was */
template <int ST> __global__ void __launch_bounds__(256) h264e_scale_rgb_float_kernel(h264e_scale_src_t S, uint8_t *dst)
{
    __shared__ __attribute__((aligned(16))) ScaleRgbLds lds;
    LDS_AS ScaleRgbLds *L = (LDS_AS ScaleRgbLds *)&lds;
    ScaleTile T;
    if (!scale_tile(S, 0, (int)blockIdx.x, (int)blockIdx.y, T)) return;
    scale_tables(&L->s, T, (int)threadIdx.x);
    __syncthreads();
    const int items = scale_src_rows(&L->s, T) << 6;
    for (int ch = 0; ch < 3; ch++)
    {
        for (int it = (int)threadIdx.x; it < items; it += 256) scale_hpass_float<ST>(&L->s, S.c[ch], T, it);
        __syncthreads();
        for (int it = (int)threadIdx.x; it < T.nrows*16; it += 256) scale_rgb_vpass(L, T, ch, it);
        __syncthreads();
    }
    for (int it = (int)threadIdx.x; it < scale_rgb_items(T); it += 256) scale_rgb_convert(S.cm, L, T, (GLOBAL_AS uint8_t *)dst, it);
}

/* the luma histogram of one resident input frame (enc_scenecut.h): the plane's dwords are dealt to the workgroups in chunks of 256 lanes x
 * SCENECUT_UNROLL dwords (all loads of a chunk issued before the first sample is counted), every workgroup counts into its own LDS histogram
 * and adds its 64 sums to the frame's record (zeroed by the host in front of the launch) */
#define SCENECUT_UNROLL 8
__global__ void __launch_bounds__(256) h264e_scenecut_kernel(const uint8_t *luma, uint32_t nbytes, int *record)
{
    __shared__ uint32_t hist[SCENECUT_LDS_DWORDS];
    for (int k = (int)threadIdx.x; k < SCENECUT_LDS_DWORDS; k += 256) hist[k] = 0;
    __syncthreads();
    const gu8 *plane = (const gu8 *)luma;
    const uint32_t ndw = scenecut_dwords(plane, nbytes);
    const int rep = (int)(threadIdx.x & (SCENECUT_REPLICAS - 1));
    for (uint32_t c0 = blockIdx.x*(256u*SCENECUT_UNROLL); c0 < ndw; c0 += gridDim.x*(256u*SCENECUT_UNROLL))
    {
        uint32_t v[SCENECUT_UNROLL];
#pragma unroll
        for (int k = 0; k < SCENECUT_UNROLL; k++)
        {
            const uint32_t i = c0 + 256u*(uint32_t)k + threadIdx.x;
            v[k] = i < ndw ? scenecut_load(plane, i) : 0u;
        }
#pragma unroll
        for (int k = 0; k < SCENECUT_UNROLL; k++)
        {
            const uint32_t i = c0 + 256u*(uint32_t)k + threadIdx.x;
            if (i < ndw) scenecut_count((LDS_AS uint32_t *)hist, plane, nbytes, i, v[k], rep);
        }
    }
    __syncthreads();
    if (threadIdx.x < SCENECUT_BINS) scenecut_flush((const LDS_AS uint32_t *)hist, (GLOBAL_AS int *)record, (int)threadIdx.x);
}

/* the cost sums of one resident input frame (enc_lookahead.h): a wave takes 8 blocks at a time, 8 lanes per block and one block row per
 * lane; a workgroup of four waves takes 32 consecutive blocks per pass, so a wave's loads cover 128 contiguous bytes of 16 luma rows and
 * its stores 512 contiguous bytes of the half-resolution entry.  Lanes behind the last block load nothing and add nothing, but take part
 * in the butterflies. */
DEV int lookahead_oct_sum(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);      /* quad_perm [1,0,3,2] */
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true);      /* quad_perm [2,3,0,1] */
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true);     /* row_half_mirror: the other quad of the 8 lanes */
    return v;
}
__global__ void __launch_bounds__(256) h264e_lookahead_kernel(lookahead_args_t A)
{
    __shared__ int part[4][3];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6), r = lane & 7;
    int si = 0, sp = 0, sn = 0;             /* at most a few passes of one block each: far below 2^31 */
    for (int b0 = (int)blockIdx.x*32; b0 < A.nblk; b0 += (int)gridDim.x*32)
    {
        const int b = b0 + wave*8 + (lane >> 3), on = b < A.nblk;
        lookahead_row_t R = { { 0u, 0u }, { 0u, 0u } };
        if (on) R = lookahead_row(A, b, r);
        const int m = (lookahead_oct_sum(lookahead_row_sum(R)) + 32) >> 6;
        const int intra = lookahead_oct_sum(lookahead_row_intra(R, m));
        const int inter = A.prev ? lookahead_oct_sum(lookahead_row_inter(R)) : intra;
        if (on && r == 0) { si += intra; sp += intra < inter ? intra : inter; sn += intra < inter; }
    }
    si = wave_reduce_add(si); sp = wave_reduce_add(sp); sn = wave_reduce_add(sn);
    if (lane == 0) { part[wave][0] = si; part[wave][1] = sp; part[wave][2] = sn; }
    __syncthreads();
    if (threadIdx.x < 3)
    {
        const int k = (int)threadIdx.x;
        lookahead_record_add(A.record + k, (unsigned long long)(part[0][k] + part[1][k] + part[2][k] + part[3][k]));
    }
}

/* the cost pass with a motion search (enc_lookahead_search.h): one wave per workgroup and strip of 8 blocks, blockIdx.x the strip and
 * blockIdx.y the block row.  The only LDS traffic between lanes is inside the one wave: wave_sync orders it. */
DEV int lookahead_wave_min(int v)
{
    v = imin_raw(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false));     /* quad_perm [1,0,3,2] */
    v = imin_raw(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false));     /* quad_perm [2,3,0,1] */
    v = imin_raw(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false));    /* row_half_mirror */
    v = imin_raw(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false));    /* row_mirror */
    return imin_raw(imin_raw(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), imin_raw(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
__global__ void __launch_bounds__(64) h264e_lookahead_search_kernel(lookahead_search_args_t S)
{
    __shared__ lookahead_search_lds_t sh;
    LDS_AS uint32_t *prev = (LDS_AS uint32_t *)sh.prev, *cur = (LDS_AS uint32_t *)sh.cur;
    LDS_AS int *intra_of = (LDS_AS int *)sh.intra;
    const int lane = (int)threadIdx.x, i = lane >> 3, r = lane & 7;
    const int bx0 = (int)blockIdx.x*LOOKAHEAD_SEARCH_STRIP, by = (int)blockIdx.y, nb = imin_raw(LOOKAHEAD_SEARCH_STRIP, S.a.nbx - bx0);
    const int b = by*S.a.nbx + bx0 + i, on = i < nb;
    lookahead_row_t R = { { 0u, 0u }, { 0u, 0u } };
    if (on) R = lookahead_row(S.a, b, r);
    const int m = (lookahead_oct_sum(lookahead_row_sum(R)) + 32) >> 6;
    const int intra = lookahead_oct_sum(lookahead_row_intra(R, m));
    int key = LOOKAHEAD_SEARCH_NO_KEY;          /* lane i < nb: the winning key of strip block i */
    if (r == 0) intra_of[i] = intra;
    if (S.a.prev)
    {
        cur[2*lane] = R.lo[0]; cur[2*lane + 1] = R.lo[1];
        for (int c = lane; c < LOOKAHEAD_SEARCH_CELLS; c += 64) lookahead_search_stage(S, bx0, by, c, prev);
        if (lane == 0) prev[LOOKAHEAD_SEARCH_PREV_DWORDS - 1] = 0u;
    }
    wave_sync();
    if (S.a.prev)
    {
        const int side = 2*S.range + 1, rounds = (side*side + 63) >> 6;
        int cand[LOOKAHEAD_SEARCH_ROUNDS];
#pragma unroll
        for (int k = 0; k < LOOKAHEAD_SEARCH_ROUNDS; k++) cand[k] = lookahead_search_candidate(S.range, 64*k + lane);
        for (int j = 0; j < nb; j++)
        {
            const int best = lookahead_wave_min(lookahead_search_lane(S, prev, cur, bx0 + j, by, j, cand, rounds));
            if (lane == j) key = best;
        }
    }
    int si = 0, sp = 0, sn = 0;
    if (lane < nb)
    {
        /* frame 0 of the clip: inter = intra, the vector (0, 0) */
        const int mine = intra_of[lane];
        const int inter = S.a.prev ? key >> 15 : mine;
        lookahead_search_field_store(S, by*S.a.nbx + bx0 + lane, lookahead_search_cell(S.a.prev ? key : lookahead_search_key(mine, 0, 0)));
        si = mine; sp = mine < inter ? mine : inter; sn = mine < inter;
    }
    si = wave_reduce_add(si); sp = wave_reduce_add(sp); sn = wave_reduce_add(sn);
    if (lane < 3) lookahead_record_add(S.a.record + lane, (unsigned long long)(lane == 0 ? si : lane == 1 ? sp : sn));
}

/* one frame step of the cost tree (enc_lookahead_tree.h): one wave per workgroup and 8 consecutive blocks, lane = (block, row).  Lanes
 * behind the last block load nothing and add nothing, but take part in the butterflies and the reduction. */
__global__ void __launch_bounds__(64) h264e_lookahead_tree_kernel(lookahead_tree_args_t T)
{
    const int lane = (int)threadIdx.x, r = lane & 7;
    const int b = (int)blockIdx.x*LOOKAHEAD_TREE_WAVE_BLOCKS + (lane >> 3), on = b < T.nblk;
    lookahead_row_t R = { { 0u, 0u }, { 0u, 0u } };
    if (on) R = lookahead_tree_row(T, b, r);
    const int m = (lookahead_oct_sum(lookahead_row_sum(R)) + 32) >> 6;
    const int intra = lookahead_oct_sum(lookahead_row_intra(R, m));
    unsigned long long g = 0;
    if (on && r == 0) g = lookahead_tree_block(T, b, intra);
    /* 8 values of at most 2^40: the low 21 bits and the 20 above them, each sum below 2^24 */
    const int s0 = wave_reduce_add((int)(g & 0x1fffffu)), s1 = wave_reduce_add((int)(g >> 21));
    if (lane == 0) lookahead_record_add(T.sum, (unsigned long long)s0 + ((unsigned long long)s1 << 21));
}

/* the motion-compensated denoiser (enc_mcdenoise.h): one wave per workgroup and tile of 16x16 luma + 8x8 + 8x8 chroma samples, blockIdx.x
 * / .y the tile.  The only LDS traffic between lanes is inside the one wave: wave_sync orders it. */
template <int MODE> __global__ void __launch_bounds__(64) h264e_mcdenoise_kernel(mcdenoise_args_t A)
{
    __shared__ mcdenoise_lds_t sh;
    mcdenoise_block<MODE>(A, (LDS_AS mcdenoise_lds_t *)&sh, (int)blockIdx.x, (int)blockIdx.y);
}

/* ------------------------------------------------------------------ launches (what h264e_pool.h calls) */

/* variant: 0 = intra frames only (one wave per row, 4 per SIMD), 1 = one wave per row, 2 = two waves per row (3 per SIMD), 3 = the latency variant: four
 * waves per row (search | reconstruction | 8x8 search helper | deblocking and stores), 4 = two waves per row at 4 per SIMD */
static void bk_launch_mb(const h264e_geom_t &G, int narrow, int variant, int njobs, unsigned nblocks, const h264e_frame_task_t *td, const uint32_t *od, hipStream_t st)
{
    const dim3 grid(nblocks);
    (void)njobs;
    if (variant == 0) hipLaunchKernelGGL((h264e_mb_kernel<GEOM_INTRA, 1, H264E_WPEI>), grid, dim3(64), 0, st, G, td, od);
    else if (variant == 4)
    {
        if (narrow) hipLaunchKernelGGL((h264e_mb_kernel<GEOM_NARROW, 2, 4>), grid, dim3(128), 0, st, G, td, od);
        else hipLaunchKernelGGL((h264e_mb_kernel<GEOM_WIDE, 2, 4>), grid, dim3(128), 0, st, G, td, od);
    } else if (variant == 3)
    {
        if (narrow) hipLaunchKernelGGL((h264e_mb_kernel<GEOM_NARROW, 4, 2>), grid, dim3(256), 0, st, G, td, od);
        else hipLaunchKernelGGL((h264e_mb_kernel<GEOM_WIDE, 4, 2>), grid, dim3(256), 0, st, G, td, od);
    } else if (variant == 2)
    {
        if (narrow) hipLaunchKernelGGL((h264e_mb_kernel<GEOM_NARROW, 2, H264E_WPE2>), grid, dim3(128), 0, st, G, td, od);
        else hipLaunchKernelGGL((h264e_mb_kernel<GEOM_WIDE, 2, H264E_WPE2>), grid, dim3(128), 0, st, G, td, od);
    } else
    {
        if (narrow) hipLaunchKernelGGL((h264e_mb_kernel<GEOM_NARROW, 1, H264E_WPE1>), grid, dim3(64), 0, st, G, td, od);
        else hipLaunchKernelGGL((h264e_mb_kernel<GEOM_WIDE, 1, H264E_WPE1>), grid, dim3(64), 0, st, G, td, od);
    }
}

static void bk_launch_synth(uint8_t *dst, int w, int h, int t, uint32_t seed, hipStream_t st)
{
    hipLaunchKernelGGL(h264e_synth_kernel, dim3(1024), dim3(256), 0, st, dst, w, h, t, seed);
}
static void bk_launch_ssd(int n, const uint8_t *clip, size_t frame_bytes, int width, int height, int in0, int in_mod, const h264e_chain_dev_t *chains, int pic0, int pic_mod, int W,
                          unsigned long long *out, hipStream_t st)
{
    hipLaunchKernelGGL(h264e_ssd_kernel, dim3(64, (unsigned)n, 3), dim3(256), 0, st, clip, frame_bytes, width, height, in0, in_mod, chains, pic0, pic_mod, W, out);
}
static void bk_launch_nal_selftest(uint8_t *dst, uint32_t cap, const uint8_t *src, uint32_t n, uint32_t *out, hipStream_t st)
{
    hipLaunchKernelGGL(h264e_nal_escape_selftest_kernel, dim3(1), dim3(64), 0, st, dst, cap, src, n, out);
}
static void bk_launch_denoise(const uint8_t *in, const uint8_t *prev, uint8_t *out, int width, int height, hipStream_t st)
{
    const unsigned gx = (unsigned)((((width + 3) >> 2) + 255) >> 8);
    hipLaunchKernelGGL(h264e_denoise_kernel, dim3(gx, (unsigned)height, 3), dim3(256), 0, st, in, prev, out, width, height);
}
/* planar RGB by sample type: the 8-bit kernel K8, or the float kernel KF<H264E_SAMPLE_*>, 256 lanes per workgroup */
#define LAUNCH_BY_SAMPLE(sample, K8, KF, grid, st, ...) do { \
    if ((sample) == H264E_SAMPLE_F16) hipLaunchKernelGGL(KF<H264E_SAMPLE_F16>, grid, dim3(256), 0, st, __VA_ARGS__); \
    else if ((sample) == H264E_SAMPLE_BF16) hipLaunchKernelGGL(KF<H264E_SAMPLE_BF16>, grid, dim3(256), 0, st, __VA_ARGS__); \
    else if ((sample) == H264E_SAMPLE_F32) hipLaunchKernelGGL(KF<H264E_SAMPLE_F32>, grid, dim3(256), 0, st, __VA_ARGS__); \
    else hipLaunchKernelGGL(K8, grid, dim3(256), 0, st, __VA_ARGS__); } while (0)
static void bk_launch_ingest(const h264e_ingest_src_t &S, uint8_t *dst, hipStream_t st)
{
    const unsigned gx = (unsigned)((((S.width + 3) >> 2) + 255) >> 8);
    if (S.c422)
    {
        const dim3 grid(gx, (unsigned)S.height, 2);
#define LAUNCH_422(PACK) do { if (S.depth) hipLaunchKernelGGL((h264e_ingest_422_kernel<2, PACK>), grid, dim3(256), 0, st, S, dst); \
                              else hipLaunchKernelGGL((h264e_ingest_422_kernel<1, PACK>), grid, dim3(256), 0, st, S, dst); } while (0)
        if (S.pack == H264E_PACK_YUYV) LAUNCH_422(H264E_PACK_YUYV);
        else if (S.pack == H264E_PACK_UYVY) LAUNCH_422(H264E_PACK_UYVY);
        else LAUNCH_422(H264E_PACK_NONE);
#undef LAUNCH_422
        return;
    }
    if (S.depth || S.c444)
    {
        const dim3 grid(gx, (unsigned)S.height, 2);
        if (!S.depth) hipLaunchKernelGGL((h264e_ingest_hbd_kernel<1, 1>), grid, dim3(256), 0, st, S, dst);
        else if (S.c444) hipLaunchKernelGGL((h264e_ingest_hbd_kernel<2, 1>), grid, dim3(256), 0, st, S, dst);
        else hipLaunchKernelGGL((h264e_ingest_hbd_kernel<2, 0>), grid, dim3(256), 0, st, S, dst);
        return;
    }
    LAUNCH_BY_SAMPLE(S.sample, h264e_ingest_kernel, h264e_ingest_float_kernel, dim3(gx, (unsigned)S.height, 2), st, S, dst);
}
static void bk_launch_tonemap(const h264e_tonemap_src_t &S, uint8_t *dst, hipStream_t st)
{
    const dim3 grid((unsigned)((((S.width + 3) >> 2) + 255) >> 8), (unsigned)(((S.height >> 1) + TM_WG_ROWS - 1)/TM_WG_ROWS), 1);
    if (S.format == H264E_INGEST_NV12) hipLaunchKernelGGL(h264e_tonemap_kernel<H264E_INGEST_NV12>, grid, dim3(256), 0, st, S, dst);
    else hipLaunchKernelGGL(h264e_tonemap_kernel<H264E_INGEST_I420>, grid, dim3(256), 0, st, S, dst);
}
static void bk_launch_egress(const h264e_egress_dst_t &D, const uint8_t *src, hipStream_t st)
{
    const unsigned gx = (unsigned)((((D.width + 3) >> 2) + 255) >> 8);
    const int rgb = D.format == H264E_INGEST_RGB || D.format == H264E_INGEST_RGBP;
    LAUNCH_BY_SAMPLE(D.sample, h264e_egress_kernel, h264e_egress_float_kernel, dim3(gx, (unsigned)(rgb ? D.height >> 1 : D.height), rgb ? 1 : 2), st, D, src);
}
static void bk_launch_scale(const h264e_scale_src_t &S, uint8_t *dst, hipStream_t st)
{
    if (S.c422)
    {
        const dim3 grid((unsigned)((S.dw + SCL_TW - 1)/SCL_TW), (unsigned)S.tiles_y, 3);
        if (S.depth) hipLaunchKernelGGL(h264e_scale_422_kernel<2>, grid, dim3(256), 0, st, S, dst);
        else hipLaunchKernelGGL(h264e_scale_422_kernel<1>, grid, dim3(256), 0, st, S, dst);
        return;
    }
    if (S.depth || S.c444)
    {
        const dim3 grid((unsigned)((S.dw + SCL_TW - 1)/SCL_TW), (unsigned)S.tiles_y, 3);
        if (S.depth) hipLaunchKernelGGL(h264e_scale_hbd_kernel<2>, grid, dim3(256), 0, st, S, dst);
        else hipLaunchKernelGGL(h264e_scale_hbd_kernel<1>, grid, dim3(256), 0, st, S, dst);
        return;
    }
    hipLaunchKernelGGL(h264e_scale_kernel, dim3((unsigned)((S.dw + SCL_TW - 1)/SCL_TW), (unsigned)((S.dh + S.th - 1)/S.th), 3), dim3(256), 0, st, S, dst);
}
static void bk_launch_scale_rgb(const h264e_scale_src_t &S, uint8_t *dst, hipStream_t st)
{
    LAUNCH_BY_SAMPLE(S.sample, h264e_scale_rgb_kernel, h264e_scale_rgb_float_kernel, dim3((unsigned)((S.dw + SCL_TW - 1)/SCL_TW), (unsigned)((S.dh + S.th - 1)/S.th), 1), st, S, dst);
}
/* one workgroup per chunk, at most 256 (one per CU): at most 256 adders per record word, 254 at 1080p */
static void bk_launch_scenecut(const uint8_t *luma, uint32_t nbytes, int *record, hipStream_t st)
{
    const uint32_t ndw = (nbytes + 9) >> 2, per_wg = 256*SCENECUT_UNROLL;
    uint32_t wgs = (ndw + per_wg - 1)/per_wg;
    if (wgs > 256) wgs = 256;
    hipLaunchKernelGGL(h264e_scenecut_kernel, dim3(wgs ? wgs : 1), dim3(256), 0, st, luma, nbytes, record);
}
/* one workgroup per 32 blocks, at most 1024 (8K: 4 passes each) */
static void bk_launch_lookahead(const lookahead_args_t &A, hipStream_t st)
{
    int wgs = (A.nblk + 31)/32;
    if (wgs > 1024) wgs = 1024;
    hipLaunchKernelGGL(h264e_lookahead_kernel, dim3((unsigned)(wgs > 0 ? wgs : 1)), dim3(256), 0, st, A);
}
/* one single-wave workgroup per strip of 8 blocks of a block row (1080p: 8 x 67) */
static void bk_launch_lookahead_search(const lookahead_search_args_t &S, hipStream_t st)
{
    hipLaunchKernelGGL(h264e_lookahead_search_kernel, dim3((unsigned)((S.a.nbx + LOOKAHEAD_SEARCH_STRIP - 1)/LOOKAHEAD_SEARCH_STRIP), (unsigned)S.nby), dim3(64), 0, st, S);
}
/* one single-wave workgroup per 8 blocks (1080p: 503) */
static void bk_launch_lookahead_tree(const lookahead_tree_args_t &T, hipStream_t st)
{
    hipLaunchKernelGGL(h264e_lookahead_tree_kernel, dim3((unsigned)((T.nblk + LOOKAHEAD_TREE_WAVE_BLOCKS - 1)/LOOKAHEAD_TREE_WAVE_BLOCKS)), dim3(64), 0, st, T);
}
static void bk_launch_stage_selftest(int stage, const uint8_t *in, const int *args, uint8_t *out, hipStream_t st)
{
    hipLaunchKernelGGL(h264e_stage_selftest_kernel, dim3(1), dim3(64), 0, st, stage, in, args, out);
}
static void bk_launch_finalizer_selftest(const h264e_geom_t &G, const h264e_frame_task_t *task, int mode, const int *args, const int32_t *in, int32_t *hdr, mv32 *traj, hipStream_t st)
{
    hipLaunchKernelGGL(h264e_finalizer_selftest_kernel, dim3(1), dim3(64), 0, st, G, task, mode, args, in, hdr, traj);
}
/* n frames x planes (3, or 1 for a plane pair) in one launch, then the means */
static void bk_launch_ssim(const h264e_ssim_args_t &A, int n, int planes, hipStream_t st)
{
    if (planes == 3)
    {
        hipLaunchKernelGGL(h264e_ssim_kernel<3>, dim3((unsigned)A.max_tiles, (unsigned)n, 3), dim3(256), 0, st, A);
        hipLaunchKernelGGL(h264e_ssim_mean_kernel<3>, dim3((unsigned)n, 3), dim3(256), 0, st, A);
    } else
    {
        hipLaunchKernelGGL(h264e_ssim_kernel<1>, dim3((unsigned)A.max_tiles, (unsigned)n, 1), dim3(256), 0, st, A);
        hipLaunchKernelGGL(h264e_ssim_mean_kernel<1>, dim3((unsigned)n, 1), dim3(256), 0, st, A);
    }
}
/* (the last launch here: its kernels are instantiated, and so emitted, behind all the others) */
static void bk_launch_mcdenoise(const mcdenoise_args_t &A, int mode, hipStream_t st)
{
    const dim3 grid((unsigned)((A.width + 15)/16), (unsigned)((A.height + 15)/16));
    if (mode == 2) hipLaunchKernelGGL(h264e_mcdenoise_kernel<2>, grid, dim3(64), 0, st, A);
    else hipLaunchKernelGGL(h264e_mcdenoise_kernel<1>, grid, dim3(64), 0, st, A);
}

#include "h264e_pool.h"
