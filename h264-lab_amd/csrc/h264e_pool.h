/*
 * h264e_pool.h -- host side of the device boundary (include/h264e_hip.h): pools, launch groups, submits, results.
 *
 * Written ONCE against the HIP runtime API and five launch functions (bk_launch_mb, bk_launch_synth, bk_launch_ssd,
 * bk_launch_nal_selftest, bk_launch_stage_selftest) that the including translation unit defines in front of it (the product also
 * defines bk_launch_denoise, bk_launch_ingest, bk_launch_tonemap, bk_launch_egress, bk_launch_scale, bk_launch_scale_rgb, bk_launch_scenecut, bk_launch_lookahead, bk_launch_lookahead_search, bk_launch_lookahead_tree, bk_launch_mcdenoise, bk_launch_ssim and bk_launch_finalizer_selftest; the emulation's versions of those thirteen are lane loops in this file):
 *   - h264e_kernels.hip : the product -- the real HIP runtime, the kernels launched with hipLaunchKernelGGL;
 *   - tests/emu/emu_backend.cpp : the test-only emulation -- a host-memory stand-in for the handful of runtime calls used here
 *     (tests/emu/emu_hip.h) and launch functions that run the same kernel sources as lane loops, row after row.
 * Nothing in this file knows which of the two it is compiled into.
 */
#ifndef H264E_POOL_H
#define H264E_POOL_H
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

/* The matrix rows (tests/color_model.py): Kr / Kb scaled by 219/255 and 224/255 (limited) or 1 (full), times 256,
 * rounded; one coefficient per row moved by 1 so that luma sums to 220 or 256 and chroma to 0 -- grey stays neutral.  Full-range chroma:
 * the 0.5 weight is 127, not 128 (128 gives 256 for a saturated blue or red), and the nearer of the other two takes the 1, so that no
 * result leaves 8 bits for any input (tests/test_color_model.py, all 2^24).  Index 2*bt709 + full_range; [0] is the matrix the project had. */
static const h264e_color_t k_color_rows[4] = {
    { { 66, 129, 25 }, { -38, -74, 112 }, { 112, -94, -18 }, 16 },
    { { 77, 150, 29 }, { -43, -84, 127 }, { 127, -107, -20 }, 0 },
    { { 47, 157, 16 }, { -26, -86, 112 }, { 112, -102, -10 }, 16 },
    { { 54, 183, 19 }, { -29, -98, 127 }, { 127, -116, -11 }, 0 } };

/* ... and their inverses for the way out (enc_egress.h, DESIGN.md 4.5g, tests/egress_model.py): ky = 256 or 256*255/219; rv = 2(1 - Kr),
 * gu = -2 Kb (1 - Kb)/Kg, gv = -2 Kr (1 - Kr)/Kg, bu = 2(1 - Kb), times 256, or 256*255/224 for limited range; rounded.  Same index. */
static const h264e_icolor_t k_icolor_rows[4] = {
    { 298, 16, 409, -100, -208, 516 },
    { 256, 0, 359, -88, -183, 454 },
    { 298, 16, 459, -55, -136, 541 },
    { 256, 0, 403, -48, -120, 475 } };

static thread_local char g_err[256];       /* per calling thread */
#define FAIL(...) do { snprintf(g_err, sizeof(g_err), __VA_ARGS__); return -1; } while (0)
extern "C" const char *h264e_hip_last_error(void) { return g_err; }

/* ------------------------------------------------------------------ host side: pool */

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) FAIL("%s: %s", #x, hipGetErrorString(e_)); } while (0)
static int dev_malloc(void **p, size_t n) { return hipMalloc(p, n ? n : 1) == hipSuccess ? 0 : -1; }
static void dev_free(void *p) { if (p) (void)hipFree(p); }

/* pinned, device-mapped, coherent host memory: the kernel writes results here while it runs, the host polls it */
static int host_malloc(void **p, size_t n)
{
    if (hipHostMalloc(p, n ? n : 1, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return -1;
    memset(*p, 0, n ? n : 1);
    return 0;
}
static void host_free(void *p) { if (p) (void)hipHostFree(p); }

#define TASK_RING 128
static int imin_h(int a, int b) { return a < b ? a : b; }

/* One launch at a time per device, process-wide.  The macroblock kernel's forward-progress argument (every workgroup waits for
 * workgroups dispatched before it, which are resident or finished) assumes the launch has the device's wave slots to itself: two
 * such launches side by side can fill the slots with waiting workgroups of one while the workgroups they wait for sit undispatched
 * behind the other's (measured: "bounded spin expired" with 3-4 concurrent clip encoders, tools/multi_clip_probe.py).  A pool takes
 * its device's token with its first submit and gives it back when its launches have drained (h264e_hip_sync / release / destroy). */
#include <pthread.h>
#include <stdarg.h>
#define H264E_MAX_DEVICES 64
/* a token, not a mutex: a launch group takes it on the thread that launches the merged grid and gives it back on whichever member
 * thread sees the launch drained -- a pthread mutex may only be unlocked by the thread that locked it */
static pthread_mutex_t g_device_mu = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t g_device_cv = PTHREAD_COND_INITIALIZER;
static int g_device_held[H264E_MAX_DEVICES];
static void device_token_take(int device)
{
    const unsigned d = (unsigned)device % H264E_MAX_DEVICES;
    pthread_mutex_lock(&g_device_mu);
    while (g_device_held[d]) pthread_cond_wait(&g_device_cv, &g_device_mu);
    g_device_held[d] = 1;
    pthread_mutex_unlock(&g_device_mu);
}
static void device_token_give(int device)
{
    const unsigned d = (unsigned)device % H264E_MAX_DEVICES;
    pthread_mutex_lock(&g_device_mu);
    g_device_held[d] = 0;
    pthread_cond_broadcast(&g_device_cv);
    pthread_mutex_unlock(&g_device_mu);
}

/*
 * One encoder PROCESS per device.  The launch lock above only orders the launches of one process; a second process on the same GPU
 * would put its persistent launches next to ours (bounded spins expire, launches are repeated: slow, never wrong).  The first pool a
 * process creates on a device therefore takes an advisory lock on a file named after the device's PCI bus id and keeps it until its
 * last pool on that device is gone; a second process fails fast with a message that says who holds the device.
 * H264E_SHARE_DEVICE=1 skips the guard (e.g. to run two small encoders side by side on purpose).
 */
#include <errno.h>
#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>
static pthread_mutex_t g_guard_mu = PTHREAD_MUTEX_INITIALIZER;
static int g_guard_fd[H264E_MAX_DEVICES], g_guard_pools[H264E_MAX_DEVICES], g_guard_init;
static int process_guard_acquire(int device)
{
    const char *share = getenv("H264E_SHARE_DEVICE");
    int rc = 0;
    if ((share && atoi(share) == 1) || device < 0 || device >= H264E_MAX_DEVICES) return 0;
    pthread_mutex_lock(&g_guard_mu);
    if (!g_guard_init) { for (int i = 0; i < H264E_MAX_DEVICES; i++) g_guard_fd[i] = -1; g_guard_init = 1; }
    if (g_guard_pools[device]++ == 0)
    {
        char bus[64] = "", path[160];
        if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess || !bus[0]) snprintf(bus, sizeof(bus), "dev%d", device);
        for (char *q = bus; *q; q++) if (*q == ':' || *q == '.' || *q == '/') *q = '_';
        snprintf(path, sizeof(path), "%s/h264e_mi355x_%s.lock", getenv("H264E_LOCK_DIR") ? getenv("H264E_LOCK_DIR") : "/tmp", bus);
        /* O_CLOEXEC: the lock must not leak into fork+exec children (the device would stay "in use" while an unrelated child lives);
         * O_NOFOLLOW: a planted symlink is refused, not followed and truncated; the file is made world-usable so that another user's
         * encoder can take the same lock -- and when it still cannot be opened for that reason, somebody else's encoder owns it */
        int fd = open(path, O_RDWR | O_CREAT | O_CLOEXEC | O_NOFOLLOW, 0666);
        if (fd >= 0) (void)fchmod(fd, 0666);
        if (fd < 0 && (errno == EACCES || errno == EPERM)) fd = open(path, O_RDONLY | O_CLOEXEC | O_NOFOLLOW);      /* flock needs no write access */
        if (fd >= 0)
        {
            if (flock(fd, LOCK_EX | LOCK_NB))
            {
                char who[32] = "";
                const ssize_t n = read(fd, who, sizeof(who) - 1);
                if (n > 0) { who[n] = 0; for (char *q = who; *q; q++) if (*q == '\n') *q = 0; }
                snprintf(g_err, sizeof(g_err), "device %d (%s) is in use by another encoder process (pid %s): the macroblock kernel needs the device's wave slots to itself -- "
                         "give each process its own GPU, or encode several streams in ONE process (H264E_clip_encode_multi); H264E_SHARE_DEVICE=1 overrides", device, bus, who[0] ? who : "?");
                close(fd);
                g_guard_pools[device]--;
                rc = -1;
            } else
            {
                char me[32];
                const int n = snprintf(me, sizeof(me), "%ld\n", (long)getpid());
                if (ftruncate(fd, 0) == 0 && write(fd, me, (size_t)n) != n) { /* the pid is informational (and not writable through a read-only descriptor) */ }
                g_guard_fd[device] = fd;
            }
        } else if (errno == EACCES || errno == EPERM)
        {
            snprintf(g_err, sizeof(g_err), "device %d: lock file %.100s belongs to another user (their encoder owns the device); H264E_SHARE_DEVICE=1 overrides", device, path);
            g_guard_pools[device]--;
            rc = -1;
        } else if (errno != ENOENT && errno != ENOTDIR)
        {
            snprintf(g_err, sizeof(g_err), "device %d: cannot open lock file %.100s: %.40s (see H264E_LOCK_DIR, H264E_SHARE_DEVICE)", device, path, strerror(errno));
            g_guard_pools[device]--;
            rc = -1;
        }       /* (no lock directory at all: no guard) */
    }
    pthread_mutex_unlock(&g_guard_mu);
    return rc;
}
static void process_guard_release(int device)
{
    if (device < 0 || device >= H264E_MAX_DEVICES) return;
    pthread_mutex_lock(&g_guard_mu);
    if (g_guard_init && g_guard_pools[device] > 0 && --g_guard_pools[device] == 0 && g_guard_fd[device] >= 0) { close(g_guard_fd[device]); g_guard_fd[device] = -1; }
    pthread_mutex_unlock(&g_guard_mu);
}

struct h264e_hip_group;
typedef struct h264e_hip_group h264e_hip_group_t;

struct h264e_hip_pool
{
    int device, nchains, frames_resident;
    h264e_geom_t G;
    size_t frame_bytes;
    uint8_t *clip;                       /* device: resident input frames, packed I420 */
    /* temporal denoiser (h264e_hip_denoise_*): denoised frames parallel to `clip` (slot i = the denoised input slot i), then the zero
     * state; a single-slot pool ping-pongs two frames instead (den_flip: the current one).  NULL until the denoiser is switched on. */
    uint8_t *den;
    int den_frames, den_flip;
    hipEvent_t ev_copy;                  /* the copy stream's uploads, waited for by the launches of a frame pass (wait_for_copy_stream) */
    hipEvent_t ev_pass[2];               /* around the launches of one synchronous pass call, scene-cut or cost pass (their HIP-event time) */
    int *sc_rec;                         /* device [frames_resident][64]: luma histogram records of the scene-cut detector; NULL until it is switched on */
    /* cost pass of the lookahead rate control (enc_lookahead.h); NULL until it first runs */
    uint8_t *la_lo;                      /* device [la_entries][la_entry_bytes]: the half-resolution pictures, frame f in entry f % la_entries */
    unsigned long long *la_rec;          /* device [la_entries][3]: I, P, N of the frame in that entry */
    int la_entries; size_t la_entry_bytes;
    uint32_t *la_field;                  /* device [la_entries][nblk]: the motion fields of the pass with search (enc_lookahead_search.h); NULL until it first runs */
    /* cost tree over the field (enc_lookahead_tree.h): what every block received, a ring beside la_field with the same entries and
     * indexing, and the frames' sums; NULL until it first runs */
    unsigned long long *la_tree;         /* device [la_entries][nblk] */
    unsigned long long *la_tree_sum;     /* device [la_entries] */
    h264e_color_t cm;                    /* the RGB -> YCbCr matrix of the RGB / RGBP ingest and scale launches (h264e_hip_set_color) */
    /* HDR10 input (enc_tonemap.h, h264e_hip_tonemap_set): while tm_on, 16-bit I420 / NV12 device frames are tone-mapped on their way in */
    int tm_on;
    float *tm_tables;                    /* device [TM_TABLE_FLOATS]: eotf, scale, thresh; NULL until tone mapping is first switched on */
    uint8_t *tm_scratch;                 /* device: the tone-mapped window of a scaled frame, packed 8-bit I420; NULL until the first one, grows with the largest window */
    size_t tm_scratch_bytes;
    hipEvent_t ev_ingest[2];             /* what a device-input ingest waits for: the producer's stream, this pool's own stream */
    hipEvent_t ev_in[2];                 /* h264e_hip_copy_timer_*: around a caller's launches on the copy stream */
    h264e_icolor_t icm;                  /* the YCbCr -> RGB matrix of the RGB / RGBP egress launches: the inverse of cm (h264e_hip_set_color) */
    hipEvent_t ev_out[2];                /* h264e_hip_egress_time: around each egress launch while the timing is on */
    int out_timed; double out_ms; long long out_calls;
    /* quality metrics (h264e_hip_ssim_frames / _ssim_planes / _quality_last): one allocation that appears with the first use -- a one-entry
     * picture descriptor (quality_last), then the SSIM results and tile partials, qual_doubles of them */
    uint8_t *qual_dev; size_t qual_doubles;
    hipEvent_t ev_q[2];                  /* h264e_hip_quality_time: around the SSD launch / the SSIM launches of a call while the timing is on */
    int q_timed; double q_ssd_ms, q_ssim_ms; long long q_frames, q_ssd_frames;
    h264e_chain_dev_t *chains_host;      /* host mirror of the device descriptors */
    h264e_chain_dev_t *chains_dev;
    h264e_frame_task_t *tasks_dev;       /* ring of TASK_RING task arrays */
    h264e_frame_task_t *tasks_host;      /* [nchains] the task array of the submit being built (fill_task) */
    int *progress_all;
    int *progress_img;                   /* host image of progress_all for a submit that keeps rows (reset_progress); allocated with the first one */
    int *errflag;
    unsigned long long *mb_counter;      /* device: macroblocks reconstructed by this pool's rows, delivered or not (h264e_hip_mb_counter) */
    uint32_t *order;                     /* device [nchains*(nmby+1)] (job << 16) | row in dispatch order of the current launch shape */
    int *stepflags;                      /* device [nchains][2]: {clusters_moved, overflow} of each job, where the finalizers still write them (nobody reads them) */
    uint32_t *order_host;                /* host copy being built (build_order) */
    int order_jobs, order_narrow, order_sliced;   /* the launch shape `order` holds: jobs, window geometry, row-band slices or not (-1: none yet) */
    size_t order_count;                  /* ... and its entries = the launch's workgroups (banded orders carry padding) */
    uint8_t *order_led, *led;            /* [nchains] each: the led jobs `order` was built for (part of its cache key), and those of the launch being made (lead_jobs) */
    int key_lead;                        /* h264e_hip_set_key_lead: -1 the default budget, 0 off, N that many row workgroups */
    int led_jobs, led_rows, led_last;    /* the last launch's led key frames, their row workgroups, the last led job (-1: none) (h264e_hip_last_lead) */
    /* per chain slot: host-mapped result buffers the finalizer workgroups fill while the launch runs */
    h264e_hostdone_t *host_done;         /* [nchains] */
    uint8_t **host_rbsp;                 /* [nchains], each host_rbsp_cap bytes */
    h264e_hip_mbrec_t **host_mbrec;      /* [nchains], each nmb records */
    uint32_t host_rbsp_cap;
    int *abort_word;                     /* host-mapped: source of the host's own abort request */
    int *abort_dev;                      /* device: the word the kernel polls */
    h264e_walkrec_t *walkrec;            /* device [nchains] */
    int32_t **traj_dev;                  /* per chain: two [nmb][2] trajectory buffers behind each other */
    int *traj_cur;                       /* per chain: which of the two holds the latest device walk */
    unsigned long long *ssd_dev;         /* [nchains][3] sums of squared differences (h264e_hip_ssd_frames) */
    uint8_t *heap; size_t heap_bytes;    /* ONE device allocation; every device buffer of the pool is carved out of it */
    uint8_t *hheap; size_t hheap_bytes;  /* ONE host-mapped allocation for the streaming mirrors */
    int launch_counter;
    int holds_device;                    /* this pool has launches in flight and owns its device's launch lock */
    int *slot_launch;                    /* per chain slot: launch id of its current job */
    int32_t **clu_dev;                   /* per chain: optional per-macroblock mv_clusters array */
    int *ref_sel;                        /* per chain */
    int ring_pos, pending;
    int profile, prof_launches;
    int guarded;                         /* this pool counts in its device's process guard */
    struct h264e_hip_group *group;       /* launch group this pool's submits go through, or NULL */
    int group_round;                     /* the group round of its last submit */
    int waves;                           /* wavefronts per macroblock row forced by H264E_WAVES (1 or 2); 0 = chosen per launch (h264e_hip_submit) */
    int test_upload_fail_at, async_uploads;     /* fault injection (H264E_TEST_KNOBS): the n-th asynchronous upload of this pool fails */
    int test_keep_rows_cap;              /* H264E_TEST_KNOBS: h264e_hip_stream_rows_complete reports at most this many rows; -1 = off */
    int test_lead_resident;              /* H264E_TEST_KNOBS: the resident workgroups lead_jobs is told (small clips then have led key frames); -1 = off */
    double prof_mb_ms, prof_splice_ms;
    hipStream_t stream;
    hipStream_t copy_stream;             /* uploads that overlap with kernels on `stream` */
    hipStream_t abort_stream;            /* carries nothing but abort requests (h264e_hip_stream_abort) */
    hipEvent_t ev_t0, ev_t1, ev_prep;
    hipEvent_t ev[TASK_RING][3];         /* per pending submit: before / between / after the two kernels */
    int ev_pending;
    /* motion-compensated denoiser (enc_mcdenoise.h, h264e_hip_mcdenoise_*): its vector cells, a ring beside la_field with the same
     * entries and indexing; NULL until it first runs.  ev_mcd: around the launches of one call, read when the next call or
     * h264e_hip_mcdenoise_time asks (mcd_pending: the frames between them) */
    uint32_t *mcd_cells;
    hipEvent_t ev_mcd[2];
    int mcd_pending; double mcd_ms; long long mcd_frames;
};

/* One description of a launch, computed in ONE place from the host tasks (submit_check): what pick_variant, the dispatch order and a
 * launch group's merge need to know about it.  A group member hands its shape to the group, which merges them (shape_merge). */
typedef struct
{
    int jobs, narrow;                    /* jobs up to the last active one; their window geometry (every job of a launch has the same) */
    int forced, all_intra;               /* kernel variant forced by H264E_WAVES (0: chosen per launch); no job has anything to search */
    int sliced, parallel, tree;          /* a job has two or more row-band slices (the band policy of build_order); see pick_variant */
} launch_shape_t;

/* launch groups (see h264e_hip_group_create below) */
#define H264E_GROUP_MAX 8
struct h264e_hip_group
{
    int device, nmembers, arrived, round, failed;
    struct
    {
        h264e_hip_pool_t *pool;
        h264e_frame_task_t *tasks;       /* what the member wants launched this round: shape.jobs device jobs (owned) */
        launch_shape_t shape;
        int pending;
    } member[H264E_GROUP_MAX];
    pthread_mutex_t mu;
    pthread_cond_t cv;
    hipStream_t stream;
    hipEvent_t ev_done, ev_t0[2], ev_t1[2];     /* launch times per window geometry (a round has at most one launch of each) */
    int timed[2];                        /* which of the two launched in the last round */
    h264e_frame_task_t *tasks_dev; size_t tasks_cap;
    uint32_t *order_dev; size_t order_cap;
    int holds_device;                    /* the group's merged launch owns the device's launch token (taken at the launch, given back when it has drained) */
    char err[256];                       /* why the last round failed: every member reports it, not only the thread that launched */
};

extern "C" int h264e_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static void device_acquire(h264e_hip_pool_t *p)
{
    if (p->holds_device) return;
    device_token_take(p->device);
    p->holds_device = 1;
}
static void device_release(h264e_hip_pool_t *p)
{
    if (!p->holds_device) return;
    p->holds_device = 0;
    device_token_give(p->device);
}

extern "C" void h264e_hip_pool_destroy(h264e_hip_pool_t *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    if (p->copy_stream) (void)hipStreamSynchronize(p->copy_stream);
    if (p->abort_stream) (void)hipStreamSynchronize(p->abort_stream);
    device_release(p);
    host_free(p->hheap);
    free(p->host_rbsp); free(p->host_mbrec); free(p->slot_launch); free(p->order_host); free(p->order_led); free(p->led); free(p->progress_img); free(p->tasks_host);
    dev_free(p->heap);
    dev_free(p->den);
    dev_free(p->sc_rec);
    dev_free(p->tm_tables);
    dev_free(p->tm_scratch);
    dev_free(p->la_lo); dev_free(p->la_rec); dev_free(p->la_field); dev_free(p->la_tree); dev_free(p->la_tree_sum); dev_free(p->mcd_cells);
    dev_free(p->qual_dev);
    if (p->stream)
    {
        (void)hipEventDestroy(p->ev_q[0]); (void)hipEventDestroy(p->ev_q[1]);
        for (int i = 0; i < TASK_RING; i++) for (int k = 0; k < 3; k++) (void)hipEventDestroy(p->ev[i][k]);
        (void)hipEventDestroy(p->ev_t0); (void)hipEventDestroy(p->ev_t1); (void)hipEventDestroy(p->ev_prep); (void)hipEventDestroy(p->ev_copy);
        (void)hipEventDestroy(p->ev_ingest[0]); (void)hipEventDestroy(p->ev_ingest[1]); (void)hipEventDestroy(p->ev_in[0]); (void)hipEventDestroy(p->ev_in[1]);
        (void)hipEventDestroy(p->ev_out[0]); (void)hipEventDestroy(p->ev_out[1]);
        (void)hipEventDestroy(p->ev_pass[0]); (void)hipEventDestroy(p->ev_pass[1]);
        (void)hipEventDestroy(p->ev_mcd[0]); (void)hipEventDestroy(p->ev_mcd[1]);
        (void)hipStreamDestroy(p->stream);
        if (p->copy_stream) (void)hipStreamDestroy(p->copy_stream);
        if (p->abort_stream) (void)hipStreamDestroy(p->abort_stream);
    }
    free(p->chains_host); free(p->clu_dev); free(p->ref_sel); free(p->traj_dev); free(p->traj_cur);
    if (p->guarded) process_guard_release(p->device);
    free(p);
}

/* Dispatch order of a launch: the jobs of `nmembers` streams, member after member (member i's job j is launch job base_i + j), as
 * (job << 16) | row words sorted by the step at which the row can start when consecutive jobs of a member are consecutive frames of one
 * stream (lag*j + 2*row: a counting sort); ties go by j, then member, then row, so several streams are interleaved frame by frame.
 * Every workgroup still only waits for workgroups that precede it in this order (far reads: a bounded distance ahead).  Built for the
 * number of jobs a launch really has, so that a pool with many slots does not dispatch thousands of empty workgroups with every short
 * launch.  Pure: no pool, no runtime call, no environment.  `out` takes rows * (all jobs) words; -1 = out of host memory.
 *
 * LED jobs (`led`, one byte per launch job, NULL = none; lead_jobs chooses them): key frames further back in the launch.  A key frame's
 * row reads no reference and no candidates; it waits for the row above it in its own job and for nothing else, so its ROW workgroups
 * (row < rows - 1) sort at 2*row, as if the job stood at the launch's start, and take the wave slots that are empty while the chain in
 * front fills the pipeline.  Its FINALIZER (row == rows - 1) keeps lag*j + 2*(rows - 1): it waits for the verdict of the frame in front,
 * so it stays behind that frame's finalizer -- and exactly where it was.  Why the order is still safe:
 * - a led row waits only for the row above it, which has the smaller key; led rows wait for no workgroup that is not led, so they
 *   always run to their end and give their slots back, whatever stands behind them;
 * - every other workgroup waits for what it waited for before; of those, the rows of a led job have moved FORWARD (a P row of job j + 1
 *   and the led job's own finalizer find them earlier), everything else keeps its relative order;
 * - the far-read bound (h264e_hip_group_join: a far read waits for a workgroup at most (12 - lag) keys ahead of its own, all of which
 *   must fit the chip with it) counts workgroups between a P row and the rows of the frame it reads: taking led rows out of that
 *   stretch only shortens it, and a far read into a led key frame looks backwards.  The led rows in front hold at most the budget
 *   lead_jobs gave them, and only until they end.
 * With no led job the order is the unled one, word for word. */
#define H264E_ORDER_MAX_JOBS 65536     /* a job has 16 bits of the order word */
static int order_by_start_step(uint32_t *out, int rows, int lag, const int *member_jobs, int nmembers, const uint8_t *led)
{
    int maxjobs = 0;
    for (int i = 0; i < nmembers; i++) if (member_jobs[i] > maxjobs) maxjobs = member_jobs[i];
    if (maxjobs < 1) return 0;
    const int maxkey = lag*(maxjobs - 1) + 2*(rows - 1);
    int *start = (int *)calloc((size_t)maxkey + 2, sizeof(int));
    if (!start) return -1;
    const auto key = [&](int job, int j, int r) { return (led && led[job] && r < rows - 1) ? 2*r : lag*j + 2*r; };
    for (int i = 0, base = 0; i < nmembers; base += member_jobs[i], i++) for (int j = 0; j < member_jobs[i]; j++) for (int r = 0; r < rows; r++) start[key(base + j, j, r) + 1]++;
    for (int k = 0; k <= maxkey; k++) start[k + 1] += start[k];
    for (int j = 0; j < maxjobs; j++)
        for (int i = 0, base = 0; i < nmembers; base += member_jobs[i], i++)
            if (j < member_jobs[i])
                for (int r = 0; r < rows; r++) out[start[key(base + j, j, r)]++] = ((uint32_t)(base + j) << 16) | (uint32_t)r;
    free(start);
    return 0;
}

/* entries a launch of `jobs` jobs can take in the dispatch order (banded: eight equally long queues per job, padded) */
static size_t order_capacity(const h264e_geom_t &G, int jobs) { return (size_t)jobs*(size_t)(8*((G.nmby + 7)/8 + 1)); }

/* The second step on top of that order: 8 XCD bands (profiles/r02_xcd_bands.txt).  Workgroups are dealt round-robin over the 8 XCDs
 * (MI355X_MICROARCH.md: blocks b and b+8 share one), so the `total` words of `in` are arranged so that a macroblock row lands on the XCD
 * of its band of rows (row*8/nmby): the rows whose reference windows overlap then share an L2.  Returns the entries written to `out`
 * (order_capacity of them), 0 = out of host memory.
 * Eight queues in key order, one per XCD; slot i takes entry i / 8 of queue i % 8.  The queues are EQUALLY LONG, job by job: a band that
 * has fewer rows than the tallest one (nmby is rarely a multiple of 8; one band also carries the finalizer) is padded with entries that
 * are nobody's.  Without that the queues drift apart by a row or two per job, and because workgroups are dispatched strictly in index
 * order, an XCD whose resident workgroups all wait for rows of a queue that lags behind blocks the dispatch of exactly those rows:
 * measured as 2-4 % at 1080p with fixed bands, and as a dead launch ("bounded spin expired") once a launch is long enough -- 600 jobs
 * of 720p, CIF, or 1080p with 8 slices.
 * A LED job (order_by_start_step; `led` NULL = none) has its rows long before its finalizer, in front of earlier jobs' rows.  It takes
 * its `per` entries of every queue in two steps, so that the queues are equally long behind each: per - 1 entries with its rows (a band
 * has at most per - 1 rows; the padding again behind the job's last row of the queue), and one entry with its finalizer -- the finalizer
 * in the last band's queue, padding in the other seven. */
static size_t order_into_bands(const h264e_geom_t &G, int jobs, const uint32_t *in, int total, uint32_t *out, const uint8_t *led)
{
    const int bands = 8, per = (G.nmby + 7)/8 + 1;
    const size_t qlen = (size_t)per*jobs;
    uint32_t *q = (uint32_t *)malloc(sizeof(uint32_t)*8*qlen);
    int *fill = (int *)calloc((size_t)8*jobs, sizeof(int)), *want = (int *)calloc((size_t)8*jobs, sizeof(int));
    size_t cnt[8] = { 0 }, n = 0;
    if (!q || !fill || !want) { free(q); free(fill); free(want); return 0; }
    for (size_t i = 0; i < 8*qlen; i++) q[i] = H264E_ORDER_PAD;
    /* queue x, job j owns the entries [j*per, (j+1)*per) ... in KEY order that would interleave the jobs; so: append in key order, and
     * when a job's last entry of a queue has gone in, append its padding right behind it */
    for (int i = 0; i < total; i++)
    {
        const int row = (int)(in[i] & 0xffffu), x = (row >= G.nmby ? bands - 1 : imin_h(bands - 1, row*bands/G.nmby)) & 7;      /* band b -> XCD b % 8 */
        if (!(led && led[in[i] >> 16] && row >= G.nmby)) want[8*(in[i] >> 16) + x]++;      /* (a led job's finalizer is a step of its own) */
    }
    for (int i = 0; i < total; i++)
    {
        const int row = (int)(in[i] & 0xffffu), jb = (int)(in[i] >> 16), x = (row >= G.nmby ? bands - 1 : imin_h(bands - 1, row*bands/G.nmby)) & 7;
        const int own = (led && led[jb]) ? per - 1 : per;       /* entries per queue of the step this entry belongs to */
        if (own < per && row >= G.nmby)
        {
            /* a led job's finalizer: one entry in every queue */
            q[(size_t)x*qlen + cnt[x]] = in[i];
            for (int y = 0; y < 8; y++) cnt[y]++;
            continue;
        }
        /* a picture of fewer than 8 rows leaves queues without a row of this job: they get the job's padding with its first entry */
        if (row == 0) for (int y = 0; y < 8; y++) if (!want[8*jb + y]) cnt[y] += (size_t)own;
        q[(size_t)x*qlen + cnt[x]++] = in[i];
        if (++fill[8*jb + x] == want[8*jb + x]) cnt[x] += (size_t)(own - want[8*jb + x]);        /* the padding stays H264E_ORDER_PAD */
    }
    for (size_t k = 0; k < qlen; k++) for (int x = 0; x < 8; x++) out[n++] = q[(size_t)x*qlen + k];
    free(q); free(fill); free(want);
    return n;
}

/* The order of a pool's own launch of `jobs` jobs into p->order_host / order_count: the one-member case of order_by_start_step, then the
 * bands.  bands = 0: none; 8: banded; -1: the default policy below, or what H264E_XCD_BANDS forces.  The per-XCD queues are sized for
 * eight bands, so any other count is refused.  Fails with the error text set. */
static int build_order(h264e_hip_pool_t *p, int jobs, int narrow, int sliced, int bands, const uint8_t *led)
{
    const h264e_geom_t &G = p->G;
    const int rows = G.nmby + 1, total = jobs*rows, lag = narrow ? H264E_NARROW_FRAME_LAG : H264E_FRAME_LAG;
    /* measured (profiles/r04_xcd_bands.txt, one MI355X, padded queues): 8 bands nearly halve FETCH_SIZE everywhere (1080p: 1521 -> 830 MB per
     * launch, WRITE_SIZE 765 -> 603) -- HBM traffic nobody waits for at 2 % of the bandwidth -- and what they do to the SPEED depends on
     * what a launch is short of: single-slice streams of big pictures gain (4K +5 %, 8K +14 %: a frame's rows no longer fit the L2s at
     * random), everything else loses 1-13 % (1080p -4 %, 720p -1 %, CIF -13 %, rate control -4 %; row-band slices -9 % at every size,
     * 4K and 8K included: a slice is a band, and an XCD cannot share its slice's load with the others).  So: on for single-slice
     * launches from 4K up, H264E_XCD_BANDS=8 / 0 forces */
    if (bands < 0) bands = getenv("H264E_XCD_BANDS") ? atoi(getenv("H264E_XCD_BANDS")) : (G.nmb >= 30000 && !sliced ? 8 : 0);
    if (bands != 0 && bands != 8) FAIL("dispatch order: %d XCD bands (H264E_XCD_BANDS): only 0 and 8 are supported", bands);
    uint32_t *tmp = bands ? (uint32_t *)malloc(sizeof(uint32_t)*(size_t)total) : p->order_host;
    int rc = tmp ? order_by_start_step(tmp, rows, lag, &jobs, 1, led) : -1;
    p->order_count = (size_t)total;
    if (!rc && bands && !(p->order_count = order_into_bands(G, jobs, tmp, total, p->order_host, led))) rc = -1;
    if (bands) free(tmp);
    if (rc) FAIL("out of host memory");
    return 0;
}

extern "C" int h264e_hip_pool_create(h264e_hip_pool_t **pool, int device, int width, int height, int nchains,
                                     int frames_resident)
{
    if (!pool || width <= 0 || height <= 0 || ((width | height) & 1) || nchains <= 0 || frames_resident <= 0)
        FAIL("h264e_hip_pool_create: bad argument");
    h264e_hip_pool_t *p = (h264e_hip_pool_t *)calloc(1, sizeof(*p));
    if (!p) FAIL("out of host memory");
    p->device = device; p->nchains = nchains; p->frames_resident = frames_resident;
    h264e_geom_t &G = p->G;
    G.width = width; G.height = height;
    G.nmbx = (width + 15) >> 4; G.nmby = (height + 15) >> 4; G.nmb = G.nmbx*G.nmby;
    G.W = G.nmbx*16; G.H = G.nmby*16;
    G.cropping = !!((width | height) & 15);
    G.lim_x0 = G.lim_y0 = -14*4;                                    /* h264-lab.h:6322-6324, MV_GUARD 14 */
    G.lim_x1 = (G.W - 2)*4; G.lim_y1 = (G.H - 2)*4;
    G.row_words = G.nmbx*(H264E_ROW_BYTES_PER_MB/4);
    /* knobs for the failure-path tests only: a tiny row bit buffer (overflow), a short spin bound, a row that never publishes, an
     * asynchronous upload that fails.  They are looked at ONLY under the explicit switch H264E_TEST_KNOBS=1, so that a stray
     * H264E_TEST_* variable inherited from somebody's environment cannot make a production encode fail. */
    const int knobs = getenv("H264E_TEST_KNOBS") && atoi(getenv("H264E_TEST_KNOBS")) == 1;
    G.spin_limit = 1u << 24;
    G.test_stall_row = -1;
    G.fz_wait_all = getenv("H264E_FZ_WAIT_ALL") ? atoi(getenv("H264E_FZ_WAIT_ALL")) : 0;
    p->test_upload_fail_at = -1;
    p->test_keep_rows_cap = -1;
    p->test_lead_resident = -1;
    if (knobs)
    {
        if (getenv("H264E_TEST_LEAD_RESIDENT")) p->test_lead_resident = atoi(getenv("H264E_TEST_LEAD_RESIDENT"));
        if (getenv("H264E_TEST_KEEP_ROWS_CAP")) p->test_keep_rows_cap = atoi(getenv("H264E_TEST_KEEP_ROWS_CAP"));
        if (getenv("H264E_TEST_ROW_BYTES_PER_MB")) { const int b = atoi(getenv("H264E_TEST_ROW_BYTES_PER_MB"))/4; G.row_words = G.nmbx*(b > 1 ? b : 1); }
        if (getenv("H264E_TEST_SPIN_LIMIT")) G.spin_limit = (unsigned)atol(getenv("H264E_TEST_SPIN_LIMIT"));
        if (getenv("H264E_TEST_STALL_ROW")) G.test_stall_row = atoi(getenv("H264E_TEST_STALL_ROW"));
        if (getenv("H264E_TEST_UPLOAD_FAIL_AT")) p->test_upload_fail_at = atoi(getenv("H264E_TEST_UPLOAD_FAIL_AT"));
    }
#if defined(H264E_EMU) && defined(H264E_EMU_HANDOFFS_H)
    /* the emulation only, where its translation unit has included tests/emu/emu_handoffs.h in front of this file: the arrival order of the
     * macroblock step's wave hand-offs, and of the verdict in front of a finalizer, as scripts */
    if (emu_handoffs_configure(knobs ? getenv("H264E_EMU_HANDOFFS") : NULL)) { free(p); FAIL("H264E_EMU_HANDOFFS: unknown schedule"); }
#ifdef H264E_EMU_VERDICT_SCHEDULES       /* (its own mark, so that an emu_handoffs.h written before the verdict schedules still builds) */
    if (emu_verdict_configure(knobs ? getenv("H264E_EMU_VERDICT") : NULL)) { free(p); FAIL("H264E_EMU_VERDICT: unknown schedule"); }
#endif
#endif
    p->frame_bytes = (size_t)width*height*3/2;
    p->waves = getenv("H264E_WAVES") ? atoi(getenv("H264E_WAVES")) : 0;                  /* 1 / 2 / 3 / 4: forced (A-B measurements, tests); else chosen per launch */
    if (p->waves != 1 && p->waves != 2 && p->waves != 3 && p->waves != 4) p->waves = 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    {
        free(p);
        FAIL("no HIP device: the HIP path is mandatory (there is no CPU fallback)");
    }
    if (hipSetDevice(device) != hipSuccess) { free(p); FAIL("hipSetDevice(%d) failed", device); }
    {
        const int share = getenv("H264E_SHARE_DEVICE") && atoi(getenv("H264E_SHARE_DEVICE")) == 1;
        if (process_guard_acquire(device)) { free(p); return -1; }
        p->guarded = !share;
    }
    p->cm = k_color_rows[0]; p->icm = k_icolor_rows[0];
    if (hipStreamCreate(&p->stream) != hipSuccess || hipStreamCreate(&p->copy_stream) != hipSuccess || hipStreamCreate(&p->abort_stream) != hipSuccess) { if (p->guarded) process_guard_release(device); free(p); FAIL("hipStreamCreate failed"); }
    for (int i = 0; i < TASK_RING; i++) for (int k = 0; k < 3; k++) (void)hipEventCreate(&p->ev[i][k]);
    (void)hipEventCreate(&p->ev_t0); (void)hipEventCreate(&p->ev_t1); (void)hipEventCreate(&p->ev_prep); (void)hipEventCreate(&p->ev_copy);
    (void)hipEventCreate(&p->ev_ingest[0]); (void)hipEventCreate(&p->ev_ingest[1]); (void)hipEventCreate(&p->ev_in[0]); (void)hipEventCreate(&p->ev_in[1]);
    (void)hipEventCreate(&p->ev_out[0]); (void)hipEventCreate(&p->ev_out[1]);
    (void)hipEventCreate(&p->ev_pass[0]); (void)hipEventCreate(&p->ev_pass[1]);
    (void)hipEventCreate(&p->ev_mcd[0]); (void)hipEventCreate(&p->ev_mcd[1]);
    (void)hipEventCreate(&p->ev_q[0]); (void)hipEventCreate(&p->ev_q[1]);
    p->chains_host = (h264e_chain_dev_t *)calloc((size_t)nchains, sizeof(h264e_chain_dev_t));
    p->clu_dev = (int32_t **)calloc((size_t)nchains, sizeof(int32_t *));
    p->ref_sel = (int *)calloc((size_t)nchains, sizeof(int));
    p->traj_dev = (int32_t **)calloc((size_t)nchains, sizeof(int32_t *));
    p->traj_cur = (int *)calloc((size_t)nchains, sizeof(int));
    p->slot_launch = (int *)calloc((size_t)nchains, sizeof(int));
    p->host_rbsp = (uint8_t **)calloc((size_t)nchains, sizeof(uint8_t *));
    p->host_mbrec = (h264e_hip_mbrec_t **)calloc((size_t)nchains, sizeof(h264e_hip_mbrec_t *));
    p->tasks_host = (h264e_frame_task_t *)calloc((size_t)nchains, sizeof(h264e_frame_task_t));
    if (!p->chains_host || !p->clu_dev || !p->ref_sel || !p->traj_dev || !p->traj_cur || !p->slot_launch || !p->host_rbsp || !p->host_mbrec || !p->tasks_host)
    {
        h264e_hip_pool_destroy(p);
        FAIL("out of host memory");
    }
    int bad = 0;
    const size_t plane = (size_t)G.W*G.H*3/2;
    const uint32_t arena_cap = (uint32_t)((size_t)G.nmb*640 + 1024);
    /* host-mapped mirror per slot: sized for ordinary frames (160 B per macroblock; a 1080p key frame at QP 26 needs ~20); a
     * frame that does not fit stays in the slot's device NAL arena (worst-case size) and is fetched with a copy */
    const uint32_t nal_cap = (uint32_t)((size_t)G.nmb*660 + 4096);
    p->host_rbsp_cap = getenv("H264E_HOST_MIRROR_BYTES") ? (uint32_t)atol(getenv("H264E_HOST_MIRROR_BYTES")) : (uint32_t)((size_t)G.nmb*160 + 65536);
    if (p->host_rbsp_cap > nal_cap) p->host_rbsp_cap = nal_cap;
    /* One device allocation and one host-mapped allocation per pool, carved by a bump pointer: pass 0 sizes them, pass 1
     * hands out the pointers.  (Hundreds of separate small allocations get small page-table fragments; one large block is
     * mapped with large ones, and every macroblock touches about ten of these buffers.) */
    for (int pass = 0; pass < 2 && !bad; pass++)
    {
        size_t pos = 0, hpos = 0;
        uint8_t *base = pass ? p->heap : 0, *hbase = pass ? p->hheap : 0;
        auto carve = [&](size_t n, size_t align) -> void * { pos = (pos + align - 1) & ~(align - 1); void *r = base ? base + pos : 0; pos += n ? n : 1; return r; };
        auto hcarve = [&](size_t n) -> void * { hpos = (hpos + 255) & ~(size_t)255; void *r = hbase ? hbase + hpos : 0; hpos += n; return r; };
        p->clip = (uint8_t *)carve(p->frame_bytes*(size_t)frames_resident, 4096);
        p->chains_dev = (h264e_chain_dev_t *)carve(sizeof(h264e_chain_dev_t)*(size_t)nchains, 256);
        p->tasks_dev = (h264e_frame_task_t *)carve(sizeof(h264e_frame_task_t)*(size_t)nchains*TASK_RING, 256);
        p->progress_all = (int *)carve(sizeof(int)*2*(size_t)nchains*G.nmby, 256);     /* per slot: nmby row counters, then nmby `decided` counters */
        p->errflag = (int *)carve(sizeof(int), 256);
        p->mb_counter = (unsigned long long *)carve(sizeof(unsigned long long), 256);
        p->stepflags = (int *)carve(sizeof(int)*2*(size_t)nchains, 256);
        p->abort_dev = (int *)carve(64, 256);
        p->walkrec = (h264e_walkrec_t *)carve(sizeof(h264e_walkrec_t)*(size_t)nchains, 256);
        p->ssd_dev = (unsigned long long *)carve(sizeof(unsigned long long)*3*(size_t)nchains, 256);
        p->order = (uint32_t *)carve(sizeof(uint32_t)*order_capacity(G, nchains), 256);
        p->host_done = (h264e_hostdone_t *)hcarve(sizeof(h264e_hostdone_t)*(size_t)nchains);
        p->abort_word = (int *)hcarve(64);
        for (int c = 0; c < nchains; c++)
        {
            h264e_chain_dev_t &C = p->chains_host[c];
            uint8_t *rec = (uint8_t *)carve(2*plane, 4096);
            for (int k = 0; k < 2; k++)
            {
                C.rec[k][0] = rec + k*plane;
                C.rec[k][1] = C.rec[k][0] + (size_t)G.W*G.H;
                C.rec[k][2] = C.rec[k][1] + (size_t)G.W*G.H/4;
            }
            C.bottom = (h264e_mbbottom_t *)carve(sizeof(h264e_mbbottom_t)*(size_t)G.nmb, 256);
            C.pend = (h264e_mbpend_t *)carve(sizeof(h264e_mbpend_t)*(size_t)G.nmb, 256);
            C.progress = p->progress_all + (size_t)c*2*G.nmby;
            C.rowbits = (uint32_t *)carve(sizeof(uint32_t)*(size_t)G.nmby*G.row_words, 256);
            C.rowmeta = (h264e_rowmeta_t *)carve(sizeof(h264e_rowmeta_t)*(size_t)G.nmby, 256);
            C.mbrec = (h264e_mbrec_t *)carve(sizeof(h264e_mbrec_t)*(size_t)G.nmb, 256);
            C.arena = (uint8_t *)carve(arena_cap, 256);
            C.arena_cap = arena_cap;
            C.nal_arena = (uint8_t *)carve(nal_cap, 256);
            C.nal_cap = nal_cap;
            C.cursor = (uint32_t *)carve(16, 256);
            C.fout = (h264e_frameout_t *)carve(sizeof(h264e_frameout_t), 256);
            C.prof = (unsigned long long *)carve(sizeof(unsigned long long)*48, 256);     /* 0..31 the rows' phases, 32..47 the finalizer's */
            C.far_reads = (int *)carve(sizeof(int)*(size_t)G.nmby, 256);
            p->clu_dev[c] = (int32_t *)carve(sizeof(int32_t)*2*(size_t)G.nmb, 256);      /* per-macroblock mv_clusters array of a re-encode */
            p->traj_dev[c] = (int32_t *)carve(sizeof(int32_t)*4*(size_t)G.nmb, 256);    /* two walk trajectories (device-side validation) */
            /* one result per chain slot, exported by its frame's finalizer to these host-mapped mirrors */
            p->host_rbsp[c] = (uint8_t *)hcarve(p->host_rbsp_cap + 64);
            p->host_mbrec[c] = (h264e_hip_mbrec_t *)hcarve(sizeof(h264e_hip_mbrec_t)*(size_t)G.nmb + 64);
        }
        if (!pass)
        {
            p->heap_bytes = pos + 4096; p->hheap_bytes = hpos + 4096;
            bad |= dev_malloc((void **)&p->heap, p->heap_bytes);
            bad |= host_malloc((void **)&p->hheap, p->hheap_bytes);
        }
    }
    if (bad)
    {
        h264e_hip_pool_destroy(p);
        FAIL("device allocation failed");
    }
    (void)hipMemset(p->heap, 0, p->heap_bytes);
    if (hipMemcpy(p->chains_dev, p->chains_host, sizeof(h264e_chain_dev_t)*(size_t)nchains, hipMemcpyHostToDevice) != hipSuccess)
    {
        h264e_hip_pool_destroy(p);
        FAIL("descriptor upload failed");
    }
    p->order_host = (uint32_t *)malloc(sizeof(uint32_t)*order_capacity(G, nchains));
    p->order_led = (uint8_t *)calloc((size_t)nchains, 1); p->led = (uint8_t *)calloc((size_t)nchains, 1);
    if (!p->order_host || !p->order_led || !p->led) { h264e_hip_pool_destroy(p); FAIL("out of host memory"); }
    p->order_jobs = -1;
    p->key_lead = -1; p->led_last = -1;
    *pool = p;
    return 0;
}

extern "C" int h264e_hip_upload_i420(h264e_hip_pool_t *p, int first, int nframes, const uint8_t *host)
{
    if (!p || first < 0 || nframes < 0 || first + nframes > p->frames_resident) FAIL("upload_i420: bad range");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpyAsync(p->clip + p->frame_bytes*(size_t)first, host, p->frame_bytes*(size_t)nframes, hipMemcpyHostToDevice, p->stream));
    return 0;
}

extern "C" int h264e_hip_upload_i420_async(h264e_hip_pool_t *p, int first, int nframes, const uint8_t *host)
{
    if (!p || first < 0 || nframes < 0 || first + nframes > p->frames_resident) FAIL("upload_i420_async: bad range");
    if (p->async_uploads++ == p->test_upload_fail_at) FAIL("upload_i420_async: injected failure (H264E_TEST_UPLOAD_FAIL_AT)");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpyAsync(p->clip + p->frame_bytes*(size_t)first, host, p->frame_bytes*(size_t)nframes, hipMemcpyHostToDevice, p->copy_stream));
    return 0;
}

extern "C" int h264e_hip_upload_wait(h264e_hip_pool_t *p)
{
    if (!p) FAIL("upload_wait: null pool");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->copy_stream));
    return 0;
}

extern "C" int h264e_hip_upload_busy(h264e_hip_pool_t *p)
{
    if (!p) return 0;
    (void)hipSetDevice(p->device);
    const hipError_t e = hipStreamQuery(p->copy_stream);
    if (e == hipErrorNotReady) return 1;
    if (e != hipSuccess) FAIL("upload: %s", hipGetErrorString(e));      /* -1: the copy was lost, not finished */
    return 0;
}

extern "C" void *h264e_hip_host_alloc(size_t bytes)
{
    void *q = 0;
    return hipHostMalloc(&q, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? q : 0;
}

extern "C" void h264e_hip_host_free(void *q)
{
    if (q) (void)hipHostFree(q);
}


/* the launch against the pictures `chains` describes (the pool's own, or h264e_hip_quality_last's one-entry descriptor) */
static int ssd_run(h264e_hip_pool_t *p, int n, int in0, int in_mod, const h264e_chain_dev_t *chains, int pic0, int pic_mod, uint64_t *out)
{
    const h264e_geom_t &G = p->G;
    HIPCHK(hipMemsetAsync(p->ssd_dev, 0, sizeof(unsigned long long)*3*(size_t)n, p->stream));
    if (p->q_timed) HIPCHK(hipEventRecord(p->ev_q[0], p->stream));
    bk_launch_ssd(n, (const uint8_t *)p->clip, p->frame_bytes, G.width, G.height, in0, in_mod, chains, pic0, pic_mod, G.W, p->ssd_dev, p->stream);
    HIPCHK(hipGetLastError());
    if (p->q_timed) HIPCHK(hipEventRecord(p->ev_q[1], p->stream));
    HIPCHK(hipMemcpyAsync(out, p->ssd_dev, sizeof(unsigned long long)*3*(size_t)n, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    if (p->q_timed)
    {
        float f = 0;
        HIPCHK(hipEventElapsedTime(&f, p->ev_q[0], p->ev_q[1]));
        p->q_ssd_ms += f; p->q_ssd_frames += n;
    }
    return 0;
}

extern "C" int h264e_hip_ssd_frames(h264e_hip_pool_t *p, int n, int in0, int in_mod, int pic0, int pic_mod, uint64_t *out)
{
    if (!p || !out || n <= 0 || n > p->nchains || in_mod <= 0 || in_mod > p->frames_resident || pic_mod <= 0 || pic_mod > p->nchains) FAIL("ssd_frames: bad argument");
    HIPCHK(hipSetDevice(p->device));
    return ssd_run(p, n, in0, in_mod, (const h264e_chain_dev_t *)p->chains_dev, pic0, pic_mod, out);
}

/* ---- frame passes: one kernel launch per uploaded frame on the pool's stream, in stream order.  What they share: */
/* the inputs may have come over the copy stream (asynchronous uploads, device input): the launches wait for everything issued there */
static int wait_for_copy_stream(h264e_hip_pool_t *p)
{
    HIPCHK(hipEventRecord(p->ev_copy, p->copy_stream));
    HIPCHK(hipStreamWaitEvent(p->stream, p->ev_copy, 0));
    return 0;
}

/* A device ring of E records of `bytes` each, frame f's in entry f % E, and a call over frames [first, first + n), n <= frames_resident <= E:
 * no entry is used twice and the entries wrap at most once -- zeroed in front of the launches, copied to the host behind them, in one or two pieces */
static int ring_records_pieces(h264e_hip_pool_t *p, void *host, void *ring, size_t bytes, int E, int first, int n)
{
    for (int done = 0, run; done < n; done += run)
    {
        uint8_t *const entry = (uint8_t *)ring + bytes*(size_t)((first + done) % E);
        run = imin_h(n - done, E - (first + done) % E);
        if (!host) HIPCHK(hipMemsetAsync(entry, 0, bytes*(size_t)run, p->stream));
        else HIPCHK(hipMemcpyAsync((uint8_t *)host + bytes*(size_t)done, entry, bytes*(size_t)run, hipMemcpyDeviceToHost, p->stream));
    }
    return 0;
}
static int ring_records_zero(h264e_hip_pool_t *p, void *ring, size_t bytes, int E, int first, int n) { return ring_records_pieces(p, NULL, ring, bytes, E, first, n); }
static int ring_records_read(h264e_hip_pool_t *p, void *host, void *ring, size_t bytes, int E, int first, int n) { return ring_records_pieces(p, host, ring, bytes, E, first, n); }

/* the cost pass' block grid: 8x8 blocks of the half-resolution picture; the motion-compensated denoiser's 16x16 luma blocks are the same grid */
static int la_nbx(const h264e_hip_pool_t *p) { return (p->G.width >> 1) >> 3; }
static int la_nby(const h264e_hip_pool_t *p) { return (p->G.height >> 1) >> 3; }

/* ---- temporal denoiser (enc_denoise.h): one h264e_denoise_kernel launch per frame on the pool's stream, in stream order */

#ifdef H264E_EMU
/* the emulation's launch: the kernel's per-group code as a lane loop, plane by plane, row by row */
static void bk_launch_denoise(const uint8_t *in, const uint8_t *prev, uint8_t *out, int width, int height, hipStream_t)
{
    for (int pl = 0; pl < 3; pl++)
    {
        const int w = width >> (pl ? 1 : 0), h = height >> (pl ? 1 : 0);
        const size_t off = pl ? (size_t)width*height + (pl == 2 ? (size_t)(width/2)*(height/2) : 0) : 0;
        const int aligned = !((((uintptr_t)in + off) | ((uintptr_t)prev + off) | ((uintptr_t)out + off) | (uintptr_t)w) & 3);
        for (int y = 0; y < h; y++)
            for (int g = 0; g < (w + 3)/4; g++) denoise_group(k_denoise_gain, in + off, prev + off, out + off, w, h, g, y, aligned);
    }
}
#endif

static int den_index(const h264e_hip_pool_t *p, int slot) { return p->frames_resident == 1 ? p->den_flip : slot; }
static uint8_t *den_frame(const h264e_hip_pool_t *p, int index) { return p->den + p->frame_bytes*(size_t)index; }

/* the frame in input slot s: filtered against the denoised frame *prev -- the zero state for the first frame of a call from zero, else
 * the one in front -- into the one returned; a single-slot pool ping-pongs, and flips here */
static int den_step(h264e_hip_pool_t *p, int s, int first_from_zero, int *prev)
{
    const int R = p->frames_resident;
    *prev = first_from_zero ? p->den_frames - 1 : R == 1 ? p->den_flip : (s + R - 1) % R;
    if (R == 1) p->den_flip ^= 1;
    return den_index(p, s);
}

extern "C" int h264e_hip_denoise_reset(h264e_hip_pool_t *p)
{
    if (!p) FAIL("denoise_reset: null pool");
    HIPCHK(hipSetDevice(p->device));
    if (!p->den)
    {
        p->den_frames = (p->frames_resident == 1 ? 2 : p->frames_resident) + 1;
        if (dev_malloc((void **)&p->den, p->frame_bytes*(size_t)p->den_frames)) { p->den = 0; FAIL("denoise: device allocation failed (%d frames)", p->den_frames); }
    }
    p->den_flip = 0;
    HIPCHK(hipMemsetAsync(p->den, 0, p->frame_bytes*(size_t)p->den_frames, p->stream));
    return 0;
}

extern "C" int h264e_hip_denoise_frames(h264e_hip_pool_t *p, int first, int n, int from_zero)
{
    const int R = p ? p->frames_resident : 0;
    if (!p || !p->den || first < 0 || first >= R || n < 0 || n > R) FAIL("denoise_frames: bad argument (or the denoiser is not on)");
    if (!n) return 0;
    HIPCHK(hipSetDevice(p->device));
    if (wait_for_copy_stream(p)) return -1;
    for (int i = 0; i < n; i++)
    {
        const int s = (first + i) % R;
        int prev;
        const int out = den_step(p, s, i == 0 && from_zero, &prev);
        bk_launch_denoise(p->clip + p->frame_bytes*(size_t)s, den_frame(p, prev), den_frame(p, out), p->G.width, p->G.height, p->stream);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int h264e_hip_read_denoised(h264e_hip_pool_t *p, int slot, uint8_t *dst)
{
    if (!p || !dst || !p->den || slot < 0 || slot >= p->frames_resident) FAIL("read_denoised: bad argument (or the denoiser is not on)");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipMemcpy(dst, den_frame(p, den_index(p, slot)), p->frame_bytes, hipMemcpyDeviceToHost));
    return 0;
}

/* ---- motion-compensated denoiser (enc_mcdenoise.h): one h264e_mcdenoise_kernel launch per frame on the pool's stream, into the
 * denoised ring above, from the field ring of the searched cost pass (below) */

#ifdef H264E_EMU
/* the emulation's launch: the workgroup's code, tile after tile */
static void bk_launch_mcdenoise(const mcdenoise_args_t &A, int mode, hipStream_t)
{
    for (int by = 0; by < (A.height + 15)/16; by++)
        for (int bx = 0; bx < (A.width + 15)/16; bx++)
        {
            mcdenoise_lds_t sh;
            memset(&sh, 0, sizeof(sh));
            if (mode == 2) mcdenoise_block<2>(A, &sh, bx, by);
            else mcdenoise_block<1>(A, &sh, bx, by);
        }
}
#endif

/* the HIP-event time of the last call's launches, once they are over */
static int mcdenoise_collect(h264e_hip_pool_t *p)
{
    if (!p->mcd_pending) return 0;
    float f = 0;
    HIPCHK(hipEventSynchronize(p->ev_mcd[1]));
    HIPCHK(hipEventElapsedTime(&f, p->ev_mcd[0], p->ev_mcd[1]));
    p->mcd_ms += f; p->mcd_frames += p->mcd_pending; p->mcd_pending = 0;
    return 0;
}

/* frames first, first + 1, ... of the STREAM: input slot f % frames_resident and field entry f % la_entries, as the cost pass counts */
extern "C" int h264e_hip_mcdenoise_frames(h264e_hip_pool_t *p, int first, int n, int mode, int from_zero)
{
    const int R = p ? p->frames_resident : 0;
    if (!p || !p->den || first < 0 || n < 0 || n > R || mode < 1 || mode > 2) FAIL("mcdenoise_frames: bad argument (or the denoiser is not on)");
    if (!p->la_field) FAIL("mcdenoise_frames: no frame of this pool has a motion field (h264e_hip_lookahead_search_frames comes first)");
    if (p->G.width < MCDENOISE_MIN_SIDE || p->G.height < MCDENOISE_MIN_SIDE) FAIL("mcdenoise: pictures below %dx%d have no block (%dx%d)", MCDENOISE_MIN_SIDE, MCDENOISE_MIN_SIDE, p->G.width, p->G.height);
    if (!n) return 0;
    HIPCHK(hipSetDevice(p->device));
    mcdenoise_args_t A;
    A.width = p->G.width; A.height = p->G.height; A.nbx = la_nbx(p); A.nby = la_nby(p);
    const size_t nblk = (size_t)A.nbx*(size_t)A.nby;
    if (!p->mcd_cells && dev_malloc((void **)&p->mcd_cells, nblk*MCDENOISE_CELL_BYTES*(size_t)p->la_entries)) { p->mcd_cells = 0; FAIL("mcdenoise: device allocation failed (%d vector fields)", p->la_entries); }
    if (mcdenoise_collect(p)) return -1;
    if (wait_for_copy_stream(p)) return -1;
    HIPCHK(hipEventRecord(p->ev_mcd[0], p->stream));
    for (int i = 0; i < n; i++)
    {
        const int f = first + i, s = f % R, e = f % p->la_entries;
        int prev;
        const int out = den_step(p, s, i == 0 && from_zero, &prev);
        A.cur = p->clip + p->frame_bytes*(size_t)s; A.prev = den_frame(p, prev); A.out = den_frame(p, out);
        A.field = p->la_field + nblk*(size_t)e; A.cells = p->mcd_cells + nblk*(size_t)e;
        bk_launch_mcdenoise(A, mode, p->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->ev_mcd[1], p->stream));
    p->mcd_pending = n;
    return 0;
}

/* the vector cells of STREAM frame `frame` from its ring entry: what is there is the caller's to know */
extern "C" int h264e_hip_mcdenoise_read_vectors(h264e_hip_pool_t *p, int frame, void *dst)
{
    if (!p || !dst || frame < 0) FAIL("mcdenoise_read_vectors: bad argument");
    if (!p->mcd_cells) FAIL("mcdenoise_read_vectors: no frame has been filtered");
    HIPCHK(hipSetDevice(p->device));
    const size_t bytes = (size_t)la_nbx(p)*(size_t)la_nby(p)*MCDENOISE_CELL_BYTES;
    HIPCHK(hipMemcpyAsync(dst, (const uint8_t *)p->mcd_cells + bytes*(size_t)(frame % p->la_entries), bytes, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return 0;
}

extern "C" int h264e_hip_mcdenoise_time(h264e_hip_pool_t *p, double *kernel_ms, long long *frames)
{
    if (!p) FAIL("mcdenoise_time: null pool");
    HIPCHK(hipSetDevice(p->device));
    if (mcdenoise_collect(p)) return -1;
    if (kernel_ms) *kernel_ms = p->mcd_ms;
    if (frames) *frames = p->mcd_frames;
    return 0;
}

/* ---- scene-cut detection (enc_scenecut.h): one h264e_scenecut_kernel launch per frame on the pool's stream */

#ifdef H264E_EMU
/* the emulation's launch: the kernel's per-dword code as a lane loop over one workgroup, then its flush */
static void bk_launch_scenecut(const uint8_t *luma, uint32_t nbytes, int *record, hipStream_t)
{
    uint32_t *hist = (uint32_t *)calloc(SCENECUT_LDS_DWORDS, sizeof(uint32_t));
    if (!hist) return;
    const uint32_t ndw = scenecut_dwords(luma, nbytes);
    for (uint32_t i = 0; i < ndw; i++) scenecut_count(hist, luma, nbytes, i, scenecut_load(luma, i), (int)(i & (SCENECUT_REPLICAS - 1)));
    for (int b = 0; b < SCENECUT_BINS; b++) scenecut_flush(hist, record, b);
    free(hist);
}
#endif

extern "C" int h264e_hip_scenecut_frames(h264e_hip_pool_t *p, int first, int n, uint32_t *hist, float *kernel_ms)
{
    const int R = p ? p->frames_resident : 0;
    if (!p || !hist || first < 0 || first >= R || n < 0 || n > R) FAIL("scenecut_frames: bad argument");
    if (kernel_ms) *kernel_ms = 0;
    if (!n) return 0;
    HIPCHK(hipSetDevice(p->device));
    if (!p->sc_rec && dev_malloc((void **)&p->sc_rec, sizeof(int)*SCENECUT_BINS*(size_t)R)) { p->sc_rec = 0; FAIL("scenecut: device allocation failed (%d records)", R); }
    if (wait_for_copy_stream(p)) return -1;
    HIPCHK(hipEventRecord(p->ev_pass[0], p->stream));
    if (ring_records_zero(p, p->sc_rec, sizeof(int)*SCENECUT_BINS, R, first, n)) return -1;
    for (int i = 0; i < n; i++)
        bk_launch_scenecut(p->clip + p->frame_bytes*(size_t)((first + i) % R), (uint32_t)((size_t)p->G.width*p->G.height), p->sc_rec + (size_t)((first + i) % R)*SCENECUT_BINS, p->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->ev_pass[1], p->stream));
    if (ring_records_read(p, hist, p->sc_rec, sizeof(int)*SCENECUT_BINS, R, first, n)) return -1;
    HIPCHK(hipStreamSynchronize(p->stream));
    if (kernel_ms) HIPCHK(hipEventElapsedTime(kernel_ms, p->ev_pass[0], p->ev_pass[1]));
    return 0;
}

/* ---- cost pass of the lookahead rate control (enc_lookahead.h): one h264e_lookahead_kernel launch per frame on the pool's stream */

#ifdef H264E_EMU
/* the emulation's launch: the kernel's lane-level code as a loop over the blocks and their eight row lanes */
static void bk_launch_lookahead(const lookahead_args_t &A, hipStream_t)
{
    unsigned long long sum[3] = { 0, 0, 0 };
    for (int b = 0; b < A.nblk; b++)
    {
        lookahead_row_t R[8];
        int s = 0, intra = 0, inter = 0;
        for (int r = 0; r < 8; r++) { R[r] = lookahead_row(A, b, r); s += lookahead_row_sum(R[r]); }
        const int m = (s + 32) >> 6;
        for (int r = 0; r < 8; r++) { intra += lookahead_row_intra(R[r], m); inter += lookahead_row_inter(R[r]); }
        if (!A.prev) inter = intra;
        sum[0] += (unsigned)intra; sum[1] += (unsigned)(intra < inter ? intra : inter); sum[2] += intra < inter;
    }
    for (int k = 0; k < 3; k++) lookahead_record_add(A.record + k, sum[k]);
}
/* ... with search: strip after strip, the wave's lanes once as (block, row) and once per block as the candidates */
static void bk_launch_lookahead_search(const lookahead_search_args_t &S, hipStream_t)
{
    unsigned long long sum[3] = { 0, 0, 0 };
    const int side = 2*S.range + 1, rounds = (side*side + 63) >> 6;
    for (int by = 0; by < S.nby; by++)
        for (int bx0 = 0; bx0 < S.a.nbx; bx0 += LOOKAHEAD_SEARCH_STRIP)
        {
            lookahead_search_lds_t sh;
            const int nb = imin_h(LOOKAHEAD_SEARCH_STRIP, S.a.nbx - bx0);
            memset(&sh, 0, sizeof(sh));
            for (int i = 0; i < nb; i++)
            {
                lookahead_row_t R[8];
                int s = 0, intra = 0;
                for (int r = 0; r < 8; r++) { R[r] = lookahead_row(S.a, by*S.a.nbx + bx0 + i, r); s += lookahead_row_sum(R[r]); sh.cur[16*i + 2*r] = R[r].lo[0]; sh.cur[16*i + 2*r + 1] = R[r].lo[1]; }
                for (int r = 0; r < 8; r++) intra += lookahead_row_intra(R[r], (s + 32) >> 6);
                sh.intra[i] = intra;
            }
            if (S.a.prev) for (int c = 0; c < LOOKAHEAD_SEARCH_CELLS; c++) lookahead_search_stage(S, bx0, by, c, sh.prev);
            for (int i = 0; i < nb; i++)
            {
                const int intra = sh.intra[i];
                int key = lookahead_search_key(intra, 0, 0);
                if (S.a.prev)
                {
                    key = LOOKAHEAD_SEARCH_NO_KEY;
                    WAVE_FOR(l)
                    {
                        int cand[LOOKAHEAD_SEARCH_ROUNDS];
                        for (int k = 0; k < LOOKAHEAD_SEARCH_ROUNDS; k++) cand[k] = lookahead_search_candidate(S.range, 64*k + l);
                        key = imin_h(key, lookahead_search_lane(S, sh.prev, sh.cur, bx0 + i, by, i, cand, rounds));
                    }
                }
                const int inter = key >> 15;
                lookahead_search_field_store(S, by*S.a.nbx + bx0 + i, lookahead_search_cell(key));
                sum[0] += (unsigned)intra; sum[1] += (unsigned)(intra < inter ? intra : inter); sum[2] += intra < inter;
            }
        }
    for (int k = 0; k < 3; k++) lookahead_record_add(S.a.record + k, sum[k]);
}
/* one frame step of the cost tree: wave after wave, its lanes once as (block, row) and once as the blocks' row-0 lanes */
static void bk_launch_lookahead_tree(const lookahead_tree_args_t &T, hipStream_t)
{
    for (int b0 = 0; b0 < T.nblk; b0 += LOOKAHEAD_TREE_WAVE_BLOCKS)
    {
        lookahead_row_t R[64];
        int s[LOOKAHEAD_TREE_WAVE_BLOCKS] = { 0 }, intra[LOOKAHEAD_TREE_WAVE_BLOCKS] = { 0 };
        unsigned long long sum = 0;
        WAVE_FOR(l) if (b0 + (l >> 3) < T.nblk) { R[l] = lookahead_tree_row(T, b0 + (l >> 3), l & 7); s[l >> 3] += lookahead_row_sum(R[l]); }
        WAVE_FOR(l) if (b0 + (l >> 3) < T.nblk) intra[l >> 3] += lookahead_row_intra(R[l], (s[l >> 3] + 32) >> 6);
        WAVE_FOR(l) if (b0 + (l >> 3) < T.nblk && !(l & 7)) sum += lookahead_tree_block(T, b0 + (l >> 3), intra[l >> 3]);
        lookahead_record_add(T.sum, sum);
    }
}
#endif

/* frames first, first + 1, ... of the STREAM (input slot f % frames_resident): their records into rec [n][3] on return; range 0 = the
 * pass without search, 1..8 = h264e_lookahead_search_kernel, which also fills the frames' entries of the field ring */
static int lookahead_frames(h264e_hip_pool_t *p, int first, int n, int range, unsigned long long *rec, float *kernel_ms)
{
    const int R = p ? p->frames_resident : 0;
    if (!p || !rec || first < 0 || n < 0 || n > R || range < 0 || range > LOOKAHEAD_SEARCH_MAX_RANGE) FAIL("lookahead_frames: bad argument");
    if (p->G.width < LOOKAHEAD_MIN_SIDE || p->G.height < LOOKAHEAD_MIN_SIDE) FAIL("lookahead: pictures below %dx%d have no cost block (%dx%d)", LOOKAHEAD_MIN_SIDE, LOOKAHEAD_MIN_SIDE, p->G.width, p->G.height);
    if (kernel_ms) *kernel_ms = 0;
    if (!n) return 0;
    HIPCHK(hipSetDevice(p->device));
    lookahead_args_t A;
    A.width = p->G.width; A.nbx = la_nbx(p); A.nblk = A.nbx*la_nby(p);
    if (!p->la_lo)
    {
        p->la_entries = R > 1 ? R : 2;
        p->la_entry_bytes = (size_t)A.nblk*LOOKAHEAD_BLOCK_BYTES;
        if (dev_malloc((void **)&p->la_lo, p->la_entry_bytes*(size_t)p->la_entries)) { p->la_lo = 0; FAIL("lookahead: device allocation failed (%d half-resolution pictures)", p->la_entries); }
        if (dev_malloc((void **)&p->la_rec, sizeof(unsigned long long)*3*(size_t)p->la_entries)) { dev_free(p->la_lo); p->la_lo = 0; p->la_rec = 0; FAIL("lookahead: device allocation failed (%d records)", p->la_entries); }
    }
    if (range && !p->la_field && dev_malloc((void **)&p->la_field, (size_t)A.nblk*LOOKAHEAD_FIELD_CELL_BYTES*(size_t)p->la_entries)) { p->la_field = 0; FAIL("lookahead: device allocation failed (%d motion fields)", p->la_entries); }
    const int E = p->la_entries;
    if (wait_for_copy_stream(p)) return -1;
    HIPCHK(hipEventRecord(p->ev_pass[0], p->stream));
    if (ring_records_zero(p, p->la_rec, sizeof(unsigned long long)*3, E, first, n)) return -1;
    for (int i = 0; i < n; i++)
    {
        const int f = first + i, e = f % E;
        A.luma = p->clip + p->frame_bytes*(size_t)(f % R);
        A.prev = f ? p->la_lo + p->la_entry_bytes*(size_t)((f - 1) % E) : NULL;
        A.cur = p->la_lo + p->la_entry_bytes*(size_t)e;
        A.record = p->la_rec + 3*(size_t)e;
        if (range)
        {
            lookahead_search_args_t S;
            S.a = A; S.field = p->la_field + (size_t)A.nblk*(size_t)e; S.range = range; S.nby = la_nby(p);
            bk_launch_lookahead_search(S, p->stream);
        }
        else bk_launch_lookahead(A, p->stream);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(p->ev_pass[1], p->stream));
    if (ring_records_read(p, rec, p->la_rec, sizeof(unsigned long long)*3, E, first, n)) return -1;
    HIPCHK(hipStreamSynchronize(p->stream));
    if (kernel_ms) HIPCHK(hipEventElapsedTime(kernel_ms, p->ev_pass[0], p->ev_pass[1]));
    return 0;
}

extern "C" int h264e_hip_lookahead_frames(h264e_hip_pool_t *p, int first, int n, unsigned long long *rec, float *kernel_ms) { return lookahead_frames(p, first, n, 0, rec, kernel_ms); }

extern "C" int h264e_hip_lookahead_search_frames(h264e_hip_pool_t *p, int first, int n, int range, unsigned long long *rec, float *kernel_ms)
{
    if (range < 1) FAIL("lookahead_search_frames: bad argument");
    return lookahead_frames(p, first, n, range, rec, kernel_ms);
}

/* the field of STREAM frame `frame` from its ring entry: what is there is the caller's to know */
extern "C" int h264e_hip_lookahead_read_field(h264e_hip_pool_t *p, int frame, void *dst)
{
    if (!p || !dst || frame < 0) FAIL("lookahead_read_field: bad argument");
    if (!p->la_field) FAIL("lookahead_read_field: no frame has been analysed with a search");
    HIPCHK(hipSetDevice(p->device));
    const size_t bytes = (size_t)la_nbx(p)*(size_t)la_nby(p)*LOOKAHEAD_FIELD_CELL_BYTES;
    HIPCHK(hipMemcpyAsync(dst, (const uint8_t *)p->la_field + bytes*(size_t)(frame % p->la_entries), bytes, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return 0;
}

/* ---- cost tree over the motion field (enc_lookahead_tree.h): one h264e_lookahead_tree_kernel launch per frame on the pool's stream, in
 * REVERSE frame order: the launch of frame f reads what the launch of frame f + 1 has added */
extern "C" int h264e_hip_lookahead_tree_frames(h264e_hip_pool_t *p, int first, int n, const uint8_t *key, unsigned long long *sums, float *kernel_ms)
{
    if (!p || !key || !sums || first < 0 || n < 0) FAIL("lookahead_tree_frames: bad argument");
    if (!p->la_field) FAIL("lookahead_tree_frames: no frame of this pool has a motion field (h264e_hip_lookahead_search_frames comes first)");
    const int E = p->la_entries;
    if (n > E) FAIL("lookahead_tree_frames: %d frames do not fit the field ring (%d entries)", n, E);
    if (kernel_ms) *kernel_ms = 0;
    if (!n) return 0;
    HIPCHK(hipSetDevice(p->device));
    lookahead_tree_args_t T;
    T.nbx = la_nbx(p); T.nby = la_nby(p); T.nblk = T.nbx*T.nby;
    const size_t nblk = (size_t)T.nblk;
    if (!p->la_tree)
    {
        if (dev_malloc((void **)&p->la_tree, nblk*LOOKAHEAD_TREE_CELL_BYTES*(size_t)E)) { p->la_tree = 0; FAIL("lookahead_tree: device allocation failed (%d block maps)", E); }
        if (dev_malloc((void **)&p->la_tree_sum, sizeof(unsigned long long)*(size_t)E)) { dev_free(p->la_tree); p->la_tree = 0; p->la_tree_sum = 0; FAIL("lookahead_tree: device allocation failed (%d sums)", E); }
    }
    HIPCHK(hipEventRecord(p->ev_pass[0], p->stream));
    if (ring_records_zero(p, p->la_tree, nblk*LOOKAHEAD_TREE_CELL_BYTES, E, first, n) || ring_records_zero(p, p->la_tree_sum, sizeof(unsigned long long), E, first, n)) return -1;
    for (int i = n - 1; i >= 0; i--)
    {
        const int f = first + i, e = f % E;
        T.lo = p->la_lo + p->la_entry_bytes*(size_t)e;
        T.field = p->la_field + nblk*(size_t)e;
        T.in = p->la_tree + nblk*(size_t)e;
        T.out = i && !key[i] ? p->la_tree + nblk*(size_t)((f - 1) % E) : NULL;
        T.sum = p->la_tree_sum + e;
        bk_launch_lookahead_tree(T, p->stream);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(p->ev_pass[1], p->stream));
    if (ring_records_read(p, sums, p->la_tree_sum, sizeof(unsigned long long), E, first, n)) return -1;
    HIPCHK(hipStreamSynchronize(p->stream));
    for (int i = 0; i < n; i++) if (sums[i] > LOOKAHEAD_TREE_SUM_MAX) sums[i] = LOOKAHEAD_TREE_SUM_MAX;
    if (kernel_ms) HIPCHK(hipEventElapsedTime(kernel_ms, p->ev_pass[0], p->ev_pass[1]));
    return 0;
}

/* the block map of STREAM frame `frame` from its ring entry: what is there is the caller's to know */
extern "C" int h264e_hip_lookahead_read_tree(h264e_hip_pool_t *p, int frame, void *dst)
{
    if (!p || !dst || frame < 0) FAIL("lookahead_read_tree: bad argument");
    if (!p->la_field) FAIL("lookahead_read_tree: no frame of this pool has a motion field (h264e_hip_lookahead_search_frames comes first)");
    if (!p->la_tree) FAIL("lookahead_read_tree: no cost tree has been run");
    HIPCHK(hipSetDevice(p->device));
    const size_t bytes = (size_t)la_nbx(p)*(size_t)la_nby(p)*LOOKAHEAD_TREE_CELL_BYTES;
    HIPCHK(hipMemcpyAsync(dst, (const uint8_t *)p->la_tree + bytes*(size_t)(frame % p->la_entries), bytes, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return 0;
}

extern "C" int h264e_hip_read_recon_slot(h264e_hip_pool_t *p, int slot, uint8_t *dst)
{
    if (!p || !dst || slot < 0 || slot >= p->nchains) FAIL("read_recon_slot: bad argument");
    const size_t n = (size_t)p->G.W*p->G.H*3/2;
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpy(dst, p->chains_host[slot].rec[0][0], n, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int h264e_hip_upload_planes(h264e_hip_pool_t *p, int index, const uint8_t *const yuv[3], const int stride[3])
{
    if (!p || index < 0 || index >= p->frames_resident) FAIL("upload_planes: bad index");
    uint8_t *d = p->clip + p->frame_bytes*(size_t)index;
    for (int c = 0; c < 3; c++)
    {
        const int w = p->G.width >> (c ? 1 : 0), h = p->G.height >> (c ? 1 : 0);
        HIPCHK(hipSetDevice(p->device));
        HIPCHK(hipMemcpy2DAsync(d, (size_t)w, yuv[c], (size_t)stride[c], (size_t)w, (size_t)h, hipMemcpyHostToDevice, p->stream));
        d += (size_t)w*h;
    }
    return 0;
}

/* ---- device-resident input (enc_ingest.h): one h264e_ingest_kernel launch per frame on the pool's copy stream, where the asynchronous
 * uploads are ordered too, so that it overlaps with a macroblock launch on the encode stream like they do */

#ifdef H264E_EMU
/* the emulation's launch: the kernel's per-group code as a lane loop, row by row */
/* ST = H264E_SAMPLE_*: the 8-bit code, or the float kernels' (one dispatch per launch: EMU_BY_SAMPLE) */
#define EMU_BY_SAMPLE(sample, F, ...) do { \
    if ((sample) == H264E_SAMPLE_F16) F<H264E_SAMPLE_F16>(__VA_ARGS__); else if ((sample) == H264E_SAMPLE_BF16) F<H264E_SAMPLE_BF16>(__VA_ARGS__); \
    else if ((sample) == H264E_SAMPLE_F32) F<H264E_SAMPLE_F32>(__VA_ARGS__); else F<H264E_SAMPLE_U8>(__VA_ARGS__); } while (0)
template <int ST> static void emu_ingest(const h264e_ingest_src_t &S, uint8_t *dst)
{
    for (int y = 0; y < S.height; y++)
        for (int g = 0; g < (S.width + 3)/4; g++)
        {
            if constexpr (ST == H264E_SAMPLE_U8) { ingest_luma(S, dst, g, y); ingest_chroma(S, dst, g, y); }
            else { ingest_float_luma<ST>(S, dst, g, y); ingest_float_chroma<ST>(S, dst, g, y); }
        }
}
/* ... of 16-bit samples and / or 4:4:4 chroma (enc_hbd.h) */
template <int SB, int C444> static void emu_ingest_hbd(const h264e_ingest_src_t &S, uint8_t *dst)
{
    for (int y = 0; y < S.height; y++)
        for (int g = 0; g < (S.width + 3)/4; g++) { ingest_hbd_luma<SB>(S, dst, g, y); ingest_hbd_chroma<SB, C444>(S, dst, g, y); }
}
/* ... of 4:2:2 sources (enc_422.h) */
template <int SB, int PACK> static void emu_ingest_422(const h264e_ingest_src_t &S, uint8_t *dst)
{
    for (int y = 0; y < S.height; y++)
        for (int g = 0; g < (S.width + 3)/4; g++) { ingest_422_luma<SB, PACK>(S, dst, g, y); ingest_422_chroma<SB, PACK>(S, dst, g, y); }
}
template <int SB> static void emu_ingest_422_by_pack(const h264e_ingest_src_t &S, uint8_t *dst)
{
    if (S.pack == H264E_PACK_YUYV) emu_ingest_422<SB, H264E_PACK_YUYV>(S, dst);
    else if (S.pack == H264E_PACK_UYVY) emu_ingest_422<SB, H264E_PACK_UYVY>(S, dst);
    else emu_ingest_422<SB, H264E_PACK_NONE>(S, dst);
}
static void bk_launch_ingest(const h264e_ingest_src_t &S, uint8_t *dst, hipStream_t)
{
    if (S.c422) { if (S.depth) emu_ingest_422_by_pack<2>(S, dst); else emu_ingest_422_by_pack<1>(S, dst); }
    else if (S.depth && S.c444) emu_ingest_hbd<2, 1>(S, dst);
    else if (S.depth) emu_ingest_hbd<2, 0>(S, dst);
    else if (S.c444) emu_ingest_hbd<1, 1>(S, dst);
    else EMU_BY_SAMPLE(S.sample, emu_ingest, S, dst);
}
/* ... and the egress's (enc_egress.h): the same, per part */
template <int ST> static void emu_egress(const h264e_egress_dst_t &D, const uint8_t *src)
{
    const int rgb = D.format == H264E_INGEST_RGB || D.format == H264E_INGEST_RGBP;
    for (int part = 0; part < (rgb ? 1 : 2); part++)
        for (int y = 0; y < (rgb ? D.height >> 1 : D.height); y++)
            for (int g = 0; g < (D.width + 3)/4; g++)
            {
                if constexpr (ST == H264E_SAMPLE_U8) egress_group(D, src, g, y, part); else egress_rgb<0, ST>(D, src, g, y);
            }
}
/* HDR10 input (enc_tonemap.h): the tables staged as the kernel's 256 lanes stage them, then one lane per group of every row pair */
static void bk_launch_tonemap(const h264e_tonemap_src_t &S, uint8_t *dst, hipStream_t)
{
    float *L = (float *)malloc(sizeof(float)*TM_TABLE_FLOATS);
    if (!L) return;
    memset(L, 0xEE, sizeof(float)*TM_TABLE_FLOATS);
    for (int t = 0; t < 256; t++) tm_stage(L, S.tables, t);
    for (int j = 0; j < S.height/2; j++)
        for (int g = 0; g < (S.width + 3)/4; g++) tonemap_group(S, L, dst, g, j);
    free(L);
}
static void bk_launch_egress(const h264e_egress_dst_t &D, const uint8_t *src, hipStream_t) { EMU_BY_SAMPLE(D.sample, emu_egress, D, src); }
/* ... and the scaler's (enc_scale.h): tile by tile, each of the kernel's three steps as a lane loop over the tile's LDS */
static void bk_launch_scale(const h264e_scale_src_t &S, uint8_t *dst, hipStream_t)
{
    ScaleLds *L = (ScaleLds *)malloc(sizeof(ScaleLds));
    if (!L) return;
    if (S.c422)                         /* enc_422.h: the kernel's choice of horizontal pass */
    {
        for (int comp = 0; comp < 3; comp++)
            for (int ty = 0; ty < S.tiles_y; ty++)
                for (int tx = 0; tx < (S.dw + SCL_TW - 1)/SCL_TW; tx++)
                {
                    ScaleTile T;
                    if (!scale_tile_422(S, comp, tx, ty, T)) continue;
                    memset(L, 0xEE, sizeof(*L));
                    for (int t = 0; t < 256; t++) scale_tables(L, T, t);
                    const int items = scale_src_rows(L, T) << 6;
                    for (int it = 0; it < items; it++)
                    {
                        if (S.depth) scale_hpass_hbd(L, S.c[comp], T, S.qround, S.qshift, it);
                        else if (S.pack) scale_hpass_pk(L, S.c[comp], T, it);
                        else scale_hpass(L, S.c[comp], T, it);
                    }
                    for (int it = 0; it < T.nrows*16; it++) scale_vpass(L, T, dst + scale_plane_offset(S, comp), it);
                }
        free(L);
        return;
    }
    if (S.depth || S.c444)              /* enc_hbd.h: a source geometry per plane, 16-bit taps quantised by the horizontal pass */
    {
        for (int comp = 0; comp < 3; comp++)
            for (int ty = 0; ty < S.tiles_y; ty++)
                for (int tx = 0; tx < (S.dw + SCL_TW - 1)/SCL_TW; tx++)
                {
                    ScaleTile T;
                    if (!scale_tile_hbd(S, comp, tx, ty, T)) continue;
                    memset(L, 0xEE, sizeof(*L));
                    for (int t = 0; t < 256; t++) scale_tables(L, T, t);
                    const int items = scale_src_rows(L, T) << 6;
                    for (int it = 0; it < items; it++)
                    {
                        if (S.depth) scale_hpass_hbd(L, S.c[comp], T, S.qround, S.qshift, it); else scale_hpass(L, S.c[comp], T, it);
                    }
                    for (int it = 0; it < T.nrows*16; it++) scale_vpass(L, T, dst + scale_plane_offset(S, comp), it);
                }
        free(L);
        return;
    }
    for (int comp = 0; comp < 3; comp++)
        for (int ty = 0; ty < (S.dh + S.th - 1)/S.th; ty++)
            for (int tx = 0; tx < (S.dw + SCL_TW - 1)/SCL_TW; tx++)
            {
                ScaleTile T;
                if (!scale_tile(S, comp, tx, ty, T)) continue;
                memset(L, 0xEE, sizeof(*L));
                for (int t = 0; t < 256; t++) scale_tables(L, T, t);
                const int items = scale_src_rows(L, T) << 6;
                for (int it = 0; it < items; it++) scale_hpass(L, S.c[comp], T, it);
                for (int it = 0; it < T.nrows*16; it++) scale_vpass(L, T, dst + scale_plane_offset(S, comp), it);
            }
    free(L);
}
/* ... and the planar RGB scaler's (enc_scale_rgb.h): per tile the taps, per channel the two passes into the LDS tile, then the conversion */
template <int ST> static void emu_scale_rgb(const h264e_scale_src_t &S, uint8_t *dst)
{
    ScaleRgbLds *L = (ScaleRgbLds *)malloc(sizeof(ScaleRgbLds));
    if (!L) return;
    for (int ty = 0; ty < (S.dh + S.th - 1)/S.th; ty++)
        for (int tx = 0; tx < (S.dw + SCL_TW - 1)/SCL_TW; tx++)
        {
            ScaleTile T;
            if (!scale_tile(S, 0, tx, ty, T)) continue;
            memset(L, 0xEE, sizeof(*L));
            for (int t = 0; t < 256; t++) scale_tables(&L->s, T, t);
            const int items = scale_src_rows(&L->s, T) << 6;
            for (int ch = 0; ch < 3; ch++)
            {
                for (int it = 0; it < items; it++)
                {
                    if constexpr (ST == H264E_SAMPLE_U8) scale_hpass(&L->s, S.c[ch], T, it); else scale_hpass_float<ST>(&L->s, S.c[ch], T, it);
                }
                for (int it = 0; it < T.nrows*16; it++) scale_rgb_vpass(L, T, ch, it);
            }
            for (int it = 0; it < scale_rgb_items(T); it++) scale_rgb_convert(S.cm, L, T, dst, it);
        }
    free(L);
}
static void bk_launch_scale_rgb(const h264e_scale_src_t &S, uint8_t *dst, hipStream_t) { EMU_BY_SAMPLE(S.sample, emu_scale_rgb, S, dst); }
#else
/* the product refuses what the runtime does not know as device memory of this pool's device, and a plane that does not lie inside ONE
 * allocation from its first to its last byte: a host address or a read beyond the allocation is a memory fault in the kernel, not an
 * error code (the kernel itself only sees raw addresses) */
static int ingest_is_device_memory(const h264e_hip_pool_t *p, const void *q, size_t nbytes)
{
    hipPointerAttribute_t a;
    hipDeviceptr_t base = 0;
    size_t size = 0;
    memset(&a, 0, sizeof(a));
    if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void)hipGetLastError(); return 0; }
    if (a.type != hipMemoryTypeDevice || a.device != p->device) return 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)q) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return (const char *)q >= (const char *)base && (const char *)q + nbytes <= (const char *)base + size;
}
#endif

/* H264E_dev_frame_t.format: the layout in bits 0-1, the sample type in bits 4-5 (planar RGB only) and, on the way in alone (hbd != NULL),
 * the depth of 16-bit samples in bits 8-11 (depth - 8: I420 and NV12), 4:4:4 chroma in bit 12 (I420), 4:2:2 chroma in bit 14 (I420 and
 * NV12) and its packed orders in bits 2-3 (I420 | 4:2:2); nothing else.  *sb = a sample's bytes, hbd[0] = the depth (0: 8-bit samples),
 * hbd[1] = 4:4:4, hbd[2] = 4:2:2, hbd[3] = H264E_PACK_* */
#define H264E_SAMPLE_U16 4              /* the name of a 16-bit sample in the messages */
static const char *const k_format_names[4] = { "I420", "NV12", "RGB", "RGBP" }, *const k_sample_names[5] = { "u8", "f16", "bf16", "f32", "u16" },
                  *const k_pack_names[3] = { "", "YUYV", "UYVY" };
static int dev_format_split(const char *who, int format, int *base, int *sample, int *sb, int *hbd)
{
    const int dcode = hbd ? (format >> 8) & 15 : 0, c444 = hbd ? (format >> 12) & 1 : 0, c422 = hbd ? (format >> 14) & 1 : 0, pk = hbd ? (format >> 2) & 3 : 0;
    if (format & ~(hbd ? 0x5f3f : 0x33) || dcode > 8) FAIL("%s: unknown format %d", who, format);
    *base = format & 3; *sample = (format >> 4) & 3;
    if (hbd)
    {
        hbd[0] = dcode ? dcode + 8 : 0; hbd[1] = c444; hbd[2] = c422; hbd[3] = pk;
        if (dcode && *sample)
            FAIL("%s: format %d asks for both %d-bit integer samples (0x%x) and %s samples (0x%x) of %s (format %d): one sample type", who, format, dcode + 8, dcode << 8,
                 k_sample_names[*sample], *sample << 4, k_format_names[*base], *base);
        if ((dcode || c444) && (*base == H264E_INGEST_RGB || *base == H264E_INGEST_RGBP))
            FAIL("%s: format %d asks for %s of %s (format %d): 16-bit samples are I420 and NV12 only, 4:4:4 chroma I420 only", who, format,
                 dcode ? "16-bit samples" : "4:4:4 chroma", k_format_names[*base], *base);
        if (c444 && *base == H264E_INGEST_NV12)
            FAIL("%s: format %d asks for 4:4:4 chroma (0x1000) of NV12 (format %d): 4:4:4 is three planes, I420 (format %d) only", who, format, *base, H264E_INGEST_I420);
        if (pk == 3) FAIL("%s: format %d sets both pack bits (0xc): one order of the packed samples, YUYV (0x4) or UYVY (0x8)", who, format);
        if (pk && !c422)
            FAIL("%s: unknown format %d: packed %s samples (0x%x) come with 4:2:2 chroma (0x4000) alone", who, format, k_pack_names[pk], pk << 2);
        if (c422 && c444) FAIL("%s: format %d asks for both 4:2:2 chroma (0x4000) and 4:4:4 chroma (0x1000): one chroma geometry", who, format);
        if (c422 && *sample)
            FAIL("%s: format %d asks for 4:2:2 chroma (0x4000) of %s samples (0x%x): 4:2:2 takes 8-bit samples or 16-bit integer words", who, format, k_sample_names[*sample], *sample << 4);
        if (c422 && (*base == H264E_INGEST_RGB || *base == H264E_INGEST_RGBP))
            FAIL("%s: format %d asks for %s of %s (format %d): 4:2:2 chroma is I420 and NV12 only, packed samples I420 only", who, format,
                 pk ? "packed 4:2:2 samples" : "4:2:2 chroma", k_format_names[*base], *base);
        if (pk && *base == H264E_INGEST_NV12)
            FAIL("%s: format %d asks for packed %s samples (0x%x) of NV12 (format %d): a packed frame is one plane, on I420 (format %d) only", who, format, k_pack_names[pk], pk << 2,
                 *base, H264E_INGEST_I420);
    }
    *sb = *sample == H264E_SAMPLE_F32 ? 4 : *sample || dcode ? 2 : 1;
    if (*sample && *base != H264E_INGEST_RGBP)
        FAIL("%s: format %d asks for %s samples (0x%x) of %s (format %d): float samples are planar RGB (format %d) only", who, format, k_sample_names[*sample], *sample << 4,
             k_format_names[*base], *base, H264E_INGEST_RGBP);
    return 0;
}
/* float planes: every pointer and stride a multiple of the sample's bytes (what the kernels' loads and stores rest on) */
static int dev_sample_aligned(const char *who, int k, const void *plane, int stride, int sb, int sample)
{
    if (sb == 2 && !sample) sample = H264E_SAMPLE_U16;
    if ((uintptr_t)plane % (unsigned)sb) FAIL("%s: plane %d (%p) is not a multiple of the %d bytes of a %s sample", who, k, plane, sb, k_sample_names[sample]);
    if (stride % sb) FAIL("%s: stride %d of plane %d is not a multiple of the %d bytes of a %s sample", who, stride, k, sb, k_sample_names[sample]);
    return 0;
}

extern "C" int h264e_hip_set_color(h264e_hip_pool_t *p, int bt709, int full_range)
{
    if (!p || (unsigned)bt709 > 1 || (unsigned)full_range > 1) FAIL("set_color: bad argument");
    p->cm = k_color_rows[2*bt709 + full_range];
    p->icm = k_icolor_rows[2*bt709 + full_range];
    return 0;
}

/* ---- HDR10 input (enc_tonemap.h): a setting of the pool.  The tables go to the device when it is switched on (the buffer appears with
 * the first time); switching it off keeps the buffer and launches what the pool launched before */
extern "C" int h264e_hip_tonemap_tables(int transfer, int curve, double peak_nits, double ref_white_nits, int ycc[8], float eotf[1024], float scale[1024], float thresh[256])
{
    float t[TM_TABLE_FLOATS];
    if (!ycc || !eotf || !scale || !thresh) FAIL("tonemap_tables: null argument");
    if (tonemap_params("tonemap_tables", transfer, curve, &peak_nits, &ref_white_nits, g_err, sizeof(g_err))) return -1;
    tonemap_tables(curve, peak_nits, ref_white_nits, ycc, t);
    memcpy(eotf, t + TM_EOTF, sizeof(float)*1024); memcpy(scale, t + TM_SCALE, sizeof(float)*1024); memcpy(thresh, t + TM_THRESH, sizeof(float)*256);
    return 0;
}

/* the refusals of the parameters alone (0 = they would be accepted) */
extern "C" int h264e_hip_tonemap_check(const char *who, int transfer, int curve, double peak_nits, double ref_white_nits)
{
    return tonemap_params(who ? who : "set_tonemap", transfer, curve, &peak_nits, &ref_white_nits, g_err, sizeof(g_err));
}

extern "C" int h264e_hip_tonemap_set(h264e_hip_pool_t *p, const char *who, int transfer, int curve, double peak_nits, double ref_white_nits)
{
    float t[TM_TABLE_FLOATS];
    int ycc[8];
    if (!p) FAIL("%s: null argument", who ? who : "set_tonemap");
    if (tonemap_params(who ? who : "set_tonemap", transfer, curve, &peak_nits, &ref_white_nits, g_err, sizeof(g_err))) return -1;
    if (transfer == H264E_TM_OFF) { p->tm_on = 0; return 0; }
    HIPCHK(hipSetDevice(p->device));
    tonemap_tables(curve, peak_nits, ref_white_nits, ycc, t);
    if (!p->tm_tables && dev_malloc((void **)&p->tm_tables, sizeof(t))) { p->tm_tables = 0; FAIL("%s: device allocation failed (%zu bytes)", who ? who : "set_tonemap", sizeof(t)); }
    HIPCHK(hipStreamSynchronize(p->copy_stream));           /* a launch of the tables' earlier contents has read them */
    HIPCHK(hipMemcpy(p->tm_tables, t, sizeof(t), hipMemcpyHostToDevice));
    p->tm_on = 1;
    return 0;
}

/* state[0] = on, state[1] = bytes of the device table buffer (0: none), state[2] = bytes of the scratch surface (0: none) */
extern "C" int h264e_hip_tonemap_state(const h264e_hip_pool_t *p, long long state[3])
{
    if (!p || !state) FAIL("tonemap_state: null argument");
    state[0] = p->tm_on; state[1] = p->tm_tables ? (long long)(sizeof(float)*TM_TABLE_FLOATS) : 0; state[2] = p->tm_scratch ? (long long)p->tm_scratch_bytes : 0;
    return 0;
}

/* while tone mapping is on a device frame is HDR10: 16-bit words of 10 .. 16 significant bits in the I420 or NV12 layout, 4:2:0 */
static int tonemap_format_refused(const char *who, int dev_format, int format, int sample, const int *hbd)
{
    char what[64];
    if (format == H264E_INGEST_RGB || format == H264E_INGEST_RGBP) snprintf(what, sizeof(what), "%s%s%s", k_format_names[format], sample ? " of " : "", sample ? k_sample_names[sample] : "");
    else if (hbd[2]) snprintf(what, sizeof(what), "4:2:2 %s%s", hbd[3] ? "packed " : k_format_names[format], hbd[3] ? k_pack_names[hbd[3]] : "");
    else if (hbd[1]) snprintf(what, sizeof(what), "4:4:4 %s", k_format_names[format]);
    else if (!hbd[0]) snprintf(what, sizeof(what), "8-bit %s", k_format_names[format]);
    else if (hbd[0] < 10) snprintf(what, sizeof(what), "%s of depth %d", k_format_names[format], hbd[0]);
    else return 0;
    FAIL("%s: format %d is %s, but tone mapping is on: HDR10 frames are I420 or NV12 (P010 / P016) with H264E_DEV_DEPTH(10 .. 16)", who, dev_format, what);
}

/* the tone-map kernel's view of a w x h picture whose planes begin at plane[] (a frame, or the window of one) */
static void tonemap_src(const h264e_hip_pool_t *p, int format, int depth, const uint8_t *const plane[3], const int stride[3], int w, int h, h264e_tonemap_src_t *T)
{
    memset(T, 0, sizeof(*T));
    for (int k = 0; k < (format == H264E_INGEST_NV12 ? 2 : 3); k++) { T->plane[k] = plane[k]; T->stride[k] = stride[k]; }
    T->format = format; T->width = w; T->height = h;
    T->qshift = depth - 10; T->qround = T->qshift ? 1 << (T->qshift - 1) : 0;
    T->cm = p->cm; T->tables = p->tm_tables;
}

/* everything that is refused, without a launch; fills the kernel's view of the source */
static int ingest_check(const h264e_hip_pool_t *p, int slot, int dev_format, const void *const planes[3], const int strides[3], int pixel_bytes, h264e_ingest_src_t *S)
{
    int format, sample, sb, hbd[4];
    if (!p || !planes || !strides) FAIL("ingest_device: null argument");
    if (slot < 0 || slot >= p->frames_resident) FAIL("ingest_device: slot %d outside the %d resident frames", slot, p->frames_resident);
    if (dev_format_split("ingest_device", dev_format, &format, &sample, &sb, hbd)) return -1;
    if (format == H264E_INGEST_RGB && pixel_bytes != 3 && pixel_bytes != 4) FAIL("ingest_device: RGB pixels of %d bytes (3 or 4)", pixel_bytes);
    if (p->tm_on && tonemap_format_refused("ingest_device", dev_format, format, sample, hbd)) return -1;
    memset(S, 0, sizeof(*S));
    S->format = format; S->pixel_bytes = format == H264E_INGEST_RGB ? pixel_bytes : 1; S->sample = sample;
    S->width = p->G.width; S->height = p->G.height;
    S->cm = p->cm;
    S->depth = hbd[0]; S->c444 = hbd[1]; S->c422 = hbd[2]; S->pack = hbd[3];
    if (hbd[0]) { S->qround = 1 << (hbd[0] - 9); S->qshift = hbd[0] - 8; }
    const int nplanes = hbd[3] ? 1 : format == H264E_INGEST_I420 || format == H264E_INGEST_RGBP ? 3 : format == H264E_INGEST_NV12 ? 2 : 1;
    for (int k = 0; k < nplanes; k++)
    {
        /* bytes and rows of source plane k: RGB pixels; full-size luma, R, G, B and 4:4:4 chroma planes (sb bytes per sample); half-size chroma (NV12: U,V pairs, so `width` samples again);
         * a packed 4:2:2 row holds two samples per pixel; 4:2:2 chroma planes have all the rows */
        const int row_bytes = format == H264E_INGEST_RGB ? S->width*pixel_bytes : hbd[3] ? 2*S->width*sb
                            : (k == 0 || format == H264E_INGEST_NV12 || format == H264E_INGEST_RGBP || hbd[1]) ? S->width*sb : (S->width/2)*sb;
        if (!planes[k]) FAIL("ingest_device: plane %d is NULL", k);
        if (dev_sample_aligned("ingest_device", k, planes[k], strides[k], sb, sample)) return -1;
        if (strides[k] < row_bytes) FAIL("ingest_device: stride %d of plane %d is below its %d row bytes", strides[k], k, row_bytes);
#ifndef H264E_EMU
        const int rows = k == 0 || format == H264E_INGEST_RGBP || hbd[1] || hbd[2] ? S->height : S->height/2;
        const void *q = planes[k];
        if (!ingest_is_device_memory(p, q, (size_t)(rows - 1)*(size_t)strides[k] + (size_t)row_bytes))
            FAIL("ingest_device: plane %d (%p, %d rows %d bytes apart) is not memory of device %d, or not inside one allocation", k, planes[k], rows, strides[k], p->device);
#endif
        S->plane[k] = (const uint8_t *)planes[k]; S->stride[k] = strides[k];
    }
    return 0;
}

extern "C" int h264e_hip_ingest_check(h264e_hip_pool_t *p, int slot, int format, const void *const planes[3], const int strides[3], int pixel_bytes)
{
    h264e_ingest_src_t S;
    if (p) (void)hipSetDevice(p->device);
    return ingest_check(p, slot, format, planes, strides, pixel_bytes, &S);
}

/* the checks, then the launch on the copy stream behind (a) everything queued on the producer's stream so far and (b), while no macroblock
 * launch of this pool is in flight, everything queued on the pool's own stream (h264e_hip_upload_i420 / upload_planes / generate_synth
 * into the same slot).  A launch in flight does not read the slot: the caller keeps the bounded-ring rule of H264E_clip_upload. */
/* the copy stream waits for the producer's stream and, while no launch is in flight, for the pool's own */
static int ingest_order(h264e_hip_pool_t *p, void *producer_stream)
{
    if (producer_stream)
    {
        HIPCHK(hipEventRecord(p->ev_ingest[0], (hipStream_t)producer_stream));
        HIPCHK(hipStreamWaitEvent(p->copy_stream, p->ev_ingest[0], 0));
    }
    if (!p->pending)
    {
        HIPCHK(hipEventRecord(p->ev_ingest[1], p->stream));
        HIPCHK(hipStreamWaitEvent(p->copy_stream, p->ev_ingest[1], 0));
    }
    return 0;
}

static int ingest_enqueue(h264e_hip_pool_t *p, int slot, int format, const void *const planes[3], const int strides[3], int pixel_bytes, void *producer_stream)
{
    h264e_ingest_src_t S;
    if (p) HIPCHK(hipSetDevice(p->device));
    if (ingest_check(p, slot, format, planes, strides, pixel_bytes, &S)) return -1;
    if (ingest_order(p, producer_stream)) return -1;
    if (p->tm_on)                       /* enc_tonemap.h: the checked frame is HDR10 */
    {
        h264e_tonemap_src_t T;
        tonemap_src(p, S.format, S.depth, S.plane, S.stride, S.width, S.height, &T);
        bk_launch_tonemap(T, p->clip + p->frame_bytes*(size_t)slot, p->copy_stream);
    }
    else bk_launch_ingest(S, p->clip + p->frame_bytes*(size_t)slot, p->copy_stream);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int h264e_hip_ingest_device_async(h264e_hip_pool_t *p, int slot, int format, const void *const planes[3], const int strides[3], int pixel_bytes, void *producer_stream)
{
    return ingest_enqueue(p, slot, format, planes, strides, pixel_bytes, producer_stream);
}

extern "C" int h264e_hip_ingest_device(h264e_hip_pool_t *p, int slot, int format, const void *const planes[3], const int strides[3], int pixel_bytes, void *producer_stream)
{
    if (ingest_enqueue(p, slot, format, planes, strides, pixel_bytes, producer_stream)) return -1;
    HIPCHK(hipStreamSynchronize(p->copy_stream));
    return 0;
}

/* ---- device-resident input of another size (enc_scale.h, enc_scale_rgb.h): one h264e_scale_kernel or h264e_scale_rgb_kernel launch per frame,
 * ordered like the ingest */

/* everything that is refused, without a launch; fills the kernel's view of the source.  win = {src_width, src_height, crop_x, crop_y,
 * crop_width, crop_height}, crop_width 0 = the whole source.  Plane extents come from the SOURCE size and the window: what must be
 * device memory inside one allocation is [the window's first byte, the last byte of its last row] of every plane. */
static int scale_check(const h264e_hip_pool_t *p, int tm, int slot, int dev_format, const void *const planes[3], const int strides[3], const int *win, h264e_scale_src_t *S)
{
    int format, sample, sb, hbd[4];
    if (!p || !planes || !strides || !win) FAIL("scale_device: null argument");
    if (slot < 0 || slot >= p->frames_resident) FAIL("scale_device: slot %d outside the %d resident frames", slot, p->frames_resident);
    if (dev_format_split("scale_device", dev_format, &format, &sample, &sb, hbd)) return -1;
    if (tm && tonemap_format_refused("scale_device", dev_format, format, sample, hbd)) return -1;
    if (format == H264E_INGEST_RGB) FAIL("scale_device: interleaved RGB (format %d) cannot be combined with a window: convert at the picture's size, or hand over planar RGB (format %d), I420 or NV12", format, H264E_INGEST_RGBP);
    const int srcw = win[0], srch = win[1], dw = p->G.width, dh = p->G.height;
    if (srcw <= 0 || srch <= 0) FAIL("scale_device: source of %d x %d samples", srcw, srch);
    const int cx = win[4] ? win[2] : 0, cy = win[4] ? win[3] : 0, sw = win[4] ? win[4] : srcw, sh = win[4] ? win[5] : srch;
    if (cx < 0 || (cx & 1)) FAIL("scale_device: crop_x %d (even, not negative)", cx);
    if (cy < 0 || (cy & 1)) FAIL("scale_device: crop_y %d (even, not negative)", cy);
    if (sw <= 0 || (sw & 1)) FAIL("scale_device: window width %d (even, positive)", sw);
    if (sh <= 0 || (sh & 1)) FAIL("scale_device: window height %d (even, positive)", sh);
    if (sw > SCL_MAX_DIM) FAIL("scale_device: window width %d above %d", sw, SCL_MAX_DIM);
    if (sh > SCL_MAX_DIM) FAIL("scale_device: window height %d above %d", sh, SCL_MAX_DIM);
    if (cx > srcw - sw) FAIL("scale_device: window columns %d..%d leave the source's %d", cx, cx + sw - 1, srcw);
    if (cy > srch - sh) FAIL("scale_device: window rows %d..%d leave the source's %d", cy, cy + sh - 1, srch);
    if (sw < dw) FAIL("scale_device: window width %d below the picture's %d (no upscaling)", sw, dw);
    if (sh < dh) FAIL("scale_device: window height %d below the picture's %d (no upscaling)", sh, dh);
    if (sw > SCL_MAX_RATIO*dw) FAIL("scale_device: window width %d is more than %d times the picture's %d", sw, SCL_MAX_RATIO, dw);
    if (sh > SCL_MAX_RATIO*dh) FAIL("scale_device: window height %d is more than %d times the picture's %d", sh, SCL_MAX_RATIO, dh);
    /* a 4:4:4 chroma plane goes from the luma's window to half the picture: no plane by more than SCL_MAX_RATIO */
    if (hbd[1] && sw > SCL_MAX_RATIO/2*dw)
        FAIL("scale_device: 4:4:4 window width %d is more than %d times the picture's %d (its chroma planes are reduced to %d columns: at most %d to 1)", sw, SCL_MAX_RATIO/2, dw, dw/2, SCL_MAX_RATIO);
    if (hbd[1] && sh > SCL_MAX_RATIO/2*dh)
        FAIL("scale_device: 4:4:4 window height %d is more than %d times the picture's %d (its chroma planes are reduced to %d rows: at most %d to 1)", sh, SCL_MAX_RATIO/2, dh, dh/2, SCL_MAX_RATIO);
    /* a 4:2:2 chroma plane goes from half the window's width and all of its height to half the picture: 16:1 in width as it is, 8:1 in height */
    if (hbd[2] && sh > SCL_MAX_RATIO/2*dh)
        FAIL("scale_device: 4:2:2 window height %d is more than %d times the picture's %d (its chroma planes are reduced to %d rows: at most %d to 1)", sh, SCL_MAX_RATIO/2, dh, dh/2, SCL_MAX_RATIO);
    memset(S, 0, sizeof(*S));
    S->sw = sw; S->sh = sh; S->dw = dw; S->dh = dh;
    S->cm = p->cm; S->sample = sample;
    S->th = (int)((long long)(SCL_ROWS - 2)*dh/sh);            /* th*sh/dh + 2 source rows at most: <= SCL_ROWS */
    if (S->th > SCL_TH_MAX) S->th = SCL_TH_MAX;
    const int rgbp = format == H264E_INGEST_RGBP;
    if (rgbp) S->th &= ~1;                                      /* a tile of all three output planes: whole 2x2 blocks (>= 4 rows at 16:1) */
    S->depth = hbd[0]; S->c444 = hbd[1]; S->c422 = hbd[2]; S->pack = hbd[3];
    if (hbd[0]) { S->qround = 1 << (hbd[0] - 9); S->qshift = hbd[0] - 8; }
    S->thc = (int)((long long)(SCL_ROWS - 2)*(dh/2)/sh);        /* 4:4:4 and 4:2:2 chroma: sh rows -> dh/2, so thc*sh/(dh/2) + 2 source rows at most (>= 4 rows at 8:1) */
    if (S->thc > SCL_TH_MAX) S->thc = SCL_TH_MAX;
    S->tiles_y = (dh + S->th - 1)/S->th;
    if ((hbd[1] || hbd[2]) && (dh/2 + S->thc - 1)/S->thc > S->tiles_y) S->tiles_y = (dh/2 + S->thc - 1)/S->thc;
    const int nplanes = hbd[3] ? 1 : format == H264E_INGEST_NV12 ? 2 : 3, cw = (srcw + 1)/2;
    for (int k = 0; k < nplanes; k++)
    {
        /* bytes of a source row, and the window in this plane: x0 bytes into row y0, wbytes x rows (planar RGB: every plane as luma, sb bytes per sample;
         * a packed 4:2:2 plane: two samples per pixel; 4:2:2 chroma: all the window's rows) */
        const int nv = k && format == H264E_INGEST_NV12, full = k == 0 || rgbp || hbd[1], pk = hbd[3];
        const int row_bytes = pk ? 2*srcw*sb : full ? srcw*sb : nv ? 2*cw*sb : cw*sb;
        const int x0 = pk ? 2*cx*sb : full ? cx*sb : nv ? cx*sb : cx/2*sb, y0 = full || hbd[2] ? cy : cy/2;
        const int wbytes = pk ? 2*sw*sb : full ? sw*sb : nv ? sw*sb : sw/2*sb, rows = full || hbd[2] ? sh : sh/2;
        if (!planes[k]) FAIL("scale_device: plane %d is NULL", k);
        if (dev_sample_aligned("scale_device", k, planes[k], strides[k], sb, sample)) return -1;
        if (strides[k] < row_bytes) FAIL("scale_device: stride %d of plane %d is below the %d bytes of a source row", strides[k], k, row_bytes);
        const uint8_t *lo = (const uint8_t *)planes[k] + (size_t)y0*(size_t)strides[k] + (size_t)x0;
        const size_t nbytes = (size_t)(rows - 1)*(size_t)strides[k] + (size_t)wbytes;
#ifndef H264E_EMU
        if (!ingest_is_device_memory(p, lo, nbytes))
            FAIL("scale_device: plane %d (%p, source %d x %d, window %d x %d at (%d, %d), rows %d bytes apart) is not memory of device %d, or not inside one allocation",
                 k, planes[k], srcw, srch, sw, sh, cx, cy, strides[k], p->device);
#endif
        for (int c = k; c < (pk || nv ? 3 : k + 1); c++)
        {
            /* a packed group of four samples: Y0 U Y1 V (YUYV) or U Y0 V Y1 (UYVY) */
            const int at = !pk ? (nv && c == 2 ? 1 : 0) : pk == H264E_PACK_YUYV ? (c == 0 ? 0 : c == 1 ? 1 : 3) : (c == 0 ? 1 : c == 1 ? 0 : 2);
            S->c[c].base = lo + at*sb; S->c[c].lo = lo; S->c[c].hi = lo + nbytes;
            S->c[c].stride = strides[k]; S->c[c].step = pk ? (c ? 4*sb : 2*sb) : nv ? 2*sb : sb;
        }
    }
    return 0;
}

extern "C" int h264e_hip_scale_check(h264e_hip_pool_t *p, int slot, int format, const void *const planes[3], const int strides[3], const int *win)
{
    h264e_scale_src_t S;
    if (p) (void)hipSetDevice(p->device);
    return scale_check(p, p ? p->tm_on : 0, slot, format, planes, strides, win, &S);
}

/* HDR10 input through a window (enc_tonemap.h): S is the checked 16-bit source.  Its window is tone-mapped at the source's resolution into
 * the pool's scratch surface, an 8-bit packed I420 picture of the window's size, and the existing scale kernel runs from there as for
 * any I420 source of that size: two launches on the copy stream, one behind the other, so the surface is reused frame after frame */
static int tonemap_scale(h264e_hip_pool_t *p, int slot, int dev_format, const h264e_scale_src_t &S, void *producer_stream)
{
    const size_t need = (size_t)S.sw*(size_t)S.sh*3/2;
    if (p->tm_scratch_bytes < need)
    {
        HIPCHK(hipStreamSynchronize(p->copy_stream));       /* an earlier frame's launches may still use the smaller surface */
        dev_free(p->tm_scratch);
        p->tm_scratch = 0; p->tm_scratch_bytes = 0;
        if (dev_malloc((void **)&p->tm_scratch, need)) { p->tm_scratch = 0; FAIL("scale_device: device allocation failed (%zu bytes for the tone-mapped window of %d x %d)", need, S.sw, S.sh); }
        p->tm_scratch_bytes = need;
    }
    const uint8_t *src[3] = { S.c[0].base, S.c[1].base, S.c[2].base };
    const int sst[3] = { S.c[0].stride, S.c[1].stride, S.c[2].stride };
    h264e_tonemap_src_t T;
    tonemap_src(p, dev_format & 3, S.depth, src, sst, S.sw, S.sh, &T);
    const void *planes[3] = { p->tm_scratch, p->tm_scratch + (size_t)S.sw*S.sh, p->tm_scratch + (size_t)S.sw*S.sh + (size_t)(S.sw/2)*(S.sh/2) };
    const int strides[3] = { S.sw, S.sw/2, S.sw/2 }, win[6] = { S.sw, S.sh, 0, 0, 0, 0 };
    h264e_scale_src_t S8;
    if (scale_check(p, 0, slot, H264E_INGEST_I420, planes, strides, win, &S8)) return -1;
    if (ingest_order(p, producer_stream)) return -1;
    bk_launch_tonemap(T, p->tm_scratch, p->copy_stream);
    HIPCHK(hipGetLastError());
    bk_launch_scale(S8, p->clip + p->frame_bytes*(size_t)slot, p->copy_stream);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int h264e_hip_scale_device_async(h264e_hip_pool_t *p, int slot, int format, const void *const planes[3], const int strides[3], const int *win, void *producer_stream)
{
    h264e_scale_src_t S;
    if (p) HIPCHK(hipSetDevice(p->device));
    if (scale_check(p, p ? p->tm_on : 0, slot, format, planes, strides, win, &S)) return -1;
    if (p->tm_on) return tonemap_scale(p, slot, format, S, producer_stream);
    if (ingest_order(p, producer_stream)) return -1;
    if ((format & 3) == H264E_INGEST_RGBP) bk_launch_scale_rgb(S, p->clip + p->frame_bytes*(size_t)slot, p->copy_stream);
    else bk_launch_scale(S, p->clip + p->frame_bytes*(size_t)slot, p->copy_stream);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int h264e_hip_scale_device(h264e_hip_pool_t *p, int slot, int format, const void *const planes[3], const int strides[3], const int *win, void *producer_stream)
{
    if (h264e_hip_scale_device_async(p, slot, format, planes, strides, win, producer_stream)) return -1;
    HIPCHK(hipStreamSynchronize(p->copy_stream));
    return 0;
}

/* ---- device-resident output (enc_egress.h): one h264e_egress_kernel launch per picture on the pool's copy stream */

/* everything that is refused, without a launch; fills the kernel's view of the destination */
static int egress_check(const h264e_hip_pool_t *p, int slot, int dev_format, void *const planes[3], const int strides[3], int pixel_bytes, h264e_egress_dst_t *D)
{
    int format, sample, sb;
    if (!p || !planes || !strides) FAIL("egress: null argument");
    if (slot < 0 || slot >= p->nchains) FAIL("egress: picture slot %d outside the pool's %d", slot, p->nchains);
    if (dev_format_split("egress", dev_format, &format, &sample, &sb, NULL)) return -1;
    if (format == H264E_INGEST_RGB && pixel_bytes != 3 && pixel_bytes != 4) FAIL("egress: RGB pixels of %d bytes (3 or 4)", pixel_bytes);
    memset(D, 0, sizeof(*D));
    D->format = format; D->pixel_bytes = format == H264E_INGEST_RGB ? pixel_bytes : 1; D->sample = sample;
    D->width = p->G.width; D->height = p->G.height; D->W = p->G.W; D->H = p->G.H;
    D->cm = p->icm;
    const int nplanes = format == H264E_INGEST_I420 || format == H264E_INGEST_RGBP ? 3 : format == H264E_INGEST_NV12 ? 2 : 1;
    for (int k = 0; k < nplanes; k++)
    {
        /* bytes and rows of destination plane k, as the ingest counts them for a source */
        const int row_bytes = format == H264E_INGEST_RGB ? D->width*pixel_bytes : (k == 0 || format == H264E_INGEST_NV12 || format == H264E_INGEST_RGBP) ? D->width*sb : D->width/2;
        if (!planes[k]) FAIL("egress: plane %d is NULL", k);
        if (dev_sample_aligned("egress", k, planes[k], strides[k], sb, sample)) return -1;
        if (strides[k] < row_bytes) FAIL("egress: stride %d of plane %d is below its %d row bytes", strides[k], k, row_bytes);
#ifndef H264E_EMU
        /* what will be written: from the first byte of the first row to the last byte of the last */
        const int rows = k == 0 || format == H264E_INGEST_RGBP ? D->height : D->height/2;
        if (!ingest_is_device_memory(p, planes[k], (size_t)(rows - 1)*(size_t)strides[k] + (size_t)row_bytes))
            FAIL("egress: plane %d (%p, %d rows %d bytes apart) is not memory of device %d, or not inside one allocation", k, planes[k], rows, strides[k], p->device);
#endif
        D->plane[k] = (uint8_t *)planes[k]; D->stride[k] = strides[k];
    }
    return 0;
}

extern "C" int h264e_hip_egress_check(h264e_hip_pool_t *p, int slot, int format, void *const planes[3], const int strides[3], int pixel_bytes)
{
    h264e_egress_dst_t D;
    if (p) (void)hipSetDevice(p->device);
    return egress_check(p, slot, format, planes, strides, pixel_bytes, &D);
}

/* the checks, then the launch on the copy stream behind (a) everything queued on the producer's stream so far -- the caller's earlier work
 * may still read the destination -- and (b) the pool's encode stream (and its launch group's merged launch), which writes the picture;
 * returns when the destination has been written */
static int egress_run(h264e_hip_pool_t *p, int slot, int sel, int format, void *const planes[3], const int strides[3], int pixel_bytes, void *producer_stream)
{
    h264e_egress_dst_t D;
    if (p) HIPCHK(hipSetDevice(p->device));
    if (egress_check(p, slot, format, planes, strides, pixel_bytes, &D)) return -1;
    if (producer_stream)
    {
        HIPCHK(hipEventRecord(p->ev_ingest[0], (hipStream_t)producer_stream));
        HIPCHK(hipStreamWaitEvent(p->copy_stream, p->ev_ingest[0], 0));
    }
    HIPCHK(hipEventRecord(p->ev_ingest[1], p->stream));
    HIPCHK(hipStreamWaitEvent(p->copy_stream, p->ev_ingest[1], 0));
    if (p->group) HIPCHK(hipStreamWaitEvent(p->copy_stream, p->group->ev_done, 0));
    if (p->out_timed) HIPCHK(hipEventRecord(p->ev_out[0], p->copy_stream));
    bk_launch_egress(D, p->chains_host[slot].rec[sel][0], p->copy_stream);
    HIPCHK(hipGetLastError());
    if (p->out_timed) HIPCHK(hipEventRecord(p->ev_out[1], p->copy_stream));
    HIPCHK(hipStreamSynchronize(p->copy_stream));
    if (p->out_timed)
    {
        float f = 0;
        HIPCHK(hipEventElapsedTime(&f, p->ev_out[0], p->ev_out[1]));
        p->out_ms += f; p->out_calls++;
    }
    return 0;
}

/* stream pools: the picture h264e_hip_read_recon_slot reads */
extern "C" int h264e_hip_egress_slot(h264e_hip_pool_t *p, int slot, int format, void *const planes[3], const int strides[3], int pixel_bytes, void *producer_stream)
{
    return egress_run(p, slot, 0, format, planes, strides, pixel_bytes, producer_stream);
}

/* frame at a time: the picture h264e_hip_read_recon reads (after the swap: the chain's last reconstruction) */
extern "C" int h264e_hip_egress_last(h264e_hip_pool_t *p, int chain, int format, void *const planes[3], const int strides[3], int pixel_bytes, void *producer_stream)
{
    return egress_run(p, chain, p && chain >= 0 && chain < p->nchains ? p->ref_sel[chain] : 0, format, planes, strides, pixel_bytes, producer_stream);
}

/* HIP-event time of the egress launches made while `enable` was set: the totals since the pool was created (the probe) */
extern "C" int h264e_hip_egress_time(h264e_hip_pool_t *p, int enable, double *ms, long long *calls)
{
    if (!p) FAIL("egress_time: null pool");
    p->out_timed = enable != 0;
    if (ms) *ms = p->out_ms;
    if (calls) *calls = p->out_calls;
    return 0;
}

/* HIP-event time of what the caller queues on the copy stream between the two calls (ingest and scale launches: the probes) */
extern "C" int h264e_hip_copy_timer_start(h264e_hip_pool_t *p)
{
    if (!p) FAIL("copy_timer_start: null pool");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipEventRecord(p->ev_in[0], p->copy_stream));
    return 0;
}

extern "C" int h264e_hip_copy_timer_stop(h264e_hip_pool_t *p, double *ms)
{
    if (!p || !ms) FAIL("copy_timer_stop: null argument");
    float f = 0;
    *ms = 0;
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipEventRecord(p->ev_in[1], p->copy_stream));
    HIPCHK(hipEventSynchronize(p->ev_in[1]));
    HIPCHK(hipEventElapsedTime(&f, p->ev_in[0], p->ev_in[1]));
    *ms = f;
    return 0;
}

/* plain device memory for callers without a HIP toolchain of their own (H264E_dev_malloc / _free / _memcpy) */
/* ---- structural similarity (enc_ssim.h): h264e_ssim_kernel + h264e_ssim_mean_kernel on the pool's stream, all frames and planes of a call
 * in one pair of launches */

#ifdef H264E_EMU
#ifdef H264E_EMU_REVERSE
#define EMU_LANES256(t) for (int t = 255; t >= 0; --t)
#else
#define EMU_LANES256(t) for (int t = 0; t < 256; ++t)
#endif
/* the emulation's launch: tile by tile, each of the kernel's steps as a lane loop over the tile's LDS, then the second kernel's per plane */
static void bk_launch_ssim(const h264e_ssim_args_t &A, int n, int planes, hipStream_t)
{
    SsimLds *L = (SsimLds *)malloc(sizeof(SsimLds));
    if (!L) return;
    for (int pass = 0; pass < 2; pass++)
        for (int i = 0; i < n; i++)
            for (int pl = 0; pl < planes; pl++)
            {
                const ssim_plane_t P = ssim_plane(A, i, pl);
                const int ntx = ssim_tiles(P.bw - 1), nty = ssim_tiles(P.bh - 1);
                double *partial = A.partial + ((size_t)i*planes + pl)*(size_t)A.max_tiles;
                for (int k = 0; k < (pass ? 1 : ntx*nty); k++)
                {
                    memset(L, 0xEE, sizeof(*L));
                    if (!pass)
                    {
                        EMU_LANES256(t) ssim_block(L, P, k % ntx, k/ntx, t);
                        EMU_LANES256(t) ssim_window(L, P, k % ntx, k/ntx, t);
                    } else EMU_LANES256(t) ssim_gather(L->red, partial, ntx*nty, t);
                    for (int s = 128; s; s >>= 1) EMU_LANES256(t) ssim_reduce(L->red, t, s);
                    if (!pass) ssim_store(partial + k, L->red[0]);
                    else ssim_store(A.out + (size_t)i*planes + pl, L->red[0]/((double)(P.bw - 1)*(double)(P.bh - 1)));
                }
            }
    free(L);
}
#endif

#define QUAL_HEAD 512                   /* bytes in front of the doubles: h264e_hip_quality_last's picture descriptor */
#define SSIM_MAX_DIM 32768
static int qual_reserve(h264e_hip_pool_t *p, size_t doubles)
{
    static_assert(sizeof(h264e_chain_dev_t) <= QUAL_HEAD, "the descriptor fits the head of the quality buffer");
    if (p->qual_dev && p->qual_doubles >= doubles) return 0;
    HIPCHK(hipStreamSynchronize(p->stream));
    dev_free(p->qual_dev);
    p->qual_dev = 0; p->qual_doubles = 0;
    if (dev_malloc((void **)&p->qual_dev, QUAL_HEAD + sizeof(double)*doubles)) { p->qual_dev = 0; FAIL("quality: device allocation failed (%zu bytes)", QUAL_HEAD + sizeof(double)*doubles); }
    p->qual_doubles = doubles;
    return 0;
}
static int ssim_max_tiles(int w, int h) { return ssim_tiles((w >> 2) - 1)*ssim_tiles((h >> 2) - 1); }

/* both launches for n x planes pairs (A: everything but the buffers), the values to the host; complete on return */
static int ssim_run(h264e_hip_pool_t *p, h264e_ssim_args_t &A, int n, int planes, double *out)
{
    const size_t nres = (size_t)n*(size_t)planes;
    A.out = (double *)(p->qual_dev + QUAL_HEAD);
    A.partial = A.out + nres;
    if (p->q_timed) HIPCHK(hipEventRecord(p->ev_q[0], p->stream));
    bk_launch_ssim(A, n, planes, p->stream);
    HIPCHK(hipGetLastError());
    if (p->q_timed) HIPCHK(hipEventRecord(p->ev_q[1], p->stream));
    HIPCHK(hipMemcpyAsync(out, A.out, sizeof(double)*nres, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    if (p->q_timed)
    {
        float f = 0;
        HIPCHK(hipEventElapsedTime(&f, p->ev_q[0], p->ev_q[1]));
        p->q_ssim_ms += f; p->q_frames += n;
    }
    return 0;
}

/* frames of the pool's picture size: the input slots against the first pictures of `chains` */
static int ssim_frames_run(h264e_hip_pool_t *p, const char *who, int n, int cap, int in0, int in_mod, const h264e_chain_dev_t *chains, int pic0, int pic_mod, double *out)
{
    const h264e_geom_t &G = p->G;
    h264e_ssim_args_t A;
    if (G.width < 2*SSIM_MIN_DIM || G.height < 2*SSIM_MIN_DIM)
        FAIL("%s: a %d x %d picture has a chroma plane without an 8 x 8 window: SSIM needs 16 x 16 at least", who, G.width, G.height);
    memset(&A, 0, sizeof(A));
    A.a = p->clip; A.frame_bytes = p->frame_bytes; A.in0 = in0; A.in_mod = in_mod;
    A.chains = chains; A.pic0 = pic0; A.pic_mod = pic_mod;
    A.width = G.width; A.height = G.height; A.W = G.W;
    A.max_tiles = ssim_max_tiles(G.width, G.height);
    if (qual_reserve(p, 3*(size_t)cap*(1 + (size_t)A.max_tiles))) return -1;
    return ssim_run(p, A, n, 3, out);
}

extern "C" int h264e_hip_ssim_frames(h264e_hip_pool_t *p, int n, int in0, int in_mod, int pic0, int pic_mod, double *out)
{
    if (!p || !out || n <= 0 || n > p->nchains || in_mod <= 0 || in_mod > p->frames_resident || pic_mod <= 0 || pic_mod > p->nchains) FAIL("ssim_frames: bad argument");
    HIPCHK(hipSetDevice(p->device));
    return ssim_frames_run(p, "ssim_frames", n, p->nchains, in0, in_mod, (const h264e_chain_dev_t *)p->chains_dev, pic0, pic_mod, out);
}

extern "C" int h264e_hip_ssim_planes(h264e_hip_pool_t *p, const void *a, int a_stride, const void *b, int b_stride, int w, int h, double *out)
{
    h264e_ssim_args_t A;
    if (!p || !a || !b || !out) FAIL("ssim_planes: null argument");
    if (w < SSIM_MIN_DIM || w > SSIM_MAX_DIM) FAIL("ssim_planes: width %d (%d to %d: one 8 x 8 window at least)", w, SSIM_MIN_DIM, SSIM_MAX_DIM);
    if (h < SSIM_MIN_DIM || h > SSIM_MAX_DIM) FAIL("ssim_planes: height %d (%d to %d: one 8 x 8 window at least)", h, SSIM_MIN_DIM, SSIM_MAX_DIM);
    if (a_stride < w) FAIL("ssim_planes: stride %d of plane a is below its %d row bytes", a_stride, w);
    if (b_stride < w) FAIL("ssim_planes: stride %d of plane b is below its %d row bytes", b_stride, w);
    HIPCHK(hipSetDevice(p->device));
#ifndef H264E_EMU
    if (!ingest_is_device_memory(p, a, (size_t)(h - 1)*(size_t)a_stride + (size_t)w))
        FAIL("ssim_planes: plane a (%p, %d rows %d bytes apart) is not memory of device %d, or not inside one allocation", a, h, a_stride, p->device);
    if (!ingest_is_device_memory(p, b, (size_t)(h - 1)*(size_t)b_stride + (size_t)w))
        FAIL("ssim_planes: plane b (%p, %d rows %d bytes apart) is not memory of device %d, or not inside one allocation", b, h, b_stride, p->device);
#endif
    memset(&A, 0, sizeof(A));
    A.a = (const uint8_t *)a; A.b = (const uint8_t *)b; A.a_stride = a_stride; A.b_stride = b_stride;
    A.width = w; A.height = h; A.W = w;
    A.max_tiles = ssim_max_tiles(w, h);
    if (qual_reserve(p, 1 + (size_t)A.max_tiles)) return -1;
    return ssim_run(p, A, 1, 1, out);
}

/* frame at a time: input slot 0 against the picture h264e_hip_read_recon / h264e_hip_egress_last read, through a one-entry descriptor whose
 * first picture it is, so that both kernels see the pair the way a stream pool hands it over */
extern "C" int h264e_hip_quality_last(h264e_hip_pool_t *p, int chain, uint64_t ssd[3], double ssim[3])
{
    if (!p) FAIL("quality_last: null pool");
    if (chain < 0 || chain >= p->nchains) FAIL("quality_last: chain %d outside the pool's %d", chain, p->nchains);
    if (!ssd && !ssim) FAIL("quality_last: both outputs are NULL");
    if (ssim && (p->G.width < 2*SSIM_MIN_DIM || p->G.height < 2*SSIM_MIN_DIM))
        FAIL("quality_last: a %d x %d picture has a chroma plane without an 8 x 8 window: SSIM needs 16 x 16 at least", p->G.width, p->G.height);
    HIPCHK(hipSetDevice(p->device));
    if (qual_reserve(p, ssim ? 3*(1 + (size_t)ssim_max_tiles(p->G.width, p->G.height)) : 1)) return -1;
    h264e_chain_dev_t d = p->chains_host[chain];
    for (int pl = 0; pl < 3; pl++) d.rec[0][pl] = d.rec[p->ref_sel[chain]][pl];
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipMemcpy(p->qual_dev, &d, sizeof(d), hipMemcpyHostToDevice));
    if (ssd && ssd_run(p, 1, 0, 1, (const h264e_chain_dev_t *)p->qual_dev, 0, 1, ssd)) return -1;
    if (ssim && ssim_frames_run(p, "quality_last", 1, 1, 0, 1, (const h264e_chain_dev_t *)p->qual_dev, 0, 1, ssim)) return -1;
    return 0;
}

/* HIP-event time of the SSD and SSIM launches made while `enable` was set: the totals since the pool was created (the probe) */
extern "C" int h264e_hip_quality_time(h264e_hip_pool_t *p, int enable, double *ssd_ms, double *ssim_ms, long long *frames)
{
    if (!p) FAIL("quality_time: null pool");
    p->q_timed = enable != 0;
    if (ssd_ms) *ssd_ms = p->q_ssd_ms;
    if (ssim_ms) *ssim_ms = p->q_ssim_ms;
    if (frames) *frames = p->q_frames > p->q_ssd_frames ? p->q_frames : p->q_ssd_frames;      /* both cover the same frames when both are on */
    return 0;
}

extern "C" void *h264e_hip_dev_malloc(int device, size_t bytes)
{
    void *q = 0;
    if (hipSetDevice(device) != hipSuccess) { snprintf(g_err, sizeof(g_err), "dev_malloc: hipSetDevice(%d) failed", device); return 0; }
    if (dev_malloc(&q, bytes)) { snprintf(g_err, sizeof(g_err), "dev_malloc: no %zu bytes on device %d", bytes, device); return 0; }
    return q;
}
extern "C" void h264e_hip_dev_free(void *q) { dev_free(q); }
extern "C" int h264e_hip_dev_memcpy(void *dst, const void *src, size_t bytes, int to_device)
{
    if (!dst || !src) FAIL("dev_memcpy: null argument");
    HIPCHK(hipMemcpy(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int h264e_hip_generate_synth(h264e_hip_pool_t *p, int first, int nframes, int t0, uint32_t seed)
{
    if (!p || first < 0 || nframes < 0 || first + nframes > p->frames_resident) FAIL("generate_synth: bad range");
    for (int i = 0; i < nframes; i++)
    {
        uint8_t *d = p->clip + p->frame_bytes*(size_t)(first + i);
        HIPCHK(hipSetDevice(p->device));
        bk_launch_synth(d, p->G.width, p->G.height, t0 + i, seed, p->stream);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int h264e_hip_sync(h264e_hip_pool_t *p)
{
    if (!p) FAIL("sync: null pool");
    HIPCHK(hipSetDevice(p->device));
    if (p->group)
    {
        /* the merged launch of the round this pool submitted in (all members' jobs) */
        h264e_hip_group_t *g = p->group;
        const hipError_t eg = hipEventSynchronize(g->ev_done);
        /* the merged launch has drained (or is lost): the first member to see that gives the device's launch token back */
        pthread_mutex_lock(&g->mu);
        if (g->holds_device && !g->arrived) { g->holds_device = 0; device_token_give(g->device); }
        pthread_mutex_unlock(&g->mu);
        if (eg != hipSuccess) FAIL("group launch: %s", hipGetErrorString(eg));
        if (p->profile && g->nmembers && g->member[0].pool == p)
            for (int k = 0; k < 2; k++)
            {
                float a = 0;
                if (g->timed[k] && hipEventElapsedTime(&a, g->ev_t0[k], g->ev_t1[k]) == hipSuccess) { p->prof_mb_ms += a; p->prof_launches++; }
            }
    }
    {
        const hipError_t es = hipStreamSynchronize(p->stream);
        device_release(p);              /* drained (or lost): the next launch on this device may go */
        if (es != hipSuccess) FAIL("hipStreamSynchronize: %s", hipGetErrorString(es));
    }
    for (int i = 0; i < p->ev_pending; i++)
    {
        float a = 0, b = 0;
        HIPCHK(hipEventElapsedTime(&a, p->ev[i][0], p->ev[i][1]));
        HIPCHK(hipEventElapsedTime(&b, p->ev[i][1], p->ev[i][2]));
        p->prof_mb_ms += a; p->prof_splice_ms += b; p->prof_launches++;
    }
    p->ev_pending = 0;
    int err = 0;
    HIPCHK(hipMemcpy(&err, p->errflag, sizeof(int), hipMemcpyDeviceToHost));
    if (err)
    {
        (void)hipMemset(p->errflag, 0, sizeof(int));
        FAIL("macroblock kernel gave up waiting for the row above (bounded spin expired)");
    }
    device_release(p);
    p->pending = 0;
    return 0;
}

/* give the device back after a failure in the middle of a launch sequence (no error reporting of its own) */
extern "C" void h264e_hip_release(h264e_hip_pool_t *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    device_release(p);
}


/* ------------------------------------------------------------------ launch groups: several streams in ONE launch
 *
 * A single-slice stream is latency bound: after every mis-speculated mv_clusters state its pipeline drains and refills, and the chip
 * idles meanwhile.  Independent streams of the same picture size can fill each other's gaps -- but not as separate launches (see
 * g_device_lock: two persistent launches side by side can starve each other).  A group merges the launches of its member pools into ONE
 * grid: every member submits as usual (h264e_hip_submit blocks until all members that are still encoding have submitted or left), the
 * last one to arrive concatenates the jobs, interleaves the members' dispatch orders by start step -- so the streams advance in lock step
 * and every workgroup still only waits for workgroups in front of it -- and launches once.  Each job keeps its own pool's buffers, abort
 * word, error word and host mirrors (h264e_frame_task_t), so one stream's abort stops only its own jobs; h264e_hip_sync of a member
 * returns when the merged launch has drained.  Members are encoded by different host threads (H264E_clip_encode_multi).
 */
extern "C" int h264e_hip_group_create(h264e_hip_group_t **out, int device)
{
    if (!out) FAIL("group_create: null argument");
    h264e_hip_group_t *g = (h264e_hip_group_t *)calloc(1, sizeof(*g));
    if (!g) FAIL("out of host memory");
    g->device = device;
    pthread_mutex_init(&g->mu, 0); pthread_cond_init(&g->cv, 0);
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&g->stream) != hipSuccess) { free(g); FAIL("group_create: no stream on device %d", device); }
    (void)hipEventCreate(&g->ev_done);
    for (int k = 0; k < 2; k++) { (void)hipEventCreate(&g->ev_t0[k]); (void)hipEventCreate(&g->ev_t1[k]); }
    *out = g;
    return 0;
}

/* Kernel variant of a launch of `jobs` jobs of `nmby` macroblock rows each (bk_launch_mb); `jobs` is the shape's own or, in a launch group,
 * the MERGED count: a member's own few rows say nothing about how full the chip will be.  Two wavefronts per macroblock row (search |
 * reconstruction pipeline) halve the macroblock latency for twice the wave slots: the better trade wherever a launch is latency bound
 * (single-slice streams: mis-speculation events; rate control and the frame-at-a-time API: a few frames per launch) and still level for
 * multi-slice streams -- variant 2.  Around it:
 * 0, the intra-only variant of the one-wave kernel: an all-intra launch has nothing to search and no events -- no inter code, half the
 *    registers, twice the rows in flight (22.4 vs 18.3 M MB/s at 1080p);
 * 4, the two-wave kernel allocated for 4 waves per SIMD (2048 resident workgroups), where the rows fill the chip and the launch is
 *    `parallel`: it has more independent work than one single-slice stream's temporal wavefront -- several slices per frame, pictures of
 *    200+ macroblock rows (8K class), several streams merged.  Only there do the extra resident rows buy more than the 128-register
 *    allocation costs (spills in the search; round-4 sweep profiles/r04_variant_sweep.txt: 1080p 2 / 4 / 8 slices +5 %, 8K single slice +34 %, two
 *    slices +20 %; a single-slice 1080p / 4K / 720p stream -6 % / -5 % / -3 % -- its passes are bound by the mis-speculation refills,
 *    i.e. by the macroblock latency).  Not with a `tree`: a launch that carries hedge leaves (rate control) ever uses a few frames of it,
 *    pure latency (1080p 4 Mbit/s: 245 vs 213 fps, 8 slices 413 vs 381);
 * 3, the latency variant -- four waves per row, the 8x8 partition search and the deblocking + stores on waves of their own (192 VGPRs:
 *    512 resident workgroups): launches of one or a few frames, where the chip is empty and only the macroblock latency counts -- ONLY
 *    where the whole grid is resident anyway, because its far reads may wait for any workgroup of the grid. */
#define H264E_RESIDENT_WG_V2 1536
#define H264E_RESIDENT_WG_V3 512
static int pick_variant(const launch_shape_t &s, int jobs, int nmby)
{
    if (s.forced) return s.forced;
    if (s.all_intra) return 0;
    if (jobs*nmby >= H264E_RESIDENT_WG_V2 && s.parallel && !s.tree) return 4;
    if (jobs*(nmby + 1) <= H264E_RESIDENT_WG_V3) return 3;
    return 2;
}
/* workgroups of a variant that the chip holds at once */
static int variant_resident(int variant) { return variant == 3 ? H264E_RESIDENT_WG_V3 : variant == 4 ? 2048 : H264E_RESIDENT_WG_V2; }

/* Which jobs of a launch are LED (order_by_start_step): key frames behind their member's first job whose row workgroups go to the front
 * of the dispatch order.  What they encode before the launch is stopped is not lost -- the clip encoder keeps a key frame's complete
 * rows for the next launch (h264e_host.c clip_keep_collect) --, so the slots that are empty while a restarted chain refills the
 * pipeline go to them.  The launch's jobs are member after member (member_jobs[i] each); key[job] != 0: an active I job that waits for no
 * other job; first_row[job]: the rows it keeps already.  Candidates in stream order, the nearest first (by job of the member, then
 * member): a frame that is whole (first_row == nmby) costs nothing and is passed over; the others are led while their row workgroups
 * (nmby - first_row each) fit `budget`, and the first one that does not fit ends it, so the led frames are always the nearest ones.
 * Nothing is led: with hedge leaves in the launch (`tree`: nothing is kept there), in an all-intra launch, with budget 0, and where the
 * whole grid is resident anyway (every workgroup is dispatched at once and the order is moot).  Pure: no pool, no environment.
 * Returns the led jobs, their mask in led[], their row workgroups in *rows_out, the last of them in *last_out (-1: none). */
#define H264E_LEAD_MAX_JOBS 64         /* (h264e_host.c CLIP_KEEP_MAX: what a stopped launch can hand on) */
static int lead_jobs(uint8_t *led, const int *member_jobs, int nmembers, const uint8_t *key, const int *first_row, int nmby, int tree, int all_intra,
                     int resident, int budget, int *rows_out, int *last_out)
{
    int jobs = 0, maxjobs = 0, n = 0, rows = 0, last = -1, full = 0;
    for (int i = 0; i < nmembers; i++) { jobs += member_jobs[i]; if (member_jobs[i] > maxjobs) maxjobs = member_jobs[i]; }
    memset(led, 0, (size_t)jobs);
    if (!tree && !all_intra && budget > 0 && (long long)jobs*(nmby + 1) > resident)
        for (int j = 1; j < maxjobs && !full; j++)
            for (int i = 0, base = 0; i < nmembers && !full; base += member_jobs[i], i++)
            {
                const int job = base + j;
                if (j >= member_jobs[i] || !key[job]) continue;
                const int fr = first_row[job] > 0 ? first_row[job] : 0, cost = nmby - fr;
                if (cost <= 0) continue;
                if (rows + cost > budget || n >= H264E_LEAD_MAX_JOBS) { full = 1; break; }
                led[job] = 1; n++; rows += cost; last = job;
            }
    if (rows_out) *rows_out = rows;
    if (last_out) *last_out = last;
    return n;
}
/* the budget of a launch: a quarter of the variant's resident workgroups (five 1080p key frames from row 0), or what the pool was told */
static int lead_budget(int key_lead, int resident) { return key_lead >= 0 ? key_lead : resident/4; }
/* a job that lead_jobs may lead */
static int lead_candidate(const h264e_frame_task_t &t) { return t.active && t.slice_type == 2 && !t.dep_progress; }

/* the macroblock kernel on `stream`, between two events when they are given; what the launch itself reports */
static hipError_t launch_mb(const h264e_geom_t &G, int narrow, int variant, int jobs, size_t nblocks, const h264e_frame_task_t *tasks, const uint32_t *order,
                            hipEvent_t before, hipEvent_t after, hipStream_t stream)
{
    hipError_t e = before ? hipEventRecord(before, stream) : hipSuccess;
    if (e != hipSuccess) return e;
    bk_launch_mb(G, narrow, variant, jobs, (unsigned)nblocks, tasks, order, stream);
    e = after ? hipEventRecord(after, stream) : hipSuccess;
    const hipError_t le = hipGetLastError();
    return le != hipSuccess ? le : e;
}

/* why a round failed: every member reports the text, not only the thread that launched */
static int group_fail(h264e_hip_group_t *g, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g->err, sizeof(g->err), fmt, ap);
    va_end(ap);
    return -1;
}

/* room in one of the group's device buffers.  Both are sized for a whole round BEFORE its first launch: growing them between two launches
 * of a round would free memory the first one is still reading */
static int group_grow(h264e_hip_group_t *g, void **buf, size_t *cap, size_t need, size_t slack, size_t elem)
{
    if (need <= *cap) return 0;
    if (*buf) (void)hipFree(*buf);           /* (synchronises with the previous round's launch, which every member has waited for anyway) */
    *cap = need + slack;
    if (hipMalloc(buf, elem**cap) == hipSuccess) return 0;
    *buf = 0; *cap = 0;
    return group_fail(g, "group launch: device allocation failed");
}

/* ONE launch for the pending members of one window geometry (narrow / wide: different kernels), into td / od: the jobs member after
 * member, the shapes merged -- two or more streams in the grid are parallel work like slices are (a group of one: what solo_launch
 * would decide) --, the dispatch orders interleaved (order_by_start_step) with the coming key frames in front (lead_jobs).  The four-wave latency variant (512 resident workgroups)
 * must never carry a grid that does not fit the chip: pick_variant sees the merged job count.  Returns the jobs launched, -1 on failure. */
static int group_launch_geometry(h264e_hip_group_t *g, int narrow, h264e_frame_task_t *td, uint32_t *od)
{
    launch_shape_t m = { 0, narrow, 0, 1, 0, 0, 0 };
    int idx[H264E_GROUP_MAX], jobs[H264E_GROUP_MAX], n = 0, rc = 0;
    for (int k = 0; k < g->nmembers; k++)
        if (g->member[k].pending && g->member[k].shape.narrow == narrow)
        {
            const launch_shape_t &s = g->member[k].shape;
            idx[n] = k; jobs[n++] = s.jobs; m.jobs += s.jobs;
            if (s.forced) m.forced = s.forced;                          /* H264E_WAVES: the same for every pool of the process */
            m.all_intra &= s.all_intra; m.parallel |= s.parallel; m.tree |= s.tree;
        }
    if (!n) return 0;
    m.parallel |= n >= 2;
    const h264e_geom_t &G = g->member[idx[0]].pool->G;
    const size_t total = (size_t)m.jobs*(size_t)(G.nmby + 1);
    if (m.jobs >= H264E_ORDER_MAX_JOBS) return group_fail(g, "group launch: too many jobs");
    h264e_frame_task_t *th = (h264e_frame_task_t *)malloc(sizeof(h264e_frame_task_t)*(size_t)m.jobs);
    uint32_t *oh = (uint32_t *)malloc(sizeof(uint32_t)*total);
    uint8_t *led = (uint8_t *)calloc((size_t)m.jobs, 2);
    int *fr = (int *)malloc(sizeof(int)*(size_t)m.jobs);
    if (!th || !oh || !led || !fr) rc = group_fail(g, "out of host memory");
    /* the members prepared their slots (progress counters, ...) on their own streams: the launch waits for all of that */
    for (int i = 0, b = 0; i < n && !rc; b += jobs[i++])
    {
        h264e_hip_pool_t *p = g->member[idx[i]].pool;
        memcpy(th + b, g->member[idx[i]].tasks, sizeof(h264e_frame_task_t)*(size_t)jobs[i]);
        if (hipEventRecord(p->ev_prep, p->stream) != hipSuccess || hipStreamWaitEvent(g->stream, p->ev_prep, 0) != hipSuccess) rc = group_fail(g, "group launch: cannot order the launch behind a member's stream");
    }
    const int variant = pick_variant(m, m.jobs, G.nmby);
    if (!rc)
    {
        /* led key frames (lead_jobs): the budget is what the members' far-read windows leave of the 1400 workgroups h264e_hip_group_join
         * counts on, at most the solo budget; a member that switched leading off switches it off for the launch, the smallest explicit
         * budget holds */
        const int window = (12 - H264E_NARROW_FRAME_LAG)*(G.nmby + 1)/2, left = 1400 - n*(window > 0 ? window : 1);
        uint8_t *key = led + m.jobs;
        int key_lead = -1;
        for (int i = 0; i < n; i++) { const int k = g->member[idx[i]].pool->key_lead; if (k >= 0 && (key_lead < 0 || k < key_lead)) key_lead = k; }
        for (int j = 0; j < m.jobs; j++) { key[j] = (uint8_t)lead_candidate(th[j]); fr[j] = th[j].first_row; }
        const int budget = imin_h(lead_budget(key_lead, variant_resident(variant)), left > 0 ? left : 0);
        (void)lead_jobs(led, jobs, n, key, fr, G.nmby, m.tree, m.all_intra, variant_resident(variant), budget, 0, 0);
        for (int i = 0, b = 0; i < n; b += jobs[i++])
        {
            h264e_hip_pool_t *p = g->member[idx[i]].pool;
            p->led_jobs = p->led_rows = 0; p->led_last = -1;
            for (int j = 0; j < jobs[i]; j++) if (led[b + j]) { p->led_jobs++; p->led_rows += G.nmby - (fr[b + j] > 0 ? fr[b + j] : 0); p->led_last = j; }
        }
        if (order_by_start_step(oh, G.nmby + 1, narrow ? H264E_NARROW_FRAME_LAG : H264E_FRAME_LAG, jobs, n, led)) rc = group_fail(g, "out of host memory");
    }
    free(led); free(fr);
    if (!rc && (hipMemcpyAsync(td, th, sizeof(h264e_frame_task_t)*(size_t)m.jobs, hipMemcpyHostToDevice, g->stream) != hipSuccess ||
                hipMemcpyAsync(od, oh, sizeof(uint32_t)*total, hipMemcpyHostToDevice, g->stream) != hipSuccess)) rc = group_fail(g, "group launch: task upload failed");
    free(th); free(oh);            /* pageable sources: staged before the calls return */
    if (!rc)
    {
        const hipError_t le = launch_mb(G, narrow, variant, m.jobs, total, td, od, g->ev_t0[narrow], g->ev_t1[narrow], g->stream);
        if (le != hipSuccess) rc = group_fail(g, "group launch: %s", hipGetErrorString(le));
        else g->timed[narrow] = 1;
    }
    return rc ? rc : m.jobs;
}

/* all members that are still in the group have submitted: merge and launch (g->mu held), one launch per window geometry */
static int group_launch_locked(h264e_hip_group_t *g)
{
    const size_t rows = (size_t)g->member[0].pool->G.nmby + 1;         /* one picture size per group (h264e_hip_group_join) */
    size_t need_tasks = 0, off = 0;
    int rc = 0;
    g->err[0] = 0;
    g->timed[0] = g->timed[1] = 0;
    for (int k = 0; k < g->nmembers; k++) if (g->member[k].pending) need_tasks += (size_t)g->member[k].shape.jobs;
    if (hipSetDevice(g->device) != hipSuccess) rc = group_fail(g, "group launch: hipSetDevice(%d) failed", g->device);
    if (!rc) rc = group_grow(g, (void **)&g->tasks_dev, &g->tasks_cap, need_tasks, 64, sizeof(h264e_frame_task_t));
    if (!rc) rc = group_grow(g, (void **)&g->order_dev, &g->order_cap, need_tasks*rows, 4096, sizeof(uint32_t));
    /* the merged launch owns the device like any other persistent launch (g_device_held): taken here, given back by the first member whose
     * h264e_hip_sync sees the launch drained, or when the group goes away */
    if (!rc && need_tasks && !g->holds_device) { device_token_take(g->device); g->holds_device = 1; }
    for (int narrow = 0; narrow < 2 && !rc; narrow++)
    {
        const int jobs = group_launch_geometry(g, narrow, g->tasks_dev + off, g->order_dev + off*rows);
        if (jobs < 0) rc = -1; else off += (size_t)jobs;
    }
    if (hipEventRecord(g->ev_done, g->stream) != hipSuccess && !rc) rc = group_fail(g, "group launch: hipEventRecord failed");
    if (rc && !g->err[0]) (void)group_fail(g, "group launch failed");
    if (rc) snprintf(g_err, sizeof(g_err), "%s", g->err);
    for (int k = 0; k < g->nmembers; k++) { free(g->member[k].tasks); g->member[k].tasks = 0; g->member[k].pending = 0; }
    g->arrived = 0;
    g->failed = rc;
    g->round++;
    pthread_cond_broadcast(&g->cv);
    return rc;
}

/* a member's launch: hand its jobs and its shape to the group and wait until the merged launch is on its way */
static int group_submit(h264e_hip_pool_t *p, const h264e_frame_task_t *host, const launch_shape_t &s)
{
    h264e_hip_group_t *g = p->group;
    int rc = 0, k;
    pthread_mutex_lock(&g->mu);
    for (k = 0; k < g->nmembers && g->member[k].pool != p; k++) ;
    if (k == g->nmembers) { pthread_mutex_unlock(&g->mu); FAIL("group_submit: not a member"); }
    g->member[k].tasks = (h264e_frame_task_t *)malloc(sizeof(h264e_frame_task_t)*(size_t)s.jobs);
    if (!g->member[k].tasks) { pthread_mutex_unlock(&g->mu); FAIL("out of host memory"); }
    memcpy(g->member[k].tasks, host, sizeof(h264e_frame_task_t)*(size_t)s.jobs);
    g->member[k].shape = s; g->member[k].pending = 1;
    p->group_round = g->round;
    g->arrived++;
    if (g->arrived == g->nmembers) rc = group_launch_locked(g);
    else
    {
        const int r = g->round;
        while (g->round == r) pthread_cond_wait(&g->cv, &g->mu);
        rc = g->failed;
    }
    if (rc) snprintf(g_err, sizeof(g_err), "%s", g->err[0] ? g->err : "group launch failed");       /* g_err is per thread: every member gets the text */
    pthread_mutex_unlock(&g->mu);
    return rc;
}

extern "C" int h264e_hip_group_join(h264e_hip_group_t *g, h264e_hip_pool_t *p)
{
    if (!g || !p || p->group) FAIL("group_join: bad argument");
    pthread_mutex_lock(&g->mu);
    /* how many streams one grid can hold: a far reference read waits for a workgroup up to (12 - lag) dispatch keys AHEAD of its own
     * (enc_kernels.h rv_wait_rect), i.e. about (12 - lag)*(nmby + 1)/2 workgroups per member stream, and all of those must be resident
     * together with the waiting one.  The variant is chosen from the merged grid (pick_variant): the two-wave kernels hold 1536 / 2048
     * workgroups -- 1400 with a margin --, and the four-wave latency variant (512) only ever carries a grid that is resident as a whole */
    const int window = (12 - H264E_NARROW_FRAME_LAG)*(p->G.nmby + 1)/2, room = 1400/(window > 0 ? window : 1);
    int bad = g->nmembers >= H264E_GROUP_MAX || (g->nmembers >= 1 && g->nmembers >= room) || p->device != g->device || g->arrived;
    if (!bad && g->nmembers)
    {
        const h264e_geom_t &A = g->member[0].pool->G, &B = p->G;
        bad = A.width != B.width || A.height != B.height || A.row_words != B.row_words || A.spin_limit != B.spin_limit;
    }
    if (!bad) { memset(&g->member[g->nmembers], 0, sizeof(g->member[0])); g->member[g->nmembers++].pool = p; p->group = g; }
    pthread_mutex_unlock(&g->mu);
    if (bad) FAIL("group_join: the group is full (at most %d streams of this picture size share a launch), busy, on another device or holds another picture size", room < H264E_GROUP_MAX ? room : H264E_GROUP_MAX);
    return 0;
}

extern "C" void h264e_hip_group_leave(h264e_hip_group_t *g, h264e_hip_pool_t *p)
{
    if (!g || !p || p->group != g) return;
    pthread_mutex_lock(&g->mu);
    int k;
    for (k = 0; k < g->nmembers && g->member[k].pool != p; k++) ;
    if (k < g->nmembers)
    {
        if (g->member[k].pending) { free(g->member[k].tasks); g->arrived--; }
        memmove(&g->member[k], &g->member[k + 1], sizeof(g->member[0])*(size_t)(g->nmembers - 1 - k));
        g->nmembers--;
        /* the others may have been waiting for this member only */
        if (g->nmembers && g->arrived == g->nmembers) (void)group_launch_locked(g);
        if (!g->nmembers && g->holds_device)
        {
            /* the last member is gone: nobody will sync the group's launches any more */
            (void)hipSetDevice(g->device);
            (void)hipStreamSynchronize(g->stream);
            g->holds_device = 0; device_token_give(g->device);
        }
    }
    p->group = 0;
    pthread_mutex_unlock(&g->mu);
}

extern "C" void h264e_hip_group_destroy(h264e_hip_group_t *g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    (void)hipStreamSynchronize(g->stream);
    for (int k = 0; k < g->nmembers; k++) { g->member[k].pool->group = 0; if (g->member[k].pending) free(g->member[k].tasks); }
    if (g->tasks_dev) (void)hipFree(g->tasks_dev);
    if (g->order_dev) (void)hipFree(g->order_dev);
    if (g->holds_device) { g->holds_device = 0; device_token_give(g->device); }
    (void)hipEventDestroy(g->ev_done);
    for (int k = 0; k < 2; k++) { (void)hipEventDestroy(g->ev_t0[k]); (void)hipEventDestroy(g->ev_t1[k]); }
    (void)hipStreamDestroy(g->stream);
    pthread_mutex_destroy(&g->mu); pthread_cond_destroy(&g->cv);
    free(g);
}

/* ---- h264e_hip_submit: check, fill, token, upload, then launch or hand to the group */

/* Every refusal of a submit, and the launch's shape.  The pool is const: a refused submit has changed nothing. */
static int submit_check(const h264e_hip_pool_t *p, const h264e_hip_task_t *tasks, launch_shape_t *s)
{
    const h264e_geom_t &G = p->G;
    int any_narrow = 0, any_wide = 0, max_slices = 1;
    memset(s, 0, sizeof(*s));
    s->forced = p->waves; s->all_intra = 1;
    for (int c = 0; c < p->nchains; c++)
    {
        const h264e_hip_task_t &t = tasks[c];
        if (!t.active) continue;
        if (t.frame_index < 0 || t.frame_index >= p->frames_resident ||
            t.qp < 10 || t.qp > 51 || t.hdr_nbits < 0 || t.hdr_nbits > 56 || t.nslices < 0 || t.nslices > H264E_MAX_SLICES || t.nslices > G.nmby)
            FAIL("submit: bad task for chain %d", c);
        if (t.denoised && !p->den) FAIL("submit: task %d asks for the denoised picture, but the denoiser is not on", c);
        /* temporal wavefront: job c builds the picture of chain slot t.slot from the picture of slot t.ref_slot */
        if (t.stream_mode && (t.slot < 0 || t.slot >= p->nchains || t.ref_slot >= p->nchains || (t.slice_type == 0 && t.ref_slot < 0) ||
                              (t.ref_in_flight && t.ref_slot < 0)))
            FAIL("submit: bad stream task %d", c);
        s->jobs = c + 1;
        if (t.slice_type != 2) s->all_intra = 0;
        if (t.nslices > max_slices) max_slices = t.nslices;
        /* hedge leaves.  (The device job's walk_quiet, which is only set under walk_on_device, would say the same: the clip encoder
         * only ever sets walk_quiet on copies of tasks that have both -- h264e_host.c clip_plan_launch.) */
        if (t.stream_mode && t.walk_quiet) s->tree = 1;
        if (t.stream_mode && t.narrow_window) any_narrow = 1; else any_wide = 1;
    }
    if (any_narrow && any_wide) FAIL("submit: the jobs of one launch must agree on narrow_window");
    if (s->jobs >= H264E_ORDER_MAX_JOBS) FAIL("submit: too many jobs");
    s->narrow = any_narrow;
    s->sliced = max_slices >= 2;
    s->parallel = s->sliced || G.nmby >= 200;
    return 0;
}

/* reference and decoded picture of job c: a stream task names its slots (and may walk on the device), a frame-at-a-time task
 * ping-pongs the two pictures of its chain */
static void fill_pictures(h264e_hip_pool_t *p, const h264e_hip_task_t *tasks, int c, h264e_frame_task_t &d)
{
    const h264e_hip_task_t &t = tasks[c];
    if (!t.stream_mode)
    {
        const int rs = p->ref_sel[c];
        d.chain = c;
        for (int k = 0; k < 3; k++) { d.ref[k] = p->chains_host[c].rec[rs][k]; d.dec[k] = p->chains_host[c].rec[rs ^ 1][k]; }
        p->ref_sel[c] ^= 1;
        return;
    }
    d.chain = t.slot;
    d.abort_word = p->abort_dev;
    if (t.walk_on_device)
    {
        const int par = t.walk_parent > 0 ? t.walk_parent - 1 : c - 1;
        d.walk_on_device = 1;
        d.walk_quiet = t.walk_quiet;
        d.exact_state[0] = t.exact_state[0]; d.exact_state[1] = t.exact_state[1];
        d.walk_out = p->walkrec + t.slot;
        d.walk_prev = (par >= 0 && par < c && tasks[par].active && tasks[par].stream_mode && tasks[par].walk_on_device) ? p->walkrec + tasks[par].slot : 0;
        d.traj_out = p->traj_dev[t.slot] + (size_t)(p->traj_cur[t.slot] ^ 1)*2*p->G.nmb;
    }
    for (int k = 0; k < 3; k++)
    {
        d.dec[k] = p->chains_host[t.slot].rec[0][k];
        d.ref[k] = t.ref_slot >= 0 ? p->chains_host[t.ref_slot].rec[0][k] : p->chains_host[t.slot].rec[1][k];
    }
    d.dep_progress = t.ref_in_flight ? p->chains_host[t.ref_slot].progress : 0;
}

/* row bands exactly as the reference splits them (h264-lab.h:6530): mby += (nmby - mby)/(nthreads - ithr) */
static void fill_slice_rows(const h264e_geom_t &G, int nslices, h264e_frame_task_t &d)
{
    int mby = 0;
    d.nslices = nslices > 1 ? nslices : 1;
    for (int k = 0; k < d.nslices; k++) { d.slice_row[k] = (int16_t)mby; mby += (G.nmby - mby)/(d.nslices - k); }
    d.slice_row[d.nslices] = (int16_t)G.nmby;
}

/* where the job's per-macroblock mv_clusters come from: the latest device walk of its slot, a host array (the re-encode path, rare
 * and synchronous: a blocking copy keeps the host array's lifetime simple), or nowhere */
static int fill_clusters(h264e_hip_pool_t *p, const h264e_hip_task_t &t, int c, h264e_frame_task_t &d)
{
    const size_t n = sizeof(int32_t)*2*(size_t)p->G.nmb;
    const int cs = t.stream_mode ? t.slot : c;
    d.clusters[0] = t.mv_clusters[0]; d.clusters[1] = t.mv_clusters[1];
    if (t.stream_mode && t.traj_from_device) d.clusters_per_mb = p->traj_dev[t.slot] + (size_t)p->traj_cur[t.slot]*2*p->G.nmb;
    else if (t.mv_clusters_per_mb)
    {
        if (hipStreamSynchronize(p->stream) != hipSuccess || hipMemcpy(p->clu_dev[cs], t.mv_clusters_per_mb, n, hipMemcpyHostToDevice) != hipSuccess) FAIL("mv_clusters upload failed");
        d.clusters_per_mb = p->clu_dev[cs];
    }
    return 0;
}

/* the device job of the checked, active task c (d is zeroed), and what the pool remembers about it */
static int fill_task(h264e_hip_pool_t *p, const h264e_hip_task_t *tasks, int c, int launch_id, h264e_frame_task_t &d)
{
    const h264e_geom_t &G = p->G;
    const h264e_hip_task_t &t = tasks[c];
    const uint8_t *f = t.denoised ? den_frame(p, den_index(p, t.frame_index)) : p->clip + p->frame_bytes*(size_t)t.frame_index;
    d.active = t.active;
    d.in[0] = f; d.in[1] = f + (size_t)G.width*G.height; d.in[2] = d.in[1] + (size_t)(G.width/2)*(G.height/2);
    d.in_stride[0] = G.width; d.in_stride[1] = d.in_stride[2] = G.width/2;
    d.slice_type = t.slice_type; d.qp = t.qp; d.speed = t.speed;
    d.no_deblock = (t.speed == 8 || t.speed == 10);                 /* h264-lab.h:6717 */
    fill_pictures(p, tasks, c, d);
    /* the finalizer exports the slot's result to host-mapped memory: the host reads NALs, flags and records without a
     * device-to-host copy */
    d.arena_reset = 1;
    d.stepflags = p->stepflags + 2*c;
    d.host_done = p->host_done + d.chain;
    d.host_rbsp = p->host_rbsp[d.chain]; d.host_rbsp_cap = p->host_rbsp_cap;
    d.host_mbrec = (h264e_mbrec_t *)p->host_mbrec[d.chain];
    d.chain_desc = p->chains_dev + d.chain;
    d.errflag = p->errflag;
    d.mb_counter = p->mb_counter;
    /* (first_row == nmby: every row is kept, only the job's finalizer runs -- a key frame that a stopped launch had completed) */
    d.first_row = (t.stream_mode && t.first_row > 0 && t.first_row <= G.nmby) ? t.first_row : 0;
    d.narrow = t.stream_mode && t.narrow_window;
    d.hdr_nal = t.hdr_nal; d.hdr_nbits = t.hdr_nbits; d.hdr_bits = t.hdr_bits;
    fill_slice_rows(G, t.nslices, d);
    if (fill_clusters(p, t, c, d)) return -1;
    memcpy(d.qdat, t.qdat, sizeof(d.qdat));
    d.launch_id = launch_id;
    p->host_done[d.chain].done = 0;
    p->slot_launch[d.chain] = launch_id;
    if (d.walk_on_device) p->traj_cur[t.slot] ^= 1;         /* this launch's walk writes the other buffer: it is the latest from now on */
    return 0;
}

/* every row and `decided` counter to zero; rows kept from the previous encode of a frame (first_row) count as complete */
static int reset_progress(h264e_hip_pool_t *p, const h264e_frame_task_t *host)
{
    const h264e_geom_t &G = p->G;
    const size_t words = 2*(size_t)p->nchains*G.nmby;
    int kept = 0;
    for (int c = 0; c < p->nchains; c++) kept += host[c].active && host[c].first_row > 0;
    hipError_t e;
    if (!kept) e = hipMemsetAsync(p->progress_all, 0, sizeof(int)*words, p->stream);
    else
    {
        /* one image of all counters and ONE copy: with led key frames a launch of a small picture starts dozens of jobs below row 0, and
         * two small copies for each of them were 0.5 ms of host time per launch (352x288 x 3000) */
        if (!p->progress_img) p->progress_img = (int *)malloc(sizeof(int)*words);
        int *img = p->progress_img;
        if (!img) FAIL("out of host memory");
        memset(img, 0, sizeof(int)*words);
        for (int c = 0; c < p->nchains; c++)
            if (host[c].active && host[c].first_row > 0)
            {
                int *progress = img + (size_t)host[c].chain*2*G.nmby;       /* = chains_host[chain].progress - progress_all */
                for (int r = 0; r < host[c].first_row; r++) progress[r] = progress[G.nmby + r] = G.nmbx + 1;
            }
        e = hipMemcpyAsync(p->progress_all, img, sizeof(int)*words, hipMemcpyHostToDevice, p->stream);     /* (the image is the pool's: written again only by the next submit with kept rows, which follows a sync) */
    }
    if (e != hipSuccess) FAIL("progress reset: %s", hipGetErrorString(e));
    return 0;
}

/* a pool's own launch of the uploaded jobs `slot`: the dispatch order is cached for the launch's shape (jobs up to the last active
 * one; window geometry; sliced or not; which jobs are led), the launch is timed when the pool is profiled.  `host`: the jobs as uploaded
 * to `slot`.  The led set (lead_jobs) is part of the cache key as the set itself -- a led job's first_row matters only where it decides
 * whether the job is in the set --, so a launch whose key frames stand elsewhere builds and uploads its order again: 44 KB for 160 jobs
 * of 1080p, some 0.1 ms of host time per launch next to the 6-12 ms a relaunch takes to deliver its first frame. */
static int solo_launch(h264e_hip_pool_t *p, const h264e_frame_task_t *slot, const h264e_frame_task_t *host, const launch_shape_t &s)
{
    const int pe = p->ev_pending, variant = pick_variant(s, s.jobs, p->G.nmby), resident = p->test_lead_resident >= 0 ? p->test_lead_resident : variant_resident(variant);
    {
        uint8_t *key = (uint8_t *)malloc((size_t)s.jobs);
        int *fr = (int *)malloc(sizeof(int)*(size_t)s.jobs);
        if (!key || !fr) { free(key); free(fr); FAIL("out of host memory"); }
        for (int j = 0; j < s.jobs; j++) { key[j] = (uint8_t)lead_candidate(host[j]); fr[j] = host[j].first_row; }
        p->led_jobs = lead_jobs(p->led, &s.jobs, 1, key, fr, p->G.nmby, s.tree, s.all_intra, resident, lead_budget(p->key_lead, resident), &p->led_rows, &p->led_last);
        free(key); free(fr);
    }
    if (s.jobs != p->order_jobs || s.narrow != p->order_narrow || s.sliced != p->order_sliced || memcmp(p->led, p->order_led, (size_t)s.jobs))
    {
        if (build_order(p, s.jobs, s.narrow, s.sliced, -1, p->led_jobs ? p->led : 0)) return -1;
        HIPCHK(hipMemcpyAsync(p->order, p->order_host, sizeof(uint32_t)*p->order_count, hipMemcpyHostToDevice, p->stream));     /* pageable: staged before the call returns */
        p->order_jobs = s.jobs; p->order_narrow = s.narrow; p->order_sliced = s.sliced;
        memcpy(p->order_led, p->led, (size_t)s.jobs);
    }
    const hipError_t e = launch_mb(p->G, s.narrow, variant, s.jobs, p->order_count, slot, p->order,
                                   p->profile ? p->ev[pe][0] : 0, p->profile ? p->ev[pe][1] : 0, p->stream);
    if (e != hipSuccess) FAIL("macroblock kernel launch: %s", hipGetErrorString(e));
    if (p->profile)
    {
        HIPCHK(hipEventRecord(p->ev[pe][2], p->stream));
        p->ev_pending++;
    }
    return 0;
}

extern "C" int h264e_hip_submit(h264e_hip_pool_t *p, const h264e_hip_task_t *tasks)
{
    launch_shape_t s;
    if (!p || !tasks) FAIL("submit: null argument");
    HIPCHK(hipSetDevice(p->device));
    if (submit_check(p, tasks, &s)) return -1;
    if (!s.jobs) return 0;
    if (p->pending >= TASK_RING - 1 && h264e_hip_sync(p)) return -1;
    h264e_frame_task_t *host = p->tasks_host;
    const int launch_id = ++p->launch_counter;
    memset(host, 0, sizeof(h264e_frame_task_t)*(size_t)p->nchains);
    for (int c = 0; c < p->nchains; c++)
        if (tasks[c].active && fill_task(p, tasks, c, launch_id, host[c])) return -1;
    if (!p->group) device_acquire(p);   /* one launch at a time per device (see g_device_held); a launch group takes the token for its merged launch (group_launch_locked) */
    h264e_frame_task_t *slot = p->tasks_dev + (size_t)p->ring_pos*p->nchains;
    p->ring_pos = (p->ring_pos + 1) % TASK_RING;
    p->pending++;
    /* pageable source: the runtime stages the copy before returning, so the next submit may overwrite `host` */
    const hipError_t e = hipMemcpyAsync(slot, host, sizeof(h264e_frame_task_t)*(size_t)p->nchains, hipMemcpyHostToDevice, p->stream);
    if (e != hipSuccess) FAIL("task upload: %s", hipGetErrorString(e));
    if (reset_progress(p, host)) return -1;
    /* member of a launch group: the launch is merged with the other members' and the variant is chosen from the MERGED grid */
    return p->group ? group_submit(p, host, s) : solo_launch(p, slot, host, s);
}

/* Leading the coming key frames (lead_jobs): budget < 0 the default budget, 0 off, N that many row workgroups per launch.  _last_lead:
 * what the pool's last submit led -- key frames, their row workgroups, and the last led job of the submit (-1: none). */
extern "C" void h264e_hip_set_key_lead(h264e_hip_pool_t *p, int budget) { if (p) p->key_lead = budget < 0 ? -1 : budget; }
extern "C" void h264e_hip_last_lead(h264e_hip_pool_t *p, int *jobs, int *rows, int *last)
{
    if (jobs) *jobs = p ? p->led_jobs : 0;
    if (rows) *rows = p ? p->led_rows : 0;
    if (last) *last = p ? p->led_last : -1;
}

/* ---- results: every job's finalizer exports them to the host-mapped mirrors of its chain slot */

extern "C" int h264e_hip_stream_done(h264e_hip_pool_t *p, int slot, h264e_hip_result_t *res)
{
    if (!p || slot < 0 || slot >= p->nchains) FAIL("stream_done: bad argument");
    const volatile h264e_hostdone_t *d = p->host_done + slot;
    const int v = d->done;
    if (v != p->slot_launch[slot] && v != -p->slot_launch[slot]) return 0;      /* not yet */
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (res)
    {
        res->walk_status = d->walk_status; res->first_bad = d->first_bad; res->state_out[0] = d->state_out[0]; res->state_out[1] = d->state_out[1];
        if (v > 0)
        {
            res->nbytes = d->nbytes; res->all_skipped = d->all_skipped; res->clusters_moved = d->clusters_moved; res->overflow = d->overflow; res->far_reads = d->far_reads;
            res->nslices = d->nslices; res->in_device = d->in_device;
            for (int k = 0; k < H264E_HIP_MAX_SLICES; k++) res->slice_nbytes[k] = d->slice_nbytes[k];
        }
    }
    return v > 0 ? 1 : 2;                                   /* 2: the job was aborted (or failed its own validation: walk_status) */
}

/* Macroblock rows of `slot`, counted from the top, that the last launch left complete (counter = nmbx + 1: row buffer, records, samples
 * and the lines pending for the row below are all written).  Call after h264e_hip_sync and before the next submit, which resets the
 * counters.  A job of that launch whose finalizer raised its done word has spliced every row: all of them, without a look at the
 * counters (the answer for the frames behind a full output buffer, which were simply not taken; the emulation, whose rows publish no
 * counters, knows complete frames only this way).  Otherwise the counters are copied, on the pool's own stream: a copy on the null
 * stream would wait for every other stream of the device. */
extern "C" int h264e_hip_stream_rows_complete(h264e_hip_pool_t *p, int slot, int *rows)
{
    if (!p || !rows || slot < 0 || slot >= p->nchains) FAIL("stream_rows_complete: bad argument");
    const h264e_geom_t &G = p->G;
    int n = 0;
    if (p->slot_launch[slot] == p->launch_counter && ((const volatile h264e_hostdone_t *)p->host_done)[slot].done == p->launch_counter) n = G.nmby;
    else
    {
        int *host = (int *)malloc(sizeof(int)*(size_t)G.nmby);
        if (!host) FAIL("out of host memory");
        (void)hipSetDevice(p->device);
        hipError_t e = hipMemcpyAsync(host, p->chains_host[slot].progress, sizeof(int)*(size_t)G.nmby, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
        while (e == hipSuccess && n < G.nmby && host[n] == G.nmbx + 1) n++;
        free(host);
        if (e != hipSuccess) FAIL("stream_rows_complete: %s", hipGetErrorString(e));
    }
    if (p->test_keep_rows_cap >= 0 && n > p->test_keep_rows_cap) n = p->test_keep_rows_cap;
    *rows = n;
    return 0;
}

extern "C" int h264e_hip_stream_fetch_traj(h264e_hip_pool_t *p, int slot, int consumed, int32_t *dst)
{
    if (!p || !dst || slot < 0 || slot >= p->nchains) FAIL("stream_fetch_traj: bad argument");
    const int32_t *src = p->traj_dev[slot] + (size_t)(p->traj_cur[slot] ^ (consumed ? 1 : 0))*2*p->G.nmb;
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpy(dst, src, sizeof(int32_t)*2*(size_t)p->G.nmb, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int h264e_hip_stream_copy_picture(h264e_hip_pool_t *p, int from, int to)
{
    if (!p || from < 0 || to < 0 || from >= p->nchains || to >= p->nchains) FAIL("stream_copy_picture: bad argument");
    if (from == to) return 0;
    const size_t plane = (size_t)p->G.W*p->G.H*3/2;
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpyAsync(p->chains_host[to].rec[0][0], p->chains_host[from].rec[0][0], plane, hipMemcpyDeviceToDevice, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return 0;
}

extern "C" const uint8_t *h264e_hip_stream_rbsp(h264e_hip_pool_t *p, int slot)
{
    return (p && slot >= 0 && slot < p->nchains) ? p->host_rbsp[slot] : 0;
}

/* a frame whose NALs did not fit the host mirror (res.in_device): copy them from the slot's device NAL arena; works while the
 * launch is still running (copy stream) */
extern "C" int h264e_hip_stream_fetch_nals(h264e_hip_pool_t *p, int slot, uint8_t *dst, uint32_t nbytes)
{
    if (!p || !dst || slot < 0 || slot >= p->nchains || nbytes > p->chains_host[slot].nal_cap) FAIL("stream_fetch_nals: bad argument");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpyAsync(dst, p->chains_host[slot].nal_arena, nbytes, hipMemcpyDeviceToHost, p->copy_stream));
    HIPCHK(hipStreamSynchronize(p->copy_stream));
    return 0;
}

extern "C" int h264e_hip_download_i420(h264e_hip_pool_t *p, int first, int nframes, uint8_t *host)
{
    if (!p || !host || first < 0 || nframes < 0 || first + nframes > p->frames_resident) FAIL("download_i420: bad range");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpy(host, p->clip + p->frame_bytes*(size_t)first, p->frame_bytes*(size_t)nframes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" const h264e_hip_mbrec_t *h264e_hip_stream_mbrec(h264e_hip_pool_t *p, int slot)
{
    return (p && slot >= 0 && slot < p->nchains) ? p->host_mbrec[slot] : 0;
}

/* ask every job of the most recent submit to stop (the launch drains quickly; sync afterwards) */
extern "C" int h264e_hip_stream_abort(h264e_hip_pool_t *p)
{
    if (!p || !p->abort_word) FAIL("stream_abort: bad argument");
    __atomic_store_n(p->abort_word, p->launch_counter, __ATOMIC_RELEASE);
    /* the kernel polls a word in device memory: the launch id is written there BY VALUE on a stream of its own, next to the running
     * launch -- not behind the application's staging uploads on the copy stream (up to hundreds of MB), and not as a copy whose source
     * could have moved on to the next launch's id by the time it executes */
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)p->abort_dev, p->launch_counter, 1, p->abort_stream));
    return 0;
}

/* 1 while work submitted to the pool is still running */
extern "C" int h264e_hip_busy(h264e_hip_pool_t *p)
{
    if (!p) return 0;
    (void)hipSetDevice(p->device);
    if (p->group && hipEventQuery(p->group->ev_done) == hipErrorNotReady) return 1;
    return hipStreamQuery(p->stream) == hipErrorNotReady;
}

extern "C" int h264e_hip_read_recon(h264e_hip_pool_t *p, int chain, uint8_t *dst)
{
    if (!p || !dst || chain < 0 || chain >= p->nchains) FAIL("read_recon: bad argument");
    const size_t n = (size_t)p->G.W*p->G.H*3/2;
    const uint8_t *src = p->chains_host[chain].rec[p->ref_sel[chain]][0];   /* after the swap: last reconstruction */
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int h264e_hip_rewind_frame(h264e_hip_pool_t *p, int chain)
{
    if (!p || chain < 0 || chain >= p->nchains) FAIL("rewind_frame: bad argument");
    p->ref_sel[chain] ^= 1;
    return 0;
}

/* test hook: the dispatch order build_order makes for a launch of `jobs` jobs (banded = 1 forces the XCD bands with their padding, 0 none);
 * returns the number of entries (out gets at most cap of them), -1 on failure.  Leaves the pool's cached order invalid. */
extern "C" long h264e_hip_selftest_order(h264e_hip_pool_t *p, int jobs, int narrow, int banded, uint32_t *out, size_t cap)
{
    if (!p || jobs < 1 || jobs > p->nchains || !out) { snprintf(g_err, sizeof(g_err), "selftest_order: bad argument"); return -1; }
    const int rc = build_order(p, jobs, narrow, 0, banded ? 8 : 0, 0);
    p->order_jobs = -1;
    if (rc) return -1;
    memcpy(out, p->order_host, sizeof(uint32_t)*(p->order_count < cap ? p->order_count : cap));
    return (long)p->order_count;
}

/* test hook: order_by_start_step itself, for a launch that merges `nmembers` streams of member_jobs[i] jobs each; returns the number of
 * entries (out gets at most cap of them), -1 on failure */
extern "C" long h264e_hip_selftest_merged_order(int rows, int lag, const int *member_jobs, int nmembers, uint32_t *out, size_t cap)
{
    size_t jobs = 0;
    for (int i = 0; member_jobs && i < nmembers; i++) jobs += member_jobs[i] > 0 ? (size_t)member_jobs[i] : H264E_ORDER_MAX_JOBS;
    if (rows < 1 || rows > 65536 || lag < 1 || !member_jobs || nmembers < 1 || !out || jobs >= H264E_ORDER_MAX_JOBS) { snprintf(g_err, sizeof(g_err), "selftest_merged_order: bad argument"); return -1; }
    uint32_t *ord = (uint32_t *)malloc(sizeof(uint32_t)*jobs*(size_t)rows);
    const int rc = ord ? order_by_start_step(ord, rows, lag, member_jobs, nmembers, 0) : -1;
    if (!rc) memcpy(out, ord, sizeof(uint32_t)*(jobs*(size_t)rows < cap ? jobs*(size_t)rows : cap));
    free(ord);
    if (rc) { snprintf(g_err, sizeof(g_err), "out of host memory"); return -1; }
    return (long)(jobs*(size_t)rows);
}

/* test hook: lead_jobs and the order it gives, for a launch that merges `nmembers` streams of member_jobs[i] jobs of nmby rows each (one
 * member: a pool's own launch).  key / first_row: per launch job, member after member; tree / all_intra: the launch's shape; resident:
 * the workgroups of its variant that the chip holds; budget: row workgroups that may be led.  banded != 0: through the XCD bands (one
 * member only).  led_out (may be NULL) gets the led set, one byte per job; out at most cap of the order's entries.  Returns the number
 * of entries, -1 on failure. */
extern "C" long h264e_hip_selftest_lead_order(int nmby, int lag, const int *member_jobs, int nmembers, const uint8_t *key, const int *first_row,
                                              int tree, int all_intra, int resident, int budget, int banded, uint32_t *out, size_t cap, uint8_t *led_out)
{
    size_t jobs = 0;
    for (int i = 0; member_jobs && i < nmembers; i++) jobs += member_jobs[i] > 0 ? (size_t)member_jobs[i] : H264E_ORDER_MAX_JOBS;
    if (nmby < 1 || nmby >= 65535 || lag < 1 || !member_jobs || nmembers < 1 || !key || !first_row || !out || jobs >= H264E_ORDER_MAX_JOBS || (banded && nmembers != 1))
    { snprintf(g_err, sizeof(g_err), "selftest_lead_order: bad argument"); return -1; }
    const size_t rows = (size_t)nmby + 1, total = jobs*rows;
    h264e_geom_t G;
    memset(&G, 0, sizeof(G));
    G.nmby = nmby;
    const size_t room = banded ? order_capacity(G, (int)jobs) : total;
    uint32_t *ord = (uint32_t *)malloc(sizeof(uint32_t)*total), *res = banded ? (uint32_t *)malloc(sizeof(uint32_t)*room) : ord;
    uint8_t *led = (uint8_t *)malloc(jobs);
    size_t n = total;
    int rc = (ord && res && led) ? 0 : -1;
    if (!rc)
    {
        const int nled = lead_jobs(led, member_jobs, nmembers, key, first_row, nmby, tree, all_intra, resident, budget, 0, 0);
        rc = order_by_start_step(ord, (int)rows, lag, member_jobs, nmembers, nled ? led : 0);
        if (!rc && banded && !(n = order_into_bands(G, (int)jobs, ord, (int)total, res, nled ? led : 0))) rc = -1;
    }
    if (!rc) memcpy(out, res, sizeof(uint32_t)*(n < cap ? n : cap));
    if (!rc && led_out) memcpy(led_out, led, jobs);
    if (banded) free(res);
    free(ord); free(led);
    if (rc) { snprintf(g_err, sizeof(g_err), "out of host memory"); return -1; }
    return (long)n;
}

extern "C" int h264e_hip_selftest_nal_escape(h264e_hip_pool_t *p, const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t cap, uint32_t *out_n)
{
    if (!p || !src || !dst || !out_n) FAIL("selftest_nal_escape: bad argument");
    const size_t sb = ((size_t)n + 64 + 15) & ~(size_t)15, db = ((size_t)cap + 15) & ~(size_t)15;
    uint8_t *buf = 0;
    uint32_t res[2] = { 0, 0 };
    HIPCHK(hipSetDevice(p->device));
    if (hipMalloc((void **)&buf, sb + db + 64) != hipSuccess) FAIL("selftest_nal_escape: device allocation failed");
    hipError_t e = hipMemset(buf, 0, sb + db + 64);
    if (e == hipSuccess) e = hipMemcpy(buf, src, n, hipMemcpyHostToDevice);
    if (e == hipSuccess)
    {
        bk_launch_nal_selftest(buf + sb, cap, (const uint8_t *)buf, n, (uint32_t *)(buf + sb + db), p->stream);
        e = hipStreamSynchronize(p->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(res, buf + sb + db, sizeof(res), hipMemcpyDeviceToHost);
    if (e == hipSuccess && !res[1] && res[0] <= cap) e = hipMemcpy(dst, buf + sb, res[0], hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) FAIL("selftest_nal_escape: %s", hipGetErrorString(e));
    *out_n = res[0];
    return res[1] ? 1 : 0;
}

extern "C" int h264e_hip_selftest_stage(h264e_hip_pool_t *p, int stage, const uint8_t *in, uint32_t nin, const int *args /* [24] */, uint8_t *out, uint32_t nout)
{
    const uint32_t out_max = stage == 16 ? 4*STAGE_AVG4_DWORDS : STAGE_OUT_MAX;          /* stage 16 writes all of it, whatever nout asks for */
    if (!p || !in || !args || !out || stage < 1 || stage > 16 || nin > STAGE_IN_MAX || nout > out_max) FAIL("selftest_stage: bad argument");
    uint8_t *buf = 0;
    HIPCHK(hipSetDevice(p->device));
    if (hipMalloc((void **)&buf, STAGE_IN_MAX + out_max + 256) != hipSuccess) FAIL("selftest_stage: device allocation failed");
    hipError_t e = hipMemset(buf, 0, STAGE_IN_MAX + out_max + 256);
    if (e == hipSuccess) e = hipMemcpy(buf, in, nin, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + STAGE_IN_MAX, args, STAGE_NARGS*sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess)
    {
        bk_launch_stage_selftest(stage, (const uint8_t *)buf, (const int *)(buf + STAGE_IN_MAX), buf + STAGE_IN_MAX + 128, p->stream);
        e = hipStreamSynchronize(p->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(out, buf + STAGE_IN_MAX + 128, nout, hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) FAIL("selftest_stage: %s", hipGetErrorString(e));
    return 0;
}

/* test hook: the finalizer wave's functions on caller-supplied operands in this pool's geometry (enc_selftest.h finalizer_selftest lists
 * the modes).  The task and the chain descriptor are built in device memory as a submit builds them, pointing into one allocation:
 *   args (all modes that have slices): [5] nslices, [10..26] slice_row[17]
 *   1 splice  args: [0] slice_type, [1] hdr_nal, [2] hdr_nbits, [3] / [4] low / high word of hdr_bits, [6] arena_reset, [7] cursor,
 *                   [8] arena capacity, [9] guard bytes behind it
 *             in:   h264e_rowmeta_t[nmby] | int32 far_reads[nmby] | per row its first (nbits + 31)/32 words, row after row
 *             out:  int32 hdr[32] | the arena, capacity + guard bytes; it holds 0xA5 wherever the splice did not write
 *   2 walk    args: [1] per-macroblock candidates, [2..3] start state, [6] n, [7..8] the frame's candidate pair, [32..32+n) upto values
 *             in:   h264e_mbrec_t[nmb] | mv32 per_mb[nmb][2] (with args[1])
 *             out:  int32 hdr[32] | mv32 traj[2][nmb][2] (0xA5 bytes where nothing was written)
 *   3 step    args: [0] n     in: n x 3 int32     out: n x 5 int32 */
#ifdef H264E_EMU
/* the emulation's launch: the one wave as a lane loop (here, not in the emulation's backend, so that a backend written before this hook still builds) */
static void bk_launch_finalizer_selftest(const h264e_geom_t &G, const h264e_frame_task_t *task, int mode, const int *args, const int32_t *in, int32_t *hdr, mv32 *traj, hipStream_t)
{
    finalizer_selftest(G, *task, mode, args, in, hdr, traj);
}
#endif
extern "C" int h264e_hip_selftest_finalizer(h264e_hip_pool_t *p, int mode, const int *args /* [96] */, const uint8_t *in, uint32_t nin, uint8_t *out, uint32_t nout)
{
    if (!p || !args || !in || !out || mode < 1 || mode > 3) FAIL("selftest_finalizer: bad argument");
    const h264e_geom_t &G = p->G;
    const size_t A = 256;
    const auto up = [&](size_t n) { return (n + A - 1) & ~(A - 1); };
    h264e_frame_task_t T;
    h264e_chain_dev_t D;
    memset(&T, 0, sizeof(T)); memset(&D, 0, sizeof(D));
    T.active = 1;
    size_t in_bytes = 0, out_bytes = 0, row_off = 0;
    if (mode != 3)
    {
        T.nslices = args[5];
        if (T.nslices < 1 || T.nslices > H264E_MAX_SLICES || T.nslices > G.nmby || args[10] != 0 || args[10 + T.nslices] != G.nmby) FAIL("selftest_finalizer: bad slice rows");
        for (int k = 0; k <= T.nslices; k++)
        {
            if (k && args[10 + k] <= args[10 + k - 1]) FAIL("selftest_finalizer: bad slice rows");
            T.slice_row[k] = (int16_t)args[10 + k];
        }
    }
    const h264e_rowmeta_t *meta = (const h264e_rowmeta_t *)in;
    if (mode == 1)
    {
        const uint32_t cap = (uint32_t)args[8], guard = (uint32_t)args[9];
        row_off = (size_t)G.nmby*(sizeof(h264e_rowmeta_t) + sizeof(int));
        if (args[2] < 0 || args[2] > 56 || cap > (4u << 20) || guard > 4096u || (uint32_t)args[7] > (4u << 20) || nin < row_off) FAIL("selftest_finalizer: bad splice argument");
        in_bytes = row_off;
        for (int r = 0; r < G.nmby; r++)
        {
            if (meta[r].nbits > (uint32_t)G.row_words*32u || meta[r].lead_skips < 0 || meta[r].lead_skips > G.nmbx || meta[r].trail_skips < 0 || meta[r].trail_skips > G.nmbx)
                FAIL("selftest_finalizer: bad row %d", r);
            in_bytes += 4*(size_t)((meta[r].nbits + 31) >> 5);
        }
        out_bytes = FZ_HDR_INTS*4 + (size_t)cap + guard;
        T.slice_type = args[0]; T.hdr_nal = args[1]; T.hdr_nbits = args[2]; T.hdr_bits = (uint64_t)(uint32_t)args[3] | ((uint64_t)(uint32_t)args[4] << 32);
        T.arena_reset = args[6];
        D.arena_cap = cap;
    } else if (mode == 2)
    {
        const int n = args[6];
        if (n < 1 || n > FZ_NARGS - 32 || args[32 + n - 1] != G.nmby - 1) FAIL("selftest_finalizer: bad walk argument");
        for (int i = 0; i < n; i++) if (args[32 + i] < 0 || args[32 + i] >= G.nmby) FAIL("selftest_finalizer: bad walk argument");
        in_bytes = (size_t)G.nmb*(sizeof(h264e_mbrec_t) + (args[1] ? 2*sizeof(mv32) : 0));
        out_bytes = FZ_HDR_INTS*4 + (size_t)G.nmb*16;
        T.clusters[0] = args[7]; T.clusters[1] = args[8];
    } else
    {
        if (args[0] < 1 || args[0] > FZ_STEP_MAX) FAIL("selftest_finalizer: bad step argument");
        in_bytes = (size_t)args[0]*12; out_bytes = (size_t)args[0]*20;
    }
    if (nin != in_bytes || nout != out_bytes) FAIL("selftest_finalizer: operands of %u / %u bytes where mode %d takes %zu / %zu", nin, nout, mode, in_bytes, out_bytes);
    /* one allocation: task | chain descriptor | args | input | row bit buffers (splice) | frame record + cursor | output */
    const size_t oT = 0, oD = oT + up(sizeof(T)), oA = oD + up(sizeof(D)), oIn = oA + up(FZ_NARGS*sizeof(int)), oRows = oIn + up(in_bytes);
    const size_t oF = oRows + (mode == 1 ? up((size_t)G.nmby*G.row_words*4) : 0), oOut = oF + up(sizeof(h264e_frameout_t) + 16), total = oOut + up(out_bytes);
    uint8_t *buf = 0;
    HIPCHK(hipSetDevice(p->device));
    if (hipMalloc((void **)&buf, total) != hipSuccess) FAIL("selftest_finalizer: device allocation failed");
    uint8_t *const body = buf + oOut + FZ_HDR_INTS*4;
    D.rowmeta = (h264e_rowmeta_t *)(buf + oIn); D.far_reads = (int *)(buf + oIn + (size_t)G.nmby*sizeof(h264e_rowmeta_t));
    D.rowbits = (uint32_t *)(buf + oRows);
    D.mbrec = (h264e_mbrec_t *)(buf + oIn);
    D.fout = (h264e_frameout_t *)(buf + oF); D.cursor = (uint32_t *)(buf + oF + sizeof(h264e_frameout_t));
    D.arena = body;
    T.chain_desc = (const h264e_chain_dev_t *)(buf + oD);
    if (mode == 2 && args[1]) T.clusters_per_mb = (const mv32 *)(buf + oIn + (size_t)G.nmb*sizeof(h264e_mbrec_t));
    hipError_t e = hipMemset(buf + oF, 0, oOut - oF + FZ_HDR_INTS*4);
    if (e == hipSuccess && mode != 3) e = hipMemset(body, 0xA5, out_bytes - FZ_HDR_INTS*4);
    if (e == hipSuccess) e = hipMemcpy(buf + oT, &T, sizeof(T), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + oD, &D, sizeof(D), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + oA, args, FZ_NARGS*sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + oIn, in, mode == 1 ? row_off : in_bytes, hipMemcpyHostToDevice);
    if (mode == 1)
    {
        const uint32_t cursor = (uint32_t)args[7];
        const uint8_t *src = in + row_off;
        if (e == hipSuccess) e = hipMemcpy(D.cursor, &cursor, 4, hipMemcpyHostToDevice);
        for (int r = 0; r < G.nmby && e == hipSuccess; r++)
        {
            const size_t n = 4*(size_t)((meta[r].nbits + 31) >> 5);
            if (n) e = hipMemcpy(buf + oRows + (size_t)r*G.row_words*4, src, n, hipMemcpyHostToDevice);
            src += n;
        }
    }
    if (e == hipSuccess)
    {
        int32_t *hdr = (int32_t *)(buf + oOut);
        bk_launch_finalizer_selftest(G, (const h264e_frame_task_t *)(buf + oT), mode, (const int *)(buf + oA), (const int32_t *)(buf + oIn), hdr, (mv32 *)body, p->stream);
        e = hipStreamSynchronize(p->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(out, buf + oOut, out_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) FAIL("selftest_finalizer: %s", hipGetErrorString(e));
    return 0;
}

/* diagnostic: per-phase cycle sums of the -DH264E_STAMPS build, summed over chains (zeros in the product build): [0..31] the rows'
 * phases, [32..47] the finalizer workgroups' (10 ns ticks of the constant 100 MHz clock) */
extern "C" int h264e_hip_stamps_read(h264e_hip_pool_t *p, unsigned long long *dst /* [48] */, int reset)
{
    if (!p || !dst) FAIL("stamps_read: bad argument");
    memset(dst, 0, 48*sizeof(unsigned long long));
    for (int c = 0; c < p->nchains; c++)
    {
        unsigned long long t[48];
        HIPCHK(hipSetDevice(p->device));
        HIPCHK(hipMemcpy(t, p->chains_host[c].prof, sizeof(t), hipMemcpyDeviceToHost));
        if (reset) HIPCHK(hipMemset(p->chains_host[c].prof, 0, sizeof(t)));
        for (int i = 0; i < 48; i++) dst[i] += t[i];
    }
    return 0;
}

/* macroblocks this pool's rows have reconstructed since the last reset -- everything the kernel worked on, including frames that a
 * mis-speculation or a rate-control miss threw away.  Call after h264e_hip_sync. */
extern "C" int h264e_hip_mb_counter(h264e_hip_pool_t *p, unsigned long long *count, int reset)
{
    if (!p || !count) FAIL("mb_counter: bad argument");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpy(count, p->mb_counter, sizeof(*count), hipMemcpyDeviceToHost));
    if (reset) HIPCHK(hipMemset(p->mb_counter, 0, sizeof(*count)));
    return 0;
}

extern "C" void h264e_hip_profile(h264e_hip_pool_t *p, int enable)
{
    if (!p) return;
    p->profile = enable; p->prof_launches = 0; p->prof_mb_ms = p->prof_splice_ms = 0;
}

extern "C" int h264e_hip_profile_read(h264e_hip_pool_t *p, double *mb_ms, double *splice_ms, int *launches)
{
    if (!p) FAIL("profile_read: null pool");
    if (mb_ms) *mb_ms = p->prof_mb_ms;
    if (splice_ms) *splice_ms = p->prof_splice_ms;
    if (launches) *launches = p->prof_launches;
    return 0;
}

extern "C" int h264e_hip_timer_start(h264e_hip_pool_t *p)
{
    if (!p) FAIL("timer_start: null pool");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipEventRecord(p->ev_t0, p->stream));
    return 0;
}

extern "C" int h264e_hip_timer_stop(h264e_hip_pool_t *p, double *ms)
{
    if (!p || !ms) FAIL("timer_stop: null argument");
    *ms = 0;
    float f = 0;
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipEventRecord(p->ev_t1, p->stream));
    HIPCHK(hipEventSynchronize(p->ev_t1));
    HIPCHK(hipEventElapsedTime(&f, p->ev_t0, p->ev_t1));
    *ms = f;
    return 0;
}

#endif
