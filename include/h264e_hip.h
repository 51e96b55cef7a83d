/*
 * h264e_hip.h -- thin C ABI over the HIP kernels of the per-frame encode path (libh264e_mi355x.so).
 *
 * This is the device boundary the C host code (h264e_host.c: H264E_sizeof / H264E_init / H264E_encode,
 * encode_app) sits on.  It replaces, for the macroblock loop, the reference's internal call
 *     H264E_encode_one -> encode_slice -> mb_encode          (/root/reference/src/h264-lab.h:6477, :6409, :5724)
 * i.e. everything the reference reaches through its function table h264e_* (h264-lab.h:3274-3364).
 * Plain pointers and sizes only; no C++ or torch types.
 *
 * A POOL holds `nchains` slots of one picture geometry on one GPU (picture, row bit buffers, per-macroblock
 * records, ONE result).  One h264e_hip_submit() call launches the macroblock kernel once for up to nchains
 * jobs (one wavefront per macroblock row plus one finalizer wavefront per job that splices the slices and exports
 * the job's result to the host-mapped mirrors of its slot, where h264e_hip_stream_* picks it up):
 *  - frame at a time (stream_mode = 0): job c is the next frame of chain c, which keeps two pictures in
 *    reference / reconstruction ping-pong (H264E_encode);
 *  - stream mode: the jobs are consecutive frames of ONE stream, run as a temporal wavefront (a P frame starts
 *    while its reference frame is a few macroblock rows ahead); finished frames can be
 *    consumed while the launch runs.
 * Calls are asynchronous on the pool's stream until h264e_hip_sync().
 */
#ifndef H264E_HIP_H
#define H264E_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct h264e_hip_pool h264e_hip_pool_t;

/* one frame of one chain */
typedef struct
{
    int active;                 /* 0: chain idles in this step */
    int frame_index;            /* which resident input frame (see h264e_hip_upload_*) */
    int slice_type;             /* 0 = P, 2 = I   (h264-lab.h:3203-3204) */
    int qp;                     /* frame QP, 10..51 */
    int speed;                  /* H264E_run_param_t.encode_speed (h264-lab.h:181) */
    /* slice header (h264-lab.h:4182-4333) as a template: NAL header byte, then ue(first_mb_in_slice) -- written by the kernel
     * for every slice -- then `hdr_nbits` <= 56 tail bits (slice_type ... deblocking fields), right-aligned in hdr_bits */
    int hdr_nal;
    int hdr_nbits;
    uint64_t hdr_bits;
    /* row-band slices (h264-lab.h:6511-6574, the reference's H264E_MAX_THREADS build): 0 / 1 = one slice per frame; N > 1 =
     * N slices of consecutive macroblock rows, split like the reference (h264-lab.h:6530); <= H264E_HIP_MAX_SLICES */
    int nslices;
    int32_t mv_clusters[2];     /* speculated enc->mv_clusters for the whole frame (h264-lab.h:766) */
    const int32_t *mv_clusters_per_mb;  /* optional HOST array [nmb][2]: exact per-macroblock values (re-encode path) */
    uint16_t qdat[2][42];       /* quantizer tables of rc_set_qp (h264-lab.h:5839-5912) */
    /* temporal wavefront (stream_mode = 1): the tasks of one submit are consecutive frames of ONE stream, in order;
     * task i builds the picture of chain slot `slot` and references the picture of `ref_slot` (-1: none, I slice),
     * which is either complete or (ref_in_flight) being built by an earlier task of this same submit, a few rows ahead */
    int stream_mode, slot, ref_slot, ref_in_flight;
    /* stream mode: encode this frame again from macroblock row first_row; the rows above it (bits, records, picture) are
     * kept from the previous encode of the same frame in the same slot (0 = whole frame) */
    int first_row;
    /* stream mode, device walk: index + 1 of the task whose verdict this frame's walk starts from; 0 = the task in front of it */
    int walk_parent;
    /* ... and a frame whose failed validation concerns nobody but itself (a leaf): it reports the verdict but does not stop the launch */
    int walk_quiet;
    /* stream mode: the job's finalizer validates the mv_clusters speculation ON THE DEVICE (exact walk over the frame's records,
     * enc_finalize.h device_clusters_walk): task 0 of a submit starts from exact_state, task i from the verdict of task i-1; a mismatch
     * stops the launch (device abort word) and is reported in the result (walk_status, first_bad, state_out); the walked
     * per-macroblock trajectory stays on the device and becomes the candidates of a re-encode with traj_from_device */
    int walk_on_device;
    int32_t exact_state[2];
    int traj_from_device;
    /* stream mode: 1 = narrow valid window (53 x 52 samples, consecutive frames 4 macroblock steps apart), 0 = the whole
     * 64 x 64 window (7 steps apart); see h264e_dev.h.  Same bits either way. */
    int narrow_window;
    /* 1 = encode the denoised picture of resident slot frame_index (h264e_hip_denoise_frames) instead of the raw input; the
     * sums of squared differences (h264e_hip_ssd_frames) keep reading the raw input */
    int denoised;
} h264e_hip_task_t;

#define H264E_HIP_MAX_SLICES 16

typedef struct
{
    uint32_t nbytes;            /* bytes of the frame's slice RBSPs as exported: slice k starts at the sum of the 16-byte-rounded sizes before it */
    int nslices;
    uint32_t slice_nbytes[H264E_HIP_MAX_SLICES];   /* RBSP bytes of each slice NAL (header byte included, no start code, no escapes) */
    int all_skipped;            /* every macroblock was skipped (rc_frame_end's skip_flag, h264-lab.h:6596) */
    int clusters_moved;         /* the speculated mv_clusters state is not a fixed point of this frame */
    int overflow;               /* a bit buffer overflowed: the result is invalid */
    int far_reads;              /* reference accesses that left the valid window and took the HBM path (stream mode) */
    int in_device;              /* the NALs did not fit the host-mapped mirror: h264e_hip_stream_fetch_nals() gets them */
    int walk_status;            /* device-side validation: 0 not done, 1 ok, 2 this frame consumed wrong candidates (first_bad), 3 void (a frame before it failed) */
    int first_bad;
    int32_t state_out[2];       /* ok: exact mv_clusters behind the frame; bad: the walk's end state */
} h264e_hip_result_t;

typedef struct { int32_t mv0; int8_t type; uint8_t used_cand; uint8_t pad[2]; } h264e_hip_mbrec_t;

int  h264e_hip_device_count(void);
/* frames_resident: input frames kept in HBM */
int  h264e_hip_pool_create(h264e_hip_pool_t **pool, int device, int width, int height, int nchains,
                           int frames_resident);
void h264e_hip_pool_destroy(h264e_hip_pool_t *pool);
/* packed I420 frames (width*height*3/2 bytes each) from host memory into resident slots first.. */
int  h264e_hip_upload_i420(h264e_hip_pool_t *pool, int first, int nframes, const uint8_t *host_i420);
/* the same from pinned host memory (h264e_hip_host_alloc) on the pool's copy stream, concurrently with kernels on the encode
 * stream; h264e_hip_upload_wait() blocks until every such copy has landed */
int  h264e_hip_upload_i420_async(h264e_hip_pool_t *pool, int first, int nframes, const uint8_t *pinned_i420);
int  h264e_hip_upload_wait(h264e_hip_pool_t *pool);
int  h264e_hip_upload_busy(h264e_hip_pool_t *pool);         /* 1 while such a copy is still in flight, 0 when all have landed, -1 when the copy stream failed */
void *h264e_hip_host_alloc(size_t bytes);
void h264e_hip_host_free(void *p);
/* one frame from three planes with arbitrary strides (the H264E_io_yuv_t of the drop-in API) */
int  h264e_hip_upload_planes(h264e_hip_pool_t *pool, int index, const uint8_t *const yuv[3], const int stride[3]);
/* Device-resident input (enc_ingest.h): one frame that already lies in this pool's device memory -- format 0 = I420 (three planes),
 * 1 = NV12 (Y, interleaved UV), 2 = interleaved RGB of pixel_bytes 3 or 4 (BT.601 limited range, integer), 3 = planar RGB (three planes
 * R, G, B, the same arithmetic); 3 | 0x10 / 0x20 / 0x30 = planar RGB of float16 / bfloat16 / float32 samples in [0, 1], quantised to
 * 8 bits as they are loaded (enc_ingest.h fq_quant; pointers and strides multiples of the sample's size; a sample type on another
 * format is refused) -- into resident slot `slot`,
 * by ONE kernel launch on the pool's copy stream.  planes / strides: a pointer and a row stride in bytes (>= the row's bytes) per
 * source plane; unused entries are ignored.  producer_stream: the hipStream_t whose queued work writes the source (the launch waits
 * for everything queued there so far), or NULL when the caller has synchronised.  Returns when the slot has been written: the source
 * may be reused at once.  Refused without a launch: a NULL plane, a short stride, an unknown format / pixel_bytes, a slot out of range,
 * and a plane that the runtime does not report as memory of the pool's device.  The slot must not be the input of a frame that a
 * running launch still encodes (the bounded-ring rule of H264E_clip_upload).
 * _async: the same without the final wait; h264e_hip_upload_wait() completes every ingest issued so far.
 * _check: the refusals alone (0 = this frame would be accepted), nothing is launched. */
int  h264e_hip_ingest_check(h264e_hip_pool_t *pool, int slot, int format, const void *const planes[3], const int strides[3], int pixel_bytes);
int  h264e_hip_ingest_device(h264e_hip_pool_t *pool, int slot, int format, const void *const planes[3], const int strides[3], int pixel_bytes, void *producer_stream);
int  h264e_hip_ingest_device_async(h264e_hip_pool_t *pool, int slot, int format, const void *const planes[3], const int strides[3], int pixel_bytes, void *producer_stream);
/* The matrix that later RGB / RGBP ingest and scale launches of this pool convert with: bt709 0 = BT.601, 1 = BT.709; full_range 0 =
 * limited (16..235 / 16..240), 1 = full (0..255).  A new pool has (0, 0).  Slots already written keep their bytes. */
int  h264e_hip_set_color(h264e_hip_pool_t *pool, int bt709, int full_range);
/* HDR10 input (enc_tonemap.h): while it is on, h264e_hip_ingest_device / _scale_device and their _async and _check forms take only 16-bit
 * I420 / NV12 frames of depth 10 .. 16 (every other format is refused by name, nothing is launched) and tone-map them -- PQ transfer,
 * BT.2020 NCL limited range in; 8-bit BT.709 R'G'B' converted by the matrix of h264e_hip_set_color out -- by ONE launch of
 * h264e_tonemap_kernel on the copy stream, ordered and completed like the ingest.  Through a window: that launch writes the tone-mapped
 * window into a scratch surface of the pool (8-bit I420, sized on first use, reused, freed with the pool) and the scale kernel of an
 * I420 source runs from it: two launches.  transfer 0 = off (a new pool; launches, bytes and allocations are those of a pool that never
 * heard of it), 1 = PQ; curve 0 = hable, 1 = reinhard, 2 = clip; peak_nits 0 = 1000, ref_white_nits 0 = 203.  _set uploads the tables
 * (9 KB of device memory, allocated the first time it is switched on); `who` names the caller in the refusals.  _check: the refusals of
 * the parameters alone.  _tables: the tables the kernel will use for these parameters, by the one function _set uses; ycc = ky, crv,
 * cgu, cgv, cbu in Q14, then 64, 512, 14.  _state: state[0] = on, state[1] = bytes of the device table buffer, state[2] = bytes of the
 * scratch surface (0 = not allocated). */
int  h264e_hip_tonemap_check(const char *who, int transfer, int curve, double peak_nits, double ref_white_nits);
int  h264e_hip_tonemap_set(h264e_hip_pool_t *pool, const char *who, int transfer, int curve, double peak_nits, double ref_white_nits);
int  h264e_hip_tonemap_tables(int transfer, int curve, double peak_nits, double ref_white_nits, int ycc[8], float eotf[1024], float scale[1024], float thresh[256]);
int  h264e_hip_tonemap_state(const h264e_hip_pool_t *pool, long long state[3]);
/* Device-resident input of another size (enc_scale.h): a window of an I420 or NV12 source frame is reduced to the pool's picture by an
 * exact area filter, by ONE kernel launch on the copy stream, ordered and completed like h264e_hip_ingest_device.  Planar RGB (format 3,
 * enc_scale_rgb.h): each channel is reduced by that filter at luma geometry, the result converted as the ingest does.  win = six ints:
 * src_width, src_height, crop_x, crop_y, crop_width, crop_height (crop_width 0 = the whole source).  Refused without a launch, besides
 * what the ingest refuses: interleaved RGB, an odd or negative window value, a window that leaves the source, is smaller than the picture, larger
 * than 4096 samples or more than 16 times the picture in an axis, and a plane whose bytes from the window's first to its last -- by the
 * SOURCE's size and stride -- are not inside one allocation of the pool's device. */
int  h264e_hip_scale_check(h264e_hip_pool_t *pool, int slot, int format, const void *const planes[3], const int strides[3], const int *win);
int  h264e_hip_scale_device(h264e_hip_pool_t *pool, int slot, int format, const void *const planes[3], const int strides[3], const int *win, void *producer_stream);
int  h264e_hip_scale_device_async(h264e_hip_pool_t *pool, int slot, int format, const void *const planes[3], const int strides[3], const int *win, void *producer_stream);
/* HIP-event time of what is queued on the copy stream between the two calls (the ingest / scale launches of the probes); _stop waits */
int  h264e_hip_copy_timer_start(h264e_hip_pool_t *pool);
int  h264e_hip_copy_timer_stop(h264e_hip_pool_t *pool, double *ms);
/* plain device memory and blocking copies, for callers that have no HIP toolchain of their own (to_device: 1 host -> device, 0 back) */
void *h264e_hip_dev_malloc(int device, size_t bytes);
void h264e_hip_dev_free(void *p);
int  h264e_hip_dev_memcpy(void *dst, const void *src, size_t bytes, int to_device);
/* fill resident frames [first, first+n) with the synth_v1 test clip ON THE DEVICE (bench input, already in HBM) */
int  h264e_hip_generate_synth(h264e_hip_pool_t *pool, int first, int nframes, int t0, uint32_t seed);
int  h264e_hip_submit(h264e_hip_pool_t *pool, const h264e_hip_task_t *tasks /* [nchains] */);
/* Temporal denoiser (the reference's h264e_denoise_run, enc_denoise.h).  reset: allocates the denoised frames on first use (one per
 * resident input slot -- two for a single-slot pool, which ping-pongs -- plus the zero state) and zeroes them.  frames: denoises
 * resident input slots first, first + 1, ... (mod frames_resident) in order on the pool's stream, one kernel launch per frame, after
 * every upload issued on the copy stream; the first one's previous picture is the zero state (from_zero) or the denoised picture of
 * the slot in front of it, each later one that of the frame before it.  read_denoised: the denoised picture of a slot (test hook). */
int  h264e_hip_denoise_reset(h264e_hip_pool_t *pool);
int  h264e_hip_denoise_frames(h264e_hip_pool_t *pool, int first, int n, int from_zero);
int  h264e_hip_read_denoised(h264e_hip_pool_t *pool, int slot, uint8_t *dst);
/* Scene-cut detection (enc_scenecut.h): the 64-bin luma histograms (Y >> 2) of resident input slots first, first + 1, ... (mod
 * frames_resident), one kernel launch per frame on the pool's stream after every upload issued on the copy stream, read back into
 * hist [n][64] on return (the call waits for the stream).  The device records are allocated on first use.  kernel_ms (optional): the HIP-event
 * time of the launches of this call. */
int  h264e_hip_scenecut_frames(h264e_hip_pool_t *pool, int first, int n, uint32_t *hist, float *kernel_ms);
/* Cost pass of the lookahead rate control (enc_lookahead.h): the records {I, P, N} of STREAM frames first, first + 1, ... (input slot
 * f % frames_resident; n <= frames_resident), one kernel launch per frame in order on the pool's stream after every upload issued on
 * the copy stream, read back into rec [n][3] on return (the call waits for the stream).  Frame f > 0 is measured against the
 * half-resolution picture that the pass made of frame f - 1, kept in a ring of the pool (allocated on first use): frames must be
 * analysed in order, and f - 1 no more than the ring's length before.  Refused below 16x16.  kernel_ms (optional): as above. */
int  h264e_hip_lookahead_frames(h264e_hip_pool_t *pool, int first, int n, unsigned long long *rec, float *kernel_ms);
/* The same pass with a motion search of +-range half-resolution samples per block, range in 1..8 (enc_lookahead_search.h): P and N of
 * the records come from the searched inter cost, and every analysed frame's motion field -- one cell {int8 dx, int8 dy, uint16 cost}
 * per block, nbx x nby = ((width/2) >> 3) x ((height/2) >> 3) of them, row by row -- goes into a field ring of the pool with the entries of
 * the half-resolution ring (allocated on first use).  The half-resolution entries are those of the call above: frames analysed with and
 * without search may follow each other. */
int  h264e_hip_lookahead_search_frames(h264e_hip_pool_t *pool, int first, int n, int range, unsigned long long *rec, float *kernel_ms);
/* The field ring's entry of STREAM frame `frame` (entry frame % max(frames_resident, 2)) into dst [nbx*nby*4 bytes]; the call waits for
 * the stream.  Which frame the entry holds is the caller's to know.  Refused before the first call with a search. */
int  h264e_hip_lookahead_read_field(h264e_hip_pool_t *pool, int frame, void *dst);
/* Cost tree over the motion field (enc_lookahead_tree.h): one run over STREAM frames [first, first + n), n at most the field ring's
 * entries, whose half-resolution pictures and fields are in their rings (analysed with a search, and not overwritten since).  The
 * frames' block maps in_f -- uint64 [nby][nbx], in a ring beside the field ring with the same entries and indexing, allocated on first
 * use -- are zeroed, then one kernel launch per frame runs on the pool's stream in REVERSE frame order: frame f adds what it received
 * into its sum and, unless key[f - first] is set or f == first, passes its blocks' amounts on into in_{f-1}.  sums [n] on return (the
 * call waits for the stream): S(f) = min(sum over the blocks of min(in_f, 2^40), 2^48).  kernel_ms (optional): as above.  read_tree: the
 * map ring's entry of STREAM frame `frame` into dst [nbx*nby*8 bytes]; which frame and which run the entry holds is the caller's to
 * know.  Both are refused while the pool has no field ring. */
int  h264e_hip_lookahead_tree_frames(h264e_hip_pool_t *pool, int first, int n, const uint8_t *key, unsigned long long *sums, float *kernel_ms);
int  h264e_hip_lookahead_read_tree(h264e_hip_pool_t *pool, int frame, void *dst);
/* Motion-compensated temporal denoiser (enc_mcdenoise.h), a sibling of h264e_hip_denoise_frames: STREAM frames first, first + 1, ...
 * (input slot f % frames_resident, n <= frames_resident) are filtered against the previous denoised picture displaced by frame f's
 * entry of the field ring, one kernel launch per frame in order on the pool's stream after every upload issued on the copy stream.
 * It writes the SAME denoised ring (slot f % frames_resident, the zero state with from_zero, the single-slot pool's ping-pong), so a
 * task's `denoised` flag and h264e_hip_read_denoised work as they do for the plain denoiser; h264e_hip_denoise_reset comes first.
 * mode: 1 = the field's vectors, 2 = refined by one luma sample with a zero-vector candidate.  Each frame's vectors -- one cell {int8
 * vx, int8 vy, uint16 sad} per block, in luma samples -- go into a ring beside the field ring (same entries, same indexing, allocated
 * on first use).  Refused while the pool has no field ring (no searched cost pass has run), and below 16x16.
 * read_vectors: that ring's entry of STREAM frame `frame` into dst [nbx*nby*4 bytes]; the call waits for the stream; which frame the
 * entry holds is the caller's to know.  time: the HIP-event time of the filter's launches since the pool was created and the frames
 * they filtered (the call waits for the last ones). */
int  h264e_hip_mcdenoise_frames(h264e_hip_pool_t *pool, int first, int n, int mode, int from_zero);
int  h264e_hip_mcdenoise_read_vectors(h264e_hip_pool_t *pool, int frame, void *dst);
int  h264e_hip_mcdenoise_time(h264e_hip_pool_t *pool, double *kernel_ms, long long *frames);
/* Launch groups: the submits of the member pools (same device, same picture size, one host thread each) are merged into ONE kernel
 * launch per round -- the streams' jobs interleaved in dispatch order, every job with its own pool's buffers / abort word / results --
 * so that independent streams fill each other's pipeline drains.  h264e_hip_submit of a member blocks until all members that are
 * still in the group have submitted (or left); h264e_hip_sync returns when the merged launch has drained. */
typedef struct h264e_hip_group h264e_hip_group_t;
int  h264e_hip_group_create(h264e_hip_group_t **group, int device);
int  h264e_hip_group_join(h264e_hip_group_t *group, h264e_hip_pool_t *pool);
void h264e_hip_group_leave(h264e_hip_group_t *group, h264e_hip_pool_t *pool);
void h264e_hip_group_destroy(h264e_hip_group_t *group);
int  h264e_hip_sync(h264e_hip_pool_t *pool);
/* results: every job has a finalizer inside the launch that copies its NALs and macroblock records to the host-mapped
 * mirrors of its chain slot (stream mode: task.slot; else the task's index) and raises a done word, so the host can
 * consume frame after frame while later frames of the same launch are still running.
 * h264e_hip_stream_done: 0 not finished, 1 finished (res filled), 2 aborted. */
/* A pool owns its device's launch lock (process-wide, one persistent launch at a time per device) from its first submit until
 * h264e_hip_sync returns; h264e_hip_release gives it back after a failure in between (waits for the stream, reports nothing). */
void h264e_hip_release(h264e_hip_pool_t *pool);
int  h264e_hip_stream_done(h264e_hip_pool_t *pool, int slot, h264e_hip_result_t *res);
const uint8_t *h264e_hip_stream_rbsp(h264e_hip_pool_t *pool, int slot);
const h264e_hip_mbrec_t *h264e_hip_stream_mbrec(h264e_hip_pool_t *pool, int slot);
/* a per-macroblock trajectory of `slot` ([nmb][2]): consumed = 0 the one its last device walk produced (what a re-encode with
 * traj_from_device will consume), 1 the one its last encode consumed (traj_from_device) */
int  h264e_hip_stream_fetch_traj(h264e_hip_pool_t *pool, int slot, int consumed, int32_t *dst);
int  h264e_hip_stream_fetch_nals(h264e_hip_pool_t *pool, int slot, uint8_t *dst, uint32_t nbytes);
/* after the launch has drained: the reconstructed picture of slot `from` becomes the picture of slot `to` (a frame that was
 * encoded in a spare slot is moved to the slot its frame number owns) */
int  h264e_hip_stream_copy_picture(h264e_hip_pool_t *pool, int from, int to);
/* resident input frames back to the host (measurement helper) */
int  h264e_hip_download_i420(h264e_hip_pool_t *pool, int first, int nframes, uint8_t *host_i420);
int  h264e_hip_stream_abort(h264e_hip_pool_t *pool);
/* macroblock rows of `slot`, from the top, that the last launch completed (after h264e_hip_sync, before the next submit): what a task
 * for the same frame in the same slot may pass as first_row -- up to all of them, then only the job's finalizer runs */
int  h264e_hip_stream_rows_complete(h264e_hip_pool_t *pool, int slot, int *rows);
/* Key frames behind a launch's first job have their row workgroups dispatched FIRST, as far as a budget of row workgroups goes (DESIGN.md
 * 5; what they encode before a stop is what h264e_hip_stream_rows_complete reports afterwards).  budget < 0: the default (a quarter of
 * the kernel variant's resident workgroups), 0: off, N: that many.  _last_lead: what the pool's last submit led -- key frames, their
 * row workgroups, the last led job (-1: none); any pointer may be NULL. */
void h264e_hip_set_key_lead(h264e_hip_pool_t *pool, int budget);
void h264e_hip_last_lead(h264e_hip_pool_t *pool, int *jobs, int *rows, int *last);
int  h264e_hip_busy(h264e_hip_pool_t *pool);
/* reconstructed picture of the chain's last frame, coded size, packed I420 */
int  h264e_hip_read_recon(h264e_hip_pool_t *pool, int chain, uint8_t *dst);
/* stream pools: the picture of chain slot `slot` (coded size, packed I420) */
int  h264e_hip_read_recon_slot(h264e_hip_pool_t *pool, int slot, uint8_t *dst);
/* Device-resident output (enc_egress.h), the way back of h264e_hip_ingest_device: a reconstructed picture, cropped to the pool's width x
 * height, into device memory of the pool's device in one of the ingest's four formats (RGB / RGBP: converted by the inverse of the matrix
 * h264e_hip_set_color selected, chroma replicated over its 2x2 block, a fourth byte of an RGB pixel written as 255; 3 | 0x10 / 0x20 /
 * 0x30: the planar RGB values v as float16 / bfloat16 / float32 v / 255, enc_egress.h egr_float_sample), by ONE kernel launch
 * on the pool's copy stream.  planes / strides: a pointer and a row stride in bytes (>= the row's bytes) per destination plane, counted
 * as for a source; only the rows' bytes are written, never the padding between them.  _slot: the picture h264e_hip_read_recon_slot
 * reads; _last: the one h264e_hip_read_recon reads.  producer_stream: the hipStream_t whose queued work may still use the destination
 * (the launch waits for everything queued there so far), or NULL; the launch also waits for the pool's encode stream.  Returns when the
 * destination has been written.  Refused without a launch (h264e_hip_last_error names the value): null arguments, a slot out of range,
 * an unknown format / pixel_bytes, a NULL plane, a short stride, and a plane that the runtime does not report as memory of the pool's
 * device inside one allocation from the first byte written to the last.
 * _check: the refusals alone (0 = this destination would be accepted), nothing is launched.
 * _time: enable != 0 times the later launches with HIP events; ms / calls: the totals since the pool was created (tools/egress_probe.py). */
int  h264e_hip_egress_check(h264e_hip_pool_t *pool, int slot_or_chain, int format, void *const planes[3], const int strides[3], int pixel_bytes);
int  h264e_hip_egress_slot(h264e_hip_pool_t *pool, int slot, int format, void *const planes[3], const int strides[3], int pixel_bytes, void *producer_stream);
int  h264e_hip_egress_last(h264e_hip_pool_t *pool, int chain, int format, void *const planes[3], const int strides[3], int pixel_bytes, void *producer_stream);
int  h264e_hip_egress_time(h264e_hip_pool_t *pool, int enable, double *ms, long long *calls);
/* sums of squared differences between resident input frames and stream pictures, one small kernel per call: frame i uses input
 * slot (in0 + i) % in_mod and picture slot (pic0 + i) % pic_mod; out = host [n][3] (Y, U, V), picture size width x height */
int  h264e_hip_ssd_frames(h264e_hip_pool_t *pool, int n, int in0, int in_mod, int pic0, int pic_mod, uint64_t *out);
/* Structural similarity (enc_ssim.h: 8x8 windows in steps of 4, the SSIM of x264 and of ffmpeg's filter, per plane) of the same pairs of
 * pictures, with h264e_hip_ssd_frames' arguments and checks: out = host [n][3] (Y, U, V), each the mean over its plane's windows.  Two
 * launches on the pool's stream (tile partials, then their sums in tile order: no atomics, the values do not depend on scheduling),
 * complete on return.  A picture below 16 x 16 has a chroma plane without a window and is refused, with the size in the message.  The
 * partials and results buffer is allocated with the first call.
 * _planes: ONE pair of 8-bit planes of w x h samples in device memory (rows a_stride / b_stride bytes apart, any addresses) through the same
 * kernel; out = host [1].  Refused without a launch, with the value in the message: NULL, w or h below 8, a stride below w, and memory
 * that the runtime does not report as one allocation of the pool's device.  The caller has synchronised whatever wrote the planes.
 * _quality_last: for a pool that encodes frame at a time -- input slot 0 against the picture h264e_hip_egress_last reads for `chain`: the sums of
 * squared differences into ssd[3], the SSIM into ssim[3]; either may be NULL (SSIM: 16 x 16 at least).
 * _quality_time: enable != 0 times the later SSD and SSIM launches with HIP events; the totals since the pool was created, and the frames
 * they covered (tools/quality_probe.py). */
int  h264e_hip_ssim_frames(h264e_hip_pool_t *pool, int n, int in0, int in_mod, int pic0, int pic_mod, double *out);
int  h264e_hip_ssim_planes(h264e_hip_pool_t *pool, const void *a, int a_stride, const void *b, int b_stride, int w, int h, double *out);
int  h264e_hip_quality_last(h264e_hip_pool_t *pool, int chain, uint64_t ssd[3], double ssim[3]);
int  h264e_hip_quality_time(h264e_hip_pool_t *pool, int enable, double *ssd_ms, double *ssim_ms, long long *frames);
/* drop the chain's last submitted frame (stream_mode = 0): undo the reference/reconstruction swap, so the frame can be
 * submitted again (re-encode path) */
int  h264e_hip_rewind_frame(h264e_hip_pool_t *pool, int chain);
/* kernel timing on the pool's stream (HIP events around every macroblock-kernel launch) */
/* macroblocks the pool's rows have reconstructed since the last reset, delivered or thrown away (call after h264e_hip_sync) */
int h264e_hip_mb_counter(h264e_hip_pool_t *pool, unsigned long long *count, int reset);
void h264e_hip_profile(h264e_hip_pool_t *pool, int enable);
int  h264e_hip_profile_read(h264e_hip_pool_t *pool, double *mb_kernel_ms, double *splice_kernel_ms, int *launches);
/* diagnostic: per-phase cycle sums of a -DH264E_STAMPS build of the kernels (all zero in the product build) */
int  h264e_hip_stamps_read(h264e_hip_pool_t *pool, unsigned long long *dst /* [32] */, int reset);
/* wall clock of a region on the pool's stream, by HIP events */
int  h264e_hip_timer_start(h264e_hip_pool_t *pool);
int  h264e_hip_timer_stop(h264e_hip_pool_t *pool, double *ms);
/* self-test hook: runs the device's NAL emulation-prevention pass (enc_finalize.h nal_escape_copy, one wavefront) on n payload bytes;
 * dst receives start code + escaped payload, *out_n its size.  Used by tests with adversarial inputs (real streams need an
 * escape about once per 4 MB). */
/* test hook: the dispatch order of a launch of `jobs` jobs as (job << 16 | row) entries, 0xffffffff = padding (banded orders: eight
 * equally long per-XCD queues, h264e_pool.h build_order); returns the number of entries, -1 on failure */
long h264e_hip_selftest_order(h264e_hip_pool_t *pool, int jobs, int narrow, int banded, uint32_t *out, size_t cap);
/* test hook: the unbanded order of a launch that merges several streams (a launch group): member i contributes member_jobs[i] jobs of
 * `rows` workgroups, numbered member after member; entries sorted by lag*j + 2*row, ties by j, then member, then row */
long h264e_hip_selftest_merged_order(int rows, int lag, const int *member_jobs, int nmembers, uint32_t *out, size_t cap);
/* test hook: which key frames of such a launch are led -- their row workgroups at the front of the order (h264e_pool.h lead_jobs) -- and
 * the order that gives.  key / first_row: per launch job, member after member (key != 0: an I job that waits for no other job; the rows
 * it already has); tree / all_intra: the launch carries hedge leaves / nothing but I jobs; resident: workgroups of the launch's kernel
 * variant that the chip holds; budget: row workgroups that may be led; banded != 0: through the XCD bands (one member); led_out, when
 * not NULL, gets one byte per job */
long h264e_hip_selftest_lead_order(int nmby, int lag, const int *member_jobs, int nmembers, const uint8_t *key, const int *first_row,
                                   int tree, int all_intra, int resident, int budget, int banded, uint32_t *out, size_t cap, uint8_t *led_out);
int  h264e_hip_selftest_nal_escape(h264e_hip_pool_t *pool, const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t cap, uint32_t *out_n);
/* test hook: one wave-level stage of the macroblock pipeline on caller-supplied operands (h264e_kernels.hip stage_selftest lists
 * the stages and their operand layouts; tests/test_stages.py and tests/test_stage_edges.py compare them with the reference's own functions) */
int  h264e_hip_selftest_stage(h264e_hip_pool_t *pool, int stage, const uint8_t *in, uint32_t nin, const int *args /* [24] */, uint8_t *out, uint32_t nout);
/* test hook: the finalizer wave's own functions -- the slice splice, the mv_clusters walks, the single update step -- on caller-supplied
 * operands in the pool's geometry (h264e_pool.h lists the modes and operand layouts; tests/test_finalizer.py compares them with
 * tests/finalizer_model.py and tests/golden/finalizer.json) */
int  h264e_hip_selftest_finalizer(h264e_hip_pool_t *pool, int mode, const int *args /* [96] */, const uint8_t *in, uint32_t nin, uint8_t *out, uint32_t nout);
/* test hook: the host's own mv_clusters walk of one frame (h264e_host.c clusters_walk; slices split nmby evenly as the encoder splits them);
 * returns the first mismatching macroblock or -1, state = the state behind the frame, traj (optional) [nmb][2] */
int  h264e_hip_selftest_host_clusters_walk(int32_t state[2], const h264e_hip_mbrec_t *rec, int nmbx, int nmby, int nslices, const int32_t *used, int per_mb, int32_t *traj);
const char *h264e_hip_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
