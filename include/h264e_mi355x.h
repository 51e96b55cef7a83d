/*
 * h264e_mi355x.h -- the reference's public encoder API, served by the MI355X HIP path.
 *
 * Drop-in boundary: the four entry points and three structs below are what an application written
 * against /root/reference/src/h264-lab.h:1-318 links to; layouts are ABI (x86-64 LP64, built with the
 * reference's default H264E_SVC_API=1, H264E_MAX_THREADS=0: create 56 B, run 48 B, io_yuv 40 B).
 *
 *   H264E_sizeof          replaces h264-lab.h:6868-6892   (same sizes as the reference reports)
 *   H264E_init            replaces h264-lab.h:6375-6407
 *   H264E_encode          replaces h264-lab.h:6654-6861   (macroblock loop runs as HIP kernels, include/h264e_hip.h)
 *   H264E_set_vbv_state   replaces h264-lab.h:6898-6913
 *
 * Scope: AVC baseline, key and P frames, one reference frame, one slice per frame or N
 * row-band slices (H264E_set_slices / H264E_clip_param_t.slices: the reference's H264E_MAX_THREADS build),
 * constant QP or frame-level rate control, and the reference's temporal denoiser through the extension calls
 * H264E_set_denoise / H264E_clip_set_denoise (the create parameter temporal_denoise_flag itself is still refused).
 * Long-term reference frame types, SVC layers, MB-level rate control and NALU-size slicing answer
 * H264E_STATUS_BAD_PARAMETER at init / H264E_STATUS_BAD_FRAME_TYPE at encode instead of silently producing a
 * different stream.
 * The encoder needs a HIP device: without one H264E_init fails (H264E_STATUS_BAD_ARGUMENT) -- there is
 * no CPU fallback.
 */
#ifndef H264E_MI355X_H
#define H264E_MI355X_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* h264-lab.h:25-34 */
#define H264E_STATUS_SUCCESS                0
#define H264E_STATUS_BAD_ARGUMENT           1
#define H264E_STATUS_BAD_PARAMETER          2
#define H264E_STATUS_BAD_FRAME_TYPE         3
#define H264E_STATUS_SIZE_NOT_MULTIPLE_16   4
#define H264E_STATUS_SIZE_NOT_MULTIPLE_2    5
#define H264E_STATUS_BAD_LUMA_ALIGN         6
#define H264E_STATUS_BAD_LUMA_STRIDE        7
#define H264E_STATUS_BAD_CHROMA_ALIGN       8
#define H264E_STATUS_BAD_CHROMA_STRIDE      9

/* h264-lab.h:63-70 */
#define H264E_FRAME_TYPE_DEFAULT    0
#define H264E_FRAME_TYPE_KEY        6
#define H264E_FRAME_TYPE_I          5
#define H264E_FRAME_TYPE_GOLDEN     4
#define H264E_FRAME_TYPE_RECOVERY   3
#define H264E_FRAME_TYPE_P          2
#define H264E_FRAME_TYPE_DROPPABLE  1
#define H264E_FRAME_TYPE_CUSTOM     99

/* h264-lab.h:83-172 */
typedef struct H264E_create_param_tag
{
    int width;
    int height;
    int gop;                                /* key frame period; 0 = only the first frame; 1 = all intra */
    int vbv_size_bytes;                     /* selects the SPS level; VBV model for rate control */
    int vbv_overflow_empty_frame_flag;
    int vbv_underflow_stuffing_flag;
    int fine_rate_control_flag;             /* MB-level rate control: not supported (must be 0) */
    int const_input_flag;                   /* 0: the reconstruction is written back into the input planes */
    int max_long_term_reference_frames;     /* must be 0 */
    int enableNEON;                         /* ignored */
    int temporal_denoise_flag;              /* must be 0: the denoiser is switched on with H264E_set_denoise() */
    int sps_id;
    int num_layers;                         /* SVC: must be 0 or 1 */
    int inter_layer_pred_flag;
} H264E_create_param_t;

/* h264-lab.h:177-226 */
typedef struct H264E_run_param_tag
{
    int encode_speed;
    int frame_type;
    int long_term_idx_use;
    int long_term_idx_update;
    int desired_frame_bytes;
    int qp_min;
    int qp_max;
    int desired_nalu_bytes;                 /* must be 0: byte-budget slicing (h264-lab.h:6418-6430) is refused; row-band slices: H264E_set_slices() */
    void (*nalu_callback)(const unsigned char *nalu_data, int sizeof_nalu_data, void *token);
    void *nalu_callback_token;
} H264E_run_param_t;

/* h264-lab.h:231-237 */
typedef struct H264E_io_yuv_tag
{
    unsigned char *yuv[3];
    int stride[3];
} H264E_io_yuv_t;

typedef struct H264E_persist_tag H264E_persist_t;
typedef struct H264E_scratch_tag H264E_scratch_t;

int  H264E_sizeof(const H264E_create_param_t *param, int *sizeof_persist, int *sizeof_scratch);
int  H264E_init(H264E_persist_t *enc, const H264E_create_param_t *param);
int  H264E_encode(H264E_persist_t *enc, H264E_scratch_t *scratch, const H264E_run_param_t *run_param,
                  H264E_io_yuv_t *frame, unsigned char **coded_data, int *sizeof_coded_data);
void H264E_set_vbv_state(H264E_persist_t *enc, int vbv_size_bytes, int vbv_fullness_bytes);

/* ---- extensions (not in the reference) ---------------------------------------------------------------- */

/* The reference API has no destructor: device resources of an encoder are released when the
 * same persist blob is initialised again, at process exit, or explicitly here. */
void H264E_close(H264E_persist_t *enc);
/* Row-band slices per frame for the drop-in encoder: the reference selects this through H264E_create_param_t.max_threads,
 * a field that only exists when it is compiled with -DH264E_MAX_THREADS=N (h264-lab.h:142-170, :6511-6574) and that changes
 * the struct ABI; this library keeps the default ABI and takes the number here instead.  0 / 1 = one slice per frame,
 * 2..16 = N slices (deblocking idc 2, contexts / availability / mv_clusters restarted per slice).  Call after H264E_init. */
int  H264E_set_slices(H264E_persist_t *enc, int nslices);
/* The reference's temporal denoiser (h264-lab.h:1547-1621, its temporal_denoise_flag): 1 = on, 0 = off.  Only after H264E_init and
 * before the first H264E_encode; the denoiser's state starts at zero.  Every frame with encode_speed < 2 is then denoised on the
 * device and the denoised picture is encoded (the reconstruction still goes back to the caller's planes with const_input_flag = 0);
 * frames with encode_speed >= 2 are encoded raw and leave the state alone.  H264E_STATUS_BAD_PARAMETER after the first frame. */
int  H264E_set_denoise(H264E_persist_t *enc, int on);
/* Colour and frame rate of the stream, signalled in the VUI of every SPS (H.264 Annex E); with nothing set the SPS has no VUI and is
 * byte for byte the reference's.
 *   matrix: an H.264 matrix_coefficients code (Table E-5).  1 or 6 (a) selects how RGB and RGBP device input is converted from now on, at
 *   the picture's size and through a window alike, and (b) is written into every SPS as video_signal_type: video_format 5,
 *   video_full_range_flag = full_range, and a colour description with colour_primaries = transfer_characteristics = matrix_coefficients
 *   = matrix.  For I420, NV12 and host input the call only says what the caller's samples are: they are not touched.  (0, 0) returns to
 *   the default -- BT.601 limited conversion, nothing signalled; (0, 1) and every other matrix value are refused.
 *   The conversion keeps the form above, Y = ((yr R + yg G + yb B + 128) >> 8) + yo, U and V from the rounded 2x2 means + 128:
 *       matrix 6 limited (= 0)   66 129  25, 16    -38  -74 112    112  -94 -18
 *       matrix 1 limited         47 157  16, 16    -26  -86 112    112 -102 -10
 *       matrix 6 full            77 150  29,  0    -43  -84 127    127 -107 -20
 *       matrix 1 full            54 183  19,  0    -29  -98 127    127 -116 -11
 *   (Kr / Kb scaled by 219/255 and 224/255, or by 1, times 256, rounded; one coefficient per row moved by 1 so that luma sums to 220 or
 *   256 and chroma to 0; in full-range chroma the 0.5 weight is 127, since 128 would give 256 for a saturated blue or red, and the
 *   nearer neighbour takes the 1.  Grey stays neutral and no result leaves 16..235 / 16..240, or 0..255 -- there is no clamp;
 *   tests/color_model.py restates it and proves the ranges over all 2^24 inputs).  With a window: scale each channel, round to 8 bits,
 *   then this matrix.
 *   frame rate num/den, 0 < num <= 2^30, 0 < den < 2^31: timing_info with num_units_in_tick = den, time_scale = 2 num,
 *   fixed_frame_rate_flag = 1; 0/0 clears it.
 * The SPS is repeated at every key frame and must not change inside a stream: the per-frame calls are accepted after H264E_init and
 * before the first H264E_encode* only (H264E_STATUS_BAD_PARAMETER afterwards, as H264E_set_denoise), the clip calls only while the
 * clip stands at frame 0 (after open or rewind; a rewind keeps the setting; 0 = done, -1 = refused).  Frames already uploaded were
 * converted with the setting that held at their upload: change the colour BEFORE uploading.  A refusal changes nothing and names the
 * offending value in H264E_last_error.  With rate control the parameter sets count in the frame's bytes as in the reference, so a
 * signalled stream may differ from an unsignalled one behind the first key frame. */
#define H264E_MATRIX_UNSPECIFIED 0
#define H264E_MATRIX_BT709       1
#define H264E_MATRIX_BT601       6
int  H264E_set_color(H264E_persist_t *enc, int matrix, int full_range);
int  H264E_set_frame_rate(H264E_persist_t *enc, int num, int den);
/* Select the HIP device used by subsequent H264E_init calls of this process (default 0 / $H264E_DEVICE). */
void H264E_set_device(int device);
int  H264E_device_count(void);
/* Last device-side error text (empty when none). */
const char *H264E_last_error(void);

/* Whole-clip streaming encode: consecutive frames run as a temporal wavefront inside one
 * kernel launch, finished frames are validated and NAL-assembled by the host while the launch runs (DESIGN.md
 * sections 4-5).  Bit-identical to feeding the frames one by one to H264E_encode.  With rate control (kbps) a frame's QP depends on the size
 * of the frame before it: the frames behind the first one of a launch run on a speculated QP and are stopped when the exact
 * controller disagrees. */
typedef struct
{
    int width, height, gop, qp, speed;      /* qp: constant QP, clamped to 10..51 -- except 0, which runs the frame-level controller over
                                               QP 10..51 without a byte target, as qp_min = qp_max = 0 does in H264E_encode (h264-lab.h:6707-6715) */
    int vbv_size_bytes;                     /* SPS level only */
    int device;
    int max_chains;                         /* cap of the slot ring (frame f lives in slot f % K; K - 1 = most frames one launch can hold); 0 = sized by the
                                               memory budget: 622 slots at 1080p, 162 at 4K, 40 at 8K, at most 1024 */
    int first_idr_pic_id_state;             /* enc->next_idr_pic_id before the first frame (0 for a fresh stream) */
    int32_t mv_clusters_in[2];              /* enc->mv_clusters before the first frame (0,0 for a fresh stream) */
    int slices;                             /* row-band slices per frame: 0 / 1 = one; N = the reference's H264E_MAX_THREADS build with --threads N;
                                               N above the macroblock rows R = R slices (the reference codes rows twice there) */
    int kbps;                               /* 0 = constant QP `qp`; > 0 = frame-level rate control as encode_app --kbps (a few frames per launch then, on a speculated QP that is validated against the exact controller) */
    int resident_frames;                    /* input frames kept in HBM (a ring, frame f in slot f % resident_frames); 0 = the whole clip */
    int keep_records;                       /* keep what every frame consumed, for H264E_clip_revalidate (GOP shards of one stream) */
} H264E_clip_param_t;

typedef struct
{
    double upload_ms, encode_ms, readback_ms, assemble_ms;      /* host wall clock of the phases */
    double mb_kernel_ms, splice_kernel_ms;                      /* HIP-event time inside the kernel launches (when profiled); the splice runs inside the macroblock kernel: second value ~0 */
    int kernel_launches;
    int chains, rounds, reencoded_gops;                         /* frames in flight per launch, launches, relaunches after a mis-speculated mv_clusters state */
    int32_t mv_clusters_out[2];
    int next_idr_pic_id_state;
    int first_frame, frames;                                    /* the frames this call encoded: [first_frame, first_frame + frames) */
    int spin_relaunches;                                        /* launches repeated because a bounded in-kernel wait expired (workgroups starved of wave slots: nothing wrong was returned) */
    /* event bookkeeping of this call (round-3 VERDICT item 4): what the kernel worked on against what was delivered */
    int relaunches_timed;                                       /* launches that followed a stopped one (mis-speculated mv_clusters state, rate-control miss) and delivered a frame */
    long long processed_mbs;                                    /* macroblocks reconstructed by the kernel, including those of frames that were thrown away */
    long long delivered_mbs;                                    /* macroblocks of the frames that were accepted = frames x macroblocks per frame */
    double first_frame_ms_after_relaunch;                       /* SUM over relaunches_timed launches of: submit -> first accepted frame (host wall clock) */
    int kept_key_frames, kept_key_rows;                         /* key frames that started below row 0 on rows a stopped launch had completed, and those rows (H264E_KEEP_KEY_ROWS) */
} H264E_clip_stats_t;

/* Device-resident input: a frame that already lies in the memory of the encoder's GPU (left there by a decoder, a renderer, a
 * capture path, a torch model) is taken from there by one small kernel, without a trip through host memory.
 *   format I420: plane[0..2] = Y, U, V, each with its own stride (separately allocated, padded planes are fine);
 *          NV12: plane[0] = Y, plane[1] = interleaved U,V pairs;
 *          RGB:  plane[0] = interleaved 8-bit R,G,B of pixel_bytes 3 or 4 (a fourth byte is ignored), converted to BT.601 limited
 *                range in integers (another matrix or full range: H264E_set_color): Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16 per pixel; chroma from the rounded 2x2 mean of each
 *                channel, m = (a + b + c + d + 2) >> 2: U = ((-38 Rm - 74 Gm + 112 Bm + 128) >> 8) + 128,
 *                V = ((112 Rm - 94 Gm - 18 Bm + 128) >> 8) + 128 (arithmetic shifts).
 *          RGBP: plane[0..2] = the R, G and B planes, 8 bits per sample, each with its own pointer and stride (a CHW tensor, three
 *                allocations, padded or odd strides and addresses); pixel_bytes is ignored.  The same arithmetic: byte for byte what
 *                RGB gives for the same image.
 *          RGBP | H264E_DEV_SAMPLE_F16 / _BF16 / _F32 (bits 4-5 of format; on any other layout they are refused): the same three
 *                planes of float16, bfloat16 or float32 samples in [0, 1], as vision models and renderers hold them.  Every sample x
 *                is widened to float32 (exact) and quantised, q = clamp(rint(x * 255), 0, 255): ONE float32 multiply, round to nearest
 *                even; NaN, negative values and -0.0 give 0, values above 1 give 255 -- torch's nan_to_num((x.float() * 255).round()
 *                .clamp(0, 255), nan=0).to(uint8).  From q on the frame IS the 8-bit RGBP frame: the stream and the input slot are
 *                exactly those of the quantised planes (tests/float_model.py restates it).  Strides stay in bytes; plane pointers and
 *                strides must be multiples of the sample's size.
 *          I420 | H264E_DEV_DEPTH(d), NV12 | H264E_DEV_DEPTH(d), d = 9 .. 16 (bits 8-11 of format; on RGB and RGBP, together with a float
 *                sample type, and on the way out they are refused): what hardware decoders and 10-bit software decoders leave.  Samples are
 *                unsigned 16-bit little-endian words with d significant bits, LSB aligned (yuv420p10le: d = 10); a P010 / P012 / P016
 *                surface is MSB aligned, which is simply d = 16 (H264E_DEV_FORMAT_P016, alias _P010).  Every word v is quantised as
 *                it is loaded, q = min(255, (v + (1 << (d - 9))) >> (d - 8)): round half up, one clamp; words above 2^d - 1 (garbage
 *                in the unused high bits) saturate to 255; 10-bit limited range maps 64 -> 16 and 940 -> 235.  From q on the frame IS
 *                the 8-bit frame: the stream and the input slot are exactly those of the quantised planes (tests/hbd_model.py restates
 *                it).  Strides stay in bytes; plane pointers and strides must be multiples of 2.
 *          I420 | H264E_DEV_CHROMA_444 (bit 12: H264E_DEV_FORMAT_I444; the I420 layout only, with or without a depth): U and V have the
 *                luma's size.  Luma is copied (or quantised); U(i,j) = (a + b + c + d + 2) >> 2 over the 2x2 block of the 8-bit
 *                (quantised first) chroma samples, the rounded mean of the RGB path; V likewise.  The slot is that of an I420 frame
 *                with those chroma planes.
 *          I420 | H264E_DEV_CHROMA_422, NV12 | H264E_DEV_CHROMA_422 (bit 14 -- bit 13 stays unassigned and refused: H264E_DEV_FORMAT_I422 = ffmpeg's yuv422p, _NV16; with or
 *                without a depth; together with 4:4:4, on RGB and RGBP, with a float sample type and on the way out they are refused):
 *                what capture cards, pro-video decoders and MJPEG cameras leave.  U and V have the luma's HEIGHT and half its width:
 *                plane[1], plane[2] = width/2 x height samples each, or for NV16 plane[1] = height rows of width/2 U,V pairs.  Luma
 *                is copied (or quantised); U(i,j) = (a + b + 1) >> 1 with a = U422(i, 2j) and b = U422(i, 2j + 1), the 8-bit
 *                (quantised first, the order 4:4:4 uses) samples of one column in a pair of rows; V likewise.  The slot is that of an
 *                I420 frame with those chroma planes (tests/c422_model.py restates it).
 *          I420 | H264E_DEV_CHROMA_422 | H264E_DEV_PACK_YUYV or _UYVY (bits 2-3: H264E_DEV_FORMAT_YUYV = YUY2, _UYVY; valid only with
 *                bit 14 on the I420 layout; both bits, a pack bit without bit 14 or on NV12 are refused): ONE plane, only plane[0] and
 *                stride[0] are read.  A row is 2 * width samples in groups of four, Y0 U Y1 V (YUYV) or U Y0 V Y1 (UYVY); the samples
 *                are de-interleaved as they are loaded and the arithmetic is that of I422.  With H264E_DEV_DEPTH(d) all four 4:2:2
 *                layouts hold 16-bit little-endian words, quantised as above: H264E_DEV_FORMAT_P210 / _P216 = NV16 | DEPTH(16) and
 *                _Y210 / _Y216 = YUYV | DEPTH(16) are MSB aligned like P010; yuv422p10le is I422 | DEPTH(10).
 * stride: bytes from row to row, at least the row's bytes; no alignment is asked of pointers or strides of 8-bit samples.  producer_stream: the
 * hipStream_t on which the work that writes the frame was queued -- the encoder waits for everything queued there so far -- or NULL
 * when the caller has synchronised.  Every call that takes such frames returns when they have been read: the memory may be reused
 * at once.  The pointers must be device memory of the encoder's GPU; anything else is refused (H264E_last_error says why). */
#define H264E_DEV_FORMAT_I420 0
#define H264E_DEV_FORMAT_NV12 1
#define H264E_DEV_FORMAT_RGB  2
#define H264E_DEV_FORMAT_RGBP 3
#define H264E_DEV_SAMPLE_U8    0x00         /* the sample type, OR-ed into format: RGBP only */
#define H264E_DEV_SAMPLE_F16   0x10
#define H264E_DEV_SAMPLE_BF16  0x20
#define H264E_DEV_SAMPLE_F32   0x30
#define H264E_DEV_DEPTH(d) (((d) - 8) << 8)  /* 16-bit samples with d = 9 .. 16 significant bits, OR-ed into format: I420 and NV12, input only */
#define H264E_DEV_CHROMA_444   0x1000       /* U and V of the luma's size, OR-ed into format: I420, input only */
#define H264E_DEV_FORMAT_I444  (H264E_DEV_FORMAT_I420 | H264E_DEV_CHROMA_444)
#define H264E_DEV_FORMAT_P016  (H264E_DEV_FORMAT_NV12 | H264E_DEV_DEPTH(16))
#define H264E_DEV_FORMAT_P010  H264E_DEV_FORMAT_P016       /* MSB aligned: the unused low bits take part in the rounding, as they should */
#define H264E_DEV_CHROMA_422   0x4000       /* U and V of the luma's height and half its width, OR-ed into format: I420 and NV12, input only */
#define H264E_DEV_PACK_YUYV    0x4          /* one plane, Y0 U Y1 V: only with H264E_DEV_CHROMA_422 on I420, input only */
#define H264E_DEV_PACK_UYVY    0x8          /* one plane, U Y0 V Y1: likewise */
#define H264E_DEV_FORMAT_I422  (H264E_DEV_FORMAT_I420 | H264E_DEV_CHROMA_422)
#define H264E_DEV_FORMAT_NV16  (H264E_DEV_FORMAT_NV12 | H264E_DEV_CHROMA_422)
#define H264E_DEV_FORMAT_YUYV  (H264E_DEV_FORMAT_I422 | H264E_DEV_PACK_YUYV)
#define H264E_DEV_FORMAT_UYVY  (H264E_DEV_FORMAT_I422 | H264E_DEV_PACK_UYVY)
#define H264E_DEV_FORMAT_P216  (H264E_DEV_FORMAT_NV16 | H264E_DEV_DEPTH(16))
#define H264E_DEV_FORMAT_P210  H264E_DEV_FORMAT_P216       /* MSB aligned, like P010 */
#define H264E_DEV_FORMAT_Y216  (H264E_DEV_FORMAT_YUYV | H264E_DEV_DEPTH(16))
#define H264E_DEV_FORMAT_Y210  H264E_DEV_FORMAT_Y216
typedef struct
{
    int format;                             /* H264E_DEV_FORMAT_*, for RGBP | H264E_DEV_SAMPLE_*, for I420 / NV12 | H264E_DEV_DEPTH(d), for I420 | H264E_DEV_CHROMA_444, for I420 / NV12 | H264E_DEV_CHROMA_422 (| H264E_DEV_PACK_*) */
    int pixel_bytes;                        /* RGB: 3 or 4; ignored otherwise (RGBP included) */
    const void *plane[3];
    int stride[3];
    void *producer_stream;
} H264E_dev_frame_t;
/* H264E_encode with the frame taken from the device: rate control, slices, denoiser, nalu_callback and frame types as there.  The
 * encoder must have been created with const_input_flag = 1 (the reconstruction is not written back to the device):
 * H264E_STATUS_BAD_PARAMETER otherwise.  A frame that is refused (H264E_STATUS_BAD_ARGUMENT) leaves the stream where it was. */
int  H264E_encode_device(H264E_persist_t *enc, H264E_scratch_t *scratch, const H264E_run_param_t *run_param,
                         const H264E_dev_frame_t *frame, unsigned char **coded_data, int *sizeof_coded_data);
/* Device-resident input of another size: a window of the source frame is reduced to the encoder's picture on the way into the encoder,
 * by one small kernel (a 4K render streamed at 1080p, the rungs of a ladder from one source, a region of a larger surface).  The frame
 * is described as above, its planes having the SOURCE's size; the window is crop_width x crop_height luma samples at (crop_x, crop_y),
 * crop_width = 0 meaning the whole source.  The filter is an exact area (box) filter per plane -- the reference has no scaler, this
 * integer definition is the definition (tests/scale_model.py restates it): with the plane window Sw x Sh, the destination Dw x Dh,
 *     wx(i,k)  = max(0, min((i+1) Sw, (k+1) Dw) - max(i Sw, k Dw))        (wy(j,l) likewise with Sh, Dh),
 *     out(i,j) = floor((sum_l sum_k wy(j,l) wx(i,k) src(crop_x + k, crop_y + l) + ((Sw Sh) >> 1)) / (Sw Sh)),
 * so equal sizes copy (a pure crop) and 2:1 is (a + b + c + d + 2) >> 2.  Chroma planes: the same with every value halved; the
 * half-sample shift of the chroma siting is ignored.  NV12 chroma is de-interleaved.  RGBP: each of R, G, B is reduced by that filter
 * from the window to Dw x Dh (rounded to 8 bits, all three at luma geometry), and the conversion above is applied to that RGB picture --
 * the order a caller scaling and converting in two steps would use; chroma is the matrix of the rounded 2x2 mean of already rounded
 * samples (tests/rgbp_model.py restates it).  A pure crop equals the plain ingest of the cropped region, a constant colour stays the
 * same at every ratio.  Float RGBP: the window filters the QUANTISED samples, so the slot is that of the quantised 8-bit planes.
 * 16-bit samples: likewise, the filter runs on the quantised samples of every plane.  4:4:4 (H264E_DEV_CHROMA_444): a chroma plane's
 * window is the luma's, Sw x Sh at (crop_x, crop_y), reduced directly to Dw/2 x Dh/2 by the same formula -- at Sw = Dw exactly the 2x2
 * rounded mean of the plain ingest, so a pure crop equals the ingest of the cropped region; no plane is reduced by more than 16:1, so a
 * 4:4:4 window may be at most 8 times the picture in an axis.  4:2:2 (H264E_DEV_CHROMA_422, planes, U,V pairs or packed): a chroma
 * plane's window is Sw/2 x Sh at (crop_x/2, crop_y), reduced directly to Dw/2 x Dh/2 by the same formula -- at Sw = Dw, Sh = Dh exactly
 * (a + b + 1) >> 1 of the plain ingest, so a pure crop equals the ingest of the cropped region; a 4:2:2 window may be at most 16 times the
 * picture in width and 8 times in height.
 * Refused (H264E_last_error names the value): interleaved RGB
 * with a window, odd or negative crop values, a window that leaves the source, is smaller than the picture in an axis (no upscaling),
 * larger than 4096 samples or more than 16 times the picture in an axis, a stride below the source row's bytes, and planes that are
 * not device memory of the encoder's GPU from the window's first byte to its last. */
typedef struct { int src_width, src_height, crop_x, crop_y, crop_width, crop_height; } H264E_dev_window_t;   /* crop_width = 0: the whole source */
int  H264E_encode_device_scaled(H264E_persist_t *enc, H264E_scratch_t *scratch, const H264E_run_param_t *run_param,
                                const H264E_dev_frame_t *frame, const H264E_dev_window_t *win, unsigned char **coded_data, int *sizeof_coded_data);
/* Device-resident output, the way back: the reconstruction of an encoded frame -- the picture a decoder shows for it, which lies in the
 * GPU's memory as the next frame's reference -- is cropped to width x height and written into device memory the caller owns by one small
 * kernel, without a trip through host memory (quality metrics against the source tensor, codec-in-the-loop training, a preview, choosing
 * the rung of a ladder).  dst describes the destination exactly as H264E_dev_frame_t describes a source: format, pixel_bytes, a pointer
 * and a row stride (bytes, at least the row's bytes; no alignment is asked of either) per plane; the plane pointers are written through.
 * Only the bytes of the rows are written: padding between rows and everything around the planes keeps what it held.
 *   I420: plane[0..2] = Y, U, V;   NV12: plane[0] = Y, plane[1] = interleaved U,V pairs: copies of the coded samples.
 *   RGB:  plane[0] = interleaved R,G,B of pixel_bytes 3 or 4 (the fourth byte is written as 255);   RGBP: plane[0..2] = R, G, B planes.
 *   RGBP | H264E_DEV_SAMPLE_F16 / _BF16 / _F32: the 8-bit R, G, B values v of RGBP written as float32 v / 255 (ONE correctly rounded
 *         division, not a multiplication by 1/255), for float16 and bfloat16 that float32 value rounded to nearest even: torch's
 *         (u8.float() / 255).to(dtype) with IEEE division (torch on the CPU), bit for bit.  Pointers and strides: multiples of the sample's size.
 * The conversion for RGB and RGBP -- the reference has none, this integer definition is the definition (tests/egress_model.py restates it):
 * every chroma sample serves the 2x2 luma block it belongs to (sample replication, the counterpart of the ingest's 2x2 mean; no
 * interpolation), and per pixel, with C = Y - yo, D = U - 128, E = V - 128 and arithmetic shifts,
 *     R = clamp((ky C + rv E + 128) >> 8),   G = clamp((ky C + gu D + gv E + 128) >> 8),   B = clamp((ky C + bu D + 128) >> 8),
 * clamped to 0..255 (a coded picture can hold any Y, U, V triple).  The coefficients are the inverse, in 1/256, of the matrix that
 * H264E_set_color / H264E_clip_set_color selected (nothing set: BT.601 limited):
 *                                 ky  yo   rv    gu    gv   bu
 *       matrix 6 limited (= 0)   298  16  409  -100  -208  516
 *       matrix 1 limited         298  16  459   -55  -136  541
 *       matrix 6 full            256   0  359   -88  -183  454
 *       matrix 1 full            256   0  403   -48  -120  475
 *   (rv = 2(1 - Kr), bu = 2(1 - Kb), gu = -2 Kb (1 - Kb)/Kg, gv = -2 Kr (1 - Kr)/Kg, times 255/224 for limited range; ky = 255/219 or 1;
 *   times 256, rounded.  Grey (U = V = 128) stays grey, black and white give 0 and 255.)
 * producer_stream: the hipStream_t whose queued work may still read or write the destination -- the kernel waits for everything queued
 * there so far -- or NULL when the caller has synchronised.  The calls return when the destination has been written.  Refused, with the
 * value named in H264E_last_error and the destination untouched: an unknown format, pixel_bytes other than 3 or 4 for RGB, a NULL plane,
 * a sample type on another layout than RGBP, a pointer or stride that is not a multiple of a float sample's size,
 * a stride below the row's bytes, and a plane that is not device memory of the encoder's GPU inside one allocation from the first byte
 * written to the last.  Nothing is scaled on the way out.
 * H264E_read_recon_device: the picture the last successful H264E_encode / H264E_encode_device / H264E_encode_device_scaled left -- what
 * const_input_flag = 0 writes back into host planes; it works with either value of that flag (H264E_encode_device still needs 1) and
 * leaves the stream alone.  H264E_STATUS_BAD_ARGUMENT before the first frame and for a refused destination. */
int  H264E_read_recon_device(H264E_persist_t *enc, const H264E_dev_frame_t *dst);
/* device memory and blocking copies for callers without a HIP toolchain (to_device: 1 = host to device, 0 = device to host) */
void *H264E_dev_malloc(int device, size_t bytes);
void  H264E_dev_free(void *p);
int   H264E_dev_memcpy(void *dst, const void *src, size_t bytes, int to_device);

/* sizeof of the extension structs as THIS build sees them (0: H264E_clip_param_t, 1: H264E_clip_stats_t, 2: H264E_dev_frame_t): lets a binding in another language check its mirror */
int  H264E_struct_size(int which);

typedef struct H264E_clip_tag H264E_clip_t;
/* Create a clip encoder for a stream of at most nframes frames. */
int  H264E_clip_open(H264E_clip_t **clip, const H264E_clip_param_t *par, int nframes);
/* Input: packed I420 frames [first, first + nframes) of the stream from host memory, or the synth_v1 test clip generated in HBM.
 * With a bounded input ring (resident_frames) a frame can be uploaded once frame (f - resident_frames) has been encoded. */
int  H264E_clip_upload(H264E_clip_t *clip, int first, int nframes, const uint8_t *i420);
int  H264E_clip_generate_synth(H264E_clip_t *clip, int first, int nframes, int t0, uint32_t seed);
/* the same from device memory: frames[i] is frame first + i (frame range, ring and "uploading frame f again makes f onward new" rules
 * of H264E_clip_upload).  Returns when the frames have been read; all of them are checked before the first is touched. */
int  H264E_clip_upload_device(H264E_clip_t *clip, int first, int nframes, const H264E_dev_frame_t *frames);
/* ... every frame a source of another size, all reduced through the same window (see H264E_dev_window_t); same rules */
int  H264E_clip_upload_device_scaled(H264E_clip_t *clip, int first, int nframes, const H264E_dev_frame_t *frames, const H264E_dev_window_t *win);
/* diagnostic: enable != 0 times the kernel launches of later device uploads with HIP events; kernel_ms / frames: the totals since open
 * (tools/scale_probe.py) */
int  H264E_clip_input_time(H264E_clip_t *clip, int enable, double *kernel_ms, long long *frames);
/* the same from pinned host memory on the copy engine, overlapping with a running encode; H264E_clip_upload_wait() completes it */
void *H264E_clip_host_alloc(size_t bytes);
void  H264E_clip_host_free(void *p);
int  H264E_clip_upload_async(H264E_clip_t *clip, int first, int nframes, const uint8_t *pinned_i420);
int  H264E_clip_upload_wait(H264E_clip_t *clip);
int  H264E_clip_upload_poll(H264E_clip_t *clip);              /* 1 = landed (frames count as uploaded), 0 = still copying */
/* where the stream stands: next frame to encode, frames uploaded so far */
void H264E_clip_position(const H264E_clip_t *clip, int *next_frame, int *uploaded_frames);
/* called (from the calling thread) while H264E_clip_encode waits for the GPU: a file-fed application issues and completes its
 * uploads from here, so that frames keep arriving while earlier ones are being encoded */
void H264E_clip_set_idle_hook(H264E_clip_t *clip, void (*hook)(void *token), void *token);
/* Encode the frames uploaded so far and not yet encoded -- or as many of them as fit `out` -- and append their Annex-B bytes;
 * stats->first_frame / frames say which; frame_bytes[i] is the size of frame first_frame + i.  The stream continues with the
 * next call.  profile != 0 adds per-kernel HIP-event timing. */
int  H264E_clip_encode(H264E_clip_t *clip, uint8_t *out, size_t cap, size_t *out_bytes, int *frame_bytes /* [frames of this call] or NULL */,
                       int profile, H264E_clip_stats_t *stats);
/* Several independent clips of the same picture size on ONE device at the same time: each clip is encoded exactly like
 * H264E_clip_encode does (same bytes), by a host thread of its own, and the device layer merges the clips' kernel launches so that one
 * stream's pipeline drains (after a mis-speculated mv_clusters state) are filled by the other streams' frames.  out[i] / cap[i] /
 * out_bytes[i] / frame_bytes[i] / stats[i] belong to clips[i] (frame_bytes and stats may be NULL).  At most 8 clips; all on the same
 * device; large pictures allow fewer (the group refuses a clip it cannot hold safely). */
int  H264E_clip_encode_multi(H264E_clip_t **clips, int nclips, uint8_t **out, const size_t *cap, size_t *out_bytes, int **frame_bytes, H264E_clip_stats_t *stats);
/* back to frame 0 with the stream state of H264E_clip_open (the uploaded frames stay): encode the clip again */
void H264E_clip_rewind(H264E_clip_t *clip);
/* resident input frames back to host memory (whole-clip residency only; bench.py's PCIe-inclusive measurement) */
int  H264E_clip_download(H264E_clip_t *clip, int first, int nframes, uint8_t *i420);
/* reconstruction (coded size, packed I420) of one of the last frames encoded (its picture slot must not have been reused: the last
 * ring - 1 frames in constant-QP mode; with rate control only the frames accepted since the last launch began -- the launches' hedge
 * leaves are encoded over the pictures of older frames).  -1 outside that window. */
int  H264E_clip_read_recon(H264E_clip_t *clip, int frame, uint8_t *dst);
/* the same picture, cropped to the clip's width x height, into device memory in the layout dst describes (see H264E_read_recon_device
 * for formats, conversion, ordering and what is refused).  The same window of frames as H264E_clip_read_recon: the last ring - 1 frames,
 * with rate control only those accepted since the last launch began.  0 = done, -1 = refused: outside that window (a frame not yet
 * encoded, one whose picture slot has been reused) H264E_last_error names the frame and the frames that can be read. */
int  H264E_clip_read_recon_device(H264E_clip_t *clip, int frame, const H264E_dev_frame_t *dst);
/* diagnostic: enable != 0 times the kernel launches of later H264E_clip_read_recon_device calls with HIP events; kernel_ms / frames: the
 * totals since open (tools/egress_probe.py) */
int  H264E_clip_output_time(H264E_clip_t *clip, int enable, double *kernel_ms, long long *frames);
/* per encoded frame [3] sums of squared differences input vs reconstruction (Y, U, V), computed on the device: encode_app --psnr */
void H264E_clip_set_ssd_output(H264E_clip_t *clip, uint64_t *ssd);
/* ... and [3] SSIM values (Y, U, V), indexed like the SSD output: the 8x8-window, step-4 SSIM of x264 and of ffmpeg's `ssim` filter, per
 * plane of the PICTURE (cropped size), the mean over the plane's windows, computed on the device with a fixed order of the sum (two runs
 * give the same doubles); ffmpeg's "All" is (4 Y + U + V) / 6.  Both metrics compare the RAW input with the reconstruction, also with the
 * denoiser on.  NULL switches it off.  -1, with the size named in H264E_last_error, for a picture below 16 x 16 (a chroma plane without
 * a window). */
int  H264E_clip_set_ssim_output(H264E_clip_t *clip, double *ssim);
/* diagnostic: enable != 0 times the SSD and SSIM launches of later calls with HIP events; the totals since open and the frames they
 * covered (tools/quality_probe.py) */
int  H264E_clip_quality_time(H264E_clip_t *clip, int enable, double *ssd_ms, double *ssim_ms, long long *frames);
/* frame at a time: after a successful H264E_encode / H264E_encode_device / H264E_encode_device_scaled, that call's input as it lies in the
 * encoder's input slot (host or device input, either const_input_flag) against the reconstruction it left: the sums of squared differences
 * into ssd[3] and the SSIM into ssim[3] (Y, U, V); either may be NULL.  After a transparent VBV-overflow frame the reconstruction is the
 * unchanged picture, which is what a decoder shows.  H264E_STATUS_BAD_ARGUMENT, with H264E_last_error saying why: before the first frame,
 * both pointers NULL, SSIM for a picture below 16 x 16 (the SSD works at every size). */
int  H264E_read_quality(H264E_persist_t *enc, uint64_t ssd[3], double ssim[3]);
/* the same SSIM of ONE pair of 8-bit planes of width x height samples in memory of `device` (-1: the default device), rows a_stride /
 * b_stride bytes apart, any addresses, through the same kernel; the caller has synchronised whatever wrote them.  -1, with the value
 * named in H264E_last_error: NULL, width or height below 8, a stride below width, memory that is not one allocation of that device. */
int  H264E_ssim_planes(int device, const void *a, int a_stride, const void *b, int b_stride, int width, int height, double *ssim);
/* The temporal denoiser for the clip encoder (see H264E_set_denoise; the clip's speed < 2 selects it for every frame): only while the
 * clip stands at frame 0 (after open or rewind); the denoised pictures are a pure function of the inputs, kept across a rewind and
 * made again from the first frame that is uploaded again.  The sums of squared differences compare the RAW input with the
 * reconstruction, as the reference's --psnr does.  Refused with keep_records (GOP shards).  0 = done, -1 = refused. */
int  H264E_clip_set_denoise(H264E_clip_t *clip, int on);
/* HDR10 device input: tone mapping.  A setting of the encoder, not a format bit, off by default; with it off no byte, record, launch or
 * allocation differs from an encoder that never heard of it.  While it is on, the 16-bit device frames of H264E_encode_device[_scaled]
 * and H264E_clip_upload_device[_scaled] are taken as HDR10 -- PQ transfer (SMPTE ST 2084), BT.2020 primaries, BT.2020 non-constant
 * luminance Y'CbCr in limited range -- and tone-mapped by one gfx950 kernel to an 8-bit SDR R'G'B' picture with BT.709 primaries and
 * transfer, which is converted to the 4:2:0 input exactly as an RGB device frame is, with the matrix H264E_set_color selected (the
 * pairing that players expect is H264E_MATRIX_BT709: the stream then says what it holds).  Host-frame calls are unchanged.
 *   Accepted while on: I420 | H264E_DEV_DEPTH(d) and NV12 | H264E_DEV_DEPTH(d), d = 10 .. 16 (H264E_DEV_FORMAT_P010 / _P016 included).
 *   Every other device format -- 8-bit, RGB, RGBP, 4:2:2, 4:4:4 -- and d = 9 is refused by name; the refusal moves nothing.  4:2:2 and
 *   4:4:4 HDR surfaces and the HLG transfer are out of scope.
 * The definition (the reference has none; tests/tonemap_model.py restates it bit for bit; integers, or single float32 operations each
 * rounded on its own, never fused).  Per 2x2 luma block with its one chroma pair; chroma is REPLICATED over the block, the siting
 * shift is ignored as elsewhere:
 *   1. word to 10-bit code: c = min(1023, (v + r) >> s), s = d - 10, r = s ? 1 << (s - 1) : 0 -- a 12-bit source is reduced to 10-bit codes;
 *   2. to R'G'B' codes 0 .. 1023 in Q14, y = Y - 64, u = Cb - 512, v = Cr - 512, arithmetic shift, clamp to 0 .. 1023:
 *          R = clamp((ky y + crv v + 8192) >> 14), G = clamp((ky y - cgu u - cgv v + 8192) >> 14), B = clamp((ky y + cbu u + 8192) >> 14)
 *      ky = 19133, crv = 27584, cgu = 3078, cgv = 10688, cbu = 35194: rint(16384 x) of 1023/876, 1.4746 * 1023/896,
 *      (0.0593 * 1.8814 / 0.6780) * 1023/896, (0.2627 * 1.4746 / 0.6780) * 1023/896, 1.8814 * 1023/896;
 *   3. m = max(R, G, B) of the codes; L_ch = eotf[ch] * scale[m], one multiply per channel.  eotf[c] = float32 of
 *      10000 PQ_EOTF(c / 1023) / ref_white; scale[c] = float32 of t(min(x, p)) / x, x that value before it is rounded to float32,
 *      p = peak / ref_white, 1 where x = 0.  t: clip min(x, 1); reinhard x (1 + x / p^2) / (1 + x); hable h(x) / h(p) with
 *      h(x) = (x (A x + C B) + D E) / (x (A x + B) + D F) - E / F, A .. F = .15, .50, .10, .20, .02, .30.  t(p) = 1 for all three;
 *   4. gamut, BT.2020 to BT.709 (BT.2087): o = (m0 L_R + m1 L_G) + m2 L_B with the rows 1.6605 -0.5876 -0.0728 / -0.1246 1.1329 -0.0083 /
 *      -0.0182 -0.1006 1.1187 as float32 constants.  Colours outside BT.709 are CLIPPED by the next step, not compressed;
 *   5. BT.709 OETF, exactly rounded: code = #{k in 1 .. 255 : o >= thresh[k]}, thresh[k] = float32 of the inverse OETF at (k - 0.5) / 255
 *      (x / 4.5 below 4.5 * 0.018, ((x + 0.099) / 1.099)^(1 / 0.45) above);
 *   6. the 8-bit R'G'B' picture to Y, U, V by the integer rows of the RGB device input above.
 * Through an H264E_dev_window_t (crop values even, as for I420): the window is tone-mapped at the source's resolution into an 8-bit I420
 * surface that the encoder owns (sized on first use, reused, freed with the encoder), and the I420 window path runs from it: by
 * construction what the tone-mapped crop fed as I420 with that source size gives; the limits and refusals are I420's.
 * peak_nits: the brightest light of the source that is kept apart from white (0 = 1000); ref_white_nits: the light that becomes SDR
 * white 1.0 (0 = 203).  Refused, with the value in H264E_last_error: an unknown transfer or curve, non-finite values, a reference white
 * outside 50 .. 1000, a peak below the reference white or above 10000.  Accepted where H264E_set_color / H264E_clip_set_color are --
 * before the first frame, while the clip stands at frame 0 -- with their statuses; a rewind keeps the setting.
 * H264E_tonemap_tables: a pure host function, the tables the kernel will use for these parameters (0 = done, -1 = refused);
 * ycc = ky, crv, cgu, cgv, cbu, then 64, 512, 14. */
#define H264E_TONEMAP_OFF 0
#define H264E_TONEMAP_PQ  1                 /* ST 2084, BT.2020 non-constant luminance, limited range */
#define H264E_TONECURVE_HABLE 0
#define H264E_TONECURVE_REINHARD 1
#define H264E_TONECURVE_CLIP 2
int  H264E_set_tonemap(H264E_persist_t *enc, int transfer, int curve, double peak_nits, double ref_white_nits);
int  H264E_clip_set_tonemap(H264E_clip_t *clip, int transfer, int curve, double peak_nits, double ref_white_nits);
int  H264E_tonemap_tables(int transfer, int curve, double peak_nits, double ref_white_nits, int ycc[8], float eotf[1024], float scale[1024], float thresh[256]);
/* state[0] = tone mapping is on, state[1] = bytes of the device table buffer, state[2] = bytes of the window surface (0 = not allocated) */
int  H264E_tonemap_state(H264E_persist_t *enc, long long state[3]);
int  H264E_clip_tonemap_state(H264E_clip_t *clip, long long state[3]);
/* H264E_set_color / H264E_set_frame_rate for the clip encoder (see there) */
int  H264E_clip_set_color(H264E_clip_t *clip, int matrix, int full_range);
int  H264E_clip_set_frame_rate(H264E_clip_t *clip, int num, int den);
/* Key frames where the caller wants them (a receiver asked for one, a splice point, a chapter mark): frames[0..n) (ascending, inside
 * the clip) are coded as key frames in addition to the periodic ones.  The stream is exactly what H264E_encode writes for the same
 * pictures with frame_type = H264E_FRAME_TYPE_KEY on the listed frames and H264E_FRAME_TYPE_DEFAULT on all others (h264-lab.h:6725-6775,
 * :6611-6614): SPS / PPS in front of every key frame, frame_num and the periodic GOP counter restart there (the next periodic key
 * frame comes `gop` frames after the last key frame of either kind), idr_pic_id toggles per key frame; with gop = 1 the frame behind a
 * forced key frame is a P frame, as in the reference.  Only while the clip stands at frame 0 (after open or rewind); a rewind keeps
 * the list, n = 0 clears it.  Refused with keep_records (GOP shards assume fixed GOP blocks), for a frame outside the clip and for a
 * list that is not ascending; a refusal changes nothing.  0 = done, -1 = refused (H264E_last_error says why). */
int  H264E_clip_set_key_frames(H264E_clip_t *clip, const int *frames, int n);
/* Scene-cut detection, which fills the same schedule: threshold in 1/1024 of the picture (0 = off, H264E_SCENECUT_DEFAULT = 128).  With
 * H_f[b] = the number of luma samples of the RAW input frame f (width x height, before the denoiser) with Y >> 2 == b (b = 0..63) and
 *     D(f) = (sum over b of |H_f[b] - H_(f-1)[b]|) * 1024 / (2 * width * height)       (floor; D(0) = 0),
 * frame f > 0 becomes a key frame when D(f) > threshold, unless it is one already (periodic, or on the explicit list).  The reference has
 * no detector: this integer definition is the definition (tests/scenecut_model.py restates it).  The histograms are made on the
 * device by one small kernel per frame in front of the launch that first encodes the frame (enc_scenecut.h); uploading frame f again
 * makes f onward new, a rewind keeps them.  At 352x288 and above the test clips stay at or below 21 between consecutive frames and
 * reach 280 at a hard cut, which is where the default comes from; pictures of a few thousand samples have noisy histograms (64x48: a
 * pan reaches 160) and are no basis for claims about detection.  Same rules as H264E_clip_set_key_frames for when it may be called. */
#define H264E_SCENECUT_DEFAULT 128
int  H264E_clip_set_scenecut(H264E_clip_t *clip, int threshold);
/* what the detector saw: D(f) for frames [first, first + n) and whether f was made a key frame by it (either pointer may be NULL).
 * Only frames that an H264E_clip_encode call has reached (or analysed in front of its launch); -1 otherwise, or when the detector was never on. */
int  H264E_clip_read_scenecut(H264E_clip_t *clip, int first, int n, int *dist, uint8_t *is_cut);
/* diagnostic: HIP-event time of the detector's kernel launches since open, and the frames they analysed (tools/scenecut_probe.py) */
int  H264E_clip_scenecut_time(H264E_clip_t *clip, double *kernel_ms, long long *frames);
/* A QP per frame: qp[0..n), n = the clip's nframes (0 clears the schedule), every value in 10..51.  The stream is byte for byte what
 * H264E_encode writes when frame f is given qp_min = qp_max = qp[f] and desired_frame_bytes = 0; frame types, slices, speed,
 * denoiser, colour and forced / detected key frames stay as the clip is set up.  The PPS of a key frame carries that frame's
 * pic_init_qp (clamp(30, qp_min, qp_max) = its own QP), the P frames behind it code slice_qp_delta against it.  Launches keep their
 * length: nothing is speculated and no QP stops a launch.  While the clip stands at frame 0; kept across a rewind.  Refused -- nothing
 * changes, H264E_last_error names the value -- with kbps > 0 or qp == 0 (the reference's rate control chooses the QPs), with
 * keep_records, with another n, with a value outside 10..51, and while the lookahead controller below is on. */
int  H264E_clip_set_qp_schedule(H264E_clip_t *clip, const uint8_t *qp, int n);
/* Lookahead rate control: THIS PROJECT'S OWN controller, not the reference's (whose kbps mode, H264E_clip_param_t.kbps, is untouched
 * and makes every frame's QP a function of the frame before it).  It chooses one QP per window of `window` frames before the window
 * is launched and writes it into the per-frame schedule above: the QPs are this project's choice, the bytes for those QPs are the
 * reference's.  kbps 0 = off; window 0 = the default (32, or what the input ring and the slot ring allow); qp_min = 0 / qp_max = 0
 * select 10 / 50.  While the clip stands at frame 0; settings and cost records are kept across a rewind, the controller's state is
 * reset, so the same stream results.  Refused with an explicit schedule, kbps > 0, qp == 0, keep_records, pictures below 16x16, and
 * a window above a bounded input ring's resident_frames or above the slot ring minus one.
 *   Cost pass (enc_lookahead.h, one kernel launch per frame in front of the launch that plans its window; tests/lookahead_model.py):
 * L_f = 2x2 rounded means of the RAW luma; 8x8 blocks of L_f wholly inside it; m = (sum + 32) >> 6; intra(b) = sum |L_f - m|;
 * inter(b) = sum |L_f - L_{f-1}| co-located (frame 0: intra(b)); I(f) = sum intra, P(f) = sum min(intra, inter),
 * N(f) = #{intra < inter}.  Uploading frame f again makes the records from f onward new.
 *   Controller: dfb = kbps*1000/8/30; windows [jW, (j+1)W) over frame numbers, W_j frames long; T = 8*dfb*W;
 * T_j = 8*dfb*W_j + clamp(sum over finished windows of (8*dfb*W_i - actual bits), -T/2, +T/2).  Predicted bits of frame f at QP q:
 * H(f) + min((k[t]*C(f)*Lq[t][min(q,50) - 10]) >> 24, 2^50), t = 1 and C = I for key frames, t = 0 and C = P otherwise, Lq the
 * reference's bits-per-macroblock table, H(f) = 40 bits per slice (start code, NAL header) + for key frames the parameter sets at
 * their size for pic_init_qp 26.  QP_j = the smallest q in [lo_j, hi_j] whose predicted window sum is <= T_j, else hi_j, where
 * [lo_0, hi_0] = [qp_min, qp_max] and, for j > 0, [lo_j, hi_j] = [max(qp_min, QP_{j-1} - 6), min(qp_max, QP_{j-1} + 6)]: a window's QP
 * stays within 6 (one doubling of the quantiser step) of the window before it, because k was measured at that window's QP and the
 * table does not carry it far.  When
 * window j has been accepted, for each frame type in it k[t] = ((actual bits - H of those frames, at least 0) << 24) /
 * sum C(f)*Lq[t][q_f - 10], clamped to [k_old/4, min(4*k_old, 2^40)] and to at least 1; left alone when the divisor is 0.  A launch never
 * crosses a window boundary, and a window whose frames are not all uploaded is not started: H264E_clip_encode returns with what it
 * encoded (zero frames is not an error) -- except the clip's last window once all frames are uploaded.  Zero-motion inter cost
 * overestimates pans; the calibration absorbs a steady bias, H264E_clip_set_lookahead_search below removes the cause.  VBV compliance
 * is not claimed. */
int  H264E_clip_set_lookahead(H264E_clip_t *clip, int kbps, int window, int qp_min, int qp_max);
/* I(f), P(f), N(f) and the QP of frames first .. first + n - 1; each pointer may be NULL.  Costs: only frames already analysed; QPs:
 * only frames of an explicit schedule or of windows already planned in this pass; -1 otherwise. */
int  H264E_clip_read_lookahead(H264E_clip_t *clip, int first, int n, uint64_t *intra, uint64_t *inter, int *intra_blocks, uint8_t *qp);
/* Motion search in the cost pass: range 0 = off (the pass above, the default), 1..8 = every block's inter cost is the smallest SAD over
 * the displacements of up to +-range half-resolution samples (enc_lookahead_search.h, tests/lookahead_motion_model.py).  With
 * A = [0, 8*nbx) x [0, 8*nby), nbx = (width/2) >> 3, nby = (height/2) >> 3: candidates d = (dx, dy), |dx|, |dy| <= range, whose 8x8
 * block at (8bx + dx, 8by + dy) lies wholly inside A (left out otherwise, not clamped); sad(b, d) = sum |L_f(x, y) - L_{f-1}(x + dx,
 * y + dy)|; inter(b) = the smallest sad, mv(b) = the candidate that reaches it and is first by (|dx| + |dy|, dy, dx) -- no vector
 * penalty; frame 0 of the clip: inter = intra, mv = (0, 0).  I, P, N are formed as above from this inter(b), so
 * H264E_clip_read_lookahead returns the searched P and N, and the controller is the one above with C(f) = the searched P(f) and the
 * initial k[0] = 53818 instead of 15086 (measured the same way).  The setting takes effect whenever the controller runs
 * its cost pass.  While the clip stands at frame 0; kept across a rewind.  Refused -- nothing changes, H264E_last_error names the
 * value -- with a range outside 0..8, with keep_records, and with another range than the current one once a frame of the clip has been
 * analysed (the stored records belong to the old range, and a bounded input ring cannot make them again). */
int  H264E_clip_set_lookahead_search(H264E_clip_t *clip, int range);
/* The motion field of an analysed frame: nbx*nby cells {int8 dx, int8 dy, uint16 cost = inter(b)}, row by row, into dst; *nbx, *nby
 * (optional) receive the field's size for every clip, also when the call is refused (a call with dst NULL asks for the size alone
 * and returns -1).  The fields live in a ring of max(resident_frames, 2) entries on the device: -1, with the readable
 * frames named in H264E_last_error, when the frame has not been analysed, when its entry has been taken by a later frame, and when the
 * search is off.  Uploading frame f again makes the fields from f onward new. */
int  H264E_clip_read_lookahead_motion(H264E_clip_t *clip, int frame, void *dst, int *nbx, int *nby);
/* diagnostic: HIP-event time of the cost pass' kernel launches since open, and the frames they analysed (tools/lookahead_probe.py) */
int  H264E_clip_lookahead_time(H264E_clip_t *clip, double *kernel_ms, long long *frames);
/* Cost tree over the motion field: per-frame QP offsets inside a window, from cost propagated backwards through the fields of the
 * searched cost pass -- x264's macroblock tree summed to frame level (enc_lookahead_tree.h, tests/lookahead_tree_model.py).  strength 0
 * = off (the default: nothing is launched or allocated, every record and byte is as without the call), 1..16 = quarter QP steps per
 * doubling of a frame's importance; ahead 0..255 = frames behind a window that its tree starts from, below 0 = min(W, resident_frames -
 * W), at least 0.  With key(f) the key-frame schedule (periodic, forced and scene-cut), window j = [a, b) and horizon e = min(b + ahead,
 * nframes): in_f(t) = 0 for every block t of every frame in [a, e); for f = e - 1 down to a + 1, unless key(f), every block s = (sx, sy)
 * of frame f: i = intra_f(s), c = min(i, inter_f(s)), g = min(in_f(s), 2^40); amt = g when i == 0, else ((i + g)*(i - c))/i floored;
 * x = 8sx + dx, y = 8sy + dy with (dx, dy) = mv_f(s); tx = x >> 3, ox = x & 7, ty = y >> 3, oy = y & 7; the four targets (tx + u,
 * ty + v), u, v in {0, 1}, have the weights wx = u ? ox : 8 - ox times wy = v ? oy : 8 - oy, a target of weight 0 is left out, and each
 * gets in_{f-1}(target) += (amt*wx*wy) >> 6.  Then S(f) = min(sum_t min(in_f(t), 2^40), 2^48); lg(f) = 0 when I(f) == 0, else with
 * r = ((I(f) + S(f)) << 8)/I(f) and e2 = floor(log2 r) - 8: lg = 256*e2 + ((r >> e2) - 256), a piecewise-linear log2 in 1/256 units;
 * delta(f) = -min(6, (strength*lg(f) + 512) >> 10): a key frame passes nothing back and receives from its followers, and the cap is the
 * controller's one doubling of the quantiser step.
 *   Controller with the tree: window j has a BASE QP Q_j and frame f of it q_f = clamp(Q_j + delta(f), qp_min, qp_max); Q_j = the smallest
 * value in [lo_j, hi_j] whose predicted window sum, each frame at its own q_f, is <= T_j, else hi_j; [lo_j, hi_j] lies around Q_{j-1}, the
 * base of the window before, not around a frame's QP; a window is planned only when the frames up to its horizon are uploaded; only
 * delta(f) of [a, b) is used, and a frame's S, delta and block map are those of the run that planned its own window.  k, H(f), the
 * carry and the calibration stay as above.  While the clip stands at frame 0; the setting is kept across a rewind, sums and offsets
 * belong to a window's plan and are made again with it.  Refused -- nothing changes, H264E_last_error names the value -- with strength
 * outside 0..16 or ahead above 255, with the controller off, with search range 0, with keep_records, and when W + ahead exceeds a
 * bounded input ring's resident_frames; while it is on, H264E_clip_set_lookahead(kbps 0) and H264E_clip_set_lookahead_search(0) are. */
int  H264E_clip_set_lookahead_tree(H264E_clip_t *clip, int strength, int ahead);
/* What the blocks of a frame received, in_f: nbx*nby uint64, row by row, into dst.  Size-only call and *nbx, *nby as for
 * H264E_clip_read_lookahead_motion.  The maps live in a ring beside the field ring: -1, with the readable frames named in
 * H264E_last_error, when the frame's window has not been planned in this pass, when its entry has been taken by a later run, and when
 * the tree is off. */
int  H264E_clip_read_lookahead_tree(H264E_clip_t *clip, int frame, void *dst, int *nbx, int *nby);
/* S(f), delta(f) and the base QP of the window of frames first .. first + n - 1; each pointer may be NULL.  -1 when the window of one
 * of them has not been planned in this pass, or the tree is off. */
int  H264E_clip_read_lookahead_tree_sums(H264E_clip_t *clip, int first, int n, uint64_t *sum, int8_t *delta, uint8_t *base_qp);
/* diagnostic: HIP-event time of the tree's kernel launches since open, and the frame steps they made (tools/lookahead_probe.py) */
int  H264E_clip_lookahead_tree_time(H264E_clip_t *clip, double *kernel_ms, long long *steps);
/* Motion-compensated temporal denoiser: THIS PROJECT'S OWN filter, a mode of the denoiser above.  mode 0 = off, 1 = the previous
 * denoised picture is displaced by the motion field of the searched cost pass, 2 = by that field refined (enc_mcdenoise.h,
 * tests/mcdenoise_model.py).  Per frame f: cur = the RAW input, D_{f-1} = the previous output of this filter (zeros in front of frame 0),
 * (dx, dy) = frame f's field cell of block (bx, by) (H264E_clip_read_lookahead_motion; frame 0 has a zero field).
 *   Luma vector of the 16x16 block at (16bx, 16by): mode 1 (2dx, 2dy); mode 2 the first candidate with the smallest
 * sad = sum |Y_f(x, y) - D_{f-1}(x + vx, y + vy)| among (0, 0) and then (2dx + rx, 2dy + ry), rx, ry in -1..1 in the order
 * (|rx| + |ry|, ry, rx); a candidate whose displaced block does not lie wholly inside the plane is left out.  Chroma vector of the 8x8
 * block (bx, by): (dx, dy), in both modes.  Samples that no block covers: (0, 0).
 *   Filter, per plane, with the vector v of the sample's own block: first / last row and column out = cur; otherwise the plain
 * denoiser's formula with p = D_{f-1}(clamp(s + v)) and the neighbour sum over cur(n) - D_{f-1}(clamp(n + v)), coordinates clamped to the
 * plane.  The output is the picture that is encoded and the next frame's state.  With an all-zero field it is the plain denoiser.
 *   It shares the plain denoiser's pictures, HBM budget check and rules: while the clip stands at frame 0, kept across a rewind;
 * uploading frame f again makes cost records, fields and filtered pictures from f onward new; the SSD / SSIM metrics compare the RAW
 * input with the reconstruction.  H264E_clip_set_denoise(clip, 0) switches it off too; H264E_clip_set_denoise(clip, 1) leaves the mode
 * as it is; changing the mode makes every picture again from frame 0.  In front of every launch the searched cost pass runs for the
 * frames about to be filtered -- with the lookahead controller off it runs for its field alone (H264E_clip_read_lookahead then returns
 * costs, no QPs), and H264E_clip_set_lookahead_search's refusal to change the range applies as before; range 0 is refused while this
 * filter is on.  Refused -- nothing changes, H264E_last_error names the value -- with a mode outside 0..2, with keep_records, while the
 * lookahead search range is 0 (call H264E_clip_set_lookahead_search first), below 16x16, and with speed >= 2 (the denoiser runs for
 * speed 0 and 1 only). */
int  H264E_clip_set_denoise_motion(H264E_clip_t *clip, int mode);
/* The denoised picture of a frame (either denoiser's) as packed I420, width*height*3/2 bytes: the pictures live in a ring of
 * resident_frames slots on the device; -1, with the readable frames named in H264E_last_error, when the frame has not been denoised,
 * when its slot has been taken by a later frame, and when the denoiser is off. */
int  H264E_clip_read_denoised(H264E_clip_t *clip, int frame, uint8_t *i420);
/* The vectors the motion-compensated filter used: nbx*nby cells {int8 vx, int8 vy, uint16 sad}, in luma samples, row by row; sad is
 * that of the luma vector (mode 1: of (2dx, 2dy)).  Size-only call and *nbx, *nby as for H264E_clip_read_lookahead_motion; the same
 * frames are readable as for H264E_clip_read_denoised. */
int  H264E_clip_read_denoise_motion(H264E_clip_t *clip, int frame, void *dst, int *nbx, int *nby);
/* diagnostic: HIP-event time of the motion-compensated filter's kernel launches since open, and the frames they filtered
 * (tools/mcdenoise_probe.py) */
int  H264E_clip_denoise_time(H264E_clip_t *clip, double *kernel_ms, long long *frames);
/* GOP shards of ONE stream (one clip encoder per shard / GPU, the shard starting at a key frame with first_idr_pic_id_state =
 * its GOP index & 1 and a SPECULATED mv_clusters_in): once the exact state in front of the shard is known, revalidate walks the
 * kept records (keep_records) and either confirms the shard (*restart_frame = -1, end_state = exact state behind it) or names the
 * GOP from which it has to be encoded again (restart_frame, restart_state); H264E_clip_restart rewinds the encoder to that point. */
int  H264E_clip_revalidate(H264E_clip_t *clip, const int32_t exact_in[2], int *restart_frame, int32_t restart_state[2], int32_t end_state[2]);
int  H264E_clip_restart(H264E_clip_t *clip, int frame, const int32_t state[2]);
/* kept records of an encoded frame (keep_records): per macroblock {int32 mv[0] packed (y << 16) | (x & 0xffff); int8 type: -1 skip,
 * 0..3 inter partitioning, 5 I4x4, 6 I16x16; uint8 used-cluster-candidates; 2 pad bytes} -- a per-macroblock trace for debugging */
int  H264E_clip_read_records(H264E_clip_t *clip, int frame, void *dst /* macroblocks x 8 bytes */);
void H264E_clip_close(H264E_clip_t *clip);
/* diagnostic: per-phase sums [48] of a -DH264E_STAMPS kernel build since the last call (zeros in the product): [0..31] the rows' phases in cycles, [32..47] the finalizers' in 10 ns ticks */
int  H264E_clip_stamps(H264E_clip_t *clip, unsigned long long *dst);

#ifdef __cplusplus
}
#endif
#endif
