/*
 * submit_refusals.c -- TEST ONLY (tests/test_submit_refusals.py compiles it against include/h264e_hip.h, include/h264e_mi355x.h and
 * either the emulation library or the product library).  A refused h264e_hip_submit must leave nothing behind: for each class of bad
 * task array, against a 64x48 pool with 3 chains,
 *   - the call returns -1 with its text,
 *   - h264e_hip_busy is 0 and h264e_hip_stream_done answers for every slot what it answered before the call,
 *   - and WITHOUT any h264e_hip_release, a plain H264E_clip_* encode of three 64x48 frames in this same process finishes (under
 *     alarm(): a refusal that kept the device's launch token would block it for ever) and writes its stream to argv[2], which the
 *     test compares with the stream of a run that refused nothing.
 * Every submit here is refused before anything is launched: the only kernels this program runs are those of the final encode.
 *
 *   submit_refusals none|qp|slot|denoised|mixed|all out.264
 */
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "h264e_hip.h"
#include "h264e_mi355x.h"

enum { W = 64, H = 48, CHAINS = 3, FRAMES = 3 };
static int g_failed;

static void check(int ok, const char *what, const char *detail)
{
    printf("%s: %s%s%s\n", ok ? "ok" : "FAILED", what, detail ? " -- " : "", detail ? detail : "");
    if (!ok) g_failed++;
}

static h264e_hip_task_t plain_task(int frame)
{
    h264e_hip_task_t t;
    memset(&t, 0, sizeof(t));
    t.active = 1; t.frame_index = frame; t.slice_type = 2; t.qp = 26;
    return t;
}

static h264e_hip_task_t stream_task(int slot, int ref_slot, int narrow)
{
    h264e_hip_task_t t = plain_task(slot);
    t.stream_mode = 1; t.slot = slot; t.ref_slot = ref_slot; t.ref_in_flight = ref_slot >= 0; t.slice_type = ref_slot >= 0 ? 0 : 2;
    t.narrow_window = narrow;
    return t;
}

/* one class of bad task array: returns the text h264e_hip_submit must refuse it with */
static const char *bad_tasks(const char *name, h264e_hip_task_t *t)
{
    memset(t, 0, sizeof(*t)*CHAINS);
    if (!strcmp(name, "qp")) { t[0] = plain_task(0); t[1] = plain_task(1); t[1].qp = 9; return "submit: bad task for chain 1"; }
    if (!strcmp(name, "slot")) { t[0] = stream_task(0, -1, 1); t[0].slot = CHAINS; return "submit: bad stream task 0"; }
    if (!strcmp(name, "denoised")) { t[0] = plain_task(0); t[0].denoised = 1; return "submit: task 0 asks for the denoised picture, but the denoiser is not on"; }
    if (!strcmp(name, "mixed")) { t[0] = stream_task(0, -1, 1); t[1] = stream_task(1, 0, 0); return "submit: the jobs of one launch must agree on narrow_window"; }
    return 0;
}

static void refuse(h264e_hip_pool_t *pool, const char *name)
{
    h264e_hip_task_t t[CHAINS];
    int before[CHAINS], same = 1;
    const char *want = bad_tasks(name, t);
    char what[160];
    for (int s = 0; s < CHAINS; s++) before[s] = h264e_hip_stream_done(pool, s, 0);
    const int rc = h264e_hip_submit(pool, t);
    snprintf(what, sizeof(what), "%s: refused with -1 and \"%s\"", name, want);
    check(rc == -1 && !strcmp(h264e_hip_last_error(), want), what, rc == -1 ? h264e_hip_last_error() : "the submit was accepted");
    snprintf(what, sizeof(what), "%s: the pool is not busy", name);
    check(h264e_hip_busy(pool) == 0, what, 0);
    for (int s = 0; s < CHAINS; s++) same &= h264e_hip_stream_done(pool, s, 0) == before[s];
    snprintf(what, sizeof(what), "%s: every slot answers h264e_hip_stream_done as before the call", name);
    check(same, what, 0);
}

static void on_alarm(int sig)
{
    static const char msg[] = "FAILED: the encode behind the refused submits did not finish (the device's launch token is still held)\n";
    (void)sig;
    if (write(1, msg, sizeof(msg) - 1) < 0) { /* nothing left to report it to */ }
    _exit(3);
}

static int encode(const char *path)
{
    H264E_clip_param_t par;
    H264E_clip_t *clip = 0;
    static uint8_t out[1 << 18];
    size_t n = 0;
    memset(&par, 0, sizeof(par));
    par.width = W; par.height = H; par.gop = 30; par.qp = 26; par.vbv_size_bytes = 100000/8;
    if (H264E_clip_open(&clip, &par, FRAMES)) { printf("FAILED: H264E_clip_open: %s\n", H264E_last_error()); return -1; }
    int rc = H264E_clip_generate_synth(clip, 0, FRAMES, 0, 1);
    if (!rc) rc = H264E_clip_encode(clip, out, sizeof(out), &n, 0, 0, 0);
    if (rc) printf("FAILED: encode: %s\n", H264E_last_error());
    H264E_clip_close(clip);
    if (rc) return -1;
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(out, 1, n, f) != n) { printf("FAILED: cannot write %s\n", path); if (f) fclose(f); return -1; }
    fclose(f);
    printf("ok: encoded %d frames, %zu bytes\n", FRAMES, n);
    return 0;
}

int main(int argc, char **argv)
{
    static const char *const all[] = { "qp", "slot", "denoised", "mixed" };
    h264e_hip_pool_t *pool = 0;
    h264e_hip_task_t probe[CHAINS];
    if (argc != 3 || (strcmp(argv[1], "none") && strcmp(argv[1], "all") && !bad_tasks(argv[1], probe)))
    {
        fprintf(stderr, "usage: %s none|qp|slot|denoised|mixed|all out.264\n", argv[0]);
        return 2;
    }
    setvbuf(stdout, 0, _IONBF, 0);
    if (h264e_hip_pool_create(&pool, 0, W, H, CHAINS, FRAMES)) { printf("FAILED: pool_create: %s\n", h264e_hip_last_error()); return 1; }
    for (int k = 0; k < 4; k++)
        if (!strcmp(argv[1], "all") || !strcmp(argv[1], all[k])) refuse(pool, all[k]);
    signal(SIGALRM, on_alarm);
    alarm(20);
    if (encode(argv[2])) g_failed++;
    alarm(0);
    h264e_hip_pool_destroy(pool);
    return g_failed ? 1 : 0;
}
