/*
 * emu_handoffs.h -- TEST ONLY: the arrival order of the macroblock step's wave hand-offs as a script (tests/handoff_cases.py).
 *
 * On the GPU the reconstruction wave decides the intra candidates of a macroblock while the search wave is still at work on it, and what it
 * knows of the inter decision at that moment -- nothing, the bound inter_choose announced (sig.bound(u)), the tighter one search_type writes
 * behind the 16x16 partition (L.early_bound), the final cost -- is whatever the clock produced (h264e_kernels.hip SearchSignals /
 * InterFromSearchWave).  The emulation runs a macroblock's search to its end before its reconstruction starts, so everything the search
 * wave would ever say is known: a RECORDING signal policy notes it, and a SCRIPTED policy for mb_intra_decide decides how much of it is
 * visible at every call of intra4_choose's bound (call 0 in front of the first block, call n behind block n).  A script never shows a value
 * earlier than the real pipeline could: u only where sig.bound was called, the tightened value only behind u, and an early skip -- which
 * raises nothing but the inter decision -- ends the first wait with that decision.
 *
 * H264E_EMU_HANDOFFS (read under H264E_TEST_KNOBS=1 when a pool is created, h264e_pool.h) selects the schedule:
 *   plain            the inter decision is there from the start (what row_step does)
 *   late             never there before wait_ready, and no bound at all
 *   announced        never there; u from call 0
 *   tightened@J      never there; u from call 0, the tightened value from call J
 *   arrive@K         the final cost arrives at call K (0..16), u from call 0
 *   mixed:SEED       every macroblock draws its own (arrival, first call with u, first call with the tightened value)
 * "+helper" behind any of them: the 8x8 partition type goes through a request record like the helper wave's (RecordingSignals below) and is
 * searched from that record alone once the other types are done.  The helper wave's loop itself runs on the GPU only.
 *
 * Every macroblock of a P frame leaves a record (handoff_rec_t, 16 words), kept per input frame and read with h264e_emu_handoff_records.
 * cost16 / cost4 are the macroblock's own intra costs from a run on a copy of the row state with no bound at all: what the decision has to
 * be, whichever bound the scripted run saw.
 */
#ifndef H264E_EMU_HANDOFFS_H
#define H264E_EMU_HANDOFFS_H
#ifndef H264E_EMU
#error "emulation only"
#endif
#include <map>
#include <vector>

#define HANDOFF_NEVER 99
#define HANDOFF_NONE 0x7fffffff

typedef struct
{
    int32_t flags;                      /* 1 recorded, 2 noskip() called, 4 bound(u) called, 8 the 8x8 type went through the request record */
    int32_t u, tight;                   /* bound(u); L.early_bound behind inter_choose */
    int32_t inter_type, inter_cost;     /* B.type / B.cost behind inter_choose */
    int32_t min_gcost;                  /* the smallest cost of the partition types searched: differs from inter_cost where the skip vector's cost was taken */
    int32_t cost16, cost4;              /* unbounded intra costs (cost4 = HANDOFF_NONE: intra 4x4 is off for this frame) */
    int32_t k_ready, j_u, j_tight;      /* the script: first call with the inter decision (-1 = from the start), with u, with the tightened value */
    int32_t calls;                      /* calls of the bound that asked the policy (those in front of the arrival, and the one it arrived at) */
    int32_t arrived_at;                 /* the call at which the inter decision arrived (enc_row.h mb_intra_decide, "arrived while ..."), -1 = none */
    int32_t seen_min;                   /* the smallest early bound the policy handed out */
    int32_t final_type, final_cost;
} handoff_rec_t;

struct HandoffState
{
    handoff_rec_t r;
    int nready, call;
};

static struct
{
    int on, kind, arg, helper;
    uint32_t seed;
    uint64_t counter;
    pthread_mutex_t mu;
    std::map<const uint8_t *, std::vector<handoff_rec_t> > *frames;
} g_handoff = { 0, 0, 0, 0, 0, 0, PTHREAD_MUTEX_INITIALIZER, 0 };

enum { HO_PLAIN, HO_LATE, HO_ANNOUNCED, HO_TIGHTENED, HO_ARRIVE, HO_MIXED };

/* NULL or "": off (row_step as it is).  Returns -1 for a schedule it does not know. */
static int emu_handoffs_configure(const char *s)
{
    pthread_mutex_lock(&g_handoff.mu);
    if (!g_handoff.frames) g_handoff.frames = new std::map<const uint8_t *, std::vector<handoff_rec_t> >();
    g_handoff.frames->clear();
    g_handoff.on = 0; g_handoff.helper = 0; g_handoff.counter = 0; g_handoff.arg = 0; g_handoff.seed = 0;
    int rc = 0;
    if (s && s[0])
    {
        char name[64];
        snprintf(name, sizeof(name), "%s", s);
        char *plus = strchr(name, '+');
        if (plus) { g_handoff.helper = !strcmp(plus, "+helper"); if (!g_handoff.helper) rc = -1; *plus = 0; }
        int v = 0;
        if (!strcmp(name, "plain")) g_handoff.kind = HO_PLAIN;
        else if (!strcmp(name, "late")) g_handoff.kind = HO_LATE;
        else if (!strcmp(name, "announced")) g_handoff.kind = HO_ANNOUNCED;
        else if (sscanf(name, "tightened@%d", &v) == 1 && v >= 0 && v <= 16) { g_handoff.kind = HO_TIGHTENED; g_handoff.arg = v; }
        else if (sscanf(name, "arrive@%d", &v) == 1 && v >= 0 && v <= 16) { g_handoff.kind = HO_ARRIVE; g_handoff.arg = v; }
        else if (sscanf(name, "mixed:%d", &v) == 1) { g_handoff.kind = HO_MIXED; g_handoff.seed = (uint32_t)v; }
        else rc = -1;
        g_handoff.on = !rc;
    }
    pthread_mutex_unlock(&g_handoff.mu);
    return rc;
}

static uint64_t handoff_mix(uint64_t z)          /* splitmix64 */
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30))*0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27))*0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

/* the script of the next macroblock */
static void handoff_draw(handoff_rec_t &r)
{
    int kind = g_handoff.kind, arg = g_handoff.arg;
    uint64_t h = 0;
    if (kind == HO_MIXED)
    {
        pthread_mutex_lock(&g_handoff.mu);
        h = handoff_mix(((uint64_t)g_handoff.seed << 32) ^ g_handoff.counter++);
        pthread_mutex_unlock(&g_handoff.mu);
        kind = (int)(h % 5); h /= 5;
    }
    r.k_ready = r.j_u = r.j_tight = HANDOFF_NEVER;
    switch (kind)
    {
    case HO_PLAIN: r.k_ready = -1; break;
    case HO_LATE: break;
    case HO_ANNOUNCED: r.j_u = (int)(h % 4); break;
    case HO_TIGHTENED: r.j_u = (int)(h % 3); h /= 3; r.j_tight = g_handoff.kind == HO_MIXED ? r.j_u + (int)(h % 15) : arg; break;
    case HO_ARRIVE:
        r.k_ready = g_handoff.kind == HO_MIXED ? (int)(h % 17) : arg; h /= 17;
        r.j_u = (int)(h % (unsigned)(r.k_ready + 1)); h /= 17;
        if (g_handoff.kind == HO_MIXED && (h & 1)) r.j_tight = r.j_u + (int)((h >> 1) % 17);
        break;
    }
}

/* the helper wave's request: what SearchSignals::t3_request leaves in LDS for it, and its copy of the predictor context */
struct HandoffRequest { mv32 mv_best; int sad_best, lim[4]; GCtx ctx; };

/* what the search wave says, noted; the 8x8 type through the request record when the schedule has a helper.  The helper wave's own loop
 * (h264e_kernels.hip) is not code the emulation can call, so its step is written out again in t3_wait, and the hand-off is made one: the
 * request is copied out, its live values in LDS are overwritten while the search wave goes on with the other types (it has handed them
 * over: nothing of its own may depend on them any more), and the helper's step sees only what was copied */
template <int GEOM> struct RecordingSignals
{
    RowLds *L; handoff_rec_t *r; HandoffRequest *q; const h264e_geom_t *G; const RowTask *T; int row, x, row0; bool help;
    void noskip() const { r->flags |= 2; }
    void bound(int u) const { r->flags |= 4; r->u = u; L->early_bound = u; }
    bool helper() const { return help; }
    void t3_request(mv32 mv_best, int sad_best, const rect_t &lim) const
    {
        r->flags |= 8;
        q->mv_best = mv_best; q->sad_best = sad_best;
        q->lim[0] = lim.x0; q->lim[1] = lim.y0; q->lim[2] = lim.x1; q->lim[3] = lim.y1;
        q->ctx = L->gctx[3];
        L->t3_mv_best = 0x5a5a5a5a; L->t3_sad_best = 0x5a5a5a5a;
        memset(L->t3_lim, 0x5a, sizeof(L->t3_lim));
        memset(&L->gctx[3], 0x5a, sizeof(GCtx));
    }
    /* the helper wave's turn: it knows the macroblock's index and the request, nothing of inter_choose's own state */
    bool t3_wait() const
    {
        L->t3_mv_best = q->mv_best; L->t3_sad_best = q->sad_best;
        memcpy(L->t3_lim, q->lim, sizeof(L->t3_lim));
        L->gctx[3] = q->ctx;
        MbCtx m;
        mb_ctx_init<GEOM>(m, *L, *G, *T, row, x, row0, 2);
        const rect_t lim = { L->t3_lim[0], L->t3_lim[1], L->t3_lim[2], L->t3_lim[3] };
        search_type(*L, L->mb[x & 1], m, 3, L->t3_mv_best, L->t3_sad_best, lim, 0);
        return true;
    }
};

/* what the reconstruction wave sees of it, call by call */
struct ScriptedInter
{
    HandoffState *s;
    bool ready() const
    {
        handoff_rec_t &r = s->r;
        const int n = s->nready++;
        /* in front of the intra candidates: the first look, and the one behind wait_noskip_or_ready -- which only the inter decision ends
         * for an early skip */
        if (n < 2) return r.k_ready < 0 || (n == 1 && !(r.flags & 2));
        s->call = n - 2;
        r.calls = s->call + 1;
        const bool there = s->call >= r.k_ready;
        if (there && r.arrived_at < 0) r.arrived_at = s->call;
        return there;
    }
    int early_bound() const
    {
        handoff_rec_t &r = s->r;
        int v = HANDOFF_NONE;
        if (r.flags & 4) v = s->call >= r.j_tight ? r.tight : s->call >= r.j_u ? r.u : HANDOFF_NONE;
        if (v < r.seen_min) r.seen_min = v;
        return v;
    }
    bool wait_noskip_or_ready() const { return true; }
    bool wait_bound_or_ready() const { return true; }
    bool wait_ready() const { return true; }
    bool before_decide() const { return true; }
};

/* row_step (enc_row.h) with the two policies above, and the record */
template <int GEOM> static void handoff_row_step(RowLds &L, const h264e_geom_t &G, const ChainG &C, const RowTask &T, const uint8_t *frame_key, int row, int x, int row0, int row1)
{
    MbBuf &B = L.mb[x & 1];
    MbCtx m;
    HandoffState s;
    HandoffRequest q;
    memset(&s, 0, sizeof(s));
    memset(&q, 0, sizeof(q));
    handoff_rec_t &r = s.r;
    const bool inter = GEOM != GEOM_INTRA && T.slice_type == 0;
    handoff_draw(r);
    r.arrived_at = -1; r.seen_min = HANDOFF_NONE; r.cost4 = HANDOFF_NONE; r.cost16 = HANDOFF_NONE; r.u = r.tight = HANDOFF_NONE;
    load_top<LOAD_TOP_ALL>(L, B, G, C.bottom + (size_t)(row - 1)*G.nmbx, C.pend + (size_t)(row - 1)*G.nmbx, x, row > row0);
    if (inter) for (int t = 0; t < 4; t++) L.gcost[t] = HANDOFF_NONE;        /* (only the types searched are ever read) */
    mb_search<GEOM>(L, B, G, T, row, x, row0, RecordingSignals<GEOM>{ &L, &r, &q, &G, &T, row, x, row0, g_handoff.helper != 0 });
    mb_ctx_init<GEOM>(m, L, G, T, row, x, row0, 1);
    if (inter)
    {
        r.flags |= 1;
        r.inter_type = B.type; r.inter_cost = B.cost;
        if (r.flags & 4) r.tight = L.early_bound;
        r.min_gcost = imin(imin(L.gcost[0], L.gcost[1]), imin(L.gcost[2], L.gcost[3]));
        if (B.type >= 0)
        {
            /* the macroblock's own intra costs, no bound: on a copy of the row state, which the candidates write all over */
            RowLds *keep = (RowLds *)malloc(sizeof(RowLds));
            if (!keep) abort();
            memcpy(keep, &L, sizeof(RowLds));
            MbCtx mc = m;
            unsigned nz = 0;
            r.cost16 = intra16_cost(L, B, mc);
            if (T.speed < 2) r.cost4 = intra4_choose(L, B, mc, []() -> int { return HANDOFF_NONE; }, nz);
            memcpy(&L, keep, sizeof(RowLds));
            free(keep);
        }
    }
    if (!inter)
    {
        r.k_ready = -1;                         /* an I frame has no search wave to wait for, and leaves no records: only its place among the frames */
        pthread_mutex_lock(&g_handoff.mu);
        (*g_handoff.frames)[frame_key].clear();
        pthread_mutex_unlock(&g_handoff.mu);
    }
    mb_intra_decide(L, B, m, T, ScriptedInter{ &s });
    r.final_type = m.type; r.final_cost = m.cost;
    if (inter)
    {
        pthread_mutex_lock(&g_handoff.mu);
        std::vector<handoff_rec_t> &v = (*g_handoff.frames)[frame_key];
        if ((int)v.size() != G.nmb) v.assign((size_t)G.nmb, handoff_rec_t());
        v[(size_t)m.num] = r;
        pthread_mutex_unlock(&g_handoff.mu);
    }
    mb_recon_write<GEOM>(L, B, m, G, C, T, row, x, row0, row1, NoHook{});
}

/* the records of the P frame whose input is `frame` frames of `frame_bytes` behind the lowest input address seen since the schedule was
 * set (a clip that is resident as a whole: its frame index).  Returns the number of macroblocks, 0 when that frame left no record (an I
 * frame), -1 when dst is too small. */
extern "C" int h264e_emu_handoff_records(int frame, size_t frame_bytes, int32_t *dst, int cap_records)
{
    int n = 0;
    pthread_mutex_lock(&g_handoff.mu);
    if (g_handoff.frames && !g_handoff.frames->empty())
    {
        const uint8_t *base = g_handoff.frames->begin()->first;
        std::map<const uint8_t *, std::vector<handoff_rec_t> >::const_iterator it = g_handoff.frames->find(base + frame_bytes*(size_t)frame);
        if (it != g_handoff.frames->end())
        {
            n = (int)it->second.size();
            if (n > cap_records) n = -1;
            else memcpy(dst, it->second.data(), sizeof(handoff_rec_t)*(size_t)n);
        }
    }
    pthread_mutex_unlock(&g_handoff.mu);
    return n;
}

/*
 * The same for the finalizer (enc_finalize.h job_finalize): on the GPU the verdict of the frame in front arrives whenever the clock has
 * it -- before this frame's first row, somewhere in the middle, behind its last row.  Here the frame in front is always done, so WHEN its
 * flag reads "up" is a script.  H264E_EMU_VERDICT (H264E_TEST_KNOBS=1, read with H264E_EMU_HANDOFFS) selects it:
 *   from_start       up at the first look (what FinalizerInOrder shows)
 *   at_row@K         not up until the finalizer asks for row K of its own frame
 *   after_last       not up at any look; it arrives in a wait
 * A wait for the flag is where time passes: it ends with the flag up under every schedule (a verdict that never comes is a launch failure,
 * and not scripted).  A row is "late" once: what the finalizer does while it waits for a row runs once in front of every row.
 * Every run of a finalizer leaves a record (verdict_rec_t, 8 words), in the order they ran, read with h264e_emu_verdict_records.
 */
#define H264E_EMU_VERDICT_SCHEDULES      /* h264e_pool.h configures the schedule where it sees this */
enum { VERDICT_NOT_NEEDED, VERDICT_BY_LOOK, VERDICT_BY_WAIT_IN_SPLICE, VERDICT_BY_WAIT_BEHIND, VERDICT_NEVER };
typedef struct
{
    int32_t frame;                      /* filled in by the reader: the input frame's place, like h264e_emu_handoff_records */
    int32_t launch_id;
    int32_t how, row;                   /* VERDICT_*: how the verdict of the frame in front was taken, and the row asked for then (nmby behind the splice) */
    int32_t status, first_bad;          /* the verdict this frame published (0: none) */
    int32_t fixed;                      /* the walk ran on the fixed state (more than one slice) */
    int32_t nmby;
} verdict_rec_t;

enum { VS_FROM_START, VS_AT_ROW, VS_AFTER_LAST };
static struct
{
    int on, kind, arg;
    std::vector<std::pair<const uint8_t *, verdict_rec_t> > *runs;
} g_verdict = { 0, 0, 0, 0 };

/* NULL or "": off.  Returns -1 for a schedule it does not know. */
static int emu_verdict_configure(const char *s)
{
    int rc = 0, v = 0;
    pthread_mutex_lock(&g_handoff.mu);
    if (!g_verdict.runs) g_verdict.runs = new std::vector<std::pair<const uint8_t *, verdict_rec_t> >();
    g_verdict.runs->clear();
    g_verdict.on = 0; g_verdict.arg = 0;
    if (s && s[0])
    {
        if (!strcmp(s, "from_start")) g_verdict.kind = VS_FROM_START;
        else if (!strcmp(s, "after_last")) g_verdict.kind = VS_AFTER_LAST;
        else if (sscanf(s, "at_row@%d", &v) == 1 && v >= 0) { g_verdict.kind = VS_AT_ROW; g_verdict.arg = v; }
        else rc = -1;
        g_verdict.on = !rc;
    }
    pthread_mutex_unlock(&g_handoff.mu);
    return rc;
}

struct FinalizerScripted : FinalizerInOrder
{
    verdict_rec_t *r;
    int kind, arg;
    int cur_row = 0, spliced = 0, waited = 0;
    template <class IDLE> int wait_row(int row, IDLE idle) { cur_row = row; return idle() ? 1 : 0; }
    bool prev_up()
    {
        waited = 0;
        return (kind == VS_FROM_START || (kind == VS_AT_ROW && cur_row >= arg)) && FinalizerInOrder::prev_up();
    }
    bool wait_prev()
    {
        waited = 1;
        const bool up = FinalizerInOrder::prev_up();
        if (!up) r->how = VERDICT_NEVER;
        return up;
    }
    void acquire_prev()
    {
        r->how = !waited ? VERDICT_BY_LOOK : spliced ? VERDICT_BY_WAIT_BEHIND : VERDICT_BY_WAIT_IN_SPLICE;
        r->row = spliced ? r->nmby : cur_row;
    }
    void publish_verdict(h264e_walkrec_t *w) const { r->status = w->status; r->first_bad = w->first_bad; FinalizerInOrder::publish_verdict(w); }
    void stamp(int id) { if (id == 32) spliced = 1; }      /* stamp 32: the splice is over */
};

static void verdict_job_finalize(const h264e_geom_t &G, const ChainG &C, const h264e_frame_task_t &T)
{
    verdict_rec_t r;
    memset(&r, 0, sizeof(r));
    r.launch_id = T.launch_id; r.how = VERDICT_NOT_NEEDED; r.row = -1; r.first_bad = -1; r.fixed = T.nslices > 1; r.nmby = G.nmby;
    FinalizerScripted s{ { T }, &r, g_verdict.kind, g_verdict.arg };
    job_finalize(G, C, T, s);
    pthread_mutex_lock(&g_handoff.mu);
    g_verdict.runs->push_back(std::make_pair(T.in[0], r));
    pthread_mutex_unlock(&g_handoff.mu);
}

/* every finalizer run since the schedule was set, in the order they ran; `frame` = the input's place, in frames of `frame_bytes` behind
 * the lowest input address among them.  Returns their number, -1 when dst is too small. */
extern "C" int h264e_emu_verdict_records(size_t frame_bytes, int32_t *dst, int cap_records)
{
    pthread_mutex_lock(&g_handoff.mu);
    int n = g_verdict.runs ? (int)g_verdict.runs->size() : 0;
    if (n > cap_records) n = -1;
    else if (n)
    {
        const uint8_t *base = (*g_verdict.runs)[0].first;
        for (int i = 0; i < n; i++) if ((*g_verdict.runs)[(size_t)i].first < base) base = (*g_verdict.runs)[(size_t)i].first;
        for (int i = 0; i < n; i++)
        {
            verdict_rec_t r = (*g_verdict.runs)[(size_t)i].second;
            r.frame = (int32_t)((size_t)((*g_verdict.runs)[(size_t)i].first - base)/frame_bytes);
            memcpy(dst + 8*i, &r, sizeof(r));
        }
    }
    pthread_mutex_unlock(&g_handoff.mu);
    return n;
}

#endif
