"""CPU: which key frames of a launch are led, and the dispatch order that gives (h264e_pool.h lead_jobs, order_by_start_step,
order_into_bands), through the test hook h264e_hip_selftest_lead_order of the emulation library -- the product's own host
code.  A led job's ROW workgroups sort at 2*row, as if the job stood at the launch's start; its finalizer stays where it was.  Checked
on pictures of 18 rows (352x288) and 128 rows (16x2048), 20-160 jobs, both window lags, one and three member streams, plain and through
the XCD bands: the order is complete, equal to the unled one when nothing is led, and every workgroup still stands behind everything it
waits for.  The emulation runs a launch's jobs one after the other and ignores the order, so the clip encodes at the end pin the host's
bookkeeping only (clip_keep_collect with led frames, the launch line)."""
import ctypes as C
import functools
import os
import subprocess

import pytest

import key_keep_cases as cases
import key_lead_cases as lead
import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
PAD = 0xffffffff
DEP_ROWS = {4: 1, 7: 2}           # window lag -> rows of the frame in front below a row's own that its reference window needs
BIG = 1 << 20


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


@functools.lru_cache(maxsize=None)
def _lib():
    L = pkg.load_pkg().load(pkg.EMU_LIB)
    L.h264e_hip_selftest_lead_order.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_int), C.c_int, C.c_int,
                                                C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint8)]
    L.h264e_hip_selftest_lead_order.restype = C.c_long
    L.h264e_hip_selftest_merged_order.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_uint32), C.c_size_t]
    L.h264e_hip_selftest_merged_order.restype = C.c_long
    L.h264e_hip_pool_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.h264e_hip_pool_destroy.argtypes = [C.c_void_p]
    L.h264e_hip_selftest_order.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_size_t]
    L.h264e_hip_selftest_order.restype = C.c_long
    return L


def lead_order(nmby, lag, member_jobs, key, first_row, resident, budget, tree=0, all_intra=0, banded=0):
    """(order, led) of the hook"""
    jobs = sum(member_jobs)
    cap = jobs * 8 * ((nmby + 7) // 8 + 1) + 8
    buf, led = (C.c_uint32 * cap)(), (C.c_uint8 * jobs)()
    n = _lib().h264e_hip_selftest_lead_order(nmby, lag, (C.c_int * len(member_jobs))(*member_jobs), len(member_jobs), (C.c_uint8 * jobs)(*key),
                                             (C.c_int * jobs)(*first_row), tree, all_intra, resident, budget, banded, buf, cap, led)
    assert 0 < n <= cap
    return list(buf[:n]), list(led)


def merged_order(rows, lag, member_jobs):
    cap = rows * sum(member_jobs)
    buf = (C.c_uint32 * cap)()
    assert _lib().h264e_hip_selftest_merged_order(rows, lag, (C.c_int * len(member_jobs))(*member_jobs), len(member_jobs), buf, cap) == cap
    return list(buf)


def streams(member_jobs, gop):
    """(key, first_row, candidates): every member's job j is a key frame when j % gop == gop - 1 (never job 0 of a member), with no row
    yet; the key frames' launch jobs in candidate order -- job of the member, then member"""
    key, first_row, cand = [], [], []
    for m, nj in enumerate(member_jobs):
        for j in range(nj):
            key.append(1 if j % gop == gop - 1 else 0)
            first_row.append(0)
            if key[-1]:
                cand.append((j, m, len(key) - 1))
    cand.sort()
    return key, first_row, [job for _, _, job in cand]


def members_of(member_jobs):
    """launch job -> (member, job within the member)"""
    return [(m, j) for m, nj in enumerate(member_jobs) for j in range(nj)]


def model_led(member_jobs, key, first_row, nmby, resident, budget, tree=0, all_intra=0):
    """lead_jobs, from its description: candidates nearest first (job of the member, then member), whole frames passed over, the first
    that does not fit the budget ends it"""
    jobs = sum(member_jobs)
    led = [0] * jobs
    if tree or all_intra or budget <= 0 or jobs * (nmby + 1) <= resident:
        return led
    who, used = members_of(member_jobs), 0
    for j, m, job in sorted((who[job][1], who[job][0], job) for job in range(jobs) if key[job] and who[job][1] > 0):
        cost = nmby - first_row[job]
        if cost <= 0:
            continue
        if used + cost > budget:
            break
        led[job], used = 1, used + cost
    return led


def model_order(member_jobs, led, nmby, lag):
    who = members_of(member_jobs)
    ents = sorted(((2 * r if led[job] and r < nmby else lag * who[job][1] + 2 * r), who[job][1], who[job][0], r, job)
                  for job in range(len(who)) for r in range(nmby + 1))
    return [(job << 16) | r for _, _, _, r, job in ents]


SHAPES = [(18, (20,)), (18, (160,)), (128, (20,)), (128, (40,)), (18, (60, 35, 50)), (128, (7, 9, 4))]
IDS = ["18rows-20", "18rows-160", "128rows-20", "128rows-40", "18rows-60+35+50", "128rows-7+9+4"]


def check_safe(order, led, member_jobs, nmby, lag):
    """every workgroup stands behind what it waits for"""
    pos = {e: i for i, e in enumerate(order) if e != PAD}
    who, base = members_of(member_jobs), [sum(member_jobs[:m]) for m in range(len(member_jobs))]
    at = lambda job, r: pos[(job << 16) | r]
    for job, (m, j) in enumerate(who):
        for r in range(1, nmby + 1):
            assert at(job, r) > at(job, r - 1)                    # the row above; the finalizer behind the last row (and so all rows)
        if j > 0:
            front = base[m] + j - 1
            assert at(job, nmby) > at(front, nmby)                # the verdict of the frame in front
            if not led[job]:                                     # (a led job is a key frame: it reads no reference)
                for r in range(nmby):
                    assert at(job, r) > at(front, min(r + DEP_ROWS[lag], nmby - 1))


@pytest.mark.parametrize("lag", [4, 7])
@pytest.mark.parametrize("nmby,member_jobs", SHAPES, ids=IDS)
def test_led_order_is_a_safe_permutation_and_the_finalizers_stay(nmby, member_jobs, lag):
    jobs, rows = sum(member_jobs), nmby + 1
    key, first_row, cand = streams(member_jobs, 3)
    first_row[cand[0]] = nmby                   # the nearest key frame is whole, the next has its upper third
    first_row[cand[1]] = nmby // 3
    budget = 4 * nmby
    order, led = lead_order(nmby, lag, member_jobs, key, first_row, 64, budget)
    assert led == model_led(member_jobs, key, first_row, nmby, 64, budget) and sum(led) >= 3
    assert sorted(order) == [(j << 16) | r for j in range(jobs) for r in range(rows)]
    assert order == model_order(member_jobs, led, nmby, lag)
    check_safe(order, led, member_jobs, nmby, lag)
    # a led job's finalizer sits exactly where it sat without the lead: between the same neighbours.  (Its index grows by the led rows
    # of later jobs that now stand in front of it.)  Nothing but the led rows has moved: without them the two orders are the same
    plain = merged_order(rows, lag, member_jobs)
    moved = lambda e: led[e >> 16] and (e & 0xffff) < nmby
    assert [e for e in order if not moved(e)] == [e for e in plain if not moved(e)]
    at, plain_at = {e: i for i, e in enumerate(order)}, {e: i for i, e in enumerate(plain)}
    for job in range(jobs):
        if led[job]:
            fin = (job << 16) | nmby
            later = sum(1 for e in plain[plain_at[fin]:] if moved(e))
            assert at[fin] == plain_at[fin] + later
    # the led rows are what the launch starts with: in front of the last of them stand only workgroups of a key up to 2*(nmby - 1) --
    # led rows, and the rows of every member's first 2*(nmby - 1)/lag + 1 jobs
    pos = {e: i for i, e in enumerate(order)}
    last = max(pos[(job << 16) | r] for job in range(jobs) if led[job] for r in range(nmby))
    assert last < (len(member_jobs) * (2 * (nmby - 1) // lag + 1) + sum(led)) * rows


@pytest.mark.parametrize("lag", [4, 7])
@pytest.mark.parametrize("nmby,jobs", [(18, 20), (18, 160), (128, 20), (128, 40), (5, 30)], ids=["18rows-20", "18rows-160", "128rows-20", "128rows-40", "5rows-30"])
def test_led_order_through_the_xcd_bands(nmby, jobs, lag):
    rows, per = nmby + 1, (nmby + 7) // 8 + 1
    key, first_row, cand = streams((jobs,), 5)
    first_row[cand[1]] = nmby // 2
    order, led = lead_order(nmby, lag, (jobs,), key, first_row, 64, 3 * nmby, banded=1)
    assert sum(led) >= 2
    assert len(order) == 8 * per * jobs                     # equally long queues
    real = [e for e in order if e != PAD]
    assert sorted(real) == [(j << 16) | r for j in range(jobs) for r in range(rows)]
    # the workgroups of one XCD's queue keep the order they have in the plain led order, which is safe: a workgroup waits only for
    # workgroups in front of it in its own queue or in other queues
    plain, plain_led = lead_order(nmby, lag, (jobs,), key, first_row, 64, 3 * nmby)
    assert plain_led == led
    check_safe(plain, led, (jobs,), nmby, lag)
    plain_at = {e: i for i, e in enumerate(plain)}
    owner = [[None if e == PAD else e >> 16 for e in order[x::8]] for x in range(8)]
    for x in range(8):
        q = order[x::8]
        for e in q:
            if e != PAD and (e & 0xffff) < nmby:
                assert min(7, (e & 0xffff) * 8 // nmby) == x        # a row on the XCD of its band
        # inside a queue the entries keep the order of the plain led order
        at = [plain_at[e] for e in q if e != PAD]
        assert at == sorted(at)
    for job in range(jobs):
        assert sum(o == job for x in range(8) for o in owner[x]) == rows
        if led[job]:
            assert all(sum(o == job for o in owner[x]) <= per - 1 for x in range(7))    # its rows take per - 1 entries of a queue, the finalizer one
    # the queues advance together: entry k of every queue belongs to a led job or to a job within one of k // per, give or take the
    # entries the led jobs took in front (at most a job's worth each)
    for x in range(8):
        for k, job in enumerate(owner[x]):
            if job is not None and not led[job]:
                assert abs(job - k // per) <= (2 * rows) // lag + 1 + sum(led)


def test_no_led_job_gives_the_unled_order_word_for_word():
    L = _lib()
    for nmby, member_jobs in SHAPES:
        for lag in (4, 7):
            key, first_row, _ = streams(member_jobs, 6)
            want = merged_order(nmby + 1, lag, member_jobs)
            # budget 0; no key frame; a grid that is resident; hedge leaves; all intra; every key frame whole
            for kw in (dict(budget=0), dict(key=[0] * len(key)), dict(resident=sum(member_jobs) * (nmby + 1)), dict(tree=1), dict(all_intra=1),
                       dict(first_row=[nmby] * len(key))):
                a = dict(key=key, first_row=first_row, resident=512, budget=4 * nmby)
                a.update(kw)
                order, led = lead_order(nmby, lag, member_jobs, **a)
                assert not any(led) and order == want, kw
    # ... and through the bands: the pool's own banded order
    for w, h, jobs, narrow in ((352, 288, 20, 1), (16, 2048, 20, 0)):
        nmby = (h + 15) // 16
        pool = C.c_void_p()
        assert L.h264e_hip_pool_create(C.byref(pool), 0, w, h, jobs, 1) == 0
        try:
            cap = jobs * 8 * ((nmby + 7) // 8 + 1)
            buf = (C.c_uint32 * cap)()
            assert L.h264e_hip_selftest_order(pool, jobs, narrow, 1, buf, cap) == cap
            key, first_row, _ = streams((jobs,), 6)
            order, led = lead_order(nmby, 4 if narrow else 7, (jobs,), key, first_row, 512, 0, banded=1)
            assert not any(led) and order == list(buf)
            assert L.h264e_hip_selftest_order(pool, jobs, narrow, 0, buf, cap) == jobs * (nmby + 1)
            order, led = lead_order(nmby, 4 if narrow else 7, (jobs,), key, first_row, BIG, 4 * nmby)
            assert not any(led) and order == list(buf[:jobs * (nmby + 1)])
        finally:
            L.h264e_hip_pool_destroy(pool)


def test_grid_against_the_resident_workgroups_decides():
    nmby, jobs = 18, 81                         # 81 x 19 = 1539 workgroups
    key, first_row, _ = streams((jobs,), 6)
    for resident, on in ((1536, True), (1539, False), (2048, False), (512, True)):
        _, led = lead_order(nmby, 4, (jobs,), key, first_row, resident, 384)
        assert any(led) == on


@pytest.mark.parametrize("member_jobs", [(160,), (60, 35, 50)], ids=["one-member", "three-members"])
def test_budget_whole_frames_and_nearest_first(member_jobs):
    nmby = 18
    key, first_row, cand = streams(member_jobs, 6)
    who = members_of(member_jobs)
    assert all(who[job][1] > 0 for job in cand)
    first_row[cand[0]] = nmby                   # whole: costs nothing, is not led
    first_row[cand[2]] = 11                     # costs 7
    for budget in (1, 17, 18, 24, 25, 42, 43, 60, 61, 384, 5000):
        _, led = lead_order(nmby, 4, member_jobs, key, first_row, 512, budget)
        assert led == model_led(member_jobs, key, first_row, nmby, 512, budget)
        used = sum(nmby - first_row[job] for job in range(len(led)) if led[job])
        assert used <= budget
        assert not led[cand[0]]
        assert not any(led[job] and not key[job] for job in range(len(led)))
        # the led ones are the nearest candidates that are not whole, without a gap
        rest = [job for job in cand if first_row[job] < nmby]
        n = sum(led)
        assert [job for job in rest if led[job]] == rest[:n]
        assert n <= 64
        if n < len(rest) and n < 64:
            assert used + nmby - first_row[rest[n]] > budget      # the next one did not fit
    _, led = lead_order(nmby, 4, member_jobs, key, first_row, 512, 18)
    assert sum(led) == 1 and led[cand[1]]
    # job 0 of a member is never led, key frame or not
    key0 = list(key)
    for m in range(len(member_jobs)):
        key0[sum(member_jobs[:m])] = 1
    _, led = lead_order(nmby, 4, member_jobs, key0, first_row, 512, 5000)
    assert not any(led[sum(member_jobs[:m])] for m in range(len(member_jobs)))


# ---- the clip encoder with led key frames (the emulation: bookkeeping only)

N, W, H, KW = 24, 96, 80, dict(gop=4, qp=26)
KNOBS = {"H264E_TEST_LEAD_RESIDENT": "8"}      # a launch of two frames is already "larger than the chip"


@functools.lru_cache(maxsize=None)
def _clip_run(budget, cap):
    want, want_sizes = cases.reference("pan", W, H, N, **KW)
    return lead.encode("pan", W, H, N, lead=budget, lib=pkg.EMU_LIB, cap=cases.cap_for_three(want_sizes) if cap else None, knobs=KNOBS, **KW)


@pytest.mark.parametrize("cap", [False, True], ids=["one-call", "buffer-of-3"])
@pytest.mark.parametrize("budget", [10, 5, 3, 0], ids=["two-frames", "one-frame", "less-than-a-frame", "off"])
def test_clip_with_led_key_frames_is_the_oracles(budget, cap):
    want, want_sizes = cases.reference("pan", W, H, N, **KW)
    out, sizes, tot = _clip_run(budget, cap)
    assert sizes == want_sizes and out == want
    if budget >= 5:
        assert tot["led_frames"] > 0 and 0 < tot["led_rows"] <= budget * tot["calls"] * N
    else:
        assert tot["led_frames"] == 0 and tot["led_rows"] == 0
    if cap:
        # the kept frames are whole in the emulation, so the launch behind a stop leads the key frames behind them
        assert tot["calls"] > 1 and tot["kept_key_frames"] > 0
        assert tot["kept_key_rows"] == tot["kept_key_frames"] * ((H + 15) // 16)


def test_without_the_knob_a_small_clip_leads_nothing():
    want, want_sizes = cases.reference("pan", W, H, N, **KW)
    out, sizes, tot = lead.encode("pan", W, H, N, lead=10, lib=pkg.EMU_LIB, **KW)
    assert sizes == want_sizes and out == want
    assert tot["led_frames"] == 0                # 24 x 6 workgroups are resident as a whole


def test_keeping_off_switches_the_lead_off():
    out, sizes, tot = lead.encode("pan", W, H, N, lead=10, lib=pkg.EMU_LIB, keep=False, knobs=KNOBS, **KW)
    assert (out, sizes) == _clip_run(10, False)[:2]
    assert tot["led_frames"] == 0 and tot["kept_key_frames"] == 0
