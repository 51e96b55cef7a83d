"""Replay of tests/golden/run_params.json: streams of the REFERENCE encoder whose H264E_run_param_t changes from frame to frame
(oracle/api_harness.c, tests/golden/make_golden_run_params.py) through the oracle and through the product's H264E_encode.

A case is {"create": [w, h, gop, vbv_size_bytes, const_input_flag, temporal_denoise_flag, slices], "frames": [line, ...]} plus what the
reference answered; a line is [frame_type, encode_speed, desired_frame_bytes, qp_min, qp_max, vbv_size, vbv_fullness, null_run_param]:
vbv_size >= 0 calls H264E_set_vbv_state(vbv_size, vbv_fullness) in front of the frame, null_run_param passes run_param = NULL.  A line
whose frame type is none of DEFAULT / P / KEY is a call the product refuses (H264E_STATUS_BAD_FRAME_TYPE): the reference was not
called for it, its recorded size is -1, and the picture it was offered goes to the next line.  Pictures are synth_v1 frames 0, 1, ..."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

import clips
import denoise_model

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "run_params.json")
DEFAULT, P_FRAME, KEY = 0, 2, 6
ACCEPTED = (DEFAULT, P_FRAME, KEY)
REFUSED_TYPES = {"I": 5, "DROPPABLE": 1, "GOLDEN": 4, "RECOVERY": 3, "CUSTOM": 99}
BAD_FRAME_TYPE = 3
EMU_PIXEL_BUDGET = 352 * 288 * 8          # the budget of tests/test_emu_parity.py


def load():
    return json.load(open(FIXTURE))


def script_text(case):
    return "".join(" ".join(str(x) for x in l) + "\n" for l in [case["create"]] + case["frames"])


def pixels(case):
    w, h = case["create"][:2]
    return w * h * sum(1 for l in case["frames"] if l[0] in ACCEPTED)


def line_text(case, i):
    return "line %d: frame_type=%d speed=%d desired_frame_bytes=%d qp_min=%d qp_max=%d set_vbv_state=(%d, %d) null_run_param=%d" % ((i,) + tuple(case["frames"][i]))


def pictures(case):
    """(raw pictures, the pictures the encoder codes): one per accepted call; the second differ with the denoiser on, which runs on
    frames with encode_speed < 2 (h264-lab.h:6684-6695).  (Denoiser cases have no NULL run_param: the reference reads opt there.)"""
    w, h, den = case["create"][0], case["create"][1], case["create"][5]
    lines = [l for l in case["frames"] if l[0] in ACCEPTED]
    raw = clips.make("synth", w, h, len(lines))
    if not den:
        return raw, raw
    assert not any(l[7] for l in lines)
    return raw, denoise_model.clip(raw, w, h, apply=[l[1] < 2 for l in lines])


def compare(case, got, what):
    """got: per line (status, coded bytes, written-back planes or None).  Exact bytes; names the first line that differs."""
    cinp = case["create"][4]
    for i, (status, data, planes) in enumerate(got):
        where = "%s: %s" % (what, line_text(case, i))
        if case["sizes"][i] < 0:
            assert status == BAD_FRAME_TYPE and not data, "%s: a refused frame type must answer H264E_STATUS_BAD_FRAME_TYPE, got status %d, %d bytes" % (where, status, len(data))
            continue
        assert status == 0, "%s: status %d" % (where, status)
        assert len(data) == case["sizes"][i], "%s: %d bytes, the reference %d" % (where, len(data), case["sizes"][i])
        assert hashlib.md5(data).hexdigest() == case["md5"][i], "%s: same size, other bytes than the reference" % where
        if not cinp:
            assert hashlib.md5(planes).hexdigest() == case["recon_md5"][i], "%s: the planes written back differ from the reference's reconstruction" % where
    assert len(got) == len(case["frames"])
    whole = b"".join(d for _, d, _ in got)
    assert (len(whole), hashlib.md5(whole).hexdigest()) == (case["bytes"], case["stream_md5"])


def replay_oracle(case):
    import oracle_lib
    w, h, gop, vbv, cinp, _den, slices = case["create"]
    _, pics = pictures(case)
    par = oracle_lib.Param(w, h, gop, 0, 0, vbv, 0, slices)
    L = oracle_lib.lib()
    e = L.h264o_open(C.byref(par))
    assert e
    got, t = [], 0
    back = np.empty(w * h * 3 // 2, np.uint8)
    try:
        for ft, speed, dfb, qmin, qmax, vsize, vfull, null in case["frames"]:
            st = L.h264o_set_run_param(e, ft, speed, dfb, qmin, qmax, null if ft in ACCEPTED else 0)
            if st:
                got.append((st, b"", None))
                continue
            if vsize >= 0:
                L.h264o_set_vbv_state(e, vsize, vfull)
            f = np.ascontiguousarray(pics[t], np.uint8)
            t += 1
            base = f.ctypes.data
            yuv = (C.c_void_p * 3)(base, base + w * h, base + w * h * 5 // 4)
            stride = (C.c_int * 3)(w, w // 2, w // 2)
            p, n = C.c_void_p(), C.c_int()
            st = L.h264o_encode(e, yuv, stride, C.byref(p), C.byref(n))
            data = C.string_at(p, n.value) if not st else b""
            if not cinp and not st:
                L.h264o_get_written_back(e, back.ctypes.data)
            got.append((st, data, back.tobytes() if not cinp else None))
    finally:
        L.h264o_close(e)
    return got


def replay_product(P, case, lib=None, device=None):
    """every line through H264E_encode of P.Encoder (lib: the emulation library, or None for the product library): the fields of e.rp,
    the frame type and the NULL pointer per line.  device: a function picture -> (frame, fmt) in GPU memory; the line then goes
    through H264E_encode_device (const_input_flag = 1 cases only)."""
    w, h, gop, vbv, cinp, den, slices = case["create"]
    raw, _ = pictures(case)
    e = P.Encoder(w, h, gop=gop, const_input=cinp, vbv_size_bytes=vbv, lib=lib, slices=slices if slices > 1 else 0, denoise=bool(den))
    got, t = [], 0
    try:
        for ft, speed, dfb, qmin, qmax, vsize, vfull, null in case["frames"]:
            if vsize >= 0:
                e.set_vbv_state(vsize, vfull)
            e.rp.frame_type, e.rp.encode_speed, e.rp.desired_frame_bytes, e.rp.qp_min, e.rp.qp_max = ft, speed, dfb, qmin, qmax
            f = np.ascontiguousarray(raw[min(t, len(raw) - 1)], np.uint8).copy()
            before = f.copy()
            data, n = C.c_void_p(), C.c_int()
            rp = None if null else C.byref(e.rp)
            if device is None:
                base = f.ctypes.data
                io = P.IoYuv((C.c_void_p * 3)(base, base + w * h, base + w * h * 5 // 4), (C.c_int * 3)(w, w // 2, w // 2))
                st = e.L.H264E_encode(e.persist, e.scratch, rp, C.byref(io), C.byref(data), C.byref(n))
            else:
                frame, fmt = device(f)
                d, _keep = P.dev_frame(frame, fmt, w, h)
                st = e.L.H264E_encode_device(e.persist, e.scratch, rp, C.byref(d), C.byref(data), C.byref(n))
            if st:
                assert np.array_equal(f, before), "%s: a refused call wrote to the caller's planes" % line_text(case, len(got))
                got.append((st, b"", None))
                continue
            t += 1
            got.append((0, C.string_at(data, n.value), f.tobytes() if not cinp else None))
    finally:
        e.close()
    return got


def _effective(case):
    """per line: (the line as the encoder sees it -- a NULL run_param repeats the stored one --, overflow event or not)"""
    stored, out = None, []
    for l in case["frames"]:
        if l[0] not in ACCEPTED:
            out.append((None, False))
            continue
        if not l[7]:
            stored = l
        over = l[5] > 0 and l[6] * 8 - stored[2] * 8 > l[5] * 8        # h264-lab.h:6497-6498 right after H264E_set_vbv_state
        out.append((stored, over))
    return out


def coverage(cases):
    """what the fixture is FOR, counted over what the reference answered (asserted by the generator and by a CPU test)"""
    c = dict(transparent_p=0, overflow_first_key=0, overflow_gop_key=0, overflow_forced_key=0, frame_num_wrap=0, key_below_30=0, key_above_30=0,
             refused=0, null_after_key=0, refused_then_null=0)
    for case in cases.values():
        run, seen, prev_refused = 0, 0, False
        w, h = case["create"][:2]
        # SPS + PPS + a slice that is one skip run stay under 40 bytes at these sizes; a coded intra picture has > 1 bit per macroblock
        full = 40 + ((w + 15) // 16) * ((h + 15) // 16) // 8
        eff = _effective(case)
        for i, l in enumerate(case["frames"]):
            if case["sizes"][i] < 0:
                c["refused"] += 1
                prev_refused = True
                continue
            stored, over = eff[i]
            key = case["key"][i]
            run = 0 if key else run + 1
            c["frame_num_wrap"] += run == 32
            if key and stored[3] == stored[4] and 10 <= stored[3] <= 51:
                c["key_below_30"] += stored[3] < 30
                c["key_above_30"] += stored[3] > 30
            if over and not key and case["sizes"][i] <= 16:
                c["transparent_p"] += 1
            if over and key and case["sizes"][i] > full:
                kind = "overflow_first_key" if seen == 0 else "overflow_forced_key" if stored[0] == KEY else "overflow_gop_key"
                c[kind] += 1
            c["null_after_key"] += bool(l[7] and stored[0] == KEY)
            c["refused_then_null"] += bool(l[7] and prev_refused)
            prev_refused = False
            seen += 1
    return c


def check_coverage(cases):
    c = coverage(cases)
    assert all(v > 0 for v in c.values()), c
    return c
