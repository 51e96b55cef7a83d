"""The per-stage fixtures at the EDGES of every stage's input range, and the decision stages test_stages.py has no case of
(tests/golden/stage_edges.json, made by `oracle/stage_harness.c edges` from the reference's own functions; bit-exact, no tolerances):
  * the existing hooks 1-8: footprints across the picture borders (the reference reads a picture padded by replication, the hooks the
    bare 64x64 picture: the clamped loads ARE the border), reconstructions and normal-strength filter edges whose clip at 0 / 255 acts, 13..16 coefficients,
    escape levels, CAVLC blocks that start mid-word, searches that end on their range and on / just beyond each side of the sub-sample limit, every intra 4x4 mode eight times;
  * new hooks 9-15: intra 16x16 estimate + prediction + cost, chroma prediction, the median vector predictor (get / put over one
    macroblock's partitions), boundary strengths, partition hints, vector cost, the bit writer.
Checked three ways like test_stages.py: the oracle's restatement (CPU), the kernel sources in the lane-loop emulation build (CPU), the
same on the GPU (-m gpu, split by stage group), plus a test that the committed fixture contains what it is for."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib
import pkg
from test_stages import QMODE, _BitW, _hook, _olib, _recon_flow

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "stage_edges.json")))
MV_NA = 0x8000
PARTS = [[(0, 0, 4, 4)], [(0, 0, 4, 2), (0, 2, 4, 2)], [(0, 0, 2, 4), (2, 0, 2, 4)], [(0, 0, 2, 2), (2, 0, 2, 2), (0, 2, 2, 2), (2, 2, 2, 2)]]
PAD = 32


def _b(h):
    """the harness's hex strings, where "(count*xx)" stands for a run of equal bytes"""
    return bytes.fromhex(re.sub(r"\((\d+)\*(..)\)", lambda m: m.group(2) * int(m.group(1)), h))


def _i32(v):
    """a packed vector printed as a signed int -> the 32-bit pattern"""
    return v & 0xffffffff


# ------------------------------------------------------------------ the fixture's compact forms

def _digest(b):
    """64-bit FNV-1a, as the harness prints it for outputs that are compared only as a whole"""
    d = 0xcbf29ce484222325
    for v in b:
        d = ((d ^ v) * 0x100000001b3) & 0xffffffffffffffff
    return "%016x" % d


def _rows(b, stride, w, h):
    return np.frombuffer(b, np.uint8)[: stride * h].reshape(h, stride)[:, :w].tobytes()


def _padded(pic, n, pad=PAD):
    return np.pad(np.frombuffer(pic, np.uint8).reshape(n, n), pad, mode="edge").copy()


def _sad_block(pad, c):
    """the harness's block of a SAD case: the padded picture one sample to the right and two down, low bits stirred"""
    blk = pad[PAD + c["y"] + 2: PAD + c["y"] + 18, PAD + c["x"] + 1: PAD + c["x"] + 17].copy().reshape(256)
    return (blk ^ ((np.arange(256) * 37) & 7).astype(np.uint8)).tobytes()


def _diamond_ref():
    """the harness's 96x96 reference picture of the motion-search cases"""
    y, x = np.mgrid[0:96, 0:96]
    a, b = (x * 4 + y * 2) % 64, (y * 4 - x + 960) % 48
    a, b = np.where(a < 32, a, 63 - a), np.where(b < 24, b, 47 - b)
    return np.minimum(60 + 3 * a + 2 * b + (x * 131 + y * 71) % 5, 255).astype(np.uint8).tobytes()


def _i16_block(b):
    """the harness's input macroblock whose corner / centre-line gradients add up to (dx, dy)"""
    dx, dy = b["dx"], b["dy"]
    x1, y1 = min(dx // 2, 110), min(dy // 2, 110)
    p = (90 + (np.arange(256) * 29 + dx * 7 + dy * 13) % 41).astype(np.uint8)
    p[[0, 15, 240, 255, 128, 143, 8, 248]] = [0, x1, y1, x1 + y1, 0, dx - 2 * x1, 0, dy - 2 * y1]
    return p.tobytes()


def _quant_blocks(c):
    """input, prediction and reconstruction of a quantiser case as 16x16 blocks (the fixture keeps the samples the mode works on)"""
    m = 4 * (c["mode"] >> 1)
    return [_tile(c[k], 16, m, 0).tobytes() for k in ("inp", "pred", "out")]


def _tile(h, n, m, o):
    """m x m samples -> an n x n neighbourhood with them at (o, o): the macroblock with 4 / 2 samples of its left and top neighbours"""
    p = np.zeros((n, n), np.uint8)
    p[o: o + m, o: o + m] = np.frombuffer(_b(h), np.uint8).reshape(m, m)
    return p


def _strength_mv(c):
    return [_i32(v) for v in c.get("mv", [_i32((-4 << 16) | 8)] * 24)] + [0]


def _mv_cost_records():
    f = FIX["mv_cost"]
    px, py = f["pred"]
    d = f["diffs"]
    recs = []
    for qi, qp in enumerate(range(10, 52)):
        for k in range(len(d)):
            recs.append((px + d[(k + qp) % len(d)], py + d[k], px, py, qp, f["cost"][qi][k]))
    return recs


# ------------------------------------------------------------------ the oracle's restatement

def _elib():
    L = _olib()
    L.bw_put.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    L.i4_choose.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.deblock_mb.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int]
    L.bw_ue.argtypes = [C.c_void_p, C.c_uint32]
    L.bw_se.argtypes = [C.c_void_p, C.c_int]
    L.pred_chroma.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    L.h264o_test_mvp.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.h264o_test_strengths.argtypes = [C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p]
    L.h264o_test_partition_hints.argtypes = [C.c_void_p, C.c_void_p]
    L.h264o_test_mv_cost.argtypes = [C.c_int] * 5
    L.h264o_test_intra16.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int)]
    return L


def test_oracle_sad_and_interpolation_across_the_borders():
    """the oracle reads a stored border like the reference: the picture padded by replication"""
    L = oracle_lib.lib()
    f = FIX["border"]
    pad = _padded(_b(f["pic"]), 64)
    s = 64 + 2 * PAD
    org = pad.ctypes.data + PAD * s + PAD
    sad = L.sad_16x16_q
    sad.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    for c in f["sad"]:
        s4 = (C.c_int * 4)()
        assert sad(org + c["y"] * s + c["x"], s, _sad_block(pad, c), 16, s4) == c["sad"] and list(s4) == c["sad4"], (c["x"], c["y"])
    for name, fn, q in (("luma", L.interp_luma, 4), ("chroma", L.interp_chroma, 8)):
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p]
        for c in f[name]:
            dst = C.create_string_buffer(256)
            fn(org, s, q * c["x"] + c["dx"], q * c["y"] + c["dy"], c["w"], c["h"], dst)
            assert _digest(_rows(dst.raw, 16, c["w"], c["h"])) == c["dst"], (name, c)


def test_oracle_quant_cavlc_intra4_deblock_edges():
    L = _elib()
    for c in FIX["quant"]:
        mode = c["mode"]
        nblk = 1 if mode == QMODE["i4"] else (mode >> 1) ** 2
        plane = 1 if mode == QMODE["chroma"] else 0
        qd = np.zeros((2, 42), np.uint16)
        L.build_qdat(qd.ctypes.data, c["qp"], c["p_slice"])
        assert qd[plane].tobytes() == _b(c["qdat"])
        q, dc, lev = np.zeros((16, 32), np.int16), np.zeros(16, np.int16), np.zeros(16, np.int16)
        inp, pred, want = _quant_blocks(c)
        nz = L.xform_quant(inp, 16, pred, mode, q.ctypes.data, dc.ctypes.data, qd[plane].ctypes.data)
        dcflag = 0
        if mode == QMODE["i16"]:
            L.quant_luma_dc(q.ctypes.data, dc.ctypes.data, lev.ctypes.data, qd[plane].ctypes.data)
        if mode == QMODE["chroma"]:
            dcflag = L.quant_chroma_dc(q.ctypes.data, dc.ctypes.data, lev.ctypes.data, qd[plane].ctypes.data)
        assert (nz, dcflag) == (c["nz"], c["dcflag"]) and q[:nblk].tobytes() == _b(c["q"]), (c["what"], mode)
        if mode & 1:
            n = 16 if mode == QMODE["i16"] else 4
            assert dc[:n].tobytes() == _b(c["dc"])[: 2 * n] and lev[:n].tobytes() == _b(c["deq_dc"])[: 2 * n], (c["what"], mode)
        out = C.create_string_buffer(pred, 256)
        _recon_flow(mode, nz, dcflag, q, lambda sd, mask: L.recon_blocks(out, 16, pred, q.ctypes.data, sd, mask))
        assert out.raw == want, (c["what"], mode)
    for c in FIX["cavlc"]:
        buf = C.create_string_buffer(64)
        bw = _BitW()
        L.bw_init(C.byref(bw), buf, 64)
        if c["start"]:
            L.bw_put(C.byref(bw), c["start"], (1 << c["start"]) - 1)
        coef = np.frombuffer(_b(c["coef"]), np.int16).copy()
        nnz = C.create_string_buffer(1)
        L.cavlc_block(C.byref(bw), coef.ctypes.data, 1 if c["maxn"] == 15 else 0, c["maxn"], c["left"] + c["top"], nnz)
        nbits = bw.pos * 8 + bw.nacc
        L.bw_flush(C.byref(bw))
        assert (nnz.raw[0], nbits) == (c["nnz"], c["nbits"]) and buf.raw[: (nbits + 7) // 8] == _b(c["bits"]), c
    for c in FIX["intra4"]:
        e = _b(c["edge"])
        pred = C.create_string_buffer(64)
        sad = C.c_int()
        mode = L.i4_choose(_tile(c["in"], 16, 4, 0).tobytes()[:64], pred, c["avail"], e[5:13], bytes(reversed(e[0:4])), e[4], c["mpred"], c["penalty"], C.byref(sad))
        assert (mode, sad.value) == (c["mode"], c["cost"]) and _rows(pred.raw, 16, 4, 4) == _b(c["pred"]), c
    for c in FIX["deblock"]:
        y, u, v = _tile(c["y_in"], 32, 20, 4), _tile(c["u_in"], 16, 10, 2), _tile(c["v_in"], 16, 10, 2)
        L.deblock_mb(y.ctypes.data + 8 * 32 + 8, 32, u.ctypes.data + 4 * 16 + 4, v.ctypes.data + 4 * 16 + 4, 16, _b(c["bs"]), c["qp"], c["qp_left"], c["qp_top"])
        for got, k, n, m, o in ((y, "y_out", 32, 20, 4), (u, "u_out", 16, 10, 2), (v, "v_out", 16, 10, 2)):
            assert (got == _tile(c[k], n, m, o)).all(), ("deblock", k, c["mb_type"], c["qp"], c["kind"])


def test_oracle_intra16_and_chroma_prediction():
    L = _elib()
    for c in FIX["intra16"]:
        blk = _i16_block(FIX["intra16_blocks"][c["block"]])
        pred = C.create_string_buffer(256)
        cost = C.c_int()
        mode = L.h264o_test_intra16(blk, _b(c["left"]) if c["avail"] & 2 else None, _b(c["top"]) if c["avail"] & 1 else None, c["avail"], c["qp"], pred, C.byref(cost))
        assert (mode, cost.value, _digest(pred.raw)) == (c["mode"], c["cost"], c["pred"]), c
    for c in FIX["pred_chroma"]:
        pred = C.create_string_buffer(128)
        L.pred_chroma(pred, _b(c["left"]) if c["avail"] & 2 else None, _b(c["top"]) if c["avail"] & 1 else None, c["mode"])
        assert pred.raw == _b(c["pred"]), {k: v for k, v in c.items() if k != "pred"}


def test_oracle_vector_predictor_strengths_and_scalars():
    L = _elib()
    for c in FIX["mvp"]:
        ctx = np.array([_i32(v) for v in c["ctx"]], np.uint32)
        parts = np.array(PARTS[c["type"]], np.int32)
        mvs = np.array([_i32(v) for v in c["mv"]], np.uint32)
        preds = np.zeros(len(mvs), np.uint32)
        L.h264o_test_mvp(ctx.ctypes.data, c["avail"], len(mvs), parts.ctypes.data, mvs.ctypes.data, preds.ctypes.data)
        assert list(preds) == [_i32(v) for v in c["pred"]] and list(ctx) == [_i32(v) for v in c["after"]], c
    for c in FIX["strength"]:
        mv = np.array(_strength_mv(c), np.uint32)
        bs = C.create_string_buffer(32)
        L.h264o_test_strengths(c["nz"], mv.ctypes.data, c["type"], c["left"], c["top"], c["x"], c["slice_top"], bs)
        assert bs.raw == _b(c["bs"]), c
    for c in FIX["hints"]:
        sad, mode = np.array(c["sad"], np.int32), np.zeros(4, np.int32)
        L.h264o_test_partition_hints(sad.ctypes.data, mode.ctypes.data)
        assert list(mode) == c["mode"], c
    for vx, vy, px, py, qp, want in _mv_cost_records():
        assert L.h264o_test_mv_cost(vx, vy, px, py, qp) == want, (vx, vy, px, py, qp)


def test_oracle_bit_writer():
    L = _elib()
    for c in FIX["bitwriter"]:
        buf = C.create_string_buffer(64)
        bw = _BitW()
        L.bw_init(C.byref(bw), buf, 64)
        for kind, v, n in c["ops"]:
            if kind == 0:
                L.bw_put(C.byref(bw), n, v)
            elif kind == 1:
                L.bw_ue(C.byref(bw), v)
            else:
                L.bw_se(C.byref(bw), v)
        nbits = bw.pos * 8 + bw.nacc
        L.bw_flush(C.byref(bw))
        assert nbits == c["nbits"] and buf.raw[: (nbits + 7) // 8] == _b(c["bits"]), c


# ------------------------------------------------------------------ the kernel sources' stages (emulation build / GPU)

def _check_borders(run):
    """Stages 1-3 with footprints that leave the picture.  How far the encoder lets one leave: a vector may point 14 samples outside on
    every side (h264e_geom_t lim_*: -14*4 .. (W - 2)*4 for the macroblock's origin), and sub-sample positions exist only 4 samples inside
    that (the quarter-sample limit), where the 6-tap filter adds 2 samples before and 3 after: 14 samples for a full-sample block, 12 / 14
    (10 + the fraction + taps) for an interpolated one; chroma, at half the resolution with one more sample for the bilinear taps, 8.
    Every case stays within that."""
    f = FIX["border"]
    pic = _b(f["pic"])
    pad = _padded(pic, 64)
    for window in (0, 1):
        for c in f["sad"]:
            r = np.frombuffer(run(1, pic + _sad_block(pad, c), [c["x"], c["y"], window], 20), np.int32)
            assert list(r[:4]) == c["sad4"] and r[4] == c["sad"], ("sad", window, c)
        for c in f["luma"]:
            r = run(2, pic, [c["x"], c["y"], c["w"], c["h"], c["dx"], c["dy"], window], 256)
            assert _digest(_rows(r, 16, c["w"], c["h"])) == c["dst"], ("luma", window, c)
    for c in f["chroma"]:
        r = run(3, pic, [c["x"], c["y"], c["w"], c["h"], c["dx"], c["dy"]], 256)
        assert _digest(_rows(r, 16, c["w"], c["h"])) == c["dst"] and _digest(_rows(r[8:] + bytes(8), 16, c["w"], c["h"])) == c["dst"], ("chroma", c)


def _check_coding(run):
    for c in FIX["quant"]:
        mode = c["mode"]
        nblk = 1 if mode == QMODE["i4"] else (mode >> 1) ** 2
        inp, pred, want = _quant_blocks(c)
        r = run(4, inp + pred + _b(c["qdat"]), [mode], 8 + 1024 + 32 + 32 + 256)
        assert tuple(np.frombuffer(r[:8], np.int32)) == (c["nz"], c["dcflag"]) and r[8: 8 + 64 * nblk] == _b(c["q"]), ("quant levels", c["what"], mode)
        if mode & 1:
            n = 16 if mode == QMODE["i16"] else 4
            assert r[1064: 1064 + 2 * n] == _b(c["deq_dc"])[: 2 * n], ("quant dc levels", c["what"], mode)
        assert r[1096: 1096 + 256] == want, ("reconstruction", c["what"], mode)
    for c in FIX["cavlc"]:
        r = run(5, _b(c["coef"]), [1 if c["maxn"] == 15 else 0, c["maxn"], c["left"] + c["top"], c["start"]], 8 + 64)
        words = np.frombuffer(r[8:72], "<u4").astype(">u4").tobytes()      # the kernel's bit buffer is MSB-first 32-bit words
        assert tuple(np.frombuffer(r[:8], np.int32)) == (c["nnz"], c["nbits"]) and words[: (c["nbits"] + 7) // 8] == _b(c["bits"]), ("cavlc", c)
    for c in FIX["bitwriter"]:
        ops = np.array([[k, _i32(v), n] for k, v, n in c["ops"]], np.uint32)
        r = run(15, ops.tobytes(), [len(c["ops"])], 8 + 64)
        nbits, overflow = np.frombuffer(r[:8], np.int32)
        words = np.frombuffer(r[8:72], "<u4").astype(">u4").tobytes()
        assert (nbits, overflow) == (c["nbits"], 0) and words[: (nbits + 7) // 8] == _b(c["bits"]), ("bit writer", c)


def _check_decisions(run):
    for c in FIX["intra4"]:
        r = run(6, _b(c["edge"]) + bytes(3) + _tile(c["in"], 16, 4, 0).tobytes()[:64], [c["avail"], c["mpred"], c["penalty"]], 8 + 64)
        assert tuple(np.frombuffer(r[:8], np.int32)) == (c["mode"], c["cost"]) and _rows(r[8:72], 16, 4, 4) == _b(c["pred"]), ("intra4", c)
    for c in FIX["intra16"]:
        blk = _i16_block(FIX["intra16_blocks"][c["block"]])
        r = run(9, blk + _b(c["left"]) + _b(c["top"]), [c["avail"], c["qp"]], 8 + 256)
        mode, cost = np.frombuffer(r[:8], np.int32)
        assert (mode, cost, _digest(r[8:264])) == (c["mode"], c["cost"], c["pred"]), ("intra16", c)
    for c in FIX["pred_chroma"]:
        r = run(10, _b(c["left"]) + _b(c["top"]), [c["avail"], c["mode"]], 128)
        assert r == _b(c["pred"]), ("chroma prediction", {k: v for k, v in c.items() if k != "pred"})
    for c in FIX["mvp"]:
        ctx = [_i32(v) for v in c["ctx"]] + [0, 0, 0]
        ops = [w for p, v in zip(PARTS[c["type"]], c["mv"]) for w in (p[0], p[1], p[2], p[3], _i32(v))]
        r = np.frombuffer(run(11, np.array(ctx + ops, np.uint32).tobytes(), [c["avail"], len(c["mv"])], 128), np.uint32)
        assert list(r[: len(c["mv"])]) == [_i32(v) for v in c["pred"]], ("vector predictor", c)
        assert list(r[16:29]) == [_i32(v) for v in c["after"]], ("vector predictor context", c)
    for c in FIX["strength"]:
        r = run(12, np.array(_strength_mv(c), np.uint32).tobytes(), [c["nz"], c["left"], c["top"], c["type"], c["x"], c["slice_top"]], 32)
        assert r == _b(c["bs"]), ("strengths", c)
    h = FIX["hints"]
    for i in range(0, len(h), 64):
        part = h[i: i + 64]
        r = np.frombuffer(run(13, np.array([c["sad"] for c in part], np.int32).tobytes(), [len(part)], 16 * len(part)), np.int32).reshape(-1, 4)
        for c, got in zip(part, r):
            assert list(got) == c["mode"], ("partition hints", c)
    recs = _mv_cost_records()
    for i in range(0, len(recs), 256):
        part = recs[i: i + 256]
        r = np.frombuffer(run(14, np.array([p[:5] for p in part], np.int32).tobytes(), [len(part)], 4 * len(part)), np.int32)
        for p, got in zip(part, r):
            assert got == p[5], ("vector cost", p)


def _check_search_and_filter(run):
    ref = _diamond_ref()
    for window in (0, 1):
        for ci, c in enumerate(FIX["diamond"]):
            # args[20]: which 16-lane group of the wave runs the search
            args = [c["px"], c["py"], c["w"], c["h"]] + c["mv_in"] + c["mv_pred"] + [c["min_sad_in"], c["qp"], c["speed"]] + c["range"] + c["limit"] + [window, ci % 4]
            r = run(8, ref + _b(c["cur"]), args, 16 + 256)
            cost, mx, my = np.frombuffer(r[:12], np.int32)
            info = {k: v for k, v in c.items() if k not in ("cur", "pred")}
            assert (cost, [mx, my]) == (c["cost"], c["mv"]), ("motion search", window, info)
            assert _rows(r[16 + 16 * c["py"] + c["px"]: 272] + bytes(256), 16, c["w"], c["h"]) == _b(c["pred"]), ("motion search prediction", window, info)
    for c in FIX["deblock"]:
        # the kernel filters on its LDS tiles: the macroblock with 4 (luma) / 2 (chroma) samples of its left and top neighbours, row strides 24 / 12
        tiles = [np.zeros((20, 24), np.uint8), np.zeros((10, 12), np.uint8), np.zeros((10, 12), np.uint8)]
        for t, k in zip(tiles, ("y_in", "u_in", "v_in")):
            m = t.shape[0]
            t[:, :m] = np.frombuffer(_b(c[k]), np.uint8).reshape(m, m)
        r = run(7, b"".join(t.tobytes() for t in tiles) + _b(c["bs"]), [c["qp"], c["qp_left"], c["qp_top"]], 480 + 240)
        for got, k, stride, m in ((r[:480], "y_out", 24, 20), (r[480:600], "u_out", 12, 10), (r[600:720], "v_out", 12, 10)):
            assert _rows(got, stride, m, m) == _b(c[k]), ("deblock", k, c["mb_type"], c["qp"], c["kind"])


GROUPS = [_check_borders, _check_coding, _check_decisions, _check_search_and_filter]


def test_emulated_kernel_stages_match_reference_functions_at_the_edges():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    run, close = _hook(pkg.EMU_LIB)
    try:
        for g in GROUPS:
            g(run)
    finally:
        close()


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS, ids=lambda g: g.__name__[7:])
def test_gpu_kernel_stages_match_reference_functions_at_the_edges(group):
    run, close = _hook(None)
    try:
        group(run)
    finally:
        close()


# ------------------------------------------------------------------ the fixture contains what it is for

def test_edge_fixture_contains_what_it_is_for():
    """Asserted on the committed JSON, so that a regenerated fixture cannot quietly lose a case.  (All conditions of the issue are
    reachable by the reference; none had to be dropped.)"""
    for mode in QMODE.values():
        outs = b"".join(_b(c["out"]) for c in FIX["quant"] if c["mode"] == mode)
        assert 0 in outs and 255 in outs, mode
    assert {c["what"] for c in FIX["quant"]} == {"+255 qp10", "+255 qp51", "-255 qp10", "-255 qp51", "zero", "single +-1", "dc only", "near the range qp22", "near the range qp40"}
    for mode in QMODE.values():
        assert len([c for c in FIX["quant"] if c["mode"] == mode]) == 9, mode
        m = 4 * (mode >> 1)
        for c in FIX["quant"]:
            if c["mode"] == mode and c["what"].startswith("near"):
                # predictions near 0 and near 255 in every 4x4 block, reconstructions that reach both ends of the range
                pr = np.frombuffer(_b(c["pred"]), np.uint8).reshape(m, m)
                assert all(pr[y: y + 4, x: x + 4].min() < 6 and pr[y: y + 4, x: x + 4].max() >= 250 for y in range(0, m, 4) for x in range(0, m, 4)), (mode, c["what"])
                assert 0 in _b(c["out"]) and 255 in _b(c["out"]), (mode, c["what"])
    # deblocking: normal-strength edges where the clip at 0 / 255 ACTS.  A normal filter moves p0 by +delta and q0 by -delta; where the
    # reference moved one of them and left the other, which sat on the end of the range, the other's value left 0..255 and was clipped.
    # All four (p0 / q0 clipped, at 0 / at 255) in luma (tile column 3 | 4 is the macroblock's left edge) and in chroma (column 1 | 2).
    for keys, e in ((("y",), 4), (("u", "v"), 2)):
        seen = set()
        for c in FIX["deblock"]:
            for k in keys:
                n = 20 if k == "y" else 10
                a, b = (np.frombuffer(_b(c["%s_%s" % (k, io)]), np.uint8).reshape(n, n).astype(int) for io in ("in", "out"))
                for y in range(n):
                    p0, q0, dp, dq = a[y, e - 1], a[y, e], b[y, e - 1] - a[y, e - 1], b[y, e] - a[y, e]
                    if p0 == q0 and p0 in (0, 255) and {dp, dq} == {0, 1 if p0 == 0 else -1} and _b(c["bs"])[0] in (1, 2, 3):
                        seen.add(("q0" if dq == 0 else "p0", p0))
        assert seen == {("p0", 0), ("q0", 0), ("p0", 255), ("q0", 255)}, (keys, seen)
    assert {13, 14, 15, 16} <= {c["nnz"] for c in FIX["cavlc"] if c["maxn"] == 16} and {13, 14, 15} <= {c["nnz"] for c in FIX["cavlc"] if c["maxn"] == 15}
    assert {c["start"] for c in FIX["cavlc"]} == set(range(32))
    big = max(abs(int(v)) for c in FIX["cavlc"] for v in np.frombuffer(_b(c["coef"]), np.int16))
    assert big == FIX["quant_max_level"] >= 1000          # the largest level of the QP 10 / +-255 quantiser cases
    assert {c["left"] + c["top"] for c in FIX["cavlc"] if c["maxn"] != 4} >= {0, 5, 11, 21}      # nC 0, 3, 6, 11: the four tables

    def on_edge(c):
        return c["mv"][0] in (c["range"][0], c["range"][2]) or c["mv"][1] in (c["range"][1], c["range"][3])
    assert sum(on_edge(c) for c in FIX["diamond"]) >= 8
    # per side of the sub-sample limit (the vector limit 16 quarter-samples in): a full-sample result exactly on it whose sub-sample probes
    # changed the result, and one a sample beyond it that was left alone
    for side in range(4):
        for beyond in (0, 1):
            cs = [c for c in FIX["diamond"] if (c["qside"], c["qbeyond"]) == (side, beyond)]
            assert cs, (side, beyond)
            for c in cs:
                low = side in (0, 2)            # sides: x0, x1, y0, y1; limit = [x0, y0, x1, y1]
                lim = c["limit"][(0, 2, 1, 3)[side]] + (16 if low else -16)
                assert c["fs_mv"][side >> 1] == lim + (0 if not beyond else -4 if low else 4) and (c["mv"] == c["fs_mv"]) == bool(beyond), c["limit"]
    assert {(c["px"], c["py"], c["w"], c["h"]) for c in FIX["diamond"] if on_edge(c)} >= {(4 * x, 4 * y, 4 * w, 4 * h) for t in PARTS for x, y, w, h in t}
    assert any(c["mv_in"][0] in (c["limit"][0], c["limit"][2]) and c["mv_in"][1] in (c["limit"][1], c["limit"][3]) for c in FIX["diamond"])
    for mode in range(9):
        assert sum(c["mode"] == mode for c in FIX["intra4"]) >= 8, mode
    edges4 = b"".join(_b(c["edge"]) for c in FIX["intra4"])
    assert 0 in edges4 and 255 in edges4
    assert {c["avail"] for c in FIX["mvp"]} == set(range(16)) and {c["type"] for c in FIX["mvp"]} == {0, 1, 2, 3}
    assert any(MV_NA in [_i32(v) for v in c["ctx"]] for c in FIX["mvp"])
    assert set(b"".join(_b(c["bs"]) for c in FIX["strength"])) == {0, 1, 2, 3, 4}
    assert {c["diff"] for c in FIX["strength"]} >= {3, 4} and any(c["x"] == 0 for c in FIX["strength"]) and any(c["slice_top"] for c in FIX["strength"])
    assert {c["nz"] for c in FIX["strength"]} >= {1 << k for k in range(25)}
    assert {(c["mode"], c["avail"] & 3) for c in FIX["pred_chroma"]} >= {(0, 1), (1, 2), (2, 0), (2, 1), (2, 2), (2, 3)}
    assert {c["mode"] for c in FIX["intra16"]} == {0, 1, 2} and {c["avail"] & 3 for c in FIX["intra16"]} == {0, 1, 2, 3} and {c["qp"] for c in FIX["intra16"]} == {10, 26, 51}
    b = FIX["intra16_blocks"]
    for qp in (10, 26, 51):
        for d in (-1, 0, 1):
            assert any((x["dx"], x["dy"]) == (30 + 3 * 6 + d, 6) for x in b) and any((x["dy"], x["dx"]) == (30 + 3 * 6 + d, 6) for x in b)
            assert any(x["dy"] == 150 - qp + d and x["dx"] > 30 + 3 * x["dy"] for x in b) and any(x["dx"] == 150 - qp + d and x["dy"] > 30 + 3 * x["dx"] for x in b)
    assert {n for c in FIX["bitwriter"] for k, v, n in c["ops"][:1] if k == 0} >= set(range(1, 32))
    for op in ([2, 0, 0], [2, 1, 0], [2, -1, 0], [1, 0, 0]):
        assert sum(op in c["ops"] for c in FIX["bitwriter"]) >= 6, op          # se(0) is the mb_qp_delta of every coded macroblock
    # border cases on all four sides, and loads on both sides of both path boundaries of ref_load4 (x >= 0; x + 7 < width): the
    # full-sample 16x16 cases load four samples at x, x + 4, x + 8, x + 12
    for name in ("sad", "luma", "chroma"):
        cs = FIX["border"][name]
        w = lambda c: c.get("w", 16)
        h = lambda c: c.get("h", 16)
        assert any(c["x"] < 0 for c in cs) and any(c["x"] + w(c) > 64 for c in cs) and any(c["y"] < 0 for c in cs) and any(c["y"] + h(c) > 64 for c in cs), name
        assert any(c["x"] < 0 and c["y"] < 0 for c in cs) and any(c["x"] + w(c) > 64 and c["y"] + h(c) > 64 for c in cs), name
    loads = {c["x"] + 4 * k for c in FIX["border"]["sad"] for k in range(4)} | {c["x"] + 4 * k for c in FIX["border"]["luma"] if (c["w"], c["dx"], c["dy"]) == (16, 0, 0) for k in range(4)}
    assert loads >= {-1, 0, 56, 57, 58}         # x + 7 = 63, 64, 65 at a width of 64
    assert {(c["dx"], c["dy"]) for c in FIX["border"]["luma"] if c["w"] == c["h"] == 16 and (c["x"] < 0 or c["x"] > 48 or c["y"] < 0 or c["y"] > 48)} == {(x, y) for x in range(4) for y in range(4)}
    assert os.path.getsize(os.path.join(HERE, "golden", "stage_edges.json")) <= os.path.getsize(os.path.join(HERE, "golden", "stages.json"))
