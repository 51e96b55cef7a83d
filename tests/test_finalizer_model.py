"""CPU: the plain models of tests/finalizer_model.py themselves -- hand-written slices, the mv_clusters step and rounding against the
reference's own functions (tests/golden/finalizer.json), and the two ways of writing a slice against each other."""
import json
import os
import random

import finalizer_model as M
from finalizer_model import Bits

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "finalizer.json")))


def _s(b):
    return format(b.v, "0%db" % b.n) if b.n else ""


def _b(s):
    return Bits(int(s, 2), len(s)) if s else Bits()


def test_exp_golomb_codes():
    assert [_s(M.ue(v)) for v in (0, 1, 2, 3, 6, 7)] == ["1", "010", "011", "00100", "00111", "0001000"]
    for k in range(1, 12):
        # the length steps from 2k - 1 to 2k + 1 bits between 2^k - 2 and 2^k - 1
        assert (M.ue((1 << k) - 2).n, M.ue((1 << k) - 1).n) == (2 * k - 1, 2 * k + 1)


def test_slice_writer_on_hand_written_slices():
    p = [(1, Bits()), (0, _b("1100")), (1, Bits()), (1, Bits())]
    bits, run = M.slice_bits(0, 0x41, 0, _b("101"), p)
    assert (_s(bits), run) == ("01000001" "1" "101" "010" "1100" "011", 2)
    assert M.slice_rbsp(0, 0x41, 0, _b("101"), p) == (bytes([0x41, 0b11010101, 0b10001110]), 2)          # + stop bit, then 0 to the byte
    # an I slice writes no runs; first_mb_in_slice 5 = 00110
    assert _s(M.slice_bits(2, 0x65, 5, Bits(), [(0, _b("0")), (0, _b("11"))])[0]) == "01100101" "00110" "0" "11"
    # everything skipped: header, ue(count), stop bit
    assert M.slice_rbsp(0, 0x41, 0, Bits(), [(1, Bits())] * 4) == (bytes([0x41, 0b10010110]), 4)
    # a stop bit that lands on a byte boundary adds no byte of its own
    assert M.slice_rbsp(2, 0x65, 0, _b("000000"), [(0, Bits())]) == (bytes([0x65, 0b10000001]), 0)


def test_frame_layout_on_a_hand_written_frame():
    mbs = [(0, _b("1" * 9)), (1, Bits())] * 2                                # two rows of two macroblocks, one slice each
    f = M.frame(2, 0, 0x41, Bits(), [0, 1, 2], mbs, 0, 37, 80, 8, far_reads=[3, 4])
    s0 = bytes([0x41, 0b11111111, 0b11101010])                               # 1 | ue(0) | nine ones | ue(1) = 010 | stop
    s1 = bytes([0x41, 0b01111111, 0b11111010, 0b10000000])                   # ue(2) = 011 | ue(0) | nine ones | 010 | stop
    assert (f["start"], f["nbytes"], f["slice_nbytes"], f["overflow"], f["all_skipped"], f["far_reads"]) == (48, 20, [3, 4], 0, 0, 7)
    a = bytes([M.SENTINEL])
    assert f["arena"] == a * 48 + s0 + b"\0" + a * 12 + s1 + a * (88 - 68)
    # one word short: the second slice's word is not written, nothing else changes
    g = M.frame(2, 0, 0x41, Bits(), [0, 1, 2], mbs, 0, 37, 67, 8)
    assert g["overflow"] == 1 and g["arena"] == a * 48 + s0 + b"\0" + a * (75 - 52) and g["nbytes"] == 20
    assert M.frame(1, 0, 0x41, Bits(), [0, 3], [(1, Bits())] * 3, 1, 99, 16, 0)["all_skipped"] == 1
    assert M.frame(1, 0, 0x41, Bits(), [0, 1, 3], [(1, Bits())] * 3, 1, 99, 64, 0)["all_skipped"] == 0


def test_rows_joined_equal_the_serial_slice():
    rng = random.Random(7)
    for _ in range(300):
        nmbx, nrows, st = rng.choice((1, 2, 5)), rng.randint(1, 6), rng.choice((0, 0, 2))
        mbs = []
        for _ in range(nmbx * nrows):
            n = rng.choice((0, 1, 7, 31, 32, 33, 70))
            mbs.append((0, Bits(rng.getrandbits(n), n)) if st == 2 or rng.random() < 0.4 else (1, Bits()))
        rows = [M.row_wave(st, mbs[r * nmbx: (r + 1) * nmbx]) for r in range(nrows)]
        hdr = Bits(rng.getrandbits(11), 11)
        assert M.rows_joined(nmbx, st, 0x41, 3 * nmbx, hdr, rows) == M.slice_rbsp(st, 0x41, 3 * nmbx, hdr, mbs)


def test_step_and_rounding_are_the_references():
    for v, rx, ry in FIX["round"]:
        assert M.rnd((v, -v)) == (rx, ry)
    for r in FIX["steps"]:
        assert M.step((r[0], r[1]), (r[2], r[3]), (r[4], r[5])) == ((r[6], r[7]), (r[8], r[9])), r
    for q in FIX["sequences"]:
        st = q["steps"]
        rec = [((r[4], r[5]), 0, 0) for r in st]
        start = ((st[0][0], st[0][1]), (st[0][2], st[0][3]))
        fb, end, traj = M.walk(rec, len(rec), [0, 1], start, start, 0)
        assert fb == -1 and traj == [((r[0], r[1]), (r[2], r[3])) for r in st]
        assert end == ((q["end"][0], q["end"][1]), (q["end"][2], q["end"][3]))


def test_pack_unpack_and_walk_rules():
    for p in ((0, 0), (-1, 1), (32767, -32768), (-2048, 2047)):
        assert M.unpack(M.pack(p)) == p
    z = ((0, 0), (0, 0))
    big = (2048, 0)
    # the check sees the state in front of the macroblock: a mover that consumed the right candidates is no mismatch, the next consumer is
    rec = [(big, 0, 1), ((0, 0), 0, 0), ((0, 0), 0, 1), ((0, 0), 0, 1)]
    fb, end, traj = M.walk(rec, 4, [0, 1], z, z, 0)
    assert fb == 2 and traj[0] == z and traj[1] == ((0, 0), (32, 0)) and end != z
    # intra macroblocks are checked but do not update; every slice restarts and the parent's state stays
    assert M.walk([(big, 5, 1), ((0, 0), 0, 1)], 2, [0, 1], z, z, 0)[:2] == (-1, z)
    fb, end, traj = M.walk(rec, 1, [0, 2, 4], z, z, 0)
    assert (fb, end, traj[2]) == (-1, z, z)
    assert M.moved(rec, z) == 1 and M.moved(rec[1:], z) == 0 and M.moved([(big, 5, 1)], z) == 0
