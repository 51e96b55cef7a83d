"""Plain models of what the frame finalizer computes (h264-lab_amd/csrc/enc_finalize.h, "slice splice"), for tests/test_finalizer.py:
  * the slice writer, macroblock-serial as the reference writes a slice (h264-lab.h:4247 header, 6451-6456 / 3999 tail), on Python integers
    used as bit strings -- no rows, no words, no carries;
  * what a row wave leaves behind for the finalizer (h264e_rowmeta_t + the row's bits), built from the same per-macroblock bits;
  * the straight mv_clusters walk (h264e_host.c clusters_walk) with its step and rounding written on (x, y) tuples.
Nothing here shares code with the kernels, the host or the oracle."""

SENTINEL = 0xA5


# ------------------------------------------------------------------ bit strings

class Bits:
    """a bit string: the integer `v` written MSB first in `n` bits"""

    def __init__(self, v=0, n=0):
        assert 0 <= v < (1 << n) or (n == 0 and v == 0)
        self.v, self.n = v, n

    def __add__(self, o):
        return Bits((self.v << o.n) | o.v, self.n + o.n)

    def __eq__(self, o):
        return (self.v, self.n) == (o.v, o.n)

    def bytes(self, multiple=1):
        """zero-padded at the end to a multiple of `multiple` bytes"""
        nb = -(-self.n // (8 * multiple)) * multiple
        return (self.v << (8 * nb - self.n)).to_bytes(nb, "big") if nb else b""


def ue(v):
    """Exp-Golomb: v + 1 in binary behind as many zeros as it has bits after the first"""
    n = (v + 1).bit_length()
    return Bits(v + 1, 2 * n - 1)


# ------------------------------------------------------------------ the slice, macroblock by macroblock

def slice_bits(slice_type, hdr_nal, first_mb, hdr, mbs):
    """mbs: (skipped, Bits) per macroblock in raster order.  Returns (the RBSP's bits in front of the stop bit, the final run)."""
    out = Bits(hdr_nal, 8) + ue(first_mb) + hdr
    run = 0
    for skipped, bits in mbs:
        if skipped:
            assert slice_type != 2
            run += 1
        else:
            if slice_type != 2:
                out = out + ue(run)
            out = out + bits
            run = 0
    if run:
        out = out + ue(run)
    return out, run


def slice_rbsp(slice_type, hdr_nal, first_mb, hdr, mbs):
    bits, run = slice_bits(slice_type, hdr_nal, first_mb, hdr, mbs)
    return (bits + Bits(1, 1)).bytes(), run


def frame(nmbx, slice_type, hdr_nal, hdr, slice_row, mbs, arena_reset, cursor, cap, guard, row_overflow=(), far_reads=()):
    """The finalizer's result for one frame: every slice's RBSP at a 16-byte aligned offset behind `start`, whole 32-bit words written
    while they fit the capacity, the sentinel everywhere else."""
    nslices = len(slice_row) - 1
    start = 0 if arena_reset else (cursor + 15) & ~15
    arena = bytearray([SENTINEL]) * (cap + guard)
    off, overflow, sizes, run = 0, 0, [], 0
    for k in range(nslices):
        m0, m1 = slice_row[k] * nmbx, slice_row[k + 1] * nmbx
        rbsp, run = slice_rbsp(slice_type, hdr_nal, m0, hdr, mbs[m0:m1])
        words = rbsp + bytes(-len(rbsp) % 4)
        room = max(cap - (start + off), 0) // 4 * 4
        fit = min(len(words), room)
        arena[start + off: start + off + fit] = words[:fit]
        overflow |= len(words) > room
        sizes.append(len(rbsp))
        off += (len(rbsp) + 15) & ~15 if k + 1 < nslices else len(rbsp)
    return {"start": start, "nbytes": off, "overflow": int(bool(overflow or row_overflow)), "all_skipped": int(nslices == 1 and run == len(mbs)),
            "far_reads": sum(far_reads), "slice_nbytes": sizes, "arena": bytes(arena)}


# ------------------------------------------------------------------ what the row waves leave

def row_wave(slice_type, mbs_row):
    """One macroblock row as its wave leaves it: (lead_skips, trail_skips, Bits).  The run in front of the row's first coded macroblock
    and the one behind its last are left to the finalizer; the runs between coded macroblocks are in the row's bits."""
    coded = [i for i, (skipped, _) in enumerate(mbs_row) if not skipped]
    if not coded:
        return len(mbs_row), 0, Bits()
    bits, last = Bits(), None
    for i in coded:
        if last is not None and slice_type != 2:
            bits = bits + ue(i - last - 1)
        bits = bits + mbs_row[i][1]
        last = i
    return coded[0], len(mbs_row) - 1 - coded[-1], bits


def rows_joined(nmbx, slice_type, hdr_nal, first_mb, hdr, rows):
    """a slice from row_wave() results at bit level: the rule the finalizer follows, without its words and carries"""
    out = Bits(hdr_nal, 8) + ue(first_mb) + hdr
    run = 0
    for lead, trail, bits in rows:
        run += lead
        if lead < nmbx or bits.n:
            if slice_type != 2:
                out = out + ue(run)
            out = out + bits
            run = trail
    if run:
        out = out + ue(run)
    return (out + Bits(1, 1)).bytes(), run


# ------------------------------------------------------------------ mv_clusters

def s16(v):
    v &= 0xffff
    return v - 0x10000 if v & 0x8000 else v


def pack(p):
    """(x, y) -> the packed vector's 32-bit pattern"""
    return ((p[1] & 0xffff) << 16) | (p[0] & 0xffff)


def unpack(v):
    return s16(v), s16(v >> 16)


def rnd(p):
    """quarter-sample vector -> full sample (h264-lab.h:3498)"""
    return ((p[0] + 1) & ~3, (p[1] + 1) & ~3)


def step(c0, c1, mv):
    """the update of the short / long cluster means by one vector (h264-lab.h:5263-5278)"""
    def norm(p):
        return p[0] * p[0] + p[1] * p[1]

    def smooth(c):
        return (s16((63 * c[0] + mv[0] + 32) >> 6), s16((63 * c[1] + mv[1] + 32) >> 6))
    n, n0, n1 = norm(mv), norm(c0), norm(c1)
    return (smooth(c0) if n < n1 else c0), (smooth(c1) if n >= n0 else c1)


def walk(rec, nmbx, slice_row, start, used, per_mb):
    """rec: (mv, type, used_cand) per macroblock; used: one (c0, c1) pair, or one per macroblock.  Every slice starts from `start`; a
    macroblock's consumed candidates are compared (rounded) with the state in front of it, then its vector updates the state; the walk
    goes on behind the first mismatch.  Returns (first_bad, end state, the state in front of every macroblock)."""
    first_bad, traj = -1, []
    nslices = len(slice_row) - 1
    c = start
    for k in range(nslices):
        c = start
        for i in range(slice_row[k] * nmbx, slice_row[k + 1] * nmbx):
            mv, typ, used_cand = rec[i]
            u = used[i] if per_mb else used
            traj.append(c)
            if used_cand and first_bad < 0 and (rnd(u[0]) != rnd(c[0]) or rnd(u[1]) != rnd(c[1])):
                first_bad = i
            if typ < 5:
                c = step(c[0], c[1], mv)
    return first_bad, (start if nslices > 1 else c), traj


def moved(rec, pair):
    """some macroblock's update changes the frame's candidate pair"""
    return int(any(typ < 5 and step(pair[0], pair[1], mv) != (pair[0], pair[1]) for mv, typ, _ in rec))
