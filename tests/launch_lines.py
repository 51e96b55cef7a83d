"""The streaming clip encoder's H264E_DEBUG lines (h264e_host.c clip_debug_line, clip_take_frame), parsed from captured stderr: one
"clip launch" line per launch, one "clip frame" line per delivered frame."""
import collections
import contextlib
import os
import re
import sys
import tempfile

Launch = collections.namedtuple("Launch", "first_row geometry frames_in_flight valid ended_by far_reads hedged index")

_LAUNCH = re.compile(r"clip launch (\d+) \(first row (\d+), (narrow|wide) window, (-?\d+) far reads\): (\d+) frames in flight, (\d+) valid, "
                     r"next \d+;.*?; ended by: (.*?)( \(\+ hedge leaves\))?$", re.M)
_FRAME = re.compile(r"^clip frame (\d+): (-?\d+) far reads$", re.M)


def parse(err):
    """the launches of `err` in order; the first five fields are (first_row, geometry, frames_in_flight, valid, ended_by), then the
    far reads of the frames it delivered, whether it carried hedge leaves, and its number within the encode call"""
    return [Launch(int(m[2]), m[3], int(m[5]), int(m[6]), m[7], int(m[4]), bool(m[8]), int(m[1])) for m in _LAUNCH.finditer(err)]


def frame_far_reads(err):
    """{frame: far reads} of the delivered frames"""
    return {int(f): int(v) for f, v in _FRAME.findall(err)}


def geometries(launches):
    """the launches' geometries as a string, "n" / "w" per launch"""
    return "".join(l.geometry[0] for l in launches)


@contextlib.contextmanager
def captured_stderr():
    """what the library writes to file descriptor 2 inside the block, as text in the list that is yielded (pytest's capfd belongs to one
    test; this serves encodes that several tests share)"""
    got = []
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            yield got
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            f.seek(0)
            got.append(f.read().decode())
