#!/usr/bin/env python3
"""Regenerate tests/golden/lookahead_off.json: cost records, QPs, frame sizes and the stream's md5 of one lookahead-controlled clip
WITHOUT the cost pass' motion search, as an encoder library writes them.  The committed file was recorded with the emulation library
of the commit BEFORE the search existed (this script copied into a checkout of that commit and run there, after `make -C tests/emu`,
with its libh264e_emu.so): it pins that search 0, the default, keeps every record and every byte (tests/test_gpu_lookahead_motion.py).

    python tests/golden/make_golden_lookahead_off.py /path/to/libh264e_emu.so
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import clips  # noqa: E402
import pkg  # noqa: E402

CASE = dict(clip="synth", w=176, h=144, frames=24, gop=8, window=4, kbps=120)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    P = pkg.load_pkg()
    g = dict(CASE)
    c = clips.make(g["clip"], g["w"], g["h"], g["frames"])
    ce = P.ClipEncoder(g["w"], g["h"], g["frames"], lib=sys.argv[1], gop=g["gop"], qp=30, abr_kbps=g["kbps"], lookahead=g["window"])
    ce.upload(c)
    out, sizes, _ = ce.encode()
    (i, p, n), qp = ce.read_lookahead()
    ce.close()
    g.update(input_md5=hashlib.md5(c.tobytes()).hexdigest(), intra=i.tolist(), inter=p.tolist(), intra_blocks=n.tolist(), qp=qp.tolist(),
             frame_bytes=sizes, md5=hashlib.md5(out).hexdigest())
    with open(os.path.join(HERE, "lookahead_off.json"), "w") as f:
        f.write(json.dumps(g, sort_keys=True) + "\n")
    print(g["md5"], sum(sizes), "bytes, QPs", sorted(set(g["qp"])))


if __name__ == "__main__":
    main()
