"""Runs for the key frames whose row workgroups a launch dispatches first (h264e_pool.h lead_jobs / order_by_start_step),
shared by tests/test_emu_key_lead.py and tests/test_gpu_key_lead.py: a clip through a ClipEncoder with H264E_KEY_LEAD as given, the
launches' "led K key frames, R rows" read from the H264E_DEBUG lines."""
import re

import key_keep_cases as cases
import launch_lines
import pkg

_LED = re.compile(r"led (\d+) key frames, (\d+) rows; ended by", re.M)


def led_totals(err):
    """(key frames led, their row workgroups) summed over the launch lines of `err`"""
    found = _LED.findall(err)
    return sum(int(k) for k, _ in found), sum(int(r) for _, r in found)


def encode(name, w, h, n, lead=None, lib=None, cap=None, **kw):
    """(stream, sizes, totals) as key_keep_cases.encode, with totals["led_frames"] / ["led_rows"] added.  lead: the value of
    H264E_KEY_LEAD while the clip is opened (None: unset, the default budget)"""
    def go():
        with launch_lines.captured_stderr() as err:
            extra = dict(lib=lib) if lib else {}
            res = cases.encode(pkg.load_pkg(), cases.clip(name, w, h, n), w, h, cap=cap, **extra, **kw)
        return res, err[0]
    (out, sizes, tot), err = cases.with_env({"H264E_DEBUG": "1", "H264E_KEY_LEAD": None if lead is None else str(lead)}, go)
    tot["led_frames"], tot["led_rows"] = led_totals(err)
    return out, sizes, tot


def encode_pair(specs, w, h, lead=None, lib=None):
    """the clips of specs = [(name, frames, stream parameters)] as one launch group (ClipEncoder.encode_multi): ([(stream, sizes, stats)],
    (led frames, led rows))"""
    P = pkg.load_pkg()

    def go():
        encs = []
        try:
            for name, n, kw in specs:
                e = P.ClipEncoder(w, h, n, **(dict(lib=lib) if lib else {}), **kw)
                encs.append(e)
                e.upload(cases.clip(name, w, h, n))
            with launch_lines.captured_stderr() as err:
                res = P.ClipEncoder.encode_multi(encs)
            return [(o, s, dict(spin_relaunches=st.spin_relaunches, kept_key_frames=st.kept_key_frames, kept_key_rows=st.kept_key_rows)) for o, s, st in res], err[0]
        finally:
            for e in encs:
                e.close()
    res, err = cases.with_env({"H264E_DEBUG": "1", "H264E_KEY_LEAD": None if lead is None else str(lead)}, go)
    return res, led_totals(err)
