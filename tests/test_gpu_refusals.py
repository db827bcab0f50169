"""The refusal table of the batch entry points: what each call returns, and what cimbar_hip_last_error then says, for arguments it must
refuse -- and in which order the checks run where a call breaks two rules at once. Every expected code and text below is a literal copied
from the source the table was written against; nothing here is produced by the code under test. Every row but the four flushes is refused
before anything is enqueued, so the file needs one mode-68 and one mode-4 context and no decode work."""
import ctypes

import numpy as np
import pytest

from libcimbar_amd import decoder as D

pytestmark = pytest.mark.gpu

EINVAL, EDIM = -1, -2
H, BAD = D.MEM_HOST, 7
NV21 = 21
MEM = " must be CIMBAR_HIP_MEM_HOST or CIMBAR_HIP_MEM_DEVICE"
NULLN = ": null buffer or n <= 0"
SMALL = ": null buffer, n <= 0 or a capture smaller than 8x8"
DIMS = ": a 4:2:0 capture (format 12 / 21 / 420) needs an even width and height, a 4:2:2 capture (format 422 / 4221) an even width"
LEGACY = ": modes 4 and 8 are not covered; the ink signature was checked on the palettes of modes 68 / 67 / 66"

# argument lists in the order of include/cimbar_hip.h, the context left out. "F" = one 1024x1024 zero frame, "C" = one capture buffer,
# "P" = scratch that a refused call never touches, "G" = room for one group slot (what a flush writes)
FRAME = [("rgb", "F"), ("n", 1), ("rgb_mem", H), ("pre", 0), ("cc", 2)]
CAPTURE = [("img", "C"), ("w", 8), ("h", 8), ("format", 3), ("n", 1), ("img_mem", H)]
OUT = [("chunks", "P"), ("masks", "P")]
END = [("out_mem", H), ("stream", None)]
COMBINE = [("groups_in", None), ("min_agree", 0), ("max_group", 0)]
COMBINE_OUT = [("groups_out", None), ("gchunks", "G"), ("gmasks", "G"), ("n_groups", None)]
STREAM = [("min_agree", 0), ("max_group", 0), ("flush", 0)]
STREAM_OUT = [("groups_out", None), ("gchunks", "G"), ("gmasks", "G"), ("gsizes", "G"), ("n_groups", None)]
STITCH = [("axis", 0), ("min_agree", 0), ("min_band", 0)]
STITCH_OUT = [("schunks", "P"), ("smasks", "P"), ("tears", None)]
ONCE = [("min_agree", 0), ("max_run", 0)]
ONCE_OUT = [("runs_out", None), ("roles", None), ("rchunks", None), ("rmasks", None), ("n_runs", None)]
PRE = [("pre", 0), ("cc", 2)]
STATUS = [("status", None)]

# name -> (arguments, who, the null / n text, the flag names of the mem text, input, its flag, first output, its flag)
FRAME_CALLS = {
    "decode_batch": FRAME + OUT + END,
    "decode_batch_combined": FRAME + COMBINE + OUT + COMBINE_OUT + END,
    "decode_batch_combined_stream": FRAME + STREAM + OUT + STREAM_OUT + END,
    "decode_batch_stitched": FRAME + STITCH + OUT + STITCH_OUT + END,
    "decode_batch_stitched_stream": FRAME + STITCH + OUT + STITCH_OUT + END,
    "decode_batch_once": FRAME + ONCE + OUT + ONCE_OUT + END,
    "decode_batch_once_stream": FRAME + ONCE + OUT + ONCE_OUT + [("continued", None)] + END,
}
CAPTURE_CALLS = {
    "scan_extract_decode_batch": CAPTURE + PRE + OUT + STATUS + END,
    "scan_extract_decode_batch_combined": CAPTURE + PRE + COMBINE + OUT + STATUS + COMBINE_OUT + END,
    "scan_extract_decode_batch_combined_stream": CAPTURE + PRE + STREAM + OUT + STATUS + STREAM_OUT + END,
    "scan_extract_decode_batch_stitched": CAPTURE + PRE + STITCH + OUT + STATUS + STITCH_OUT + END,
    "scan_extract_decode_batch_stitched_stream": CAPTURE + PRE + STITCH + OUT + STATUS + STITCH_OUT + END,
    "scan_extract_decode_batch_once": CAPTURE + PRE + ONCE + OUT + STATUS + ONCE_OUT + END,
    "scan_extract_decode_batch_once_stream": CAPTURE + PRE + ONCE + OUT + STATUS + ONCE_OUT + [("continued", None)] + END,
}
ONCE_CALLS = [k for k in list(FRAME_CALLS) + list(CAPTURE_CALLS) if "_once" in k]


class Entry:
    def __init__(self, fn, args, who, nulln, flags, inp, inflag, out, outflag, out_text=None, small=(4, 4)):
        self.fn, self.args, self.who, self.nulln, self.flags = fn, args, who, who + nulln, who + ": " + flags + MEM
        self.inp, self.inflag, self.out, self.outflag = inp, inflag, out, outflag
        self.out_text = out_text or self.nulln
        self.capture, self.small = any(k == "w" for k, _ in args), small

    def rows(self):
        """the rows every entry point gets: (label, overrides, return code, text)"""
        flush = any(k == "flush" for k, _ in self.args)   # the combined-stream calls: n == 0 is theirs (test_flush_rows)
        r = [("null input", {self.inp: None}, EINVAL, self.nulln),
             ("null " + self.out, {self.out: None}, EINVAL, self.out_text),
             ("n = -1", {"n": -1}, EINVAL, self.nulln),
             ("input flag 7", {self.inflag: BAD}, EINVAL, self.flags)]
        if not flush:
            r += [("n = 0", {"n": 0}, EINVAL, self.nulln),
                  ("n = 0 and a bad flag", {"n": 0, self.inflag: BAD}, EINVAL, self.nulln)]
        if self.outflag:
            r.append(("output flag 7", {self.outflag: BAD}, EINVAL, self.flags))
        if self.capture:
            r += [("a capture below the smallest", {"w": self.small[0], "h": self.small[1]}, EINVAL, self.nulln),
                  ("odd width with NV21", {"w": 9, "format": NV21}, EDIM, self.who + DIMS),
                  ("a bad flag and odd width with NV21", {"w": 9, "format": NV21, self.inflag: BAD}, EINVAL, self.flags)]
        return r


def entries():
    E = {}
    for name, args in FRAME_CALLS.items():
        E[name] = Entry("cimbar_hip_" + name, args, name, NULLN, "rgb_mem / out_mem", "rgb", "rgb_mem", "chunks", "out_mem")
    for name, args in CAPTURE_CALLS.items():
        E[name] = Entry("cimbar_hip_" + name + "_fmt", args, name, SMALL, ("img_mem" if "_once" in name else "rgb_mem") + " / out_mem", "img", "img_mem",
                        "chunks", "out_mem")
    E["decode_plain_batch"] = Entry("cimbar_hip_decode_plain_batch", FRAME + [("bytes", "P"), ("block_ok", None)] + END, "decode_plain_batch", NULLN,
                                    "rgb_mem / out_mem", "rgb", "rgb_mem", "bytes", "out_mem")
    E["scan_undistort_extract_decode_batch"] = Entry(
        "cimbar_hip_scan_undistort_extract_decode_batch_fmt", CAPTURE + PRE + OUT + STATUS + [("undistort_ok", None)] + END,
        "scan_undistort_extract_decode_batch", SMALL, "img_mem / out_mem", "img", "img_mem", "chunks", "out_mem",
        out_text="scan_undistort_extract_decode_batch: null chunks / masks")
    E["scan_preprocess"] = Entry("cimbar_hip_scan_preprocess_fmt", CAPTURE + [("binary", "P"), ("thresholds", None)] + END, "scan_preprocess",
                                 ": null buffer, n <= 0 or a frame smaller than 8x8", "rgb_mem / out_mem", "img", "img_mem", "binary", "out_mem")
    E["deskew_batch"] = Entry("cimbar_hip_deskew_batch_fmt", CAPTURE + [("corners", "P"), ("frames", "P")] + END, "deskew_batch",
                              ": null buffer, n <= 0 or an empty frame", "rgb_mem / out_mem", "img", "img_mem", "frames", "out_mem", small=(1, 1))
    E["extract_batch"] = Entry("cimbar_hip_extract_batch_fmt", CAPTURE + [("frames", "P"), ("status_out", "P"), ("corners", None)] + END, "extract_batch",
                               SMALL, "rgb_mem / out_mem", "img", "img_mem", "frames", "out_mem")
    E["undistort_calibrate"] = Entry("cimbar_hip_undistort_calibrate_fmt", CAPTURE + [("ok", "P"), ("k1", "P"), ("stream", None)], "undistort_calibrate",
                                     SMALL, "img_mem / out_mem", "img", "img_mem", "ok", None, out_text="undistort_calibrate: null ok / k1")
    E["undistort_batch"] = Entry("cimbar_hip_undistort_batch_fmt",
                                 CAPTURE + [("params", None), ("out_rgb", "P"), ("out_mem", H), ("ok", None), ("k1_out", None), ("stream", None)],
                                 "undistort_batch", SMALL, "img_mem / out_mem", "img", "img_mem", "out_rgb", "out_mem", out_text="undistort_batch: null out_rgb")
    E["rs_decode_erasures"] = Entry("cimbar_hip_rs_decode_erasures",
                                    [("blocks", "P"), ("n", 1), ("erasures", "P"), ("counts", "P"), ("mem", H), ("msgs", "P"), ("status", "P"), ("stream", None)],
                                    "rs_decode_erasures", NULLN, "mem", "blocks", "mem", "msgs", None)
    E["deliver_chunks"] = Entry("cimbar_hip_deliver_chunks",
                                [("chunks", "P"), ("masks", "P"), ("n", 1), ("in_mem", H), ("flags", 0), ("packed", "P"), ("src", None), ("count", "P")] + END,
                                "deliver_chunks", NULLN, "in_mem / out_mem", "chunks", "in_mem", "packed", "out_mem")
    return E


ENTRIES = entries()
# the single-flag text has no "a / b" in it
assert ENTRIES["rs_decode_erasures"].flags == "rs_decode_erasures: mem must be CIMBAR_HIP_MEM_HOST or CIMBAR_HIP_MEM_DEVICE"


class Rig:
    def __init__(self):
        self.lib = D.load_library()
        self.d68, self.d4 = D.HipDecoder(0, mode=68), D.HipDecoder(0, mode=4)
        self.bufs = {"F": np.zeros(1024 * 1024 * 3, np.uint8), "C": np.zeros(256, np.uint8), "P": np.zeros(1 << 16, np.uint8), "G": np.zeros(1 << 14, np.uint8)}

    def call(self, dec, name, **over):
        e = ENTRIES[name]
        unknown = set(over) - {k for k, _ in e.args}
        assert not unknown, (name, unknown)
        vals = [over.get(k, v) for k, v in e.args]
        vals = [self.bufs[v].ctypes.data if isinstance(v, str) else v for v in vals]
        rc = getattr(self.lib, e.fn)(dec._ctx, *vals)
        return int(rc), self.lib.cimbar_hip_last_error(dec._ctx).decode()

    def refused(self, dec, name, label, over, rc, text):
        got = self.call(dec, name, **over)
        assert got == (rc, text), (name, label, got)


@pytest.fixture(scope="module")
def rig():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r = Rig()
    yield r
    r.d68.close()
    r.d4.close()


@pytest.mark.parametrize("name", list(ENTRIES))
def test_common_rows(rig, name):
    """null input, null first output, n = 0 / -1, each flag 7; captures: below the smallest size, a size the format refuses (EDIM) -- and the
    orders: null / n before the flags, the flags before the capture's size"""
    for label, over, rc, text in ENTRIES[name].rows():
        rig.refused(rig.d68, name, label, over, rc, text)


def test_once_checks_come_first(rig):
    """check_once runs in front of everything else: a mode-4 context gets the modes text even with null buffers, a mode-68 one the
    min_agree text with a null input"""
    for name in ONCE_CALLS:
        inp = ENTRIES[name].inp
        rig.refused(rig.d4, name, "mode 4", {}, EINVAL, name + LEGACY)
        rig.refused(rig.d4, name, "mode 4, null buffers", {inp: None, "chunks": None}, EINVAL, name + LEGACY)
        rig.refused(rig.d68, name, "min_agree 1001 and a null input", {"min_agree": 1001, inp: None}, EINVAL, name + ": min_agree_permille above 1000")
        rig.refused(rig.d68, name, "max_run 9", {"max_run": 9}, EINVAL, name + ": max_run above 8")


def test_combine_and_stitch_checks_come_last(rig):
    """null / n, the flags and the capture's size (EDIM) all come before check_combine and check_stitch"""
    for name in ("decode_batch_combined", "decode_batch_combined_stream", "scan_extract_decode_batch_combined", "scan_extract_decode_batch_combined_stream"):
        e = ENTRIES[name]
        rig.refused(rig.d68, name, "max_group 9", {"max_group": 9}, EINVAL, name + ": max_group above 8")
        rig.refused(rig.d68, name, "null gchunks", {"gchunks": None}, EINVAL, name + ": null gchunks / gmasks")
        rig.refused(rig.d68, name, "max_group 9 and a bad flag", {"max_group": 9, e.outflag: BAD}, EINVAL, e.flags)
        rig.refused(rig.d68, name, "max_group 9 and a null input", {"max_group": 9, e.inp: None}, EINVAL, e.nulln)
        if e.capture:
            rig.refused(rig.d68, name, "max_group 9 and odd width with NV21", {"max_group": 9, "w": 9, "format": NV21}, EDIM, name + DIMS)
    for name in ("decode_batch_stitched", "decode_batch_stitched_stream", "scan_extract_decode_batch_stitched", "scan_extract_decode_batch_stitched_stream"):
        e = ENTRIES[name]
        rig.refused(rig.d68, name, "axis 2", {"axis": 2}, EINVAL, name + ": axis must be 0 (grid rows) or 1 (grid columns)")
        rig.refused(rig.d68, name, "axis 2 and a bad flag", {"axis": 2, e.inflag: BAD}, EINVAL, e.flags)
        rig.refused(rig.d68, name, "axis 2 and n = 0", {"axis": 2, "n": 0}, EINVAL, e.nulln)
        if e.capture:
            rig.refused(rig.d68, name, "axis 2 and odd width with NV21", {"axis": 2, "w": 9, "format": NV21}, EDIM, name + DIMS)


def test_undistort_composite_checks_its_outputs_first(rig):
    name = "scan_undistort_extract_decode_batch"
    for over in ({"masks": None}, {"chunks": None, "img": None}, {"masks": None, "n": 0, "img_mem": BAD}):
        rig.refused(rig.d68, name, str(over), over, EINVAL, name + ": null chunks / masks")


def test_flush_rows(rig):
    """n == 0 is a flush for the two combined-stream calls: no image argument is read and a fresh stream returns 0 groups. The frame call
    still checks both flags; the capture call checks out_mem alone and accepts any img_mem (a quirk of the order its checks are written in:
    kept, and pinned here, so that removing it is a decision)."""
    lib, ctx = rig.lib, rig.d68._ctx
    f, c = "decode_batch_combined_stream", "scan_extract_decode_batch_combined_stream"
    assert lib.cimbar_hip_combine_stream_reset(ctx) == 0
    rig.refused(rig.d68, f, "n = 0 without a flush", {"n": 0}, EINVAL, f + ": n == 0 without a flush")
    rig.refused(rig.d68, c, "n = 0 without a flush", {"n": 0}, EINVAL, c + ": n == 0 without a flush")
    rig.refused(rig.d68, f, "flush, rgb_mem 7", {"n": 0, "flush": 1, "rgb": None, "rgb_mem": BAD}, EINVAL, f + ": rgb_mem / out_mem" + MEM)
    rig.refused(rig.d68, f, "flush, out_mem 7", {"n": 0, "flush": 1, "rgb": None, "out_mem": BAD}, EINVAL, f + ": rgb_mem / out_mem" + MEM)
    rig.refused(rig.d68, c, "flush, out_mem 7", {"n": 0, "flush": 1, "img": None, "out_mem": BAD}, EINVAL, c + ": out_mem" + MEM)
    assert rig.call(rig.d68, f, n=0, flush=1, rgb=None, chunks=None, masks=None)[0] == 0
    assert rig.call(rig.d68, c, n=0, flush=1, img=None, chunks=None, masks=None, w=0, h=0)[0] == 0
    assert rig.call(rig.d68, c, n=0, flush=1, img=None, img_mem=BAD)[0] == 0   # the quirk
    assert lib.cimbar_hip_combine_stream_reset(ctx) == 0


def test_contexts_still_decode(rig):
    """after every test above: one decode_frame on each context returns CHUNK (625 in mode 68) * popcount(mask)"""
    for dec in (rig.d68, rig.d4):
        dec.reset_ccm()
        good, _, m = dec.decode_frame(np.zeros(dec.geo.FRAME_SHAPE, np.uint8))
        assert good == dec.geo.CHUNK * bin(m).count("1")
    assert rig.d68.geo.CHUNK == 625
