"""The colour half of the decoder under camera colour casts, on the CPU: the classifier of the oracle and of the reference build against a float32
restatement written from CimbDecoder.cpp (tests/colour_cases.py), exhaustively under active matrices; the oracle against the reference build on
cast frames with the matrix carried; the oracle's matrices against a float64 pseudo-inverse. (The device is held to the oracle on the same inputs in
tests/test_gpu_colour_casts.py.)"""
import ctypes

import numpy as np
import pytest
import torch

from libcimbar_amd import framegen, geometry
from oracle import pyref
from oracle.pyref import P
from tests import colour_cases as C

MODES = (68, 67, 66, 4, 8)
PALETTE_MODES = (68, 4, 8)          # 67 and 66 classify with mode 68's palette


def _ccm(m):
    c = pyref.CoCcm()
    if m is not None:
        c.m[:] = [float(v) for v in np.asarray(m, np.float32).reshape(-1)]
        c.active = 1
    return c


def oracle_classes(mode, rgb, m):
    out = np.zeros(len(rgb), np.uint8)
    pyref.oracle_lib(mode).co_best_color_batch(P(rgb), len(rgb), ctypes.byref(_ccm(m)) if m is not None else None, P(out))
    return out


def ref_classes(mode, rgb, m):
    with pyref.ref_mode(mode) as R:
        R.ref_set_ccm(P(np.asarray(m if m is not None else np.zeros(9), np.float32).reshape(-1).copy()), int(m is not None))
        out = np.zeros(len(rgb), np.uint8)
        R.ref_best_color_batch(P(rgb), len(rgb), P(out))
        R.ref_set_ccm(P(np.zeros(9, np.float32)), 0)
    return out


def cast_frames(mode, seeds=(0,), payload_seed=5):
    """(name, frame, payload) for every family and seed, rendered in `mode`"""
    geo = geometry.for_mode(mode)
    synth = framegen.FrameSynth("cpu", mode)
    n = len(C.FAMILIES) * len(seeds)
    pay = framegen.synth_payload(n, seed=payload_seed, mode=mode).numpy()
    fr = synth.frames_from_payload(torch.from_numpy(pay)).numpy()
    out = []
    for i, fam in enumerate(C.FAMILIES):
        for j, s in enumerate(seeds):
            k = i * len(seeds) + j
            out.append((f"{fam}/{s}", C.family_cast(fam, 1000 * mode + 100 * i + s, fr[k], geo), pay[k]))
    return out


def colour_headers(geo, payload):
    sym_chunks, nhdr = C.chunk_counts(geo)
    return payload.reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)[sym_chunks:sym_chunks + nhdr, :6]


def family_matrices():
    """matrices the oracle derives from cast frames in mode 68 (colour_correction 2), one per family that yields one"""
    out = {}
    for name, fr, _ in cast_frames(68, seeds=(1,), payload_seed=8):
        _, _, _, ccm = pyref.oracle_decode(fr, 0, 2, None)
        if ccm.active:
            out[name] = np.array(list(ccm.m), np.float32)
    return out


def vk_matrix(white):
    m = (ctypes.c_float * 9)()
    pyref.oracle_lib().co_von_kries_ccm((ctypes.c_float * 3)(*white), m)
    return np.array(list(m), np.float32)


@pytest.fixture(scope="module")
def strong_matrix():
    m = family_matrices()["strong/1"]
    assert (m < 0).any(), m
    return m


def exhaustive_matrices(mode, strong):
    """no matrix, the identity, a strong-cast matrix and a von Kries matrix (the legacy palettes: the two cast matrices -- with no matrix they are
    the mode-68 code path with another table)"""
    mats = {"strong": strong, "von_kries": vk_matrix((182.0, 201.5, 139.25))}
    if mode == 68:
        mats = {"inactive": None, "identity": np.eye(3, dtype=np.float32).reshape(-1), **mats}
    return mats


def each_quarter():
    step = 1 << 22
    for lo in range(0, 1 << 24, step):
        yield C.all_rgb(lo, lo + step)


def assert_same(name, who, x, got, want):
    bad = np.flatnonzero(got != want)
    assert not len(bad), f"{name}: {who} differs at {len(bad)} inputs, first {x[bad[0]]}: {got[bad[0]]} vs {want[bad[0]]}"


@pytest.mark.parametrize("mode", PALETTE_MODES)
def test_classifier_exhaustive_under_active_matrices(mode, strong_matrix):
    """all 2^24 integer RGB: the oracle's classifier equals the restatement under each matrix, and every class is reached"""
    pal = C.palette(mode)
    for name, m in exhaustive_matrices(mode, strong_matrix).items():
        counts = np.zeros(len(pal), np.int64)
        for x in each_quarter():
            want = C.best_color(x, m, pal)
            assert_same(name, "oracle", x, oracle_classes(mode, x, m), want)
            counts += np.bincount(want, minlength=len(pal))
        assert (counts > 0).all(), (name, counts)


@pytest.fixture(scope="module")
def ref_colour(ref):
    if not pyref.ref_has_colour_batch(ref):
        pytest.skip("this reference build predates ref_set_ccm / ref_best_color_batch (oracle/ref/ref_colour.cpp): rebuild oracle/_ref")
    return ref


@pytest.mark.parametrize("mode", PALETTE_MODES)
def test_reference_classifier_exhaustive_under_active_matrices(mode, ref_colour, strong_matrix):
    """the same 2^24 inputs and matrices through the reference build's own CimbDecoder::get_best_color"""
    pal = C.palette(mode)
    for name, m in exhaustive_matrices(mode, strong_matrix).items():
        for x in each_quarter():
            assert_same(name, "reference", x, ref_classes(mode, x, m), C.best_color(x, m, pal))


def panel_matrices():
    rng = np.random.default_rng(77)
    out = {f"family_{k}": m for k, m in family_matrices().items()}
    out["negative"] = np.array([1.6, -0.5, -0.2, -0.4, 1.3, -0.3, -0.1, -0.7, 1.9], np.float32)
    out["large"] = np.array([12.5, -3.0, 0.5, -2.0, 10.25, 1.0, 0.0, -4.0, 14.0], np.float32)
    out["near_singular"] = np.array([1.0, 1.0, 0.0, 1.0, 1.0 + 2 ** -20, 0.0, 0.2, 0.3, 0.5], np.float32)
    out["rank_one"] = np.array([0.4, 0.5, 0.1] * 3, np.float32)
    out["random"] = rng.uniform(-2, 3, 9).astype(np.float32)
    out["von_kries_dark"] = vk_matrix((21.0, 30.5, 12.0))
    return out


@pytest.mark.parametrize("mode", PALETTE_MODES)
def test_classifier_panel_of_matrices(mode):
    """a stratified 2^20 sample of the RGB cube under negative entries, entries above 10, near-singular matrices and the matrices the cast families
    produce: oracle == restatement"""
    x = C.stratified_rgb(20, seed=mode)
    pal = C.palette(mode)
    for name, m in panel_matrices().items():
        assert_same(name, "oracle", x, oracle_classes(mode, x, m), C.best_color(x, m, pal))


@pytest.mark.parametrize("mode", PALETTE_MODES)
def test_reference_classifier_panel_of_matrices(mode, ref_colour):
    """the same sample and panel through the reference build: reference == restatement"""
    x = C.stratified_rgb(20, seed=mode)
    pal = C.palette(mode)
    for name, m in panel_matrices().items():
        assert_same(name, "reference", x, ref_classes(mode, x, m), C.best_color(x, m, pal))


def test_header_designs_are_what_they_claim():
    """the 27 header designs per mode: all four colours in every first-appearance order, colour 3 once, colour 3 never, id 0"""
    for mode in (68, 67, 66):
        d = C.header_designs(mode)
        assert len([k for k in d if k.startswith("order")]) == 24 and {"one_cell", "absent", "zero_id"} <= set(d)
        geo = geometry.for_mode(mode)
        # the payload carries exactly the headers the reader will predict
        p = C.design_payload(1, 3, mode, *d["absent"][:2])[0].reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)
        sym_chunks, nhdr = C.chunk_counts(geo)
        assert np.bincount(C.expected_colours(p[sym_chunks:sym_chunks + nhdr, :6]), minlength=4)[3] == 0


@pytest.mark.parametrize("mode", MODES)
def test_oracle_equals_reference_on_cast_frames(ref, mode):
    """whole decode with the matrix carried frame to frame, color_correction 0 / 1 / 2: every cast family and (modes with a header) the header
    designs under a strong cast -- good bytes, mask, chunks, matrix bytes and active flag"""
    frames = [(nm, fr) for nm, fr, _ in cast_frames(mode)]
    if mode in (68, 67, 66):
        geo = geometry.for_mode(mode)
        synth = framegen.FrameSynth("cpu", mode)
        designs = C.header_designs(mode)
        for k, name in enumerate(["zero_id", "absent", "one_cell", "order3210", "order1302"]):
            pay = C.design_payload(1, 40 + k, mode, *designs[name][:2])
            fr = synth.frames_from_payload(torch.from_numpy(pay)).numpy()[0]
            frames.append((name, C.family_cast("strong", 500 + k, fr, geo)))
    for cc in (0, 1, 2):
        with pyref.ref_mode(mode) as R:
            R.ref_reset_ccm()
            ccm = pyref.CoCcm()
            for name, fr in frames:
                r1, c1, m1 = pyref.ref_decode(fr, 0, cc, reset_ccm=0, mode=mode)
                r2, c2, m2, ccm = pyref.oracle_decode(fr, 0, cc, ccm, mode=mode)
                assert (r1, m1) == (r2, m2), (cc, name)
                assert (c1 == c2).all(), (cc, name)
                rc = (ctypes.c_float * 9)()
                active = R.ref_get_ccm(rc)
                assert active == ccm.active, (cc, name)
                if active:
                    assert np.array(list(rc), np.float32).tobytes() == np.array(list(ccm.m), np.float32).tobytes(), (cc, name)


def test_oracle_ccm_against_float64_reference():
    """every cast family in modes 68 / 67 / 66: the matrix init_ccm derives (oracle, float32 Jacobi SVD) within c kappa 2^-23 |ccm64| of the float64
    desired^T pinv(actual^T); the von Kries matrix of color_correction 1 likewise. Frames whose system has a singular value near the cut-off are
    skipped and counted; no well-conditioned family may be skipped entirely. Prints the per-family counts."""
    stats = {}
    for mode in (68, 67, 66):
        geo = geometry.for_mode(mode)
        for name, fr, pay in cast_frames(mode, seeds=(0, 1, 2)):
            fam = name.split("/")[0]
            st = stats.setdefault(fam, [0, 0, 0, 0, 0])
            st[0] += 1
            _, _, mask, ccm = pyref.oracle_decode(fr, 0, 2, None, mode=mode)
            pos = pyref.oracle_stage(mode=mode)[2]
            sysm = C.ccm_system(fr, geo, colour_headers(geo, pay))
            # a header needs one chunk of the symbol stream delivered; then the matrix exists iff all four colours are expected
            assert bool(ccm.active) == (sysm is not None and (mask & ((1 << C.chunk_counts(geo)[0]) - 1)) != 0), name
            if ccm.active:
                st[1] += 1
                c64, s, thr = C.ccm64(*sysm)
                bound = C.ccm_bound(c64, s, thr)
                if bound is None:
                    st[2] += 1
                else:
                    err = np.abs(np.array(list(ccm.m), np.float64).reshape(3, 3) - c64).max()
                    assert err <= bound, (mode, name, err, bound, s, thr)
                # cells within one unit of a classifier tie under the matrix in force, at the positions the decoder read them
                xy = pos + 1
                rgb = np.stack([fr[y:y + 6, x:x + 6].reshape(-1, 3).astype(np.int64).sum(0) // 36 for x, y in xy[::7]]).astype(np.float32)
                st[3] += int(C.near_tie(rgb, np.array(list(ccm.m), np.float32), C.palette(mode)).sum())
                st[4] += len(rgb)
            # color_correction 1: von Kries from the anchor white
            _, _, _, vk = pyref.oracle_decode(fr, 0, 1, None, mode=mode)
            v64 = C.von_kries64(C.white64(fr, geo).astype(np.float32))
            err = np.abs(np.array(list(vk.m), np.float64).reshape(3, 3) - v64).max()
            assert vk.active and err <= 64 * 2.0 ** -23 * np.abs(v64).max() * np.linalg.cond(v64), (mode, name, err)
    print("\nfamily: frames / with a matrix / skipped (conditioning) / sampled cells within one unit of a tie of sampled cells")
    for fam, st in stats.items():
        print(f"  {fam}: {st[0]} / {st[1]} / {st[2]} / {st[3]} of {st[4]}")
    for fam in C.WELL_CONDITIONED:
        assert stats[fam][1] > stats[fam][2], (fam, stats[fam])
    assert stats["mild"][1] == stats["mild"][0]
