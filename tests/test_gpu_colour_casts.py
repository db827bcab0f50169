"""GPU: the colour half of the decoder under camera colour casts (tests/colour_cases.py) -- k_frame_mid's matrix (init_ccm / von Kries), k_colors'
classifier and the matrix in force (the frame's own, else the newest earlier one of the batch, else the carried one) -- bit-exact against the oracle
per frame: symbols, drifted positions, colours, matrix bytes and active flag, masks and chunks. Every mode, color_correction 0 / 1 / 2, both
preprocess settings; the header designs; the carry over more than 256 frames through the split tail chain, the pipelined entry and the plain path;
and the device's matrices against the float64 pseudo-inverse."""
import os

import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from libcimbar_amd import framegen, geometry
from oracle import pyref
from tests import colour_cases as C
from tests.test_gpu_modes import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[68, 67, 66, 4, 8])
def MODE(request):
    return request.param


@pytest.fixture(scope="module")
def dec(MODE):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = D.HipDecoder(0, MODE)
    yield d
    d.close()


@pytest.fixture(scope="module", params=[68, 67, 66])
def HMODE(request):
    """the modes whose colour pass follows a fountain header (the legacy modes 4 and 8 never derive a header matrix)"""
    return request.param


@pytest.fixture(scope="module")
def hdec(HMODE):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = D.HipDecoder(0, HMODE)
    yield d
    d.close()


def render(mode, payload):
    return framegen.FrameSynth("cpu", mode).frames_from_payload(torch.from_numpy(np.ascontiguousarray(payload))).numpy()


def make_cast_set(MODE):
    geo = geometry.for_mode(MODE)
    seeds = (0, 1)
    pay = framegen.synth_payload(len(C.FAMILIES) * len(seeds), seed=17, mode=MODE).numpy()
    fr = render(MODE, pay)
    names, frames = [], []
    for i, fam in enumerate(C.FAMILIES):
        for j, s in enumerate(seeds):
            k = i * len(seeds) + j
            names.append(f"{fam}/{s}")
            frames.append(C.family_cast(fam, 7000 + 100 * i + s, fr[k], geo))
    return names, frames, pay


@pytest.fixture(scope="module")
def cast_set(MODE):
    return make_cast_set(MODE)


@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("cc", [0, 1, 2])
def test_cast_families_bit_exact(dec, MODE, cast_set, cc, pre):
    names, frames, _ = cast_set
    _, masks, want = check(dec, frames, pre=pre, cc=cc, names=names)
    if MODE == 68 and cc == 2 and pre == 0:
        mild = [k for k, nm in enumerate(names) if nm.startswith("mild")]
        assert (masks[mild] == dec.geo.FULL_MASK).all(), "the mild casts must decode fully: the generator is too harsh"
    if cc == 2 and not dec.geo.LEGACY:
        assert sum(w["active"] for w in want) >= len(frames) // 2        # most frames carry a matrix of their own or an earlier one


def test_header_designs_bit_exact(hdec, HMODE):
    """the 24 first-appearance orders, one colour in one header cell, a colour never seen, an all-zero id -- each under a mild and a strong cast.
    The frames without a matrix come first, so that nothing is carried into them."""
    dec, MODE = hdec, HMODE
    geo = dec.geo
    designs = C.header_designs(MODE)
    order = ["zero_id", "absent"] + [k for k in designs if k not in ("zero_id", "absent")]
    names, frames = [], []
    for k, name in enumerate(order):
        pay = C.design_payload(2, 300 + k, MODE, *designs[name][:2])
        fr = render(MODE, pay)
        for j, fam in enumerate(("mild", "strong")):
            names.append(f"{name}/{fam}")
            frames.append(C.family_cast(fam, 900 + 2 * k + j, fr[j], geo))
    _, masks, want = check(dec, frames, cc=2, names=names)
    n = len(frames)
    ccm = dec.tap(D.TAP_CCM, n)
    assert not ccm[:4, 9].any(), "no header / a colour never seen: no matrix"
    assert ccm[4:, 9].all() and all(w["active"] for w in want[4:])
    assert masks[0] == geo.FULL_MASK and not dec.tap(D.TAP_FLOOD, n)[0], "zero id: decodes fully on the parallel path"
    # every frame from the fifth on derives a matrix of its own: consecutive frames' matrices differ
    assert all(ccm[k, :9].tobytes() != ccm[k - 1, :9].tobytes() for k in range(5, n))


# ---------------------------------------------------------------------------------------------- the carry at scale (mode 68)
N_CARRY, N_SECOND, HEADER_FRAMES, POOL = 600, 300, (0, 5, 300), 8


@pytest.fixture(scope="module")
def carry_case():
    """a 600-frame batch in which only frames 0, 5 and 300 carry a usable header (frames 261-299 find their matrix more than 256 frames back),
    and a 300-frame batch without any header (it takes the first batch's last matrix). Frames are drawn from a pool of distinctly cast frames;
    the oracle is run once per (frame, matrix carried in)."""
    geo = geometry.for_mode(68)
    designs = C.header_designs(68)
    zero = C.design_payload(POOL, 41, 68, *designs["zero_id"][:2])
    hdr = np.concatenate([C.design_payload(1, 50 + k, 68, *designs[name][:2]) for k, name in enumerate(("order0123", "order2301", "order3120"))])
    pool = render(68, np.concatenate([zero, hdr]))
    pool = np.stack([C.family_cast("strong" if k % 2 else "mild", 4000 + k, pool[k], geo) for k in range(len(pool))])
    first = [POOL + HEADER_FRAMES.index(f) if f in HEADER_FRAMES else (f * 5) % POOL for f in range(N_CARRY)]
    second = [(f * 3 + 1) % POOL for f in range(N_SECOND)]
    memo = {}
    state = pyref.CoCcm()
    want = []
    for idx in first + second:
        key = (idx, bytes(state.m), state.active)
        if key not in memo:
            c = pyref.CoCcm()
            c.m[:] = list(state.m)
            c.active = state.active
            r, ch, mask, c = pyref.oracle_decode(pool[idx], 0, 2, c)
            sym, col, pos = pyref.oracle_stage()
            memo[key] = dict(r=r, chunks=ch.copy(), mask=mask, sym=sym, col=col, pos=pos, ccm=np.array(list(c.m), np.float32), active=c.active)
        w = memo[key]
        want.append(w)
        state = pyref.CoCcm()
        state.m[:] = list(w["ccm"])
        state.active = w["active"]
    # the case is what it claims: three distinct matrices, frames 261-299 on frame 5's, the second batch on frame 300's
    m = [want[f]["ccm"].tobytes() for f in HEADER_FRAMES]
    assert all(want[f]["active"] for f in HEADER_FRAMES) and len(set(m)) == 3
    assert all(want[f]["ccm"].tobytes() == m[1] for f in range(261, 300))
    assert all(want[N_CARRY + f]["ccm"].tobytes() == m[2] for f in range(N_SECOND))
    return pool, first, second, want


def compare(dec, n, chunks, masks, want, tag):
    xy = dec.geo.cell_positions()
    sym, col, drift, ccm = dec.tap(D.TAP_SYMBOLS, n), dec.tap(D.TAP_COLORS, n), dec.tap(D.TAP_DRIFT, n), dec.tap(D.TAP_CCM, n)
    assert not dec.tap(D.TAP_FLOOD, n).any(), f"{tag}: a frame took the flood path (the split chain wants none)"
    for k in range(n):
        w = want[k]
        assert bool(ccm[k, 9]) == bool(w["active"]), f"{tag} frame {k}: CCM active flag"
        assert not w["active"] or ccm[k, :9].tobytes() == w["ccm"].tobytes(), f"{tag} frame {k}: CCM differs"
        assert (sym[k] == w["sym"]).all() and (xy + drift[k].astype(np.int32) == w["pos"]).all(), f"{tag} frame {k}: symbols / positions"
        assert (col[k] == w["col"]).all(), f"{tag} frame {k}: colours differ in {(col[k] != w['col']).sum()} cells"
        assert masks[k] == w["mask"] and (chunks[k] == w["chunks"].reshape(-1)).all(), f"{tag} frame {k}: mask / chunks"


@pytest.mark.parametrize("env", [{}, {"CIMBAR_HIP_TAIL_PARTS": "4"}, {"CIMBAR_HIP_TAIL_PARTS": "8"}, {"CIMBAR_HIP_TAIL_SPLIT": "0"}],
                         ids=["default", "parts4", "parts8", "nosplit"])
def test_carry_across_256_frames_and_split_chain(carry_case, env):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    pool, first, second, want = carry_case
    parts = int(env.get("CIMBAR_HIP_TAIL_PARTS", "2"))
    assert N_CARRY >= 64 * parts                           # host.hip.inc: a batch splits when n >= 64 * parts and the batch before did not flood
    old = {k: os.environ.get(k) for k in ("CIMBAR_HIP_TAIL_PARTS", "CIMBAR_HIP_TAIL_SPLIT")}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        dec = D.HipDecoder(0, 68)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    dev = torch.device("cuda:0")
    try:
        d_pool = torch.from_numpy(pool).to(dev)
        fb = dec.geo.FRAME_BYTES
        for tag, idx, w in (("batch 1", first, want[:N_CARRY]), ("batch 2", second, want[N_CARRY:])):
            frames = d_pool[torch.tensor(idx, device=dev)].contiguous()
            n = len(idx)
            chunks = torch.zeros((n, fb), dtype=torch.uint8, device=dev)
            masks = torch.zeros(n, dtype=torch.int32, device=dev)
            dec.decode_batch_device(frames.data_ptr(), n, chunks.data_ptr(), masks.data_ptr())
            torch.cuda.synchronize()
            compare(dec, n, chunks.cpu().numpy(), masks.cpu().numpy().astype(np.uint32), w, f"{env} {tag}")
            del frames
        active, m = dec.get_ccm()
        assert active and m.reshape(-1).tobytes() == want[-1]["ccm"].tobytes()
    finally:
        dec.close()


def test_carry_through_pipelined_batches(carry_case):
    """the same 900 frames as six 150-frame batches through decode_batch_pipelined, several in flight: masks and chunks frame by frame"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    pool, first, second, want = carry_case
    dec = D.HipDecoder(0, 68)
    dev = torch.device("cuda:0")
    try:
        idx = first + second
        d_pool = torch.from_numpy(pool).to(dev)
        fb, B = dec.geo.FRAME_BYTES, 150
        assert dec.pipeline_depth >= 2
        st = torch.cuda.current_stream().cuda_stream
        ins, chs, mks = [], [], []
        for b in range(0, len(idx), B):
            ins.append(d_pool[torch.tensor(idx[b:b + B], device=dev)].contiguous())
            chs.append(torch.zeros((B, fb), dtype=torch.uint8, device=dev))
            mks.append(torch.zeros(B, dtype=torch.int32, device=dev))
            dec.decode_batch_pipelined(ins[-1].data_ptr(), B, chs[-1].data_ptr(), mks[-1].data_ptr(), stream=st)
            if len(ins) >= dec.pipeline_depth:
                dec.pipeline_wait(stream=st, keep_newest=dec.pipeline_depth - 1)
        dec.pipeline_wait(stream=st)
        torch.cuda.synchronize()
        chunks = torch.cat(chs).cpu().numpy()
        masks = torch.cat(mks).cpu().numpy().astype(np.uint32)
        for k, w in enumerate(want):
            assert masks[k] == w["mask"] and (chunks[k] == w["chunks"].reshape(-1)).all(), f"frame {k}"
        active, m = dec.get_ccm()
        assert active and m.reshape(-1).tobytes() == want[-1]["ccm"].tobytes()
        # Decoder::decode (no fountain: no header reaches the reader) on the carried cast matrix
        zero = pool[[k for k in range(POOL)]]
        r, data, ok = dec.decode_plain_batch(zero)
        ccm = pyref.CoCcm()
        ccm.m[:] = list(want[-1]["ccm"])
        ccm.active = 1
        tot = 0
        for k in range(POOL):
            wr, wdata, wok, ccm = pyref.oracle_decode_plain(zero[k], 0, 2, ccm)
            tot += wr
            assert (ok[k] == wok).all() and (data[k] == wdata).all(), f"plain frame {k}"
        assert r == tot
        assert dec.tap(D.TAP_CCM, POOL)[:, :9].tobytes() == np.tile(want[-1]["ccm"], (POOL, 1)).tobytes()
    finally:
        dec.close()


def test_device_matrices_against_float64(hdec, HMODE):
    """every cast frame by itself (nothing carried in): the device's matrix within the CPU test's bound of the float64 pseudo-inverse (skipping
    systems with a singular value near the cut-off), and the von Kries matrix of color_correction 1 likewise"""
    dec = hdec
    geo = dec.geo
    names, frames, pay = make_cast_set(HMODE)
    sym_chunks, nhdr = C.chunk_counts(geo)
    checked = 0
    for k, fr in enumerate(frames):
        dec.reset_ccm()
        dec.decode_batch(fr[None], color_correction=2)
        m = dec.tap(D.TAP_CCM, 1)[0]
        sysm = C.ccm_system(fr, geo, pay[k].reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)[sym_chunks:sym_chunks + nhdr, :6])
        if m[9] and sysm is not None:
            c64, s, thr = C.ccm64(*sysm)
            bound = C.ccm_bound(c64, s, thr)
            if bound is not None:
                assert np.abs(m[:9].astype(np.float64).reshape(3, 3) - c64).max() <= bound, names[k]
                checked += 1
        dec.reset_ccm()
        dec.decode_batch(fr[None], color_correction=1)
        v = dec.tap(D.TAP_CCM, 1)[0]
        v64 = C.von_kries64(C.white64(fr, geo).astype(np.float32))
        assert v[9] and np.abs(v[:9].astype(np.float64).reshape(3, 3) - v64).max() <= 64 * 2.0 ** -23 * np.abs(v64).max() * np.linalg.cond(v64)
    assert checked >= len(frames) // 2
