"""GPU: cimbar_hip_rs_decode_erasures (the errors-and-erasures decode, k_rs_erasures) against tests/golden/rs_erasures.json -- libcorrect's
correct_reed_solomon_decode_with_erasures on every RS code the modes use -- in all five modes (68, 4 and 8 share RS(155,125)). Per block:
libcorrect's outcome (-1 or success), the message bytes it returns, and the acceptance status of tests/erasure_model.py; through host
memory and through device memory on a stream of its own. Nothing here touches a decode, so the context's decode state is not involved."""
import json
import os

import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rs_erasures.json")
MODES = [68, 67, 66, 4, 8]
CODE = {68: 155, 4: 155, 8: 155, 67: 179, 66: 168}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return {c["n"]: c for c in json.load(f)["codes"]}


@pytest.fixture(scope="module", params=MODES)
def MODE(request):
    return request.param


@pytest.fixture(scope="module")
def dec(MODE):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = D.HipDecoder(0, MODE)
    yield d
    d.close()


def _arrays(code):
    blocks = np.stack([np.frombuffer(bytes.fromhex(c["block"]), np.uint8) for c in code["cases"]])
    return blocks, [c["erasures"] for c in code["cases"]]


def _check(code, msgs, status):
    p, k = code["parity"], code["n"] - code["parity"]
    seen = {-1: 0, 0: 0, 1: 0}
    for b, c in enumerate(code["cases"]):
        want = -1 if c["rc"] < 0 else (1 if c["status"] == 1 else 0)
        assert int(status[b]) == want, (c["family"], len(c["erasures"]), int(status[b]), want)
        if c["rc"] > 0:
            assert bytes(msgs[b]).hex() == c["msg"], (c["family"], len(c["erasures"]))
        else:   # libcorrect fails: the received message bytes come back unchanged
            assert bytes(msgs[b]).hex() == c["block"][:2 * k]
        seen[want] += 1
    assert all(seen.values()), seen
    return seen


def test_rs_erasures_golden_host(MODE, dec, golden):
    code = golden[CODE[MODE]]
    assert (dec.geo.RS_BLOCK, dec.geo.RS_PARITY) == (code["n"], code["parity"])
    blocks, er = _arrays(code)
    msgs, status = dec.rs_decode_erasures(blocks, er)
    _check(code, msgs, status)


def test_rs_erasures_golden_device(MODE, dec, golden):
    """device buffers on a side stream; the rows repeated so that the last workgroup of the launch is a partial one"""
    code = golden[CODE[MODE]]
    n = dec.geo.RS_BLOCK
    blocks, er = _arrays(code)
    reps = 3
    blocks = np.concatenate([blocks] * reps)
    er = er * reps
    nb = len(er)
    rows = np.zeros((nb, n), np.uint8)
    counts = np.zeros(nb, np.uint8)
    for b, pos in enumerate(er):
        rows[b, :len(pos)] = pos
        counts[b] = len(pos)
    dev = torch.device("cuda", 0)
    d_blocks = torch.from_numpy(blocks).to(dev)
    d_rows = torch.from_numpy(rows).to(dev)
    d_counts = torch.from_numpy(counts).to(dev)
    d_msgs = torch.full((nb + 1, dec.geo.RS_DATA), 0xA5, dtype=torch.uint8, device=dev)    # one guard row past the end
    d_status = torch.full((nb + 8,), 0x5A, dtype=torch.int8, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    dec.rs_decode_erasures_device(d_blocks.data_ptr(), nb, d_rows.data_ptr(), d_counts.data_ptr(), d_msgs.data_ptr(), d_status.data_ptr(),
                                  stream=s.cuda_stream)
    s.synchronize()
    msgs, status = d_msgs.cpu().numpy(), d_status.cpu().numpy()
    assert (msgs[nb] == 0xA5).all() and (status[nb:] == 0x5A).all(), "wrote past the n blocks it was given"
    for r in range(reps):
        _check(code, msgs[r * len(code["cases"]):(r + 1) * len(code["cases"])], status[r * len(code["cases"]):(r + 1) * len(code["cases"])])


def test_rs_erasures_recovers_twice_the_errors(MODE, dec):
    """p corrupted bytes: errors-only decoding cannot return the sent message; with their positions as erasures every block decodes"""
    g = np.random.default_rng(MODE)
    n, p, k = dec.geo.RS_BLOCK, dec.geo.RS_PARITY, dec.geo.RS_DATA
    from tests import rs_cases
    msgs = g.integers(0, 256, (64, k), dtype=np.uint8)
    code = rs_cases.encode(msgs, p)
    bad = code.copy()
    er = []
    for b in range(64):
        pos = g.permutation(n)[:p]
        bad[b, pos] ^= g.integers(1, 256, p, dtype=np.uint8)
        er.append(pos)
    out0, st0 = dec.rs_decode_erasures(bad, [[]] * 64)
    assert not any(st0[b] == 1 and (out0[b] == msgs[b]).all() for b in range(64))
    out, st = dec.rs_decode_erasures(bad, er)
    assert (st == 1).all() and (out == msgs).all()
