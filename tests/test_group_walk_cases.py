"""CPU: the inputs of tests/test_gpu_group_walk.py vetted without a device (tests/group_walk_cases.py), on synthetic agreement counts: two
captures of one run agree on every cell, captures of two runs on none.

1. The rule's grouping of the committed cases (tests/combine_model.group_captures, tests/combine_stream_model.StreamModel) shows every shape
   a walk of 64 captures per step can get wrong: groups that straddle a step, heads at lane 0 and at lane 63, cap phases that depend on the
   run's start in an earlier step, and for the stream calls every kind of call ending at lane 63 and at lane 0.
2. walk() / walk_stream() below restate k_group_walk (groups_in == nullptr) and k_group_walk_stream lane by lane -- ballots as integers,
   lane 63's values handed to the next step, exactly the kernels' carried variables -- and reproduce the rule on every case: groups, the
   member table, the group count, the open group.
3. The same simulation with ONE carried variable forgotten at every step boundary (reset to its initial value) differs from the rule on at
   least one committed case, for each of run_carry, starts_carry, mem_carry, base_carry, prev_id, prev_u: the cases discriminate. last_u is
   not handed over a boundary -- it is taken in the step that holds the last virtual capture -- so its mutant is the one that takes it in
   the first step only and keeps the initial value when the batch ends later.
"""
import numpy as np
import pytest

from tests import combine_model as CM
from tests import combine_stream_model as SM
from tests import group_walk_cases as GW

NCELLS = 8             # of the synthetic rows
CARRIED = ("run_carry", "starts_carry", "mem_carry", "base_carry", "prev_id", "prev_u")
INITIAL = dict(run_carry=0, starts_carry=0, mem_carry=0, base_carry=0, prev_id=-1, prev_u=False)


def clz64(x):
    return 64 - int(x).bit_length()


def popc(x):
    return bin(int(x)).count("1")


def ballot(flags):
    return sum(1 << l for l in range(64) if flags[l])


def walk_stream(agree, status, c, min_agree, max_group, flush, forget=None):
    """k_group_walk_stream over c carried members and the call's n captures; agree[k] = agree(predecessor, capture k). c = 0 and flush
    is k_group_walk with groups_in == nullptr (the same walk; every group closes). -> groups (n,), gmem {(id, rank): virtual index},
    gcount {id: members}, the groups that close, the open group's size"""
    n = len(status)
    N = c + n
    groups = np.full(n, -9, np.int64)
    gmem, gcount = {}, {}
    v = dict(INITIAL)
    top, last_u = -1, False
    L = range(64)
    for j0 in range(0, N, 64):
        if forget in CARRIED and j0 > 0:
            v[forget] = INITIAL[forget]

        def a_of(j):
            k = j - c
            return int(agree[k]) if (j > 0 and k >= 0 and j < N) else 0xFFFFFFFF

        def st_of(j):
            k = j - c
            return int(status[k]) if (k >= 0 and j < N) else 1
        inn = [j0 + l < N for l in L]
        u = [inn[l] and st_of(j0 + l) > 0 for l in L]
        ub = ballot(u)
        if N - 1 - j0 < 64 and not (forget == "last_u" and j0 > 0):
            last_u = bool((ub >> (N - 1 - j0)) & 1)
        u_prev = [v["prev_u"] if l == 0 else bool((ub >> (l - 1)) & 1) for l in L]
        brk = [inn[l] and (j0 + l == 0 or not u_prev[l] or (j0 + l >= c and a_of(j0 + l) * 1000 < min_agree * NCELLS)) for l in L]
        bball = ballot(brk)
        run = []
        for l in L:
            bb = bball & ((1 << (l + 1)) - 1)
            run.append(j0 + 63 - clz64(bb) if bb else v["run_carry"])
        start = [u[l] and (j0 + l - run[l]) % max_group == 0 for l in L]
        sb = ballot(start)
        idv = [v["starts_carry"] + popc(sb & ((1 << (l + 1)) - 1)) - 1 if u[l] else -1 for l in L]
        v["run_carry"] = run[63]
        v["starts_carry"] += popc(sb)
        id_prev = [v["prev_id"] if l == 0 else idv[l - 1] for l in L]
        head = [idv[l] >= 0 and (j0 + l == 0 or id_prev[l] != idv[l]) for l in L]
        member = [idv[l] >= 0 for l in L]
        mb, hball = ballot(member), ballot(head)
        before = [v["mem_carry"] + popc(mb & ((1 << l) - 1)) for l in L]
        base = []
        for l in L:
            hb = hball & ((1 << (l + 1)) - 1)
            base.append(before[63 - clz64(hb)] if hb else v["base_carry"])
        for l in L:
            j = j0 + l
            if inn[l] and j >= c:
                groups[j - c] = idv[l]
            if member[l]:
                gmem[(idv[l], before[l] - base[l])] = j
                gcount[idv[l]] = gcount.get(idv[l], 0) + 1
            top = max(top, idv[l])
        v["prev_id"], v["prev_u"] = idv[63], u[63]
        v["mem_carry"] += popc(mb)
        v["base_carry"] = base[63]
    last_size = v["mem_carry"] - v["base_carry"] if top >= 0 else 0
    opn = (not flush) and top >= 0 and last_u and last_size < max_group
    return groups, gmem, gcount, (top if opn else top + 1), (last_size if opn else 0)


def walk(agree, status, min_agree, max_group, forget=None):
    """k_group_walk, groups_in == nullptr: agree[k] = agree(k, k + 1). -> groups, gmem, gcount, the group count"""
    groups, gmem, gcount, ng, _ = walk_stream(np.concatenate([[0], agree]), status, 0, min_agree, max_group, True, forget)
    return groups, gmem, gcount, ng


def plain_agrees(case, forget=None, usable=None):
    """does the simulated k_group_walk give the rule's groups, member table and count on this case?"""
    name, cap = case
    sym, col = GW.synthetic_cells(GW.RUN_LISTS[name])
    n = len(sym)
    usable = np.ones(n, bool) if usable is None else usable
    want = CM.group_captures(sym, col, usable=usable, min_agree_permille=GW.AGREE_3, max_group=cap)
    min_agree, max_group = CM.resolve(GW.AGREE_3, cap)
    groups, gmem, gcount, ng = walk(CM.agree(sym, col), usable.astype(int), min_agree, max_group, forget)
    ok = (groups == want).all() and ng == CM.n_groups(want)
    for g in range(CM.n_groups(want)):
        mem = CM.members(want, g)
        ok = ok and [gmem.get((g, r)) for r in range(len(mem))] == mem and gcount.get(g) == len(mem)
    return bool(ok) and len(gmem) == int((want >= 0).sum())


def stream_calls(case):
    """the calls of a stream case: [(lo, n, flush)]; the last call and a call without captures are flushed"""
    name, cap, sizes = case
    out, lo = [], 0
    for i, n in enumerate(sizes):
        out.append((lo, n, i == len(sizes) - 1 or n == 0))
        lo += n
    assert lo == sum(r[0] for r in GW.RUN_LISTS[name])
    return out


def stream_facts(case, usable=None, forget=None):
    """the rule over a stream case, call by call, and whether the simulated k_group_walk_stream agrees with it.
    -> [dict(c, n, N, ending, lane, head_step, last_step, flush_only, agrees)]"""
    name, cap, sizes = case
    sym, col = GW.synthetic_cells(GW.RUN_LISTS[name])
    total = len(sym)
    usable = np.ones(total, bool) if usable is None else usable
    a_all = CM.agree(sym, col)
    min_agree, max_group = CM.resolve(GW.AGREE_3, cap)
    model = SM.StreamModel(GW.AGREE_3, cap)
    facts, c = [], 0
    open_src = []                                        # the carried members, (call, index), slot by slot
    for call, (lo, n, flush) in enumerate(stream_calls(case)):
        want, closed, gsizes = model.call(sym[lo:lo + n], col[lo:lo + n], usable[lo:lo + n], flush=flush)
        still = [src for _, _, src in model.open]
        agree = np.array([a_all[lo + k - 1] if lo + k > 0 else 0 for k in range(n)], np.int64)
        groups, gmem, gcount, ng, osz = walk_stream(agree, usable[lo:lo + n].astype(int), c, min_agree, max_group, flush, forget)
        src_of = lambda j: open_src[j] if j < c else (call, j - c)      # noqa: E731
        ok = ng == len(closed) and osz == len(still)
        for k in range(n):
            w = int(want[k])
            ok = ok and int(groups[k]) == (ng if w == SM.GROUP_OPEN else w)
        for g, mem in enumerate(closed + ([still] if still else [])):
            got = [gmem.get((g, r)) for r in range(len(mem))]
            ok = ok and None not in got and [src_of(j) for j in got] == mem and gcount.get(g) == len(mem)
        ok = ok and len(gmem) == sum(map(len, closed)) + len(still)
        N = c + n
        last_usable = n > 0 and bool(usable[lo + n - 1])
        if n == 0:
            ending = "flush"
        elif not last_usable:
            ending = "unusable"
        elif still and not flush:
            ending = "open"
        elif closed and len(closed[-1]) == max_group and closed[-1][-1] == (call, n - 1):
            ending = "cap"
        else:
            ending = "other"
        # the virtual index of the open group's head: its members are the last len(still) virtual captures
        head_step = (N - len(still)) // 64 if still else None
        facts.append(dict(c=c, n=n, N=N, ending=ending, lane=(N - 1) % 64 if N else None, head_step=head_step, last_step=(N - 1) // 64 if N else None,
                          flush_only=n == 0, agrees=bool(ok), flush=flush))
        open_src, c = still, len(still)
    return facts


# ------------------------------------------------------------------------------------------------ 1. the shapes
def _grouping(name, cap):
    sym, col = GW.synthetic_cells(GW.RUN_LISTS[name])
    return CM.group_captures(sym, col, min_agree_permille=GW.AGREE_3, max_group=cap)


def _straddles(groups, edge, each_side=2):
    """a group with at least `each_side` members at or below edge and as many above it"""
    for g in range(CM.n_groups(groups)):
        m = np.array(CM.members(groups, g))
        if (m <= edge).sum() >= each_side and (m > edge).sum() >= each_side:
            return m.tolist()
    return None


def test_every_case_is_listed_once_and_names_a_run_list():
    assert len(set(GW.WALK_CASES)) == len(GW.WALK_CASES) and all(name in GW.RUN_LISTS for name, _ in GW.WALK_CASES)
    assert {cap for _, cap in GW.WALK_CASES} == {0, 1, 3, 8}
    assert CM.resolve(0, 0)[1] == 4
    for runs in GW.RUN_LISTS.values():
        assert all(length >= 1 for length, _ in runs)


def test_straddling_groups():
    for cap in (0, 8):
        assert ("straddle", cap) in GW.WALK_CASES
        g = _grouping("straddle", cap)
        assert _straddles(g, 63) == [62, 63, 64, 65]
        assert _straddles(g, 127) == [126, 127, 128, 129]
        # these are the groups whose recovery the device test asserts, made of differently damaged captures
        _, variant, _ = GW.expand(GW.RUNS_STRADDLE)
        for first in GW.RECOVERING[("straddle", cap)]:
            m = CM.members(g, int(g[first]))
            assert m[0] == first and set(variant[m].tolist()) == {1, 2}
    assert _straddles(_grouping("straddle", 8), 191, each_side=4) == list(range(188, 196))
    assert GW.RECOVERING[("straddle", 8)][-1] == 188


def test_breaks_at_a_step_edge():
    assert ("head64", 0) in GW.WALK_CASES and ("head63", 3) in GW.WALK_CASES
    g = _grouping("head64", 0)
    _, _, run = GW.expand(GW.RUNS_HEAD_64)
    assert g[64] != g[63] and run[64] != run[63] and CM.members(g, int(g[64])) == [64, 65, 66]      # a break, not the cap
    for cap in (3, 0):
        g = _grouping("head63", cap)
        assert g[63] != g[62] and CM.members(g, int(g[63])) == [63, 64, 65]


def test_cap_phase_across_a_step():
    frame, _, run = GW.expand(GW.RUNS_LONG)
    long_run = int(run[61])
    first, last = int(np.flatnonzero(run == long_run)[0]), int(np.flatnonzero(run == long_run)[-1])
    assert (first, last) == (61, 135) and first < 64 and last - first + 1 > 64          # steps 64 .. 127 hold no break
    for cap in (3, 1, 0, 8):
        assert ("long", cap) in GW.WALK_CASES
        size = CM.resolve(0, cap)[1]
        assert last - first + 1 > 2 * size
        g = _grouping("long", cap)
        heads = [k for k in range(first, last + 1) if g[k] != g[k - 1]]
        assert heads == list(range(first, last + 1, size))                              # the cap counts from the run's start ...
        if size > 1:
            assert first % size != 0 and any(h % size != 0 for h in heads if h >= 64)   # ... which a walk that lost it would not
    assert 64 % 3 != 0


# ------------------------------------------------------------------------------------------------ 2. and 3. the plain walk
@pytest.mark.parametrize("case", GW.WALK_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_the_simulated_walk_reproduces_the_rule(case):
    assert plain_agrees(case)


@pytest.mark.parametrize("cap", GW.CAPTURE_CAPS)
def test_the_simulated_walk_reproduces_the_rule_with_blank_captures(cap):
    usable = GW.capture_usable()
    assert not usable[[63, 64, 127]].any() and not usable[190:194].any() and usable[189] and usable[194] and usable.sum() == len(usable) - 7
    assert plain_agrees(("straddle", cap), usable=usable)
    assert GW.CAPTURE_RUNS is GW.RUNS_STRADDLE


@pytest.mark.parametrize("forget", CARRIED)
def test_a_forgotten_variable_changes_the_plain_walk(forget):
    differs = [case for case in GW.WALK_CASES if not plain_agrees(case, forget=forget)]
    print(forget, "differs on", differs)
    assert differs


# ------------------------------------------------------------------------------------------------ the stream walk
def _usable_of(case_list):
    return GW.capture_usable() if case_list is GW.STREAM_CAPTURE_CASES else None


def _all_stream_facts(forget=None):
    out = []
    for cases in (GW.STREAM_CASES, GW.STREAM_CAPTURE_CASES):
        for case in cases:
            out.append((case, stream_facts(case, usable=_usable_of(cases), forget=forget)))
    return out


def test_the_simulated_stream_walk_reproduces_the_rule():
    for case, facts in _all_stream_facts():
        assert all(f["agrees"] for f in facts), (case, [i for i, f in enumerate(facts) if not f["agrees"]])


@pytest.mark.parametrize("forget", CARRIED + ("last_u",))
def test_a_forgotten_variable_changes_the_stream_walk(forget):
    differs = [case[:2] for case, facts in _all_stream_facts(forget) if not all(f["agrees"] for f in facts)]
    print(forget, "differs on", differs)
    assert differs


def test_a_stream_sequence_closes_the_groups_of_one_plain_call():
    """(a flush-only call in the middle of a sequence falls between two runs, so it splits no group the plain call would form)"""
    for cases in (GW.STREAM_CASES, GW.STREAM_CAPTURE_CASES):
        for name, cap, sizes in cases:
            sym, col = GW.synthetic_cells(GW.RUN_LISTS[name])
            usable = np.ones(len(sym), bool) if _usable_of(cases) is None else _usable_of(cases)
            plain = CM.group_captures(sym, col, usable=usable, min_agree_permille=GW.AGREE_3, max_group=cap)
            model, lo, closed = SM.StreamModel(GW.AGREE_3, cap), [0], []
            for at, n, flush in stream_calls((name, cap, sizes)):
                lo.append(at)
                closed += [[lo[c + 1] + k for c, k in g] for g in model.call(sym[at:at + n], col[at:at + n], usable[at:at + n], flush=flush)[1]]
            assert closed == [CM.members(plain, g) for g in range(CM.n_groups(plain))], (name, cap, sizes)


def test_stream_calls_cross_the_steps_with_carried_members():
    facts = [(case, f) for case, fs in _all_stream_facts() for f in fs]
    for case, f in facts:
        assert f["c"] <= CM.resolve(0, case[1])[1] - 1
    # the virtual batch crosses 64 and 128 with 1, 2 and max_group - 1 members carried in
    for want_c in ("1", "2", "cap - 1"):
        hit = [case for case, f in facts if f["N"] > 128 and f["c"] == (CM.resolve(0, case[1])[1] - 1 if want_c == "cap - 1" else int(want_c))]
        assert hit, want_c
    assert any(f["c"] >= 3 and f["N"] > 128 for _, f in facts)                 # (cap - 1 is not one of 1 and 2 everywhere)
    # ... and ends at 64, 65 and 128 exactly, each with carried members
    for N in (64, 65, 128):
        assert any(f["N"] == N and f["c"] > 0 for _, f in facts), N


def test_stream_calls_end_every_way_at_lane_63_and_at_lane_0():
    facts = [f for _, fs in _all_stream_facts() for f in fs]
    for ending in ("open", "cap", "unusable"):
        for lane in (63, 0):
            assert any(f["ending"] == ending and f["lane"] == lane and f["N"] >= 64 and not f["flush"] for f in facts), (ending, lane)


def test_an_open_group_straddles_a_step_and_a_flush_only_call_follows_a_boundary():
    straddling = flushed = False
    for _, fs in _all_stream_facts():
        for i, f in enumerate(fs):
            straddling = straddling or (f["ending"] == "open" and f["head_step"] < f["last_step"])
            if f["flush_only"]:
                before = fs[i - 1]
                flushed = flushed or (before["ending"] == "open" and before["lane"] in (63, 0) and before["N"] >= 64 and f["c"] > 0)
    assert straddling and flushed
