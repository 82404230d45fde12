"""The lists of walk_cases.py before a GPU sees them: every builder's tile lower bound for the wave counts
of the host-tier launch (128 workgroups) and of 8 workgroups per CU on 256 and on 304 CUs, the claim that
no op writes what another touches, and the models against the library's host path on a CPU pair (one
daemon, and striped over three owners), byte for byte."""
import pytest

import walk_cases
from oncilla_amd import api
from walk_cases import BUILDERS, HOST_WAVES, UNIT, WAVES, check_disjoint, check_skips, need, op_plan, row_plan, wave_ranges

N_DAEMONS = [1, 4]


@pytest.fixture(params=N_DAEMONS)
def client(request, mesh_factory, monkeypatch):
    monkeypatch.setenv("OCM_NO_GPU", "1")
    m = mesh_factory(request.param, policy="stripe")
    with api.Client(daemon_rank=0, ns=m.ns) as c:
        c.n_daemons = request.param
        yield c


def test_wave_counts():
    assert WAVES == (512, 8192, 9728) and HOST_WAVES == 512 and [need(w) for w in WAVES] == [1025, 16385, 19457]


def _bad_rows(tag):
    s = walk_cases.SKIP_OPS[tag]
    n = walk_cases.SKIP_ROWS[tag]
    return [not (0 <= l < walk_cases.WIN and 0 <= r < walk_cases.WIN)
            for l, r in zip(s["lidx"] or [0] * n, s["ridx"] or [0] * n)]


MULTIS = (walk_cases.MULTI_BYTE_TILES, walk_cases.MULTI_FIXED_TILES)


@pytest.mark.parametrize("multi", MULTIS)
@pytest.mark.parametrize("waves", WAVES)
def test_row_plans_have_their_content_in_the_middle(waves, multi):
    plan = row_plan(waves, multi)
    assert len(plan) >= 40 and sum(r for r, _, _ in plan) >= need(waves)
    total, at, mid = sum(r for r, _, _ in plan), 0, []
    for op in plan:  # the middle: the ops that start between a quarter and three quarters of the rows
        if total // 4 <= at < 3 * total // 4:
            mid.append(op)
        at += op[0]
    assert sum(r for r, c, t in mid if c == 3 and not t) >= multi and sum(r for r, c, _ in mid if c == 2) >= walk_cases.MULTI2
    assert [t for _, _, t in mid if t] == ["S", "S", "S", "E", "L"]                           # the ops with skipped rows
    assert any(a[0] == 0 and b[0] == 0 for a, b in zip(mid, mid[1:]))                         # empty ops, two side by side
    assert any(all(r == 1 for r, _, _ in mid[i:i + 3]) for i in range(len(mid) - 2))          # a run of one-row ops
    after_e = plan[[t for _, _, t in plan].index("E") + 1]
    assert after_e[0] > 0 and _bad_rows("E")[-1]                                              # a skipped last row, then an op
    for tag in walk_cases.SKIP_OPS:  # every skipped row is followed by an in-range one
        bad = _bad_rows(tag)
        assert any(bad) and not any(a and b for a, b in zip(bad, bad[1:]))
    for ids, offsets in walk_cases.BAG_SKIP_OPS.values():  # and so is every skipped id of the bag ops, in its bag or the next
        bad = [not 0 <= v < walk_cases.WIN for v in ids]
        assert any(bad) and not any(a and b for a, b in zip(bad, bad[1:])) and offsets[-1] == len(ids)
    assert {t: n for n, _, t in row_plan(waves, multi, walk_cases.BAG_SKIP_ROWS) if t} == walk_cases.BAG_SKIP_ROWS


@pytest.mark.parametrize("multi", MULTIS)
@pytest.mark.parametrize("waves", WAVES)
def test_waves_start_and_end_inside_rows_skipped_ones_too(waves, multi):
    # For the kinds whose ops have rows of a fixed number of tiles (strided, indexed and their converting forms: the
    # plan's tiles per row are theirs), the tile ranges of the waves (list_wave_range) against the plan's tile
    # positions. A condition on the list, like the lower bound: what it asks for is what makes a wave enter a row at
    # piece k > 0 (where a skipped row must not be counted again) and carry a skipped row's state into the next row.
    plan = row_plan(waves, multi)
    rows, t = [], 0  # (first tile, tiles, skipped, op number) of every row
    for n, (r, c, tag) in enumerate(plan):
        bad = _bad_rows(tag) if tag else [False] * r
        for j in range(r):
            rows.append((t, c, bad[j], n))
            t += c
    ranges = wave_ranges(t, waves)
    assert len(ranges) <= waves and all(t1 - t0 >= 3 for t0, t1 in ranges[:-1])
    starts = {t0: t1 for t0, t1 in ranges}
    entered = {(c, k, bad) for first, c, bad, _ in rows for k in range(1, c) if first + k in starts}
    # waves start at every piece k > 0 of rows of 2 and of 3 tiles, and of SKIPPED rows of 3 tiles: the wave before
    # them leaves that row half done
    assert {(2, 1, False), (3, 1, False), (3, 2, False), (3, 1, True), (3, 2, True)} <= entered
    # a skipped row of 3 tiles and its in-range successor (of the same op) inside one wave, the skipped row entered
    # at a later piece (this wave must not count it) and, where a wave has more than three tiles, at piece 0 (it must)
    carried = set()
    for (first, c, bad, n), (nfirst, _, nbad, nn) in zip(rows, rows[1:]):
        if bad and c == 3 and not nbad and nn == n:
            carried |= {k for k in range(c) if first + k in starts and starts[first + k] > nfirst}
            carried |= {0 for t0, t1 in ranges if t0 < first and t1 > nfirst}
    # (a wave of three tiles that enters a row of three at piece 0 ends with it: piece 0 needs a larger share)
    assert {1, 2} <= carried and (0 in carried or -(-t // waves) == 3)
    # op changes inside a wave: some wave covers tiles of at least three ops
    op_of = [n for first, c, _, n in rows for _ in range(c)]
    assert max(len(set(op_of[t0:t1])) for t0, t1 in ranges) >= 3


@pytest.mark.parametrize("multi", MULTIS)
@pytest.mark.parametrize("waves", WAVES)
def test_op_plans_have_their_content_in_the_middle(waves, multi):
    ops = op_plan(waves, multi)
    assert sum(1 for c in ops if c) == need(waves) and len(ops) >= 40
    n = len(ops)
    mid = ops[n // 4:3 * n // 4]
    assert sum(1 for v in mid if v == 3) >= multi and sum(1 for v in mid if v == 2) >= walk_cases.MULTI2
    assert any(a == 0 and b == 0 for a, b in zip(mid, mid[1:]))
    # the kinds whose tiles are a fixed number of elements (converting, accumulate) give an op of the plan exactly
    # its tiles: waves start at every piece k > 0 of ops of 2 and of 3 tiles, and some wave crosses three ops and more
    first, t = [], 0
    for c in ops:
        first.append(t)
        t += c
    ranges = wave_ranges(t, waves)
    starts = {t0 for t0, _ in ranges}
    assert {(2, 1), (3, 1), (3, 2)} <= {(c, k) for f, c in zip(first, ops) for k in range(1, c) if f + k in starts}
    assert all(t1 - t0 >= 3 for t0, t1 in ranges[:-1])


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("kind", list(BUILDERS))
def test_lower_bound_and_disjoint_ranges(kind, waves):
    case = BUILDERS[kind](waves)
    assert case.lower_bound >= need(waves)
    assert case.lower_bound <= need(waves) + 1200                         # and the lists stay small
    assert case.local_bytes <= 4 << 20 and case.remote_bytes <= 4 << 20
    check_disjoint(case)


@pytest.mark.parametrize("kind", list(BUILDERS))
def test_models_equal_the_host_path(client, kind):
    case = BUILDERS[kind](HOST_WAVES)
    assert case.lower_bound >= need(HOST_WAVES)
    a = client.alloc(api.OCM_REMOTE_RDMA, local_bytes=case.local_bytes, remote_bytes=case.remote_bytes,
                     flags=api.OCM_ALLOC_STRIPE, stripe_unit=UNIT)
    assert len(a.remote_info()["extents"]) == (1 if client.n_daemons == 1 else 3)
    for async_ in (False, True):
        before = api.indexed_counters()
        skipped, err = case.run(a, async_=async_)
        check_skips(case, skipped, err, async_, before, api.indexed_counters())
        a.wait()  # reported once
    a.free()
