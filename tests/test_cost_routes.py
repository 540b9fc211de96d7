"""CPU: what the route table of the cost pass holds (tests/cost_route_cases.py), and that the planner agrees with it
before a GPU is involved: every kernel cost_schedule can launch for profiles of up to 640 positions is some request's
expected launch, under either order where the kernel takes one; every (route, K at either end of the kernel's profiles)
cell holds windows of all four families; and host.cost_schedule(host.stage_plan(..)) under a request's knobs gives
exactly the launches the table states for it."""
import numpy as np

import cost_route_cases as crc
from deciphon_amd import host


def test_every_kernel_is_some_requests_launch():
    requests, _ = crc.table()
    shapes = host.engine_pack_shapes()
    seen = set()
    for r in requests:
        for e in r.expect:
            order = r.knobs["DECIPHON_HIP_XCD_PLACEMENT"] if e["kernel"] in ("class", "narrow") else None
            seen.add((e["kernel"], e["index"], order))
        if r.route and r.route.startswith("fused"):  # the fused kernel has one body per Q = 1..4 = class + 1
            seen.update(("fused body", host.engine_core_size(K)[2], None) for K in r.core_sizes())
    want = {("class", c, o) for c in range(7) for o in crc.PLACEMENTS}
    want |= {("narrow", c, o) for c in (4, 5, 6) for o in crc.PLACEMENTS}
    want |= {("fused", 0, None)} | {("fused body", c, None) for c in range(crc.FUSED_CLASSES)}
    want |= {("pack", s, None) for s in range(host.NUM_PACK_SHAPES)}
    want |= {("pack_lds", s, None) for s in range(host.NUM_PACK_SHAPES) if shapes[s][1]}
    assert len([s for s in range(host.NUM_PACK_SHAPES) if shapes[s][1]]) >= 1
    assert not want - seen, sorted(want - seen, key=str)
    # a request that pins a class or narrow route names its order; no other request forces one
    for r in requests:
        forced = r.knobs["DECIPHON_HIP_XCD_PLACEMENT"]
        assert (forced in crc.PLACEMENTS) == bool(r.route and r.route.split("[")[0] in ("class", "narrow")), r.name
        assert forced is None or r.route.endswith("/" + forced), r.name


def test_every_cell_holds_every_family():
    requests, ends = crc.table()
    cells = crc.cells(requests)
    routes = {r.route for r in requests if r.route}
    assert routes == set(ends), sorted(routes ^ set(ends))
    for route, Ks in sorted(ends.items()):
        assert 1 <= len(Ks) <= 2
        for K in sorted(Ks):
            cell = cells.get((route, K))
            assert cell is not None, f"no window of K = {K} on route {route}"
            assert all(cell[f] >= 1 for f in crc.FAMILIES), (route, K, cell)
    for (route, K), cell in cells.items():
        assert sum(cell.values()) >= 1, (route, K)
    for r in requests:
        n = len(r.windows())
        assert n >= 1 and (r.families is None or len(r.families) == n), r.name
        # nothing larger is needed: what differs between routes is the first and last rows and the exchange
        rows = r.windows()[:, 3] - r.windows()[:, 2]
        planted = np.array([f == "runs" for f in r.families]) if r.families else np.zeros(n, bool)
        assert rows.min() >= 1 and rows[~planted].max() <= 124, r.name
    # one request per route also goes through the batches in flight
    assert {r.route for r in requests if r.hits} == routes


def test_threshold_requests():
    requests, _ = crc.table()
    bulk = [r for r in requests if r.route is None]
    assert [len(r.windows()) for r in bulk] == [16384, 16385, 32768, 262144]
    for r in bulk:
        w = r.windows()
        assert len(r.load.reads) <= 32 and len(np.unique(w, axis=0)) <= 2 * 32
        assert set((w[:, 3] - w[:, 2]).tolist()) == set(range(5, 13)), r.name
    assert [e["kernel"] for e in bulk[0].expect] == ["fused"] and [e["kernel"] for e in bulk[1].expect] == ["class", "class"]
    assert [(e["kernel"], e["count"]) for r in bulk[2:] for e in r.expect] == [("pack", 16384)] * 2
    assert bulk[2].knobs["DECIPHON_HIP_PACK_LDS"] is None and bulk[3].knobs["DECIPHON_HIP_PACK_LDS"] == "0"


def test_the_planner_gives_the_tables_launches():
    requests, _ = crc.table()
    assert len(requests) >= 60
    for r in requests:
        profiles = [host.engine_core_size(K) for K in r.load.core_sizes()]
        seq_off = np.concatenate([[0], np.cumsum(r.load.read_lengths())]).astype(np.int64)
        plan = host.stage_plan(r.windows(), profiles, seq_off, pack=r.knobs["DECIPHON_HIP_PACK"] != "0",
                               pack_lds=r.knobs["DECIPHON_HIP_PACK_LDS"] != "0")
        got = host.cost_schedule(plan, narrow=r.knobs["DECIPHON_HIP_NARROW"] != "0")
        assert got == r.expect, (r.name, got, r.expect)
        assert all(v in (None, "0") for k, v in r.knobs.items() if k != "DECIPHON_HIP_XCD_PLACEMENT"), r.name
