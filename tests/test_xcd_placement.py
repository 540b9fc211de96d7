"""CPU: which windows of a cost launch share an XCD's L2 (deciphon_amd/csrc/dcp_types.h, "which XCD's L2 serves which
windows"; dcp_xcd_eighths_entry_of and dcp_xcd_placement_of in include/deciphon_host.h).

The eighths map: workgroup b runs on XCD b % 8, and XCD x walks the x-th contiguous eighth of the list -- a bijection
on [0, n) for every n, workgroups b and b + 8 on neighbouring entries.

The rule: the launches of the headline step that hold 500 windows per profile of 2.1-3.5 MB tables (8500, 5000, 2000
and 2000 workgroups) take the eighths, a launch of one profile keeps the plain order, and so does a launch whose tables
fit one L2 together."""
import pytest

from deciphon_amd import host

XCDS = 8
SIMDS_PER_XCD = 32 * 4  # 32 compute units of four SIMDs


def table_bytes(columns):
    return 1364 * (columns + 4) * 4  # every code's row: a header of four floats and the columns the kernel reads


@pytest.mark.parametrize("n", list(range(1, 71)) + [500, 2000, 8500, 16383, 16384, 20500, (1 << 17) + 5])
def test_eighths_map(n):
    entry = [host.xcd_eighths_entry(b, n) for b in range(n)]
    assert sorted(entry) == list(range(n))  # no window dropped, none scored twice
    for b in range(n - XCDS):
        assert entry[b + XCDS] == entry[b] + 1  # an XCD walks its share in list order
    shares = []
    for x in range(min(XCDS, n)):
        own = entry[x::XCDS]
        assert own == list(range(own[0], own[0] + len(own)))  # one contiguous range per XCD
        shares.append(len(own))
    assert max(shares) - min(shares) <= 1 and sum(shares) == n
    if n >= XCDS:
        firsts = [entry[x] for x in range(XCDS)]
        assert firsts == sorted(firsts) and firsts[0] == 0  # XCD x has the x-th eighth


def test_eighths_map_refuses_workgroups_outside_the_launch():
    for b, n in ((-1, 8), (8, 8), (0, 0)):
        with pytest.raises(ValueError):
            host.xcd_eighths_entry(b, n)


# the headline step's big-table launches: (workgroups, columns the kernel reads, wavefronts per SIMD it is compiled for)
HEADLINE_BIG = {
    "(6,1) 17 profiles": (8500, 384, 3),
    "(7,1) 10 profiles": (5000, 448, 2),
    "(8,1) 4 profiles": (2000, 512, 2),
    "(10,1) 4 profiles": (2000, 640, 2),
}


@pytest.mark.parametrize("name", sorted(HEADLINE_BIG))
def test_rule_takes_eighths_for_the_headline_big_tables(name):
    workgroups, columns, waves = HEADLINE_BIG[name]
    assert 2.1e6 <= table_bytes(columns) <= 3.6e6
    assert host.xcd_placement(workgroups, 500, table_bytes(columns), waves * SIMDS_PER_XCD) == host.PLACE_EIGHTHS


def test_rule_keeps_what_the_large_launches_had():
    # (5,1): 41 profiles, 20 500 workgroups, 1.7 MB tables, three wavefronts per SIMD
    assert host.xcd_placement(20500, 500, table_bytes(320), 3 * SIMDS_PER_XCD) == host.PLACE_EIGHTHS


def test_rule_keeps_plain_order():
    # one profile ((6,2) at K = 679: two wavefronts per workgroup, 3.7 MB): its table is in every L2 either way
    assert host.xcd_placement(500, 500, table_bytes(768), SIMDS_PER_XCD) == host.PLACE_PLAIN
    # three profiles of 1000 windows, 1.07 MB tables: all of them fit one L2
    assert 3 * table_bytes(192) < 4 << 20
    assert host.xcd_placement(3000, 1000, table_bytes(192), 5 * SIMDS_PER_XCD) == host.PLACE_PLAIN
    # a window or two per profile, as a small scan has: an eighth of a tiny launch still sees every profile it holds
    assert host.xcd_placement(8, 4, table_bytes(384), 3 * SIMDS_PER_XCD) == host.PLACE_PLAIN
    # nothing known about the list (windows per profile 0), an empty launch, no occupancy
    assert host.xcd_placement(8500, 0, table_bytes(384), 3 * SIMDS_PER_XCD) == host.PLACE_PLAIN
    assert host.xcd_placement(0, 500, table_bytes(384), 3 * SIMDS_PER_XCD) == host.PLACE_PLAIN
    assert host.xcd_placement(8500, 500, table_bytes(384), 0) == host.PLACE_PLAIN


def test_rule_large_database_leg():
    # 100 windows per profile: a launch under the old threshold put about twenty tables into each L2
    assert host.xcd_placement(12000, 100, table_bytes(384), 3 * SIMDS_PER_XCD) == host.PLACE_EIGHTHS
