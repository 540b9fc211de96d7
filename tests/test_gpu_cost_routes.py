"""GPU: every request of the route table (tests/cost_route_cases.py) through Engine.cost.  The engine itself says which
kernels the request ran (Engine.last_cost_launches: the launches of its last cost pass) and that must EQUAL the launches
the table states -- a request that took another kernel fails here whatever its scores are -- and every (null, alt) equals
the oracle's bit for bit.  One test per request, named by its route, so a failure names the kernel:

    pack_lds[s], pack[s]             every pack shape, rows from LDS and from global memory
    class[c]/plain, /eighths         dcp_cost_kernel<Q, W> of classes 0..6 under either order of the launch
    narrow[c]/plain, /eighths        the narrow kernels <5,1>, <7,1>, <10,1>
    fused/class[c]                   dcp_cost_kernel_fused on the windows of class c (its body for Q = c + 1)
    the four threshold requests      fused at 16384 windows (its eighths order), per class at 16385, 16384 packs twice

A window that is sent down several routes must come back with the same words from each (the first route's result is kept
and compared), so the oracle is asked once per window.  One request per route also goes through cost_hits_begin twice in a
row and cost_hits_end twice -- both buffer sets --: the same launches, and hit lists that are the host's filter of the
same scores.  Nothing here rests on a tolerance."""
import numpy as np
import pytest

import cost_route_cases as crc
from test_gpu_delete_runs import xtrans

pytestmark = pytest.mark.gpu


def _requests():
    try:
        return crc.table()[0]
    except ImportError as e:  # the library is not built: every test says so (there is no fallback)
        return [e]


REQUESTS = _requests()


@pytest.fixture(scope="module")
def state(engine):
    """loaded: the Load the engine holds; ref: the oracle's bits per (load, oracle profile, read, start, stop);
    seen: per (load, profile, read, start, stop) the first route that scored the window and its bits"""
    st = dict(loaded=None, profs=None, reads=None, ref={}, seen={})
    yield st
    engine.set_xtrans_table(np.zeros((0, 13), np.float32))


def ensure_loaded(engine, orc, st, load):
    if st["loaded"] is load:
        return
    st["loaded"] = None
    profs, reads = load.materialise()
    engine.clear_profiles()
    for p in profs:
        engine.add_profile(p.K, p.trans, p.match, p.null, p.bg)
    engine.commit()
    engine.set_sequences(reads)
    engine.set_mode(True, False)
    table = np.zeros((0, 13), np.float32)
    if load.quant:  # as tests/test_gpu_delete_runs.py load() sets it
        smax = max(len(r) // 3 for r in reads) + 1
        table = np.zeros((smax + 1, 13), np.float32)
        for s in range(1, smax + 1):
            table[s] = (np.round(orc.xtrans(s, True, False) / load.quant) * load.quant).astype(np.float32)
    engine.set_xtrans_table(table)
    st.update(loaded=load, profs=profs, reads=reads)


def reference(orc, st, load, wins):
    """uint32[n][2]: the oracle's (null, cost) words of every window, each distinct window computed once per session"""
    keyed = wins.copy()
    keyed[:, 0] = np.array([load.oracle_profile(p) for p in range(len(load.profiles))], np.int32)[wins[:, 0]]
    uniq, inv = np.unique(keyed, axis=0, return_inverse=True)
    out = np.zeros((len(uniq), 2), np.float32)
    for j, (pi, si, a, b) in enumerate(uniq.tolist()):
        key = (load.name, pi, si, a, b)
        if key not in st["ref"]:
            seq = np.ascontiguousarray(st["reads"][si][a:b])
            xt = xtrans(orc, len(seq), load.quant)
            st["ref"][key] = (orc.null(st["profs"][pi], xt, seq), orc.cost(st["profs"][pi], xt, seq))
        out[j] = st["ref"][key]
    return out.view(np.uint32)[inv.reshape(-1)]


def host_filter(nul, alt):
    """process_window's filter (c-core/thread.c:118-121) over these scores"""
    lrt = (np.float32(-2.0) * ((-nul) - (-alt))).astype(np.float32)
    keep = np.nonzero(np.isfinite(lrt) & (lrt >= 0))[0].astype(np.int32)
    return keep, lrt[keep]


@pytest.mark.parametrize("req", REQUESTS, ids=lambda r: getattr(r, "name", "library missing"))
def test_route(engine, orc, monkeypatch, state, req):
    if isinstance(req, Exception):
        raise req
    monkeypatch.delenv("DECIPHON_HIP_COST_ORDER", raising=False)
    for knob, value in req.knobs.items():
        if value is None:
            monkeypatch.delenv(knob, raising=False)
        else:
            monkeypatch.setenv(knob, value)
    ensure_loaded(engine, orc, state, req.load)
    wins = req.windows()
    nul, alt = engine.cost(wins)
    ran = engine.last_cost_launches()
    print(f"{req.name}: {len(wins)} windows;", ", ".join(f"{e['kernel']}[{e['index']}] {e['first']}+{e['count']}" for e in ran))
    assert ran == req.expect, (req.name, "the request took other kernels than the table states")

    got = np.stack([nul, alt], axis=1).view(np.uint32)
    want = reference(orc, state, req.load, wins)
    bad = np.nonzero((got != want).any(axis=1))[0]
    Ks = req.load.core_sizes()
    assert len(bad) == 0, (req.name, f"{len(bad)} of {len(wins)} windows differ from the oracle; the first: K, window, got, want",
                           [(Ks[wins[i][0]], wins[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:4]])

    # the same window down another route: the same words
    uniq, first = np.unique(wins, axis=0, return_index=True)
    for w, i in zip(uniq.tolist(), first.tolist()):
        route, words = state["seen"].setdefault((req.load.name, *w), (req.name, got[i].tolist()))
        assert got[i].tolist() == words, (req.name, "against", route, Ks[w[0]], w)

    if req.hits:
        engine.cost_hits_begin(wins)
        engine.cost_hits_begin(wins)
        try:
            assert engine.last_cost_launches() == req.expect, (req.name, "two batches in flight")
        finally:
            both = [engine.cost_hits_end(), engine.cost_hits_end()]
        keep, lrt = host_filter(nul, alt)
        for batch, (idx, hit_lrt) in enumerate(both):
            assert np.array_equal(idx, keep), (req.name, "hit windows of batch", batch)
            assert np.array_equal(hit_lrt.view(np.uint32), lrt.view(np.uint32)), (req.name, "hit lrt of batch", batch)
