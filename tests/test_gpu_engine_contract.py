"""GPU: the call-order contract of the engine API (include/deciphon_hip.h).  What is refused while cost batches are
outstanding, what ends the staged window list and the trellis of the last path pass, and -- whenever the engine does
give a result -- that it equals the CPU oracle's on the inputs in force when that result was defined.  Bit-exact:
scores as fp32 bit patterns, every path step, every trellis word.  Every test starts from a fresh engine."""
import copy
import os
import types

import numpy as np
import pytest

import deciphon_amd
from dcp_testlib import GOLDEN, bits, random_seq, synth_profile

pytestmark = pytest.mark.gpu

EFUNCUSE, EZEROSEQ = 8, 11
DCP = os.path.join(GOLDEN, "minifam.dcp")
# one profile per kernel class: packs (3, 40, 124), one wave (173), several (300, 640); quant=2.0 makes exact fp32
# ties common, pinf sprinkles +inf costs
SPEC = ((3, None, 0.0), (40, 2.0, 0.05), (124, None, 0.02), (173, 2.0, 0.0), (300, None, 0.05), (640, 2.0, 0.02))
STRIP_K = 4200  # beyond 4096: the strip class, whose literal path pass replays rows from a DP table
SHORT = 64  # the strip-class profile only ever meets reads this short


@pytest.fixture(scope="module")
def data(orc):
    from oracle.dcp_reader import read_dcp

    rng = np.random.default_rng(2026)
    d = types.SimpleNamespace()
    d.synth = [synth_profile(rng, K, q, p) for K, q, p in SPEC]
    d.strip = synth_profile(rng, STRIP_K)
    d.extra = synth_profile(rng, 60, 2.0, 0.02)

    def reads(lengths):
        r = [random_seq(rng, n) for n in lengths]
        for x in r[1:3]:  # a shared stretch: some windows hit (lrt >= 0), most of the short ones do not
            x[20 : 20 + min(200, len(x) - 20)] = r[0][20 : 20 + min(200, len(x) - 20)]
        return r

    d.reads = reads((600, 451, 300, 97, 37))
    d.other = reads((600, 451, 300, 97, 37))  # the same lengths, other bases
    d.resized = reads((520, 140, 61))
    # the walk's reads stay short: the oracle computes every result it checks
    d.walk_reads = [reads((300, 181, 64, 20)), reads((300, 181, 64, 20)), reads((250, 97, 33))]
    db = read_dcp(DCP)
    d.protein = db.proteins[0]
    d.minifam = [orc.setup_profile(p) for p in db.proteins]
    # a caller's own special transitions for amino lengths 0..149 (longer windows keep following the mode)
    d.table = np.stack([orc.xtrans(max(s, 1), True, False) + np.float32(0.5) for s in range(150)]).astype(np.float32)
    d.table2 = np.stack([orc.xtrans(max(s, 1), False, True) * np.float32(1.5) for s in range(40)]).astype(np.float32)
    d.cache = {}  # oracle results, shared by every test of the module (keys hold the profile objects above)
    return d


class Inputs:
    """The engine's inputs as the oracle sees them: profiles in engine order, reads, mode, xtrans override."""

    def __init__(self, orc, cache):
        self.orc, self.cache = orc, cache
        self.profiles, self.reads, self.mode, self.table = [], [], (True, False), None

    def copy(self):
        c = copy.copy(self)
        c.profiles, c.reads = list(self.profiles), list(self.reads)
        return c

    def xt(self, L):
        s = max(L // 3, 1)  # c-core/thread.c:112
        if self.table is not None and s < len(self.table):
            return self.table[s]
        return self.orc.xtrans(s, *self.mode)

    def _args(self, w):
        p, s, a, b = w
        return self.profiles[p], np.ascontiguousarray(self.reads[s][a:b]), self.xt(b - a)

    def _key(self, w, what):
        prof, seq, xt = self._args(w)
        return what, id(prof), seq.tobytes(), xt.tobytes()

    def cost(self, w):
        k = self._key(w, "cost")
        if k not in self.cache:
            prof, seq, xt = self._args(w)
            self.cache[k] = (self.orc.null(prof, xt, seq), self.orc.cost(prof, xt, seq))
        return self.cache[k]

    def path(self, w):
        """-> (score, xnodes, nodes, packed steps)"""
        k = self._key(w, "path")
        if k not in self.cache:
            prof, seq, xt = self._args(w)
            score, xn, nd = self.orc.path(prof, xt, seq)
            packed = np.zeros(0, np.uint32)
            if score < np.inf:  # no finite path: the engine gives 0 steps
                ids, sizes = self.orc.unzip(prof.K, len(seq), xn, nd)
                packed = ids.astype(np.uint32) | (sizes.astype(np.uint32) << np.uint32(16))
            self.cache[k] = (score, xn, nd, packed)
        return self.cache[k]


def check_cost(inp, wins, nul, alt, where):
    assert len(nul) == len(alt) == len(wins), where
    for i, w in enumerate(wins):
        n, a = inp.cost(w)
        assert bits(nul[i]) == bits(n) and bits(alt[i]) == bits(a), f"{where}: window {i} {w}"


def oracle_hits(inp, wins):
    """process_window's filter (c-core/thread.c:118-121) over the oracle's scores."""
    nul = np.array([inp.cost(w)[0] for w in wins], np.float32)
    alt = np.array([inp.cost(w)[1] for w in wins], np.float32)
    lrt = (np.float32(-2.0) * ((-nul) - (-alt))).astype(np.float32)
    keep = np.nonzero(np.isfinite(lrt) & (lrt >= 0))[0].astype(np.int32)
    return keep, lrt[keep]


def check_hits(inp, wins, got, where):
    keep, lrt = oracle_hits(inp, wins)
    assert np.array_equal(got[0], keep), f"{where}: hit windows {got[0]} != {keep}"
    assert np.array_equal(got[1].view(np.uint32), lrt.view(np.uint32)), f"{where}: hit lrt"


def steps_of(eng, i):
    return eng.path_steps_packed(i), np.float32(eng.lib.dcp_hip_path_score(eng.h, i))


def check_steps(inp, wins, eng, where):
    for i, w in enumerate(wins):
        score, _, _, packed = inp.path(w)
        got, got_score = steps_of(eng, i)
        assert bits(got_score) == bits(score), f"{where}: path score of window {i} {w}"
        assert np.array_equal(got, packed), f"{where}: path steps of window {i} {w}"


def check_trellis(inp, w, got, where):
    _, xn, nd, _ = inp.path(w)
    assert np.array_equal(got[0], xn) and np.array_equal(got[1], nd), f"{where}: trellis of {w}"


def expect(code, fn, *args, where=""):
    """fn(*args) with the return code the contract predicts: its result when that is 0."""
    if code == 0:
        try:
            return fn(*args)
        except deciphon_amd.HipError as e:
            raise AssertionError(f"{where}: refused with {e.code} ({e}), expected to succeed") from None
    with pytest.raises(deciphon_amd.HipError) as e:
        fn(*args)
    assert e.value.code == code, f"{where}: code {e.value.code} ({e.value}), expected {code}"
    return None


def refused(fn, *args, where=""):
    expect(EFUNCUSE, fn, *args, where=where)


def setup(eng, inp, profs, reads, mode=(True, False)):
    for p in profs:
        eng.add_profile(p.K, p.trans, p.match, p.null, p.bg)
    eng.commit()
    eng.set_sequences(reads)
    eng.set_mode(*mode)
    inp.profiles, inp.reads, inp.mode, inp.table = list(profs), list(reads), mode, None


def cost_windows(inp):
    """Every profile against every read, whole reads (the strip-class profile against the short ones only)."""
    return [(p, s, 0, len(r)) for p, prof in enumerate(inp.profiles) for s, r in enumerate(inp.reads)
            if prof.K <= 4096 or len(r) <= SHORT]


def path_windows(inp):
    """One window per profile: whole reads and tails of reads; the strip-class profile on the shortest read."""
    order = sorted(range(len(inp.reads)), key=lambda s: len(inp.reads[s]))
    out = []
    for p, prof in enumerate(inp.profiles):
        if prof.K > 4096:
            s = order[0]
            assert len(inp.reads[s]) <= SHORT
            out.append((p, s, 0, len(inp.reads[s])))
        else:
            s = p % len(inp.reads)
            L = len(inp.reads[s])
            out.append((p, s, 0 if p % 2 == 0 else L // 4, L))
    return out


# Every change of the inputs the header names, applied to the engine and to the oracle's view alike.
def _set_mode(eng, inp, d):
    inp.mode = (not inp.mode[0], inp.mode[1])
    eng.set_mode(*inp.mode)


def _set_mode_h3(eng, inp, d):
    inp.mode = (inp.mode[0], not inp.mode[1])
    eng.set_mode(*inp.mode)


def _set_xtrans_table(eng, inp, d):
    eng.set_xtrans_table(d.table)
    inp.table = d.table


def _clear_xtrans_table(eng, inp, d):
    eng.set_xtrans_table(np.zeros((0, 13), np.float32))
    inp.table = None


def _same_reads(eng, inp, d):
    eng.set_sequences(inp.reads)


def _other_reads(eng, inp, d):
    inp.reads = list(d.other if inp.reads[0] is not d.other[0] else d.reads)
    eng.set_sequences(inp.reads)


def _resized_reads(eng, inp, d):
    inp.reads = list(d.resized)
    eng.set_sequences(inp.reads)


def _add_profile(eng, inp, d):
    eng.add_profile(d.extra.K, d.extra.trans, d.extra.match, d.extra.null, d.extra.bg)
    inp.profiles.append(d.extra)


def _clear_and_readd(eng, inp, d):
    eng.clear_profiles()
    assert eng.num_profiles == 0
    inp.profiles = inp.profiles[::-1]  # the same count again, in another order: a stale list would pass its checks
    for p in inp.profiles:
        eng.add_profile(p.K, p.trans, p.match, p.null, p.bg)
    eng.commit()


def _commit(eng, inp, d):
    eng.commit()


def _load_dcp(eng, inp, d):
    eng.load_dcp(DCP)
    inp.profiles += d.minifam


MUTATORS = [("set_mode", _set_mode), ("set_mode hmmer3", _set_mode_h3), ("set_xtrans_table", _set_xtrans_table),
            ("set_xtrans_table rows=0", _clear_xtrans_table), ("set_sequences same reads", _same_reads),
            ("set_sequences other reads", _other_reads), ("set_sequences resized", _resized_reads),
            ("add_profile", _add_profile), ("clear_profiles + re-add", _clear_and_readd), ("commit", _commit),
            ("load_dcp", _load_dcp)]


# ---- the three breaks of the unguarded engine, each on its own ---------------------------------------------------

def test_cost_is_refused_while_only_the_second_batch_is_outstanding(orc, data):
    """Two _begins and one _end leave a batch outstanding in the second buffer set only: dcp_hip_cost is still a
    DCP_EFUNCUSE (the guard looks at every outstanding batch, not at the first buffer set)."""
    inp = Inputs(orc, data.cache)
    with deciphon_amd.Engine(0) as eng:
        setup(eng, inp, data.synth + [data.strip], data.reads)
        W = cost_windows(inp)
        A, B = W[:10], W
        eng.cost_hits_begin(A)
        eng.cost_hits_begin(B)
        got_a = eng.cost_hits_end()
        refused(eng.cost, A, where="cost with a batch outstanding in the second buffer set")
        got_b = eng.cost_hits_end()
        check_hits(inp, A, got_a, "first batch")
        check_hits(inp, B, got_b, "second batch")
        nul, alt = eng.cost(A)
        check_cost(inp, A, nul, alt, "cost once drained")


def test_set_mode_between_stage_and_run_staged_is_refused(orc, data):
    """The staged list was built for the old mode's special transitions: after dcp_hip_set_mode it is refused
    instead of returning the old mode's scores."""
    inp = Inputs(orc, data.cache)
    with deciphon_amd.Engine(0) as eng:
        setup(eng, inp, data.synth + [data.strip], data.reads)
        W = cost_windows(inp)
        eng.stage(W)
        eng.run_staged(1)
        check_cost(inp, W, *eng.fetch_staged(), "staged, first mode")
        _set_mode(eng, inp, data)
        refused(eng.run_staged, 1, where="run_staged after set_mode")
        refused(eng.fetch_staged, where="fetch_staged after set_mode")
        eng.stage(W)
        eng.run_staged(1)
        check_cost(inp, W, *eng.fetch_staged(), "staged again, other mode")


def test_set_sequences_between_path_and_trellis_is_refused(orc, data):
    """Reads of the same lengths replace the path's reads: the delayed trellis is refused (it would be the new reads'
    trellis) and the steps stay those of the path's own inputs."""
    inp = Inputs(orc, data.cache)
    with deciphon_amd.Engine(0) as eng:
        setup(eng, inp, data.synth + [data.strip], data.reads)
        P = path_windows(inp)
        eng.path(P, trellis=False)
        snap = inp.copy()
        check_steps(snap, P, eng, "path")
        _other_reads(eng, inp, data)
        for i in range(len(P)):
            refused(eng.path_trellis, i, where=f"trellis {i} after set_sequences")
        check_steps(snap, P, eng, "steps after the refused trellis")


# ---- 1. the refusal matrix ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("state", ["first set", "both sets", "second set"])
def test_refusals_while_batches_are_outstanding(orc, data, state):
    """In each outstanding state every call that changes the inputs or computes on the cost buffers is a
    DCP_EFUNCUSE and changes nothing; the read-only queries, dcp_hip_path (with its trellis) and dcp_hip_path_reserve
    go on.  Drained, each batch delivers what the one-call form and the oracle's filter give."""
    inp = Inputs(orc, data.cache)
    with deciphon_amd.Engine(0) as eng:
        setup(eng, inp, data.synth + [data.strip], data.reads)
        W = cost_windows(inp)
        A, B = W[::3], W
        pool = eng.pool_bytes
        eng.cost_hits_begin(A)
        got = []
        if state != "first set":
            eng.cost_hits_begin(B)
        if state == "second set":
            got.append(eng.cost_hits_end())
        pr, x = data.protein, data.extra
        calls = [("add_profile", eng.add_profile, (x.K, x.trans, x.match, x.null, x.bg)),
                 ("add_protein", eng.add_protein, (pr.core_size, pr.trans, pr.emission, pr.BMk, pr.null_emission,
                                                   pr.bg_emission)),
                 ("load_dcp", eng.load_dcp, (DCP,)), ("commit", eng.commit, ()),
                 ("clear_profiles", eng.clear_profiles, ()), ("set_sequences", eng.set_sequences, (data.other,)),
                 ("set_mode", eng.set_mode, (False, True)), ("set_xtrans_table", eng.set_xtrans_table, (data.table,)),
                 ("cost", eng.cost, (A,)), ("cost_hits", eng.cost_hits, (A,)),
                 ("cost_bench", eng.cost_bench, (A, 0, 1)), ("stage", eng.stage, (A,)),
                 ("run_staged", eng.run_staged, (1,)), ("fetch_staged", eng.fetch_staged, ())]
        if state == "both sets":
            calls.append(("a third cost_hits_begin", eng.cost_hits_begin, (A,)))
        for name, fn, args in calls:
            refused(fn, *args, where=f"{state}: {name}")
            assert eng.num_profiles == len(inp.profiles), f"{state}: {name} changed the profiles"
            assert eng.pool_bytes == pool, f"{state}: {name} changed the pool"
        # what goes on
        assert [eng.core_size(i) for i in range(len(inp.profiles))] == [p.K for p in inp.profiles]
        assert eng.core_size(len(inp.profiles)) == -1 and deciphon_amd.device_count() >= 1
        eng.path_reserve(64 << 20)
        P = path_windows(inp)
        paths = eng.path(P, trellis=True)
        check_steps(inp, P, eng, f"{state}: path")
        for i, w in enumerate(P):
            check_trellis(inp, w, (paths[i]["xnodes"], paths[i]["nodes"]), f"{state}: path")
            assert np.array_equal(paths[i]["literal_state_ids"], paths[i]["state_ids"])
        # drained
        while len(got) < (1 if state == "first set" else 2):
            got.append(eng.cost_hits_end())
        refused(eng.cost_hits_end, where=f"{state}: an _end with nothing outstanding")
        batches = [A] if state == "first set" else [A, B]
        for batch, g in zip(batches, got):
            one = eng.cost_hits(batch)
            assert np.array_equal(g[0], one[0]) and np.array_equal(g[1].view(np.uint32), one[1].view(np.uint32))
            check_hits(inp, batch, g, f"{state}: batch of {len(batch)}")
        assert len(oracle_hits(inp, B)[0]) > 0
        # and everything is accepted again
        nul, alt = eng.cost(A)
        check_cost(inp, A, nul, alt, f"{state}: cost once drained")
        eng.clear_profiles()
        assert eng.num_profiles == 0


# ---- 2. the staged list -------------------------------------------------------------------------------------------

def test_staged_list_runs_until_its_inputs_or_buffers_change(orc, data):
    inp = Inputs(orc, data.cache)
    with deciphon_amd.Engine(0) as eng:
        setup(eng, inp, data.synth + [data.strip], data.reads)
        W = cost_windows(inp)
        eng.stage(W)
        refused(eng.fetch_staged, where="fetch_staged before any run_staged")
        eng.run_staged(0)
        refused(eng.fetch_staged, where="fetch_staged after run_staged(0)")
        eng.run_staged(1)
        first = eng.fetch_staged()
        check_cost(inp, W, *first, "staged")
        # the same list, run and fetched again, and staged again: identical bits
        for again in ("run_staged(2)", "fetch twice", "staged anew"):
            if again == "staged anew":
                eng.stage(W)
                eng.run_staged(1)
            elif again == "run_staged(2)":
                eng.run_staged(2)
            got = eng.fetch_staged()
            for a, b in zip(first, got):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), again
        # a path pass has buffers of its own: the list stays
        P = path_windows(inp)
        eng.path(P, trellis=False)
        eng.path_trellis(0)
        eng.run_staged(1)
        check_cost(inp, W, *eng.fetch_staged(), "staged, after a path pass")
        # the cost calls reuse the list's buffers: each ends it
        few = W[:5]
        for name, call in (("cost", lambda: eng.cost(few)), ("cost_hits", lambda: eng.cost_hits(few)),
                           ("cost_hits_begin/_end", lambda: (eng.cost_hits_begin(few), eng.cost_hits_end())),
                           ("cost_bench", lambda: eng.cost_bench(few, 0, 1))):
            eng.stage(W)
            eng.run_staged(1)
            call()
            refused(eng.run_staged, 1, where=f"run_staged after {name}")
            refused(eng.fetch_staged, where=f"fetch_staged after {name}")
        # a stage that fails leaves no list
        eng.stage(W)
        expect(EFUNCUSE, eng.stage, [(0, len(inp.reads), 0, 10)], where="stage of a bad window")
        refused(eng.run_staged, 1, where="run_staged after a failed stage")
        eng.stage(W)
        expect(EZEROSEQ, eng.stage, [(0, 0, 5, 5)], where="stage of an empty window")
        refused(eng.run_staged, 1, where="run_staged after a failed stage")
        eng.stage(W)
        refused(eng.stage, [], where="stage of no windows")
        refused(eng.run_staged, 1, where="run_staged after a stage of no windows")


@pytest.mark.parametrize("name,mutate", MUTATORS, ids=[m[0] for m in MUTATORS])
def test_staged_list_is_refused_after_an_input_change(orc, data, name, mutate):
    inp = Inputs(orc, data.cache)
    with deciphon_amd.Engine(0) as eng:
        setup(eng, inp, data.synth + [data.strip], data.reads)
        W = cost_windows(inp)
        eng.stage(W)
        eng.run_staged(1)
        check_cost(inp, W, *eng.fetch_staged(), "before")
        mutate(eng, inp, data)
        refused(eng.run_staged, 1, where=f"run_staged after {name}")
        refused(eng.fetch_staged, where=f"fetch_staged after {name}")
        eng.commit()
        W = cost_windows(inp)
        eng.stage(W)
        eng.run_staged(1)
        check_cost(inp, W, *eng.fetch_staged(), f"staged again after {name}")


# ---- 3. a path, then its trellis later ----------------------------------------------------------------------------

def test_delayed_trellis_after_other_calls(orc, data):
    """Cost calls, a batch, the staged list and a reserve between dcp_hip_path and dcp_hip_path_trellis change no
    input: the trellis is the one of the path's inputs and the steps do not move."""
    inp = Inputs(orc, data.cache)
    with deciphon_amd.Engine(0) as eng:
        setup(eng, inp, data.synth + [data.strip], data.reads)
        P, W = path_windows(inp), cost_windows(inp)
        eng.path(P, trellis=False)
        check_steps(inp, P, eng, "path")
        before = [steps_of(eng, i) for i in range(len(P))]
        check_cost(inp, W, *eng.cost(W), "cost between")
        eng.cost_hits_begin(W)
        check_hits(inp, W, eng.cost_hits_end(), "batch between")
        eng.stage(W)
        eng.run_staged(1)
        eng.path_reserve(32 << 20)
        for i, w in enumerate(P):
            check_trellis(inp, w, eng.path_trellis(i), f"delayed trellis {i}")
        for i, w in enumerate(P[::-1]):  # asked again, in another order
            check_trellis(inp, w, eng.path_trellis(len(P) - 1 - i), f"trellis {len(P) - 1 - i} again")
        for i, (steps, score) in enumerate(before):
            got, got_score = steps_of(eng, i)
            assert np.array_equal(got, steps) and bits(got_score) == bits(score), f"steps of window {i} moved"
        check_steps(inp, P, eng, "after the trellis")


@pytest.mark.parametrize("name,mutate", MUTATORS, ids=[m[0] for m in MUTATORS])
def test_delayed_trellis_is_refused_after_an_input_change(orc, data, name, mutate):
    inp = Inputs(orc, data.cache)
    with deciphon_amd.Engine(0) as eng:
        setup(eng, inp, data.synth + [data.strip], data.reads)
        P = path_windows(inp)
        eng.path(P, trellis=False)
        snap = inp.copy()
        check_steps(snap, P, eng, "path")
        mutate(eng, inp, data)
        for i in range(len(P)):
            refused(eng.path_trellis, i, where=f"trellis {i} after {name}")
        check_steps(snap, P, eng, f"steps after {name}")
        # a new path pass under the new inputs has its trellis again
        eng.commit()
        P = path_windows(inp)
        eng.path(P, trellis=False)
        check_steps(inp, P, eng, f"path after {name}")
        check_trellis(inp, P[-1], eng.path_trellis(len(P) - 1), f"trellis after {name}")


def test_failed_path_leaves_no_results(orc, data):
    inp = Inputs(orc, data.cache)
    with deciphon_amd.Engine(0) as eng:
        setup(eng, inp, data.synth + [data.strip], data.reads)
        P = path_windows(inp)
        eng.path(P, trellis=False)
        bad = P[:2] + [(len(inp.profiles), 0, 0, 10)]
        refused(eng.path, bad, where="path with a bad profile index")
        assert eng.lib.dcp_hip_path_nsteps(eng.h, 0) == -1
        refused(eng.path_trellis, 0, where="trellis after a failed path")
        eng.path(P[:3], trellis=False)
        check_trellis(inp, P[2], eng.path_trellis(2), "trellis after a good path")


# ---- 4. a seeded walk against a model of the contract ---------------------------------------------------------------

class Model:
    """What the header promises, restated: the return code of every call and the inputs each result belongs to."""

    def __init__(self, inp):
        self.inp = inp
        self.committed = 0
        self.gen = 0
        self.queue = []  # outstanding batches, oldest first: (windows, inputs)
        self.staged = None  # dict(wins, inp, gen, ran)
        self.path = None  # dict(wins, inp, gen) of the last successful dcp_hip_path; None: no results

    def window_code(self, wins):
        """stage()'s checks, in its order."""
        inp = self.inp
        if self.committed != len(inp.profiles):
            return EFUNCUSE
        for p, s, a, b in wins:
            if not 0 <= p < len(inp.profiles) or not 0 <= s < len(inp.reads):
                return EFUNCUSE
            if a < 0 or b < a or b > len(inp.reads[s]):
                return EFUNCUSE
            if b - a < 1:
                return EZEROSEQ
        return 0

    def path_code(self, wins):
        inp = self.inp
        for p, s, a, b in wins:  # every window first (dcp_hip_path), then stage()'s own checks
            if not 0 <= p < len(inp.profiles) or not 0 <= s < len(inp.reads) or a < 0 or b < a or b > len(inp.reads[s]):
                return EFUNCUSE
        if wins and self.committed != len(inp.profiles):
            return EFUNCUSE
        return 0


def _walk_windows(rng, m, inp, bad, allow_empty=True):
    n = int(rng.integers(0, 5))
    wins = []
    for _ in range(n):
        p = int(rng.integers(0, max(len(m.inp.profiles), 1)))
        s = int(rng.integers(0, len(inp.reads)))
        L = len(inp.reads[s])
        a, b = [(0, L), (L // 3, L), (0, min(L, 90))][int(rng.integers(0, 3))]
        wins.append((p, s, a, b))
    if wins and rng.random() < bad:
        j = int(rng.integers(0, len(wins)))
        p, s, a, b = wins[j]
        kinds = ["profile", "negative profile", "seq", "stop"] + (["empty"] if allow_empty else [])
        kind = kinds[int(rng.integers(0, len(kinds)))]
        L = len(inp.reads[s])
        wins[j] = {"profile": (len(m.inp.profiles), s, a, b), "negative profile": (-1, s, a, b),
                   "seq": (p, len(inp.reads), 0, 1), "stop": (p, s, a, L + 1), "empty": (p, s, a, a)}[kind]
    return wins


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_seeded_walk_against_the_contract(orc, data, seed):
    """About 300 calls drawn from every entry point, refused ones and out-of-range windows included: every return code
    equals the model's, every result equals the oracle's on the inputs in force when it was defined."""
    rng = np.random.default_rng(seed)
    inp = Inputs(orc, data.cache)
    m = Model(inp)
    pool = data.synth + [data.extra]
    tally = {}  # (entry point, accepted) -> calls

    def exp(code, fn, *args, where=""):
        key = (where.split("(")[1].split(",")[0], code == 0)
        tally[key] = tally.get(key, 0) + 1
        return expect(code, fn, *args, where=where)

    with deciphon_amd.Engine(0) as eng:
        setup(eng, inp, data.synth, data.walk_reads[0])
        m.committed = len(inp.profiles)
        # "+": a short sequence in the order a caller would make it (a stage that is then run and fetched, a path whose
        # trellis is then asked for), so that the walk reaches those results and not only their refusals
        names = ["add_profile", "add_protein", "load_dcp", "add_profile+", "add_protein+", "load_dcp+", "commit",
                 "clear_profiles", "set_sequences", "set_mode", "set_xtrans_table", "cost", "cost", "cost_hits",
                 "cost_hits", "begin", "begin", "end", "end", "end", "end", "cost_bench", "cost_bench", "stage", "stage+",
                 "stage+", "stage+", "run_staged", "fetch_staged", "path", "path+", "path+", "path_trellis",
                 "path_steps", "path_reserve", "queries"]
        todo = []
        for k in range(300):
            name = todo.pop(0) if todo else names[int(rng.integers(0, len(names)))]
            chained = name.endswith("+") or bool(todo)
            if name == "stage+":  # committed first, as a caller about to stage would
                name, todo = "commit", ["stage", "run_staged", "fetch_staged"]
            elif name == "path+":
                name, todo = "path", ["path_trellis"]
            elif name.endswith("+"):  # a profile added and committed
                name, todo = name[:-1], ["commit"]
            if name == "load_dcp" and len(inp.profiles) > 12:  # keeps the oracle's work bounded
                name = "clear_profiles"
            out = len(m.queue) > 0
            where = f"seed {seed} call {k} ({name}, {len(m.queue)} outstanding)"
            if name in ("add_profile", "add_protein", "load_dcp", "commit", "clear_profiles", "set_sequences",
                        "set_mode", "set_xtrans_table"):
                code = EFUNCUSE if out else 0
                if name == "add_profile":
                    p = pool[int(rng.integers(0, len(pool)))]
                    exp(code, eng.add_profile, p.K, p.trans, p.match, p.null, p.bg, where=where)
                    new = [p]
                elif name == "add_protein":
                    pr = data.protein
                    exp(code, eng.add_protein, pr.core_size, pr.trans, pr.emission, pr.BMk, pr.null_emission,
                           pr.bg_emission, where=where)
                    new = [data.minifam[0]]
                elif name == "load_dcp":
                    exp(code, eng.load_dcp, DCP, where=where)
                    new = list(data.minifam)
                elif name == "commit":
                    exp(code, eng.commit, where=where)
                elif name == "clear_profiles":
                    exp(code, eng.clear_profiles, where=where)
                elif name == "set_sequences":
                    reads = data.walk_reads[int(rng.integers(0, len(data.walk_reads)))]
                    exp(code, eng.set_sequences, reads, where=where)
                elif name == "set_mode":
                    mode = (bool(rng.integers(0, 2)), bool(rng.integers(0, 2)))
                    exp(code, eng.set_mode, *mode, where=where)
                else:
                    table = [data.table, data.table2, None][int(rng.integers(0, 3))]
                    exp(code, eng.set_xtrans_table, np.zeros((0, 13), np.float32) if table is None else table,
                           where=where)
                if code:
                    assert eng.num_profiles == len(inp.profiles), f"{where}: a refused call changed the profiles"
                    continue
                m.gen += 1
                if name in ("add_profile", "add_protein", "load_dcp"):
                    inp.profiles = inp.profiles + new
                elif name == "commit":
                    m.committed = len(inp.profiles)
                elif name == "clear_profiles":
                    inp.profiles, m.committed = [], 0
                elif name == "set_sequences":
                    inp.reads = list(reads)
                elif name == "set_mode":
                    inp.mode = mode
                else:
                    inp.table = table
                assert eng.num_profiles == len(inp.profiles), where
            elif name in ("cost", "cost_hits", "cost_bench", "stage"):
                wins = _walk_windows(rng, m, inp, 0.05 if chained else 0.2)
                code = EFUNCUSE if out else m.window_code(wins)
                if name == "cost_bench" and not out and not wins:
                    code = EFUNCUSE
                if name == "stage":
                    if not out:
                        m.staged = None  # a stage that fails leaves no list either
                    if not wins and not out:
                        code = EFUNCUSE
                    exp(code, eng.stage, wins, where=where)
                    if not code:
                        m.staged = dict(wins=wins, inp=inp.copy(), gen=m.gen, ran=False)
                    continue
                fn = {"cost": eng.cost, "cost_hits": eng.cost_hits,
                      "cost_bench": lambda w: eng.cost_bench(w, 0, 1)[2:]}[name]
                got = exp(code, fn, wins, where=where)
                if code:
                    continue
                m.staged = None
                if name == "cost_hits":
                    check_hits(inp, wins, got, where)
                else:
                    check_cost(inp, wins, *got, where)
            elif name == "begin":
                wins = _walk_windows(rng, m, inp, 0.2)
                code = EFUNCUSE if len(m.queue) == 2 else m.window_code(wins)
                exp(code, eng.cost_hits_begin, wins, where=where)
                if not code:
                    m.queue.append((wins, inp.copy()))
                    m.staged = None
            elif name == "end":
                got = exp(0 if out else EFUNCUSE, eng.cost_hits_end, where=where)
                if out:
                    wins, snap = m.queue.pop(0)
                    check_hits(snap, wins, got, where)
            elif name in ("run_staged", "fetch_staged"):
                st = m.staged
                code = EFUNCUSE if out or st is None or st["gen"] != m.gen else 0
                if name == "run_staged":
                    reps = 1 if chained else int(rng.integers(0, 3))
                    exp(code, eng.run_staged, reps, where=where)
                    if not code and reps > 0:
                        st["ran"] = True
                else:
                    code = code or (0 if st["ran"] else EFUNCUSE)
                    got = exp(code, eng.fetch_staged, where=where)
                    if not code:
                        check_cost(st["inp"], st["wins"], *got, where)
            elif name == "path":
                wins = _walk_windows(rng, m, inp, 0.05 if chained else 0.2, allow_empty=False)
                code = m.path_code(wins)
                m.path = None
                exp(code, eng.path, wins, False, where=where)
                if not code:
                    m.path = dict(wins=wins, inp=inp.copy(), gen=m.gen)
                    check_steps(inp, wins, eng, where)
            elif name in ("path_trellis", "path_steps"):
                pth = m.path
                n = len(pth["wins"]) if pth else 0
                # one beyond the last window now and then (a chained trellis asks for one of the path's windows)
                i = int(rng.integers(0, n if chained and n else n + 1))
                if name == "path_steps":
                    assert eng.lib.dcp_hip_path_nsteps(eng.h, i) == (len(pth["inp"].path(pth["wins"][i])[3])
                                                                     if i < n else -1), where
                    if pth:
                        check_steps(pth["inp"], pth["wins"], eng, where)
                    continue
                code = 0 if i < n and pth["gen"] == m.gen else EFUNCUSE
                got = exp(code, eng.path_trellis, i, where=where)
                if not code:
                    check_trellis(pth["inp"], pth["wins"][i], got, where)
                    check_steps(pth["inp"], pth["wins"], eng, where)  # the literal pass replaced them: the same steps
            elif name == "path_reserve":
                exp(0, eng.path_reserve, 16 << 20, where=where)
            else:
                assert eng.num_profiles == len(inp.profiles), where
                Ks = [eng.core_size(i) for i in range(len(inp.profiles) + 1)]
                assert Ks == [p.K for p in inp.profiles] + [-1], where
        while m.queue:
            wins, snap = m.queue.pop(0)
            check_hits(snap, wins, eng.cost_hits_end(), f"seed {seed}: drain")
    print(f"seed {seed}:", ", ".join(f"{n} {'ok' if a else 'refused'} {c}" for (n, a), c in sorted(tally.items())))
    # the walk reached every kind of result it checks
    for n in ("cost", "cost_hits", "begin", "end", "cost_bench", "stage", "run_staged", "fetch_staged", "path",
              "path_trellis"):
        assert tally.get((n, True), 0) > 0, f"seed {seed}: no successful {n}"
