"""The routes of the cost pass, as one table: which request reaches which compiled kernel, and with which windows.
Shared by tests/test_cost_routes.py (CPU: what the table holds, and that the planner agrees with it) and
tests/test_gpu_cost_routes.py (GPU: every request through Engine.cost, its launches read back from the engine).

A window's (null, alt) comes out of one of about thirty kernels, chosen by the rest of its request
(deciphon_amd/csrc/stage_plan.cpp cost_schedule): the class kernels dcp_cost_kernel<Q, W>, the narrow kernels of
classes 4..6, one fused kernel for a small mix of the single-wave classes 0..3, and per pack shape a kernel that reads
its rows from global memory and one that keeps them in LDS.  A ROUTE here is one of those kernels, for the class and
narrow kernels under either order of the launch (DECIPHON_HIP_XCD_PLACEMENT = plain | eighths):

    pack_lds[s]   pack[s]   class[c]/plain   class[c]/eighths   narrow[c]/plain   narrow[c]/eighths   fused/class[c]

A REQUEST is a window list, the knobs it is sent under and the launches it must cause, stated here as data
(Request.expect) from the route alone: the CPU test holds host.cost_schedule(host.stage_plan(..)) to them, the GPU
test Engine.last_cost_launches().  How a request is steered:

    class[c], c <= 3   single-wave windows of class c only (K <= 124: DECIPHON_HIP_PACK=0)
    fused/class[c]     the same windows plus ONE window of a neighbouring single-wave class
    narrow[c]          windows of the narrow profiles of class c; DECIPHON_HIP_NARROW=0 sends them to class[c]
    pack_lds[s]        windows of profiles of pack shape s; DECIPHON_HIP_PACK_LDS=0 sends them to pack[s]

Which K belongs to which class, narrow kernel and pack shape comes from the engine's own tables
(host.engine_core_size, host.engine_pack_shapes); the K themselves are the two ends of every shape (PACK_KS of
tests/test_gpu_delete_runs.py and SINGLE_WAVE of tests/delete_run_cases.py).  K above 640 has one route, whose orders
tests/test_gpu_xcd_placement.py covers.

The windows of a (route, K) CELL come from four families, made by the generators the other suites use:
    ends   row_loop_cases.WINDOW_LENGTHS from a read's start, and its first 17 ending at the read's end
    k0     row_loop_cases.K0_JUNK through with_k0, against the oracle's scores of the profile with +inf there
    runs   delete_run_cases.planted: the shortest, a middle and the longest of run_lengths(K), DD over the run 0 and
           ordinary; the window is the read planted() makes, 3 (K - r) rows
    ties   synth_profile(rng, K, 2.0) under the special-transition table rounded to 2.0 -- an engine-wide setting, so
           these windows have loads and requests of their own (names ending in -ties)

Four more requests sit on the two size thresholds: 16384 single-wave windows of two classes (fused, and the fused
kernel's only launch in the eighths order: dcp_xcd_remap) and 16385 (one kernel per class); 16384 packs of the
32-lane shape of K = 124 and 16384 packs of K = 3 from global memory (the pack kernels' eighths order).  Their windows
are whole reads of 5..12 rows, 32 reads in all, so the oracle is asked once per (profile, read).

Nothing here needs a GPU, an engine or the oracle: profiles and reads are described (Load.profiles, Load.reads) and
made only by Load.materialise()."""
import functools

KNOBS = ("DECIPHON_HIP_PACK", "DECIPHON_HIP_PACK_LDS", "DECIPHON_HIP_NARROW", "DECIPHON_HIP_XCD_PLACEMENT")
FAMILIES = ("ends", "k0", "runs", "ties")
PLACEMENTS = ("plain", "eighths")
K0_CUTS = (1, 7, 25, 60)       # window lengths of the k0 family, as tests/test_gpu_row_loop_ends.py cuts them
RUN_DD = ("zero", "ordinary")  # DD over a planted run
TIE_QUANT = 2.0
FUSED_CLASSES = 4              # cost_schedule fuses classes 0..3 ...
FUSED_LIMIT = 16384            # ... when they hold at most this many windows; dcp_xcd_remap changes order from it on
BULK_LENGTHS = tuple(range(5, 13))
BULK_READS = 32
MAX_K = 640


def launch(kernel, index, first, count, windows_per_profile=0):
    """a launch as host.cost_schedule and Engine.last_cost_launches state it"""
    branch = "narrow" if kernel == "narrow" else "pack" if kernel.startswith("pack") else "class"
    return dict(kernel=kernel, index=index, first=first, count=count, windows_per_profile=windows_per_profile,
                branch=branch)


class Load:
    """What the engine holds for a group of requests: profiles and reads, described, not made.
    profiles: ("synth", K) | ("k0", K, base profile, index into K0_JUNK) | ("planted", K, r, dd)
    reads:    ("random", n) | ("planted", profile)"""

    def __init__(self, name, seed, quant=None):
        self.name, self.seed, self.quant = name, seed, quant
        self.profiles, self.reads = [], []
        self.windows = {}  # K -> [((profile, read, start, stop), family)]

    def core_sizes(self):
        return [p[1] for p in self.profiles]

    def read_lengths(self):
        return [r[1] if r[0] == "random" else 3 * (self.profiles[r[1]][1] - self.profiles[r[1]][2]) for r in self.reads]

    def oracle_profile(self, i):
        """the profile whose oracle scores profile i must have: a k0 form scores as the form with +inf there"""
        return self.profiles[i][2] if self.profiles[i][0] == "k0" else i

    def _add(self, profile, read=None):
        self.profiles.append(profile)
        if read is not None:
            self.reads.append(read)
        return len(self.profiles) - 1

    def add_core_size(self, K):
        from delete_run_cases import run_lengths
        from row_loop_cases import K0_JUNK, WINDOW_LENGTHS

        n = max(WINDOW_LENGTHS)
        base, read = self._add(("synth", K), ("random", n)), len(self.reads) - 1
        w = self.windows.setdefault(K, [])
        if self.quant:
            w += [((base, read, 0, L), "ties") for L in WINDOW_LENGTHS]
            return
        w += [((base, read, 0, L), "ends") for L in WINDOW_LENGTHS]
        w += [((base, read, n - L, n), "ends") for L in WINDOW_LENGTHS[:17]]
        w += [((base, read, 0, L), "k0") for L in K0_CUTS]
        for j in range(len(K0_JUNK)):
            form = self._add(("k0", K, base, j))
            w += [((form, read, 0, L), "k0") for L in K0_CUTS]
        runs = run_lengths(K)
        for r in sorted({runs[0], runs[len(runs) // 2], runs[-1]}):
            for dd in RUN_DD:
                p = self._add(("planted", K, r, dd))
                self.reads.append(("planted", p))
                w.append(((p, len(self.reads) - 1, 0, 3 * (K - r)), "runs"))

    def materialise(self):
        """-> (profiles, reads) as oracle.pyoracle.Profile and uint8 arrays"""
        import numpy as np

        from dcp_testlib import random_seq, synth_profile
        from delete_run_cases import planted
        from row_loop_cases import K0_JUNK, with_k0

        rng = np.random.default_rng(self.seed)
        profs, planted_reads = [], {}
        for i, p in enumerate(self.profiles):
            if p[0] == "synth":
                profs.append(synth_profile(rng, p[1], self.quant))
            elif p[0] == "k0":
                profs.append(with_k0(profs[p[2]], K0_JUNK[p[3]]))
            else:
                prof, planted_reads[i], _ = planted(rng, p[1], p[2], p[3], self.quant)
                profs.append(prof)
        reads = [random_seq(rng, r[1]) if r[0] == "random" else planted_reads[r[1]] for r in self.reads]
        assert [len(r) for r in reads] == self.read_lengths()
        return profs, reads


class Request:
    """route: the kernel it pins (None: a threshold request); knobs: the value of every name of KNOBS (None: unset);
    windows(): int32[n][4]; families: per window; expect: its launches, in launch order; hits: also sent through
    cost_hits_begin / _end"""

    def __init__(self, route, load, knobs, windows, families, expect, hits=False, name=None):
        self.route, self.load, self.hits = route, load, hits
        self.name = name or f"{route}@{load.name}"
        self.knobs = {k: knobs.get(k) for k in KNOBS}
        self._windows, self.families, self.expect = windows, families, expect

    def windows(self):
        import numpy as np

        w = self._windows() if callable(self._windows) else self._windows
        return np.ascontiguousarray(w, np.int32).reshape(-1, 4)

    def core_sizes(self):
        K = self.load.core_sizes()
        return [K[w[0]] for w in self.windows()]


def _windows_of(load, Ks):
    pairs = [p for K in Ks for p in load.windows[K]]
    return [w for w, _ in pairs], [f for _, f in pairs]


def _per_profile(wins):
    n = {}
    for w in wins:
        n[w[0]] = n.get(w[0], 0) + 1
    return n


def _one_class(route, load, knobs, c, Ks, kernel="class", **kw):
    wins, fam = _windows_of(load, Ks)
    expect = [launch(kernel, c, 0, len(wins), len(wins) // len(_per_profile(wins)))]
    if kernel == "narrow":  # the class's branch is entered and left with nothing to launch
        expect.append(launch("none", c, len(wins), 0))
    return Request(route, load, knobs, wins, fam, expect, **kw)


def _class_routes(load, by_class, knobs, hits):
    """class[c] under either order, and for the single-wave classes the fused kernel through one more window"""
    out = []
    for c, Ks in sorted(by_class.items()):
        for place in PLACEMENTS:
            out.append(_one_class(f"class[{c}]/{place}", load, dict(knobs, DECIPHON_HIP_XCD_PLACEMENT=place), c, Ks, hits=hits))
        if c < FUSED_CLASSES:
            other = c + 1 if c + 1 in by_class and c + 1 < FUSED_CLASSES else c - 1
            assert other in by_class and 0 <= other < FUSED_CLASSES, (load.name, c)
            wins, fam = _windows_of(load, Ks)
            extra = [p for p in load.windows[by_class[other][0]] if p[0][3] - p[0][2] == 12][0]  # two and a half iterations
            wins, fam = wins + [extra[0]], fam + [extra[1]]
            out.append(Request(f"fused/class[{c}]", load, knobs, wins, fam, [launch("fused", 0, 0, len(wins))], hits=hits))
    return out


def _pack_routes(load, by_shape, shapes, hits):
    out = []
    for s, Ks in sorted(by_shape.items()):
        G, waves = shapes[s]
        wins, fam = _windows_of(load, Ks)
        packs = [-(-n // G) for n in _per_profile(wins).values()]  # a pack holds up to G windows of ONE profile
        from_global = Request(f"pack[{s}]", load, {"DECIPHON_HIP_PACK_LDS": None if not waves else "0"}, wins, fam,
                              [launch("pack", s, 0, sum(packs))], hits=hits)
        if waves:  # a workgroup holds up to `waves` packs of one profile
            out.append(Request(f"pack_lds[{s}]", load, {}, wins, fam,
                               [launch("pack_lds", s, 0, sum(-(-p // waves) for p in packs))], hits=hits))
        out.append(from_global)
    return out


def _bulk(describe, shapes):
    """the four threshold requests, over one load of four profiles and 32 short reads"""
    load = Load("thresholds", 2690)
    Ks = (125, 129, 124, 3)
    cls = [describe(K)[2] for K in Ks]
    assert cls[0] != cls[1] and max(cls[:2]) < FUSED_CLASSES and describe(125)[4] < 0 and describe(129)[4] < 0
    for K in Ks:
        load.profiles.append(("synth", K))
    for i in range(BULK_READS):
        load.reads.append(("random", BULK_LENGTHS[i % len(BULK_LENGTHS)]))

    def whole_reads(profiles, reps, extra=0):
        def make():
            import numpy as np

            one = [(p, s, 0, load.reads[s][1]) for p in profiles for s in range(BULK_READS)]
            return np.concatenate([np.tile(np.array(one, np.int32), (reps, 1)), np.array(one[:extra], np.int32).reshape(-1, 4)])
        return make

    half = FUSED_LIMIT // 2
    lo, hi = (0, 1) if cls[0] < cls[1] else (1, 0)  # the problem list is in class order; the extra window is profile 0's
    n = [half + (lo == 0), half + (hi == 0)]
    out = [Request(None, load, {}, whole_reads((0, 1), half // BULK_READS), None, [launch("fused", 0, 0, FUSED_LIMIT)],
                   name="fused, 16384 windows"),
           Request(None, load, {}, whole_reads((0, 1), half // BULK_READS, extra=1), None,
                   [launch("class", cls[hi], n[0], n[1], n[1]), launch("class", cls[lo], 0, n[0], n[0])],
                   name="one kernel per class, 16385 windows")]
    for p, knobs in ((2, {}), (3, {"DECIPHON_HIP_PACK_LDS": "0"})):
        s = describe(Ks[p])[4]
        G, waves = shapes[s]
        assert s >= 0 and (not waves or knobs)
        out.append(Request(None, load, knobs, whole_reads((p,), FUSED_LIMIT * G // BULK_READS), None,
                           [launch("pack", s, 0, FUSED_LIMIT)], name=f"pack[{s}], 16384 packs of K = {Ks[p]}"))
    return out


@functools.lru_cache(None)
def table():
    """-> (requests, ends): every request, grouped by load; ends[route] = the core sizes at either end of the
    profiles the route's kernel serves (up to MAX_K), whose cells must hold every family"""
    from deciphon_amd import host
    from delete_run_cases import SINGLE_WAVE
    from test_gpu_delete_runs import PACK_KS

    describe = functools.lru_cache(None)(host.engine_core_size)  # (K, Kp, class, narrow, pack shape)
    shapes = [tuple(int(v) for v in row) for row in host.engine_pack_shapes()]
    assert len(shapes) == host.NUM_PACK_SHAPES
    served = range(min(PACK_KS), MAX_K + 1)

    def both_ends(Ks):
        Ks = list(Ks)
        return {min(Ks), max(Ks)} if Ks else set()

    ends = {}
    for s in range(host.NUM_PACK_SHAPES):
        e = both_ends(K for K in served if describe(K)[4] == s)
        assert e, f"no profile of pack shape {s}"
        ends[f"pack[{s}]"] = e
        if shapes[s][1]:
            ends[f"pack_lds[{s}]"] = e
    for c in sorted({describe(K)[2] for K in served}):
        assert 0 <= c < host.NUM_CLASSES
        e = both_ends(K for K in served if describe(K)[2] == c)
        narrow = both_ends(K for K in served if describe(K)[2] == c and describe(K)[3])
        for place in PLACEMENTS:
            ends[f"class[{c}]/{place}"] = e
            if narrow:
                ends[f"narrow[{c}]/{place}"] = narrow
        if c < FUSED_CLASSES:
            ends[f"fused/class[{c}]"] = e

    packed = sorted(set(PACK_KS) | {K for r, e in ends.items() if r.startswith("pack[") for K in e})
    above = [K for _, K in SINGLE_WAVE if describe(K)[4] < 0]
    assert all(describe(K)[4] >= 0 for K in packed) and max(above) == MAX_K
    tiers = (("packed", packed),
             ("single-wave", [K for K in above if describe(K)[2] < FUSED_CLASSES]),
             ("narrow", [K for K in above if describe(K)[3]]),
             ("wide", [K for K in above if describe(K)[2] >= FUSED_CLASSES and not describe(K)[3]]))
    requests = []
    for t, (tier, Ks) in enumerate(tiers):
        for quant in (None, TIE_QUANT):
            load = Load(tier + ("-ties" if quant else ""), 2600 + 2 * t + bool(quant), quant)
            for K in Ks:
                load.add_core_size(K)
            by_class, by_shape = {}, {}
            for K in Ks:
                by_class.setdefault(describe(K)[2], []).append(K)
                by_shape.setdefault(describe(K)[4], []).append(K)
            hits = not quant  # one request per route through the batches in flight as well
            if tier == "packed":
                requests += _pack_routes(load, by_shape, shapes, hits)
                requests += _class_routes(load, by_class, {"DECIPHON_HIP_PACK": "0"}, hits)
            elif tier == "narrow":
                for c, Kc in sorted(by_class.items()):
                    for place in PLACEMENTS:
                        requests.append(_one_class(f"narrow[{c}]/{place}", load, {"DECIPHON_HIP_XCD_PLACEMENT": place}, c, Kc,
                                                   kernel="narrow", hits=hits))
                requests += _class_routes(load, by_class, {"DECIPHON_HIP_NARROW": "0"}, hits)
            else:
                requests += _class_routes(load, by_class, {}, hits)
    requests += _bulk(describe, shapes)
    names = [r.name for r in requests]
    assert len(set(names)) == len(names)
    return requests, ends


def cells(requests):
    """-> {(route, K): {family: windows}} over the requests that pin a route"""
    out = {}
    for r in requests:
        if r.route is None:
            continue
        for K, f in zip(r.core_sizes(), r.families):
            cell = out.setdefault((r.route, K), dict.fromkeys(FAMILIES, 0))
            cell[f] += 1
    return out
