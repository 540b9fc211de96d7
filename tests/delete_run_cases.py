"""Profiles with planted deletions, shared by tests/test_emul_delete_runs.py and tests/test_gpu_delete_runs.py.

A case is a profile of K positions and a read that matches positions 1..a and a+r+1..K codon by codon: the best
alignment deletes the r positions between them, so the D chain of every row behind position a carries one value
through the whole run -- across r / Q lane boundaries of a kernel that keeps Q positions per lane
(deciphon_amd/csrc/viterbi_body.h, dcp_lazy_turns_carry).  DD over the run is 0.0, tiny or whatever the random
profile holds ("ordinary": the carry dies after a few positions); `quant` rounds every other cost to a multiple of
it, which makes exact fp32 ties between the carried value and a lane's own chain common.

Above one wavefront (tests/test_emul_wave_exchange.py, tests/test_gpu_wave_exchange.py) the cases are short-anchor runs
(short_anchor, wave_cases: eight codons on either side of the run, 48 rows whatever K is) placed against the wavefront
and strip boundaries of every multi-wave shape, and runs whose cost cancels what entered them (cancelling_run)."""
import numpy as np

from dcp_testlib import CODE_OFF, synth_profile

LAZY_POSITIONS = 6  # DCP_LAZY_POSITIONS (viterbi_body.h): positions covered by the turns taken without a vote
LONG_RUN = 4 * LAZY_POSITIONS  # a run this long crosses four or more lane boundaries whatever the shape
TINY = np.float32(2.0 ** -20)
DD_KINDS = ("zero", "tiny", "ordinary")

# (Q, W of the kernel, K): every single-wave shape at the lower and the upper end of the profiles it serves
# (viterbi_kernels.hip, dcp_class_of and dcp_launch_cost_narrow: (5,1), (7,1), (10,1) run on the layouts of
# (6,1), (8,1), (6,2))
SINGLE_WAVE = ((1, 5), (1, 60), (2, 61), (2, 128), (3, 129), (3, 192), (4, 193), (4, 256), (5, 257), (5, 320),
               (6, 321), (6, 384), (7, 385), (7, 448), (8, 449), (8, 512), (10, 513), (10, 640))
LAYOUT = {5: (6, 1), 7: (8, 1), 10: (6, 2)}  # Q of the narrow kernels -> (Q, W) of the layout they read

# every shape of PackWave (S lanes per group, Q positions per lane), viterbi_kernels.hip
PACK_SHAPES = ((4, 1), (4, 2), (4, 4), (8, 2), (8, 4), (16, 2), (16, 3), (16, 4), (32, 2), (32, 3), (32, 4))


def run_lengths(K):
    """delete runs from 1 up to K - 2 positions, half of them LONG_RUN or longer where K allows"""
    want = (1, 3, LONG_RUN, LONG_RUN + 13, max(K // 2, LONG_RUN), K - 2)
    return sorted({r for r in want if 1 <= r <= K - 2})


def planted(rng, K, r, dd, quant=None, a=None):
    """-> (profile, read, a): the read matches positions 1..a and a+r+1..K (1-based), DD over the run is `dd`"""
    assert 1 <= r <= K - 2 and dd in DD_KINDS
    prof = synth_profile(rng, K, quant)
    if a is None:
        a = int(rng.integers(1, K - r))  # 1 <= a, a + r + 1 <= K
    codons = rng.integers(0, 64, size=K)
    low = np.float32(quant if quant else 0.25)
    for k in range(K):
        prof.match[CODE_OFF[2] + int(codons[k]), k] = low
    prof.trans[0, 1:] += np.float32(16.0)  # BM: entering behind the run costs more than deleting it
    prof.trans[1, 1:] = low                # MM
    prof.trans[3, a] = low                 # MD into the first deleted position (0-based a)
    prof.trans[6, a + r] = low             # DM out of the last one
    if dd != "ordinary":
        prof.trans[7, a + 1 : a + r + 1] = np.float32(0.0) if dd == "zero" else TINY
    kept = np.concatenate([codons[:a], codons[a + r :]])
    read = np.stack([kept // 16, (kept // 4) % 4, kept % 4], axis=1).reshape(-1).astype(np.uint8)
    return prof, read, a


def single_wave_cases():
    """-> [(Q, K, r, dd, quant)]"""
    return [(Q, K, r, dd, quant) for Q, K in SINGLE_WAVE for r in run_lengths(K) for dd in DD_KINDS
            for quant in (None, (1.0, 4.0)[r % 2])]


# ---- above one wavefront: the exchange between the wavefronts of a row (CostWave<Q, W>, W > 1, and StripWave) ----
ANCHOR = 8   # codons matched in front of and behind the run: a window of 48 rows whatever K is
WINDOW = 3 * 2 * ANCHOR
# (Q, W, K): both ends of every multi-wave class of DCP_CLASS_TABLE (viterbi_kernels.hip, classes 6..10)
MULTI_WAVE = ((6, 2, 641), (6, 2, 768), (4, 4, 769), (4, 4, 1024), (6, 4, 1025), (6, 4, 1536), (8, 4, 1537), (8, 4, 2048),
              (8, 8, 2049), (8, 8, 4096))
STRIP_Q, STRIP_W = 4, 8  # the strip class: strips of 64 * 4 * 8 = 2048 positions (launch_strip)
STRIP = 64 * STRIP_Q * STRIP_W
STRIP_KS = (4097, 6144, 16383)  # one position in the second strip, three whole strips, the largest profile
# K -> index into SWEEP of a window with rows on either protocol (asserted by tests/test_emul_wave_exchange.py; the
# whole table: profiles/r09_wave_exchange_tests.txt): the sweep case that the GPU test sends through the path pass
MIXED_AT = {641: 9, 768: 11, 769: 12, 1024: 13, 1025: 12, 1536: 11, 1537: 10, 2048: 11, 2049: 10, 4096: 11, 4097: 13}
SWEEP = tuple(float(np.float32(10.0 ** (-3.0 + 3.0 * i / 23))) for i in range(24))  # DD over the run, 1e-3 .. 1


def short_anchor(rng, K, a, r, dd, entry="blocked", everywhere=False, quant=None, anchor=ANCHOR):
    """-> (profile, read): the read matches the `anchor` positions in front of 0-based position a and the `anchor`
    positions from a + r on, so the alignment that uses both deletes positions a .. a + r - 1.  dd: one of DD_KINDS or
    a number, over the run only or (`everywhere`) over the whole profile.  entry "blocked": entering the profile at
    or behind a costs 1000 more, so the run is on the best path and what enters a wavefront at its first lane wins in
    every wavefront behind a; "open": entering anywhere behind position 0 costs 16 more, as in planted(), and whether
    the run pays depends on DD."""
    assert anchor <= a and r >= 1 and a + r + anchor <= K and entry in ("blocked", "open")
    prof = synth_profile(rng, K, quant)
    low = np.float32(0.0 if quant else 0.25)  # a multiple of quant that keeps the run on the best path
    kept = np.concatenate([np.arange(a - anchor, a), np.arange(a + r, a + r + anchor)])
    codons = rng.integers(0, 64, size=2 * anchor)
    for k, c in zip(kept, codons):
        prof.match[CODE_OFF[2] + int(c), k] = low / 4
    if entry == "blocked":
        prof.trans[0, a:] += np.float32(1000.0)
        prof.trans[0, a - anchor] = low
        prof.match[:, a : a + r] += np.float32(30.0)  # nothing matches inside the run: every position of it is deleted
    else:
        prof.trans[0, 1:] += np.float32(16.0)
    prof.trans[1, kept[1:]] = low / 4  # MM along the anchors
    prof.trans[3, a] = low             # MD into the first deleted position
    prof.trans[6, a + r] = low         # DM out of the last one
    if dd != "ordinary":
        c = np.float32(0.0) if dd == "zero" else TINY if dd == "tiny" else np.float32(dd)
        if everywhere:
            prof.trans[7, 1:] = c
        else:
            prof.trans[7, a + 1 : a + r] = c  # the D->D steps inside the run
    read = np.stack([codons // 16, (codons // 4) % 4, codons % 4], axis=1).reshape(-1).astype(np.uint8)
    return prof, read


def wave_geometries(K, per, span=None):
    """-> {name: (a, r)}: where the runs lie for a kernel that keeps `per` positions per wavefront (span: positions
    per strip, strip class only).  `whole` deletes exactly wavefront 1, the eight around it miss or overshoot either
    end by one; where the closing anchor leaves no room behind wavefront 1 (two wavefronts: (6,2)) the nine runs
    start around its first position and end around the last position a run can end at, K - ANCHOR - 1."""
    end = K - ANCHOR  # a + r of a run that reaches the last position a run can reach
    nw = (min(K, span or K) + per - 1) // per  # wavefronts that hold positions (of the first strip)
    g = {"inside": (per // 2, 24), "mid to mid": (per // 2, per), "to the end": (per // 2, end - per // 2)}
    g["mid of wave 0 into the last wave"] = (per // 2, min((nw - 1) * per + 4, end) - per // 2)
    for da in (-1, 0, 1):
        for dr in (-1, 0, 1):
            name = "whole" if da == dr == 0 else f"whole{da:+d}{dr:+d}"
            g[name] = (per + da, per + dr) if 2 * per + 1 + ANCHOR <= K else (per + da, end - (per + da) + dr - 1)
    if span:
        for b in (span - 1, span, span + 1):
            g[f"across the strip boundary, from {b}"] = (b - 40, 80) if b - 40 + 80 + ANCHOR <= K else (b - 40, end - b + 40)
        if 2 * span + ANCHOR <= K:
            g["whole strip"] = (span, span)
    assert all(ANCHOR <= a and r >= 1 and a + r <= end for a, r in g.values()), (K, per, g)
    return g


def wave_cases(Q, W, K, span=None, brief=False):
    """-> [(name, a, r, dd, entry, everywhere, quant)] of one profile size, about fifty: every geometry with the late
    entry blocked and a free or nearly free run; ordinary DD; the sweep of DD with the entry open, on the run that
    deletes wavefront 1 (two wavefronts: over the whole profile, or the DD in front of and behind the run would
    decide); three tie-rich ones.  brief: the geometries alone (the largest profiles: the sweep is the shape's, and the
    shape has it at a smaller K)"""
    per = 64 * Q
    geo = wave_geometries(K, per, span)
    cases = []
    for i, (name, (a, r)) in enumerate(geo.items()):
        if not brief or not name.startswith("whole") or name in ("whole", "whole strip"):
            cases.append((name, a, r, ("zero", "tiny")[i % 2], "blocked", i % 3 == 0, None))
    sweep_on = "to the end" if W == 2 else "whole"
    last = "mid of wave 0 into the last wave"
    cases.append(("whole", *geo["whole"], "ordinary", "blocked", False, None))
    cases.append((last, *geo[last], "zero", "open", False, None))
    cases.append(("whole", *geo["whole"], "zero", "blocked", False, 1.0))
    if brief:
        return cases
    for name in ("inside", "to the end"):
        cases.append((name, *geo[name], "ordinary", "blocked", False, None))
    for c in SWEEP:
        cases.append((sweep_on, *geo[sweep_on], c, "open", W == 2, None))
    for dd in ("tiny", "ordinary"):
        cases.append((last, *geo[last], dd, "open", False, None))
    cases.append(("mid to mid", *geo["mid to mid"], "tiny", "blocked", True, 4.0))
    cases.append((sweep_on, *geo[sweep_on], SWEEP[12], "open", W == 2, 1.0 / 64))
    return cases


def wave_shapes():
    """-> [(Q, W, K, span, brief)]: every multi-wave cost shape at both ends of its class, then the strip class"""
    return [(Q, W, K, None, False) for Q, W, K in MULTI_WAVE] + \
           [(STRIP_Q, STRIP_W, K, STRIP, K > STRIP_KS[0]) for K in STRIP_KS]


# ---- a run whose cost cancels what entered it: E + tdd(w) small, |E| and tdd(w) large ----
CANCEL_QUANT = 0.25  # the xtrans table of these cases is rounded to it: E of the planted row is then exact


def wave_tdd(DD, Q, w):
    """put_tdd (lane_ops_gpu.h) in numpy: the DD of wavefront w but the first, every lane its own Q, then a butterfly"""
    d = np.asarray(DD[64 * Q * w : 64 * Q * (w + 1)], np.float32).reshape(64, Q)
    t = np.where(np.arange(64) == 0, np.float32(0.0), d[:, 0]).astype(np.float32)
    for q in range(1, Q):
        t = (t + d[:, q]).astype(np.float32)
    for s in (32, 16, 8, 4, 2, 1):
        t = (t + t[np.arange(64) ^ s]).astype(np.float32)
    return t[63]


def cancelling_run(rng, Q, K, xt, neg=-125.0, frac=0.484, land=2.0, place=0.8):
    """-> (profile, read, facts).  Match costs may be negative (deciphon_hip.h asks for non-negative MD and DD only), so
    E of a row can be about -1000 while running through a wavefront costs about +1000.  Here the eight codons in front
    of the run match at `neg` each, and row l = 24 has its E at the last position of wavefront 0.  MD into wavefront 1
    is 0, so what enters it IS E, and every DD of wavefront 1 is chosen so that the fp32 chain E + DD + DD + ... rounds
    DOWN by `frac` of an ulp at every step: the chain arrives about 5e-3 BELOW the exact sum, near `land`, while
    s = E + tdd(1) -- tdd a butterfly sum, nearly exact -- stays at it.  One entry at the wavefront's last position but
    one gives it a D of its own, `own`, `place` of the way from the chain up to s * (1 - 1e-4), the bound of a margin
    taken relative to s: below that bound the wavefront publishes `own` as final although the chain through ALL its
    positions beats it, and the next wavefront (the eight codons behind the run, at 2 * neg) starts from a stale D.
    xt: the xtrans row of a 16-codon read, multi hits, rounded to CANCEL_QUANT."""
    f32 = np.float32
    per = 64 * Q
    a, r, l = per, per, 3 * ANCHOR
    assert a + r + ANCHOR <= K and np.all(np.round(xt / CANCEL_QUANT) * CANCEL_QUANT == xt)
    prof = synth_profile(rng, K)
    kept = np.concatenate([np.arange(a - ANCHOR, a), np.arange(a + r, a + r + ANCHOR)])
    codons = rng.integers(0, 64, size=2 * ANCHOR)
    for k, c in zip(kept, codons):
        prof.match[CODE_OFF[2] + int(c), k] = f32(neg if k < a else 2 * neg)
    low = f32(0.25)
    prof.trans[0, 1:] += f32(3000.0)             # one way in: the first anchor ...
    prof.trans[0, a - ANCHOR] = low
    prof.trans[1, kept[1:]] = low
    prof.trans[3, a] = f32(0.0)                  # MD into the run
    prof.trans[6, a + r] = low                   # DM out of it
    prof.match[:, a : a + r] += f32(3000.0)      # nothing matches inside the run ...
    prof.trans[6, a + 1 : a + r] += f32(3000.0)  # ... and nothing leaves it before its end
    prof.trans[7, 1:] = f32(50.0)                # every other wavefront passes the test with room to spare
    # M of the anchor's rows, as the kernels and the reference add them: ((B + BM) + match) + MM ...
    m = f32(f32(f32(xt[3]) + low) + f32(neg))    # xt[3]: S -> B
    for _ in range(ANCHOR - 1):
        e_before, m = m, f32(f32(m + low) + f32(neg))
    E = m
    # the chain: step i leaves the exact sum `frac` of an ulp above a representable value, so fp32 rounds it down
    n = r - 1
    base = (land - float(E)) / n
    x, dd = E, np.zeros(n, f32)
    for i in range(n):
        g = float(np.spacing(f32(abs(x))))
        dd[i] = f32(np.floor((float(x) + base) / g) * g + frac * g - float(x))
        x = f32(x + dd[i])
    assert np.all(dd > 0)
    prof.trans[7, a + 1 : a + r] = dd
    chain = x
    tdd = wave_tdd(np.pad(prof.trans[7], (0, 64 * Q * 64)), Q, 1)
    s = f32(E + tdd)
    relative = min(f32(s * f32(0.9999)), f32(s * f32(1.0001)))         # the bound of a margin relative to s
    absolute = f32(float(s) - 1e-4 * (abs(float(E)) + float(tdd)))     # of one absolute in what is summed (to ~1 ulp)
    own = f32(float(chain) + place * (float(relative) - float(chain)))
    # wavefront 1's own D: B of row l - 3 (E of that row + E -> B) enters at its last position but one
    k = a + r - 2
    code = CODE_OFF[2] + int(codons[ANCHOR - 1])
    b = f32(e_before + f32(xt[5]))               # xt[5]: E -> B
    prof.trans[0, k] = low
    prof.match[code, k] = f32(-10.0 - float(f32(b + low)))
    prof.trans[3, k + 1] = f32(float(own) + 10.0)
    own = f32(f32(-10.0) + prof.trans[3, k + 1])
    read = np.stack([codons // 16, (codons // 4) % 4, codons % 4], axis=1).reshape(-1).astype(np.uint8)
    facts = dict(l=l, a=a, r=r, E=E, chain=chain, exact=float(E) + float(dd.astype(np.float64).sum()), tdd=tdd, s=s,
                 relative=relative, absolute=absolute, own=own)
    return prof, read, facts


# (Q, W, K, span) of the cancelling runs: every shape with a wavefront behind wavefront 1 (with two wavefronts nothing
# reads what the last one published)
CANCEL_SHAPES = ((4, 4, 1024, None), (6, 4, 1536, None), (8, 4, 2048, None), (8, 8, 2049, None), (8, 8, 4096, None),
                 (STRIP_Q, STRIP_W, 4097, STRIP))
