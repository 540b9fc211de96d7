"""CPU: pieces of the path that the REFERENCE's own code can check directly.  oracle/Makefile `ref` compiles,
unmodified where they lie in the reference tree, every c-core file of the path that needs nothing but libc and the
reference's own headers: viterbi.c (the DP, used by test_oracle.py), error.c, partition_size.c, state.c,
disambiguate.c, uppercase.c.  Here the product's host code (include/deciphon_host.h) and the oracle restatement are
compared with what those functions themselves answer: tests/golden/reference_pins.npz holds their answers on every
input used here (tests/golden/make_golden.py pins), and where oracle/_ref was built the functions are called live as
well and must still give what the record holds."""
import os

import numpy as np
import pytest

import deciphon_amd
from deciphon_amd import host
from dcp_testlib import GOLDEN, random_seq, ref_encode, ref_pins_lib, ref_state_name, reflib, synth_profile


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLDEN, "reference_pins.npz"))


@pytest.fixture(scope="module")
def ref():
    """The reference's functions (oracle/_ref) where they were built, else None."""
    r = reflib()
    return None if r is None else ref_pins_lib(r)


def _makers(ref):
    return (ref.state_make_match_id, ref.state_make_insert_id, ref.state_make_delete_id)  # M I D: tags 0 1 2


def test_partition_size_is_the_references(ref, orc, pins):
    """c-core/partition_size.c:13-16 against dcp_partition_size and the by-count partition bounds
    (c-core/protein_reader.c:112-128 sums the same sizes)."""
    off = 0
    for n, parts in pins["part_cases"]:
        n, parts = int(n), int(parts)
        want = [int(v) for v in pins["part_sizes"][off : off + parts]]
        off += parts
        if ref is not None:
            assert [ref.partition_size(n, parts, i) for i in range(parts)] == want, (n, parts)
        assert [host.partition_size(n, parts, i) for i in range(parts)] == want, (n, parts)
        assert [orc.partition_size(n, parts, i) for i in range(parts)] == want, (n, parts)
        if n > 0:
            f = host.partition_bounds(np.ones(n, np.int32), parts, False)
            assert [int(f[i + 1] - f[i]) for i in range(parts)] == want, (n, parts)
            assert int(f[-1]) == n == sum(want)
    assert off == len(pins["part_sizes"]) and len(pins["part_cases"]) == 208


def test_state_ids_are_the_references(ref, orc, pins):
    """c-core/state.c:25,92-96 (+ state.h:9-25): every id the unzip can emit -- M/I/D of every core index up to
    the 14-bit limit and the specials -- is named, classified and built the same way."""
    ks = [int(k) for k in pins["state_ks"]]
    assert ks == list(range(0, 300)) + [4095, 4096, 8191, 16382]
    for tag in range(3):
        for j, k in enumerate(ks):
            sid, name, mute = int(pins["state_ids"][tag, j]), str(pins["state_names"][tag, j]), bool(pins["state_mute"][tag, j])
            if ref is not None:
                assert _makers(ref)[tag](k) == sid and ref.state_core_idx(sid) == k
                assert ref_state_name(ref, sid) == name and bool(ref.state_is_mute(sid)) == mute
            assert sid == (tag << 14) | (k + 1)
            assert int(pins["state_core_idx"][tag, j]) == k
            assert host.state_name(sid) == name == orc.state_name(sid)
            assert host.state_is_mute(sid) == mute
    assert [int(s) for s in pins["special_ids"]] == [0xC000 | n for n in range(3, 10)]  # S, N, B, E, J, C, T
    for sid, name, mute in zip(pins["special_ids"], pins["special_names"], pins["special_mute"]):
        sid, name, mute = int(sid), str(name), bool(mute)
        if ref is not None:
            assert ref_state_name(ref, sid) == name and bool(ref.state_is_mute(sid)) == mute
        assert host.state_name(sid) == name == orc.state_name(sid)
        assert host.state_is_mute(sid) == mute
    if ref is not None:
        assert ref.state_make_end() == int(pins["state_end"])
    assert int(pins["state_end"]) == 0xC000 | 9


def test_unzipped_paths_hold_reference_state_ids(ref, orc, pins):
    """The ids of real unzipped paths (oracle trellis -> product's dcp_unzip) named and re-made as the reference's
    state.c names and makes them."""
    names = {int(s): str(n) for s, n in zip(pins["state_ids"].ravel(), pins["state_names"].ravel())}
    names.update({int(s): str(n) for s, n in zip(pins["special_ids"], pins["special_names"])})
    made = {(names[int(s)][0], int(k)): int(s) for row in pins["state_ids"] for k, s in zip(pins["state_ks"], row)}
    rng = np.random.default_rng(21)
    for it in range(60):
        K = int(rng.choice([2, 7, 33, 100, 257]))
        prof = synth_profile(rng, K, [None, 1.0][it % 2])
        seq = random_seq(rng, int(rng.integers(1, 120)))
        xt = orc.xtrans(max(len(seq) // 3, 1), bool(it % 2), False)
        _, xn, nd = orc.path(prof, xt, seq)
        ids, sizes = host.unzip(K, len(seq), xn, nd)
        for sid in ids:
            sid = int(sid)
            name = names[sid]
            if ref is not None:
                assert ref_state_name(ref, sid) == name
            assert name == host.state_name(sid)
            if name[0] in "MID":
                k = int(name[1:]) - 1
                if ref is not None:
                    assert _makers(ref)["MID".index(name[0])](k) == sid
                assert made[(name[0], k)] == sid and 0 <= k < K
        assert int(ids[-1]) == int(pins["state_end"])


def test_read_encoding_is_the_references(ref, orc, pins):
    """c-core/uppercase.c + c-core/disambiguate.c (sequence_setup's first steps, c-core/sequence.c:20-24) against
    dcp_encode_sequence (and the oracle's); symbol indices A, C, G, T|U = 0..3: imm's DNA / RNA alphabets, SURVEY 8a
    row S."""
    assert len(pins["enc_cases"]) == 1212
    for s, rc, text in zip(pins["enc_cases"], pins["enc_rc"], pins["enc_texts"]):
        s, rc, text = str(s), int(rc), str(text)
        if ref is not None:
            assert ref_encode(ref, s) == (rc, text), s
        assert rc == 0, s
        assert len(text) == len(s) and set(text) <= set("ACGTU"), (s, text)
        want = np.array(["ACGTU".index(c) if c != "U" else 3 for c in text], np.uint8)
        assert np.array_equal(deciphon_amd.encode(s), want), (s, text)
        assert np.array_equal(orc.encode(s), want), (s, text)
    # T and U in one read: the reference refuses (DCP_ENUCLTSEQTU), so does the product
    rc = int(pins["enc_tu_rc"])
    if ref is not None:
        assert ref_encode(ref, "ACGTU")[0] == rc
    assert rc == 74
    with pytest.raises(deciphon_amd.HipError) as e:
        deciphon_amd.encode("ACGTU")
    assert e.value.code == rc


def test_error_strings_are_the_references(ref, pins):
    """c-core/error.c's table (dcp_error_string) against the product's, for every code and beyond."""
    assert [int(c) for c in pins["err_codes"]] == list(range(-2, 125))
    holes = []
    for code, null, want in zip(pins["err_codes"], pins["err_null"], pins["err_strings"]):
        code, null, want = int(code), bool(null), str(want)
        if ref is not None:
            live = ref.dcp_error_string(code)
            assert (live is None) == null and (live or b"").decode() == want, code
        if null:  # a hole in the reference's designated-initialiser table: it returns NULL there
            holes.append(code)
            assert deciphon_amd.error_string(code) == ""  # the product returns an empty string, never NULL
        else:
            assert deciphon_amd.error_string(code) == want, code
    assert holes == [62]
