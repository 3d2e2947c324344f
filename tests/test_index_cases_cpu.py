"""The closed-form index tables of tests/index_cases.py on the CPU oracle: its
index is held to `where` (built from the insertion order alone), every missing
probe reports its error, and the cases' epochs decide by the formula and zero
F0 exactly at the written rows.  With that, a GPU result that differs from
the oracle is the engine's fault.  Also the probe's arithmetic
(deneva-plus_amd/csrc/dvcc_index_math.h) against exact 128-bit division in a
sanitized host program of its own, tests/cpp/index_math_test.cpp.
"""
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
import index_cases as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OCC_ID = {"NO_WAIT": O.NO_WAIT, "WAIT_DIE": O.WAIT_DIE, "OCC": O.OCC, "CALVIN": O.CALVIN}
NAMES = I.case_names()


def test_the_families_are_all_there():
    fam = {I.case(n).family for n in NAMES}
    assert fam == {"D1", "DP", "IM", "EN", "CH", "RP"}
    K = I.structural_constants()
    assert all(K[k] > 0 for k in ("kTagWide", "kMaxTables", "kPV", "kBlock", "kTile", "kProbeHistTiles"))
    # the structures the families are there for
    assert {(I.case(n).part_cnt, I.case(n).part_id) for n in NAMES if I.case(n).family == "DP"} == set(I.DP_PARTS)
    parts = {I.case(n).part_id for n in NAMES}
    assert K["kTagWide"] - 1 in parts and any(p >= K["kTagWide"] for p in parts)  # the last narrow home tag; a wide one
    rp = I.case("RP_mod_97")
    counts = {}
    for k in rp.keys:
        counts[k] = counts.get(k, 0) + 1
    assert {2, 3} <= set(counts.values())
    assert I.case("CH_empty_97").n == 0 and not I.case("CH_empty_97").where
    top = (1 << 64) - 1
    assert all(top in I.case(n).where for n in NAMES if I.case(n).family in ("IM", "EN"))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_index_is_where(name):
    c = I.case(name)
    t = I.oracle_table(c)
    if c.form == "ycsb":
        assert np.array_equal(t.f0, c.f0), "the loader's column"
    for k, row in c.where.items():  # every key, the labelled present probes among them
        assert I.oracle_read(t, k) == row, (name, k)
    for lab, k in c.present:
        assert I.oracle_read(t, k) == c.where[k], (name, lab)
    for lab, k in c.missing:
        assert k not in c.where and I.oracle_read(t, k) is None, (name, lab)


def _run(t, f0, cc, e):
    c, _, st = O.epoch_run(OCC_ID[cc], t.ix, f0, e.n_txn, e.txn_begin, e.keys, e.types)
    return c, st


@pytest.mark.parametrize("name", NAMES)
def test_oracle_epochs_follow_the_formula(name):
    c = I.case(name)
    t = I.oracle_table(c)
    for cc in I.CCS:
        f0 = c.f0.copy()
        written = []
        for what, ec in (("read", I.read_epoch(c)), ("write", I.write_epoch(c)), ("pair", I.pair_epoch(c))):
            got, st = _run(t, f0, cc, ec.epoch)
            assert np.array_equal(got, ec.expected[cc]), (name, cc, what)
            written += ec.written[cc]
            assert np.array_equal(f0, I.column_after(c, written)), (name, cc, what)
            assert st.committed == int(ec.expected[cc].sum())
            if what == "write":
                assert st.write_cnt == len(c.present_keys())
        zero = np.flatnonzero(f0[:c.n] == 0).tolist()  # (of the loaded rows)
        assert zero == sorted({c.where[k] for k in written}), (name, cc)


@pytest.mark.parametrize("name", NAMES)
def test_digest_formula_is_the_oracles(name):
    """index_cases.read_digest over the read epoch's committed reads of (value
    of where[key], txn, key) is the oracle's digest -- a row off changes it"""
    c = I.case(name)
    ks = c.present_keys()
    assert int(I.mix64([12345])[0]) == O.lib().or_mix64(12345)
    _, st = _run(I.oracle_table(c), c.f0.copy(), "NO_WAIT", I.read_epoch(c).epoch)
    assert st.read_digest == I.read_digest([c.f0[c.where[k]] for k in ks], range(len(ks)), ks)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_rejects_every_missing_probe(name):
    """a missing key anywhere in an epoch fails the oracle's epoch"""
    c = I.case(name)
    t = I.oracle_table(c)
    for lab, k in c.missing:
        e = I.pad_epoch(c, [k], 3)
        with pytest.raises(RuntimeError):
            _run(t, c.f0.copy(), "NO_WAIT", e)


@pytest.mark.parametrize("world", [2, 3])
def test_replicated_partitions(world):
    """the partitions of tests/index_cases.rep_group: the oracle's index over
    each partition's insertions holds every present key at its bucket's row
    and none of the missing ones; the home tag is the partition's own where
    home_q = 0 and another where home_q = 1"""
    for p, c in enumerate(I.rep_group(world)):
        t = I.oracle_table(c)
        for k, row in c.where.items():
            assert I.oracle_read(t, k) == row == c.bucket(k)
        for lab, k in c.present:
            assert k % world == p and I.oracle_read(t, k) == k // world, (c.name, lab)
        for lab, k in c.missing:
            assert I.oracle_read(t, k) is None, (c.name, lab)
        tags = [(k // world // c.nbuckets) * world + k % world for k in c.keys if k // world // c.nbuckets < I.W]
        home = max(set(tags), key=tags.count)
        assert (home == p) == (p % 2 == 0), (c.name, home)


def test_index_arithmetic_against_128_bit_division(tmp_path):
    exe = str(tmp_path / "index_math_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "deneva-plus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "index_math_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    out = r.stdout.split()
    assert int(out[1]) > 100_000 and out[2] == "corrections" and 1 <= int(out[3]) <= 2, r.stdout
