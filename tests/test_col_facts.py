"""Column facts of a batch (kyv_batch_col_facts, kyv_layout.h ColFacts): what the flattener reports for crafted batches
must equal a straightforward recomputation from the documents -- a list in the last lane of a wave only, in the first
resource of the next wave only, a nested list in one container of one resource, list positions that hold something
other than a list, a wave that spans two kinds; the rows do not depend on the thread count; KYV_FACT_COLS=0 reports
"nothing known". What KYV_JIT_COLFACTS does to the generated source, and the
oracle's view of the parity corpus (computed once, shared with test_gpu_col_facts.py)."""
import collections
import copy
import functools
import hashlib
import re

import numpy as np
import pytest

import cases
import col_facts_cases as M
import parity_util as PU
from kyverno_amd import engine as E


@pytest.fixture(scope="module")
def ruleset():
    return E.Ruleset(M.policies())


def check_rows(ruleset, docs, threads=0):
    b = E.Batch(ruleset, docs, threads=threads)
    order = b.wave_facts()["order"]
    f = b.col_facts()
    assert f["rows"].shape == ((len(docs) + 63) // 64,)
    assert [int(e) for e in f["rows"]] == M.expected_rows(docs, order, f)
    f["order"] = order
    return f


def wave_of(f, doc_index):
    return int(np.nonzero(f["order"] == doc_index)[0][0]) // 64


def list_bit(f, *path):
    return f["lists"].index(list(path))


@pytest.fixture
def input_order(monkeypatch):
    """batches in input order within a kind, so that a document's index is its lane"""
    monkeypatch.setenv("KYV_SHAPE_ORDER", "0")


@pytest.mark.parametrize("n", M.SIZES)
def test_clean_batch(ruleset, n):
    f = check_rows(ruleset, M.clean(n))
    assert 0 < len(f["lists"])
    for e in f["rows"]:
        assert not (int(e) >> list_bit(f, "spec", "containers")) & 1
        for path in (("spec", "initContainers"), ("spec", "ephemeralContainers"), ("spec", "containers", "[*]", "ports"),
                     ("spec", "template", "spec", "containers")):
            assert (int(e) >> list_bit(f, *path)) & 1, path


@pytest.mark.parametrize("n", M.SIZES)
def test_list_in_the_last_lane_of_a_wave(ruleset, input_order, n):
    at = min(n, 64) - 1
    docs = M.clean(n)
    docs[at]["spec"]["ephemeralContainers"] = [M.good_container("debug")]
    f = check_rows(ruleset, docs)
    assert list(f["order"]) == list(range(n))
    eph = list_bit(f, "spec", "ephemeralContainers")
    assert [(int(e) >> eph) & 1 for e in f["rows"]] == [0] + [1] * (len(f["rows"]) - 1)


def test_list_in_the_first_resource_of_the_next_wave(ruleset, input_order):
    for n in (65, 130):
        docs = M.clean(n)
        docs[64]["spec"]["initContainers"] = [M.good_container("init")]
        f = check_rows(ruleset, docs)
        init = list_bit(f, "spec", "initContainers")
        assert [(int(e) >> init) & 1 for e in f["rows"]] == [1, 0] + [1] * (len(f["rows"]) - 2)


@pytest.mark.parametrize("n", M.SIZES)
def test_ports_in_one_container_of_one_resource(ruleset, n):
    docs = M.clean(n)
    at = n - 1
    docs[at]["spec"]["containers"].append(dict(M.good_container("web"), ports=[{"containerPort": 8080}]))
    f = check_rows(ruleset, docs)
    ports = list_bit(f, "spec", "containers", "[*]", "ports")
    for w, e in enumerate(f["rows"]):
        assert (int(e) >> ports) & 1 == (w != wave_of(f, at))


@pytest.mark.parametrize("value", M.ODD_LISTS, ids=repr)
def test_a_list_position_that_holds_something_is_not_empty(ruleset, value):
    for member, nested in (("initContainers", False), ("ports", True)):
        docs = M.clean(130)
        (docs[70]["spec"]["containers"][0] if nested else docs[70]["spec"])[member] = copy.deepcopy(value)
        f = check_rows(ruleset, docs)
        bit = list_bit(f, "spec", "containers", "[*]", "ports") if nested else list_bit(f, "spec", member)
        for w, e in enumerate(f["rows"]):
            assert (int(e) >> bit) & 1 == (w != wave_of(f, 70)), (member, value)


def test_a_wave_that_spans_two_kinds(ruleset):
    for n in M.SIZES:
        docs = M.clean(n) + [M.deployment(i) for i in range(n)]
        docs[n - 1]["spec"]["ephemeralContainers"] = [M.good_container("debug")]
        docs[n]["spec"]["template"]["spec"]["initContainers"] = ["x"]
        docs[2 * n - 1]["spec"]["template"]["spec"]["securityContext"] = 5
        f = check_rows(ruleset, docs)
        kinds = [docs[int(p)]["kind"] for p in f["order"]]
        if n % 64:
            w = n // 64
            assert len(set(kinds[64 * w:64 * w + 64])) == 2  # the wave at the kind boundary holds both kinds


@pytest.mark.parametrize("threads", [2, 3, 8])
def test_rows_do_not_depend_on_the_thread_count(ruleset, threads):
    docs = M.clean(130)
    docs[63]["spec"]["ephemeralContainers"] = [M.good_container("debug")]
    docs[64]["spec"]["initContainers"] = []
    docs[65]["spec"]["containers"][0]["securityContext"]["capabilities"] = "x"
    docs[100]["spec"]["containers"][0]["ports"] = [{"containerPort": 1}]
    serial = check_rows(ruleset, docs, threads=1)
    par = check_rows(ruleset, docs, threads=threads)
    assert np.array_equal(serial["rows"], par["rows"])


def test_switch_reports_nothing_known(ruleset, monkeypatch):
    b = E.Batch(ruleset, M.clean(130))
    on = b.col_facts()["rows"]
    assert on.all()
    monkeypatch.setenv("KYV_FACT_COLS", "0")
    assert (b.col_facts()["rows"] == 0).all()
    monkeypatch.delenv("KYV_FACT_COLS")
    assert np.array_equal(b.col_facts()["rows"], on)
    assert b.wave_facts()["facts"].all()  # (the all-maps facts have their own switch)


# ---------------------------------------------------------------- generated source
def source(pols):
    return E.Ruleset(pols).jit_source()[0]


def clear_switches(monkeypatch):
    for name in ("KYV_JIT_COLFACTS", "KYV_JC_PRELOAD", "KYV_META_KEYS"):
        monkeypatch.delenv(name, raising=False)


def test_switch_off_restores_the_source(monkeypatch):
    """KYV_JIT_COLFACTS=0: the source of the C3 ruleset is, byte for byte, what the commit before the column facts
    generated (size and hash recorded from that commit: golden/col_facts_parent_source.json); so it is whenever
    KYV_JC_PRELOAD=0 or KYV_META_KEYS=0 asks for the source of an earlier round"""
    clear_switches(monkeypatch)
    on = source(M.policies())
    monkeypatch.setenv("KYV_JIT_COLFACTS", "0")
    off = source(M.policies())
    parent = cases.load("col_facts_parent_source.json")
    assert len(off.encode()) == parent["bytes"] and hashlib.sha256(off.encode()).hexdigest() == parent["sha256"]
    assert "wave_cols(" not in off and "jc_empty(" not in off and "kColFacts" not in off
    assert "wave_cols(v, w).empty" in on and "jc_empty(v, r)" in on and "w.ce = ce;" in on
    monkeypatch.delenv("KYV_JIT_COLFACTS")
    assert source(M.policies()) == on
    for name in ("KYV_JC_PRELOAD", "KYV_META_KEYS"):
        monkeypatch.setenv(name, "0")
        src = source(M.policies())
        assert "wave_cols(" not in src and "jc_empty(" not in src
        monkeypatch.setenv("KYV_JIT_COLFACTS", "1")  # asked for or not
        assert source(M.policies()) == src
        monkeypatch.delenv("KYV_JIT_COLFACTS")
        monkeypatch.delenv(name)


def test_default_source_reads_the_plane_and_compiles_for_gfx950(monkeypatch):
    clear_switches(monkeypatch)
    monkeypatch.setenv("KYV_JIT_CACHE", "0")  # compile for real; keep the in-tree code-object cache untouched
    rs = E.Ruleset(M.parity_policies())
    src = rs.jit_source()[0]
    # root scopes, LDS root-cache fills and the condition rules' member loads all take the empty bit as their row
    assert "ce >> " in src and "? NONE : row)" in src and "(((ce >> " in src
    # the condition rules read the wave's word once per rule function and hand it down
    assert src.count("jc_empty(v, r)") == len(re.findall(r"uint8_t jr\d+\(const View& v", src)) > 0
    secs, size = rs.jit_compile()
    assert size > 1000


# ---------------------------------------------------------------- the parity corpus
@functools.lru_cache(maxsize=None)
def oracle():
    docs, nsl = M.parity_corpus()
    return PU.oracle_pairs(M.parity_policies(), docs, nsl)


def test_parity_corpus_is_decided_by_the_oracle():
    """no pair is nondeterministic or unsupported, so the GPU runs leave none out; every kind is more than a wave and
    no multiple of one; every rule passes and fails somewhere"""
    docs, _ = M.parity_corpus()
    kinds = collections.Counter(d["kind"] for d in docs)
    assert all(kinds[k] > 64 and kinds[k] % 64 for k in ("Pod", "Deployment", "CronJob")), kinds
    n = collections.defaultdict(collections.Counter)
    for (pol, rule, ri), rr in oracle().items():
        n[(pol, rule)][rr["status"]] += 1
        n[(pol, rule)]["nd"] += bool(rr.get("nondeterministic"))
    assert len(n) >= 3 * (len(M.PATTERN_POLICIES) + 4), sorted(n)
    for key, c in n.items():
        assert c["nd"] == 0 and c["unsupported"] == 0, (key, c)
        assert c["pass"] > 0 and c["fail"] > 0, (key, c)


def test_cpu_backend_parity():
    docs, nsl = M.parity_corpus()
    ora = oracle()
    saved = PU.oracle_pairs
    PU.oracle_pairs = lambda *a, **k: ora
    try:
        st, _ = PU.compare(M.parity_policies(), docs, nsl, backend="cpu")
    finally:
        PU.oracle_pairs = saved
    assert st["nbad"] == 0, st["bad"]
    assert st["nd"] == 0 and st["compared"] > 5000, st
