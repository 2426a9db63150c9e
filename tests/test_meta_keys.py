"""The meta-key plane on the CPU (generators and the Python model: meta_keys_cases.py): the rows the host computes
(kyv_batch_meta_keys) against the documents, the corpus's coverage, and what the generated source does with the plane."""
import collections
import functools
import hashlib
import re

import pytest

import cases
import meta_keys_cases as M
import parity_util as PU
from kyverno_amd import engine as E

OVERRIDES = ("none-resolved", "none-unresolved", "panic", "fallback", "nd")


@functools.lru_cache(maxsize=None)
def built(name):
    """(ruleset, batch, plane of the host, batch order) of one test ruleset over the corpus"""
    docs, nsl, _ = M.corpus()
    rs = E.Ruleset(M.ruleset(name))
    b = E.Batch(rs, docs, nsl)
    return rs, b, b.meta_keys(), b.wave_facts()["order"]


@functools.lru_cache(maxsize=None)
def oracle(name):
    """the oracle's rule results of one test ruleset over the corpus (computed once, shared with the GPU tests)"""
    docs, nsl, _ = M.corpus()
    return PU.oracle_pairs(M.ruleset(name), docs, nsl)


def row_class(cls, want):
    if want["st"] != M.ST_NONE:
        return {M.ST_PANIC: "panic", M.ST_FALLBACK: "fallback", M.ST_ND: "nd"}[want["st"]]
    globs = cls["wild_labels"] + cls["wild_annotations"]
    return "none-resolved" if any(k != g for k, g in zip(want["keys"], globs)) else "none-unresolved"


def test_glob_model():
    assert M.glob("a/*", "a/") and M.glob("a/*", "a/*") and M.glob("a/?*", "a/x") and not M.glob("a/?*", "a/")
    assert not M.glob("a/*", "b/c") and M.glob("team-*", "team-*") and M.glob("?", "*") and not M.glob("", "x")


@pytest.mark.parametrize("name", ["apparmor", "two_slot", "indirect"])
def test_classes(name):
    rs, b, mk, _ = built(name)
    assert [c["pos"] for c in mk["classes"]] == [0, 1, 2]
    two = name == "two_slot"
    for c in mk["classes"]:
        assert c["annotations"] and c["labels"] == two
        assert len(c["wild_annotations"]) == 1 and len(c["wild_labels"]) == (1 if two else 0)
    assert mk["rows"].shape == (3, b.n, 4)


def test_no_class_ruleset_has_no_plane():
    rs, b, mk, _ = built("no_class")
    assert mk["classes"] == [] and mk["rows"].shape == (0, b.n, 4)
    kinds = {r["name"]: r["kind"] for r in rs.rules}
    assert kinds == {"claim-annotation": "fallback", "job-annotation": "pattern"}, kinds


@pytest.mark.parametrize("name", ["apparmor", "two_slot", "indirect", "same_shape"])
def test_host_rows_match_documents(name):
    docs, _, tags = M.corpus()
    rs, b, mk, order = built(name)
    bad = []
    for c, cls in enumerate(mk["classes"]):
        for p in range(b.n):
            want, got = M.model_row(cls, docs[order[p]]), mk["decoded"][c][p]
            word0 = int(mk["rows"][c, p, 0])
            assert word0 >> 28 == got["st"]
            if want["st"] != got["st"] or (want["st"] == M.ST_NONE and (want["keys"], want["values"]) != (got["keys"], got["values"])):
                bad.append((c, tags[order[p]], want, got))
    assert not bad, bad[:5]


def test_corpus_is_not_vacuous():
    """every override class in at least 3 (class, resource) pairs at every position, for the one-slot and the two-slot
    classes; all three verdicts among the oracle's results; kind boundaries and a partial last wave inside waves"""
    docs, _, _ = M.corpus()
    for name in ("apparmor", "two_slot"):
        rs, b, mk, order = built(name)
        for cls in mk["classes"]:
            n = collections.Counter(row_class(cls, M.model_row(cls, d)) for d in docs)
            assert all(n[o] >= 3 for o in OVERRIDES), (name, cls["pos"], n)
    seen = collections.Counter()
    for name in M.RULESETS:
        for rr in oracle(name).values():
            seen[rr["status"]] += 1
            seen["nd"] += bool(rr.get("nondeterministic"))
    assert all(seen[s] >= 3 for s in ("pass", "fail", "skip", "panic", "nd")), seen
    rs, b, mk, order = built("apparmor")
    kinds = [docs[i]["kind"] for i in order]
    assert b.n % 64 not in (0, 63) and b.n > 128
    assert any(len(set(kinds[w:w + 64])) > 1 for w in range(0, b.n, 64))


@pytest.mark.parametrize("name", list(M.RULESETS))
def test_cpu_backend_parity(name):
    docs, nsl, _ = M.corpus()
    st, _ = PU.compare(M.ruleset(name), docs, nsl, backend="cpu")
    assert st["nbad"] == 0, st["bad"]
    assert st["compared"] > 20


# ---------------------------------------------------------------- generated source
def source(pols):
    return E.Ruleset(pols).jit_source()[0]


def kernels(src):
    return sorted(line.split("(")[0] for line in src.split("\n") if line.startswith("kyv_jit_"))


def c3_policies():
    return cases.best_practices() + cases.chart_restricted()


def test_c3_source_reads_the_plane():
    src = source(c3_policies())
    assert "expand_meta" not in src
    assert "kyv_jit_fused_1" not in kernels(src) and "kyv_jit_fused_0" in kernels(src)
    assert src.count("jc_meta(") >= 3


def test_switch_off_restores_the_source(monkeypatch):
    """KYV_META_KEYS=0: the source is, byte for byte, what the commit before the plane generated for this ruleset
    (its size and hash, recorded from that commit: golden/meta_keys_parent_source.json) -- the heavy kernel and its
    expand_meta calls are back, and nothing of the plane is left in it. The recorded size and hash hold while the
    generator's output for this ruleset is that commit's: a later change to what jit.cpp emits records them again from
    its own parent, or drops that one assertion; the structural assertions below are the ones that last."""
    on = source(c3_policies())
    monkeypatch.setenv("KYV_META_KEYS", "0")
    off = source(c3_policies())
    parent = cases.load("meta_keys_parent_source.json")
    assert len(off.encode()) == parent["bytes"] and hashlib.sha256(off.encode()).hexdigest() == parent["sha256"]
    assert "kyv_jit_fused_1" in kernels(off) and "jc_meta(" not in off and "MK_" not in off
    assert off.count("expand_meta_root(") == 1 and off.count("expand_meta(") == 2
    assert hashlib.sha1(on.encode()).digest() != hashlib.sha1(off.encode()).digest()
    monkeypatch.delenv("KYV_META_KEYS")
    assert source(c3_policies()) == on


def test_same_shape_rules_load_their_own_class():
    """rules whose patterns differ in the glob alone have different classes and do not share a root function: every
    rule's root function loads the plane row of the class that stands for the rule's position and glob"""
    pols = M.ruleset("same_shape")
    rs = E.Ruleset(pols)
    docs, nsl, _ = M.corpus()
    classes = E.Batch(rs, docs[:4], nsl).meta_keys()["classes"]
    assert len(classes) == 6
    src = rs.jit_source()[0]
    for k, r in enumerate(rs.rules):
        pos = 2 if r["name"].startswith("autogen-cronjob-") else 1 if r["name"].startswith("autogen-") else 0
        want = [i for i, c in enumerate(classes)
                if c["pos"] == pos and c["wild_annotations"] == [M.SAME_SHAPE_GLOBS[r["name"][-4:]]]]
        assert len(want) == 1, (r["name"], classes)
        blk = src[src.index("    if (%du >= o.rule_lo" % k):]
        fn = re.search(r"(rootc?\d+(?:_\d+)?)\(vl, ", blk).group(1)
        body = src[src.index("void %s(" % fn):]
        body = body[:body.index("\n}\n")]
        assert [int(x) for x in re.findall(r"jc_meta\(v, (\d+)u", body)] == want, (r["name"], fn)
    loads = sorted(set(int(x) for x in re.findall(r"jc_meta\(v, (\d+)u", src)))
    assert loads == list(range(6))


def test_no_class_rule_keeps_expand_meta():
    """a wildcard site at no static position still calls expand_meta, in a heavy group of its own"""
    src = source(M.ruleset("no_class") + M.ruleset("apparmor"))
    assert src.count("expand_meta(") == 1 and "jc_meta(" in src
    ks = kernels(src)
    assert "kyv_jit_fused_0" in ks and "kyv_jit_fused_1" in ks and "kyv_jit_fused_1p1" not in ks
    heavy = src[src.index("struct JitFused1 "):]
    heavy = heavy[:heavy.index("\n};\n")]
    rs = E.Ruleset(M.ruleset("no_class") + M.ruleset("apparmor"))
    k = [r["name"] for r in rs.rules].index("job-annotation")
    assert heavy.count("pair_walk_alts(") == 1 and "%du >= o.rule_lo" % k in heavy
