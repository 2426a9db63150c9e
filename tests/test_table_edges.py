"""CPU side of the table-edge parity tests (generators: table_edge_cases.py; the GPU runs: test_gpu_table_edges.py):
the wildcard restatement against the reference's own vectors, the explicit CPU instantiation against the oracle on every
case, the ruleset side of the plan report, that the oracle alone finds the cases non-vacuous, and the label-selector
cases whose outcome depends on Go map order."""
import functools
import json

import numpy as np
import pytest

import parity_util as PU
import table_edge_cases as T
from kyverno_amd import _lib as K
from oracle import oracle as O


# ---------------------------------------------------------------- 3a
def test_restatement_reproduces_reference_vectors(golden):
    recs = golden("wildcard.json")
    assert len(recs) == 52
    for r in recs:
        assert T.go_match(r["pattern"], r["text"]) == r["matched"], r
    pats, texts = T.wildcard_vectors()
    assert len(pats) >= 35 and len(texts) >= 45  # 94 + the patterns must pass the 128 mask bits
    for p in pats:  # and the oracle's matcher is the same function on the whole vector set
        for t in texts:
            assert O.wildcard(p, t) == T.go_match(p, t), (p, t)


def _status_by_rule(rs, res):
    return {r["name"]: np.asarray(res.status)[k] for k, r in enumerate(rs.rules)}


def check_match_routes(pats, rs, res, docs):
    """routes (i), (ii), (iv) against the restatement: the rule of glob g has a response exactly for the ConfigMaps
    whose name / namespace / fixed-key annotation value / some annotation key it matches"""
    st = _status_by_rule(rs, res)
    n = 0
    for g, p in enumerate(pats):
        for ri, d in enumerate(docs):
            if d["kind"] != "ConfigMap":
                continue
            md = d["metadata"]
            want = {"name-%d" % g: T.go_match(p, md["name"]), "ns-%d" % g: T.go_match(p, md["namespace"]),
                    "annv-%d" % g: T.go_match(p, md["annotations"][T.FIXED_KEY]),
                    "annk-%d" % g: any(T.go_match(p, k) for k in md["annotations"])}
            for rule, w in want.items():
                got = int(st[rule][ri]) != K.ST_NONE
                assert got == w, (rule, p, md, K.STATUS_NAMES[int(st[rule][ri])])
                n += 1
    return n


def check_rung(rung, backend, jit=None):
    """one rung of the mask ladder through both rulesets; returns the two plan reports"""
    _, offset, pats, epats = rung
    docs = T.vector_resources()
    plans = []
    for pols in (T.match_route_policies(offset, pats), T.eval_route_policies(offset, epats)):
        st, res = PU.compare(pols, docs, {}, backend=backend, jit=jit)
        assert st["nbad"] == 0, st["bad"]
        assert st["nd"] == 0 and st["fallback"] == 0, st
        if backend == "gpu":
            assert bool(res.jit) == jit
        rs = res.ruleset
        assert len(rs.rules) <= 200 and len(docs) <= 60
        if pols[0]["metadata"]["name"] == "vec-match":
            assert check_match_routes(pats, rs, res, docs) > 1000
        else:
            assert st["counts"]["fail"] > 50 and st["counts"]["pass"] > 50, st["counts"]
        plans.append(res.plan())
    return plans


def check_rung_plan(rung, plans):
    """the mask regime a rung claims: half sets one word; the ladder 2, 3, 4 words, then past the 128 bits"""
    rid, offset, pats, epats = rung
    for p, words, npat in zip(plans, T.RUNG_WORDS[rid], (len(T.masked_literals(pats)), len(T.masked_literals(epats)))):
        assert p["gmask_words"] == words == (p["gmask_patterns"] + p["cond_sets"] + 31) // 32, (rid, p)
        assert p["gmask_patterns"] >= min(128, offset + npat), (rid, p)
        assert (p["unmasked_literals"] > 0) == (rid in ("pad94", "pad126")), (rid, p)
        assert p["gmask_patterns"] + p["cond_sets"] <= 128
    ev = plans[1]  # the condition sets come after the pattern bits and stop at 128: fewer sets than conditions
    assert (ev["cond_sets"] < len(epats)) == (rid in ("pad62", "pad94", "pad126")), (rid, ev)
    assert (ev["cond_sets"] == 0) == (rid in ("pad94", "pad126")), (rid, ev)


@pytest.mark.parametrize("rung", T.vector_rungs(), ids=lambda r: r[0])
def test_wildcard_routes_cpu_instantiation(rung):
    plans = check_rung(rung, "cpu")
    check_rung_plan(rung, plans)
    for p in plans:  # nothing of the device side on the CPU backend
        assert p["slices"] == [] and p["fast_records"] == 0 and not any(p["tail_used"].values())


def test_mask_ladder_covers_one_to_four_words():
    assert {w for ws in T.RUNG_WORDS.values() for w in ws} == {1, 2, 3, 4}
    assert set(T.RUNG_WORDS) == {r[0] for r in T.vector_rungs()}


# ---------------------------------------------------------------- 3b
@functools.lru_cache(maxsize=None)
def table_case(case, small=False):
    """(policies, docs, ns labels, oracle names, oracle matrix, oracle FAIL texts) of one vocabulary, computed once and
    shared by the CPU and GPU tests"""
    pols = T.table_policies(case)
    docs, nsl = T.table_corpus_small() if small else T.table_corpus()
    names, m, tx = O.validate_matrix(pols, docs, nsl, threads=8, texts=("fail",))
    return pols, docs, nsl, names, m, tx


@pytest.mark.parametrize("case", list(T.VOCAB))
def test_table_cases_oracle_non_vacuous(case):
    """from the oracle alone: ND / unsupported pairs are at most 5 % of the matched ones, every rule family (what its
    first filter carries) has matched and unmatched pairs, and FAIL pairs exist"""
    pols, docs, nsl, names, m, _ = table_case(case)
    matched = int((m != 0).sum())
    soft = int(((m == 6) | (m == 7)).sum())
    assert matched > 10000, matched
    assert soft <= 0.05 * matched, (soft, matched)
    assert int((m == 2).sum()) > 500 and int((m == 1).sum()) > 500
    fam = {}
    row = {nm: i for i, nm in enumerate(names)}
    for p in pols:
        rule = p["spec"]["rules"][0]
        res = rule["match"]["any"][0]["resources"]
        sel = res.get("selector") or {}
        keys = [k for k in ("names", "name", "namespaces", "namespaceSelector", "annotations") if k in res]
        if sel:
            wild = any("*" in k + v or "?" in k + v for k, v in (sel.get("matchLabels") or {}).items())
            keys.append("selector-wild" if wild else "selector")
        if "exclude" in rule:
            keys.append("exclude")
        if any("/" in k for k in res["kinds"]):
            keys.append("gv-kinds")
        r = m[row[(p["metadata"]["name"], rule["name"])]]
        for k in keys or ["kinds-only"]:
            f = fam.setdefault(k, [0, 0])
            f[0] += int((r != 0).sum())
            f[1] += int((r == 0).sum())
    for k in ("names", "name", "namespaces", "namespaceSelector", "annotations", "selector", "selector-wild", "exclude",
              "gv-kinds"):
        assert fam[k][0] > 0 and fam[k][1] > 0, (k, fam)


@pytest.mark.parametrize("case", list(T.VOCAB))
def test_table_cases_cpu_instantiation(case, monkeypatch):
    pols, docs, nsl, names, m, tx = table_case(case)
    monkeypatch.setattr(O, "validate_matrix", lambda *a, **k: (names, m, tx))
    st, res = PU.compare_matrix(pols, docs, nsl, backend="cpu", texts=True)
    assert st["nbad"] == 0, st["bad"]
    assert st["texts"]["fail_pairs"] > 500 and st["texts"]["messages_compared"] > 500, st["texts"]
    p = res.plan()
    nglobs = p["gmask_patterns"] + p["cond_sets"]
    assert (nglobs <= 32) == (case == "within"), p
    assert p["gmask_words"] == (nglobs + 31) // 32 and p["unmasked_literals"] == 0, p


# ---------------------------------------------------------------- label selectors and Go map order
# ReplaceInSelector (pkg/engine/wildcards/wildcards.go:13-48): every matchLabels entry with '*' / '?' in its key or value
# becomes the FIRST label of the resource, in Go map order, whose key and value match it (expandWildcards), or itself
# with the wildcard characters replaced by '0' when none does; the entries are written into one result map in the map
# order of the selector. CheckSelector (pkg/utils/match/labels.go:10-24) then builds a selector from the result
# (NewRequirement validates each key and value: an invalid one is an error) and matches it against the labels. An
# error and a mismatch both leave the rule unmatched.
# The device decides a filter's selector in three places, and each case runs through all of them: "facts" leaves
# the filter as it is (a staged match record decided from the lane tail facts, tail_facts / match_fast), "tail" adds a
# namespace selector with a wildcard entry, which the facts never cover (cb_tail / match_rule_rec), and "generic" adds
# a third name, which no record holds (match_walk_generic_kernel: match_rule itself).
VARIANTS = ("facts", "tail", "generic")
SELECTOR_NS_LABELS = {"d": {"team": "x"}}


def _selector_rule(name, where, sel, variant):
    filt = {"selector": sel}
    if variant == "tail":
        filt["namespaceSelector"] = {"matchLabels": {"te*": "*"}}  # one valid hit in SELECTOR_NS_LABELS: holds
    elif variant == "generic":
        filt["names"] = ["p*", "q", "r"]  # every resource is named p<i>
    rule = {"name": name, "validate": {"pattern": {}}}
    if where == "match":
        rule["match"] = {"any": [{"resources": dict(filt, kinds=["Pod"])}]}
    else:
        rule["match"] = {"any": [{"resources": {"kinds": ["Pod"]}}]}
        rule["exclude"] = {"any": [{"resources": filt}]}
        if where == "exclude+certain":  # a second filter that excludes on every order
            rule["exclude"]["any"].append({"resources": {"kinds": ["Pod"]}})
    return rule


def _labelled(i, labels):
    return {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "p%d" % i, "namespace": "d", "labels": labels}}


_WILD = {"matchLabels": {"label-*": "*"}}
_WILD_ZZ = {"matchLabels": {"label-*": "*"}, "matchExpressions": [{"key": "zz", "operator": "Exists"}]}
_MIXED = {"label-a": "x", "label-b": "bad value"}  # "bad value" is no label value: choosing it is a NewRequirement error

SELECTOR_CASES = [
    # (id, where the selector stands, selector, labels, the selector's outcome set by wildcards.go, expected status)
    # one entry, two valid hits: the selector becomes {label-a: x} or {label-b: y}; both match -> {match}
    ("two-valid-hits", "match", _WILD, {"label-a": "x", "label-b": "y"}, {"match"}, "pass"),
    # one entry, no hit: it becomes {label-0: 0}, which the labels do not carry -> {no match}
    ("no-hit", "match", _WILD, {"app": "x"}, {"no match"}, "none"),
    # one entry, a valid and an invalid hit: {label-a: x} matches, {label-b: bad value} is an error -> {match, error}
    ("valid-and-invalid-hit", "match", _WILD, _MIXED, {"match", "error"}, "nondeterministic"),
    # the same with the invalid label first in sorted order (an implementation that takes the first hit it meets sees
    # the error first and must still keep the response) -> {match, error}
    ("invalid-hit-sorts-first", "match", _WILD, {"label-a": "bad value", "label-b": "x"}, {"match", "error"},
     "nondeterministic"),
    # the same beside an expression that fails: {label-a: x} + Exists(zz) does not match, the other choice is an error;
    # neither leaves the rule matched -> {no match, error}, no response on any order
    ("valid-and-invalid-hit-expression-fails", "match", _WILD_ZZ, _MIXED, {"no match", "error"}, "none"),
    # one entry beside an expression that holds: every valid choice matches -> {match}
    ("two-valid-hits-expression-holds", "match",
     {"matchLabels": {"label-*": "*"}, "matchExpressions": [{"key": "label-b", "operator": "In", "values": ["y", "z"]}]},
     {"label-a": "x", "label-b": "y"}, {"match"}, "pass"),
    # ... and one that fails on the chosen key's sibling: still independent of the choice -> {no match}
    ("two-valid-hits-expression-fails", "match",
     {"matchLabels": {"label-*": "*"}, "matchExpressions": [{"key": "label-b", "operator": "DoesNotExist"}]},
     {"label-a": "x", "label-b": "y"}, {"no match"}, "none"),
    # two entries that can write one key: "label-*": "*" becomes {label-a: x} and "label-a": "y" stays; the entry
    # written last wins, {label-a: x} matches and {label-a: y} does not -> {match, no match}. The evaluator sends
    # selectors with a wildcard entry beside other entries to the reference engine (FALLBACK), which the harness accepts
    ("two-entries-one-key", "match", {"matchLabels": {"label-*": "*", "label-a": "y"}}, {"label-a": "x"},
     {"match", "no match"}, "fallback"),
    # two entries on different keys, one hit each: {label-a: x, app: web} on every order -> {match}; FALLBACK all the same
    ("two-entries-two-keys", "match", {"matchLabels": {"label-*": "*", "app": "web"}}, {"label-a": "x", "app": "web"},
     {"match"}, "fallback"),
    # the selector in an exclude block: the rule has a response on the orders where the selector does NOT match.
    # two valid hits -> {match}: excluded on every order
    ("exclude-two-valid-hits", "exclude", _WILD, {"label-a": "x", "label-b": "y"}, {"match"}, "none"),
    # a valid and an invalid hit -> {match, error}: excluded on one order, a response on the other. The first order an
    # implementation tries may well be the excluded one; the response and its flag must survive that
    ("exclude-valid-and-invalid-hit", "exclude", _WILD, _MIXED, {"match", "error"}, "nondeterministic"),
    ("exclude-invalid-hit-sorts-first", "exclude", _WILD, {"label-a": "bad value", "label-b": "x"}, {"match", "error"},
     "nondeterministic"),
    # beside an expression that fails -> {no match, error}: never excluded, a plain response
    ("exclude-valid-and-invalid-hit-expression-fails", "exclude", _WILD_ZZ, _MIXED, {"no match", "error"}, "pass"),
    # beside a second filter that excludes on every order: no response whatever the selector does
    ("exclude-valid-and-invalid-hit-beside-certain-exclusion", "exclude+certain", _WILD, _MIXED, {"match", "error"},
     "none"),
]


def check_selector_cases(variant, backend, **kw):
    """every case as rule c<i> of one ruleset and resource i of one batch; the whole rule x resource matrix goes through
    the parity harness (one-sided ND is a mismatch), the case's own pair is checked against the outcome set derived
    above on both sides. Returns the evaluation."""
    pols = [T.policy("sel", [_selector_rule("c%d" % i, c[1], c[2], variant) for i, c in enumerate(SELECTOR_CASES)])]
    docs = [_labelled(i, c[3]) for i, c in enumerate(SELECTOR_CASES)]
    ora = PU.oracle_pairs(pols, docs, SELECTOR_NS_LABELS)
    st, res = PU.compare(pols, docs, SELECTOR_NS_LABELS, backend=backend, **kw)
    assert st["nbad"] == 0, (variant, st["bad"])
    rule_index = {r["name"]: k for k, r in enumerate(res.ruleset.rules)}
    for i, (cid, where, _, _, outcomes, want) in enumerate(SELECTOR_CASES):
        # the orders on which the rule has a response
        if where == "match":
            responds = {o == "match" for o in outcomes}
        elif where == "exclude":
            responds = {o != "match" for o in outcomes}
        else:
            responds = {False}
        row = ora.get(("sel", "c%d" % i, i))
        # the oracle: a response exactly when some order has one, flagged exactly when the orders disagree
        assert (row is not None) == (True in responds), (variant, cid, row)
        if row is not None:
            assert bool(row.get("nondeterministic")) == (len(responds) > 1), (variant, cid, row)
            if len(responds) == 1:
                assert row["status"] == "pass", (variant, cid, row)
        got = K.STATUS_NAMES[int(res.status[rule_index["c%d" % i], i])]
        assert got == want, (variant, cid, got, want)
        if want != "fallback":
            assert (want == "nondeterministic") == (len(responds) > 1), (variant, cid)
    return res


@pytest.mark.parametrize("variant", VARIANTS)
def test_selector_map_order_cases(variant):
    check_selector_cases(variant, "cpu")
