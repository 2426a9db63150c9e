"""`{{ request.object.<field chain> }}` variables as leaves of validate.pattern / anyPattern, on the CPU backend
(policies, corpus and checker: pattern_vars_cases.py; the MI355X side: test_gpu_pattern_vars.py).

The rules compile (L_DYN leaves resolved once per pair) instead of going to the CPU engine with reason "variables";
every pair of about 600 documents must equal the oracle on the substituted policy; each unsupported form keeps its
own compile-time reason; the generated source covers every rule and compiles for gfx950 without a GPU."""
import copy
import re

import numpy as np
import pytest

import cases
import pattern_vars_cases as M
from kyverno_amd import _lib as K
from kyverno_amd import engine as E

N = 600


def test_policies_compile_without_fallback():
    rs = E.Ruleset(M.policies())
    assert len(rs.rules) == 14
    for r in rs.rules:
        assert r["kind"] in ("pattern", "anyPattern") and r["reason"] == "", r


def test_corpus_is_not_vacuous():
    """the oracle decides every pair of the substituted policies (none unsupported, none nondeterministic); every case
    tag is on the corpus, and any 64 consecutive documents hold several of them"""
    docs, tags = M.corpus(N)
    assert {"string", "int", "float", "bool", "null", "parent-null", "parent-nonmap", "missing", "missing2", "nonplain",
            "composite", "deploy"} == set(tags)
    for w in range(0, N - 63, 64):
        assert len(set(tags[w:w + 64])) >= 6
    two = 0
    for (rr, errs), tag in zip(M.expected(N), tags):
        for key, o in rr.items():
            assert o["status"] != "unsupported" and not o.get("nondeterministic"), (key, o)
        two += len(errs[("pv-two", "two")]) == 2
    assert two > 0  # the rule with two variables meets documents where both keys are missing
    assert not any("{{" in s or "$(" in s for s in _strings(docs))


def _strings(v):
    if isinstance(v, str):
        yield v
    elif isinstance(v, dict):
        for k, x in v.items():
            yield k
            yield from _strings(x)
    elif isinstance(v, list):
        for x in v:
            yield from _strings(x)


def test_cpu_backend_parity():
    rs, res = M.evaluate(N, "cpu")
    st = M.check(res, rs, N)
    M.check_counts(st, rs)
    assert st["compared"] > 4000 and st["messages"] > 4000, st
    assert st["errors"] > 100 and st["error_messages"] > 100, st
    assert st["fallback"] > 0  # nonplain / composite values: handed over with the new reason, nowhere else


@pytest.mark.parametrize("form", range(len(M.unsupported_forms())))
def test_unsupported_forms_keep_their_own_reason(form):
    validate, reason = M.unsupported_forms()[form]
    pol = M._pol("pv-unsupported", [M._rule("u", copy.deepcopy(validate))])
    rs = E.Ruleset([pol])
    assert [(r["kind"], r["reason"]) for r in rs.rules] == [("fallback", reason)]


def test_generated_source_covers_every_rule_and_compiles(monkeypatch):
    """jit_source() counts every pattern and anyPattern rule (none is left to the interpreted walk); each rule's root
    function resolves its variables before the walker state exists; two patterns that differ only in the variable
    they name are two shapes; the source compiles for gfx950 (hipRTC, no GPU needed)"""
    rs = E.Ruleset(M.policies())
    src, n = rs.jit_source()
    assert n == sum(r["kind"] in ("pattern", "anyPattern") for r in rs.rules) == 14
    assert "leaf_match_dyn(w.v, w.dyn[0], x, &fb)" in src and "leaf_match_dyn(w.v, w.dyn[1], x, &fb)" in src
    assert src.count("// cold: no entry") >= 14 and "ST_ERROR | ST_MARK_VAR" in src
    rs2 = E.Ruleset([p for p in M.policies() if p["metadata"]["name"] == "pv-shape"])
    src2, n2 = rs2.jit_source()
    assert n2 == 2 and len(re.findall(r"void root\d+\(", src2)) == 2  # one root function each: not one shape
    monkeypatch.setenv("KYV_JIT_CACHE", "0")  # compile for real; keep the in-tree code-object cache untouched
    secs, size = rs2.jit_compile()
    assert size > 1000
    rs3 = E.Ruleset([p for p in M.policies() if p["metadata"]["name"] in ("pv-any", "pv-containers", "pv-quoted")])
    assert rs3.jit_compile()[1] > 1000 and rs3.jit_compile(accounting=True)[1] > 1000


def test_source_without_variables_names_none():
    """a ruleset without pattern variables (synth's C3 policies): nothing of the variables' code is generated"""
    src, _ = E.Ruleset(cases.best_practices() + cases.chart_restricted()).jit_source()
    for word in ("w.dyn", "dq[", "dv[", "jdyn_value", "dyn_walk_value", "ST_MARK_VAR", "// variables"):
        assert word not in src, word


def _autogen_pols():
    def pol(name, rules, ann=None):
        return {"apiVersion": "kyverno.io/v1", "kind": "ClusterPolicy", "metadata": dict({"name": name}, **({"annotations": ann} if ann else {})),
                "spec": {"validationFailureAction": "Audit", "background": True, "rules": rules}}
    var = {"spec": {"serviceAccountName": "{{request.object.spec.nodeName}}"}}
    auto = pol("pv-autogen", [{"name": "sa", "match": {"any": [{"resources": {"kinds": ["Pod"]}}]}, "validate": {"pattern": var}}])
    none = {"pod-policies.kyverno.io/autogen-controllers": "none"}
    t = "{{request.object.spec.template.spec.nodeName}}"
    j = "{{request.object.spec.jobTemplate.spec.template.spec.nodeName}}"
    explicit = pol("pv-explicit", [
        {"name": "sa", "match": {"any": [{"resources": {"kinds": ["Pod"]}}]}, "validate": {"pattern": var}},
        {"name": "autogen-sa", "match": {"any": [{"resources": {"kinds": ["Deployment"]}}]}, "validate": {"pattern": {"spec": {"template": {
            "spec": {"serviceAccountName": t}}}}}},
        {"name": "autogen-cronjob-sa", "match": {"any": [{"resources": {"kinds": ["CronJob"]}}]}, "validate": {"pattern": {"spec": {"jobTemplate": {
            "spec": {"template": {"spec": {"serviceAccountName": j}}}}}}}},
    ], ann=none)
    return auto, explicit


def test_autogen_rewrites_the_variables():
    """device-only (the oracle does not take these rules): a Pod policy with default autogen gives, on Deployments and
    CronJobs, the statuses of the explicitly written spec.template... / spec.jobTemplate... rules"""
    auto, explicit = _autogen_pols()
    docs = []
    for i in range(90):
        tm = {"metadata": {"labels": {"a": "b"}},
              "spec": {"serviceAccountName": "sa-%d" % (i % 2), "nodeName": "sa-%d" % (i // 3 % 3), "containers": [{"name": "c", "image": "i"}]}}
        if i // 3 % 7 == 3:
            del tm["spec"]["nodeName"]  # the variable's key is missing: a substitution error
        meta = {"name": "n%d" % i, "namespace": "ns"}
        docs.append([{"apiVersion": "v1", "kind": "Pod", "metadata": meta, "spec": tm["spec"]},
                     {"apiVersion": "apps/v1", "kind": "Deployment", "metadata": meta, "spec": {"template": tm}},
                     {"apiVersion": "batch/v1", "kind": "CronJob", "metadata": meta,
                      "spec": {"schedule": "* * * * *", "jobTemplate": {"spec": {"template": tm}}}}][i % 3])
    out = []
    for p in (auto, explicit):
        rs = E.Ruleset([p])
        assert [r["kind"] for r in rs.rules] == ["pattern"] * 3 and [r["name"] for r in rs.rules] == ["sa", "autogen-sa", "autogen-cronjob-sa"]
        out.append(np.asarray(E.evaluate(rs, E.Batch(rs, docs), backend="cpu").status))
    assert np.array_equal(out[0], out[1])
    for k in range(3):
        assert {K.ST_PASS, K.ST_FAIL, K.ST_ERROR} <= set(out[0][k].tolist()), (k, out[0][k])
