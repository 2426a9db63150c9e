"""Policies, corpus and checker of the pattern-variable tests (test_pattern_vars.py on the CPU backend,
test_gpu_pattern_vars.py on the MI355X): validate.pattern / anyPattern rules whose leaves are
`{{ request.object.<field chain> }}` variables.

oracle/ answers `unsupported` for such rules, so the checker is the oracle on the SUBSTITUTED policy: substitute()
replaces every variable leaf by the resource's typed JSON value, as substitutePatterns does before the walk
(pkg/engine/validation.go:760-782, variables/vars.go:352-431; JSON-context numbers are float64) --
  a key missing from a map is an error; a field of null or of a non-map is null; a present null is null --
and O.validate runs on the result, once per resource.

Every policy carries `pod-policies.kyverno.io/autogen-controllers: none`, so the paths the helper reads are the paths
the engine reads."""
import copy
import functools
import json
import re

from kyverno_amd import _lib as K
from kyverno_amd import engine as E
from oracle import oracle as O

VAR = re.compile(r'^\{\{\s*request\.object((?:\.(?:[A-Za-z_][A-Za-z0-9_]*|"[^"\\]+"))+)\s*\}\}$')
SEG = re.compile(r'\.(?:([A-Za-z_][A-Za-z0-9_]*)|"([^"\\]+)")')
FALLBACK_REASON = "pattern variable's value outside the device subset (a map, an array, or a string with pattern syntax)"


# ---------------------------------------------------------------- policies
def _pol(name, rules):
    return {"apiVersion": "kyverno.io/v1", "kind": "ClusterPolicy",
            "metadata": {"name": name, "annotations": {"pod-policies.kyverno.io/autogen-controllers": "none"}},
            "spec": {"validationFailureAction": "Audit", "background": True, "rules": rules}}


def _rule(name, validate, kinds=("Pod",), message="pattern variable check", **extra):
    res = {"kinds": list(kinds)}
    res.update(extra.pop("resources", {}))
    r = {"name": name, "match": {"any": [{"resources": res}]}, "validate": dict({"message": message}, **validate)}
    r.update(extra)
    return r


V = "{{request.object.spec.vars.v}}"
W = "{{ request.object.spec.vars.w }}"
NAME = "{{request.object.metadata.name}}"
NS = "{{ request.object.metadata.namespace }}"
QUOTED = '{{request.object.metadata.labels."app.kubernetes.io/name"}}'


def policies(shape_names=False):
    """the policy families of the tests. shape_names: the two rules that differ only in their variable get a `names`
    filter, which takes them off the kind-gate path and onto the pattern-shape tables"""
    shape_res = {"resources": {"names": ["pv-*"]}} if shape_names else {}
    return [
        # a label must equal metadata.name; spec.serviceAccountName must equal the namespace
        _pol("pv-label-name", [_rule("label-is-name", {"pattern": {"metadata": {"labels": {"app": NAME}}}})]),
        _pol("pv-sa-ns", [_rule("sa-is-namespace", {"pattern": {"spec": {"serviceAccountName": NS}}})]),
        # the typed matrix: spec.check against the value at spec.vars.v
        _pol("pv-typed", [_rule("check-is-v", {"pattern": {"spec": {"check": V}}})]),
        # a variable under an =() anchor and under a () anchor
        _pol("pv-eq-anchor", [_rule("eq", {"pattern": {"spec": {"=(check2)": V}}})]),
        _pol("pv-cond-anchor", [_rule("cond", {"pattern": {"spec": {"(check)": V, "serviceAccountName": "?*"}}})]),
        # an element of a scalar array pattern; one variable used under an array of maps
        _pol("pv-array", [_rule("list", {"pattern": {"spec": {"list": [V]}}})]),
        _pol("pv-containers", [_rule("tags", {"pattern": {"spec": {"containers": [{"tag": V}]}}})]),
        # a quoted segment, below a pattern key that holds a '/'
        _pol("pv-quoted", [_rule("quoted", {"pattern": {"metadata": {"annotations": {"example.com/name": QUOTED}}}})]),
        # anyPattern with a variable in each of two alternatives
        _pol("pv-any", [_rule("any", {"anyPattern": [{"spec": {"check": V}}, {"spec": {"serviceAccountName": NS}}]})]),
        # a precondition that is false on part of the corpus (spec.tierclass is on every document)
        _pol("pv-pre", [_rule("pre", {"pattern": {"spec": {"check": V}}}, preconditions={"all": [
            {"key": "{{request.object.spec.tierclass}}", "operator": "Equals", "value": "gold"}]})]),
        # two rules that differ only in the variable they name; a rule with two variables
        _pol("pv-shape", [_rule("shape-v", {"pattern": {"spec": {"check": V}}}, **copy.deepcopy(shape_res)),
                          _rule("shape-w", {"pattern": {"spec": {"check": W}}}, **copy.deepcopy(shape_res))]),
        _pol("pv-two", [_rule("two", {"pattern": {"spec": {"check": V, "check3": W}}})]),
        # a Deployment rule that reads spec.template...
        _pol("pv-deploy", [_rule("template-sa", {"pattern": {"spec": {"template": {"spec": {
            "serviceAccountName": "{{request.object.spec.template.metadata.labels.sa}}"}}}}}, kinds=("Deployment",))]),
    ]


# rules a document can make skip: a conditional anchor, a precondition (a plain pattern without either has no input
# that makes it skip)
CAN_SKIP = {"cond", "pre"}


def unsupported_forms():
    """(pattern or anyPattern validate block, the compile-time fallback reason it must get)"""
    many = {"spec": {"f%d" % i: "{{request.object.spec.v%d}}" % i for i in range(5)}}
    return [
        ({"pattern": {"spec": {"{{request.object.metadata.name}}": "x"}}}, "variables: in a pattern key"),
        ({"pattern": {"spec": {"check": "prefix-{{request.object.metadata.name}}"}}}, "variables: embedded in a longer string"),
        ({"pattern": {"spec": {"check": "{{request.object.a}}{{request.object.b}}"}}}, "variables: embedded in a longer string"),
        ({"pattern": {"spec": {"check": "{{@}}"}}}, "variables: other than a request.object field chain"),
        ({"pattern": {"spec": {"check": "{{request.operation}}"}}}, "variables: other than a request.object field chain"),
        ({"pattern": {"spec": {"check": "{{serviceAccountName}}"}}}, "variables: other than a request.object field chain"),
        ({"pattern": {"spec": {"check": "{{request.object.spec.containers[0].name}}"}}},
         "variables: other than a request.object field chain"),
        ({"anyPattern": [{"spec": {"check": "ok"}}, {"spec": {"check": "{{ length(request.object.spec.containers) }}"}}]},
         "variables: other than a request.object field chain"),
        ({"pattern": {"spec": {"check": "{{request.object}}"}}}, "variables: bare request.object"),
        ({"pattern": many}, "variables: more distinct variables than the device resolves per rule"),
    ]


# ---------------------------------------------------------------- corpus
# (tag, spec.vars, spec.check): the value the variable resolves to and the tested field
_STR = [("web", "web"), ("web", "api"), ("web", True), ("true", True), ("false", False), ("", None), ("", "")]
_NUM = [(7, 7), (7, 8), (7, "7"), (7, 7.0), (-3, -3), (2 ** 40 + 1, 2 ** 40 + 1), (2 ** 40 + 1, 2 ** 40), (9007199254740991, 9007199254740991),
        (0, None), (0, 0), (0, False), (2.5, 2.5), (2.5, "2.5"), (2.5, 2), (1e3, 1000), (-0.75, -0.75), (-0.75, "x")]
_BOOL = [(True, True), (True, False), (True, "true"), (False, False), (False, None), (False, 0)]
_NULL = [(None, None), (None, ""), (None, 0), (None, False), (None, "x"), (None, 0.0)]
_NONPLAIN = ["a*", ">1", "1Gi", " web", "caf\u00e9", "a|b", "web?"]
_COMPOSITE = [{"k": "v"}, ["web"], {}, []]


def _cases():
    out = []
    for v, c in _STR:
        out.append(("string", {"v": v, "w": "web"}, c))
    for v, c in _NUM:
        out.append(("float" if isinstance(v, float) else "int", {"v": v, "w": "web"}, c))
    for v, c in _BOOL:
        out.append(("bool", {"v": v, "w": "api"}, c))
    for v, c in _NULL:
        out.append(("null", {"v": v, "w": "web"}, c))
    out.append(("parent-null", None, None))
    out.append(("parent-null", None, "web"))
    for p in ("text", 5, ["v"], True):
        out.append(("parent-nonmap", p, None))
        out.append(("parent-nonmap", p, "web"))
    out.append(("missing", {"w": "web"}, "web"))     # one key missing: v
    out.append(("missing", {"v": "web"}, "web"))     # one key missing: w
    out.append(("missing2", {}, "web"))              # two keys missing in the rule with two variables
    for s in _NONPLAIN:
        out.append(("nonplain", {"v": s, "w": "web"}, s))
        out.append(("nonplain", {"v": s, "w": "web"}, "abc"))
    out.append(("nonplain", {"v": "7", "w": "web"}, 7))  # a digit first: the number / range / quantity forms
    for c in _COMPOSITE:
        out.append(("composite", {"v": c, "w": "web"}, copy.deepcopy(c)))
        out.append(("composite", {"v": c, "w": "web"}, "web"))
    return out


def corpus(n):
    """n documents, each tagged with its case; the cases are interleaved (consecutive documents take consecutive
    cases, and the fields the other rules read vary with coprime periods), so one wave of 64 holds several of them.
    -> (docs, tags)"""
    cases = _cases()
    docs, tags = [], []
    for i in range(n):
        tag, vars_, check = cases[i % len(cases)]
        j = i // len(cases) + i
        if i % 9 == 4:
            docs.append(_deployment(i, j))
            tags.append("deploy")
            continue
        name = "pv-%04d" % i if i % 11 else "other-%04d" % i
        labels = {"app": name if j % 3 else "web", "tier": "t%d" % (j % 2)}
        ann = {"example.com/name": "n%d" % (j % 4)}
        if j % 5:
            labels["app.kubernetes.io/name"] = "n%d" % (j % 3)
        meta = {"name": name, "namespace": "ns-%d" % (j % 3), "labels": labels, "annotations": ann}
        if i % 13 == 6:
            del meta["namespace"]  # {{request.object.metadata.namespace}}: a missing key
        if i % 17 == 8:
            del meta["labels"]     # {{...labels."app.kubernetes.io/name"}}: `labels` missing
        if i % 19 == 9:
            del meta["name"]
            meta["generateName"] = "pv-"
        spec = {"tierclass": "gold" if j % 4 else "iron", "vars": copy.deepcopy(vars_), "check": copy.deepcopy(check),
                "serviceAccountName": "ns-%d" % (j % 2),
                "list": [copy.deepcopy(check)] * (1 + j % 3) if j % 4 else [copy.deepcopy(check), "zzz"],
                "containers": [{"name": "c%d" % q, "image": "img:%d" % q, "tag": copy.deepcopy(check if (q + j) % 3 else "web")}
                               for q in range(1 + j % 3)]}
        if j % 2:
            spec["check2"] = copy.deepcopy(check)
        if j % 3 == 0:
            spec["check3"] = "web"
        if j % 7 == 3:
            del spec["serviceAccountName"]
        docs.append({"apiVersion": "v1", "kind": "Pod", "metadata": meta, "spec": spec})
        tags.append(tag)
    return docs, tags


def _deployment(i, j):
    sa = "sa-%d" % (j % 2)
    tmeta = [{"labels": {"sa": "sa-%d" % (j % 3)}}, {"labels": {"app": "x"}}, None, "text", {"labels": None}, {}][(j // 2) % 6]
    d = {"apiVersion": "apps/v1", "kind": "Deployment", "metadata": {"name": "dep-%04d" % i, "namespace": "ns-0"},
         "spec": {"replicas": 1, "template": {"metadata": copy.deepcopy(tmeta), "spec": {
             "serviceAccountName": sa, "containers": [{"name": "c", "image": "img"}]}}}}
    if j % 5 == 1:
        del d["spec"]["template"]["spec"]["serviceAccountName"]
    return d


# ---------------------------------------------------------------- substitution (the few lines the checker adds)
class Missing(Exception):
    pass


def resolve(resource, segs):
    cur = resource
    for s in segs:
        if not isinstance(cur, dict):  # a field of null or of a non-map is null
            return None
        if s not in cur:               # a key missing from a map is the substitution error
            raise Missing(s)
        cur = cur[s]
    return cur


def floats(v):
    """the JSON context's numbers are float64"""
    if isinstance(v, bool):
        return v
    if isinstance(v, int):
        return float(v)
    if isinstance(v, list):
        return [floats(x) for x in v]
    if isinstance(v, dict):
        return {k: floats(x) for k, x in v.items()}
    return v


def substitute(doc, resource, path, errors):
    """the pattern document with every variable leaf replaced by its value; a leaf whose variable does not resolve is
    set to null and recorded in errors as (variable text, JSON pointer of the leaf, missing key)"""
    if isinstance(doc, str):
        m = VAR.match(doc)
        if not m:
            return doc
        segs = [a or b for a, b in SEG.findall(m.group(1))]
        try:
            return floats(resolve(resource, segs))
        except Missing as e:
            errors.append((doc[2:-2].strip(), path, e.args[0]))
            return None
    if isinstance(doc, list):
        return [substitute(x, resource, "%s/%d" % (path, i), errors) for i, x in enumerate(doc)]
    if isinstance(doc, dict):
        return {k: substitute(x, resource, path + "/" + k.replace("/", "\\/"), errors) for k, x in doc.items()}
    return doc


def substituted(pols, resource):
    """-> (policies with their patterns substituted for this resource, {(policy, rule): errors})"""
    out, errs = copy.deepcopy(pols), {}
    for p in out:
        for r in p["spec"]["rules"]:
            e = []
            for f in ("pattern", "anyPattern"):
                if f in r["validate"]:
                    r["validate"][f] = substitute(r["validate"][f], resource, "", e)
            errs[(p["metadata"]["name"], r["name"])] = e
    return out, errs


def error_text(e):
    var, path, key = e
    return ('variable substitution failed: failed to resolve %s at path %s: JMESPath query failed: Unknown key "%s" in path'
            % (var, path, key))


@functools.lru_cache(maxsize=None)
def expected(n, shape_names=False):
    """per document of corpus(n): ({(policy, rule): oracle rule result on the substituted policy}, {(policy, rule):
    substitution errors}); computed once per size and shared by the tests"""
    docs, _ = corpus(n)
    pols = policies(shape_names)
    out = []
    for d in docs:
        sub, errs = substituted(pols, d)
        rr = {}
        for p in O.validate(sub, json.dumps(d), {}):
            for r in p["rules"]:
                rr[(p["policy"], r["name"])] = r
        out.append((rr, errs))
    return out


def check(res, rs, n, shape_names=False):
    """every pair of an evaluation of corpus(n) against expected(n) -> stats; raises on a mismatch"""
    docs, tags = corpus(n)
    exp = expected(n, shape_names)
    st = res.status
    bad = []
    stats = {"compared": 0, "messages": 0, "fallback": 0, "errors": 0, "error_messages": 0,
             "counts": {r["name"]: [0] * 8 for r in rs.rules}}
    for k, rule in enumerate(rs.rules):
        key = (rs.policies[rule["policy"]]["name"], rule["name"])
        for ri in range(n):
            s = int(st[k, ri])
            stats["counts"][rule["name"]][s] += 1
            rr, errs = exp[ri]
            o, e = rr.get(key), errs[key]
            assert o is None or o["status"] != "unsupported", (key, ri, o)
            where = (key, ri, tags[ri], K.STATUS_NAMES[s])
            if o is None:
                if s != K.ST_NONE:
                    bad.append(("matched by the device only",) + where)
                continue
            if e:
                # a key is missing: the oracle's answer for the pattern with the variable leaves set to null says
                # whether the rule got as far as the substitution. The error text is restatement-level (the form
                # oracle/ocond.cpp restates for conditions); no reference golden pins it.
                if o["message"] == "preconditions not met" or o["message"].startswith("rule skipped due to policy exception"):
                    if s != K.ST_SKIP or res.message(ri, k) != o["message"]:
                        bad.append(("skip before the substitution",) + where)
                    continue
                stats["errors"] += 1
                if s != K.ST_ERROR:
                    bad.append(("substitution error expected",) + where)
                elif len(e) == 1:
                    stats["error_messages"] += 1
                    if res.message(ri, k) != error_text(e[0]):
                        bad.append(("error message",) + where + (res.message(ri, k), error_text(e[0])))
                continue
            if s == K.ST_FALLBACK:
                stats["fallback"] += 1
                if tags[ri] not in ("nonplain", "composite") or res.fallback_reason(ri, k) != FALLBACK_REASON:
                    bad.append(("fallback",) + where + (res.fallback_reason(ri, k),))
                continue
            stats["compared"] += 1
            if K.STATUS_NAMES[s].lower() != o["status"]:
                bad.append(("status",) + where + (o["status"], o["message"][:120]))
                continue
            if s == K.ST_FAIL and rule["kind"] == "pattern" and res.path(ri, k) != o["path"]:
                bad.append(("path",) + where + (res.path(ri, k), o["path"]))
            m = res.message(ri, k)
            if m is not None:
                stats["messages"] += 1
                if m != o["message"] and not o.get("message_unpinned"):
                    bad.append(("message",) + where + (m[:160], o["message"][:160]))
    assert not bad, (len(bad), bad[:12])
    return stats


def check_counts(stats, rs):
    """nonzero PASS, FAIL and ERROR counts for every rule, and SKIP for every rule a document can make skip.

    A deviation from "nonzero PASS, FAIL, SKIP and ERROR counts per policy family": SKIP is asserted only for the rules
    in CAN_SKIP. A pattern rule skips through a conditional or global anchor, or through its preconditions; the other
    families have neither, so no document makes them skip and a nonzero SKIP count there would be a wrong verdict."""
    for r in rs.rules:
        c = stats["counts"][r["name"]]
        assert c[K.ST_PASS] > 0 and c[K.ST_FAIL] > 0 and c[K.ST_ERROR] > 0, (r["name"], c)
        if r["name"] in CAN_SKIP:
            assert c[K.ST_SKIP] > 0, (r["name"], c)


def evaluate(n, backend, jit=None, shape_names=False):
    docs, _ = corpus(n)
    rs = E.Ruleset(policies(shape_names))
    b = E.Batch(rs, docs, None)
    res = E.evaluate(rs, b, backend=backend, **({} if backend != "gpu" else {"jit": jit}))
    return rs, res


def compiled_rulesets():
    """the rulesets whose compiled kernels the GPU tests load (built ahead of time by the project's build step)"""
    return [policies(False), policies(True)]
