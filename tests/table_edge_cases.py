"""Generators for the table-edge parity tests (test_table_edges.py on the CPU, test_gpu_table_edges.py on the GPU):
rulesets and batches that push the device code past the capacities its other tests stay inside -- the 128 glob-mask
bits (1 to 4 mask words per dictionary string, then byte matching), the lane tail-fact tables of the match records, and
rule slices cut through the compiled C3 kernels. Each test proves its regime from the evaluation's plan report
(Results.plan()).
"""
import functools
import random

import cases
from kyverno_amd import synth

NOAUTOGEN = {"pod-policies.kyverno.io/autogen-controllers": "none"}


def policy(name, rules):
    return {"apiVersion": "kyverno.io/v1", "kind": "ClusterPolicy", "metadata": {"name": name, "annotations": NOAUTOGEN},
            "spec": {"validationFailureAction": "Audit", "background": True, "rules": rules}}


# ---------------------------------------------------------------- 3a: wildcard semantics at every mask position
def go_match(pattern, name):
    """go-wildcard v1.0.3 Match (github.com/IGLOU-EU/go-wildcard, wildcard.go), restated plainly: an empty pattern
    matches only the empty name, "*" matches everything, otherwise deepMatchRune over the two rune slices -- '*' takes
    any run of runes (tried shortest first), '?' exactly one rune, every other rune itself. Python strings index by
    code point, as []rune does."""
    if pattern == "":
        return name == pattern
    if pattern == "*":
        return True

    @functools.lru_cache(maxsize=None)
    def deep(si, pi):
        while pi < len(pattern):
            ch = pattern[pi]
            if ch == "*":
                return deep(si, pi + 1) or (si < len(name) and deep(si + 1, pi))
            if ch == "?":
                if si >= len(name):
                    return False
            elif si >= len(name) or name[si] != ch:
                return False
            si += 1
            pi += 1
        return si == len(name)

    return deep(0, 0)


ADVERSARIAL_PATTERNS = ["a*a*a*b", "*?*", "??", "?*?", "**", "x**y", "*a*", "é?", "?é*", "é*é", "*日本*", "�*z",
                        "?", "*?", "a*b", "*aab", "日?語", "x?y"]
ADVERSARIAL_TEXTS = ["", "q", "a" * 20, "a" * 19 + "b", "é", "éé", "日本語", "x*y", "x?y", "k�z", "�z"]
LADDER = (0, 30, 62, 94, 126)  # padding globs in front of the vector globs: they straddle mask bits 32, 64, 96, 128
# the characters of the pattern-leaf mini-language (operators, ranges, alternatives): globs with one are no leaf vectors
LEAF_OPERATOR_CHARS = set("|&!<>=-")


@functools.lru_cache(maxsize=None)
def wildcard_vectors():
    """(patterns, texts): the distinct non-empty patterns and the distinct texts of tests/golden/wildcard.json, then
    the adversarial ones"""
    recs = cases.load("wildcard.json")
    pats, texts = [], []
    for r in recs:
        if r["pattern"] and r["pattern"] not in pats:
            pats.append(r["pattern"])
        if r["text"] not in texts:
            texts.append(r["text"])
    for p in ADVERSARIAL_PATTERNS:
        if p not in pats:
            pats.append(p)
    for t in ADVERSARIAL_TEXTS:
        if t not in texts:
            texts.append(t)
    return tuple(pats), tuple(texts)


def vector_rungs():
    """[(rung id, padding globs, vector patterns, vector patterns of the condition routes)]: the whole pattern set
    behind each padding of LADDER (2 to 4 mask words, the last two rungs past the 128 bits), and its two halves without
    padding (one mask word; the condition routes spend a second bit per pattern on its literal set, so they take
    every second pattern of the half)"""
    pats, _ = wildcard_vectors()
    half = len(pats) // 2
    return [("half0", 0, pats[:half], pats[:half][::2]), ("half1", 0, pats[half:], pats[half:][::2])] + \
        [("pad%d" % off, off, pats, pats) for off in LADDER]


# mask words per dictionary string each rung runs in: (match routes' ruleset, pattern-leaf / condition routes' ruleset)
RUNG_WORDS = {"half0": (1, 1), "half1": (1, 1), "pad0": (2, 3), "pad30": (3, 4), "pad62": (4, 4), "pad94": (4, 4),
              "pad126": (4, 4)}


def _padding_rule(offset):
    """`offset` prefix globs as pattern leaves of one rule no resource of the batches is gated into: pattern atoms are
    the first literals to get mask bits, so the vector globs of every route start at bit `offset`. One anyPattern
    alternative per glob keeps the rule out of the runtime-compiled kernels (a single pattern map with 126 entries
    takes hipRTC minutes)."""
    return {"name": "padding", "match": {"any": [{"resources": {"kinds": ["Secret"]}}]},
            "validate": {"anyPattern": [{"data": {"pad": "pad-%d-*" % i}} for i in range(offset)]}}


def _cm_rule(name, resources, validate=None):
    res = dict(resources)
    res["kinds"] = ["ConfigMap"]
    return {"name": name, "match": {"any": [{"resources": res}]}, "validate": validate or {"pattern": {}}}


FIXED_KEY = "vectors.example.com/text"


def match_route_policies(offset, pats):
    """routes (i), (ii), (iv): rule <route>-<g> uses vector glob g as a name (names: [glob]), a namespace
    (namespaces: [glob]), an annotation value under a fixed key and an annotation key with value "*" """
    rules = [_padding_rule(offset)] if offset else []
    for g, p in enumerate(pats):
        rules.append(_cm_rule("name-%d" % g, {"names": [p]}))
        rules.append(_cm_rule("ns-%d" % g, {"namespaces": [p]}))
        rules.append(_cm_rule("annv-%d" % g, {"annotations": {FIXED_KEY: p}}))
        rules.append(_cm_rule("annk-%d" % g, {"annotations": {p: "*"}}))
    return [policy("vec-match", rules)]


def masked_literals(pats):
    """the patterns that take a glob-mask bit: those with a wildcard character or a non-ASCII byte (the others are
    compared as dictionary ids)"""
    return [p for p in pats if "*" in p or "?" in p or any(ord(c) > 127 for c in p)]


def leaf_patterns(pats):
    return [p for p in pats if not (set(p) & LEAF_OPERATOR_CHARS)]


def eval_route_policies(offset, pats):
    """routes (iii), (v): rule leaf-<g> has the pattern leaf metadata: {name: glob}; eq-<g> / ne-<g> deny when
    {{request.object.metadata.name}} Equals / NotEquals the glob; anyin-<g> / allnotin-<g> deny Pods whose container
    names are AnyIn / AllNotIn a literal set of their own ([glob, a second literal]: one condition set per glob)"""
    rules = [_padding_rule(offset)] if offset else []
    for g, p in enumerate(pats):
        if not (set(p) & LEAF_OPERATOR_CHARS):
            rules.append(_cm_rule("leaf-%d" % g, {}, {"message": "leaf %d" % g, "pattern": {"metadata": {"name": p}}}))
        for nm, op in (("eq", "Equals"), ("ne", "NotEquals")):
            rules.append(_cm_rule("%s-%d" % (nm, g), {}, {"message": "%s %d" % (nm, g), "deny": {"conditions": {"any": [
                {"key": "{{request.object.metadata.name}}", "operator": op, "value": p}]}}}))
        for nm, op in (("anyin", "AnyIn"), ("allnotin", "AllNotIn")):
            rules.append({"name": "%s-%d" % (nm, g), "match": {"any": [{"resources": {"kinds": ["Pod"]}}]},
                          "validate": {"message": "%s %d" % (nm, g), "deny": {"conditions": {"any": [
                              {"key": "{{request.object.spec.containers[].name}}", "operator": op,
                               "value": [p, "never-%d" % g]}]}}}})
    return [policy("vec-eval", rules)]


@functools.lru_cache(maxsize=None)
def vector_resources():
    """one ConfigMap per text (its name; another text as its namespace, a third under the fixed annotation key, a fourth
    as an annotation key) and a few Pods whose container names are runs of the texts"""
    _, texts = wildcard_vectors()
    n = len(texts)
    docs = []
    for i, t in enumerate(texts):
        docs.append({"apiVersion": "v1", "kind": "ConfigMap",
                     "metadata": {"name": t, "namespace": texts[(i * 7 + 3) % n],
                                  "annotations": {FIXED_KEY: texts[(i * 5 + 1) % n], texts[(i * 3 + 2) % n]: "v%d" % i}},
                     "data": {"k": "v"}})
    for j in range(6):
        names = [texts[(j * 9 + q * 4) % n] for q in range(1 + j % 4)]
        docs.append({"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "pod-%d" % j, "namespace": "default"},
                     "spec": {"containers": [{"name": nm, "image": "img:1"} for nm in names]}})
    return docs


# ---------------------------------------------------------------- 3b: match tables past their capacities
# Vocabulary sizes of the three cases against the tables' capacities (kyv_kernels.h): 8 selector keys, 4 namespace-
# selector keys, 16 wildcard requirements, 32 annotation pairs, 16 group / version atoms; 32 glob literals keep the
# tail facts on mask word 0 (onemask).
VOCAB = {
    #            name / namespace globs, selector keys, ns keys, wildcard key globs x values, annotation pairs, gv forms
    "within": dict(names=4, nss=3, keys=6, nskeys=3, wkeys=2, wvals=4, ann=10, gvs=9),
    "between": dict(names=8, nss=6, keys=10, nskeys=3, wkeys=4, wvals=6, ann=24, gvs=21),
    "over": dict(names=12, nss=8, keys=10, nskeys=6, wkeys=4, wvals=14, ann=60, gvs=48),
}
NAME_GLOBS = ["pod-*", "*-00001*", "deployment-??0*", "pod-000?1*", "configmap-*", "*-0000?2?", "job-*", "service-0*",
              "cronjob-*", "*set-*", "pod-00?0*", "*-000010?"]
NS_GLOBS = ["ns-?0*", "ns-00*", "ns-01??", "ns-*1", "team-*", "ns-0?5*", "ns-*7", "ns-09*"]
SEL_KEYS = ["app", "tier", "owner", "app.kubernetes.io/name", "label-0", "label-1", "label-2", "label-3", "label-4", "zone"]
NS_KEYS = ["env", "tier", "team", "kubernetes.io/metadata.name", "region", "stage"]
WILD_KEYS = ["label-*", "app*", "t?er", "own*"]
WILD_VALS = ["*", "v?", "v1", "fr*", "back?nd", "data", "team-1*", "app-2*", "?*", "v[0-9]", "team-*", "app-?", "*end", "v*"]
GV_KINDS = [("apps", "Deployment"), ("apps", "StatefulSet"), ("apps", "DaemonSet"), ("apps", "ReplicaSet"),
            ("batch", "Job"), ("batch", "CronJob")]
PATTERNS = [{"metadata": {"labels": {"owner": "?*"}}}, {"metadata": {"labels": {"app": "app-*"}}},
            {"metadata": {"name": "!*-x"}}, {"metadata": {"=(annotations)": {"=(example.com/a0)": "value-?*"}}},
            {"metadata": {"labels": {"tier": "frontend | backend"}}}]


def _gv_forms(n):
    """n kinds entries with a group / version refinement -- <group>/<version>/<Kind>, <group>/*/<Kind>, v1/<Kind>,
    */<Kind> -- ordered so that every few forms add a distinct (group, version) atom"""
    forms = ["v1/Pod", "*/Pod", "v1/ConfigMap"]
    for ver in ("v1", "*", "v1beta1", "v2", "v1alpha1"):
        for grp, kind in GV_KINDS + [("extensions", "Deployment"), ("policy", "Job"), ("autoscaling", "StatefulSet")]:
            forms.append("%s/%s/%s" % (grp, ver, kind))
    return forms[:n]


def table_policies(case, n=600, seed=31):
    """C4-style generated policies (one validate rule each) over the vocabulary VOCAB[case]"""
    V = VOCAB[case]
    r = random.Random(seed)
    names, nss = NAME_GLOBS[:V["names"]], NS_GLOBS[:V["nss"]]
    keys, nskeys = SEL_KEYS[:V["keys"]], NS_KEYS[:V["nskeys"]]
    wkeys, wvals = WILD_KEYS[:V["wkeys"]], WILD_VALS[:V["wvals"]]
    gvs = _gv_forms(V["gvs"])
    plain_kinds = [["Pod"], ["Deployment"], ["ConfigMap"], ["Pod", "Service"], ["Job", "CronJob"], ["*"], ["StatefulSet"]]
    # annotation (key glob, value glob) pairs over the corpus' example.com/a<k>: value-<n> annotations
    ann = []
    for k in range(6):
        for d in range(10):
            ann.append(("example.com/a%d" % k, "value-%d*" % d))
    ann = ann[:V["ann"]]

    def selector():
        u = r.random()
        if u < 0.35:  # one wildcard matchLabels entry (more would be a FALLBACK rule), sometimes beside expressions
            sel = {"matchLabels": {r.choice(wkeys): r.choice(wvals)}}
            if r.random() < 0.4:
                sel["matchExpressions"] = [{"key": r.choice(keys), "operator": r.choice(["Exists", "DoesNotExist"])}]
            return sel
        if u < 0.6:
            return {"matchLabels": {r.choice(keys): r.choice(["frontend", "backend", "v1", "v2", "app-7"])}}
        return {"matchExpressions": [{"key": r.choice(keys), "operator": r.choice(["In", "NotIn"]),
                                      "values": ["app-%d" % r.randint(0, 300), "v%d" % r.randint(0, 9), "frontend"]},
                                     {"key": r.choice(keys), "operator": r.choice(["Exists", "DoesNotExist"])}]}

    def filt(light=False):
        res = {"kinds": list(r.choice(plain_kinds)) if r.random() < 0.55 else r.sample(gvs, r.randint(1, min(3, len(gvs))))}
        u = r.random()
        if u < 0.3:
            res["names"] = r.sample(names, r.randint(1, min(3, len(names))))
        elif u < 0.4:
            res["name"] = r.choice(names)
        if r.random() < 0.35:
            res["namespaces"] = r.sample(nss, r.randint(1, min(3, len(nss))))
        if light:
            return res
        v = r.random()
        if v < 0.4:
            res["selector"] = selector()
        elif v < 0.55:
            res["namespaceSelector"] = {"matchLabels": {r.choice(nskeys): r.choice(["prod", "dev", "frontend", "team-3"])}}
        elif v < 0.6:  # a wildcard in a namespace selector: a tail the facts never cover
            res["namespaceSelector"] = {"matchLabels": {"t?er": "*"}}
        if r.random() < 0.25:
            k, val = r.choice(ann)
            res["annotations"] = {k: val}
        return res

    out = []
    for i in range(n):
        match = {"any": [{"resources": filt()}]}
        for _ in range(r.choice([0, 0, 0, 1, 1, 2, 3])):
            match["any"].append({"resources": filt(light=r.random() < 0.5)})
        rule = {"name": "t%04d" % i, "match": match,
                "validate": {"message": "generated rule %d" % i, "pattern": r.choice(PATTERNS)}}
        w = r.random()
        if w < 0.2:
            rule["exclude"] = {"any": [{"resources": {"namespaces": [r.choice(nss)]}}]}
        elif w < 0.3:
            k, val = r.choice(ann)
            rule["exclude"] = {"any": [{"resources": {"annotations": {k: val}}}]}
        elif w < 0.35:
            rule["exclude"] = {"any": [{"resources": {"selector": selector()}}]}
        out.append(policy("tab-%04d" % i, [rule]))
    return out


@functools.lru_cache(maxsize=None)
def table_corpus():
    """the shared batch of the 3b cases: synth.mixed(1500, edge=True), whose kind boundaries fall inside waves"""
    return synth.mixed(1500, seed=5, edge=True)


@functools.lru_cache(maxsize=None)
def table_corpus_small():
    """130 resources: two full waves and a partial one"""
    docs, nsl = synth.mixed(130, seed=11, edge=True)
    return docs, nsl


# ---------------------------------------------------------------- 3c: rule slices through the compiled C3 kernels
def slice_policies():
    """exactly the ruleset whose code object the other C3 tests cache"""
    return cases.best_practices() + cases.chart_restricted()


@functools.lru_cache(maxsize=None)
def slice_corpus():
    """226 match waves (14,401 resources, the last wave holds one): at this size one pattern rule's slice buffers pass
    1 MiB, so KYV_SLICE_MB=1 leaves every walk rule alone in its slice"""
    return synth.mixed(14_401, seed=23, edge=True)


def compiled_rulesets():
    """every new ruleset the GPU tests evaluate with runtime-compiled kernels (the driver's build step compiles them
    ahead of time into the code-object cache; slice_policies() is compiled there already)"""
    out = []
    for _, offset, pats, epats in vector_rungs():
        out += [match_route_policies(offset, pats), eval_route_policies(offset, epats)]
    return out + [table_policies(case) for case in VOCAB]
