"""Corpus, rulesets and the Python model of the meta-key plane tests (test_meta_keys.py, test_gpu_meta_keys.py).

A wildcard key of a pattern's metadata.labels / metadata.annotations ("container.apparmor.../*") is resolved per
resource by ExpandInMetadata (wildcards.go:62-83). The compiled walk reads the resolution from a per-batch plane
(Batch.meta_keys); model_row() below restates it over the plain documents, with a literal glob matcher."""
import copy
import functools

import cases

APPARMOR = "container.apparmor.security.beta.kubernetes.io/"
OWNER = "owner.example.com/"
# status overrides of a plane row (include/kyvgpu.h KYV_ST_*)
ST_NONE, ST_FALLBACK, ST_PANIC, ST_ND = 0, 5, 6, 7
POS_PATH = {0: (), 1: ("spec", "template"), 2: ("spec", "jobTemplate", "spec", "template")}


def glob(p, s):
    """wildcard.Match for literal patterns: '*' any run, '?' one character"""
    if not p:
        return not s
    if p[0] == "*":
        return any(glob(p[1:], s[i:]) for i in range(len(s) + 1))
    return bool(s) and (p[0] == "?" or p[0] == s[0]) and glob(p[1:], s[1:])


def _pol(name, rules):
    return {"apiVersion": "kyverno.io/v1", "kind": "ClusterPolicy", "metadata": {"name": name},
            "spec": {"validationFailureAction": "audit", "background": True, "rules": rules}}


def apparmor():
    """the C3 app-armor policy; autogen adds the two pod-template positions"""
    return [p for p in cases.chart_restricted() if p["metadata"]["name"] == "restrict-apparmor-profiles"]


def two_slot():
    """one label wildcard under a conditional anchor and one annotation wildcard: two key slots, SKIP verdicts"""
    return [_pol("mk-two-slot", [{"name": "team-owner", "match": {"any": [{"resources": {"kinds": ["Pod"]}}]},
                                 "validate": {"message": "core teams name an ops owner", "pattern": {"metadata": {
                                     "labels": {"(team-*)": "core"}, "annotations": {OWNER + "*": "ops-?*"}}}}}])]


def no_class():
    """wildcard sites without a class: below an array element (the compiler leaves such a rule to the CPU engine) and
    at a map position that is none of the three static ones (compiled, keeps expand_meta)"""
    return [_pol("mk-no-class", [
        {"name": "claim-annotation", "match": {"any": [{"resources": {"kinds": ["StatefulSet"]}}]},
         "validate": {"message": "claims", "pattern": {"spec": {"=(volumeClaimTemplates)": [
             {"=(metadata)": {"=(annotations)": {"=(" + APPARMOR + "*)": "runtime/default | localhost/*"}}}]}}}},
        {"name": "job-annotation", "match": {"any": [{"resources": {"kinds": ["CronJob"]}}]},
         "validate": {"message": "jobs", "pattern": {"spec": {"jobTemplate": {
             "=(metadata)": {"=(annotations)": {"=(" + APPARMOR + "*)": "runtime/default | localhost/*"}}}}}}}])]


def indirect():
    """a match the kind gate does not decide (namespaces): the rule is walked from match records, not fused"""
    return [_pol("mk-indirect", [{"name": "prod-armor", "match": {"any": [{"resources": {
        "kinds": ["Pod"], "namespaces": ["prod-*"]}}]}, "validate": {"message": "prod", "pattern": {
            "=(metadata)": {"=(annotations)": {"=(" + APPARMOR + "?*)": "runtime/default | localhost/*"}}}}}])]


SAME_SHAPE_GLOBS = {"in-a": "a.example.com/*", "in-b": "b.example.com/*"}


def same_shape():
    """two rules of one kind whose patterns differ in the glob alone: one pattern shape (the generated functions of
    the two are the same text but for the class), two meta-key classes per position"""
    return [_pol("mk-same-shape", [{"name": n, "match": {"any": [{"resources": {"kinds": ["Pod"]}}]},
                                   "validate": {"message": n, "pattern": {"metadata": {"annotations": {g: "x"}}}}}
                                  for n, g in SAME_SHAPE_GLOBS.items()])]


RULESETS = {"apparmor": apparmor, "two_slot": two_slot, "no_class": no_class, "indirect": indirect,
            "same_shape": same_shape}


def ruleset(name):
    return copy.deepcopy(RULESETS[name]())


def compiled_rulesets():
    """the rulesets whose code objects build() compiles ahead of time (product and accounting builds)"""
    return [ruleset(n) for n in RULESETS]


class _Absent:
    def __deepcopy__(self, memo):
        return self


ABSENT = _Absent()


def _fill(n, hit, first):
    """an annotations map of n entries, `hit` among plain keys, first or last in key order"""
    m = {"%s-note-%d" % ("zz" if first else "aa", i): "v%d" % i for i in range(n - 1)}
    m[hit[0]] = hit[1]
    return m


def metadata_variants():
    """(tag, metadata value or ABSENT): every case of the expansion, built around the app-armor glob and the two-slot
    rule's label / annotation globs"""
    A = APPARMOR
    v = [("absent", ABSENT), ("null", None), ("string", "meta"), ("number", 7), ("list", [{"annotations": {}}]),
         ("empty", {}), ("name-only", {"name": "n"}),
         ("ann-null", {"annotations": None}), ("ann-string", {"annotations": "x"}), ("ann-list", {"annotations": [A + "c"]}),
         ("ann-nonstring", {"annotations": {A + "c": 5}}), ("ann-nonstring-other", {"annotations": {"other": True, A + "c": "runtime/default"}}),
         ("lab-null", {"labels": None, "annotations": {A + "c": "runtime/default"}}),
         ("lab-string", {"labels": "x", "annotations": {A + "c": "runtime/default"}}),
         ("lab-nonstring", {"labels": {"team-a": 3}, "annotations": {OWNER + "a": "ops-x"}}),
         ("anchor-key", {"(annotations)": {}, "labels": {"team-a": "core"}}),
         ("anchor-other-key", {"(name)": "x", "annotations": {A + "c": "runtime/default"}}),
         ("anchor-eq-key", {"=(labels)": {}, "annotations": {A + "c": "unconfined"}}),
         ("anchor-neg-key", {"X(labels)": "x"}),
         ("no-match", {"annotations": {"note": "x"}}), ("no-match-empty", {"annotations": {}}),
         ("one-pass", {"annotations": {A + "c": "runtime/default"}}), ("one-pass-local", {"annotations": {A + "c": "localhost/p"}}),
         ("one-fail", {"annotations": {A + "c": "unconfined"}}), ("one-fail-empty", {"annotations": {A + "c": ""}}),
         ("two-match", {"annotations": {A + "c": "runtime/default", A + "d": "runtime/default"}}),
         ("two-match-fail", {"annotations": {A + "c": "unconfined", A + "d": "x"}}),
         ("three-match", {"annotations": {A + "c": "a", A + "d": "b", A + "e": "c"}}),
         ("pattern-text", {"annotations": {A + "*": "runtime/default"}}), ("pattern-text-fail", {"annotations": {A + "*": "bad"}}),
         ("pattern-text-two", {"annotations": {A + "*": "runtime/default", A + "c": "runtime/default"}}),
         ("bare-prefix", {"annotations": {A: "runtime/default"}}),
         ("team-core", {"labels": {"team-a": "core"}, "annotations": {OWNER + "a": "ops-x"}}),
         ("team-core-fail", {"labels": {"team-a": "core"}, "annotations": {OWNER + "a": "dev"}}),
         ("team-core-noowner", {"labels": {"team-a": "core"}, "annotations": {"note": "x"}}),
         ("team-other", {"labels": {"team-a": "web"}, "annotations": {OWNER + "a": "dev"}}),
         ("team-two", {"labels": {"team-a": "core", "team-b": "core"}, "annotations": {OWNER + "a": "ops-x"}}),
         ("owner-two", {"labels": {"team-a": "core"}, "annotations": {OWNER + "a": "ops-x", OWNER + "b": "ops-y"}}),
         ("team-owner-two", {"labels": {"team-a": "core", "team-b": "web"}, "annotations": {OWNER + "a": "ops-x", OWNER + "b": "dev"}}),
         ("team-text", {"labels": {"team-*": "core"}, "annotations": {OWNER + "*": "ops-x"}}),
         ("ab-x-y", {"annotations": {"a.example.com/k": "x", "b.example.com/k": "y"}}),
         ("ab-y-x", {"annotations": {"a.example.com/k": "y", "b.example.com/k": "x"}}),
         ("ab-x-x", {"annotations": {"a.example.com/k": "x", "b.example.com/q": "x"}}),
         ("ab-only-a", {"annotations": {"a.example.com/k": "x"}}), ("ab-only-b", {"annotations": {"b.example.com/k": "x"}}),
         ("ab-two-a", {"annotations": {"a.example.com/k": "x", "a.example.com/l": "x", "b.example.com/k": "x"}}),
         ("team-none", {"labels": {"app": "x"}, "annotations": {OWNER + "a": "ops-x", A + "c": "localhost/q"}})]
    for n in (1, 4, 5, 9):
        for first in (True, False):
            for val in ("runtime/default", "unconfined"):
                v.append(("scan-%d-%s-%s" % (n, "first" if first else "last", val[:4]),
                          {"annotations": _fill(n, (A + "c", val), first)}))
    return v


def _pod_spec():
    return {"containers": [{"name": "c", "image": "nginx:1.25"}]}


@functools.lru_cache(maxsize=None)
def corpus():
    """-> (documents, namespace labels, tags): every metadata variant at the resource root (Pods, in two namespaces), at
    spec.template (workloads) and at spec.jobTemplate.spec.template (CronJobs), interleaved so that kind boundaries and
    a partial last wave fall inside match waves; then resources without a map at the position"""
    docs, tags = [], []

    def add(tag, d):
        docs.append(d)
        tags.append(tag)

    workloads = [("apps/v1", "Deployment"), ("apps/v1", "StatefulSet"), ("apps/v1", "DaemonSet"), ("batch/v1", "Job")]
    for i, (tag, m) in enumerate(metadata_variants()):
        m = copy.deepcopy(m)
        pod = {"apiVersion": "v1", "kind": "Pod", "spec": _pod_spec()}
        if m is not ABSENT:
            pod["metadata"] = copy.deepcopy(m)
            if isinstance(m, dict):
                pod["metadata"].update(name="pod-%d" % i, namespace="prod-a" if i % 2 else "dev")
        add("pod:" + tag, pod)
        av, kind = workloads[i % len(workloads)]
        tmpl = {"spec": _pod_spec()}
        if m is not ABSENT:
            tmpl["metadata"] = copy.deepcopy(m)
        spec = {"template": tmpl}
        if kind == "StatefulSet" and i % 8 == 1:
            spec["volumeClaimTemplates"] = [{"metadata": copy.deepcopy(m) if m is not ABSENT else {"name": "d"}}]
        add("tmpl:" + tag, {"apiVersion": av, "kind": kind, "metadata": {"name": "w-%d" % i, "namespace": "dev"}, "spec": spec})
        jt = {"spec": {"template": copy.deepcopy(tmpl)}}
        if i % 3 == 0 and m is not ABSENT:
            jt["metadata"] = copy.deepcopy(m)
        add("cron:" + tag, {"apiVersion": "batch/v1", "kind": "CronJob", "metadata": {"name": "cj-%d" % i, "namespace": "dev"},
                            "spec": {"schedule": "* * * * *", "jobTemplate": jt}})
    for i, hole in enumerate((None, "x", [], ABSENT)):
        d = {"apiVersion": "apps/v1", "kind": "Deployment", "metadata": {"name": "hole-%d" % i}, "spec": {}}
        if hole is not ABSENT:
            d["spec"]["template"] = hole
        add("tmpl-hole", d)
        c = {"apiVersion": "batch/v1", "kind": "CronJob", "metadata": {"name": "cj-hole-%d" % i}, "spec": {"jobTemplate": {"spec": {}}}}
        if hole is not ABSENT:
            c["spec"]["jobTemplate"]["spec"]["template"] = hole
        add("cron-hole", c)
    add("cron-hole", {"apiVersion": "batch/v1", "kind": "CronJob", "metadata": {"name": "cj-hole-j"}, "spec": {"jobTemplate": "x"}})
    add("other", {"apiVersion": "v1", "kind": "ConfigMap", "metadata": {"name": "cm", "annotations": {APPARMOR + "c": "x"}}})
    return docs, {"prod-a": {"env": "prod"}, "dev": {"env": "dev"}}, tags


def _anchor_key(k):
    """k is `labels` or `annotations` under an anchor: getPatternValue would take it for the map itself"""
    return any(k == pre + tag + ")" for pre in ("(", "=(", "^(", "X(", "+(", "<(") for tag in ("labels", "annotations"))


def anchorish(doc):
    """some key of a map under a `metadata` key, anywhere in the document, parses as an anchor (the batch's
    RF_ANCHORISH: metadata expansion then goes back to the caller)"""
    if isinstance(doc, dict):
        for k, v in doc.items():
            if k == "metadata" and isinstance(v, dict) and any(_anchor_key(x) for x in v):
                return True
            if anchorish(v):
                return True
    elif isinstance(doc, list):
        return any(anchorish(x) for x in doc)
    return False


def model_row(cls, doc):
    """one plane row from the document: {"st": override, "keys": [...], "values": [...]} (kyv_batch_meta_keys `desc`);
    `cls`: an entry of Batch.meta_keys()["classes"]. After an override the keys and values are not defined (None)."""
    globs = [("labels", g) for g in cls["wild_labels"]] + [("annotations", g) for g in cls["wild_annotations"]]
    row = {"st": ST_NONE, "keys": [g for _, g in globs], "values": [None] * len(globs)}
    node = doc
    for k in POS_PATH[cls["pos"]]:
        node = node.get(k, ABSENT) if isinstance(node, dict) else ABSENT
    if not isinstance(node, dict):
        return row  # the walk does not reach the site
    meta = node.get("metadata")
    if meta is None:
        return row
    over = dict(row, keys=None, values=None)
    if not isinstance(meta, dict):
        return dict(over, st=ST_PANIC)
    if anchorish(doc):
        return dict(over, st=ST_FALLBACK)
    maps = {}
    for tag in ("labels", "annotations"):
        if not cls[tag]:
            continue
        lm = meta.get(tag)
        if lm is None:
            continue
        if not isinstance(lm, dict) or any(not isinstance(x, str) for x in lm.values()):
            return dict(over, st=ST_PANIC)
        maps[tag] = lm
        for s, (t, g) in enumerate(globs):
            if t != tag:
                continue
            hits = [k for k in lm if glob(g, k)]
            if len(hits) > 1:
                return dict(over, st=ST_ND)
            if hits:
                row["keys"][s] = hits[0]
    for s, (t, g) in enumerate(globs):
        row["values"][s] = maps.get(t, {}).get(row["keys"][s])
    return row
