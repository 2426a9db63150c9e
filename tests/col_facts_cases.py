"""Crafted batches for the column facts (kyv_batch_col_facts, kyv_layout.h ColFacts), a straightforward recomputation
of the rows from the documents, and the rules and resources of the parity runs that cross every step of
[ephemeralContainers|initContainers|containers][].securityContext.* through absent, empty, well-formed and malformed
values. Shared by test_col_facts.py (CPU) and test_gpu_col_facts.py."""
import copy
import functools

import cases
import wave_facts_cases as W

SIZES = (1, 63, 64, 65, 130)
ABSENT = object()
MEMBERS = ("ephemeralContainers", "initContainers", "containers")
ODD_LISTS = ([], None, "x", {})          # a list position that holds something, but no element


@functools.lru_cache(maxsize=None)
def policies():
    """the C3 ruleset: its path trie is the one the bench's plane is numbered by"""
    return cases.best_practices() + cases.chart_restricted()


def pod(i):
    """a pod with one list only (containers) and no ports: every other list position is empty"""
    d = W.pod(i)
    for c in d["spec"]["containers"]:
        c.pop("ports", None)
    del d["spec"]["volumes"]
    return d


def deployment(i):
    p = pod(i)
    return {"apiVersion": "apps/v1", "kind": "Deployment", "metadata": {"name": "dep-%d" % i, "namespace": "default"},
            "spec": {"replicas": 1, "selector": {"matchLabels": {"app": "web"}},
                     "template": {"metadata": {"labels": {"app": "web"}}, "spec": p["spec"]}}}


def clean(n):
    return [pod(i) for i in range(n)]


# ---------------------------------------------------------------- recomputation from the documents
def _values(cur, segs):
    """every value found at the path: keys through objects, "[*]" through the elements of arrays"""
    if not segs:
        return [cur]
    if segs[0] == "[*]":
        return [x for e in cur for x in _values(e, segs[1:])] if isinstance(cur, list) else []
    return _values(cur[segs[0]], segs[1:]) if isinstance(cur, dict) and segs[0] in cur else []


def expected_rows(docs, order, desc):
    """the empty word per match wave of 64 positions of the batch order"""
    n = len(docs)
    out = []
    for w0 in range(0, n, 64):
        wave = [docs[int(order[p])] for p in range(w0, min(n, w0 + 64))]
        out.append(sum(1 << j for j, path in enumerate(desc["lists"][:64]) if not any(_values(d, path) for d in wave)))
    return out


# ---------------------------------------------------------------- parity runs
PATTERN_POLICIES = ("disallow-privileged", "disallow-privileged-containers", "disallow-host-process", "disallow-selinux",
                    "restrict-seccomp", "restrict-seccomp-strict", "disallow-proc-mount", "require-run-as-nonroot",
                    "require-run-as-non-root-user", "disallow-privilege-escalation")
CONDITION_POLICIES = ("disallow-capabilities", "disallow-capabilities-strict", "restrict-volume-types")


@functools.lru_cache(maxsize=None)
def parity_policies():
    """the C3 pattern rules that read the crossed paths and the four C3 condition rules (autogen adds their workload
    and CronJob forms)"""
    want = PATTERN_POLICIES + CONDITION_POLICIES
    pols = [p for p in policies() if p["metadata"]["name"] in want]
    assert len(pols) == len(want), [p["metadata"]["name"] for p in pols]
    return pols


def compiled_rulesets():
    """the rulesets whose kernels build() compiles ahead of time (product and accounting builds, with the column facts
    and with KYV_JIT_COLFACTS=0)"""
    return [parity_policies()]


def good_container(name="side"):
    return {"name": name, "image": "registry.example.io/web:1.0.0",
            "securityContext": {"allowPrivilegeEscalation": False, "runAsNonRoot": True, "capabilities": {"drop": ["ALL"]},
                                "seccompProfile": {"type": "RuntimeDefault"}}}


# below securityContext: (key, leaf key, passing, failing, of the wrong type)
SUBS = (("seLinuxOptions", "type", "container_t", "spc_t", 5),
        ("seccompProfile", "type", "RuntimeDefault", "Unconfined", []),
        ("windowsOptions", "hostProcess", False, True, "x"),
        ("capabilities", "add", ["NET_BIND_SERVICE"], ["SYS_ADMIN"], "CHOWN"))


def member_variants():
    """values of one member list: the list itself, its element, securityContext and each map below it crossed through
    absent, {}, an object with the leaf (absent, passing, failing, of the wrong type), null, string, number, array"""
    out = [ABSENT, None, "x", 5, {}, []]
    out += [[e] for e in (None, "x", 5, [], {})]

    def elem(sc):
        c = good_container("main")
        if sc is ABSENT:
            del c["securityContext"]
        else:
            c["securityContext"] = sc
        return [c]

    out += [elem(sc) for sc in (ABSENT, {}, None, "x", 5, [])]
    for key, leaf, ok, bad, wrong in SUBS:
        for v in ({}, None, "x", 5, [], {leaf: ok}, {leaf: bad}, {leaf: wrong}):
            out.append(elem({"runAsNonRoot": True, key: copy.deepcopy(v)}))
    out += [elem({"privileged": v}) for v in (False, True, "false", None, 5)]
    return out


@functools.lru_cache(maxsize=None)
def parity_corpus():
    """-> (docs, namespace labels): every variant in each member list and each form; 0 to 2 well-formed elements in
    front of the crossed one, so the lists have 0 to 3 elements; the other members present in some neighbours only"""
    docs = []
    for form in ("Pod", "Deployment", "CronJob"):
        for m, member in enumerate(MEMBERS):
            for j, v in enumerate(member_variants()):
                spec = {}
                if member != "containers" and j % 2:
                    spec["containers"] = [good_container("main")]
                if v is not ABSENT:
                    v = copy.deepcopy(v)
                    if isinstance(v, list) and v:
                        v = [good_container("s%d" % k) for k in range((j + m) % 3)] + v
                    spec[member] = v
                if j % 5 == 1:  # (restrict-volume-types: a volume it allows, one it denies)
                    spec["volumes"] = [{"name": "scratch", "emptyDir": {}}]
                elif j % 5 == 2:
                    spec["volumes"] = [{"name": "host", "hostPath": {"path": "/"}}]
                if j % 7 == 3:
                    spec["securityContext"] = {"seccompProfile": {"type": "RuntimeDefault"}, "runAsNonRoot": True}
                docs.append(_wrap(form, len(docs), spec))
    return docs, {}


def _wrap(form, i, spec):
    meta = {"name": "%s-%d" % (form.lower(), i), "namespace": "default"}
    if form == "Pod":
        return {"apiVersion": "v1", "kind": "Pod", "metadata": meta, "spec": spec}
    tmpl = {"metadata": {"labels": {"app": "web"}}, "spec": spec}
    if form == "Deployment":
        return {"apiVersion": "apps/v1", "kind": "Deployment", "metadata": meta,
                "spec": {"replicas": 1, "selector": {"matchLabels": {"app": "web"}}, "template": tmpl}}
    return {"apiVersion": "batch/v1", "kind": "CronJob", "metadata": meta,
            "spec": {"schedule": "* * * * *", "jobTemplate": {"spec": {"template": tmpl}}}}


def plain_batch(n=200):
    """no resource has initContainers, ephemeralContainers or ports, and every step is an object: the facts rule out
    every load of those lists"""
    return [_wrap(("Pod", "Deployment")[i % 2], i, {"containers": [good_container("main")] * (1 + i % 2)}) for i in range(n)]


def dense_batch(n=200):
    """every wave holds every list and a malformed step: the facts rule out nothing"""
    docs = []
    for i in range(n):
        spec = {m: [dict(good_container("c"), ports=[{"containerPort": 80}])] for m in MEMBERS}
        if i % 16 == 0:
            spec["containers"][0]["securityContext"] = "x"
            spec["securityContext"] = None
        docs.append(_wrap(("Pod", "Deployment")[i % 2], i, spec))
    return docs
