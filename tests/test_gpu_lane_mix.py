"""Lane-divergence parity of the compiled walk and condition kernels (jit.cpp) and of the interpreter, pair by pair
against the oracle, failing paths and messages included.

The corpus is crafted so that the lanes of one wave disagree wherever the generated code branches: 150 resources (two
full waves and a partial one; the batch is kind-major, so kind boundaries fall inside waves), container lists of 0-4
elements that differ between neighbouring lanes, array-valued / absent / null / integer / float values at leaf
positions, lanes that fail at the first entry of a pattern map beside lanes that fail at its last, an anyPattern rule
whose lanes pass on different alternatives, and the deny / foreach rules over the same container lists. The rules are
the C3 set."""
import functools

import pytest

import cases
import parity_util as PU

N = 150
KINDS = ["Pod", "Pod", "Deployment", "Pod", "CronJob", "DaemonSet", "Pod", "StatefulSet", "Job", "ConfigMap"]

# values a leaf position takes from lane to lane: the typed column entry covers strings, booleans and null; numbers
# and arrays send the lane to the node row (the array-valued-leaf loop)
BOOLISH = [False, True, None, "false", 0, 1.5, [False], [False, True], "true", []]
CAPS = [["ALL"], ["NET_RAW"], None, "ALL", [], ["ALL", "CHOWN"], ["NET_BIND_SERVICE"], [""], [None, "ALL"], 7]
SECCOMP = ["RuntimeDefault", "Localhost", "Unconfined", None, 7, ["RuntimeDefault"], 2.5]
IMAGES = ["registry.domain.com/app:1.2", "nginx:latest", "nginx", 5, None, ["nginx:1"], "a:b", 1.25]
QTY = ["100Mi", "1", 1, 1.5, None, ["1"], "", "250m"]


def _pick(lst, *k):
    h = 2166136261
    for x in k:
        h = ((h ^ (x + 0x9E37)) * 16777619) & 0xFFFFFFFF
    return lst[(h >> 7) % len(lst)]


def _container(i, j, which):
    c = {"name": "c%d-%d-%d" % (i, which, j)}
    m = (i * 7 + j * 3 + which) % 11
    if m != 3:
        c["image"] = _pick(IMAGES, i, j, which)
    sc = {}
    if m % 4 != 1:
        sc["allowPrivilegeEscalation"] = _pick(BOOLISH, i, j, which, 1)
    if m % 3 != 2:
        sc["privileged"] = _pick(BOOLISH, i, j, which, 2)
    if (i + j) % 3 != 2:
        sc["runAsNonRoot"] = True if i % 3 == 1 else _pick(BOOLISH, i, j, which, 3)
    if m % 5 != 0:
        sc["runAsUser"] = _pick([1000, 0, "1000", None, 1.5, [1], -1], i, j, which, 4)
    caps = {}
    if m % 2 == 0:
        caps["drop"] = _pick(CAPS, i, j, which, 5)
    if m % 3 == 0:
        caps["add"] = _pick(CAPS, i, j, which, 6)
    if caps or m == 7:
        sc["capabilities"] = caps if m != 7 else None
    if m % 4 == 2:
        sc["seccompProfile"] = {"type": _pick(SECCOMP, i, j, which, 7)}
    if m == 5:
        sc["seLinuxOptions"] = {"type": _pick(["container_t", "spc_t", None, 3], i, j), "user": "u" if j else None}
    if m == 9:
        sc["procMount"] = _pick(["Default", "Unmasked", None, ["Default"]], i, j)
    if m == 10:
        c["securityContext"] = _pick([None, {}, [], "x", 3], i, j, which, 8)
    elif m != 6:
        c["securityContext"] = sc
    if m % 3 != 1:
        c["resources"] = {"limits": {"memory": _pick(QTY, i, j, 9)},
                          "requests": {"cpu": _pick(QTY, i, j, 10), "memory": _pick(QTY, i, j, 11)}}
        if m == 8:
            del c["resources"]["requests"]
    if m % 4 == 0:
        c["ports"] = [{"containerPort": 80, "hostPort": _pick([0, 80, None, "0", 0.0, [0]], i, j, p)} if p != 1 else
                      {"containerPort": 81} for p in range((i + j) % 4)]
    return c


def _podspec(i):
    spec = {}
    # neighbouring lanes: 0-4 containers, and init / ephemeral lists of other lengths (or absent, or null)
    spec["containers"] = [_container(i, j, 0) for j in range(i % 5)]
    if i % 4 != 3:
        spec["initContainers"] = [_container(i, j, 1) for j in range((i * 3 + 1) % 5)]
    if i % 6 == 1:
        spec["ephemeralContainers"] = [_container(i, j, 2) for j in range((i // 6) % 3)]
    if i % 17 == 5:
        spec["containers"] = _pick([None, {}, "x"], i)
    # host namespaces: within a wave some lanes fail at the map's first entry (hostIPC), some at its last (hostPID)
    if i % 7 == 1:
        spec["hostIPC"] = True
    elif i % 7 == 2:
        spec["hostPID"] = True
    elif i % 7 == 3:
        spec["hostNetwork"] = _pick(BOOLISH, i, 12)
    elif i % 7 == 4:
        spec.update(hostIPC=False, hostNetwork=_pick(BOOLISH, i, 13), hostPID=_pick(BOOLISH, i, 14))
    # anyPattern run-as-non-root: i % 3 == 0 passes on the pod-level alternative, == 1 on the container-level one
    psc = {}
    if i % 3 == 0:
        psc["runAsNonRoot"] = True
    elif i % 9 == 2:
        psc["runAsNonRoot"] = _pick(BOOLISH, i, 15)
    if i % 4 == 0:
        psc["seccompProfile"] = {"type": _pick(SECCOMP, i, 16)}
    if i % 10 == 3:
        psc["sysctls"] = [{"name": _pick(["kernel.shm_rmid_forced", "kernel.msgmax", None, 4], i, s)} for s in range(i % 3)]
    if i % 10 == 7:
        psc["runAsUser"] = _pick([0, 1000, "0", None], i, 17)
    if psc or i % 11 == 0:
        spec["securityContext"] = psc if i % 13 != 6 else None
    if i % 5 != 2:
        spec["volumes"] = [_pick([{"name": "v", "emptyDir": {}}, {"name": "h", "hostPath": {"path": "/x"}},
                                  {"name": "n", "hostPath": None}, {"name": "s", "secret": {"secretName": "s"}},
                                  {"name": "g", "gitRepo": {}}, {}], i, q) for q in range(i % 4)]
    return spec


def _resource(i):
    kind = KINDS[i % len(KINDS)]
    meta = {"name": "r%03d" % i, "namespace": "ns%d" % (i % 3)}
    if i % 4 != 1:
        meta["labels"] = {}
        if i % 4 == 0:
            meta["labels"]["app.kubernetes.io/name"] = _pick(["web", "", "x"], i, 18)
        if i % 8 >= 5:
            meta["labels"]["app.kubernetes.io/component"] = _pick(["db", ""], i, 19)
    if i % 9 == 4:
        meta["annotations"] = {"container.apparmor.security.beta.kubernetes.io/c0":
                               _pick(["runtime/default", "unconfined", "localhost/p"], i, 20)}
    doc = {"apiVersion": "v1", "kind": kind, "metadata": meta}
    tmeta = {"labels": dict(meta.get("labels") or {})}
    if kind == "Pod":
        doc["spec"] = _podspec(i)
    elif kind == "CronJob":
        doc["apiVersion"] = "batch/v1"
        doc["spec"] = {"schedule": "* * * * *",
                       "jobTemplate": {"spec": {"template": {"metadata": tmeta, "spec": _podspec(i)}}}}
    elif kind == "ConfigMap":
        doc["data"] = {"k": "v"}
    else:
        doc["apiVersion"] = "batch/v1" if kind == "Job" else "apps/v1"
        doc["spec"] = {"template": {"metadata": tmeta, "spec": _podspec(i)}}
    return doc


@functools.lru_cache(maxsize=None)
def _corpus():
    pols = cases.best_practices() + cases.chart_restricted()
    docs = [_resource(i) for i in range(N)]
    return pols, docs, PU.oracle_pairs(pols, docs, {})


def test_corpus_is_not_vacuous():
    """from the oracle alone: the crafted pairs hold PASS, FAIL and SKIP verdicts, single-pattern, anyPattern and
    deny / foreach rules among the failing ones, and anyPattern passes on more than one alternative's resources"""
    pols, docs, ora = _corpus()
    assert len(docs) == 150
    n = {}
    for rr in ora.values():
        n[rr["status"]] = n.get(rr["status"], 0) + 1
    assert n.get("pass", 0) > 100 and n.get("fail", 0) > 100 and n.get("skip", 0) > 0, n
    by_rule = {}
    for (pol, rule, ri), rr in ora.items():
        by_rule.setdefault((pol, rule), {}).setdefault(rr["status"], []).append(ri)
    for key in (("disallow-host-namespaces", "host-namespaces"), ("require-run-as-nonroot", "run-as-non-root"),
                ("disallow-capabilities-strict", "require-drop-all"), ("restrict-volume-types", "restricted-volumes")):
        assert by_rule[key].get("pass") and by_rule[key].get("fail"), (key, {s: len(v) for s, v in by_rule[key].items()})
    # both alternatives of run-as-non-root carry passes: pod-level (i % 3 == 0) and container-level (i % 3 == 1) lanes
    passed = set(by_rule[("require-run-as-nonroot", "run-as-non-root")]["pass"])
    assert any(i % 3 == 0 for i in passed) and any(i % 3 == 1 for i in passed)
    # host-namespaces fails both at the map's first entry (hostIPC lanes) and at its last (hostPID lanes)
    failed = set(by_rule[("disallow-host-namespaces", "host-namespaces")]["fail"])
    assert any(i % 7 == 1 for i in failed) and any(i % 7 == 2 for i in failed)


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [True, False], ids=["compiled", "interpreter"])
def test_lane_mix_against_oracle(jit, monkeypatch):
    pols, docs, ora = _corpus()
    monkeypatch.setattr(PU, "oracle_pairs", lambda *a, **k: ora)  # one oracle run for every case
    st, res = PU.compare(pols, docs, {}, backend="gpu", jit=jit)
    assert bool(res.jit) == jit
    assert st["nbad"] == 0, st["bad"]
    assert st["compared"] > 2000 and st["messages"] > 100, st
