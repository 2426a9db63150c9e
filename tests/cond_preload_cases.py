"""Crafted rules and resources for the compiled condition kernels' field chains (jit.cpp CondGen, KYV_JC_PRELOAD):
every decision the generated code takes on the entry of a chain's last step alone, and on the arrays and elements
around it -- with each step absent, null, of the wrong type, empty and of lengths 0-5, in Pod, workload and CronJob
form (the autogen rules' longer chains). Shared by test_cond_preload.py (CPU) and
test_gpu_cond_preload.py."""
import copy
import functools
import random

import cases

C3_CONDITION_POLICIES = ("disallow-capabilities", "disallow-capabilities-strict", "restrict-volume-types")
ABSENT = object()


def _pol(name, rules):
    return {"apiVersion": "kyverno.io/v1", "kind": "ClusterPolicy", "metadata": {"name": name},
            "spec": {"background": True, "validationFailureAction": "audit", "rules": rules}}


def _rule(name, validate, pre=None):
    r = {"name": name, "match": {"any": [{"resources": {"kinds": ["Pod"]}}]}, "validate": validate}
    if pre:
        r["preconditions"] = {"all": pre}
    return r


# (a key below spec: the autogen forms rewrite it like the rules' own chains)
TIER = {"key": "{{ request.object.spec.priorityClassName || '' }}", "operator": "Equals", "value": "web"}


def extra_policies():
    return [
        # a deny with two conditions whose keys are chains from one row (the resource's root): both operands are
        # materialised (the program is not a single condition)
        _pol("two-chains", [_rule("image-and-volume", {"message": "bad image with a scratch volume", "deny": {"conditions": {"all": [
            {"key": "{{ request.object.spec.containers[].image }}", "operator": "AnyIn", "value": ["bad:1"]},
            {"key": "{{ request.object.spec.volumes[].name }}", "operator": "AnyIn", "value": ["scratch", "data"]},
        ]}}}, pre=[TIER])]),
        # a foreach with a nested foreach
        _pol("nested-foreach", [_rule("no-host-ports", {"message": "host ports are not allowed", "foreach": [
            {"list": "request.object.spec.containers", "foreach": [
                {"list": "element.ports", "deny": {"conditions": {"any": [
                    {"key": "{{ element.hostPort || `0` }}", "operator": "GreaterThan", "value": 0}]}}}]}]}, pre=[TIER])]),
        # a foreach whose elements must be maps (elementScope)
        _pol("element-scope", [_rule("no-bad-image", {"message": "bad image", "foreach": [
            {"list": "request.object.spec.[initContainers, containers][]", "elementScope": True,
             "deny": {"conditions": {"any": [{"key": "{{ element.image || '' }}", "operator": "Equals", "value": "bad:1"}]}}}]},
            pre=[TIER])]),
        # a precondition with a JMESPath operand
        _pol("jmes-precondition", [_rule("named-main", {"message": "main must not add capabilities", "deny": {"conditions": {"all": [
            {"key": "{{ request.object.spec.containers[].securityContext.capabilities.add[] }}", "operator": "AnyNotIn",
             "value": ["NET_BIND_SERVICE"]}]}}},
            pre=[{"key": "{{ request.object.spec.containers[].name }}", "operator": "AnyIn", "value": ["main"]}])]),
    ]


@functools.lru_cache(maxsize=None)
def policies():
    c3 = [p for p in cases.chart_restricted() if p["metadata"]["name"] in C3_CONDITION_POLICIES]
    assert len(c3) == len(C3_CONDITION_POLICIES)
    return c3 + extra_policies()


def can_skip(rule_name):
    """whether a rule (or the autogen form of one) of policies() can skip a matched resource: it has preconditions, or
    it is a foreach (no element applied). A plain deny without preconditions decides every resource it matches."""
    for prefix in ("autogen-cronjob-", "autogen-"):
        if rule_name.startswith(prefix):
            rule_name = rule_name[len(prefix):]
            break
    rule, = [r for p in policies() for r in p["spec"]["rules"] if r["name"] == rule_name]
    return "preconditions" in rule or "foreach" in rule["validate"]


def compiled_rulesets():
    """the rulesets whose kernels build() compiles ahead of time (with the chains and with KYV_JC_PRELOAD=0, product
    and accounting builds)"""
    return [policies()]


# ---------------------------------------------------------------- resources
def container(name="main", image="registry.example.io/web:1.0.0", add=ABSENT, drop=("ALL",), ports=ABSENT):
    caps = {}
    if add is not ABSENT:
        caps["add"] = copy.deepcopy(add) if not isinstance(add, tuple) else list(add)
    if drop is not ABSENT:
        caps["drop"] = copy.deepcopy(drop) if not isinstance(drop, tuple) else list(drop)
    c = {"name": name, "image": image, "securityContext": {"allowPrivilegeEscalation": False, "capabilities": caps}}
    if ports is not ABSENT:
        c["ports"] = ports
    return c


def wrap(form, i, spec, tier=None):
    meta = {"name": "%s-%d" % (form.lower(), i), "namespace": "default"}
    if tier and isinstance(spec, dict):
        spec["priorityClassName"] = tier
    if form == "Pod":
        d = {"apiVersion": "v1", "kind": "Pod", "metadata": meta}
        if spec is not ABSENT:
            d["spec"] = spec
        return d
    tmpl = {"metadata": {"labels": {"app": "web"}}}
    if spec is not ABSENT:
        tmpl["spec"] = spec
    if form == "Deployment":
        return {"apiVersion": "apps/v1", "kind": "Deployment", "metadata": meta,
                "spec": {"replicas": 1, "selector": {"matchLabels": {"app": "web"}}, "template": tmpl}}
    return {"apiVersion": "batch/v1", "kind": "CronJob", "metadata": meta,
            "spec": {"schedule": "* * * * *", "jobTemplate": {"spec": {"template": tmpl}}}}


def put(spec, path, val):
    """spec with the value at path (keys and list indices) set to val, or removed"""
    spec = copy.deepcopy(spec)
    cur = spec
    for k in path[:-1]:
        cur = cur[k]
    if val is ABSENT:
        del cur[path[-1]]
    else:
        cur[path[-1]] = val
    return spec


VOLUMES = (ABSENT, None, [], "x", {}, [{"name": "scratch", "emptyDir": {}}], [{"name": "host", "hostPath": {"path": "/"}}],
           [{"name": "data", "persistentVolumeClaim": {"claimName": "d"}}, {"name": "scratch", "emptyDir": {}}],
           [None], [{"name": "a", "configMap": {"name": "c"}}, None, {"name": "n", "nfs": {"server": "s", "path": "/"}}],
           [{"name": "s%d" % k, "secret": {"secretName": "s"}} for k in range(5)], [{}], [3])
CAPS_ADD = (ABSENT, None, "CHOWN", 7, {}, [], ["CHOWN"], ["SYS_ADMIN"], ["NET_BIND_SERVICE"], [None], ["CHOWN", None, "NET_RAW"],
            ["NET_BIND_SERVICE", "NET_BIND_SERVICE"], [""], ["KILL", "MKNOD", "SETUID", "SETGID", "CHOWN"])
CAPS_DROP = (ABSENT, None, "ALL", {}, [], ["ALL"], ["NET_RAW"], ["NET_RAW", "ALL"], [None], ["all"],
             ["CHOWN", "KILL", "MKNOD", "SETUID", "ALL"])
WRONG = (ABSENT, None, "x", 7, [], {})   # a step of the chain: absent, null, scalars, an array, an empty map


def base_spec():
    return {"containers": [container(add=["NET_BIND_SERVICE"])], "volumes": [{"name": "scratch", "emptyDir": {}}]}


def step_specs():
    """pod specs in which each step of spec.containers[].securityContext.capabilities.add[] (and drop[]) in turn is
    absent, null, a scalar where a map is expected, a map where an array is expected, an empty array"""
    out = [ABSENT, None, "x", 7, [], {}]                       # the spec itself
    b = base_spec()
    out += [put(b, ("containers",), v) for v in WRONG]          # the list
    out += [put(b, ("containers", 0), v) for v in WRONG[1:]]   # the element: null, not a map
    out += [put(b, ("containers", 0, "securityContext"), v) for v in WRONG]
    out += [put(b, ("containers", 0, "securityContext", "capabilities"), v) for v in WRONG]
    out += [put(b, ("containers", 0, "securityContext", "capabilities", "add"), v) for v in CAPS_ADD]
    out += [put(b, ("containers", 0, "securityContext", "capabilities", "drop"), v) for v in CAPS_DROP]
    # the same below initContainers and ephemeralContainers (their own trie positions and columns)
    for member in ("initContainers", "ephemeralContainers"):
        m = put(b, (member,), [container(name="aux", add=["CHOWN"])])
        out += [put(m, (member,), v) for v in WRONG[1:]]
        out += [put(m, (member, 0, "securityContext", "capabilities"), v) for v in (None, "x", [])]
        out += [put(m, (member, 0, "securityContext", "capabilities", "add"), v) for v in (None, {}, [], ["SYS_ADMIN"], [None])]
        out += [put(m, (member, 0, "securityContext", "capabilities", "drop"), v) for v in (None, {}, [], ["NET_RAW"])]
    return out


def random_spec(rng, i):
    """members of the multi-select present by the bits of i (every combination), 0-5 elements each, 0-5 capabilities
    below each element; names, images, ports and volumes for the other rules"""
    spec = {}
    for bit, member in enumerate(("containers", "initContainers", "ephemeralContainers")):
        if not (i >> bit) & 1:
            continue
        elems = []
        for k in range(rng.randint(0, 5)):
            roll = rng.random()
            if roll < 0.06:
                elems.append(rng.choice([None, "x", 5]))
                continue
            addn, dropn = rng.randint(0, 5), rng.randint(0, 5)
            good = rng.random() < 0.7
            add = [rng.choice(["NET_BIND_SERVICE"] if good else ["NET_BIND_SERVICE", "CHOWN", "SYS_ADMIN", "KILL"]) for _ in range(addn)]
            drop = [rng.choice(["ALL", "NET_RAW"]) for _ in range(dropn)]
            if good and rng.random() < 0.8:
                drop.append("ALL")
            ports = ABSENT if rng.random() < 0.4 else [
                {"containerPort": 8080, **({"hostPort": rng.choice([0, 80])} if rng.random() < 0.3 else {})}
                for _ in range(rng.randint(0, 5))]
            elems.append(container(name=rng.choice(["main", "side", "aux"]), image=rng.choice(["registry.example.io/web:1.0.0"] * 4 + ["bad:1"]),
                                   add=add if addn or rng.random() < 0.5 else ABSENT, drop=drop if drop or rng.random() < 0.5 else ABSENT,
                                   ports=ports))
        spec[member] = elems
    v = VOLUMES[i % len(VOLUMES)]
    if v is not ABSENT:
        spec["volumes"] = copy.deepcopy(v)
    return spec


@functools.lru_cache(maxsize=None)
def corpus():
    """-> (docs, namespace labels): the step variants in each of the three forms, then the random specs, shuffled so
    that the lanes of a wave differ"""
    rng = random.Random(11)
    docs = []
    for form in ("Pod", "Deployment", "CronJob"):
        for j, spec in enumerate(step_specs()):
            docs.append(wrap(form, len(docs), spec if spec is ABSENT else copy.deepcopy(spec), "web" if j % 4 else None))
    for i in range(96):  # per form, every combination of the three members four times
        form = ("Pod", "Deployment", "CronJob")[i % 3]
        docs.append(wrap(form, len(docs), random_spec(rng, i // 3), "web" if i % 5 else "db"))
    for form in ("Pod", "Deployment", "CronJob"):  # what the two-chains rule denies: both of its lists hit
        for k in range(3):
            spec = put(base_spec(), ("containers",), [container() for _ in range(k)] + [container(name="side", image="bad:1")])
            docs.append(wrap(form, len(docs), spec, "web"))
    rng.shuffle(docs)
    return docs, {}
