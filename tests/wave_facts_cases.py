"""Crafted batches for the per-wave facts and the hot header plane (kyv_batch_wave_facts), and a straightforward
recomputation of the facts from the documents. Shared by test_wave_facts.py (CPU) and test_gpu_wave_facts.py."""
import copy
import functools

import cases

SIZES = (1, 64, 65, 130)  # single resource, one full wave, one full wave plus a lane, a tail wave of 2 lanes
RF_ROOT_MAP = 1 << 4


@functools.lru_cache(maxsize=None)
def policies():
    return cases.best_practices() + cases.chart_restricted()


def pod(i):
    return {
        "apiVersion": "v1", "kind": "Pod",
        "metadata": {"name": "pod-%d" % i, "namespace": "default", "labels": {"app.kubernetes.io/name": "web"}},
        "spec": {
            "securityContext": {"runAsNonRoot": True, "seccompProfile": {"type": "RuntimeDefault"}},
            "containers": [{
                "name": "main", "image": "registry.example.io/web:1.%d.0" % (i % 7),
                "ports": [{"containerPort": 8080}],
                "resources": {"requests": {"memory": "64Mi", "cpu": "100m"}, "limits": {"memory": "128Mi"}},
                "livenessProbe": {"tcpSocket": {"port": 8080}, "periodSeconds": 10},
                "readinessProbe": {"tcpSocket": {"port": 8080}, "periodSeconds": 5},
                "securityContext": {"allowPrivilegeEscalation": False, "capabilities": {"drop": ["ALL"]},
                                    "readOnlyRootFilesystem": True},
            }] + ([{"name": "side", "image": "registry.example.io/side:2.0.1",
                    "securityContext": {"allowPrivilegeEscalation": False, "capabilities": {"drop": ["ALL"]}}}]
                  if i % 3 == 0 else []),
            "volumes": [{"name": "scratch", "emptyDir": {}}],
        },
    }


def clean(n):
    return [pod(i) for i in range(n)]


def with_ephemeral(n, at):
    docs = clean(n)
    docs[at]["spec"]["ephemeralContainers"] = [{"name": "debug", "image": "registry.example.io/debug:1.0.0",
                                                "securityContext": {"allowPrivilegeEscalation": False}}]
    return docs


# the odd element classes: lists that hold something other than an object where the patterns expect container,
# port and volume objects
ODD_CLASSES = ("containers_null", "containers_str", "containers_obj_int", "ports_null", "volumes_int")


def make_odd(doc, cls):
    d = copy.deepcopy(doc)
    sp = d["spec"]
    if cls == "containers_null":
        sp["containers"] = [None]
    elif cls == "containers_str":
        sp["containers"] = ["x"]
    elif cls == "containers_obj_int":
        sp["containers"] = [sp["containers"][0], 7]
    elif cls == "ports_null":
        sp["containers"][0]["ports"] = [None]
    elif cls == "volumes_int":
        sp["volumes"] = [3]
    else:
        raise ValueError(cls)
    return d


def with_odd(n, first):
    """a clean batch whose resources first, first + 1, ... (modulo n) are one of each odd class; -> (docs, {class: index})"""
    docs = clean(n)
    where = {}
    for j, cls in enumerate(ODD_CLASSES):
        at = (first + j) % n
        if at in where.values():  # fewer resources than classes: the classes that fit
            break
        docs[at] = make_odd(docs[at], cls)
        where[cls] = at
    return docs, where


# ---------------------------------------------------------------- recomputation from the documents
def _lists(cur, segs):
    if not segs:
        return [cur] if isinstance(cur, list) else []
    if segs[0] == "[*]":
        return [x for e in cur for x in _lists(e, segs[1:])] if isinstance(cur, list) else []
    return _lists(cur[segs[0]], segs[1:]) if isinstance(cur, dict) and segs[0] in cur else []


def _all_maps(doc, path):
    assert path[-1] == "[*]"
    return all(isinstance(e, dict) for lst in _lists(doc, path[:-1]) for e in lst)


def expected_facts(docs, order, maps):
    """all-maps word per match wave of 64 positions of the batch order"""
    n = len(docs)
    out = []
    for w0 in range(0, n, 64):
        wave = [docs[int(order[p])] for p in range(w0, min(n, w0 + 64))]
        out.append(sum(1 << j for j, path in enumerate(maps) if all(_all_maps(d, path) for d in wave)))
    return out


def count_values(x):
    if isinstance(x, dict):
        return 1 + sum(count_values(v) for v in x.values())
    if isinstance(x, list):
        return 1 + sum(count_values(v) for v in x)
    return 1
