"""Crafted batches for the order within a kind (kyv_batch_shape_keys) and a straightforward recomputation of the shape
key from the documents. Shared by test_shape_order.py (CPU) and test_gpu_shape_order.py."""
import copy

import wave_facts_cases as W


# ---------------------------------------------------------------- recomputation from the documents
def max_len(cur, segs):
    """largest length of an array at path `segs` under `cur` (a "[*]" segment follows every element); 0: none"""
    if not segs:
        return len(cur) if isinstance(cur, list) else 0
    if segs[0] == "[*]":
        return max((max_len(e, segs[1:]) for e in cur), default=0) if isinstance(cur, list) else 0
    return max_len(cur[segs[0]], segs[1:]) if isinstance(cur, dict) and segs[0] in cur else 0


def key_of(doc, paths, bits):
    key = 0
    for p in paths:
        assert p[-1] == "[*]"
        key = (key << bits) | min(max_len(doc, p[:-1]), (1 << bits) - 1)
    return key


def expected_order(docs, keys):
    cls = {}
    for d in docs:
        cls.setdefault(d["kind"], len(cls))  # classes in first-occurrence order
    return sorted(range(len(docs)), key=lambda i: (cls[docs[i]["kind"]], keys[i], i))


# ---------------------------------------------------------------- crafted batches
def deployment(i, ncont):
    spec = copy.deepcopy(W.pod(i)["spec"])
    spec["containers"] = [dict(spec["containers"][0], name="c%d" % j) for j in range(ncont)]
    return {"apiVersion": "apps/v1", "kind": "Deployment", "metadata": {"name": "dep-%d" % i, "namespace": "default"},
            "spec": {"replicas": 1, "template": {"metadata": {"labels": {"app": "web"}}, "spec": spec}}}


def equal_keys(n):
    return [W.pod(3 * i + 1) for i in range(n)]  # pod(i) has a second container when i % 3 == 0


def distinct_keys(n):
    """n pods, no two with the same key, the keys in no order: (containers, volumes, ports of container 0) lengths"""
    docs = []
    for i in range(n):
        j = (i * 37) % 343  # a permutation step: 37 and 343 are coprime
        d = W.pod(1)
        c0 = d["spec"]["containers"][0]
        c0["ports"] = [{"containerPort": 8000 + q} for q in range(j % 7)]
        d["spec"]["containers"] = [c0] + [dict(c0, name="c%d" % q, ports=[]) for q in range(j // 7 % 7)]
        d["spec"]["volumes"] = [{"name": "v%d" % q, "emptyDir": {}} for q in range(j // 49)]
        d["metadata"]["name"] = "pod-%d" % i
        docs.append(d)
    return docs


def extremes():
    """the contents of the list positions a key must cope with"""
    docs = []
    for odd in ([], None, "none"):  # containers as [], null and a string: length 0
        d = W.pod(1)
        d["spec"]["containers"] = odd
        docs.append(d)
    d = W.pod(1)  # a list of 300 elements: clamped to 7
    d["spec"]["containers"] = [dict(d["spec"]["containers"][0], name="c%d" % j) for j in range(300)]
    docs.append(d)
    d = W.pod(1)  # a non-object element beside an object
    d["spec"]["containers"] = [5, d["spec"]["containers"][0], None]
    docs.append(d)
    d = W.pod(0)  # a nested list under only one element (the second container has no ports)
    d["spec"]["containers"][0]["ports"] = [{"containerPort": 8080 + j} for j in range(4)]
    docs.append(d)
    d = W.pod(1)  # volumes missing, spec.securityContext.sysctls present
    del d["spec"]["volumes"]
    d["spec"]["securityContext"]["sysctls"] = [{"name": "kernel.shm_rmid_forced", "value": "0"}] * 2
    docs.append(d)
    for j, d in enumerate(docs):
        d["metadata"]["name"] = "extreme-%d" % j
    return docs


def cronjob(i, ncont):
    tmpl = deployment(i, ncont)["spec"]["template"]
    return {"apiVersion": "batch/v1", "kind": "CronJob", "metadata": {"name": "cj-%d" % i, "namespace": "default"},
            "spec": {"schedule": "* * * * *", "jobTemplate": {"spec": {"template": tmpl}}}}


def mixed_kinds(n):
    """pods, deployments and cron jobs interleaved, 2 : 2 : 1 (at n = 130 every kind has fewer than 64, so class and
    key boundaries fall inside one wave), the extremes spread through the pods, container counts cycling"""
    ext = extremes()
    docs = []
    for i in range(n):
        if i % 5 in (2, 3):
            docs.append(deployment(i, 1 + (i // 5) % 3))
        elif i % 5 == 4:
            docs.append(cronjob(i, 1 + (i // 5) % 4))
        elif ext and i % 5 == 0:
            docs.append(ext.pop())
        else:
            docs.append(W.pod(i))
    return docs
