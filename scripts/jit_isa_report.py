"""Instruction mix of a workload's runtime-compiled kernels, for people to read (no test depends on it).

The generated source (Ruleset.jit_source(), as scripts/jit_meta.py obtains it) is compiled to gfx950 assembly with the
options jit.cpp passes to hipRTC, and every kernel's body is counted:

  insts       instructions
  valu        v_* instructions (one issue slot each; 64-bit and lane-access ones take more than one pass)
  lane        v_readlane / v_writelane / v_readfirstlane: SGPR spill and reload traffic, plus wave-uniform broadcasts
  v_mov       v_mov_b32 / v_mov_b64 (value merges at control-flow joins, spill-lane set-up)
  s_nop       hazard padding (mostly behind lane writes)
  salu / smem / vmem / lds / branch
  sgpr_spill, vgpr_spill, scratch  from the code object's metadata (.sgpr_spill_count, .vgpr_spill_count,
                                   .private_segment_fixed_size), with the SGPR / VGPR counts

  python scripts/jit_isa_report.py [c3|c2|c4|c5] [--json OUT.json] [--asm OUT.s | --from-asm IN.s]
                                    [--src IN.hip | --save-src OUT.hip] [--acct] [extra -D defines...]

Generator knobs come from the environment (KYV_JIT_*), as in the product. hipRTC on another machine may schedule
differently in detail; the counts are static, not weighted by how often a block runs.
"""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLANG = os.environ.get("KYV_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
COLS = ("insts", "valu", "lane", "v_mov", "s_nop", "salu", "smem", "vmem", "lds", "branch", "sgpr_spill", "vgpr_spill",
        "scratch", "sgprs", "vgprs")
NOT_SALU = ("s_load", "s_buffer_load", "s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_endpgm", "s_barrier", "s_sleep",
            "s_setprio", "s_code_end", "s_sethalt", "s_trap", "s_setpc", "s_swappc", "s_getpc")


def count_body(lines):
    c = dict.fromkeys(COLS[:10], 0)
    for ln in lines:
        t = ln.strip()
        if not t or t[0] in ".;" or t.endswith(":"):
            continue
        op = t.split()[0]
        if not re.match(r"^[a-z][a-z0-9_]*$", op):
            continue
        c["insts"] += 1
        if op.startswith("v_"):
            c["valu"] += 1
            if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
                c["lane"] += 1
            elif op.startswith(("v_mov_b32", "v_mov_b64")):
                c["v_mov"] += 1
        elif op == "s_nop":
            c["s_nop"] += 1
        elif op.startswith(("s_load", "s_buffer_load")):
            c["smem"] += 1
        elif op.startswith(("s_branch", "s_cbranch")):
            c["branch"] += 1
        elif op.startswith(("global_", "flat_", "scratch_", "buffer_")):
            c["vmem"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith("s_") and not op.startswith(NOT_SALU):
            c["salu"] += 1
    return c


def parse_asm(text):
    """{kernel: counts} for every kernel the metadata names"""
    lines = text.splitlines()
    # amdhsa.kernels records: "  - .key: v" opens one, its own fields sit at four spaces (argument fields deeper)
    recs = []
    for ln in lines:
        m = re.match(r"^(  - |    )\.(\w+):\s*(\S+)", ln)
        if not m:
            continue
        if m.group(1) == "  - ":
            recs.append({})
        if recs:
            recs[-1][m.group(2)] = m.group(3)
    out = {}
    for rec in recs:
        sym = rec.get("symbol", "")
        if not sym.endswith(".kd"):
            continue
        name = sym[:-3]
        a = next((i for i, ln in enumerate(lines) if ln.startswith(name + ":")), None)
        if a is None:
            continue
        b = a
        while b < len(lines) and not lines[b].startswith(".Lfunc_end"):
            b += 1
        c = count_body(lines[a + 1:b])
        c["sgpr_spill"] = int(rec.get("sgpr_spill_count", 0))
        c["vgpr_spill"] = int(rec.get("vgpr_spill_count", 0))
        c["scratch"] = int(rec.get("private_segment_fixed_size", 0))
        c["sgprs"] = int(rec.get("sgpr_count", 0))
        c["vgprs"] = int(rec.get("vgpr_count", 0))
        out[name] = c
    return out


def main():
    args = sys.argv[1:]
    wl, js, asm_out, asm_in, src_in, src_out, acct, extra = "c3", None, None, None, None, None, False, []
    while args:
        a = args.pop(0)
        if a == "--json":
            js = args.pop(0)
        elif a == "--asm":
            asm_out = args.pop(0)
        elif a == "--from-asm":  # count an assembly file written earlier with --asm (no compile)
            asm_in = args.pop(0)
        elif a == "--src":  # a generated source saved earlier with --save-src (another build's generator)
            src_in = args.pop(0)
        elif a == "--save-src":
            src_out = args.pop(0)
        elif a == "--acct":
            acct = True
        elif a.startswith("-"):
            extra.append(a)
        else:
            wl = a
    if asm_in:
        with open(asm_in) as fh:
            report(wl, parse_asm(fh.read()), "assembly file " + os.path.basename(asm_in), js, {})
        return
    if src_in:
        with open(src_in) as fh:
            src = fh.read()
    else:
        import bench
        from kyverno_amd import engine as E
        src = E.Ruleset(bench.load_policies(wl)).jit_source()[0]
    if src_out:
        with open(src_out, "w") as fh:
            fh.write(src)
    d = tempfile.mkdtemp()
    f = os.path.join(d, "k.hip")
    with open(f, "w") as fh:
        fh.write(src)
    s = asm_out or os.path.join(d, "k.s")
    defs = os.environ.get("KYV_JIT_DEFS", "-DKYV_JIT_NOEXTRA").split()
    cmd = [CLANG, "-x", "hip", "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17",
           "-I" + os.path.join(ROOT, "kyverno_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
           "-DKYV_JIT_WPE=" + os.environ.get("KYV_JIT_WPE", "4")] + defs + (["-DKYV_ACCT=1"] if acct else []) + extra + \
          ["-S", f, "-o", s]
    t0 = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        print(r.stderr[-3000:])
        sys.exit(1)
    secs = time.time() - t0
    with open(s) as fh:
        rep = parse_asm(fh.read())
    report(wl, rep, "%d source bytes, compiled to assembly in %.0f s; defines: %s" % (len(src), secs, " ".join(defs + extra)),
           js, {"defines": defs + extra, "source_bytes": len(src), "asm_seconds": round(secs, 1)})


def report(wl, rep, how, js, extra):
    print("# %s: %d kernels, %s" % (wl, len(rep), how))
    print("%-24s" % "kernel" + "".join("%11s" % c for c in COLS))
    for k in sorted(rep):
        print("%-24s" % k + "".join("%11d" % rep[k][c] for c in COLS))
    if js:
        with open(js, "w") as fh:
            json.dump(dict(extra, workload=wl, kernels=rep), fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
