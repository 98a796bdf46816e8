"""Scheduling check of tail_chain_kernel's weight stream (CPU only, needs hipcc): compiles lpformer_amd/csrc/tail_chain.hip
to gfx950 assembly and, for every instantiation and every weight-stage load (a ``global_load`` inlined from ``tc_load``),
prints how many ``v_mfma`` lie between the load's issue and the first ``s_waitcnt vmcnt`` that covers it -- the design
wants a k-group's MFMAs there ("one k-group ahead"), the scheduler likes to sink the load to the end of the k-group, in
front of its own wait.  Also VGPRs, scratch and LDS per instantiation.  It inspects scheduling only.

How: the build carries line tables (``-gline-tables-only``: the instruction stream is the same with and without), and the
assembler comments name the chain of inlined call sites, so a load is attributed to the ``tc_load`` call that made it: the
stage is the weight pointer of that call (``A.wE`` -> E ...), a call whose stage index depends on ``kg`` is a steady-state
load, the others are a stage's first load.  From the load the walk follows the code as a full workgroup in steady state
runs it: unconditional branches and backward conditional branches (loops) are taken, forward conditional ones are not.
vmcnt counts vector memory operations in issue order: ``vmcnt(N)`` covers a load once at most N others were issued behind
it.

``kloops()`` reads the order of a k-group back: what stands between a k-group's last ``v_mfma`` and the barrier that ends
it (``tc_kgroup_barrier``) -- the design wants nothing but the wait for the LDS counter there: the weight stream's store,
its wait for the weights and the next request run among the k-group's MFMAs --, the wait that covers stage B's first
request (``tc_load(.., A.wB, 0, ..)``), and whether a load of stage A's rows (``tc_rows_request``) is issued in front of
the first store of stage C's weights, whose wait it would lengthen (vmcnt counts in issue order).

    python tools/tail_isa.py [--json] [--kloops] [--source FILE] [--extra "-D..."]
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lpformer_amd", "csrc")
MAX_WALK = 6000

_KERNEL = re.compile(r"^(_ZN\S*tail_chain_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])E\S*):")
_LOC = re.compile(r"^\s*\.loc\s.*;\s*(.*)$")
_SITE = re.compile(r"[^\s\[\]@]*?([^/\s\[\]@]+):(\d+):\d+")
_INS = re.compile(r"^\s+([a-z][a-z0-9_]+)\b(.*)$")
_LABEL = re.compile(r"^(\.L[A-Za-z0-9_]+):")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")


def find_hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


def _run(cmd, cwd):
    p = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        raise RuntimeError("%s failed:\n%s" % (" ".join(cmd), p.stderr[-4000:]))
    return p


def source_sites(path):
    """{line: (stage letter, steady)} of every tc_load call, and the line range of tc_load itself"""
    lines = open(path).read().split("\n")
    sites, body = {}, None
    for i, text in enumerate(lines, 1):
        if body is None and re.search(r"\bvoid tc_load\(", text):
            j = i
            while not lines[j - 1].startswith("}"):
                j += 1
            body = (i, j)
            continue
        m = re.search(r"\btc_load<[^;]*?>\(\w+,\s*A\.w([A-Z])\w*,\s*([^;]*?),\s*tid\)", text)
        if m:
            sites[i] = (m.group(1), "kg" in m.group(2))
    if body is None:
        raise RuntimeError("no tc_load in %s" % path)
    return sites, body


def _body(lines, pattern, close):
    """(first, last) line of the definition whose first line matches `pattern`, closed by a line starting with `close`"""
    for i, text in enumerate(lines, 1):
        if re.search(pattern, text):
            j = i
            while not lines[j - 1].startswith(close) or j == i and "{" in text and "}" not in text:
                j += 1
            return (i, j)
    return None


def source_marks(path):
    """line ranges of tc_kgroup_barrier, tc_rows_request and tc_store, and {line: stage expression} of the tc_load calls"""
    lines = open(path).read().split("\n")
    exprs = {}
    for i, text in enumerate(lines, 1):
        m = re.search(r"\btc_load<[^;]*?>\(\w+,\s*A\.w([A-Z])\w*,\s*([^;]*?),\s*tid\)", text)
        if m:
            exprs[i] = (m.group(1), m.group(2).strip())
    one = next(i for i, t in enumerate(lines, 1) if re.search(r"\bvoid tc_kgroup_barrier\(", t))
    return {"barrier": (one, one), "rows": _body(lines, r"auto tc_rows_request = ", "    };"),
            "store": _body(lines, r"\bvoid tc_store\(", "}"), "exprs": exprs}


def _inside(loc, src_name, rng):
    return any(f == src_name and rng[0] <= l <= rng[1] for f, l in loc)


def covering_wait(k, start):
    """(index, v_mfma in between, N) of the ``s_waitcnt vmcnt(N)`` that covers the load at `start`, walked as walk() does"""
    ins, labels = k["ins"], k["labels"]
    behind, mfma, i, taken = 0, 0, start + 1, set()
    for _ in range(MAX_WALK):
        if i >= len(ins):
            return None
        op, rest, _loc = ins[i]
        if op.startswith("v_mfma"):
            mfma += 1
        elif is_vmem(op):
            behind += 1
        elif op == "s_waitcnt":
            m = _VMCNT.search(rest)
            if m and int(m.group(1)) <= behind:
                return i, mfma, int(m.group(1))
        elif op == "s_endpgm":
            return None
        elif op == "s_branch":
            i = labels[rest.strip()]
            continue
        elif op.startswith("s_cbranch"):
            tgt = labels.get(rest.strip())
            if tgt is not None and tgt <= i and (i, tgt) not in taken:
                taken.add((i, tgt))
                i = tgt
                continue
        i += 1
    return None


def kloops(source=None, extra=(), hipcc=None):
    """per kernel: {"kernel", "kgroup_ends": [[what stands between the last v_mfma and a k-group's barrier], ..],
    "b_first": [{"mfma_to_wait"}] for the loads of tc_load(.., A.wB, 0, ..), "c_first_store": {"rows_in_front": row loads
    issued in front of the first store of stage C's weights, "left_in_flight": N of the wait in front of that store}}"""
    hipcc = hipcc or find_hipcc()
    if not hipcc:
        raise RuntimeError("hipcc not found")
    src = os.path.abspath(source or os.path.join(CSRC, "tail_chain.hip"))
    name = os.path.basename(src)
    marks = source_marks(src)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "tail_chain.s")
        _run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-gline-tables-only", "-S", "-I", CSRC,
              "-I", os.path.join(ROOT, "include")] + list(extra) + [src, "-o", out], CSRC)
        kernels, _meta = parse_kernels(open(out).read())
    res = []
    for k in kernels:
        ins = k["ins"]
        ends = []
        for i, (op, _rest, loc) in enumerate(ins):
            if op != "s_barrier" or not _inside(loc, name, marks["barrier"]):
                continue
            between, j = [], i - 1
            while j >= 0 and not ins[j][0].startswith("v_mfma"):
                between.append(("%s %s" % (ins[j][0], ins[j][1].strip())).strip())
                j -= 1
            ends.append(between[::-1])
        def site(loc):      # the tc_load call that made a load: (stage, expression) or None
            for (_f0, _l0), (f1, l1) in zip(loc, loc[1:]):
                if f1 == name and l1 in marks["exprs"]:
                    return marks["exprs"][l1]
            return None
        b_first, c_loads = [], []
        for i, (op, _rest, loc) in enumerate(ins):
            if not op.startswith("global_load"):
                continue
            st = site(loc)
            if st == ("B", "0"):
                w = covering_wait(k, i)
                b_first.append({"mfma_to_wait": w[1] if w else None})
            elif st and st[0] == "C":
                c_loads.append(i)
        c_store = None
        if c_loads and marks["rows"]:
            w = covering_wait(k, c_loads[0])
            if w:
                st_i = next((j for j in range(w[0], len(ins)) if ins[j][0].startswith("ds_write") and
                             _inside(ins[j][2], name, marks["store"])), None)
                if st_i is not None:
                    rows = sum(1 for j in range(st_i) if ins[j][0].startswith("global_load") and
                               _inside(ins[j][2], name, marks["rows"]))
                    c_store = {"rows_in_front": rows, "left_in_flight": w[2]}
        nta, ntb, ntc, wm, rows_, ew = k["targs"]
        res.append({"kernel": "tail_chain_kernel<%d,%d,%d,%d,%s,%s>" % (nta, ntb, ntc, wm, "true" if rows_ else "false",
                                                                         "true" if ew else "false"),
                    "kgroup_ends": ends, "b_first": b_first, "c_first_store": c_store})
    return res


def lds_bytes(hipcc, src, shapes, extra, tmp):
    """TcShape<..>::BYTES of every instantiation, read from the host assembly of a probe that includes the source"""
    probe = os.path.join(tmp, "probe.hip")
    with open(probe, "w") as f:
        f.write('#include "%s"\n' % src)
        for s in shapes:
            f.write('extern "C" { extern const unsigned long long tc_lds_%d_%d_%d; const unsigned long long '
                    "tc_lds_%d_%d_%d = TcShape<%d, %d, %d>::BYTES; }\n" % (s + s + s))
    out = os.path.join(tmp, "probe.s")
    _run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "--cuda-host-only", "-S", "-I", CSRC, "-I",
          os.path.join(ROOT, "include")] + extra + [probe, "-o", out], CSRC)
    text = open(out).read()
    res = {}
    for s in shapes:
        m = re.search(r"^tc_lds_%d_%d_%d:\s*\n\s*\.quad\s+(\d+)" % s, text, re.M)
        res[s] = int(m.group(1)) if m else None
    return res


def parse_kernels(asm):
    """[{name, targs, ins: [(op, rest, sites)], labels: {label: index}}] and the metadata of every kernel"""
    kernels, cur, loc = [], None, ()
    for raw in asm.split("\n"):
        m = _KERNEL.match(raw)
        if m:
            cur = {"name": m.group(1), "targs": tuple(int(x) for x in m.groups()[1:]), "ins": [], "labels": {}}
            kernels.append(cur)
            loc = ()
            continue
        if cur is None:
            continue
        if raw.startswith(".Lfunc_end"):
            cur = None
            continue
        m = _LABEL.match(raw)
        if m:
            cur["labels"][m.group(1)] = len(cur["ins"])
            continue
        m = _LOC.match(raw)
        if m:   # "file:line:col @[ file:line:col @[ ... ] ]": innermost first
            loc = tuple((f, int(l)) for f, l in _SITE.findall(m.group(1)))
            continue
        m = _INS.match(raw)
        if m and not raw.lstrip().startswith("."):
            cur["ins"].append((m.group(1), m.group(2).split(";")[0], loc))
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)(?=\n\s+- |\namdhsa\.|\Z)", asm, re.S):
        blk = m.group(2)
        get = lambda k: (lambda r: int(r.group(1)) if r else None)(re.search(r"\.%s:\s+(\d+)" % k, blk))
        meta[m.group(1)] = {"vgprs": get("vgpr_count"), "sgprs": get("sgpr_count"),
                            "scratch": get("private_segment_fixed_size")}
    # (.group_segment_fixed_size and .agpr_count stand IN FRONT of .name in a kernel's block: taken from the remarks instead)
    return kernels, meta


def is_vmem(op):
    return op.startswith(("global_", "buffer_", "scratch_", "flat_")) and not op.startswith("buffer_wbl2") \
        and not op.startswith("buffer_inv")


def walk(k, start):
    """v_mfma between instruction `start` (a load) and the s_waitcnt that covers it; None if the walk finds none"""
    ins, labels = k["ins"], k["labels"]
    behind, mfma, i, taken = 0, 0, start + 1, set()
    for _ in range(MAX_WALK):
        if i >= len(ins):
            return None
        op, rest, _loc = ins[i]
        if op.startswith("v_mfma"):
            mfma += 1
        elif is_vmem(op):
            behind += 1
        elif op == "s_waitcnt":
            m = _VMCNT.search(rest)
            if m and int(m.group(1)) <= behind:
                return mfma
        elif op == "s_endpgm":
            return None
        elif op == "s_branch":
            i = labels[rest.strip()]
            continue
        elif op.startswith("s_cbranch"):
            tgt = labels.get(rest.strip())
            if tgt is not None and tgt <= i and (i, tgt) not in taken:
                taken.add((i, tgt))
                i = tgt
                continue
        i += 1
    return None


def analyse(asm, sites, body, src_name):
    kernels, meta = parse_kernels(asm)
    out = []
    for k in kernels:
        nta, ntb, ntc, wm, rows, ew = k["targs"]
        tpw = {"E": ((nta + 1) & ~1) // 2, "A": ((nta + 1) & ~1) // 2, "B": ((ntb + 1) & ~1) // 2,
               "C": ((ntc + 1) & ~1) // 2}
        per_kgroup = 1 if wm == 1 else 4    # (bf16: a k-group's four fp32 MFMAs are one instruction)
        loads = []
        for i, (op, rest, loc) in enumerate(k["ins"]):
            if not op.startswith("global_load") or len(loc) < 2:
                continue
            (f0, l0), (f1, l1) = loc[0], loc[1]
            if f0 != src_name or not (body[0] <= l0 <= body[1]) or f1 != src_name or l1 not in sites:
                continue
            stage, steady = sites[l1]
            loads.append({"line": l1, "stage": stage, "steady": steady, "need": per_kgroup * tpw[stage],
                          "mfma_to_wait": walk(k, i)})
        m = meta.get(k["name"], {})
        out.append({"kernel": "tail_chain_kernel<%d,%d,%d,%d,%s,%s>" % (nta, ntb, ntc, wm, "true" if rows else "false",
                                                                         "true" if ew else "false"),
                    "targs": [nta, ntb, ntc, wm, rows, ew], "vgprs": m.get("vgprs"), "sgprs": m.get("sgprs"),
                    "scratch": m.get("scratch"), "loads": loads})
    return out


def run(source=None, extra=(), hipcc=None):
    hipcc = hipcc or find_hipcc()
    if not hipcc:
        raise RuntimeError("hipcc not found")
    src = os.path.abspath(source or os.path.join(CSRC, "tail_chain.hip"))
    sites, body = source_sites(src)
    extra = list(extra)
    with tempfile.TemporaryDirectory() as tmp:
        s = os.path.join(tmp, "tail_chain.s")
        p = _run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-gline-tables-only", "-S",
                  "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, "-I", os.path.join(ROOT, "include")] + extra +
                 [src, "-o", s], CSRC)
        res = analyse(open(s).read(), sites, body, os.path.basename(src))
        occ = {}
        for m in re.finditer(r"Function Name: (\S+).*?Occupancy \[waves/SIMD\]: (\d+)", p.stderr, re.S):
            occ[m.group(1)] = int(m.group(2))
        shapes = sorted({tuple(k["targs"][:3]) for k in res})
        lds = lds_bytes(hipcc, src, shapes, extra, tmp)
    for k in res:
        k["lds"] = lds[tuple(k["targs"][:3])]
        mangled = "tail_chain_kernelILi%dELi%dELi%dELi%dELb%dELb%dE" % tuple(int(x) for x in k["targs"])
        k["waves_per_simd"] = next((v for n, v in occ.items() if mangled in n), None)
    return res


def report(res):
    lines = []
    for k in res:
        lines.append("%s  VGPRs %s  scratch %s B  LDS %s B  waves/SIMD %s" %
                     (k["kernel"], k["vgprs"], k["scratch"], k["lds"], k["waves_per_simd"]))
        by = {}
        for l in k["loads"]:
            by.setdefault((l["line"], l["stage"], l["steady"], l["need"]), []).append(l["mfma_to_wait"])
        for (line, stage, steady, need), v in sorted(by.items()):
            short = sum(1 for x in v if x is None or x < need) if steady else 0
            lines.append("   line %3d  stage %s  %-6s  k-group = %2d v_mfma  loads %2d  v_mfma to the covering wait: %s%s" %
                         (line, stage, "steady" if steady else "first", need, len(v),
                          " ".join("-" if x is None else str(x) for x in v),
                          "   <-- %d short" % short if short else ""))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--kloops", action="store_true", help="the order of the k-groups instead (kloops())")
    ap.add_argument("--source", default=None, help="another copy of tail_chain.hip (say, the parent commit's)")
    ap.add_argument("--extra", default="", help="further compiler flags")
    a = ap.parse_args()
    if a.kloops:
        res = kloops(a.source, a.extra.split())
        if a.json:
            print(json.dumps(res))
            return
        for k in res:
            odd = [e for e in k["kgroup_ends"] if any(not x.startswith("s_waitcnt lgkmcnt") for x in e)]
            print("%s  k-group barriers %d, with more than the LDS wait in front: %d  stage B's first request: %s  "
                  "first store of stage C's weights: %s" %
                  (k["kernel"], len(k["kgroup_ends"]), len(odd), [b["mfma_to_wait"] for b in k["b_first"]],
                   k["c_first_store"]))
            for e in odd[:4]:
                print("     " + " | ".join(e))
        return
    res = run(a.source, a.extra.split())
    print(json.dumps(res) if a.json else report(res))


if __name__ == "__main__":
    sys.exit(main())
