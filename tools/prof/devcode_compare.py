#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 device code of two source trees (no GPU needed).

    python tools/prof/devcode_compare.py OLD_TREE NEW_TREE [--drop NAME:i,j ...] [--rename OLD=NEW ...] > profiles/<record>.txt

Every .hip translation unit of fluca_amd/csrc is compiled device-only with the flags of fluca_amd/build.py of its own tree, the code object is
disassembled (llvm-objdump -d) and its metadata note read (llvm-readelf --notes).  Kernels are matched by their demangled base name plus
template arguments, within their translation unit -- a kernel whose file changed is matched by name alone and listed as MOVED; `--drop k_cg_A:3,4,5` removes the 0-based template arguments 3, 4 and 5 from the OLD tree's kernels of that name (arguments
that the new tree no longer has); `--rename 'k_x<false>=k_x'` renames one kernel of the OLD tree outright.  Compared per kernel: the instruction stream (encodings and addresses stripped: inter-function padding, pc-relative displacements) and the VGPR / AGPR / SGPR /
spill / LDS / scratch / kernarg figures.  Exit status 1 if a matched kernel differs or the new tree has a kernel the old one lacks.
"""
import argparse
import difflib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FIGURES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
           ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size")


def flags_of(tree):
    spec = importlib.util.spec_from_file_location("flbuild_" + str(abs(hash(tree))), os.path.join(tree, "fluca_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HIPCC, list(mod.FLAGS)


def split_targs(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "<(":
            depth += 1
        elif ch in ">)":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


def kernel_key(demangled, drop):
    """'void fl::k_cg_A<2, 8, true>(fl::GridP, ...)' -> 'k_cg_A<2, 8, true>'"""
    s = demangled.strip()
    s = re.sub(r"^void\s+", "", s)
    depth, end = 0, len(s)
    for i, ch in enumerate(s):   # cut the parameter list: the first '(' outside template brackets
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            end = i
            break
    s = s[:end].replace("fl::", "").replace("(anonymous namespace)::", "")
    m = re.match(r"^([\w:]+)<(.*)>$", s)
    if not m:
        return s
    base, args = m.group(1), split_targs(m.group(2))
    if base in drop:
        args = [a for i, a in enumerate(args) if i not in drop[base]]
    return f"{base}<{', '.join(args)}>" if args else base


def kernels_of(tree, drop, work):
    hipcc, flags = flags_of(tree)
    csrc = os.path.join(tree, "fluca_amd", "csrc")
    out = {}

    def one(tu):
        bundle, elf = os.path.join(work, tu + ".bundle"), os.path.join(work, tu + ".elf")
        subprocess.check_call([hipcc] + flags + ["-x", "hip", "--cuda-device-only", "-c", os.path.join(csrc, tu), "-o", bundle])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               "--input=" + bundle, "--output=" + elf])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", elf], text=True)
        figs, cur = {}, None
        for line in notes.splitlines():   # one block per kernel; .name comes after the register figures that sort before it
            t = line.strip()
            if t.startswith("- .agpr_count:") or t.startswith("- .args:"):
                cur = {}
                t = t[2:]
            if cur is None or ":" not in t:
                continue
            k, v = t.split(":", 1)
            if k in FIGURES:
                cur[k] = v.strip()
            elif k == ".name":
                figs[v.strip()] = cur
        dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", elf], text=True)
        code, sym = {}, None
        for line in dis.splitlines():
            m = re.match(r"^<(.+)>:$", line)
            if m:
                sym = m.group(1)
                code[sym] = []
            elif sym and line.startswith("\t"):
                code[sym].append(re.sub(r"\s*//.*$", "", line).strip())
        for body in code.values():
            # addresses: the padding the assembler puts between two functions belongs to neither ...
            while body and body[-1] in ("...", "s_nop 0", "s_code_end"):
                body.pop()
            # ... and the displacement from the program counter to a table in .rodata depends on where the kernel landed in the code object
            for i, ins in enumerate(body):
                if ins.startswith("s_getpc_b64"):
                    for j in (i + 1, i + 2):
                        if j < len(body) and re.match(r"s_addc?_u32 ", body[j]):
                            body[j] = re.sub(r",\s*[-\w]+$", ", <pc-relative>", body[j])
        names = sorted(figs)
        dem = subprocess.check_output(["c++filt"], input="\n".join(names) + "\n", text=True).splitlines() if names else []
        return [((tu, kernel_key(d, drop)), (code.get(mangled, []), figs[mangled])) for mangled, d in zip(names, dem)]

    with ThreadPoolExecutor(max_workers=int(os.environ.get("MAX_JOBS", "8"))) as pool:
        for found in pool.map(one, sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))):
            for key, val in found:
                assert key not in out, key
                out[key] = val
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--drop", action="append", default=[], help="NAME:i,j -- template arguments of OLD's kernels NAME that NEW no longer has")
    ap.add_argument("--rename", action="append", default=[], help="OLD=NEW -- one kernel of the OLD tree under the name NEW gives it")
    a = ap.parse_args()
    drop = {d.split(":")[0]: {int(i) for i in d.split(":")[1].split(",")} for d in a.drop}
    rename = dict(r.split("=") for r in a.rename)
    with tempfile.TemporaryDirectory() as w0, tempfile.TemporaryDirectory() as w1:
        old, new = kernels_of(os.path.abspath(a.old), drop, w0), kernels_of(os.path.abspath(a.new), {}, w1)
    old = {(tu, rename.get(name, name)): v for (tu, name), v in old.items()}
    # a kernel that moved to another translation unit is matched by its name, where that name is unambiguous
    moved, where = [], {}
    for tu, name in new:
        where.setdefault(name, []).append(tu)
    for tu, name in list(old):
        tus = where.get(name, [])
        if (tu, name) not in new and len(tus) == 1 and (tus[0], name) not in old:
            old[(tus[0], name)] = old.pop((tu, name))
            moved.append((name, tu, tus[0]))
    print("device code, old tree against new tree: gfx950, product flags, per translation unit")
    print("produced by: tools/prof/devcode_compare.py OLD NEW" + "".join(" --drop " + d for d in a.drop) + "".join(f" --rename '{r}'" for r in a.rename))
    same = [k for k in old if k in new and old[k] == new[k]]
    differ = [k for k in old if k in new and old[k] != new[k]]
    gone, added = [k for k in old if k not in new], [k for k in new if k not in old]
    print(f"kernels: old {len(old)}, new {len(new)}; identical instruction stream and resource figures {len(same)}; differing {len(differ)}; "
          f"only in old {len(gone)}; only in new {len(added)}")
    print(f"instructions compared in the identical kernels: {sum(len(old[k][0]) for k in same)}")
    for tu in sorted({k[0] for k in old} | {k[0] for k in new}):
        n_old, n_new = sum(k[0] == tu for k in old), sum(k[0] == tu for k in new)
        print(f"  {tu}: old {n_old}, new {n_new}, identical {sum(k[0] == tu for k in same)}")
    for name, tu_old, tu_new in moved:
        print(f"MOVED {name}: {tu_old} -> {tu_new} (matched by name)")
    for k in differ:
        print(f"\nDIFFERS {k[0]} {k[1]}")
        for f in FIGURES:
            if old[k][1].get(f) != new[k][1].get(f):
                print(f"  {f}: {old[k][1].get(f)} -> {new[k][1].get(f)}")
        for line in list(difflib.unified_diff(old[k][0], new[k][0], "old", "new", lineterm="", n=2))[:200]:
            print("  " + line)
    for k in gone:
        print(f"ONLY IN OLD {k[0]} {k[1]}")
    for k in added:
        print(f"ONLY IN NEW {k[0]} {k[1]}")
    return 1 if differ or added else 0


if __name__ == "__main__":
    sys.exit(main())
