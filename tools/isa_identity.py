#!/usr/bin/env python
"""Device-assembly identity of two source trees:  tools/isa_identity.py PARENT_TREE NEW_TREE [--work DIR] [--jobs N] [--reuse]

For every object of each tree's easykv_amd/_build.objects() — plus, in an older tree that still splits what it links over several
lists, its all_objects() / extra_objects() / batch_kv4_objects(), and this tree's added_objects() / later_objects() — the device side is compiled to assembly (hipcc <the build's flags>
--offload-device-only -S), the compilation-unit id (__hip_cuid_<hex>) is replaced by a constant, and the texts are compared: per
object, and per kernel symbol where an object has no partner of its name or differs (a file that was split: its kernels are looked up
in whichever object of the other tree holds them; local label numbers, which count the functions of a file, are dropped for that, in
labels and in the comments that name them).
One line per object / kernel:  name sha256(parent) sha256(new) lines verdict;  differing texts are shown line by line below their entry.
The tool only compiles and diffs text.  Host-only objects (.cpp) have no device side and are listed as such."""
import argparse
import difflib
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def build_module(tree):
    spec = importlib.util.spec_from_file_location("_build_" + hashlib.md5(tree.encode()).hexdigest(), os.path.join(tree, "easykv_amd", "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assemble(tree, work, jobs, reuse):
    """{object name: normalised device assembly, or None for a host-only object}"""
    b = build_module(tree)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(work, exist_ok=True)
    todo, out = [], {}
    for name, args in getattr(b, "all_objects", b.objects)() + getattr(b, "extra_objects", list)() + getattr(b, "batch_kv4_objects", list)() + getattr(b, "added_objects", list)() + getattr(b, "later_objects", list)():      # (objects() + added_objects() + later_objects() in this tree)
        if args[-1].endswith(".cpp"):
            out[name] = None
            continue
        path = os.path.join(work, name + ".s")
        out[name] = path
        if not (reuse and os.path.exists(path)):
            todo.append([hipcc] + b.FLAGS + ["--offload-device-only", "-S"] + args + ["-o", path])
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        list(ex.map(lambda cmd: subprocess.run(cmd, check=True, cwd=b.CSRC), todo))
    for name, path in out.items():
        if path is not None:
            with open(path) as f:
                out[name] = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", f.read()).replace(os.path.abspath(tree), "TREE")
    return out


def kernels(text):
    """{kernel symbol: its code and descriptor, local label numbers dropped}"""
    found = {}
    lines = text.splitlines()
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        name = m.group(1)
        start = next(j for j, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        body = "\n".join(lines[start:end + 1])
        body = re.sub(r"\.L(BB|func_begin|func_end|tmp)\d+", r".L\1", body)
        body = re.sub(r"\bBB\d+_", "BB_", body)      # (the same index inside comments: "; in Loop: Header=BB35_4")
        found[name] = re.sub(r"[ \t]+;", " ;", body)      # (... and the padding in front of a comment, which follows the label's width)
    return found


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()[:16]


def show_diff(a, b, limit=40):
    d = [ln for ln in difflib.unified_diff(a.splitlines(), b.splitlines(), "parent", "new", lineterm="", n=0)]
    return ["    " + ln for ln in d[:limit]] + (["    ... (%d more lines)" % (len(d) - limit)] if len(d) > limit else [])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--work", default=None)
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--reuse", action="store_true", help="keep assembly files already in --work")
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="isa_identity_")
    old = assemble(os.path.abspath(a.parent), os.path.join(work, "parent"), a.jobs, a.reuse)
    new = assemble(os.path.abspath(a.new), os.path.join(work, "new"), a.jobs, a.reuse)
    old_k = {k: (obj, t) for obj, text in old.items() if text for k, t in kernels(text).items()}
    new_k = {k: (obj, t) for obj, text in new.items() if text for k, t in kernels(text).items()}
    n_diff = 0
    print("# object sha256(parent) sha256(new) lines verdict")
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name), new.get(name)
        if o is None and n is None:
            print(f"{name} - - 0 host-only")
            continue
        if o is not None and n is not None and o == n:
            print(f"{name} {sha(o)} {sha(n)} {len(n.splitlines())} same")
            continue
        print(f"{name} {sha(o) if o else '-'} {sha(n) if n else '-'} {len((n or o).splitlines())} " +
              ("differs: by kernel" if o and n else "only in the %s tree: by kernel" % ("parent" if o else "new")))
        for k in sorted(set(kernels(o or "")) | set(kernels(n or ""))):
            ko, kn = old_k.get(k), new_k.get(k)
            if ko and kn and ko[1] == kn[1]:
                print(f"  kernel {k} {sha(ko[1])} {sha(kn[1])} {len(kn[1].splitlines())} same (parent: {ko[0]}, new: {kn[0]})")
            else:
                n_diff += 1
                print(f"  kernel {k} {sha(ko[1]) if ko else '-'} {sha(kn[1]) if kn else '-'} - " + ("DIFFERS" if ko and kn else "MISSING in the %s tree" % ("new" if ko else "parent")))
                if ko and kn:
                    print("\n".join(show_diff(ko[1], kn[1])))
        twin = [x for x, t in old.items() if t and t == n and kernels(t)]
        if twin:
            print(f"  whole text: same as the parent's {twin[0]}")
        if o and n and set(kernels(o)) == set(kernels(n)):      # same kernels, so the difference is outside them: shown line by line
            print("  whole text:")
            print("\n".join(show_diff(o, n)))
    print(f"# kernels: {len(old_k)} parent, {len(new_k)} new; {n_diff} differ or are missing")
    return 1 if n_diff or set(old_k) != set(new_k) else 0


if __name__ == "__main__":
    sys.exit(main())
