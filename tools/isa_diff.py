#!/usr/bin/env python3
"""tools/isa_diff.py OLD.s NEW.s — are the kernels of OLD.s (tools/isa.sh of one unit at one commit) still
in NEW.s (the same unit at another), instruction for instruction?  Either side may be several files
joined by commas (code that moved between units: OLD.s NEW_A.s,NEW_B.s); a kernel that one side holds
in two of its files counts as differing.

A kernel's stream is every instruction line between its label and its .Lfunc_end, comments dropped and
block labels renumbered in order of appearance; symbol names are left aside.  Kernels are paired by
demangled name (c++filt); where NEW.s gave a kernel template one more trailing parameter, an
instantiation with that parameter `false` pairs with the old name without it.  Prints the kernels that
differ or have no partner and a count; exit status 1 if any old kernel differs or is missing."""
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: [normalised instruction lines]} of the .amdhsa_kernel functions of an assembly file"""
    text = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M))
    out, cur, labels = {}, None, {}
    for line in text.split("\n"):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and m.group(1) in names:
            cur, labels = [], {}
            out[m.group(1)] = cur
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        code = line.split(";")[0].rstrip()
        if not code.strip():
            continue
        if re.match(r"^\.LBB\d+_\d+:", code):
            code = "L%d:" % labels.setdefault(code[:-1], len(labels))
        elif not code.startswith("\t") or code.lstrip().startswith("."):
            continue   # directives
        else:
            code = re.sub(r"\.LBB\d+_\d+", lambda q: "L%d" % labels.setdefault(q.group(0), len(labels)), code.strip())
            code = re.sub(r"_Z[\w$.]+", "SYM", code)
        cur.append(code)
    return out


def demangle(names):
    names = list(names)
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, (re.sub(r"\(.*$", "", r) for r in res)))   # the template-id; the argument list aside


def kernels_of(paths, label):
    """kernels() of comma-joined files as one dict; the mangled names found in more than one of them"""
    out, twice = {}, []
    for path in paths.split(","):
        for k, v in kernels(path).items():
            if k in out:
                twice.append(k)
            out[k] = v
    for n in sorted(demangle(twice).values()):
        print("twice   ", n, "in", label)
    return out, len(twice)


def main(old_path, new_path):
    (old, dup_old), (new, dup_new) = kernels_of(old_path, old_path), kernels_of(new_path, new_path)
    dn_old, dn_new = demangle(old), demangle(new)
    by_name = {}
    for k, n in dn_new.items():
        by_name[n] = k
        m = re.match(r"^(.*), false>$", n)
        if m:
            by_name.setdefault(m.group(1) + ">", k)
    same, bad = 0, dup_old + dup_new
    for k, n in sorted(dn_old.items(), key=lambda q: q[1]):
        partner = by_name.get(n)
        if partner is None:
            print("missing ", n)
            bad += 1
        elif old[k] != new[partner]:
            print("differs ", n, len(old[k]), "->", len(new[partner]), "instructions and labels")
            bad += 1
        else:
            same += 1
    paired = {by_name.get(n) for n in dn_old.values()}
    added = sorted(dn_new[k] for k in new if k not in paired)
    for n in added:
        print("new     ", n)
    print(f"{old_path} -> {new_path}: {same} kernels identical, {bad} differing or missing, {len(added)} new")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
