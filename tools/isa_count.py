"""Per-kernel views of device assembly (.s from tools/isa.sh).

tools/isa_count.py FILE.s [substr...]
    instruction mix of the kernels whose name holds every substr (default: k_step_merged)
tools/isa_count.py --compare A.s [A2.s ...] -- B.s [B2.s ...]
    for every kernel name in either set of files: whether its instruction text is equal in both
    (label numbers .LBB<n>_ / .Ltmp<n> normalised, comments and directives dropped), with the
    instruction counts of both sides.  Exit status 1 if a kernel differs, is missing on one
    side, or is defined twice in one set.
"""
import re
import sys
from collections import Counter


def kernels(path):
    """[(mangled name, [instruction line, ...])] of the functions of one .s file, in file order;
    labels are kept as lines of their own so that a moved branch target shows as a difference."""
    name, body, out = None, [], []
    for line in open(path).read().split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name and line.startswith(".Lfunc_end"):
            out.append((name, body))
            name = None
            continue
        if not name:
            continue
        text = line.split(";")[0].strip()
        if text and (line.startswith("\t") and not text.startswith(".") or re.match(r"^\.L\w+:", text)):
            body.append(text)
    return out


def normalised(body):
    """Instruction text with the per-unit label numbers replaced by their order of first use."""
    seen = {}

    def sub(m):
        return seen.setdefault(m.group(0), "%s%d" % (m.group(1), len(seen)))

    return [re.sub(r"(\.LBB|\.Ltmp)\d+(?:_\d+)?", sub, " ".join(l.split())) for l in body]


def compare(a_paths, b_paths):
    sides = []
    bad = 0
    for paths in (a_paths, b_paths):
        side = {}
        for p in paths:
            txt = open(p).read()
            entry = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)$", txt, re.M))
            for n, b in kernels(p):
                if n not in entry:
                    continue
                if n in side:
                    print("DEFINED TWICE  %s (%s)" % (n, p))
                    bad += 1
                side[n] = b
        sides.append(side)
    a, b = sides
    n_eq = 0
    for n in sorted(set(a) | set(b)):
        if n not in a or n not in b:
            print("ONLY IN %s      %s" % ("A" if n in a else "B", n))
            bad += 1
            continue
        na = sum(1 for l in a[n] if not l.endswith(":"))
        nb = sum(1 for l in b[n] if not l.endswith(":"))
        if normalised(a[n]) == normalised(b[n]):
            n_eq += 1
            print("equal    %6d         %s" % (na, n))
        else:
            bad += 1
            print("DIFFERS  %6d %6d  %s" % (na, nb, n))
    print("%d kernels in A, %d in B, %d equal" % (len(a), len(b), n_eq))
    return 1 if bad else 0


def mix(path, subs):
    for n, b in kernels(path):
        if not all(s in n for s in subs):
            continue
        c = Counter(l.split()[0] for l in b if not l.endswith(":"))
        v = sum(k for i, k in c.items() if i.startswith("v_"))
        s = sum(k for i, k in c.items() if i.startswith("s_"))
        ds = sum(k for i, k in c.items() if i.startswith("ds_"))
        g = sum(k for i, k in c.items() if i.startswith(("global_", "buffer_", "flat_")))
        print(f"{n[:70]:70s} v {v:5d} s {s:5d} ds {ds:4d} mem {g:4d} div_scale {c['v_div_scale_f32']:3d} "
              f"rcp {c['v_rcp_f32']:3d} sqrt {c['v_sqrt_f32']:3d} f64 {sum(k for i, k in c.items() if i.endswith('_f64')):4d}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--compare":
        rest = sys.argv[2:]
        if "--" not in rest:
            sys.exit(__doc__)
        cut = rest.index("--")
        sys.exit(compare(rest[:cut], rest[cut + 1:]))
    mix(sys.argv[1], sys.argv[2:] or ["k_step_merged"])
