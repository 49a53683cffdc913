#!/usr/bin/env python3
"""Compare two gfx950 listings (`make -C csrc asm` / `asm_<family>`) kernel by kernel, whatever order the kernels stand in.

    python tools/isa_compare.py OLD.s NEW.s      -> one summary line; exit status 1 if anything differs

Per kernel: the text between its entry label and its .Lfunc_end label -- every instruction, label and comment, and the .amdhsa_* directives of its kernel
descriptor, which the compiler writes there.  The compiler numbers a function's local labels (.LBB<f>_<n>, and BB<f>_<n> in its loop comments) by the function's
position in the file; that number <f>, and with it the width of the blanks that pad a label's comment to its column, is all that is
taken out before comparing, so that a kernel may move.  Every kernel of OLD must be in NEW and none may be added."""
import re
import sys


def kernels(path):
    """-> ({kernel: its lines}, {kernel: its .amdhsa_* directives})"""
    lines = open(path).read().split("\n")
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), flags=re.M))
    body, desc, cur = {}, {}, None
    for ln in lines:
        m = re.match(r"^(\S+):", ln)
        if cur is None and m and m.group(1) in names:
            assert m.group(1) not in body, m.group(1)
            cur = m.group(1)
            body[cur], desc[cur] = [], []
        elif cur is not None and ln.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            (desc if ln.strip().startswith(".amdhsa_") else body)[cur].append(re.sub(r"\s+", " ", re.sub(r"(\.L[A-Za-z_]+|\bBB)\d+_(\d+)\b", r"\1_\2", ln)))
    assert cur is None and set(body) == names, "a kernel without a body or an end label in %s" % path
    return body, desc


def main():
    old, new = sys.argv[1], sys.argv[2]
    (ob, od), (nb, nd) = kernels(old), kernels(new)
    missing, added = sorted(set(ob) - set(nb)), sorted(set(nb) - set(ob))
    differ = sorted(k for k in set(ob) & set(nb) if ob[k] != nb[k] or od[k] != nd[k])
    same = len(set(ob) & set(nb)) - len(differ)
    whole = "byte-identical" if open(old).read() == open(new).read() else "kernels in another order" if not (missing or added or differ) else "differs"
    print("kernels %d  identical %d  differing %d  missing %d  added %d  whole file: %s" % (len(ob), same, len(differ), len(missing), len(added), whole))
    for what, ks in (("differs", differ), ("missing", missing), ("added", added)):
        for k in ks:
            print("  %s: %s" % (what, k))
    return 1 if missing or added or differ else 0


if __name__ == "__main__":
    sys.exit(main())
