#!/usr/bin/env python3
"""Compare the device assembly of two trees, kernel by kernel.

    tools/isa_same.py OLD_DIR NEW_DIR [--allow-new REGEX]

Each directory holds the `hipcc -S --cuda-device-only` output (*.s) of every
Makefile source of one tree, built with the Makefile's flags.  For every
kernel symbol (.amdhsa_kernel) the instruction text between its entry label
and its end label is compared -- comment lines dropped, the function index of
local labels normalised (.LBB<n>_ -> .LBB_) -- together with its .amdhsa_
resource lines.  Kernels may move between files.  Exit status 0 iff the two
sets of kernels are the same (but for new kernels matching --allow-new) and
every kernel compares equal.
"""
import argparse
import glob
import os
import re
import sys


def kernels(d):
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        lines = open(path).read().split("\n")
        names = [l.split()[1] for l in lines
                 if l.strip().startswith(".amdhsa_kernel ")]
        for name in names:
            start = next(i for i, l in enumerate(lines)
                         if l.startswith(name + ":"))
            # the code ends where the kernel descriptor's section (or, without
            # one in between, the end label) begins
            end = next(i for i in range(start, len(lines))
                       if lines[i].startswith(".Lfunc_end") or
                       lines[i].strip().startswith(".section"))
            body = []
            for l in lines[start + 1:end]:
                t = l.split(";")[0].rstrip()
                if t.strip():
                    body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
            k0 = next(i for i, l in enumerate(lines)
                      if l.strip() == ".amdhsa_kernel " + name)
            k1 = next(i for i in range(k0, len(lines))
                      if lines[i].strip() == ".end_amdhsa_kernel")
            res = [l.strip() for l in lines[k0 + 1:k1]]
            if name in out:  # internal linkage: the same symbol in two files
                sys.exit("%s: kernel %s is in %s and %s; compare such files "
                         "one by one" % (d, name, out[name][0],
                                         os.path.basename(path)))
            out[name] = (os.path.basename(path), body, res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--allow-new", default=None,
                    help="regex of kernel symbols only the new tree may have")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    gone = sorted(set(old) - set(new))
    added = sorted(set(new) - set(old))
    allowed = [n for n in added
               if a.allow_new and re.search(a.allow_new, n)]
    added = [n for n in added if n not in allowed]
    diff = []
    for n in sorted(set(old) & set(new)):
        what = [w for w, i in (("instructions", 1), ("resources", 2))
                if old[n][i] != new[n][i]]
        if what:
            diff.append("%s (%s -> %s): %s" % (n, old[n][0], new[n][0],
                                               ", ".join(what)))
    moved = sum(1 for n in set(old) & set(new) if old[n][0] != new[n][0])
    print("kernels: old %d, new %d, compared %d (%d in another file)" %
          (len(old), len(new), len(set(old) & set(new)), moved))
    print("only in new, allowed: %d %s" % (len(allowed), " ".join(allowed)))
    print("only in old: %d %s" % (len(gone), " ".join(gone)))
    print("only in new: %d %s" % (len(added), " ".join(added)))
    print("different: %d" % len(diff))
    for l in diff:
        print("  " + l)
    return 1 if gone or added or diff else 0


if __name__ == "__main__":
    sys.exit(main())
