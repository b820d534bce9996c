#!/usr/bin/env python3
"""Compare two directories written by tools/device_listings.sh function by function.

A host-side change may move template instantiations around, which reorders the functions of a listing and renumbers their local
labels without touching a single instruction. So: cut every listing into functions ("; -- Begin function SYM" up to the next one),
drop the file-wide numbering of local labels, and compare by symbol. Whatever follows the last function (metadata, one entry per
kernel) is compared as a sorted set of lines. Exit status 0 = same functions, same bodies.

usage: tools/diff_listings.py DIR_A DIR_B
"""
import os
import re
import sys

LABEL = re.compile(r"(?:\.L|\b)(BB|func_begin|func_end|JTI|CPI)\d+")  # numbered by the function's position in the file
COUNTED = re.compile(r"\.L(post_getpc|tmp|__unnamed_)\d+")           # numbered through the whole file: renumbered per function
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")  # hash of the translation unit's text and path
BEGIN = re.compile(r"; -- Begin function (\S+)")


def functions(path):
    out, name, buf, seen = {}, None, [], {}
    for line in open(path):
        m = BEGIN.search(line)
        if m:
            head = [buf.pop()] if buf and buf[-1].lstrip().startswith(".section") else []  # the function's own section line precedes it
            if name is not None:
                out[name] = buf
            name, buf, seen = m.group(1), head, {}
        line = COUNTED.sub(lambda l: f".L{l.group(1)}#{seen.setdefault(l.group(0), len(seen))}", line)
        line = CUID.sub("__hip_cuid", LABEL.sub(lambda l: ".L" + l.group(1), line))
        buf.append(re.sub(r"\s+;", " ;", line))  # (the column of a comment follows the width of the label before it)
    body, sep, tail = "".join(buf).partition("; -- End function")
    out[name] = (body + sep).splitlines(True)
    out["<after the last function>"] = sorted(tail.splitlines(True))
    return out


def main(a, b):
    bad = 0
    for f in sorted(x for x in os.listdir(a) if x.endswith(".s")):
        fa, fb = functions(os.path.join(a, f)), functions(os.path.join(b, f))
        only = sorted(set(fa) ^ set(fb))
        differ = sorted(k for k in set(fa) & set(fb) if fa[k] != fb[k])
        print(f"{f}: {len(fa) - 1} functions, {len(only)} on one side only, {len(differ)} with different bodies")
        for k in only + differ:
            print("   ", k)
        bad += len(only) + len(differ)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
