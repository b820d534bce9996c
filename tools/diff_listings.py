#!/usr/bin/env python3
"""Compare two directories written by tools/device_listings.sh function by function.

A change may move template instantiations around, or kernels from one translation unit to another, which reorders the functions of a
listing (or changes the listing they are in) and renumbers their local labels without touching a single instruction. So: cut every
listing into functions ("; -- Begin function SYM" up to the next one, the kernel descriptor and resource lines that follow the body
included), drop the file-wide numbering of local labels, and compare by symbol over ALL the listings of a directory: a function is
reported once, wherever it lives. Whatever follows the last function of a listing (variables in LDS, constants, then the metadata, one
entry per kernel) is compared as one sorted set per directory: each metadata entry one element, every other line one element.
Exit status 0 = same functions, same bodies.

usage: tools/diff_listings.py DIR_A DIR_B
"""
import os
import re
import sys

LABEL = re.compile(r"(?:\.L|\b)(BB|func_begin|func_end|JTI|CPI)\d+")  # numbered by the function's position in the file
COUNTED = re.compile(r"\.L(post_getpc|tmp|__unnamed_)\d+")           # numbered through the whole file: renumbered per function
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")  # hash of the translation unit's text and path
# the listing's own bookkeeping of .text between two functions: back to the plain section, the padding that ends the code
FILE_TEXT = re.compile(r"\t(\.text|\.p2alignl 6, 3212836864|\.fill 256, 4, 3212836864)$")
BEGIN = re.compile(r"; -- Begin function (\S+)")


def functions(path):
    out, name, buf, seen = {}, None, [], {}
    for line in open(path):
        m = BEGIN.search(line)
        if m:
            head = [buf.pop()] if buf and buf[-1].lstrip().startswith(".section") else []  # the function's own section line precedes it
            while buf and FILE_TEXT.match(buf[-1]):
                buf.pop()
            if name is not None:
                out[name] = buf
            name, buf, seen = m.group(1), head, {}
        line = COUNTED.sub(lambda l: f".L{l.group(1)}#{seen.setdefault(l.group(0), len(seen))}", line)
        line = CUID.sub("__hip_cuid", LABEL.sub(lambda l: ".L" + l.group(1), line))
        buf.append(re.sub(r"\s+;", " ;", line))  # (the column of a comment follows the width of the label before it)
    body, _, tail = "".join(buf).partition("\t.section\t.AMDGPU.gpr_maximums")  # (the last function's resource lines end here)
    out[name] = body.splitlines(True)
    while out[name] and FILE_TEXT.match(out[name][-1]):
        out[name].pop()
    return out, tail


def after_last_function(tail):
    """The elements of a listing's tail: the entries of amdhsa.kernels as blocks, every other line by itself."""
    out, entry = set(), None
    for line in tail.splitlines(True):
        if line.startswith("  - ") or not line.startswith("    "):  # an entry starts / ends
            if entry is not None:
                out.add(entry)
            entry = line if line.startswith("  - .") else None
            if entry is None:
                out.add(line)
        elif entry is not None:
            entry += line
        else:
            out.add(line)
    return out


def directory(d):
    """symbol -> the set of its bodies (one, unless two listings disagree), and the set of tail elements"""
    fns, tails, per_file = {}, set(), []
    for f in sorted(x for x in os.listdir(d) if x.endswith(".s")):
        ff, tail = functions(os.path.join(d, f))
        for k, body in ff.items():
            fns.setdefault(k, set()).add("".join(body))
        tails |= after_last_function(tail)
        per_file.append(f"{f[:-2]} {len(ff)}")
    return fns, tails, per_file


def main(a, b):
    (fa, ta, pa), (fb, tb, pb) = directory(a), directory(b)
    only = sorted(set(fa) ^ set(fb))
    differ = sorted(k for k in set(fa) & set(fb) if fa[k] != fb[k])
    tail = sorted(ta ^ tb)
    print(f"{a}: {len(fa)} functions ({', '.join(pa)})")
    print(f"{b}: {len(fb)} functions ({', '.join(pb)})")
    print(f"{len(only)} on one side only, {len(differ)} with different bodies, {len(tail)} differences after the last functions")
    for k in only + differ:
        print("   ", k)
    for k in tail:  # (a metadata entry by its symbol line)
        print("   ", "A:" if k in ta else "B:", next((l for l in k.splitlines() if ".symbol:" in l), k).strip())
    return 1 if only or differ or tail else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
