#!/usr/bin/env python3
"""Work out the decisions string of isa_path2.py from rules that name SOURCE lines, not branch numbers.
A decisions string ("nnntn...") is positional: it breaks whenever the compiler lays the blocks out differently, which is after
almost every edit.  The rules survive that: one line per conditional branch of the path,
    <file>:<text of the source line> | <opcode> | <t|n>[<t|n>...]      ## comment
The key is the source line in force at the branch (the .loc; its TEXT as it stands in stenos_amd/csrc now, blanks collapsed, 80
characters -- so lines may move --, or its number for a file that is not there and 0 for "no line") and the opcode
(s_cbranch_scc1 ...); the k-th visit of that key takes the k-th
letter, later visits the last one.  A branch without a rule stops the walk and prints its context, as isa_path2.py does; when
the compiler turns a condition round (scc0 for scc1) the opcode differs, so the rule is asked for again instead of silently
taking the wrong side.
usage: isa_decide.py <listing.s> <start line> <stop regex> <rules file> [-o decisions file]   (listing: see isa_path2.py)"""
import os
import re
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stenos_amd", "csrc")

src, start, stop_re, rules_file = sys.argv[1], int(sys.argv[2]), re.compile(sys.argv[3]), sys.argv[4]
out = sys.argv[sys.argv.index("-o") + 1] if "-o" in sys.argv else None
rules = {}
for l in open(rules_file):
    l = [f.strip() for f in l.split(" ## ")[0].rsplit(" | ", 2)]
    if len(l) == 3:
        rules[(l[0], l[1])] = l[2]
lines = open(src).read().split("\n")
files, labels, loc_at, cur_loc = {}, {}, [None] * len(lines), None
for i, l in enumerate(lines):
    m = re.match(r"^(\.LBB\d+_\d+):", l)
    if m:
        labels[m.group(1)] = i
    m = re.match(r'\s*\.file\s+(\d+)\s+"[^"]*"\s+"([^"]+)"', l)
    if m:
        files[int(m.group(1))] = m.group(2).split("/")[-1]
    m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", l)
    if m:
        cur_loc = (int(m.group(1)), int(m.group(2)))
    loc_at[i] = cur_loc


sources = {}


def source_line(name, n):
    if name not in sources:
        try:
            sources[name] = open(os.path.join(CSRC, name)).read().split("\n")
        except OSError:
            sources[name] = None
    t = sources[name]
    return " ".join(t[n - 1].split())[:80] if t and 0 < n <= len(t) else str(n)


def locname(i):
    c = loc_at[i]
    if not c:
        return "?"
    name = files.get(c[0], str(c[0]))
    return f"{name}:{source_line(name, c[1])}"


pc, steps, seen, decisions, marks = start - 1, 0, {}, [], []
while pc < len(lines) and steps < 400000:
    steps += 1
    t = lines[pc].strip()
    m = re.match(r";+\s*MARK (\S+)", t)
    if m:
        marks.append(m.group(1))
        if stop_re.search(m.group(1)) and steps > 5:
            break
        pc += 1
        continue
    if not t or t.startswith(";") or t.startswith(".") or t.endswith(":"):
        pc += 1
        continue
    op = t.split()[0]
    if op == "s_branch":
        pc = labels[t.split()[1]]
        continue
    if op.startswith("s_cbranch"):
        key = (locname(pc), op)
        if key not in rules:
            print(f"--- no rule for '{key[0]} | {key[1]}' at listing line {pc + 1} (decision #{len(decisions)}), marks so far: {' '.join(marks[-4:])}")
            for k in range(max(0, pc - 16), min(len(lines), pc + 2)):
                s = lines[k].strip()
                if s and not s.startswith("."):
                    print(f"{k + 1:6d} {locname(k):28s} {lines[k]}")
            tgt = labels[t.split()[1]]
            nxt = [locname(k) for k in range(tgt, min(tgt + 12, len(lines))) if lines[k].strip() and not lines[k].strip().startswith((".", ";"))][:3]
            fal = [locname(k) for k in range(pc + 1, min(pc + 13, len(lines))) if lines[k].strip() and not lines[k].strip().startswith((".", ";"))][:3]
            print(f"   taken -> line {tgt + 1} {nxt}; fall through -> {fal}")
            break
        n = seen.get(key, 0)
        seen[key] = n + 1
        d = rules[key][min(n, len(rules[key]) - 1)]
        decisions.append(d)
        pc = labels[t.split()[1]] if d == "t" else pc + 1
        continue
    if op == "s_endpgm":
        break
    pc += 1
s = "".join(decisions)
print("marks:", " ".join(marks))
print("decisions:", s)
if out:
    open(out, "w").write(s + "\n")
