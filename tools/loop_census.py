#!/usr/bin/env python3
"""Census of the whole-wave sampling loop of one k_gmm_step instantiation in a hipcc -S listing (tuning aid; the
kernel-wide mix is tools/asm_mix.py).

usage: loop_census.py file.s [mangled-name-substring]      default: k_gmm_stepILi3ELb1ELi512ELb0EEE (the flagship)

The whole-wave loop is the smallest loop of the kernel (a label and a later branch back to it) that holds an
s_setprio and a 16-byte store.  Its blocks are sorted into the record loops of the footprint test (the loops one level
below it, by the listing's own "in Loop: Header=" comments) and the rest;
a record loop is cut again at its first conditional branch: in front of it is what every record costs whatever the
lanes decide (the fetch and the first broad-phase test), behind it the rest of the broad phase and the narrow phase.
Per part: instructions, vector instructions, and the bookkeeping kinds the loop should not need (moves, selects and
integer compares of flags, LDS reads, LDS waits, scratch accesses)."""
import collections
import re
import sys

text = open(sys.argv[1]).read().split("\n")
key = sys.argv[2] if len(sys.argv) > 2 else "k_gmm_stepILi3ELb1ELi512ELb0EEE"
start = next(i for i, l in enumerate(text) if key in l and re.match(r"^\S+:\s*;", l))
end = next(i for i in range(start, len(text)) if "s_endpgm" in text[i])
label_at = {}
for i in range(start, end):
    m = re.match(r"^(\.LBB\S+):", text[i])
    if m:
        label_at[m.group(1)] = i
loops = []
for i in range(start, end):
    m = re.match(r"^\s+s_c?branch\S*\s+(\.LBB\S+)", text[i])
    if m and label_at.get(m.group(1), end) < i:
        loops.append((label_at[m.group(1)], i))


def is_instr(l):
    t = l.strip()
    return bool(t) and not t.startswith((";", ".")) and not re.match(r"^\S+:", t)


def inner_hdrs(text, lo, hi, cache={}):
    if (lo, hi) not in cache:
        hs = set()
        for i in range(lo, hi + 1):
            m = re.match(r"^\.L(BB\S+):", text[i])
            if m and any("This Inner Loop Header" in text[j] for j in range(i, min(i + 8, hi + 1))):
                hs.add(m.group(1))
        cache[(lo, hi)] = hs
    return cache[(lo, hi)]


def has(lo, hi, pat):
    return any(re.search(pat, text[i]) for i in range(lo, hi + 1) if is_instr(text[i]))


cands = [(hi - lo, lo, hi) for lo, hi in loops if has(lo, hi, r"s_setprio") and has(lo, hi, r"global_store_dwordx4")]
_, lo, hi = min(cands)
# every block of the listing names the loop it belongs to ("in Loop: Header=BB2_117 Depth=5", or the header's own
# "=> This Inner Loop Header: Depth=5"): the blocks of the record loops are those one level below the whole-wave loop
blocks = []                                    # (first line, last line, header or None) over [lo, hi]
cur, cur_hdr = lo, None
for i in range(lo, hi + 1):
    m = re.match(r"^(?:\.L(BB\S+):|; %bb\.\d+:)", text[i])
    if not m:
        continue
    if i > cur:
        blocks.append((cur, i - 1, cur_hdr))
    cur = i
    own = None
    for j in range(i, min(i + 8, hi + 1)):     # a header's comment runs over the following lines
        if j > i and is_instr(text[j]):
            break
        if "This Inner Loop Header" in text[j] and m.group(1):
            own = m.group(1)
    mm = re.search(r"in Loop: Header=(BB\S+) Depth=(\d+)", text[i])
    cur_hdr = own if own else (mm.group(1) if mm and mm.group(1) in inner_hdrs(text, lo, hi) else None)
blocks.append((cur, hi, cur_hdr))

KINDS = [("vector", r"^v_"), ("f64", r"_f64"), ("v_mov", r"^v_mov"), ("v_cndmask", r"^v_cndmask"),
         ("flag decode (v_and / int v_cmp)", r"^v_and_b32|^v_cmp_\w+_[ui](16|32)"), ("v_perm", r"^v_perm"),
         ("ds_read", r"^ds_read"), ("lgkmcnt wait", r"^s_waitcnt lgkmcnt"), ("scratch", r"^scratch_"), ("salu", r"^s_")]


def census(name, a, b):
    ops = [text[i].strip().split()[0] + (" " + text[i].strip().split(None, 1)[1] if text[i].strip().startswith("s_waitcnt") else "")
           for i in range(a, b + 1) if is_instr(text[i])]
    row = collections.OrderedDict()
    row["instructions"] = len(ops)
    for k, pat in KINDS:
        row[k] = sum(1 for o in ops if re.search(pat, o))
    print("%-46s %s" % (name, "  ".join("%s %d" % kv for kv in row.items())))
    return row


print("kernel %s: lines %d-%d; whole-wave loop: lines %d-%d (%s)" % (key, start + 1, end + 1, lo + 1, hi + 1, text[lo].split(":")[0]))


def census(name, ranges):
    ops = []
    for a, b in ranges:
        for i in range(a, b + 1):
            if is_instr(text[i]):
                t = text[i].strip()
                ops.append(t if t.startswith("s_waitcnt") else t.split()[0])
    row = collections.OrderedDict()
    row["instructions"] = len(ops)
    for k, pat in KINDS:
        row[k] = sum(1 for o in ops if re.search(pat, o))
    print("%-58s %s" % (name, "  ".join("%s %d" % kv for kv in row.items())))


census("whole-wave loop, static", [(lo, hi)])
census("  outside the record loops", [(a, b) for a, b, h in blocks if h is None])
for h in sorted(inner_hdrs(text, lo, hi), key=lambda h: label_at[".L" + h]):
    hl = label_at[".L" + h]
    cut = next(i for i in range(hl, hi + 1) if re.match(r"^\s+s_cbranch", text[i]))
    census("  record loop %s: fetch + broad phase, per record" % h, [(hl, cut)])
    census("  record loop %s: behind its first branch" % h, [(a, b) if a != hl else (cut + 1, b) for a, b, hh in blocks if hh == h and b > cut or (hh == h and a < hl)])
