#!/usr/bin/env python3
"""Static instruction census of the row loop of a cost kernel, from the device assembly
(hipcc --cuda-device-only -S).  Prints per basic block of the outermost loop of the chosen kernel:
VALU / DPP / s_nop / SALU / SMEM / VMEM / LDS / branch counts.  The row loop is unrolled x5, so
"per row" = loop total / 5 (lazy D->D inner loops and the blocks only a further turn reaches are listed
separately: they run a data-dependent number of times).  Only the unrolled loop is counted, not the loops of the
one to four rows behind it.  A block that runs once per unrolled iteration (the back edge: copies into the registers
the loop header expects) is part of the loop and counts at a fifth of a row like every other block.
Register copies are counted apart, among the VALU-class as well: plain VGPR <- VGPR (v_mov_b32_e32 vA, vB: a value
that is "new or old" at a join), VGPR <- SGPR or constant (v_mov_b32_e32 vA, sB: a uniform value the compiler wants
in a vector register), and v_mov_b32_dpp (a cross-lane move that was not folded into its consumer); of the DPP
instructions, those that shift by one lane (wave_shr:1) are listed by opcode.
usage: isa_census.py kernels.s <mangled-name-substring>"""
import re
import sys
from collections import Counter

src, pat = sys.argv[1], sys.argv[2]
lines = open(src).read().split("\n")
start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and pat in l)
end = next(i for i in range(start + 1, len(lines)) if lines[i].startswith("\t.section") or lines[i].startswith(".Lfunc_end"))
body = lines[start:end]


def kind(ins):
    op = ins.split()[0]
    if op.startswith("s_nop"):
        return "nop"
    if op.startswith(("s_waitcnt", "s_barrier")):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("v_"):
        if "_dpp" in op or " row_" in ins or "wave_sh" in ins or "quad_perm" in ins:
            return "dpp"
        if op.startswith(("v_readlane", "v_readfirstlane", "v_writelane")):
            return "lane"
        return "valu"
    return "other"


# A block starts at a label or at a fall-through block the compiler left unlabelled ("; %bb.N:"); the loop note of a
# label may continue on the next line ("; =>  This Inner Loop Header: Depth=2").  A block entered only by falling
# through a s_cbranch_vccz (no lane voted for another turn) or out of an inner lazy loop is BEHIND THE VOTE: it is in
# the row loop statically, but a row that needs no further turn does not execute it.
blocks, cur, last = [], None, ""
for l in body:
    m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", l) or re.match(r"^; (%bb\.\d+):\s*(;.*)?$", l)
    if m:
        behind = m.group(1).startswith("%") and cur is not None and (last.startswith("s_cbranch_vccz") or cur[3])
        cur = [m.group(1), m.group(2) or "", Counter(), False, behind]
        blocks.append(cur)
        continue
    s = l.strip()
    if cur is not None and s.startswith(";") and "Loop" in s and not sum(cur[2].values()):
        cur[1] += " " + s
        continue
    if not s or s.startswith((";", ".", "//")) or cur is None:
        continue
    if re.match(r"^[a-z_0-9]+(\s|$)", s):
        cur[2][kind(s)] += 1
        if s.startswith("v_mov_b32_e32"):
            cur[2]["mov"] += 1  # plain register copies, counted among the VALU as well
            cur[2]["mov_vv" if re.match(r"v_mov_b32_e32\s+v\d+,\s*v\d+", s) else "mov_vs"] += 1
        if s.startswith("v_mov_b32_dpp"):
            cur[2]["mov_dpp"] += 1
        if "wave_shr:1" in s:
            cur[2]["shr:" + s.split()[0]] += 1
        last = s
        cur[3] = "Depth=2" in cur[1] or "Inner Loop" in cur[1]
# the unrolled row loop: the first loop header of depth 1 and what names it (the one to four rows behind it have
# loops of their own, which are not counted)
hdr = next(b[0] for b in blocks if "This Loop Header: Depth=1" in b[1])[2:]
tot, rare, lazy = Counter(), Counter(), Counter()
print(f"{'block':12s} {'valu':>5s} {'dpp':>4s} {'lane':>4s} {'nop':>4s} {'salu':>5s} {'smem':>5s} {'vmem':>5s} {'lds':>4s} {'br':>3s}  note")
inside = False
for name, note, c, inner, behind in blocks:
    if name[2:] == hdr:
        inside = True
    elif inside and not (f"Header={hdr} " in note + " " or f"Parent Loop {hdr} " in note or "Depth=2" in note):
        break
    if not inside or not sum(c.values()):
        continue
    tag = "INNER " if inner else "BEHIND THE VOTE " if behind else ""
    print(f"{name:12s} {c['valu']:5d} {c['dpp']:4d} {c['lane']:4d} {c['nop']:4d} {c['salu']:5d} {c['smem']:5d} {c['vmem']:5d} {c['lds']:4d} {c['branch']:3d}  {tag}{note.strip('; ')[:60]}")
    (lazy if inner else rare if behind else tot).update(c)
print("row-loop blocks (5 rows), inner lazy loops and blocks behind the vote excluded:", dict(tot))
print("behind the vote, outside the inner loops (5 rows):", dict(rare))
print("inner lazy loops (5 rows; a `while` loop's header block runs once per row and once per further turn):", dict(lazy))
v = tot["valu"] + tot["dpp"] + tot["lane"]
shr = ", ".join(f"{k[4:]} {n / 5:.1f}" for k, n in sorted(tot.items()) if k.startswith("shr:")) or "none"
print(f"copies per row: v_mov_b32_e32 VGPR<-VGPR {tot['mov_vv'] / 5:.1f}, VGPR<-SGPR/constant {tot['mov_vs'] / 5:.1f}, "
      f"v_mov_b32_dpp {tot['mov_dpp'] / 5:.1f}; wave_shr:1 per row: {shr}")
print(f"per row: VALU-class {v / 5:.1f} (+ s_nop {tot['nop'] / 5:.1f}), SALU {tot['salu'] / 5:.1f}, SMEM {tot['smem'] / 5:.1f}, VMEM {tot['vmem'] / 5:.1f}, LDS {tot['lds'] / 5:.1f}, branches {tot['branch'] / 5:.1f}; of the VALU {tot['mov'] / 5:.1f} v_mov_b32_e32")
