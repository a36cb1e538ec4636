#!/usr/bin/env python3
"""VALU / DS count of the bsw_dp8 row sweep from a gfx950 assembly listing, priced by the two issue classes of
profiles/r02_valu_issue.md.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S genarchbench_amd/csrc/bsw.hip -o bsw.s
    tools/profiling/bsw_isa_count.py bsw.s [SYM MS1 [SO]]     (default 1 1 1: the flagship instantiation, score-only form)

A listing whose bsw_dp8 has two template arguments only (before score-only became the third) is read with SO left out.
Prints, for bsw_dp8<SYM, MS1, SO>: the innermost column loop (the deepest innermost loop with the most VALU instructions) -- VALU, slow / fast
split, DS, v_mov_b32 count and the weighted cost slow x 4.22 + fast x 2.56 -- and the VALU count of the blocks of the loop around it that lie outside
every inner loop (the per-row code), with the SALU instructions (s_waitcnt, s_nop and s_branch / s_cbranch_* not counted among
them), the branches and the basic blocks of the same blocks; and, for both, the s_nop (wait states the compiler had to pad), and
the full 32-bit / 64-bit multiplies (v_mul_lo_u32, v_mul_hi_*, v_mad_u64_u32), and the v_mov_b32 of the per-row blocks.

Slow class (one instruction every ~4.2 cycles at two waves per SIMD): packed 16-bit, VOP3-only integer ops (v_perm, v_lshl_or,
v_and_or, v_max3, v_bfi, v_bfe, v_alignbit, v_add3, v_lshl_add, v_mad), 32-bit max / min, 24-bit and 32-bit multiplies, left
shifts, compares and v_cndmask, SDWA / DPP forms, and any instruction with an SGPR or literal operand.  Everything else that is a
VOP1 / VOP2 instruction on VGPRs and inline constants is fast class (2.56)."""
import re
import sys

SLOW = 4.22
FAST = 2.56
SLOW_OPS = re.compile(r"^v_(pk_|perm_|lshl_or|and_or|or3|max3|min3|med3|bfi|bfe|alignb|add3|lshl_add|add_lshl|mad_|mul_|"
                      r"max_[iu]32|min_[iu]32|lshlrev_b32|lshlrev_b64|lshrrev_b64|cmp|cndmask|add_co|sub_co|subrev_co|addc|subb|readfirstlane|readlane|"
                      r"mbcnt|xnor|cvt_|ffb|sad_|dot)")
WIDE_MUL = re.compile(r"^v_(mul_lo_[iu]32|mul_hi_[iu]32|mad_[iu]64_[iu]32)")      # full multiplies (4 cycles like the 24-bit forms, profiles/bsw_row_edges.md)
INLINE = re.compile(r"^(-?\d+|0x[0-9a-f]+)$")


def is_inline(tok):
    if not INLINE.match(tok):
        return True
    v = int(tok, 0)
    return -16 <= v <= 64


def classify(line):
    """-> 'slow' / 'fast' for a VALU instruction line"""
    op, _, rest = line.partition(" ")
    if SLOW_OPS.match(op) or "_sdwa" in op or "_dpp" in op or "sdwa" in rest or "row_" in rest:
        return "slow"
    for tok in [t.strip() for t in rest.split(",")][1:]:
        tok = tok.split()[0] if tok else tok
        if re.match(r"^(s\d+|s\[|vcc|exec|m0|ttmp)", tok):
            return "slow"
        if INLINE.match(tok) and not is_inline(tok):
            return "slow"
    return "fast"


def main():
    path = sys.argv[1]
    args = [a for a in sys.argv[2:] if a != "-v"]
    sym, ms1 = (args[0], args[1]) if len(args) > 1 else ("1", "1")
    so = args[2] if len(args) > 2 else "1"
    lines = open(path).read().split("\n")
    three = any(re.match(r"^_Z\w*bsw_dp8ILb\dELb\dELb\dEE\w*:", l) for l in lines)
    want = f"bsw_dp8ILb{sym}ELb{ms1}E" + (f"Lb{so}E" if three else "") + "E"
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + want + r"\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    # (label, depth, [instructions], inner loop header): the depth is the one the block's own annotation names ("This [Inner] Loop
    # Header: Depth=N" or "in Loop: Header=... Depth=N"; its "Parent Loop" lines name the loops around it).  The row loop is the
    # column loop's parent, whatever lies around it (the score-only kernels wrap it in the loop of the prune's second pass).
    blocks = []
    own = re.compile(r"(?:Loop Header: Depth=|in Loop: Header=\S+ Depth=)(\d+)")
    member = re.compile(r"in Loop: Header=(\S+) Depth=|Parent Loop (\S+) Depth=")      # the loop a block belongs to / a header's parents
    for l in lines[start:end]:
        s = l.strip()
        m = re.match(r"^(\.LBB\d+_\d+):|^; %bb\.(\d+):", s)
        if m:
            d = own.search(l)
            blocks.append([m.group(1) or "%bb." + m.group(2), int(d.group(1)) if d else 0, [], "Inner Loop Header" in l,
                           [a or b for a, b in member.findall(l)]])
            continue
        if not blocks or not s or s.startswith((";", ".")):
            if blocks and not blocks[-1][2]:                      # continuation lines of a block's loop annotation
                d = own.search(l)
                blocks[-1][4] += [a or b for a, b in member.findall(l)]
                if d:
                    blocks[-1][1] = int(d.group(1))
                    blocks[-1][3] = blocks[-1][3] or "Inner Loop Header" in l
            continue
        blocks[-1][2].append(s.split(";")[0].strip())
    # innermost loops: a header block and the blocks of its depth behind it up to the branch back to the header
    loops = []
    for k, b in enumerate(blocks):
        if b[3]:
            body = list(b[2])
            j = k + 1
            while not any(i.startswith("s_cbranch") and i.endswith(b[0]) for i in body) and j < len(blocks) and blocks[j][1] == b[1] and not blocks[j][3]:
                body += blocks[j][2]
                j += 1
            loops.append((b[0], body, b[1], b[4][-1] if b[4] else None))
    # the column loop: of the innermost loops at the greatest depth (inside the row loop) the one with the most VALU instructions
    label, body, cdepth, rowloop = max(loops, key=lambda lb: (lb[2], sum(i.startswith("v_") for i in lb[1])))
    valu = [i for i in body if i.startswith("v_")]
    slow = sum(classify(i) == "slow" for i in valu)
    fast = len(valu) - slow
    ds = sum(i.startswith("ds_") for i in body)
    mov = sum(i.startswith("v_mov_b32") for i in valu)
    nop = sum(i.startswith("s_nop") for i in body)
    # the row loop's own blocks: its header and the blocks annotated as its members (other loops of the same depth, such as the
    # one that writes row -1, are not per-row code)
    rowblocks = [b for b in blocks if b[1] == cdepth - 1 and not b[3] and (b[0] == "." + rowloop or (b[4] and b[4][-1] == rowloop and "Loop Header" not in b[0]))]
    row = sum(i.startswith("v_") for b in rowblocks for i in b[2])
    branch = sum(i.startswith(("s_branch", "s_cbranch")) for b in rowblocks for i in b[2])
    salu = sum(i.startswith("s_") and not i.startswith(("s_waitcnt", "s_nop", "s_branch", "s_cbranch")) for b in rowblocks for i in b[2])
    lds = sum(i.startswith("ds_") for b in rowblocks for i in b[2])
    rownop = sum(i.startswith("s_nop") for b in rowblocks for i in b[2])
    rowmov = sum(i.startswith("v_mov_b32") for b in rowblocks for i in b[2])
    rowmul = sum(bool(WIDE_MUL.match(i)) for b in rowblocks for i in b[2])
    loopmul = sum(bool(WIDE_MUL.match(i)) for i in valu)
    print(f"bsw_dp8<{sym},{ms1}{',' + so if three else ''}> column loop {label}: VALU {len(valu)} (slow {slow}, fast {fast}), DS {ds}, v_mov_b32 {mov}, "
          f"s_nop {nop}, 32/64-bit multiplies {loopmul}, "
          f"weighted {slow * SLOW + fast * FAST:.1f} cycles; per-row blocks outside the inner loops: VALU {row}, SALU {salu}, "
          f"branches {branch}, DS {lds}, basic blocks {len(rowblocks)}, s_nop {rownop}, v_mov_b32 {rowmov}, 32/64-bit multiplies {rowmul}")
    if "-v" in sys.argv:
        for i in valu:
            print(f"  {classify(i):4s} {i}")


if __name__ == "__main__":
    main()
