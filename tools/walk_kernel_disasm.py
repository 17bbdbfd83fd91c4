#!/usr/bin/env python
"""Static check of one kernel of csrc/qmle_tile.hip against the rest of its unit, from two device assemblies

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -mllvm -structurizecfg-skip-uniform-regions=true \\
          --cuda-device-only -S -Iinclude -Iqml-essentials_amd/csrc qml-essentials_amd/csrc/qmle_tile.hip -o THIS.s
    python tools/walk_kernel_disasm.py KERNEL PARENT.s THIS.s [PARENT_kernel_resources.json THIS_kernel_resources.json]

KERNEL is a name as it appears in the mangled symbols (k_measure_walk).  Three parts:

  1. every instantiation of KERNEL in THIS.s: the resource figures of its .amdhsa block (and of kernel_resources.json),
     and its outermost loop -- the tile loop -- block by block: vector, scalar-ALU, scalar-memory and LDS instructions,
     lane reads / writes (SGPR spills live in VGPR lanes), global loads that are not LDS-DMA pieces, barriers;
  2. the same loop figures for k_tile2's two register-measuring walks, <NT,1,1,0,0,0>, whose outermost loop is the
     tile loop as well (the group and gate loops nest inside it);
  2b. the arithmetic of KERNEL's tile loop against that of k_tile2<NT,1,1,0,0,0>: per basic block the floating-point,
     lane-swap and 64-bit move instructions with their modifiers and operand kinds, register numbers left out; every
     such block of KERNEL must be, instruction for instruction, a block of k_tile2's loop;
  3. every other kernel of the unit, parent against this tree: identical text, identical but for register numbers and
     labels, or different (then the opcode counts that differ).

Counts are static: the text of the loop's blocks, both sides of every branch, each once -- not what a wave executes.
A block of k_tile2's group loop runs once per group iteration (two per tile on the headline), the blocks of
k_measure_walk's loop at most once per tile."""
import collections
import json
import re
import sys


def kernels(path):
    """name -> list of (label or None, instruction line) in text order, and name -> resources."""
    out, res, name, body = {}, {}, None, []
    text = open(path).read()
    for line in text.splitlines():
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith("\t.amdhsa_kernel") or line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        body.append(line)
    for name in out:
        m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", text, re.S)
        r = {}
        if m:
            for key in ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size"):
                k = re.search(r"\.amdhsa_" + key + r" (\d+)", m.group(1))
                r[key] = int(k.group(1)) if k else None
        res[name] = r
    return out, res


def is_instr(line):
    s = line.strip()
    return bool(s) and not s.startswith((";", ".")) and not s.endswith(":") and not re.match(r"^\.?\w+:", s)


def opcode(line):
    return line.strip().split()[0]


def klass(op):
    if op in ("v_readlane_b32", "v_writelane_b32"):
        return "lane_rw"
    if op.startswith("global_load_lds"):
        return "dma_piece"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "global_other"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op == "s_barrier":
        return "barrier"
    if op.startswith("v_"):
        return "vector"
    if op.startswith(("s_waitcnt", "s_nop", "s_cbranch", "s_branch", "s_endpgm", "s_setprio", "s_sleep")):
        return "s_control"
    if op.startswith("s_"):
        return "salu"
    return "other"


def outer_loop(body):
    """Lines of the outermost loop with the most instructions: its header block and every block tagged as inside it."""
    blocks, cur = [], None  # (label, comment, lines)
    for line in body:
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", line)
        if m:
            cur = (m.group(1), m.group(2) or "", [])
            blocks.append(cur)
        elif cur is not None and is_instr(line):
            cur[2].append(line)
    best = None
    for label, comment, _ in blocks:
        if "Loop Header: Depth=1" not in comment:
            continue
        head = label[2:]  # BBn_m
        mine = [b for b in blocks if b[0] == label or re.search(r"Header=" + re.escape(head) + r"\b", b[1])]
        # (blocks of nested loops name their own header; they sit between this loop's first and last block)
        first, last = blocks.index(mine[0]), blocks.index(mine[-1])
        mine = blocks[first:last + 1]
        n = sum(len(b[2]) for b in mine)
        if best is None or n > best[0]:
            best = (n, label, mine)
    return best


def loop_report(name, body):
    best = outer_loop(body)
    if best is None:
        print("    no loop")
        return
    n, label, blocks = best
    c = collections.Counter()
    for _, _, lines in blocks:
        for line in lines:
            c[klass(opcode(line))] += 1
    pk = sum(1 for _, _, lines in blocks for line in lines if opcode(line) in ("v_pk_fma_f32", "v_pk_mul_f32"))
    swaps = sum(1 for _, _, lines in blocks for line in lines if opcode(line).startswith("v_permlane"))
    xors = sum(1 for _, _, lines in blocks for line in lines if opcode(line) == "v_xor_b32_e32")
    print("    tile loop at %s: %d blocks, %d instructions" % (label, len(blocks), n))
    for key in ("vector", "salu", "smem", "lds", "s_control", "lane_rw", "dma_piece", "global_other", "barrier", "other"):
        print("        %-13s %5d" % (key, c[key]))
    print("        of the vector: packed fma / mul %d, lane swaps %d, v_xor %d" % (pk, swaps, xors))


ARITH = ("v_pk_fma_f32", "v_pk_mul_f32", "v_fmac_f32", "v_fma_f32", "v_mul_f32", "v_add_f32", "v_sub_f32", "v_mov_b64",
         "v_permlane16_swap_b32", "v_permlane32_swap_b32", "v_pk_add_f32")


def arith_blocks(body):
    """The arithmetic of the tile loop, block by block: per basic block the sequence of its floating-point, lane-swap
    and 64-bit move instructions with their modifiers (op_sel, neg_lo ...) and without register numbers."""
    best = outer_loop(body)
    out = []
    for _, _, lines in (best[2] if best else []):
        cur = []
        for line in lines:
            op = opcode(line)
            if op.startswith(("s_cbranch", "s_branch")):  # (a block may fall through a not-taken branch)
                if cur:
                    out.append(tuple(cur))
                cur = []
            elif op.split("_e32")[0].split("_e64")[0] in ARITH:
                cur.append(normalise(line))
        if cur:
            out.append(tuple(cur))
    return out


def arith_report(name, mine, theirs):
    """Every arithmetic block of `mine` must be, instruction for instruction, a block of `theirs`."""
    have = collections.Counter(theirs)
    pool = set(theirs)
    same = sum(1 for b in mine if b in pool)
    print("    %s: %d arithmetic blocks in the tile loop (%d instructions), %d of them found instruction for instruction"
          " (opcode, modifiers, operand kinds, order) among k_tile2's %d" %
          (name, len(mine), sum(len(b) for b in mine), same, len(have)))
    for b in mine:
        if b not in pool:
            ops = collections.Counter(x.split()[0] for x in b)
            print("        not found: a block of %d: %s" % (len(b), dict(ops)))


def normalise(line):
    s = line.strip()
    s = re.sub(r";.*$", "", s)
    s = re.sub(r"\.LBB\d+_\d+", ".LBB", s)
    s = re.sub(r"\b([svVa])\[\d+:\d+\]", r"\1[r]", s)
    s = re.sub(r"\b([sva])\d+\b", r"\1r", s)
    return s.strip()


def short(name):
    m = re.search(r"\d+(k_\w+?)I(.*?)EEv", name)
    if not m:
        m2 = re.search(r"\d+(k_\w+)", name)
        return m2.group(1) if m2 else name
    args = re.findall(r"L[bi](\d+)E", m.group(2))
    return "%s<%s>" % (m.group(1), ",".join(args))


def main(argv):
    kernel = argv[1]
    a, ra = kernels(argv[2])
    b, rb = kernels(argv[3])
    ja = json.load(open(argv[4])) if len(argv) > 5 else {}
    jb = json.load(open(argv[5])) if len(argv) > 5 else {}
    print("1. %s in this tree" % kernel)
    for name in sorted(n for n in b if kernel in n):
        print(short(name))
        for key, v in rb[name].items():
            print("    %-28s %6s" % (key, v))
        for key in ("VGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy"):
            if name in jb:
                print("    %-28s %6s" % (key, jb[name].get(key)))
        ins = [line for line in b[name] if is_instr(line)]
        print("    instructions %d, lane reads / writes in the whole kernel %d" %
              (len(ins), sum(1 for line in ins if klass(opcode(line)) == "lane_rw")))
        loop_report(name, b[name])
    print("2. k_tile2's register-measuring walks in this tree")
    for name in sorted(b):
        if "k_tile2" in name and short(name) in ("k_tile2<0,1,1,0,0,0>", "k_tile2<1,1,1,0,0,0>"):
            print(short(name))
            loop_report(name, b[name])
    print("2b. the arithmetic of %s's tile loop against k_tile2<NT,1,1,0,0,0>'s, block by block" % kernel)
    ref = {short(n): arith_blocks(b[n]) for n in b if "k_tile2" in n and short(n) in ("k_tile2<0,1,1,0,0,0>", "k_tile2<1,1,1,0,0,0>")}
    for name in sorted(n for n in b if kernel in n):
        nt = re.search(r"<(\d)", short(name)).group(1)
        arith_report(short(name), arith_blocks(b[name]), ref.get("k_tile2<%s,1,1,0,0,0>" % nt, []))
    print("3. every other kernel of the unit, parent | this tree")
    for name in sorted(set(a) | set(b)):
        if kernel in name:
            continue
        if name not in a or name not in b:
            print("    %-40s only in %s" % (short(name), "parent" if name in a else "this tree"))
            continue
        ia, ib = [l for l in a[name] if is_instr(l)], [l for l in b[name] if is_instr(l)]
        if [l.strip() for l in ia] == [l.strip() for l in ib]:
            verdict = "identical text"
        elif [normalise(l) for l in ia] == [normalise(l) for l in ib]:
            verdict = "identical but for register numbers and labels"
        else:
            ca, cb = collections.Counter(opcode(l) for l in ia), collections.Counter(opcode(l) for l in ib)
            diff = {k: cb[k] - ca[k] for k in set(ca) | set(cb) if ca[k] != cb[k]}
            verdict = "DIFFERENT: %d | %d instructions, opcode counts %s" % (len(ia), len(ib), diff or "equal (order differs)")
        res = ""
        if name in ja and name in jb:
            keys = ("VGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy")
            same = all(ja[name].get(k) == jb[name].get(k) for k in keys)
            res = "; resources " + ("equal" if same else " ".join("%s %s|%s" % (k, ja[name].get(k), jb[name].get(k))
                                                                  for k in keys if ja[name].get(k) != jb[name].get(k)))
        print("    %-40s %s%s" % (short(name), verdict, res))


if __name__ == "__main__":
    main(sys.argv)
