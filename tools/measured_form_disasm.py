#!/usr/bin/env python
"""Static comparison of k_tile2's instantiations between two device assemblies of csrc/qmle_tile.hip:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -mllvm -structurizecfg-skip-uniform-regions=true \\
          --cuda-device-only -S -Iinclude -Iqml-essentials_amd/csrc qml-essentials_amd/csrc/qmle_tile.hip -o THIS.s
    python tools/measured_form_disasm.py PARENT.s THIS.s [PARENT_kernel_resources.json THIS_kernel_resources.json]

Per instantiation: instructions in the body, packed FMAs / multiplies, v_mov_b64 copies, scalar loads, lane reads and
writes (SGPR spills live in VGPR lanes), and the resource figures of the .amdhsa block; with the two
kernel_resources.json files also the occupancy the compiler reports.  Counts are static: the text of a kernel, not
what a wave executes."""
import json
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\S*k_tile2\S*):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith("\t.amdhsa_kernel") or line.startswith(".Lfunc_end"):   # (whichever closes the text first)
            out[name] = {"body": body}
            name = None
            continue
        s = line.strip()
        if s and not s.startswith((";", ".")) and not s.endswith(":"):
            body.append(s.split()[0])
    text = open(path).read()
    for name in out:
        m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", text, re.S)
        res = {}
        if m:
            for key in ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size"):
                k = re.search(r"\.amdhsa_" + key + r" (\d+)", m.group(1))
                res[key] = int(k.group(1)) if k else None
        out[name]["res"] = res
    return out


def count(body):
    c = lambda pred: sum(1 for op in body if pred(op))
    return {"instr": len(body), "valu": c(lambda o: o.startswith("v_")), "pk_fma": c(lambda o: o == "v_pk_fma_f32"),
            "pk_mul": c(lambda o: o == "v_pk_mul_f32"), "mov_b64": c(lambda o: o == "v_mov_b64"),
            "s_load": c(lambda o: o.startswith("s_load")), "lane_rw": c(lambda o: o in ("v_readlane_b32", "v_writelane_b32")),
            "scratch": c(lambda o: o.startswith("scratch_") or o.startswith("buffer_"))}


def main(argv):
    a, b = kernels(argv[1]), kernels(argv[2])
    ra = json.load(open(argv[3])) if len(argv) > 4 else {}
    rb = json.load(open(argv[4])) if len(argv) > 4 else {}
    print("k_tile2 instantiations: parent %d, this tree %d" % (len(a), len(b)))
    for name in sorted(b):
        short = re.search(r"k_tile2I(.*?)EEv", name).group(1).replace("Lb", "").replace("E", "")
        ca, cb = count(a[name]["body"]), count(b[name]["body"])
        print("k_tile2<%s>" % ",".join(short))
        for key in ca:
            print("    %-8s parent %6d   this %6d   %+d" % (key, ca[key], cb[key], cb[key] - ca[key]))
        for key in b[name]["res"]:
            print("    %-28s parent %6s   this %6s" % (key, a[name]["res"].get(key), b[name]["res"].get(key)))
        if name in ra and name in rb:
            for key in ("VGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy"):
                print("    %-28s parent %6s   this %6s" % (key, ra[name].get(key), rb[name].get(key)))


if __name__ == "__main__":
    main(sys.argv)
