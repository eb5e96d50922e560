#!/usr/bin/env python3
"""Static instruction counts of a quad_sim_kernel instantiation by REGION and by CLASS, from the assembly the build leaves behind
(hcr_genesis_lr_cl_amd/csrc/obj/lg_inst_<g>.fix.s: what the assembler saw, after the DPP hazard pass).  No GPU needed.

Regions: the PROLOGUE is everything before the header of the sub-step loop (the depth-1 loop with the longest span), the LOOP is that
loop, the TAIL is everything behind the loop's last block.  Classes: scalar instructions by mnemonic, lane-to-scalar moves (v_readlane /
v_readfirstlane), plain v_mov_b32, accvgpr moves, v_cmp*, v_cndmask*, DPP forms by mnemonic, loads and stores by address form (saddr: base
in scalar registers; vaddr64: a 64-bit address in a vector register pair), s_nop, s_waitcnt.  The kernel's register and spill figures
from the code-object metadata are printed with it.

usage: tools/isa_region_stats.py [--obj DIR] [--kernel MANGLED-SUBSTRING] [--json] [--mnemonics]
  --kernel   default: the headline kernel, quad_sim_kernel<4, true, 12, 1, 3, false, true> (ILi4ELb1ELj12ELi1ELi3ELb0ELb1EE)
  --obj      default: hcr_genesis_lr_cl_amd/csrc/obj; every lg_inst_*.fix.s there is searched for the kernel
  --mnemonics  list every scalar and DPP mnemonic with its count per region (the summary has their totals only)"""
import argparse
import collections
import glob
import json
import os
import re
import sys

HEADLINE = "quad_sim_kernelILi4ELb1ELj12ELi1ELi3ELb0ELb1EE"
META = ("sgpr_count", "sgpr_spill_count", "vgpr_count", "agpr_count", "vgpr_spill_count", "private_segment_fixed_size")
SUMMARY = ("total", "valu", "scalar", "lane_to_scalar", "v_mov", "accvgpr", "v_cmp", "v_cndmask", "dpp", "load_saddr", "load_vaddr64",
           "store_saddr", "store_vaddr64", "lds", "s_load", "s_nop", "s_waitcnt")


def is_inst(line):
    t = line.strip()
    return bool(t) and not t.startswith((";", ".", "_Z")) and not t.split(";")[0].strip().endswith(":")


def find_kernel(obj, name):
    """(path, lines of the function body, metadata dict) of the first kernel whose mangled name contains `name`."""
    for path in sorted(glob.glob(os.path.join(obj, "lg_inst_*.fix.s")), key=lambda p: int(re.search(r"lg_inst_(\d+)", p).group(1))):
        lines = open(path).read().splitlines()
        start = next((i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(name) + r"\w*:", l)), None)
        if start is None:
            continue
        sym = lines[start].split(":")[0]
        end = next(i for i in range(start + 1, len(lines)) if lines[i].startswith(".Lfunc_end"))
        meta = {}
        at = next((i for i, l in enumerate(lines) if re.match(r"\s+\.name:\s+" + re.escape(sym) + r"\s*$", l)), None)
        if at is not None:
            # the fields of one kernel's metadata entry sit around its .name, between two list items ("  - .")
            # (the items of a kernel's .args list are indented deeper)
            lo = max(i for i in range(at + 1) if re.match(r"  - \.", lines[i]))
            hi = next((i for i in range(at + 1, len(lines)) if re.match(r"  - \.", lines[i])), len(lines))
            for l in lines[lo:hi]:
                m = re.match(r"\s+(?:- )?\.(\w+):\s+(\d+)\s*$", l)
                if m and m.group(1) in META:
                    meta[m.group(1)] = int(m.group(2))
        return path, sym, lines[start + 1:end], meta
    raise SystemExit(f"no kernel matching {name!r} under {obj}")


def split_regions(body):
    """-> (prologue, loop, tail) line lists: split at the longest depth-1 loop's header and behind its last block."""
    best = None
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):.*Loop Header: Depth=1", l)
        if not m:
            continue
        tag = m.group(1)[2:]
        last = max((k for k in range(i, len(body)) if re.search(r"in Loop: Header=" + tag + r"\b", body[k])), default=i)
        k = last + 1
        while k < len(body) and not body[k].startswith(".LBB"):
            k += 1
        if best is None or k - i > best[1] - best[0]:
            best = (i, k)
    if best is None:
        raise SystemExit("no depth-1 loop in the kernel")
    return body[:best[0]], body[best[0]:best[1]], body[best[1]:]


def classify(region):
    c, by = collections.Counter(), {"scalar": collections.Counter(), "dpp": collections.Counter()}
    for l in region:
        if not is_inst(l):
            continue
        text = l.split(";")[0].strip()
        mn = text.split()[0]
        ops = text[len(mn):]
        c["total"] += 1
        if mn == "s_nop":
            c["s_nop"] += 1
        elif mn == "s_waitcnt":
            c["s_waitcnt"] += 1
        elif mn.startswith("s_load") or mn.startswith("s_buffer_load"):
            c["s_load"] += 1
        elif mn.startswith("s_"):
            c["scalar"] += 1
            by["scalar"][mn] += 1
        elif mn.startswith("v_"):
            c["valu"] += 1
            if mn.endswith("_dpp") or "quad_perm" in ops or "row_" in ops:
                c["dpp"] += 1
                by["dpp"][mn] += 1
            elif mn in ("v_readlane_b32", "v_readfirstlane_b32"):
                c["lane_to_scalar"] += 1
            elif mn == "v_mov_b32_e32" or mn == "v_mov_b32":
                c["v_mov"] += 1
            elif "accvgpr" in mn:
                c["accvgpr"] += 1
            elif mn.startswith("v_cmp"):
                c["v_cmp"] += 1
            elif mn.startswith("v_cndmask"):
                c["v_cndmask"] += 1
        elif mn.startswith("ds_"):
            c["lds"] += 1
        elif mn.startswith(("global_", "flat_", "scratch_", "buffer_")):
            kind = "load" if "_load" in mn else ("store" if "_store" in mn else "atomic")
            if kind == "atomic":
                c["atomic"] += 1
                continue
            # global_load  vdst, vaddr, saddr|off      global_store vaddr, vdata, saddr|off      a v[a:b] address is the 64-bit form
            args = [a.strip() for a in ops.split(",")]
            addr = args[1] if kind == "load" else args[0]
            base = (args[2] if len(args) > 2 else "off").split()[0]
            form = "saddr" if base.startswith("s[") else ("vaddr64" if re.match(r"v\[\d+:\d+\]", addr) else "other")
            c[f"{kind}_{form}"] += 1
    return c, by


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--obj", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hcr_genesis_lr_cl_amd", "csrc", "obj"))
    ap.add_argument("--kernel", default=HEADLINE)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--mnemonics", action="store_true")
    a = ap.parse_args()
    path, sym, body, meta = find_kernel(a.obj, a.kernel)
    names = ("prologue", "loop", "tail")
    res = {n: classify(r) for n, r in zip(names, split_regions(body))}
    if a.json:
        print(json.dumps({"file": os.path.basename(path), "kernel": sym, "metadata": meta,
                          "regions": {n: {"counts": dict(res[n][0]), "scalar": dict(res[n][1]["scalar"]), "dpp": dict(res[n][1]["dpp"])} for n in names}}))
        return
    print(f"{sym}  ({os.path.basename(path)})")
    print("  " + "  ".join(f"{k} {meta[k]}" for k in META if k in meta))
    keys = list(SUMMARY) + sorted({k for n in names for k in res[n][0]} - set(SUMMARY))
    print(f"  {'class':<16}" + "".join(f"{n:>10}" for n in names))
    for k in keys:
        print(f"  {k:<16}" + "".join(f"{res[n][0].get(k, 0):>10}" for n in names))
    if a.mnemonics:
        for grp in ("scalar", "dpp"):
            print(f"  -- {grp} by mnemonic")
            for mn in sorted({m for n in names for m in res[n][1][grp]}):
                print(f"  {mn:<24}" + "".join(f"{res[n][1][grp].get(mn, 0):>10}" for n in names))


if __name__ == "__main__":
    sys.exit(main())
