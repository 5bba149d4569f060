#!/usr/bin/env python3
"""Where one sampler instantiation spills scalar registers, block by block (no GPU).

Compiles ONE instantiation of gibbs_lean.hip to gfx950 assembly with the flags of scripts/dev_lean.sh (default: config 3's
-- fp64, D = 6, M = 4, 8 chains per workgroup) and reads the assembly of one kernel.  The compiler parks scalar registers
it cannot keep in lanes of vector registers it marks "SGPR spill to VGPR lane": a v_writelane_b32 to such a register is a
spill store, a v_readlane_b32 from one a reload (a VALU instruction in front of the scalar arithmetic it feeds); every
other lane read is one of the kernel's own broadcasts.  Printed:

  * the kernel's register and spill counts (code-object notes) and the totals of the above;
  * per spill slot (register, lane): stores, reloads, the blocks that reload it, the reloads inside loops of depth >= 2,
    and the instruction that produced the value of its first store (an s_load from s[0:1] is a kernel argument);
  * per basic block: loop depth, instructions, spill stores, spill reloads, own lane reads.

    python scripts/spill_map.py                      # config 3's kernel
    python scripts/spill_map.py --schunk             # the chunked-screen build of the same shape (config 4's kind)
    DIM=3 python scripts/spill_map.py --m 8 --schunk # config 4's own instantiation
    python scripts/spill_map.py --asm some.s         # an assembly file made earlier
    python scripts/spill_map.py -- -DKDEHIP_PRELOAD_MAXB=4   # extra compiler flags behind --
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kerneldensityestimate.jl_amd", "csrc")
# (scripts/dev_lean.sh's compile line)
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", "--offload-arch=gfx950",
         "-munsafe-fp-atomics", "-mllvm", "-disable-vector-combine", "-DKDEHIP_LEAN_DEV"]

SPILL_REG = re.compile(r";\s*implicit-def:\s*\$vgpr(\d+)\s*:\s*SGPR spill to VGPR lane")
WRITELANE = re.compile(r"^\s+v_writelane_b32\s+v(\d+),\s*(\S+),\s*(\d+)")
READLANE = re.compile(r"^\s+v_readlane_b32\s+(\S+),\s*v(\d+),\s*(\S+)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
FALLTHROUGH = re.compile(r"^;\s*%bb\.(\d+):")
DEPTH = re.compile(r"Depth=(\d+)")
INSTR = re.compile(r"^\s+([a-z][a-z0-9_]+)\b")
SREG = re.compile(r"s\[(\d+):(\d+)\]|s(\d+)\b")


def compile_asm(dim, extra, out):
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc] + FLAGS + [f"-DKDEHIP_DIM={dim}"] + extra + ["--cuda-device-only", "-S", "gibbs_lean.hip", "-o", out]
    subprocess.run(cmd, cwd=CSRC, check=True, stderr=subprocess.DEVNULL)


def kernel_body(lines, pattern):
    """The lines of the one kernel whose mangled name matches, and that name."""
    starts = [(i, m.group(1)) for i, ln in enumerate(lines)
              for m in [re.match(r"^(_Z\w*gibbs_lean_kernel\w*):", ln)] if m and re.search(pattern, m.group(1))]
    if len(starts) != 1:
        names = [m.group(1) for ln in lines for m in [re.match(r"^(_Z\w*gibbs_lean_kernel\w*):", ln)] if m]
        sys.exit(f"{len(starts)} kernels match {pattern!r}; the file has:\n  " + "\n  ".join(names))
    i0, name = starts[0]
    i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[i0:i1], name


def notes(lines, name):
    """vgpr / sgpr / spill counts of the kernel from the amdhsa.kernels notes at the end of the file."""
    out = {}
    for i, ln in enumerate(lines):
        if re.match(r"\s+\.name:\s+" + re.escape(name) + r"\s*$", ln):
            j = i
            while j > 0 and not lines[j].lstrip().startswith("- ."):
                j -= 1
            k = j
            while k < len(lines) and (k == j or not lines[k].lstrip().startswith("- .")) and "..." not in lines[k][:4]:
                m = re.match(r"\s+(?:- )?\.(\w+):\s+(\d+)\s*$", lines[k])
                if m:
                    out[m.group(1)] = int(m.group(2))
                k += 1
    return out


def covers(operand, reg):
    for m in SREG.finditer(operand):
        if m.group(3) is not None:
            if int(m.group(3)) == reg:
                return True
        elif int(m.group(1)) <= reg <= int(m.group(2)):
            return True
    return False


def producer(body, at, sreg):
    """The nearest instruction above line `at` whose first operand covers scalar register `sreg`."""
    m = re.match(r"s(\d+)$", sreg)
    if not m:
        return sreg
    reg = int(m.group(1))
    for i in range(at - 1, max(at - 400, 0), -1):
        mi = INSTR.match(body[i])
        if not mi or mi.group(1).startswith(("v_writelane", "s_nop", "s_waitcnt")):
            continue
        ops = body[i].split(None, 1)[1] if len(body[i].split(None, 1)) > 1 else ""
        if covers(ops.split(",")[0], reg):
            return " ".join(body[i].split(";")[0].split())
    return "?"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--keep", help="keep the compiled assembly here")
    ap.add_argument("--m", type=int, default=4, help="densities (KDEHIP_LEAN_DEV_M)")
    ap.add_argument("--w", type=int, default=8, help="chains per workgroup (KDEHIP_LEAN_DEV_W)")
    ap.add_argument("--f32", action="store_true")
    ap.add_argument("--schunk", action="store_true", help="the chunked-screen build (last template argument true)")
    ap.add_argument("--blocks", choices=["all", "spill", "none"], default="all", help="which basic blocks to list")
    ap.add_argument("extra", nargs="*", help="extra compiler flags (behind --)")
    args = ap.parse_args()
    dim = int(os.environ.get("DIM", "6"))
    if args.asm:
        path = args.asm
    else:
        extra = list(args.extra) + [f"-DKDEHIP_LEAN_DEV_M={args.m}", f"-DKDEHIP_LEAN_DEV_W={args.w}"]
        if args.f32:
            extra += ["-DKDEHIP_LEAN_DEV_F32", "-DKDEHIP_LEAN_F32"]
        if args.m > 4:
            extra += ["-DKDEHIP_LEAN_HI"]
        path = args.keep or os.path.join(tempfile.mkdtemp(prefix="spill_map_"), "lean.s")
        compile_asm(dim, extra, path)
    with open(path) as f:
        lines = f.read().split("\n")
    t = "f" if args.f32 else "d"
    pattern = rf"gibbs_lean_kernelI{t}Li{dim}ELi{args.m}ELi{args.w}ELb0ELb{int(args.schunk or args.m == 8)}EE"
    body, name = kernel_body(lines, pattern)
    meta = notes(lines, name)
    spill_regs = {int(m.group(1)) for ln in body for m in [SPILL_REG.search(ln)] if m}

    # ---- walk the blocks ----
    Block = collections.namedtuple("Block", "label depth insts stores reloads own")
    blocks, cur = [], None
    slots = collections.defaultdict(lambda: {"stores": 0, "reloads": 0, "deep": 0, "blocks": set(), "first": None})
    nops = 0

    def close():
        if cur is not None:
            blocks.append(Block(cur["label"], cur["depth"], cur["insts"], cur["stores"], cur["reloads"], cur["own"]))

    for i, ln in enumerate(body):
        ml, mf = LABEL.match(ln), FALLTHROUGH.match(ln)
        if ml or mf or i == 0:
            close()
            # a loop header's label is followed by comment lines that name its parent loops first; "=>" marks its own depth
            md, j = DEPTH.search(ln), i
            while "=>" not in body[j] and j + 1 < len(body) and body[j + 1].startswith("      ") and \
                    body[j + 1].lstrip().startswith(";"):
                j += 1
            if "=>" in body[j]:
                md = DEPTH.search(body[j])
            label = ml.group(1) if ml else (f"%bb.{mf.group(1)}" if mf else "entry")
            cur = {"label": label, "depth": int(md.group(1)) if md else 0, "insts": 0, "stores": 0, "reloads": 0, "own": 0}
            continue
        mi = INSTR.match(ln)
        if not mi:
            continue
        cur["insts"] += 1
        if mi.group(1) == "s_nop":
            nops += 1
        mw, mr = WRITELANE.match(ln), READLANE.match(ln)
        if mw and int(mw.group(1)) in spill_regs:
            s = slots[(int(mw.group(1)), int(mw.group(3)))]
            s["stores"] += 1
            if s["first"] is None:
                s["first"] = producer(body, i, mw.group(2))
            cur["stores"] += 1
        elif mr and int(mr.group(2)) in spill_regs:
            s = slots[(int(mr.group(2)), int(mr.group(3)))]
            s["reloads"] += 1
            s["deep"] += cur["depth"] >= 2
            s["blocks"].add(cur["label"])
            cur["reloads"] += 1
        elif mr:
            cur["own"] += 1
    close()

    print(f"kernel  {name}")
    print("notes   " + "  ".join(f"{k} {meta[k]}" for k in ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count",
                                                             "group_segment_fixed_size", "private_segment_fixed_size") if k in meta))
    print(f"spill registers  {' '.join('v%d' % r for r in sorted(spill_regs)) or 'none'}")
    tot_s, tot_r = sum(b.stores for b in blocks), sum(b.reloads for b in blocks)
    print(f"blocks {len(blocks)}  instructions {sum(b.insts for b in blocks)}  s_nop {nops}")
    print(f"spill stores {tot_s}  spill reloads {tot_r} in {sum(1 for b in blocks if b.reloads)} blocks  "
          f"own v_readlane {sum(b.own for b in blocks)}")
    by_depth = collections.Counter()
    for b in blocks:
        by_depth[b.depth] += b.reloads
    print("reloads by loop depth  " + "  ".join(f"depth {d}: {n}" for d, n in sorted(by_depth.items())))

    print("\n== spill slots, most reloaded first ==")
    print("slot        stores reloads blocks  depth>=2  value of the first store")
    for (reg, lane), s in sorted(slots.items(), key=lambda kv: (-kv[1]["reloads"], kv[0])):
        print(f"v{reg}[{lane:2d}]  {s['stores']:6d} {s['reloads']:7d} {len(s['blocks']):6d} {s['deep']:9d}  {s['first']}")

    if args.blocks != "none":
        print("\n== basic blocks ==")
        print("block          depth  insts stores reloads own-readlane")
        for b in blocks:
            if args.blocks == "all" or b.stores or b.reloads:
                print(f"{b.label:14s} {b.depth:5d} {b.insts:6d} {b.stores:6d} {b.reloads:7d} {b.own:6d}")


if __name__ == "__main__":
    main()
