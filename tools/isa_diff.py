#!/usr/bin/env python3
"""Compares the gfx950 device code of two builds of the library, kernel by kernel.
usage: python tools/isa_diff.py [--subset] <object dir A> <object dir B>      (the *.so.build directories of two EGOTAP_LIB=... builds)

Per symbol of each egotap_abi_part*.o, one of
  identical          the disassembly (comments stripped) is the same text
  registers renamed  the same mnemonic sequence and the same register / spill / LDS / scratch figures in the metadata
  different          anything else
and the symbols that only one side has.  Exit status 1 if anything is different or one-sided.

--subset: B's parts may hold fewer symbols than A's (a part stopped compiling what it does not launch).  Symbols only in A are reported
per part and do not fail the run; a symbol only in B, a different one and a register-renamed one do.  The kernels that no part of B
holds any more (A's union minus B's union) are printed by name."""
import glob, os, re, subprocess, sys, tempfile
from kernel_regs import LLVM, code_object, kernel_notes

FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")


def functions(co):
    """{symbol: [instruction lines]} of the code object's text, comments stripped"""
    text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        line = re.sub(r"\s*//.*$", "", line).strip()
        if cur is not None and line:
            cur.append(line)
    return out


def part(obj):
    with tempfile.TemporaryDirectory() as td:
        co = code_object(obj, td)
        funcs, notes = functions(co), kernel_notes(co)
    meta = {n: tuple(re.search(rf"\.{f}:\s+(\d+)", b).group(1) for f in FIELDS) for n, b in notes.items()}
    return funcs, meta


def demangled(sym):
    return subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()


def main(dir_a, dir_b, subset=False):
    names = sorted({os.path.basename(p) for d in (dir_a, dir_b) for p in glob.glob(os.path.join(d, "*.o"))})
    classes = ("identical", "registers renamed", "different", "only in A", "only in B")
    count = dict.fromkeys(classes, 0)
    kernels_a, kernels_b = set(), set()
    for name in names:
        pa, pb = os.path.join(dir_a, name), os.path.join(dir_b, name)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"{name}: only in {dir_a if os.path.exists(pa) else dir_b}")
            count["only in A" if os.path.exists(pa) else "only in B"] += 1
            continue
        (fa, ma), (fb, mb) = part(pa), part(pb)
        kernels_a |= set(ma)
        kernels_b |= set(mb)
        per = dict.fromkeys(classes, 0)
        for sym in sorted(set(fa) | set(fb)):
            if sym not in fa or sym not in fb:
                cls = "only in A" if sym in fa else "only in B"
                print(f"{name}: {cls}: {sym}")
            elif fa[sym] == fb[sym] and ma.get(sym) == mb.get(sym):
                cls = "identical"
            elif [l.split()[0] for l in fa[sym]] == [l.split()[0] for l in fb[sym]] and ma.get(sym) == mb.get(sym):
                cls = "registers renamed"
            else:
                cls = "different"
            if cls in ("registers renamed", "different"):
                print(f"{name}: {cls}: {demangled(sym)}")
            per[cls] += 1
        print(f"{name}: {len(fa)} | {len(fb)} symbols, {len(ma)} | {len(mb)} kernels: " + ", ".join(f"{v} {k}" for k, v in per.items()))
        for k, v in per.items():
            count[k] += v
    print("total: " + ", ".join(f"{v} {k}" for k, v in count.items()))
    print(f"distinct kernels over all parts: {len(kernels_a)} | {len(kernels_b)}")
    if subset:
        for sym in sorted(kernels_a - kernels_b):
            print(f"in no part of B: {demangled(sym)}")
        return 1 if count["different"] or count["registers renamed"] or count["only in B"] else 0
    return 1 if count["different"] or count["only in A"] or count["only in B"] else 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--subset"]
    if len(args) != 2:
        sys.exit(__doc__)
    sys.exit(main(args[0], args[1], subset="--subset" in sys.argv[1:]))
