#!/usr/bin/env python3
"""Registers, spills and LDS of the library's kernels, from the code objects of the last build (egotap_amd/build/*.o).
usage: python tools/kernel_regs.py [substring ...]      (no argument: every kernel with a spill or >= 200 VGPRs)"""
import glob, os, re, shutil, subprocess, sys, tempfile
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def code_object(obj, td):
    """The gfx950 code object bundled in host object `obj`, extracted into directory `td`; returns its path."""
    tmp_obj = os.path.join(td, "o.o")
    shutil.copy(obj, tmp_obj)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", tmp_obj], check=True, capture_output=True)      # writes <obj>.0.<target> next to it
    return glob.glob(tmp_obj + ".*gfx950")[0]


def kernel_notes(co):
    """{kernel symbol: its block of the code object's metadata note (llvm-readelf --notes)}"""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            out[name.group(1)] = ".agpr_count" + blk
    return out


def main(pats):
    for obj in sorted(glob.glob(os.path.join(os.environ.get("KREGS_DIR", os.path.join(REPO, "egotap_amd", "build")), "*.o"))):
        with tempfile.TemporaryDirectory() as td:
            notes = kernel_notes(code_object(obj, td))
        for name, blk in notes.items():
            dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
            field = lambda f: int(re.search(rf"\.{f}:\s+(\d+)", blk).group(1))
            vg, ag, sp, lds = field("vgpr_count"), field("agpr_count"), field("vgpr_spill_count"), field("group_segment_fixed_size")
            if (pats and any(p in dem for p in pats)) or (not pats and (sp > 0 or vg >= 200)):
                print(f"{os.path.basename(obj)[-8:-2]} vgpr {vg:3d} agpr {ag:3d} spill {sp:3d} lds {lds:6d}  {dem[:150]}")


if __name__ == "__main__":
    main(sys.argv[1:])
