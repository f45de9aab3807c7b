#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of the library, kernel by kernel (CPU only).

    python tools/codegen_compare.py OLD.so NEW.so [--family REGEX] > table.txt

For every kernel symbol of either file: whether the metadata agrees (VGPR / AGPR / SGPR counts, LDS,
scratch, spills, workgroup size, kernarg size) and whether the instruction stream is identical (the
disassembly with addresses and encodings dropped, so a kernel that only moved inside the code object
compares equal).  Kernels matching --family are marked in the table: a refactor's report separates
the kernels it edited from those it only moved.  Exit status 1 if a symbol is missing on one side, a
kernel's metadata differs, or a kernel outside the family differs.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lrs-pnp-dip_amd"))
from test_codegen import OBJDUMP, code_objects, kernel_metadata   # noqa: E402

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".vgpr_spill_count", ".sgpr_spill_count", ".max_flat_workgroup_size", ".kernarg_segment_size",
        ".wavefront_size", ".uses_dynamic_stack")


def disassemble(co):
    with tempfile.NamedTemporaryFile(suffix=".co") as t:
        t.write(co)
        t.flush()
        return subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", t.name], capture_output=True, text=True, check=True).stdout


def instructions(path):
    """{symbol: [instruction text]} of every gfx950 code object in `path` (device functions included)."""
    out = {}
    for co in code_objects(path):
        cur = None
        pcrel = 0   # instructions left of a pc-relative address: s_getpc_b64; s_add_u32 lo, lo, LIT; s_addc_u32 hi, hi, LIT
        for line in disassemble(co).splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
            if m:
                cur = m.group(1)
                out[cur] = []
            elif cur and "//" in line:
                ins = line.split("//")[0].strip()
                # the literals of a pc-relative address move with the kernel; any other relocated literal shows as a
                # difference (none in this library)
                if ins.startswith("s_getpc_b64"):
                    pcrel = 2
                elif pcrel and ins.startswith(("s_add_u32", "s_addc_u32")):
                    ins = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "<pcrel>", ins)
                    pcrel -= 1
                else:
                    pcrel = 0
                out[cur].append(ins)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--family", default=r"k_bn_|k_reduce_bn|k_conv_bn_dir")
    a = ap.parse_args()
    fam = re.compile(a.family)
    mo, mn = kernel_metadata(a.old), kernel_metadata(a.new)
    io, inew = instructions(a.old), instructions(a.new)
    bad = 0
    print(f"# old {a.old}\n# new {a.new}\n# kernels: old {len(mo)}, new {len(mn)}; symbols with code: old {len(io)}, new {len(inew)}")
    print(f"# {'family':6} {'meta':5} {'code':9} {'instr old/new':>15}  vgpr agpr sgpr lds scratch  symbol")
    for name in sorted(set(io) | set(inew)):
        if name not in io or name not in inew:
            print(f"  {'':6} {'':5} {'MISSING':9} {'':>15}  only in {'old' if name in io else 'new'}: {name}")
            bad += 1
            continue
        infam = bool(fam.search(name))
        ko, kn = mo.get(name), mn.get(name)
        meta_eq = ko is None and kn is None or (ko is not None and kn is not None and all(ko.get(f) == kn.get(f) for f in META))
        code_eq = io[name] == inew[name]
        if not meta_eq or (not code_eq and not infam):
            bad += 1
        res = "" if kn is None else "%4d %4d %4d %6d %5d" % tuple(kn.get(f, 0) for f in META[:5])
        print(f"  {'bn' if infam else '':6} {'same' if meta_eq else 'DIFF':5} {'identical' if code_eq else 'DIFFERS':9} "
              f"{len(io[name]):7d}/{len(inew[name]):<7d}  {res}  {name}")
    print(f"# {bad} failing rows")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
