#!/usr/bin/env python
"""Compare the gfx950 code of two HIP object files kernel by kernel: disassembly text and the per-kernel fields of the code-object
notes (registers, LDS, scratch, spills).  Prints the symbols on one side only and the ones that differ; exit status 1 if any differ.
Usage: isa_compare.py OLD.o NEW.o"""
import glob, os, re, shutil, subprocess, sys, tempfile
LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
          "sgpr_spill_count", "kernarg_segment_size", "max_flat_workgroup_size", "uses_dynamic_stack")


def device_code(obj):
    """({symbol: disassembly}, {kernel: notes fields}) of the gfx950 code object bundled in obj"""
    d = tempfile.mkdtemp()
    try:
        tmp = shutil.copy(obj, os.path.join(d, "x.o"))
        subprocess.check_call([LLVM + "/llvm-objdump", "--offloading", tmp], stdout=subprocess.DEVNULL, cwd=d)
        found = glob.glob(tmp + ".*amdgcn*")
        if not found: return {}, {}                     # no device code in this file
        dis = subprocess.check_output([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", found[0]]).decode()
        notes = subprocess.check_output([LLVM + "/llvm-readelf", "--notes", found[0]]).decode()
    finally:
        shutil.rmtree(d)
    text, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", line)
        if m: name = m.group(1); text[name] = []
        elif name and line.strip() not in ("", "..."): text[name].append(re.sub(r"\s*//.*$", "", line).strip())
    meta = {}
    for blk in re.split(r"^\s+- \.agpr_count:", notes, flags=re.M)[1:]:
        blk = ".agpr_count:" + blk
        f = {k: m.group(1) for k in FIELDS for m in [re.search(r"^\s+\.%s:\s+(\S+)" % k, blk, re.M)] if m}
        meta[re.search(r"^\s+\.name:\s+(\S+)", blk, re.M).group(1)] = f
    return {k: "\n".join(v) for k, v in text.items()}, meta


def compare(what, old, new):
    for side, a, b in (("OLD", old, new), ("NEW", new, old)):
        for k in sorted(set(a) - set(b)): print("%s only in %s: %s" % (what, side, k))
    diff = sorted(k for k in set(old) & set(new) if old[k] != new[k])
    for k in diff: print("%s DIFFERS: %s" % (what, k))
    print("%s: %d common, %d identical, %d differ" % (what, len(set(old) & set(new)), len(set(old) & set(new)) - len(diff), len(diff)))
    return len(diff)


if __name__ == "__main__":
    (t0, m0), (t1, m1) = device_code(sys.argv[1]), device_code(sys.argv[2])
    sys.exit(1 if compare("disassembly", t0, t1) + compare("notes", m0, m1) else 0)
