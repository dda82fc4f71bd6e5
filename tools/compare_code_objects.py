"""Whether two builds of a HIP shared library carry the same device code, kernel by kernel.

    python tools/compare_code_objects.py A.so B.so

For every gfx950 code object of each library: kernel symbol -> (hash of the kernel's disassembled instruction text with addresses and
encodings stripped, the kernel's register / LDS / scratch figures from the code-object metadata).  A host-only change (planners, launch
switches) must leave every pair equal: the evidence that it cannot have moved a kernel's speed.  Prints the kernels that exist on one
side only and those that differ, then one summary line; exit code 1 if there are any."""
import hashlib
import re
import subprocess
import sys

from check_packed_forms import OBJDUMP, code_objects, disassembly

READELF = OBJDUMP.replace("llvm-objdump", "llvm-readelf")
FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
           "sgpr_spill_count", "max_flat_workgroup_size", "kernarg_segment_size", "uses_dynamic_stack")


def metadata(obj):
    """{kernel symbol: {figure: value}} from the amdhsa.kernels list of the object's metadata note."""
    notes = subprocess.run([READELF, "--notes", obj], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode(errors="replace")
    out, cur = {}, {}
    for ln in notes.splitlines():
        m = re.match(r"^\s*(- )?\.(\w+):\s*(.*?)\s*$", ln)
        if not m:
            continue
        dash, key, val = m.groups()
        if dash and re.match(r"^  - ", ln):   # a new entry of a top-level list (amdhsa.kernels)
            cur = {}
        if key in FIGURES:
            cur[key] = val
        elif key == "name" and re.match(r"^    \.name:", ln):
            out[val.strip("'\"")] = cur
    return out


def kernels(lib_path):
    """{symbol: (instruction-text hash, figures)} over every code object of the library."""
    out = {}
    with code_objects(lib_path) as objs:
        for o in objs:
            meta = metadata(o)
            text = {}
            for sym, ln in disassembly(o):
                ins = ln.split("//")[0].strip()   # "<instruction> // <address>: <encoding>"
                if ins and sym != "?":   # ("?": the lines in front of the first symbol)
                    text.setdefault(sym, hashlib.sha256()).update((ins + "\n").encode())
            if set(meta) - set(text):
                raise RuntimeError("kernels of %s with metadata and no code: %s" % (lib_path, sorted(set(meta) - set(text))))
            for sym, h in text.items():   # (a symbol without metadata is a device function that was not inlined: compared by its code)
                entry = (h.hexdigest(), tuple(sorted(meta.get(sym, {}).items())))
                if out.setdefault(sym, entry) != entry:
                    raise RuntimeError("symbol %s is in two code objects of %s with different code" % (sym, lib_path))
    return out


def main():
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    for k in only_a:
        print("only in %s: %s" % (sys.argv[1], k))
    for k in only_b:
        print("only in %s: %s" % (sys.argv[2], k))
    for k in differ:
        what = ("code" if a[k][0] != b[k][0] else "") + (" figures %s -> %s" % (dict(a[k][1]), dict(b[k][1])) if a[k][1] != b[k][1] else "")
        print("differs (%s): %s" % (what.strip(), k))
    print("%d kernels in %s, %d in %s: %d only in the first, %d only in the second, %d different" %
          (len(a), sys.argv[1], len(b), sys.argv[2], len(only_a), len(only_b), len(differ)))
    return 1 if only_a or only_b or differ else 0


if __name__ == "__main__":
    sys.exit(main())
