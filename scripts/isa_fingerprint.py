"""One line per kernel of a device-only assembly listing (hipcc <the build's flags> --cuda-device-only -S -I include X.hip -o X.s):

    demangled name | next_free_vgpr | next_free_sgpr | private_segment_fixed_size (scratch) | group_segment_fixed_size (static
    LDS) | instruction count | sha1 of the normalised body

The body is normalised so that it survives a rename of the kernel: comments and directives dropped, local labels renumbered.
Two builds emit the same code for a kernel exactly when the hashes agree; `--hashes` prints the sorted hashes only, for a
diff of two listings whose kernel names differ.  usage: python scripts/isa_fingerprint.py [--hashes] X.s"""
import hashlib
import re
import shutil
import subprocess
import sys

KERNEL = re.compile(r"^(_ZN5nrhip\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", re.S | re.M)
FIGURES = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return list(names)
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return [re.sub(r"^void |\(nrhip::FieldDev.*$", "", n) for n in out]  # (the argument list is the same for every variant)


def fingerprint(text):
    """-> [(mangled name, {figure: value}, instruction count, sha1)]"""
    rows = []
    for name, block in KERNEL.findall(text):
        figures = {k: int(re.search(rf"\.amdhsa_{k}\s+(\d+)", block).group(1)) for k in FIGURES}
        body = []
        for line in block.splitlines():
            line = line.split(";")[0].strip()
            if not line or (line.startswith(".") and not line.startswith(".LBB")):
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
        n_instr = sum(1 for l in body if not l.startswith(".LBB"))
        rows.append((name, figures, n_instr, hashlib.sha1("\n".join(body).encode()).hexdigest()))
    return rows


def main(argv):
    hashes_only = "--hashes" in argv
    (path,) = [a for a in argv if a != "--hashes"]
    rows = fingerprint(open(path).read())
    if hashes_only:
        print("\n".join(sorted(r[3] for r in rows)))
        return
    names = demangle([r[0] for r in rows])
    for shown, (_, fig, n, sha) in sorted(zip(names, rows)):
        print(f"{shown} vgpr={fig['next_free_vgpr']} sgpr={fig['next_free_sgpr']} scratch={fig['private_segment_fixed_size']} "
              f"lds={fig['group_segment_fixed_size']} instr={n} sha1={sha}")


if __name__ == "__main__":
    main(sys.argv[1:])
