"""Is the device code of two builds the same?  For a refactor that must not change a kernel.

    python -m micromix_amd.build --force --keep-temps      # in a checkout of each commit
    python tools/compare_isa.py PARENT/micromix_amd/lib/obj BRANCH/micromix_amd/lib/obj

Per product source: the SHA-256 of its gfx950 assembly (<stem>-hip-amdgcn-amd-amdhsa-gfx950.s) in both builds after every
__hip_cuid_<hash> -- a hash of the translation unit, the one symbol that follows the source text -- is replaced by one token, and
the compiler's .ident line.  Exit status 1 if a source differs; its first differing lines are printed.

    python tools/compare_isa.py --kernels PARENT/micromix_amd/lib/obj BRANCH/micromix_amd/lib/obj rope_append.hip [...]

For a source that gained instantiations (a new template parameter) and must keep its old ones: every kernel of the parent is looked
up in the branch by its name up to the template arguments the branch appended with the value `false`, and the two bodies -- the
instructions and labels between .globl and the end of the function, the kernel's own symbol and the function index of its local
labels replaced -- must be equal.  Exit status 1 if a kernel differs or is missing.
"""
import hashlib
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from micromix_amd import build  # noqa: E402


def normalised(objdir, src):
    path = os.path.join(objdir, src.replace(".hip", "") + "-hip-amdgcn-amd-amdhsa-gfx950.s")
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read()).splitlines()


def main(parent, branch):
    differ, idents = 0, set()
    for src in build.SOURCES:
        a, b = normalised(parent, src), normalised(branch, src)
        ha, hb = (hashlib.sha256("\n".join(t).encode()).hexdigest() for t in (a, b))
        idents.update((who, " ".join(line.split())) for who, t in (("parent", a), ("branch", b)) for line in t if line.lstrip().startswith(".ident"))
        print(f"{src:24s} {len(b):7d} lines  {'identical' if a == b else 'DIFFERENT'}\n    parent {ha}\n    branch {hb}")
        if a != b:
            differ += 1
            bad = [i for i in range(min(len(a), len(b))) if a[i] != b[i]]
            print(f"    {len(a)} lines against {len(b)}, {len(bad)} differ in place; the first:")
            for i in bad[:8]:
                print(f"    {i + 1}: - {a[i]}\n    {i + 1}: + {b[i]}")
    for who, ident in sorted(idents):
        print(f"{who}: {ident}")
    print(f"{len(build.SOURCES) - differ} of {len(build.SOURCES)} product sources: identical device assembly")
    return 1 if differ else 0


def kernel_bodies(objdir, src):
    """{kernel symbol: its instructions and labels} of a source's device assembly"""
    out, name = {}, None
    for line in normalised(objdir, src):
        m = re.match(r"\s*\.globl\s+(\S+)", line)
        if m:
            name = None if m.group(1).startswith("__hip_cuid") else m.group(1)      # the translation unit's hash is data, not a kernel
            if name:
                out[name] = []
        elif name and "-- End function" in line:
            name = None
        elif name:
            t = line.split(";")[0].rstrip()
            if t.strip() and not t.strip().startswith("."):
                out[name].append(re.sub(r"\.LBB\d+_", ".LBB_", t.replace(name, "SELF")))
    return out


def template_key(symbol):
    """the kernel's name and template arguments without trailing `false` arguments and without its parameter types"""
    m = re.search(r"(\d+[A-Za-z_]\w*?)I((?:L[a-z]\d+E)+)E", symbol)
    return (m.group(1), re.sub(r"(Lb0E)+$", "", m.group(2))) if m else (symbol, "")


def main_kernels(parent, branch, sources):
    bad = 0
    for src in sources:
        theirs = {template_key(n): b for n, b in kernel_bodies(branch, src).items() if "Lb1E" not in template_key(n)[1]}
        for name, body in sorted(kernel_bodies(parent, src).items()):
            same = theirs.get(template_key(name)) == body
            bad += not same
            print(f"{src:20s} {'.'.join(template_key(name)):48s} {len(body):6d} lines  {'identical' if same else 'DIFFERENT or missing'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main_kernels(sys.argv[2], sys.argv[3], sys.argv[4:]) if sys.argv[1] == "--kernels" else main(sys.argv[1], sys.argv[2]))
