"""Is the device code of two builds the same?  For a refactor that must not change a kernel.

    python -m micromix_amd.build --force --keep-temps      # in a checkout of each commit
    python tools/compare_isa.py PARENT/micromix_amd/lib/obj BRANCH/micromix_amd/lib/obj

Per product source: the SHA-256 of its gfx950 assembly (<stem>-hip-amdgcn-amd-amdhsa-gfx950.s) in both builds after every
__hip_cuid_<hash> -- a hash of the translation unit, the one symbol that follows the source text -- is replaced by one token, and
the compiler's .ident line.  Exit status 1 if a source differs; its first differing lines are printed.
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


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
