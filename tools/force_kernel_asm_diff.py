"""Compares the gfx950 instruction streams of the kernels of stencil.hip and vorticity.hip between two builds (DESIGN.md 3.25:
the instantiations the single-item step runs must not change when the force kernels gain their per-item form). No GPU needed.

  mkdir A B
  (cd A && hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -save-temps -c <parent>/fluidnet_amd/csrc/stencil.hip ...vorticity.hip)
  (cd B && the same from this tree)
  python tools/force_kernel_asm_diff.py A B [--show]

Per kernel of A: the lines of its body in the device assembly (directives, comments and blank lines dropped, basic-block labels
renumbered) against the kernel of B with the same name and IS3D argument whose table pack is empty; the instantiations with a
table are listed as new. Exit status 1 if a stream differs or a kernel is missing."""
import difflib
import re
import sys

FILES = ("stencil", "vorticity")
SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        t = line.split(";")[0].rstrip()
        if not t.strip() or (t.strip().startswith(".") and not re.match(r"^\.LBB", t.strip())):
            continue
        out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def key(name):
    """k_name<IS3D> of a templated force kernel without a table; None for one with a table; the symbol itself otherwise"""
    m = re.match(r"_ZN3tfl\d+(k_[a-z_0-9]+?)I(Lb[01]E)(J.*?E)?EEv", name)
    if not m:
        return name
    if m.group(3) and m.group(3) != "JE":
        return None
    return "%s<%s>" % (m.group(1), m.group(2)[2])


def main():
    a_dir, b_dir, show = sys.argv[1], sys.argv[2], "--show" in sys.argv
    bad = 0
    for f in FILES:
        a = {key(k): v for k, v in kernels("%s/%s%s" % (a_dir, f, SUFFIX)).items()}
        b_all = kernels("%s/%s%s" % (b_dir, f, SUFFIX))
        b = {key(k): v for k, v in b_all.items() if key(k)}
        for k in sorted(a):
            if k not in b:
                print(f, "MISSING", k)
                bad += 1
                continue
            same = a[k] == b[k]
            bad += not same
            print(f, "same" if same else "DIFF", len(a[k]), len(b[k]), k)
            if show and not same:
                print("\n".join(list(difflib.unified_diff(a[k], b[k], lineterm="", n=1))[:80]))
        print(f, "new:", sorted(k for k in b_all if not key(k) or key(k) not in a))
    print("differing:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
