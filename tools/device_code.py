"""CPU-only: the gfx950 instruction text of every kernel of csrc files, to compare two source trees kernel by kernel (the
acceptance test of a refactor that must not change the device code; profiles/advect_vel3_unify.md, profiles/scope_args_device_code.txt).

  device_code.py dump <csrc dir> <out dir> [file.hip ...]   compile each file as the Makefile does, in both flavours (build = product,
                                                            build_exp = -DTFL_EXPERIMENTS), .hip_fatbin -> clang-offload-bundler
                                                            --unbundle -> llvm-objdump -d; one <out>/<flavour>/<file>/<kernel>.s per
                                                            symbol, addresses and encodings stripped
  device_code.py cmp <out dir A> <out dir B> [--diff]       one line per kernel: identical, or how it differs; --diff adds the diff with
                                                            register numbers and branch distances masked (what is left of a diff once
                                                            a renumbering of registers no longer hides it)

Symbols are named by their demangled kernel name without namespaces, so a kernel that only moved to another namespace keeps its
file; pass --rename OLD=NEW (regular expression, on the full demangled name) to `dump` for kernels whose name changed."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

LLVM = "/opt/rocm/llvm/bin/"


def makefile_flags(csrc, obj):
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^FLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", re.search(r"^ARCH \?= (\S+)", mk, re.M).group(1)).split()
    for m in re.finditer(r"^(\$\(HERE\)build/.*): FLAGS \+= (.*)$", mk, re.M):
        if "$(HERE)build/" + obj in m.group(1).split():
            flags += m.group(2).split()
    return flags


def dump_one(job):
    csrc, out, flavour, f, renames = job
    d = os.path.join(out, flavour, f)
    os.makedirs(d, exist_ok=True)
    o = os.path.join(d, "_.o")
    flags = makefile_flags(csrc, os.path.splitext(f)[0] + ".o") + (["-DTFL_EXPERIMENTS"] if flavour == "build_exp" else [])
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + flags + ["-x", "hip", "-c", "-o", o, f], cwd=csrc)
    if ".hip_fatbin" not in subprocess.run([LLVM + "llvm-readelf", "-S", o], capture_output=True, text=True, check=True).stdout:
        os.remove(o)
        return "%s/%s: no device code" % (flavour, f)       # (a host-only .cpp of SRCS)
    subprocess.check_call([LLVM + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + o + ".fb", o])
    subprocess.check_call([LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + o + ".fb",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + o + ".co"])
    text = subprocess.run([LLVM + "llvm-objdump", "-d", o + ".co"], capture_output=True, text=True, check=True).stdout
    cur, body = None, {}
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            for old, new in renames:
                name = re.sub(old, new, name)
            name = re.sub(r"\(.*", "", re.sub(r"^void |\(anonymous namespace\)::|\b\w+::", "", name))
            cur = body.setdefault(name, [])
        elif cur is not None and line.strip() and line.strip() != "...":      # ("..." = the zero padding behind the last symbol)
            cur.append(re.sub(r"\s*<[^>]*>$", "", line.split("//")[0].rstrip()).strip())
    for o_ in (o, o + ".fb", o + ".co"):
        os.remove(o_)
    for name, b in body.items():
        open(os.path.join(d, re.sub(r"\W+", "_", name).strip("_") + ".s"), "w").write("\n".join(b) + "\n")
    return "%s/%s: %d symbols" % (flavour, f, len(body))


def masked_diff(a, b, label):
    """`diff -U1` of two kernels with register numbers and branch distances masked"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        for n, path in (("a", a), ("b", b)):
            t = re.sub(r"\b([vs])(\d+|\[\d+:\d+\])", r"\1N", open(path).read())
            open(os.path.join(tmp, n), "w").write(re.sub(r"\b(s_c?branch\w*) \d+", r"\1 L", t))
        out = subprocess.run(["diff", "-U1", "--label", "a/" + label, "--label", "b/" + label, "a", "b"], cwd=tmp, capture_output=True, text=True).stdout
    return out.splitlines()


def main():
    a = sys.argv[1:]
    if a and a[0] == "dump":
        renames = [tuple(x.split("=", 1)) for n, x in enumerate(a) if n and a[n - 1] == "--rename"]
        a = [x for n, x in enumerate(a) if x != "--rename" and a[n - 1] != "--rename"]
        csrc, out = os.path.abspath(a[1]), os.path.abspath(a[2])
        files = a[3:] or re.search(r"^SRCS := (.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
        with ThreadPoolExecutor(4) as ex:
            for r in ex.map(dump_one, [(csrc, out, fl, f, renames) for fl in ("build", "build_exp") for f in files]):
                print(r)
    elif a and a[0] == "cmp":
        A, B = a[1], a[2]
        rel = lambda top: sorted(os.path.relpath(os.path.join(d, f), top) for d, _, fs in os.walk(top) for f in fs if f.endswith(".s"))
        ra, rb = rel(A), rel(B)
        for r in sorted(set(ra) | set(rb)):
            if r not in rb or r not in ra:
                print("%s: only in %s" % (r, A if r in ra else B))
                continue
            ta, tb = open(os.path.join(A, r)).read().splitlines(), open(os.path.join(B, r)).read().splitlines()
            if ta == tb:
                print("%s: identical (%d instructions)" % (r, len(ta)))
                continue
            d = masked_diff(os.path.join(A, r), os.path.join(B, r), r)
            print("%s: DIFFERS (%d -> %d instructions; %d lines differ once registers and branch distances are masked)"
                  % (r, len(ta), len(tb), sum(1 for l in d if l[:1] in "+-" and l[:3] not in ("+++", "---"))))
            if "--diff" in a:
                print("\n".join(d))
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
