#!/usr/bin/env python3
"""Is the device code of two builds of csrc the same?  (no GPU needed)

    python tools/device_code_diff.py BUILD_A BUILD_B        # two directories holding the *.o of `make -C csrc`

For every object file present in both directories the gfx950 code object is taken out of the host object (llvm-objcopy: the .hip_fatbin
section, clang-offload-bundler: its gfx950 entry) and compared kernel by kernel:
  * the kernel symbols on either side,
  * the sha256 of each kernel's function bytes (its FUNC symbol's range of .text),
  * its LDS size, VGPR / AGPR / SGPR counts and scratch size in the code object's metadata note.
It hashes and compares; it does not look at instructions.  One line per object, the differences below it; exit status 1 on any
difference, on an object that only the first build has, or when nothing was compared.

Build both trees AT THE SAME ABSOLUTE PATH, one after the other, with the same compiler (copy the first build's objects away, replace the
sources, `make` again): the compiler derives a per-file id from the path and the command line of a compilation (the __hip_cuid_ symbol;
in -fgpu-rdc builds it is also part of the names of kernels in an anonymous namespace), and a kernel's bytes may hold addresses relative
to other things in its file.  The id symbol itself is not compared."""
import hashlib, os, re, subprocess, sys, tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
RESOURCES = (".group_segment_fixed_size", ".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size")


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool)] + list(args), check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE).stdout.decode()


def code_object(obj, tmp):
    """The gfx950 code object of a host object file as a path, or None where the object carries no device code at all."""
    fb, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    for f in (fb, co):
        if os.path.exists(f):
            os.remove(f)
    if ".hip_fatbin" not in run("llvm-readelf", "-S", "-W", obj):
        return None
    run("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, obj)
    if TARGET not in run("clang-offload-bundler", "--list", "--type=o", "--input=" + fb).split():
        return None
    run("clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fb, "--output=" + co)
    return co if os.path.getsize(co) else None


def kernels(obj, tmp):
    """{kernel name: (sha256 of its bytes, {resource: value})} of one object file."""
    co = code_object(obj, tmp)
    if co is None:
        return {}
    text = None
    for line in run("llvm-readelf", "-S", "-W", co).split("\n"):
        m = re.match(r"\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            text = tuple(int(x, 16) for x in m.groups())          # address, file offset, size
    syms = {}
    for line in run("llvm-readelf", "--dyn-syms", "-W", co).split("\n"):
        f = line.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT"):
            syms[f[7]] = (int(f[1], 16), int(f[2]), f[3])
    names = sorted(n[:-3] for n, s in syms.items() if n.endswith(".kd") and s[2] == "OBJECT")          # a kernel = a kernel descriptor
    meta = {}
    for block in re.split(r"\n  - ", run("llvm-readelf", "--notes", co)):
        name = re.search(r"^\s*\.name:\s+(\S+)", block, re.M)
        if name:
            meta[name.group(1)] = {k: int(m.group(1)) for k in RESOURCES for m in [re.search(r"^\s*%s:\s+(\d+)" % re.escape(k), block, re.M)] if m}
    raw = open(co, "rb").read()
    out = {}
    for n in names:
        addr, size, kind = syms.get(n, (0, 0, None))
        assert kind == "FUNC" and text and text[0] <= addr and addr + size <= text[0] + text[2], "%s: kernel %s has no function in .text" % (obj, n)
        off = text[1] + addr - text[0]
        assert set(meta.get(n, {})) == set(RESOURCES), "%s: kernel %s has no complete metadata" % (obj, n)
        out[n] = (hashlib.sha256(raw[off:off + size]).hexdigest(), meta[n])
    return out


def main(argv):
    if len(argv) != 3 or not all(os.path.isdir(d) for d in argv[1:]):
        print(__doc__)
        return 2
    a, b = argv[1:]
    objs = [sorted(f for f in os.listdir(d) if f.endswith(".o")) for d in (a, b)]
    bad = compared = 0
    for f in sorted(set(objs[0]) - set(objs[1])):          # (an object the second build ADDS is listed below with its kernel count)
        print("%-28s only in %s" % (f, a))
        bad += 1
    with tempfile.TemporaryDirectory() as tmp:
        for f in objs[1]:
            kb = kernels(os.path.join(b, f), tmp)
            if f not in objs[0]:
                print("%-28s new: %d kernels" % (f, len(kb)))
                continue
            ka = kernels(os.path.join(a, f), tmp)
            diffs = ["kernel only in %s: %s" % (a if n in ka else b, n) for n in sorted(set(ka) ^ set(kb))]
            for n in sorted(set(ka) & set(kb)):
                if ka[n][0] != kb[n][0]:
                    diffs.append("bytes differ: %s" % n)
                diffs += ["%s %d -> %d: %s" % (k, ka[n][1][k], kb[n][1][k], n) for k in RESOURCES if ka[n][1][k] != kb[n][1][k]]
            compared += len(set(ka) & set(kb))
            print("%-28s %2d kernels  %s" % (f, len(kb), "DIFFERENT" if diffs else "same names, bytes and resources" if kb else "no kernel"))
            for d in diffs:
                print("    " + d)
            bad += len(diffs)
    print("%d kernels compared, %d differences" % (compared, bad))
    return 1 if bad or not compared else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
