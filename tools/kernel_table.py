"""Diagnostic: one sorted line per kernel of the kernel library, from the code objects.

    python tools/kernel_table.py                 # the working tree's csrc/
    python tools/kernel_table.py --rev HEAD~1    # a git revision's csrc/
    python tools/kernel_table.py --csrc DIR      # any other copy of the sources

Every kernel source is compiled for the device only, with the library's own flags
(gfedntm_amd/ops/srchash.py), and the fields are read from the code object's symbol table
(code size) and its metadata note (registers, spills, static LDS, scratch) -- nothing is
disassembled and no GPU is needed.  Two trees that print the same table have the same set
of kernel instances with the same resources:

    mangled name, code bytes, VGPRs, SGPRs, VGPR spills, SGPR spills, static LDS bytes, scratch bytes
"""
import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.build_native import ARCH, HIPCC, KERNEL_SRCS, KFLAGS  # noqa: E402

READELF = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), "llvm", "bin", "llvm-readelf")
FIELDS = ["vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
          "group_segment_fixed_size", "private_segment_fixed_size"]


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(" ".join(cmd) + "\n" + r.stderr[-3000:])
    return r.stdout


def _code_object(src, co):
    _run([HIPCC, f"--offload-arch={ARCH}"] + KFLAGS +
         ["--cuda-device-only", "--no-gpu-bundle-output", "-c", src, "-o", co])
    return co


def _kernels(co):
    """{name: [code bytes] + FIELDS} of one code object."""
    size = {}
    for ln in _run([READELF, "-s", "--wide", co]).splitlines():
        p = ln.split()     # Num: Value Size Type Bind Vis Ndx Name
        if len(p) == 8 and p[3] == "FUNC":
            size[p[7]] = int(p[2])
    out, cur = {}, None
    # the amdhsa.kernels list of the metadata note: an entry starts at "  - .key:" and its
    # own fields sit at four spaces (the .args entries are nested deeper)
    for ln in _run([READELF, "--notes", co]).splitlines():
        m = re.match(r"^  (- | {2})\.(\w+):\s*(.*)$", ln)
        if not m:
            if not ln.startswith("   "):
                cur = None
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is None:
            continue
        cur[m.group(2)] = m.group(3).strip("'\"")
        if "name" in cur and all(f in cur for f in FIELDS):
            out[cur["name"]] = [size[cur["name"]]] + [int(cur[f]) for f in FIELDS]
    return out


def table(csrc):
    srcs = [s for s in KERNEL_SRCS if s.endswith(".hip") and os.path.exists(os.path.join(csrc, s))]
    rows = {}
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(8) as ex:
        cos = ex.map(lambda s: _code_object(os.path.join(csrc, s), os.path.join(tmp, s + ".co")), srcs)
        for co in cos:
            rows.update(_kernels(co))
    return ["%s %s" % (k, " ".join(map(str, v))) for k, v in sorted(rows.items())]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--csrc", default=os.path.join(ROOT, "csrc"))
    ap.add_argument("--rev", help="take csrc/ from this git revision")
    a = ap.parse_args()
    if not a.rev:
        print("\n".join(table(a.csrc)))
        return
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "csrc"))
        for f in _run(["git", "-C", ROOT, "ls-tree", "--name-only", a.rev, "csrc/"]).split():
            data = subprocess.run(["git", "-C", ROOT, "show", f"{a.rev}:{f}"], capture_output=True,
                                  check=True).stdout
            with open(os.path.join(tmp, f), "wb") as fh:
                fh.write(data)
        print("\n".join(table(os.path.join(tmp, "csrc"))))


if __name__ == "__main__":
    main()
