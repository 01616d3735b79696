"""The compiler's per-kernel resource figures of one HIP source, as a table: VGPRs, scratch bytes, static LDS, occupancy, SGPR / VGPR
spill counts and code bytes of every kernel (`.amdhsa_next_free_vgpr`, and `ScratchSize`, `LDSByteSize`, `Occupancy`, `codeLenInByte`
of the `; Kernel info` block, the spill counts of the metadata).  What a refactor of a kernel file has to hold.

  python scripts/kernel_figures.py planedepth_amd/csrc/pd_postprocess.hip [--json new.json] [--against parent.json]
  python scripts/kernel_figures.py some.s ...          (an assembly file that is already there)

A source is compiled with the library's flags for that file (__graft_entry__.BASE_FLAGS + FILE_FLAGS) and `--cuda-device-only -S`.
--against: the kernels that left or came, and every figure that moved; exit 1 if a kernel of both has more VGPRs, more scratch, more
static LDS or a lower occupancy than in the other file (SGPR spills and code bytes are listed, not gated)."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402

FIELDS = ["vgprs", "scratch", "lds", "occupancy", "sgpr_spills", "vgpr_spills", "code_bytes"]
GATED = {"vgprs": +1, "scratch": +1, "lds": +1, "occupancy": -1}     # the direction that costs


def assembly(src):
    out = os.path.join(tempfile.mkdtemp(prefix="kernel_figures."), os.path.basename(src) + ".s")
    cmd = [G.HIPCC] + G.BASE_FLAGS + G.FILE_FLAGS.get(os.path.basename(src), []) + \
          ["-I" + os.path.join(ROOT, "include"), "-I" + G.CSRC, "--cuda-device-only", "-S", "-o", out, src]
    print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            got = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, got))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def figures(path):
    """{mangled name: figures} of an assembly file."""
    text = open(path).read()
    kernels = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel(.*?); Occupancy: (\d+)", text, flags=re.S):
        name, desc, info = m.group(1), m.group(2), m.group(3)
        kernels[name] = dict(vgprs=int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)),
                             scratch=int(re.search(r"; ScratchSize: (\d+)", info).group(1)),
                             lds=int(re.search(r"; LDSByteSize: (\d+)", info).group(1)),
                             occupancy=int(m.group(4)),
                             code_bytes=int(re.search(r"; codeLenInByte = (\d+)", info).group(1)))
    for m in re.finditer(r"- \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target)", text, flags=re.S):
        name = re.search(r"\.name:\s+(\S+)", m.group(0)).group(1)
        for key in ("sgpr_spills", "vgpr_spills"):
            kernels[name][key] = int(re.search(r"\.%s_count:\s+(\d+)" % key[:-1], m.group(0)).group(1))
    pretty = demangle(sorted(kernels))
    return {n: dict(f, kernel=re.sub(r"^(void )?(pd::)?|\(.*\)$", "", pretty[n])) for n, f in kernels.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source", help="a .hip source (compiled here) or a .s file")
    ap.add_argument("--json", default="", help="write the figures there")
    ap.add_argument("--against", default="", help="figures of another tree (a --json file): what moved")
    a = ap.parse_args()
    new = figures(a.source if a.source.endswith(".s") else assembly(a.source))
    print("| Kernel | VGPRs | Scratch | LDS | Occupancy | SGPR spills | VGPR spills | Code bytes |\n|---|---|---|---|---|---|---|---|")
    for n in sorted(new, key=lambda n: new[n]["kernel"]):
        print("| `%s` | %s |" % (new[n]["kernel"], " | ".join(str(new[n][f]) for f in FIELDS)))
    print("%d kernels, %d code bytes" % (len(new), sum(f["code_bytes"] for f in new.values())))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(new, fh, indent=1, sort_keys=True)
    if not a.against:
        return 0
    old = json.load(open(a.against))
    worse = 0
    for n in sorted(set(old) - set(new)):
        print("left:  %s" % old[n]["kernel"])
    for n in sorted(set(new) - set(old)):
        print("came:  %s" % new[n]["kernel"])
    for n in sorted(set(new) & set(old), key=lambda n: new[n]["kernel"]):
        moved = ["%s %d -> %d" % (f, old[n][f], new[n][f]) for f in FIELDS if old[n][f] != new[n][f]]
        bad = [f for f, sign in GATED.items() if (new[n][f] - old[n][f]) * sign > 0]
        worse += bool(bad)
        if moved:
            print("moved: %s: %s%s" % (new[n]["kernel"], ", ".join(moved), "   WORSE: " + ", ".join(bad) if bad else ""))
    print("%d kernels of both, %d with more VGPRs, scratch or static LDS or a lower occupancy" % (len(set(new) & set(old)), worse))
    return 1 if worse else 0


sys.exit(main())
