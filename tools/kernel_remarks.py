"""The resource table of a HIP source's kernels, from the compiler's -Rpass-analysis=kernel-resource-usage remarks.

  python tools/kernel_remarks.py hpr-lp-c_amd/csrc/batched.hip [--only PREFIX[,PREFIX...]] [--out FILE]

Compiles the device side only (gfx950, the Makefile's flags) and prints one line per kernel, sorted by name: SGPRs, VGPRs, AGPRs,
scratch bytes per lane, spills, occupancy, LDS bytes per workgroup.  No file name or line number is part of a line, so the tables
of two versions of a source can be compared with diff (DESIGN.md "Device-resident batches" records such a comparison).
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = (("SGPRs", "TotalSGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("scratch", "ScratchSize [bytes/lane]"), ("SGPR spills", "SGPRs Spill"),
        ("VGPR spills", "VGPRs Spill"), ("occupancy", "Occupancy [waves/SIMD]"), ("LDS", "LDS Size [bytes/block]"))


def remarks(source):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hpr-lp-c_amd", "csrc"),
               "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
               "-c", source, "-o", os.path.join(tmp, "device.o")]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.exit(p.stderr)
        return p.stderr


def table(text):
    rows, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: (.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            name = subprocess.run(["c++filt", t.split(":", 1)[1].strip()], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"^void ", "", name).replace("hprlp::(anonymous namespace)::", "").replace("hprlp::", "")
            cur = re.sub(r"\((?!.*<).*$", "", name) if "<" not in name else re.sub(r">\(.*$", ">", name)
            rows[cur] = {}
        elif cur and ":" in t:
            k, v = t.split(":", 1)
            rows[cur][k.strip()] = v.strip()
    return rows


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    only = tuple(argv[argv.index("--only") + 1].split(",")) if "--only" in argv else None
    rows = table(remarks(argv[1]))
    lines = ["%s | %s" % (name, " | ".join("%s %s" % (label, rows[name].get(key, "?")) for label, key in KEYS))
             for name in sorted(rows) if only is None or name.startswith(only)]
    print("\n".join(lines))
    if "--out" in argv:
        with open(argv[argv.index("--out") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv)
