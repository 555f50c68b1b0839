"""Register / LDS / occupancy table of the core step kernels, from the compiler's own report
(hipcc -Rpass-analysis=kernel-resource-usage, device code only: no GPU needed).

    python tools/kernel_resources.py [--csrc DIR] [--keep DIR] [--filter REGEX]

--csrc: the kernel sources to compile (default: this tree's ffm_amd/csrc; point it at another
checkout's to take the same table there).  One line per kernel instantiation: VGPRs, AGPRs,
SGPRs, scratch bytes per lane, LDS bytes per block (static), occupancy in waves per SIMD.
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FILES = ["core_group.hip", "core_multi.hip", "core_lane.hip", "core_step.hip"]
FIELDS = [("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occ")]


def parse(text: str) -> dict:
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass-analysis", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return r.stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        return list(names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "ffm_amd", "csrc"))
    ap.add_argument("--keep", default=None, help="directory for the raw compiler reports")
    ap.add_argument("--filter", default=r"core_(group|multi|lane|wave|block)_kernel")
    args = ap.parse_args()
    args.csrc = os.path.abspath(args.csrc)
    from ffm_amd import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = [f for f in B.FLAGS if f not in ("-shared",)]
    tmp = args.keep or tempfile.mkdtemp(prefix="ffm_res_")
    os.makedirs(tmp, exist_ok=True)

    def one(f):
        r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                            os.path.join(tmp, f + ".o"), os.path.join(args.csrc, f)],
                           capture_output=True, text=True, cwd=args.csrc)
        if r.returncode:
            sys.exit(r.stderr)
        open(os.path.join(tmp, f + ".txt"), "w").write(r.stderr)
        return parse(r.stderr)

    with ThreadPoolExecutor(max_workers=len(FILES)) as ex:
        tables = list(ex.map(one, FILES))
    print(f"{'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'scratch':>7} {'lds':>6} {'occ':>4}  kernel")
    for t in tables:
        names = [n for n in t]
        for n, d in zip(names, demangle(names)):
            if not re.search(args.filter, d):
                continue
            v = t[n]
            print(" ".join(f"{v.get(k, -1):>{w}}" for (k, _), w in zip(FIELDS, (5, 5, 5, 7, 6, 4))) + "  " +
                  d.replace("ffm::", "").replace("(CoreStepArgs)", "").replace("(CoreStepArgs, int)", "").replace("void ", ""))


if __name__ == "__main__":
    main()
